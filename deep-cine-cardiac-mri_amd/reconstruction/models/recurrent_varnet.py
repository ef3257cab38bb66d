"""VarNet_RNN on the MI355X kernels (drop-in for the reference's models/recurrent_varnet.py:13-150)."""
import math

import torch
from torch import nn

from cine_hip import autograd as ag
from cine_hip import ops
from cine_hip.dc import Acquisition
from .recurrent_common import BCRNNlayer, CRNNBody, CRNNcell  # noqa: F401  (re-exported like the reference)
from .varnet import SensitivityModel


class VarNet_RNN(CRNNBody):
    def __init__(self, num_cascades: int = 12, sens_chans: int = 8, sens_pools: int = 4, chans: int = 18):
        super().__init__()
        self.num_cascades, self.chans = num_cascades, chans
        self.sens_net = SensitivityModel(sens_chans, sens_pools)
        self._make_body(2, chans, 2)
        self.Softplus = nn.Softplus(1.)
        self.lambda_reg = nn.Parameter(torch.full((1,), math.log(math.e - 1.0)))

    def forward(self, ref_kspace: torch.Tensor, mask: torch.Tensor, acs=None, output: str = "magnitude") -> torch.Tensor:
        """``output="complex"``: the (b, t, h, w, 2) image in front of the final magnitude (``ops.complex_output``)."""
        cplx = ops.complex_output(output)
        mask = ops.as_mask_u8(mask, ref_kspace)          # any numeric 0 / 1 mask; broadcast along batch / time like the reference
        if ag.grad_mode(self):
            return self._forward_train(ref_kspace, mask, acs, cplx)
        with torch.no_grad():
            return self._forward_infer(ref_kspace, mask, acs, cplx)

    def _forward_train(self, ref_kspace, mask, acs, cplx=False):
        """The chain of ``_forward_infer`` (reference recurrent_varnet.py:92-150) as an autograd graph: sensitivity network, BCRNN +
        conv pairs through the HIP backward kernels (hidden states flow across time AND cascades), soft DC (cine_hip/dc.py)."""
        b, t, _, h, w, _ = ref_kspace.shape
        if b != 1:
            raise NotImplementedError("training through the HIP path: batch 1")
        acq = Acquisition(ref_kspace, mask, self.sens_net(ref_kspace, mask, acs), train=True)
        img = acq.image()                                                         # (1, t, 1, h, w, 2)
        state = self.zero_state(t, b, h, w, img)
        for _ in range(self.num_cascades):
            planes = img.view(t, h, w, 2).permute(0, 3, 1, 2).contiguous()        # (t, 2, h, w): frames are the conv batch
            out, state = self.body_train(planes.view(t, 1, 2, h, w), state, planes)
            img = acq.soft_dc(out.permute(0, 2, 3, 1).reshape(1, t, 1, h, w, 2), self.lambda_reg)
        return img.squeeze(2) if cplx else ag.AbsFn.apply(img.squeeze(2))

    def _forward_infer(self, ref_kspace, mask, acs, cplx=False):
        b, t, _, h, w, _ = ref_kspace.shape
        if b != 1:
            raise NotImplementedError("the CRNN models assume batch 1, like the reference (recurrent_varnet.py:110-113)")
        acq = Acquisition(ref_kspace, mask, self.sens_net(ref_kspace, mask, acs))
        img = acq.image()                                                         # (1, t, 1, h, w, 2)
        state = self.zero_state(t, b, h, w, img)
        for _ in range(self.num_cascades):
            planes, _ = ops.normunet_pack(img.view(t, h, w, 2), norm=False)      # (t, 2, h, w)
            out, state = self.body(planes.view(t, 1, 2, h, w), state, planes)
            img = acq.soft_dc(ops.normunet_unpack(out, None, h, w).view(1, t, 1, h, w, 2), self.lambda_reg)      # :80-90 + next reduce
        return img.squeeze(2) if cplx else ops.complex_abs(img.squeeze(2))
