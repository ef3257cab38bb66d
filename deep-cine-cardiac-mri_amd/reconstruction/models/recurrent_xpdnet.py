"""XPDNet_RNN on the MI355X kernels (drop-in for the reference's models/recurrent_xpdnet.py:14-240)."""
import torch
from torch import nn

from cine_hip import autograd as ag
from cine_hip import ops
from cine_hip.dc import Acquisition
from .denoisers.kspace_net import KSpaceCNN
from .recurrent_common import BCRNNlayer, CRNNBody, CRNNcell  # noqa: F401
from .xpdnet import BackwardOperator, ForwardOperator, SensitivityModel


class XPDNet_RNN(CRNNBody):
    def __init__(self, num_cascades: int = 12, sens_chans: int = 8, sens_pools: int = 4, chans: int = 18,
                 primal_only: bool = True, n_primal: int = 5, n_dual: int = 1):
        super().__init__()
        self.num_cascades, self.chans = num_cascades, chans
        self.i_buffer_mode, self.k_buffer_mode = True, not primal_only
        self.i_buffer_size, self.k_buffer_size = n_primal, 1 if primal_only else n_dual
        self.backward_op = BackwardOperator(masked=False)
        self.forward_op = ForwardOperator(masked=True)
        self.sens_net = SensitivityModel(sens_chans, sens_pools)
        self._make_body(2 * (n_primal + 1), chans, 2 * n_primal)
        if not primal_only:
            self.kspace_net = nn.ModuleList([KSpaceCNN(in_chans=2 * (n_dual + 2), out_chans=2 * n_dual, n_convs=3,
                                                       n_filters=16) for _ in range(num_cascades)])
        else:
            self.kspace_net = [self.measurements_residual for _ in range(num_cascades)]

    @staticmethod
    def measurements_residual(concat_kspace: torch.Tensor) -> torch.Tensor:
        return concat_kspace[..., [0, 2]] - concat_kspace[..., [1, 3]]

    def forward(self, ref_kspace: torch.Tensor, mask: torch.Tensor, acs=None, output: str = "magnitude") -> torch.Tensor:
        """``output="complex"``: the (b, t, h, w, 2) image in front of the final magnitude (``ops.complex_output``)."""
        cplx = ops.complex_output(output)
        mask = ops.as_mask_u8(mask, ref_kspace)          # any numeric 0 / 1 mask; broadcast along batch / time like the reference
        if ag.grad_mode(self):
            return self._forward_train(ref_kspace, mask, acs, cplx)
        with torch.no_grad():
            return self._forward_infer(ref_kspace, mask, acs, cplx)

    def _forward_train(self, ref_kspace, mask, acs, cplx=False):
        """The chain of ``_forward_infer`` as an autograd graph: sensitivity network, K step + masked backward operator (image space for the
        primal-only model; forward / k-space net / backward Functions with the dual buffer: cine_hip/dc.py), CRNN body on the buffer planes."""
        n = self.i_buffer_size
        b, t, _, h, w, _ = ref_kspace.shape
        if b != 1:
            raise NotImplementedError("training through the HIP path: batch 1")
        pick = lambda buf: torch.stack((buf[..., 0], buf[..., n]), dim=-1)
        acq = Acquisition(ref_kspace, mask, self.sens_net(ref_kspace, mask, acs), train=True)
        image_buffer = acq.image().repeat_interleave(n, dim=-1)                                            # (1, t, 1, h, w, 2n)
        kbuf = acq.k_buffer(self.k_buffer_size) if self.k_buffer_mode else None
        state = self.zero_state(t, b, h, w, image_buffer)
        for i in range(self.num_cascades):
            bwd, kbuf = acq.k_step(pick(image_buffer), kbuf, self.kspace_net[i])
            cat = torch.cat([image_buffer[..., :n], bwd[..., :1], image_buffer[..., n:], bwd[..., 1:]], dim=-1)
            planes = cat.view(t, h, w, 2 * (n + 1)).permute(0, 3, 1, 2).contiguous()                       # (t, 2(n+1), h, w)
            out, state = self.body_train(planes.view(t, 1, 2 * (n + 1), h, w), state, torch.cat([planes[:, :n], planes[:, n + 1:2 * n + 1]], dim=1))
            image_buffer = out.permute(0, 2, 3, 1).reshape(1, t, 1, h, w, 2 * n)
        image = pick(image_buffer).squeeze(2)
        return image if cplx else ag.AbsFn.apply(image)

    def _forward_infer(self, ref_kspace, mask, acs, cplx=False):
        n = self.i_buffer_size
        b, t, _, h, w, _ = ref_kspace.shape
        if b != 1:
            raise NotImplementedError("the CRNN models assume batch 1, like the reference")
        acq = Acquisition(ref_kspace, mask, self.sens_net(ref_kspace, mask, acs))
        image_buffer = ops.repeat_complex(acq.image(), n)                                  # (1, t, 1, h, w, 2n)
        state = self.zero_state(t, b, h, w, image_buffer)
        keep = self.__dict__.get("_keep_idx")                                              # channels [:n] and [n+1:-1], as a device index made
        if keep is None or keep.device != ref_kspace.device:                               # once (a list index is a host copy: not capturable)
            keep = self.__dict__["_keep_idx"] = torch.tensor([i for i in range(2 * (n + 1)) if i not in (n, 2 * n + 1)], device=ref_kspace.device)
        kbuf = acq.k_buffer(self.k_buffer_size) if self.k_buffer_mode else None            # dual buffer + KSpaceCNN
        for i in range(self.num_cascades):
            bwd, kbuf = acq.k_step(ops.extract_complex(image_buffer, 0, n), kbuf, self.kspace_net[i])      # (:110-163)
            cat = torch.cat([image_buffer[..., :n], bwd[..., :1], image_buffer[..., n:], bwd[..., 1:]], dim=-1)
            planes = ops.chanlast_to_planes(cat.view(t, h, w, 2 * (n + 1)))                 # (t, 2(n+1), h, w)
            out, state = self.body(planes.view(t, 1, 2 * (n + 1), h, w), state, planes.index_select(1, keep))
            image_buffer = ops.planes_to_chanlast(out, h, w).view(1, t, 1, h, w, 2 * n)
        image = ops.extract_complex(image_buffer, 0, n).squeeze(2)
        return image if cplx else ops.complex_abs(image)
