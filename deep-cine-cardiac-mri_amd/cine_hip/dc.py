"""The data-consistency operators of one forward pass: which kernel sequence serves which mask layout, in one place.

``Acquisition(ref_kspace, mask, sens_maps, train)`` is built once at the top of a model's forward, from the mask that ``ops.as_mask_u8``
returned.  It decides there, once: the layout (row mask (b, t, 1, h, 1, 1), or general mask (b, t, 1, h, w, 1) that varies along w), whether
the image-space operator applies (``fused``: in inference always for a row mask, for a general one what ``ops.GENERAL_MASK_FUSED`` says at
that moment; in training only for a general mask with ``ops.GENERAL_MASK_FUSED`` and ``ops.GENERAL_MASK_FUSED_TRAIN`` both on -- a row mask
takes its autograd functions in the ``train`` branches), and whether the methods build an autograd graph (``train``).  What is constant over the cascades -- A^H M k_ref, the tile-packed maps, the
float mask of the literal chain -- is made on first use and kept.

  method                 row mask                       general mask, fused              general mask, literal           training (row / general)
  image()                kspace_to_hybrid, hybrid_reduce (= sens_reduce) in every inference form                          CoilReduceFn
  zero_filled()          masked kspace_to_hybrid,       apply_mask, sens_reduce          (not needed)                    CoilReduceFn with the mask / (not needed)
                         hybrid_reduce
  soft_dc()              image_dc, tiled maps           image_dc (both line passes)      sens_expand_dc, soft_dc_blend,  ImageDcFn / SensExpandFn, soft_dc_blend, SensReduceFn
                                                                                         sens_reduce
  residual_backward()    image_dc (1, 0, -1), tiled     image_dc (1, 0, -1)              ops.masked_residual_backward    ImageDcFixedFn / ag.masked_residual_backward
  forward_masked()       sens_expand_dc hard_mask       sens_expand_dc, apply_mask       sens_expand_dc, * mask + 0.0    SensExpandFn with the mask / SensExpandFn, * mask
  backward_masked()      * mask + 0.0, sens_reduce      apply_mask, sens_reduce          * mask + 0.0, sens_reduce       SensReduceFn with the mask / * mask, SensReduceFn

Training with a general mask and both switches on (``train and fused``) takes the row-mask column of the training forms: zero_filled() is
CoilReduceFn with the mask plane, soft_dc() ImageDcFn, residual_backward() ImageDcFixedFn (1, 0, -1) -- images saved for backward, no
coil-wise k-space.  forward_masked() / backward_masked() stay literal there: the dual net's k-space CNN needs the k-space itself.
"""
from typing import Optional

import torch

from . import autograd as ag
from . import ops


class Acquisition:
    def __init__(self, ref_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: torch.Tensor, train: bool = False):
        layout = ops.mask_layout(mask, ref_kspace)
        if layout is None:
            raise ValueError(f"mask {tuple(mask.shape)} is in neither layout for k-space {tuple(ref_kspace.shape)}: pass it through ops.as_mask_u8")
        self.kspace, self.mask, self.sens, self.train = ref_kspace, mask, sens_maps, train
        self.row = layout == "row"
        self.fused = ops.general_mask_fused_train(mask, ref_kspace) if train else (self.row or ops.GENERAL_MASK_FUSED)
        self._hyb = self._zf = self._tiled = self._mf = None

    @property
    def tiled(self) -> Optional[torch.Tensor]:
        """The maps as the row-mask DC kernel reads them fastest (``ops.sens_tile_pack``); None where no kernel reads them."""
        if self._tiled is None and self.row and not self.train:
            self._tiled = ops.sens_tile_pack(self.sens)
        return self._tiled

    @property
    def mask_float(self) -> torch.Tensor:
        if self._mf is None:
            self._mf = self.mask.to(self.kspace.dtype)
        return self._mf

    def image(self) -> torch.Tensor:
        """A^H k_ref, the first cascade's input (b, t, 1, h, w, 2).  In inference the two launches of ``ops.sens_reduce`` (cine_sens_reduce is
        cine_kspace_to_hybrid + cine_hybrid_reduce), with the hybrid-space buffer kept for ``zero_filled``."""
        if self.train:
            return ag.CoilReduceFn.apply(self.kspace, self.sens, None)
        self._hyb = ops.kspace_to_hybrid(self.kspace)
        return ops.hybrid_reduce(self._hyb, self.sens)

    def zero_filled(self) -> torch.Tensor:
        """A^H M k_ref: the constant term of the image-space operators."""
        if self._zf is None:
            hyb, self._hyb = self._hyb, None
            if self.train:
                self._zf = ag.CoilReduceFn.apply(self.kspace, self.sens, self.mask)
            elif self.row:
                self._zf = ops.hybrid_reduce(ops.kspace_to_hybrid(self.kspace, out=hyb, mask=self.mask), self.sens)
            else:
                del hyb
                self._zf = ops.sens_reduce(ops.apply_mask(self.kspace, self.mask), self.sens, destroy_input=True)
        return self._zf

    def soft_dc(self, img: torch.Tensor, lambda_reg: torch.Tensor, magnitude: bool = False) -> torch.Tensor:
        """reduce(DC(expand(img))): the soft data consistency of reference varnet.py:281-282 and the next cascade's sens_reduce."""
        if self.train:
            if self.row or self.fused:
                return ag.ImageDcFn.apply(img, self.sens, self.zero_filled(), self.mask, lambda_reg)
            k = ops.soft_dc_blend(ag.SensExpandFn.apply(img, self.sens, None), self.kspace, self.mask, lambda_reg)
            return ag.SensReduceFn.apply(k.contiguous(), self.sens, None)
        if self.fused:
            return ops.image_dc(img, self.sens, self.zero_filled(), self.mask, lambda_reg, magnitude=magnitude, sens_tiled=self.tiled)
        k = ops.soft_dc_blend(ops.sens_expand_dc(img, self.sens), self.kspace, self.mask, lambda_reg.detach())
        return ops.sens_reduce(k, self.sens, magnitude=magnitude, destroy_input=True)

    def residual_backward(self, x0: torch.Tensor) -> torch.Tensor:
        """A^H M (M A x0 - k_ref): XPDNet's K step and masked backward operator (reference xpdnet.py:128-131, 161-167) without the k-space."""
        if self.train:
            if self.row or self.fused:
                return ag.ImageDcFixedFn.apply(x0, self.sens, self.zero_filled(), self.mask, 1.0, 0.0, -1.0)
            return ag.masked_residual_backward(x0, self.sens, self.kspace, self.mask)
        if self.fused:
            return ops.image_dc(x0, self.sens, self.zero_filled(), self.mask, weights=(1.0, 0.0, -1.0), sens_tiled=self.tiled)
        return ops.masked_residual_backward(x0, self.sens, self.kspace, self.mask)

    def forward_masked(self, x0: torch.Tensor) -> torch.Tensor:
        """M A x0 as coil-wise k-space (b, t, c, h, w, 2): the masked forward operator (reference xpdnet.py:104-131)."""
        if self.train:
            return ag.SensExpandFn.apply(x0, self.sens, self.mask) if self.row else ag.SensExpandFn.apply(x0, self.sens, None) * self.mask_float
        if self.row:
            return ops.sens_expand_dc(x0, self.sens, None, self.mask, None, hard_mask=True)
        k = ops.sens_expand_dc(x0, self.sens)
        return ops.apply_mask(k, self.mask) if self.fused else k * self.mask + 0.0

    def backward_masked(self, k0: torch.Tensor) -> torch.Tensor:
        """A^H M k0: the masked backward operator (reference xpdnet.py:137-167).  ``k0`` is the caller's own tensor: it may be overwritten."""
        if self.train:
            if self.row:
                return ag.SensReduceFn.apply(k0.contiguous(), self.sens, self.mask)
            return ag.SensReduceFn.apply((k0 * self.mask_float).contiguous(), self.sens, None)
        k0 = ops.apply_mask(k0, self.mask, out=k0) if self.fused and not self.row else k0 * self.mask + 0.0
        return ops.sens_reduce(k0, self.sens)

    def k_buffer(self, n_dual: int) -> torch.Tensor:
        """The dual buffer's start value: k_ref repeated (reference xpdnet.py:306), channels [re x n_dual, im x n_dual]."""
        return self.kspace.repeat_interleave(n_dual, dim=-1) if self.train else ops.repeat_complex(self.kspace, n_dual)

    def k_step(self, x0: torch.Tensor, kbuf: Optional[torch.Tensor] = None, kspace_net=None):
        """The K step of XPDNet / XPDNet_RNN and the backward operator that follows it -> (backward image, new dual buffer).  Primal-only
        (``kbuf`` None): the measurement residual, in image space.  Dual buffer: the k-space net needs the whole k-space, so the masked
        forward operator materialises it (reference xpdnet.py:385-403) and the masked backward operator takes channel 0 of the net's output."""
        if kbuf is None:
            return self.residual_backward(x0), None
        nd, k, fwd = kbuf.shape[-1] // 2, self.kspace, self.forward_masked(x0)
        kbuf = kspace_net(torch.cat([kbuf[..., :nd], fwd[..., :1], k[..., :1], kbuf[..., nd:], fwd[..., 1:], k[..., 1:]], dim=-1))
        if self.train:
            return self.backward_masked(torch.stack((kbuf[..., 0], kbuf[..., nd]), dim=-1)), kbuf
        kbuf = kbuf.contiguous()
        return self.backward_masked(ops.extract_complex(kbuf, 0, nd)), kbuf
