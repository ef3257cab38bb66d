"""Reconstruction without trained weights: k-t SPARSE-SENSE, the compressed-sensing baseline on the package's own operators.

    minimise over x   1/2 || M A x - y ||^2  +  lam || w F_t x ||_1

with ``A x = fft2c(S_c x)``, ``M`` the sampling mask, ``F_t`` the centered ortho transform along the frames (``ops.fft1c`` variant 0) and
``w`` = 1, or 0 at the temporal DC bin with ``penalise_dc=False``.  FISTA (Beck & Teboulle 2009) from x_0 = z_0 = zf = A^H M y:

    g = A^H M A z_k - zf;   x_{k+1} = F_t^H soft(F_t (z_k - step g), step lam w);   z_{k+1} = x_{k+1} + beta_k (x_{k+1} - x_k)

One ``ops.kt_fista`` call runs all iterations: ``ops.image_dc`` and the fused proximal kernel (``ops.kt_prox``) per iteration, step and
threshold read from device memory, so nothing waits for the host and the solve can be captured into a graph.

``KtSparseSense`` is an ``nn.Module`` with CineNet's ``forward`` signature: it goes through ``SlicePipeline.submit`` / ``submit_raw``
(``sens_maps="espirit"``, ``coil_matrix=``) like a network.

Not built: CG-SENSE with a Tikhonov weight (``ops.conj_grad`` solves it for callers who want it), low-rank or total-variation regularisers,
and gradients through the solver (it is not differentiable).
"""
from typing import Optional, Union

import numpy as np
import torch
from torch import nn

from . import dc, ops
from ._lib import CineHipError

__all__ = ["fista_momentum", "kt_sparse_sense", "KtSparseSense"]


def fista_momentum(iters: int) -> np.ndarray:
    """beta_0 .. beta_{iters-1} as float32: s_0 = 1, s_{k+1} = (1 + sqrt(1 + 4 s_k^2)) / 2, beta_k = (s_k - 1) / s_{k+1}, the recurrence
    in double -- what cine_kt_fista computes on the host."""
    out = np.empty(int(iters), dtype=np.float32)
    s = 1.0
    for k in range(int(iters)):
        s1 = 0.5 * (1.0 + float(np.sqrt(1.0 + 4.0 * s * s)))
        out[k] = np.float32((s - 1.0) / s1)
        s = s1
    return out


def _no_grad_inputs(**tensors) -> None:
    for name, v in tensors.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise CineHipError(f"kt_sparse_sense: {name} requires grad, but the solver is not differentiable (it runs under torch.no_grad(), "
                               f"gradients through the iterations are not built); pass {name}.detach()")


def default_step(sens_maps: torch.Tensor) -> torch.Tensor:
    """1 / max over pixels of sum_c |S_c|^2, one device float.  A bound on 1 / ||A^H M A||: the transform is unitary and M a projection,
    so ||A^H M A|| <= ||S^H S|| = max_pixel sum_c |S_c|^2 (= 1 for RSS-normalised maps)."""
    return (sens_maps * sens_maps).sum(dim=(2, 5)).amax().reciprocal().reshape(1)


def temporal_peak(zf: torch.Tensor) -> torch.Tensor:
    """max |F_t zf|, one device float: the scale ``lam`` is a fraction of."""
    b, t = zf.shape[0], zf.shape[1]
    h, w = zf.shape[-3], zf.shape[-2]
    xf = ops.fft1c(zf.reshape(b, t, h * w, 2).permute(0, 2, 1, 3).contiguous())
    return (xf * xf).sum(dim=-1).amax().sqrt().reshape(1)


def kt_sparse_sense(masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: torch.Tensor, iters: int = 30,
                    lam: Union[float, torch.Tensor] = 0.02, step: Optional[Union[float, torch.Tensor]] = None, penalise_dc: bool = True,
                    output: str = "magnitude", record: bool = False):
    """k-t SPARSE-SENSE of ``masked_kspace`` (b, t, c, h, w, 2) with ``mask`` (any numeric 0 / 1 mask that broadcasts, as the models take)
    and ``sens_maps`` (b, 1, c, h, w, 2): ``iters`` FISTA iterations from the zero-filled image.

    ``step``: None = ``default_step(sens_maps)``; a float or a one-element device tensor is used as given.
    ``lam``: a float is a FRACTION of max |F_t zf| (formed on the device, one ``ops.fft1c`` per solve); a one-element device tensor is the
    absolute threshold weight.  The default 0.02 is a convenience that gives a sensible picture on the synthetic phantom; nobody has tuned it on
    real data -- choose it per protocol.
    ``output``: "magnitude" (b, t, h, w) or "complex" (b, t, h, w, 2) (``ops.complex_output``).  ``record``: also return the (iters, 4) device
    floats sum |x_{k+1} - x_k|^2, sum |x_{k+1}|^2, sum_f w_f |F_t x_{k+1}|, 0 per iteration.
    Not differentiable; raises ``CineHipError`` for CPU tensors (no fallback) and for an input that requires grad."""
    cplx = ops.complex_output(output)
    _no_grad_inputs(masked_kspace=masked_kspace, sens_maps=sens_maps, lam=lam, step=step)
    if not (isinstance(masked_kspace, torch.Tensor) and masked_kspace.is_cuda and isinstance(sens_maps, torch.Tensor) and sens_maps.is_cuda
            and isinstance(mask, torch.Tensor) and mask.is_cuda):
        raise CineHipError("kt_sparse_sense: masked_kspace, mask and sens_maps must be GPU tensors (the HIP path has no CPU fallback)")
    with torch.no_grad():
        mask = ops.as_mask_u8(mask, masked_kspace)
        acq = dc.Acquisition(masked_kspace, mask, sens_maps)
        zf = acq.zero_filled()                                       # (b, t, 1, h, w, 2)
        dev = zf.device
        if step is None:
            step = default_step(sens_maps)
        elif not isinstance(step, torch.Tensor):
            step = torch.full((1,), float(step), device=dev, dtype=torch.float32)
        if not isinstance(lam, torch.Tensor):
            lam = temporal_peak(zf) * float(lam)
        out = ops.kt_fista(zf, sens_maps, mask, step, lam, iters, penalise_dc=penalise_dc, sens_tiled=acq.tiled, record=record)
        x, rec = out if record else (out, None)
        x = x.squeeze(2)
        x = x if cplx else ops.complex_abs(x)
    return (x, rec) if record else x


class KtSparseSense(nn.Module):
    """``kt_sparse_sense`` as a module with CineNet's ``forward`` signature and no parameters: ``SlicePipeline(KtSparseSense(...).eval())``
    reconstructs slices in flight, raw input and ``sens_maps="espirit"`` included.  The settings are the function's; the default ``lam`` is
    untuned (see there).  Not differentiable."""

    def __init__(self, iters: int = 30, lam: Union[float, torch.Tensor] = 0.02, step: Optional[Union[float, torch.Tensor]] = None,
                 penalise_dc: bool = True):
        super().__init__()
        if int(iters) < 1:
            raise ValueError(f"KtSparseSense: iters = {iters}")
        self.iters, self.lam, self.step, self.penalise_dc = int(iters), lam, step, bool(penalise_dc)

    def forward(self, masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: torch.Tensor, output: str = "magnitude") -> torch.Tensor:
        return kt_sparse_sense(masked_kspace, mask, sens_maps, iters=self.iters, lam=self.lam, step=self.step, penalise_dc=self.penalise_dc,
                               output=output)
