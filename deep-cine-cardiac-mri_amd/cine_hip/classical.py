"""Reconstruction without trained weights: k-t SPARSE-SENSE, low-rank plus sparse (L+S), spatio-temporal total variation (TV) and locally
low-rank (LLR), the compressed-sensing baselines on the package's own operators.

    minimise over x   1/2 || M A x - y ||^2  +  lam || w F_t x ||_1

with ``A x = fft2c(S_c x)``, ``M`` the sampling mask, ``F_t`` the centered ortho transform along the frames (``ops.fft1c`` variant 0) and
``w`` = 1, or 0 at the temporal DC bin with ``penalise_dc=False``.  FISTA (Beck & Teboulle 2009) from x_0 = z_0 = zf = A^H M y:

    g = A^H M A z_k - zf;   x_{k+1} = F_t^H soft(F_t (z_k - step g), step lam w);   z_{k+1} = x_{k+1} + beta_k (x_{k+1} - x_k)

One ``ops.kt_fista`` call runs all iterations: ``ops.image_dc`` and the fused proximal kernel (``ops.kt_prox``) per iteration, step and
threshold read from device memory, so nothing waits for the host and the solve can be captured into a graph.

``KtSparseSense`` is an ``nn.Module`` with CineNet's ``forward`` signature: it goes through ``SlicePipeline.submit`` / ``submit_raw``
(``sens_maps="espirit"``, ``coil_matrix=``) like a network.

Low-rank plus sparse (Otazo et al., MRM 2015): per batch element, over L and S,

    minimise   1/2 || M A (L + S) - y ||^2  +  lam_l || C(L) ||_*  +  lam_s || F_t S ||_1

with ``C(L)`` the (h w) x t Casorati matrix.  Proximal gradient without momentum from L_0 = zf, S_0 = 0:

    g = A^H M A (L_k + S_k) - zf;   L_{k+1} = SVT(L_k - step g, step lam_l);   S_{k+1} = F_t^H soft(F_t (S_k - step g), step lam_s)

The singular values are thresholded without an SVD: t <= 64, so the t x t Gram matrix of the Casorati matrix (``ops.casorati_gram``) is
diagonalised by a Jacobi eigensolver in one workgroup (``ops.svt_weight``) and its t x t weight is applied per pixel inside the fused
proximal kernel (``ops.ls_prox``).  One ``ops.ls_solve`` call runs all iterations with nothing read by the host.  ``LowRankPlusSparse`` is
the module, as ``KtSparseSense``.

Spatio-temporal total variation: per batch element, over x,

    minimise   1/2 || M A x - y ||^2  +  lam_t || D_t x ||_1  +  lam_s sum_pixels sqrt(|D_h x|^2 + |D_w x|^2)

with ``D_t`` the forward difference along the frames (wrapping from the last frame to the first with ``periodic``, 0 at the last frame
otherwise) and ``D_h``, ``D_w`` the forward differences along h and w (0 at the last row / column); the spatial term is isotropic.
Condat-Vu primal-dual (Condat 2013, Vu 2013) from x_0 = zf, p_0 = 0 with the dual p = (p_t, p_h, p_w):

    g = A^H M A x_k - zf;   x_{k+1} = x_k - tau (g + D^H p_k);   p_{k+1} = P(p_k + sigma D (2 x_{k+1} - x_k))

``P`` projects p_t onto the ball of radius lam_t and (p_h, p_w) jointly onto the ball of radius lam_s.  Everything after g is one launch
(``ops.tv_pd_step``: a spatial stencil with a recomputed one-pixel halo), one ``ops.tv_solve`` call runs all iterations with nothing read
by the host.  The objective is not monotone under this iteration.  ``TotalVariation`` is the module, as ``KtSparseSense``.

Locally low-rank (Trzasko & Manduca 2011; Zhang et al. 2015; the usual dynamic baseline of BART's ``pics``): per batch element, over x,

    minimise   1/2 || M A x - y ||^2  +  lam sum over the blocks beta of P of || C_beta(x) ||_*

with ``C_beta(x)`` the (pixels of beta) x t Casorati matrix of the spatial block beta and ``P`` a partition of the image into
``block`` x ``block`` squares whose grid origin lies at (-shift_h, -shift_w), clipped to the image (no wrap-around).  Proximal gradient
without momentum from x_0 = zf, the partition shifted from iteration to iteration ("cycle spinning", which removes the block seams):

    g = A^H M A x_k - zf;   x_{k+1} = BlockSVT_{P_k}(x_k - step g, step lam)

Every block has a t x t eigenproblem of its own, so the step, the Gram matrix, the Jacobi eigensolver, the thresholding and the
application are ONE launch with a workgroup per block (``ops.llr_prox``); one ``ops.llr_solve`` call runs all iterations with nothing read
by the host.  With a fixed partition this is ISTA and the objective never increases at the default step; with shifts the regulariser
changes per iteration and no such statement holds.  ``LocallyLowRank`` is the module, as ``KtSparseSense``.

Not built: CG-SENSE with a Tikhonov weight (``ops.conj_grad`` solves it for callers who want it), second-order (TGV) and anisotropic
spatial penalties, overlapping blocks, momentum and multi-scale low rank for LLR, and gradients through the solvers (they are not
differentiable).
"""
from typing import Optional, Union

import numpy as np
import torch
from torch import nn

from . import dc, ops
from ._lib import CineHipError

__all__ = ["fista_momentum", "kt_sparse_sense", "KtSparseSense", "low_rank_plus_sparse", "LowRankPlusSparse", "tv_peaks", "total_variation",
           "TotalVariation", "llr_shifts", "block_sigma_max", "locally_low_rank", "LocallyLowRank"]


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


def _iters(what: str, iters) -> int:
    if int(iters) < 1:
        raise ValueError(f"{what}: iters = {iters}")
    return int(iters)


def _no_grad_inputs(what: str, **tensors) -> None:
    for name, v in tensors.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise CineHipError(f"{what}: {name} requires grad, but the solver is not differentiable (it runs under torch.no_grad(), "
                               f"gradients through the iterations are not built); pass {name}.detach()")


def _device_float(value, device) -> torch.Tensor:
    """A float or a one-element device tensor as one device float."""
    return value if isinstance(value, torch.Tensor) else torch.full((1,), float(value), device=device, dtype=torch.float32)


def _setup(what: str, masked_kspace, mask, sens_maps, step, step_scale: Optional[float] = None):
    """What the four solvers do once their inputs passed ``_no_grad_inputs`` and their own settings are validated: refuse CPU tensors,
    then (acq, zf, mask_u8, step) with zf (b, t, 1, h, w, 2) the zero-filled image and ``step`` one device float --
    ``default_step(sens_maps)`` for None (times ``step_scale`` where one is given), a float or a one-element device tensor as given.
    Call it under ``torch.no_grad()``."""
    if not all(isinstance(v, torch.Tensor) and v.is_cuda for v in (masked_kspace, sens_maps, mask)):
        raise CineHipError(f"{what}: masked_kspace, mask and sens_maps must be GPU tensors (the HIP path has no CPU fallback)")
    mask = ops.as_mask_u8(mask, masked_kspace)
    acq = dc.Acquisition(masked_kspace, mask, sens_maps)
    zf = acq.zero_filled()
    if step is None:
        step = default_step(sens_maps)
        if step_scale is not None:
            step = step_scale * step
    return acq, zf, mask, _device_float(step, zf.device)


def _weight(value, peak_fn) -> torch.Tensor:
    """A regularisation weight as one device float: a one-element device tensor is absolute and used as given, a float is a fraction
    of the device peak ``peak_fn()``."""
    return value if isinstance(value, torch.Tensor) else peak_fn() * float(value)


def _finish(x: torch.Tensor, cplx: bool) -> torch.Tensor:
    """(b, t, 1, h, w, 2) -> (b, t, h, w, 2), or its magnitude (b, t, h, w)."""
    x = x.squeeze(2)
    return x if cplx else ops.complex_abs(x)


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
    _no_grad_inputs("kt_sparse_sense", masked_kspace=masked_kspace, sens_maps=sens_maps, lam=lam, step=step)
    with torch.no_grad():
        acq, zf, mask, step = _setup("kt_sparse_sense", masked_kspace, mask, sens_maps, step)      # ops.kt_fista refuses iters < 1
        lam = _weight(lam, lambda: temporal_peak(zf))
        out = ops.kt_fista(zf, sens_maps, mask, step, lam, iters, penalise_dc=penalise_dc, sens_tiled=acq.tiled, record=record)
        out = list(out) if record else [out]
        out[0] = _finish(out[0], cplx)
    return tuple(out) if record else out[0]


class _Solver(nn.Module):
    """One of the solvers above as a module with CineNet's ``forward`` signature and no parameters: ``SlicePipeline(KtSparseSense(...).eval())``
    reconstructs slices in flight, raw input and ``sens_maps="espirit"`` included.  The settings are the function's, kept as attributes and
    handed on by ``forward``; the default weights are untuned (see the function).  Not differentiable."""
    solve = None                     # the function

    def __init__(self, **settings):
        super().__init__()
        self._settings = tuple(settings)
        for name, v in settings.items():
            setattr(self, name, v)

    def forward(self, masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: torch.Tensor, output: str = "magnitude") -> torch.Tensor:
        return type(self).solve(masked_kspace, mask, sens_maps, output=output, **{name: getattr(self, name) for name in self._settings})


class KtSparseSense(_Solver):
    """``kt_sparse_sense`` as a module (see ``_Solver``); the default ``lam`` is untuned (see the function)."""
    solve = staticmethod(kt_sparse_sense)

    def __init__(self, iters: int = 30, lam: Union[float, torch.Tensor] = 0.02, step: Optional[Union[float, torch.Tensor]] = None,
                 penalise_dc: bool = True):
        super().__init__(iters=_iters("KtSparseSense", iters), lam=lam, step=step, penalise_dc=bool(penalise_dc))


def casorati_sigma_max(zf: torch.Tensor) -> torch.Tensor:
    """The largest singular value of the (h w) x t Casorati matrix of ``zf`` over the batch, one device float: the scale ``lam_l`` is a
    fraction of.  From ``ops.casorati_gram`` and ``ops.svt_weight``'s info; nothing is read by the host."""
    zero = torch.zeros(1, device=zf.device, dtype=torch.float32)
    _, info = ops.svt_weight(ops.casorati_gram(zf), zero)
    return info[:, 0].amax().to(torch.float32).reshape(1)


def low_rank_plus_sparse(masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: torch.Tensor, iters: int = 50,
                         lam_l: Union[float, torch.Tensor] = 0.01, lam_s: Union[float, torch.Tensor] = 0.01,
                         step: Optional[Union[float, torch.Tensor]] = None, output: str = "magnitude", components: bool = False,
                         record: bool = False):
    """L+S of ``masked_kspace`` (b, t, c, h, w, 2) with ``mask`` (any numeric 0 / 1 mask that broadcasts, as the models take) and
    ``sens_maps`` (b, 1, c, h, w, 2): ``iters`` proximal-gradient iterations from L = zf, S = 0; returns L + S.

    ``step``: None = ``0.5 * default_step(sens_maps)``: the data term's gradient in the joint variable (L, S) has Lipschitz constant
    2 ||A^H M A|| <= 2 max_pixel sum_c |S_c|^2, so with this step an iteration never increases the objective.  A float or a one-element
    device tensor is used as given; ``step=1.0`` with RSS-normalised maps is Otazo's published iteration and carries no such guarantee.
    ``lam_l``: a float is a FRACTION of the largest singular value of C(zf) (``casorati_sigma_max``, formed on the device); ``lam_s``: a
    float is a FRACTION of max |F_t zf| (``temporal_peak``); a one-element device tensor is the absolute weight.  The defaults 0.01 / 0.01
    are Otazo's cine settings, taken as a convenience; nobody has tuned them here -- choose them per protocol.
    ``output``: "magnitude" (b, t, h, w) or "complex" (b, t, h, w, 2).  ``components``: also return L and S, complex (b, t, h, w, 2).
    ``record``: also return rec (iters, 4) device floats -- sum |x_{k+1} - x_k|^2, sum |x_{k+1}|^2, sum |F_t S_{k+1}|, || C(L_{k+1}) ||_* per
    iteration -- and resid (iters,) float64, the residual the Jacobi eigensolver reached in each iteration.
    The order of the results: x, [L, S,] [rec, resid].  Nothing is read by the host, so the call can be captured into a graph.
    Not differentiable; raises ``CineHipError`` for CPU tensors (no fallback) and for an input that requires grad."""
    cplx = ops.complex_output(output)
    _no_grad_inputs("low_rank_plus_sparse", masked_kspace=masked_kspace, sens_maps=sens_maps, lam_l=lam_l, lam_s=lam_s, step=step)
    iters = _iters("low_rank_plus_sparse", iters)
    with torch.no_grad():
        acq, zf, mask, step = _setup("low_rank_plus_sparse", masked_kspace, mask, sens_maps, step, step_scale=0.5)
        lam_l = _weight(lam_l, lambda: casorati_sigma_max(zf))
        lam_s = _weight(lam_s, lambda: temporal_peak(zf))
        out = ops.ls_solve(zf, sens_maps, mask, step, lam_l, lam_s, iters, sens_tiled=acq.tiled, components=components, record=record)
        out = list(out) if isinstance(out, tuple) else [out]
        out[0] = _finish(out[0], cplx)
        if components:
            out[1], out[2] = out[1].squeeze(2), out[2].squeeze(2)
    return tuple(out) if len(out) > 1 else out[0]


class LowRankPlusSparse(_Solver):
    """``low_rank_plus_sparse`` as a module (see ``_Solver``); the default ``lam_l`` and ``lam_s`` are untuned (see the function)."""
    solve = staticmethod(low_rank_plus_sparse)

    def __init__(self, iters: int = 50, lam_l: Union[float, torch.Tensor] = 0.01, lam_s: Union[float, torch.Tensor] = 0.01,
                 step: Optional[Union[float, torch.Tensor]] = None):
        super().__init__(iters=_iters("LowRankPlusSparse", iters), lam_l=lam_l, lam_s=lam_s, step=step)


def tv_peaks(zf: torch.Tensor, periodic: bool = True):
    """(max |D_t zf|, max sqrt(|D_h zf|^2 + |D_w zf|^2)), one device float each: the scales ``lam_t`` and ``lam_s`` are fractions of.  zf:
    (b, t, [1,] h, w, 2).  Plain torch, once per solve; nothing is read by the host."""
    b, t, h, w = zf.shape[0], zf.shape[1], zf.shape[-3], zf.shape[-2]
    x = zf.reshape(b, t, h, w, 2)
    dt = x.roll(-1, dims=1) - x
    if not periodic:
        dt = dt[:, :-1]
    dh = torch.zeros_like(x)
    dw = torch.zeros_like(x)
    dh[:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    dw[:, :, :, :-1] = x[:, :, :, 1:] - x[:, :, :, :-1]
    peak_t = (dt * dt).sum(dim=-1).amax().sqrt().reshape(1)
    peak_s = ((dh * dh).sum(dim=-1) + (dw * dw).sum(dim=-1)).amax().sqrt().reshape(1)
    return peak_t, peak_s


def total_variation(masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: torch.Tensor, iters: int = 50,
                    lam_t: Union[float, torch.Tensor] = 0.02, lam_s: Union[float, torch.Tensor] = 0.01,
                    step: Optional[Union[float, torch.Tensor]] = None, sigma: Optional[Union[float, torch.Tensor]] = None,
                    periodic: bool = True, output: str = "magnitude", record: bool = False, dual: bool = False):
    """Spatio-temporal total variation of ``masked_kspace`` (b, t, c, h, w, 2) with ``mask`` (any numeric 0 / 1 mask that broadcasts, as the
    models take) and ``sens_maps`` (b, 1, c, h, w, 2): ``iters`` Condat-Vu iterations from x = zf, p = 0.

    ``lam_t`` / ``lam_s``: a float is a FRACTION of max |D_t zf| / max sqrt(|D_h zf|^2 + |D_w zf|^2) (``tv_peaks``, formed on the device);
    a one-element device tensor is the absolute weight; the float 0 switches the term off (its dual planes are then neither allocated nor
    touched); both off raises ``ValueError``.  The defaults 0.02 / 0.01 are a convenience that gives a sensible picture on the synthetic
    phantom; nobody has tuned them on real data -- choose them per protocol.
    ``step`` (tau): None = ``default_step(sens_maps)`` = 1 / max sum_c |S_c|^2 <= 1 / ||A^H M A||.  ``sigma``: None = 1 / (2 tau B) with
    B = 4 [temporal on] + 8 [spatial on] >= ||D||^2, which gives 1 / tau - sigma ||D||^2 >= ||A^H M A|| / 2, Condat's condition.  A float
    or a one-element device tensor is used as given.  The objective is not monotone under this iteration.
    ``periodic``: D_t wraps from the last frame to the first (a cine is one cardiac cycle); False: its last difference is 0.
    ``output``: "magnitude" (b, t, h, w) or "complex" (b, t, h, w, 2).  ``dual``: also return the final p (3, b, t, h, w, 2) = (p_t, p_h,
    p_w), zeros in the planes of a term that is off.  ``record``: also return rec (iters, 4) device floats -- sum |x_{k+1} - x_k|^2,
    sum |x_{k+1}|^2, sum |D_t x_{k+1}|, sum sqrt(|D_h x_{k+1}|^2 + |D_w x_{k+1}|^2) per iteration (0 for a term that is off).
    The order of the results: x, [p,] [rec].  Nothing is read by the host, so the call can be captured into a graph.
    Not differentiable; raises ``CineHipError`` for CPU tensors (no fallback) and for an input that requires grad."""
    cplx = ops.complex_output(output)
    _no_grad_inputs("total_variation", masked_kspace=masked_kspace, sens_maps=sens_maps, lam_t=lam_t, lam_s=lam_s, step=step, sigma=sigma)
    iters = _iters("total_variation", iters)
    terms =(0 if not isinstance(lam_t, torch.Tensor) and float(lam_t) == 0.0 else ops.TV_TEMPORAL) | \
            (0 if not isinstance(lam_s, torch.Tensor) and float(lam_s) == 0.0 else ops.TV_SPATIAL)
    if terms == 0:
        raise ValueError("total_variation: lam_t and lam_s are both 0, no term is left")
    with torch.no_grad():
        acq, zf, mask, step = _setup("total_variation", masked_kspace, mask, sens_maps, step)
        if sigma is None:
            bound = 4.0 * bool(terms & ops.TV_TEMPORAL) + 8.0 * bool(terms & ops.TV_SPATIAL)
            sigma = (step * (2.0 * bound)).reciprocal()
        sigma = _device_float(sigma, zf.device)
        if not (isinstance(lam_t, torch.Tensor) and isinstance(lam_s, torch.Tensor)):
            peak_t, peak_s = tv_peaks(zf, periodic)
            lam_t = _weight(lam_t, lambda: peak_t) if terms & ops.TV_TEMPORAL else None
            lam_s = _weight(lam_s, lambda: peak_s) if terms & ops.TV_SPATIAL else None
        out = ops.tv_solve(zf, sens_maps, mask, step, sigma, lam_t, lam_s, iters, terms=terms, periodic=periodic, sens_tiled=acq.tiled,
                           record=record, dual=dual)
        out = list(out) if isinstance(out, tuple) else [out]
        out[0] = _finish(out[0], cplx)
        if dual:
            out[1] = out[1].squeeze(3)
    return tuple(out) if len(out) > 1 else out[0]


class TotalVariation(_Solver):
    """``total_variation`` as a module (see ``_Solver``); the default ``lam_t`` and ``lam_s`` are untuned (see the function)."""
    solve = staticmethod(total_variation)

    def __init__(self, iters: int = 50, lam_t: Union[float, torch.Tensor] = 0.02, lam_s: Union[float, torch.Tensor] = 0.01,
                 step: Optional[Union[float, torch.Tensor]] = None, sigma: Optional[Union[float, torch.Tensor]] = None, periodic: bool = True):
        super().__init__(iters=_iters("TotalVariation", iters), lam_t=lam_t, lam_s=lam_s, step=step, sigma=sigma, periodic=bool(periodic))


def llr_shifts(iters: int, block: int, seed: int = 0) -> np.ndarray:
    """The partition shifts of ``locally_low_rank(shifts="random")``: (iters, 2) int32 = ``np.random.RandomState(seed).randint(0, block,
    size=(iters, 2))``, row k = (shift_h, shift_w) of iteration k.  This sequence is the contract: the float64 yardstick of the tests draws
    the same one."""
    return np.random.RandomState(int(seed)).randint(0, int(block), size=(int(iters), 2)).astype(np.int32)


def block_sigma_max(zf: torch.Tensor, block: int) -> torch.Tensor:
    """The largest singular value over all ``block`` x ``block`` blocks (shift (0, 0)) of ``zf`` (b, t, [1,] h, w, 2) and over the batch, one
    device float: the scale ``lam`` is a fraction of.  Formed on the device by ``ops.llr_prox`` with no image output; nothing is read by
    the host."""
    zero = torch.zeros(1, device=zf.device, dtype=torch.float32)
    _, info = ops.llr_prox(zf, None, None, zero, block, image=False)
    return info[0].to(torch.float32).reshape(1)


def _llr_settings(what: str, iters, block, shifts):
    """(iters, block, the (iters, 2) int32 host array or None) of ``locally_low_rank`` / ``LocallyLowRank``, validated on the host."""
    iters, block = _iters(what, iters), int(block)
    if not ops.LLR_MIN_BLOCK <= block <= ops.LLR_MAX_BLOCK:
        raise ValueError(f"{what}: block = {block} is outside {ops.LLR_MIN_BLOCK} .. {ops.LLR_MAX_BLOCK}")
    if shifts is None or (isinstance(shifts, str) and shifts == "fixed"):
        return iters, block, None
    if isinstance(shifts, str):
        if shifts != "random":
            raise ValueError(f'{what}: shifts = {shifts!r} is not "random", "fixed", None or an (iters, 2) integer array')
        return iters, block, llr_shifts(iters, block, 0)
    return iters, block, ops.llr_shift_array(shifts, iters, block, what)


def locally_low_rank(masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: torch.Tensor, iters: int = 30,
                     lam: Union[float, torch.Tensor] = 0.005, block: int = 8, shifts="random",
                     step: Optional[Union[float, torch.Tensor]] = None, output: str = "magnitude", record: bool = False):
    """Locally low-rank reconstruction of ``masked_kspace`` (b, t, c, h, w, 2) with ``mask`` (any numeric 0 / 1 mask that broadcasts, as the
    models take) and ``sens_maps`` (b, 1, c, h, w, 2): ``iters`` proximal-gradient iterations from x = zf.

    ``block``: the side of the square blocks, 2 .. 16 (no power of two needed).  ``shifts``: "random" = ``llr_shifts(iters, block, 0)``, a
    seeded partition shift per iteration; None or "fixed" = the unshifted partition in every iteration; an (iters, 2) integer array with
    entries in [0, block) is used as given (validated on the host, ``ValueError``).
    ``step``: None = ``default_step(sens_maps)`` <= 1 / ||A^H M A||; a float or a one-element device tensor is used as given.  With a fixed
    partition the iteration is ISTA and never increases the objective at that step; with shifts the regulariser changes from iteration to
    iteration and no such statement holds.
    ``lam``: a float is a FRACTION of ``block_sigma_max(zf, block)`` (formed on the device); a one-element device tensor is the absolute
    weight.  The default 0.005 is the best of a few values tried on the synthetic phantom; nobody has tuned it on real data -- choose it per
    protocol.
    ``output``: "magnitude" (b, t, h, w) or "complex" (b, t, h, w, 2).  ``record``: also return rec (iters, 4) device floats --
    sum |x_{k+1} - x_k|^2, sum |x_{k+1}|^2, sum over the blocks of || C_beta(x_{k+1}) ||_*, 0 per iteration -- and info (iters, 4) float64:
    the largest block sigma_max of the iteration's operand, the worst residual and the most sweeps of the Jacobi eigensolver, the number of
    blocks.  The order of the results: x, [rec, info].  Nothing is read by the host, so the call can be captured into a graph; a replayed
    graph replays the shift sequence it was captured with.
    Not differentiable; raises ``CineHipError`` for CPU tensors (no fallback) and for an input that requires grad."""
    cplx = ops.complex_output(output)
    _no_grad_inputs("locally_low_rank", masked_kspace=masked_kspace, sens_maps=sens_maps, lam=lam, step=step)
    iters, block, host_shifts = _llr_settings("locally_low_rank", iters, block, shifts)
    with torch.no_grad():
        acq, zf, mask, step = _setup("locally_low_rank", masked_kspace, mask, sens_maps, step)
        lam = _weight(lam, lambda: block_sigma_max(zf, block))
        out = ops.llr_solve(zf, sens_maps, mask, step, lam, block, iters, shifts=host_shifts, sens_tiled=acq.tiled, record=record)
        out = list(out) if record else [out]
        out[0] = _finish(out[0], cplx)
    return tuple(out) if record else out[0]


class LocallyLowRank(_Solver):
    """``locally_low_rank`` as a module (see ``_Solver``); a replayed graph replays the same shift sequence, which is intended.  The
    default ``lam`` is untuned (see the function)."""
    solve = staticmethod(locally_low_rank)

    def __init__(self, iters: int = 30, lam: Union[float, torch.Tensor] = 0.005, block: int = 8, shifts="random",
                 step: Optional[Union[float, torch.Tensor]] = None):
        iters, block, shifts = _llr_settings("LocallyLowRank", iters, block, shifts)
        super().__init__(iters=iters, lam=lam, block=block, shifts=shifts, step=step)
