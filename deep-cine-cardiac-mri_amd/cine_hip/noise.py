"""Noise propagation by the pseudo multiple replica method (Robson et al., MRM 60:895-907, 2008): synthetic noise of the scanner's
covariance is added to the measured k-space at the sampled points, the slice is reconstructed N times, and the per-pixel standard
deviation of the N results is the noise map -- for any reconstruction, the non-linear ones included, for which no closed form exists.

  noise_cholesky   Psi (``frontend.noise_covariance``) -> L with Psi = L L^H, what cine_noise_add colours its normals with
  add_noise        cine_noise_add: Philox4x32-10 keyed by (seed, replica, k-space point, coil) -- reproducible, independent of layout
                   and launch shape, one pass over the sampled points only; also the noise augmentation of a training loop
  ReplicaStats     Welford's running mean and variance over the replicas in float64 (cine_replica_accum / cine_replica_finish)
  pseudo_replica   the whole method, as a loop on the current stream or through a ``SlicePipeline`` (``submit(..., noise=)``)
  add_noise_raw    cine_noise_add_raw: the same values on RAW data (t, x, y, coil), where receiver noise enters -- in front of whitening,
                   coil compression, crop and filter, which colour it as they colour a scan's own
  pseudo_replica_raw  the method for a raw scan: noise, ``frontend.prepare_masked_slice``, model -- or ``submit_raw(..., noise=)``
  g_factor         std_accel / (std_full sqrt(R)) from two noise maps

The definition of the noise source is in include/cine_hip.h.  No CPU fallback.
"""
import collections
from typing import Optional

import torch

from . import ops
from ._lib import CineHipError, check, lib

__all__ = ["NOISE_MAX_COILS", "NoiseMaps", "NoiseSpec", "noise_cholesky", "add_noise", "add_noise_raw", "ReplicaStats", "pseudo_replica",
           "pseudo_replica_raw", "g_factor"]

NOISE_MAX_COILS = 64            # cine_noise_add, cine_noise_add_raw: L and the lane's normals share the LDS (include/cine_hip.h)

NoiseMaps = collections.namedtuple("NoiseMaps", "mean std snr g replicas")
NoiseSpec = collections.namedtuple("NoiseSpec", "chol scale seed replica", defaults=(None, 1.0, 0, 0))


def noise_cholesky(cov: Optional[torch.Tensor] = None, *, noise: Optional[torch.Tensor] = None, sigma: Optional[float] = None):
    """The factor ``add_noise`` colours its normals with: L (c, c) complex64 on the device, lower-triangular with a real positive diagonal,
    Psi = L L^H.  ``cov``: Psi (c, c) as ``frontend.noise_covariance`` returns it (GPU or CPU; a CPU matrix goes to the current GPU), or
    ``noise``: the noise samples (..., coil), Psi = ``frontend.noise_covariance(noise)``.  Computed in complex128 with
    torch.linalg.cholesky_ex, once per scan (it waits for the device).  ValueError when Psi is not finite, not Hermitian or not positive
    definite, as ``frontend.noise_whitener`` raises them.
    ``sigma=s``: white noise of standard deviation s per complex sample (E|eta|^2 = s^2); returns ``(None, s)``, the ``chol`` and
    ``scale`` of ``add_noise``."""
    from . import frontend
    if sum(v is not None for v in (cov, noise, sigma)) != 1:
        raise ValueError("noise_cholesky: pass cov, noise= or sigma=, one of the three")
    if sigma is not None:
        if not float(sigma) >= 0.0:
            raise ValueError(f"noise_cholesky: sigma = {sigma!r}")
        return None, float(sigma)
    if cov is None:
        psi = frontend.noise_covariance(noise)
    else:
        if not isinstance(cov, torch.Tensor) or cov.dim() != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 1:
            raise ValueError("noise_cholesky: cov must be a square matrix (coil, coil)")
        psi = cov.to(torch.complex128)
    c = psi.shape[0]
    short = ("the noise covariance is not positive definite: too few noise samples is the usual cause (fewer samples than coils give a "
             "rank-deficient matrix); pass more of the noise scan")
    if not bool(torch.isfinite(torch.view_as_real(psi)).all()):
        raise ValueError("noise_cholesky: the noise covariance is not finite (NaN or Inf in the noise samples)")
    if float((psi - psi.conj().transpose(0, 1)).abs().max()) > 1e-12 * float(psi.abs().max()):
        raise ValueError("noise_cholesky: the noise covariance is not Hermitian")
    low, info = torch.linalg.cholesky_ex(psi)
    if int(info) != 0:
        raise ValueError(f"noise_cholesky: {short}")
    d = low.diagonal().real                      # the pivot test of frontend.noise_whitener: a pivot of rounding size is zero
    if bool((d * d <= c * torch.finfo(torch.float64).eps * psi.diagonal().real).any()):
        raise ValueError(f"noise_cholesky: {short}")
    low = frontend._lower_real_diag(low).to(torch.complex64)
    if not low.is_cuda:
        if not torch.cuda.is_available():
            raise CineHipError("noise_cholesky: no GPU (the HIP path has no CPU fallback)")
        low = low.cuda()
    return low.contiguous()


def _chol_pairs(chol, c: int, device):
    """A given factor as (c, c, 2) float32 on `device`, or None."""
    if chol is None:
        return None
    if not isinstance(chol, torch.Tensor):
        raise TypeError("chol: expected a tensor (noise_cholesky) or None")
    pairs = torch.view_as_real(chol) if chol.is_complex() else chol
    if tuple(pairs.shape) != (c, c, 2) or pairs.dtype != torch.float32:
        raise ValueError(f"chol must be ({c}, {c}) complex64 for {c} coils (noise_cholesky), got {tuple(chol.shape)} {chol.dtype}")
    if not pairs.is_cuda or pairs.device != device:
        raise CineHipError(f"chol is on {pairs.device}, the k-space on {device}")
    return pairs if pairs.is_contiguous() else pairs.contiguous()


def _no_grad_inputs(what: str, **tensors) -> None:
    for name, v in tensors.items():
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise CineHipError(f"{what}: {name} requires grad, but the noise is not differentiable (no gradient is built); "
                               f"pass {name}.detach()")


def _noise_mask(mask, kspace):
    """The mask as the kernel reads it: (uint8 tensor or None, mask_w)."""
    if mask is None:
        return None, 1
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise CineHipError("add_noise: mask must be a GPU tensor or None (the HIP path has no CPU fallback)")
    mask = ops.as_mask_u8(mask, kspace)
    mask = mask if mask.is_contiguous() else mask.contiguous()
    c, h, w = kspace.shape[-4], kspace.shape[-3], kspace.shape[-2]
    bt = kspace.numel() // (c * h * w * 2)
    plane = w > 1 and mask.numel() == bt * h * w and mask.dim() >= 3 and tuple(mask.shape[-3:]) == (h, w, 1)
    if not plane and mask.numel() != bt * h:
        raise ValueError(f"add_noise: mask {tuple(mask.shape)} does not match k-space {tuple(kspace.shape)}")
    return mask, (w if plane else 1)


def add_noise(masked_kspace: torch.Tensor, mask: Optional[torch.Tensor], chol: Optional[torch.Tensor] = None, *, scale: float = 1.0,
              seed: int = 0, replica: int = 0, replica_dev: Optional[torch.Tensor] = None, point0: int = 0,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``masked_kspace + eta`` at the sampled points of ``mask``, the input's values elsewhere (cine_noise_add, one launch).

    ``masked_kspace``: (b, t, c, h, w, 2) or (t, c, h, w, 2) float32 on the GPU.  ``mask``: the layouts ``ops.apply_mask`` takes -- a row
    mask (..., 1, h, 1, 1) or one that varies along w, (..., 1, h, w, 1); for a 6-D k-space any numeric 0 / 1 mask that broadcasts, as the
    models take; None: every point.  ``chol``: L from ``noise_cholesky`` (E eta eta^H = scale^2 L L^H), or None: white, E|eta|^2 =
    scale^2.  ``seed``, ``replica``: the stream of normals; a value depends on (seed, replica, point, coil) only, where the point index
    is ``point0`` + the flat index over (b, t, h, w) -- a stack of frames equals its frames noised one by one with ``point0`` advanced
    by h * w each.  ``replica_dev``: a one-element int64 device tensor read by the kernel in place of ``replica`` -- capture the call
    and a counter bump in a graph, and every replay draws fresh noise.  ``out``: the result's place; ``out=masked_kspace`` works in
    place and touches the sampled points only.  At most 64 coils.  Not differentiable: an input that requires grad is refused."""
    _no_grad_inputs("add_noise", masked_kspace=masked_kspace, chol=chol)
    ops._pair(masked_kspace)
    k = ops._dev(masked_kspace, "k-space")
    if k.dim() not in (5, 6):
        raise ValueError(f"add_noise: k-space {tuple(k.shape)}; expected (b, t, c, h, w, 2) or (t, c, h, w, 2)")
    c, h, w = k.shape[-4], k.shape[-3], k.shape[-2]
    if c > NOISE_MAX_COILS:
        raise CineHipError(f"add_noise: {c} coils, at most {NOISE_MAX_COILS}")
    bt = k.numel() // (c * h * w * 2) if c * h * w else 0
    m, mask_w = _noise_mask(mask, k)
    low = _chol_pairs(chol, c, k.device)
    if out is None:
        out = torch.empty_like(k)
    elif out is masked_kspace:
        if k is not masked_kspace:
            raise CineHipError("add_noise: in place needs a contiguous k-space")
        out = k
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == k.shape):
        raise CineHipError("add_noise: out must be a contiguous float32 GPU tensor of the k-space's shape")
    if replica_dev is not None and not (isinstance(replica_dev, torch.Tensor) and replica_dev.is_cuda and replica_dev.dtype == torch.int64
                                        and replica_dev.numel() == 1):
        raise CineHipError("add_noise: replica_dev must be a one-element int64 GPU tensor")
    check(lib().cine_noise_add(k.data_ptr(), out.data_ptr(), ops._p(m), mask_w, ops._p(low), float(scale), _as_long(seed), int(replica),
                               ops._p(replica_dev), int(point0), bt, c, h, w, ops._stream()), "cine_noise_add")
    return out


def _raw_noise_mask(mask, t: int, nx: int, ny: int, device, what: str = "add_noise_raw"):
    """The mask of the raw samples as cine_noise_add_raw reads it: (contiguous uint8 (t, nx) or (t, nx, ny) or None, mask_ny)."""
    if mask is None:
        return None, 1
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise CineHipError(f"{what}: noise_mask must be a GPU tensor or None (the HIP path has no CPU fallback)")
    if mask.dtype not in (torch.uint8, torch.bool):
        raise CineHipError(f"{what}: noise_mask must be uint8 or bool, got {mask.dtype}")
    if mask.device != device:
        raise CineHipError(f"{what}: noise_mask is on {mask.device}, the raw data on {device}")
    shape = tuple(mask.shape)
    if not (mask.dim() in (2, 3) and shape[0] in (1, t) and shape[1:] in ((nx,), (nx, ny))):
        raise ValueError(f"{what}: noise_mask {shape}; expected ({t} | 1, {nx}) or ({t} | 1, {nx}, {ny}) for raw data (t, x, y) = "
                         f"({t}, {nx}, {ny})")
    m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    m = m.expand((t,) + shape[1:]).contiguous()
    return m, (ny if mask.dim() == 3 else 1)


def add_noise_raw(raw: torch.Tensor, chol: Optional[torch.Tensor] = None, *, noise_mask: Optional[torch.Tensor] = None,
                  scale: float = 1.0, seed: int = 0, replica: int = 0, replica_dev: Optional[torch.Tensor] = None, point0: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``raw + eta`` at the acquired samples of RAW k-space, in front of the front-end (cine_noise_add_raw, one launch): receiver noise
    where it enters, so that whitening, coil compression, crop, filter and calibration act on it as they act on a scan's own.

    ``raw``: (t, x, y, coil) complex64 or (t, x, y, coil, 2) float32 on the GPU, contiguous -- what ``frontend.prepare_masked_slice``
    and ``SlicePipeline.submit_raw`` take; the result has the input's form.  ``noise_mask``: which samples were acquired, uint8 or bool
    on the GPU, (T | 1, x) for whole lines or (T | 1, x, y); a leading 1 is expanded; None: every sample (fully sampled raw that is
    masked retrospectively).  ``chol``, ``scale``, ``seed``, ``replica``, ``replica_dev``: as in ``add_noise``; the point index is
    ``point0`` + the flat index over (t, x, y), and the value of a (point, coil) is the one ``add_noise`` gives the permuted data
    (t, coil, h = x, w = y), bit for bit.  ``out``: the result's place; ``out=raw`` works in place and touches the acquired samples
    only.  At most 64 coils.  Not differentiable: an input that requires grad is refused."""
    _no_grad_inputs("add_noise_raw", raw=raw, chol=chol)
    if not isinstance(raw, torch.Tensor):
        raise TypeError("add_noise_raw: expected a tensor")
    if raw.is_complex() and raw.dtype != torch.complex64:
        raise CineHipError(f"add_noise_raw: raw is {raw.dtype}; expected complex64 or float32 pairs")
    cplx = raw.is_complex()
    if cplx and not raw.is_contiguous():
        raise CineHipError("add_noise_raw: raw must be contiguous")
    x = torch.view_as_real(raw) if cplx else raw
    if x.dim() != 5 or x.shape[-1] != 2:
        raise ValueError(f"add_noise_raw: raw {tuple(raw.shape)}; expected (t, x, y, coil) complex64 or (t, x, y, coil, 2) float32")
    k = ops._dev(x, "raw")
    t, nx, ny, c = (int(v) for v in k.shape[:4])
    if c > NOISE_MAX_COILS:
        raise CineHipError(f"add_noise_raw: {c} coils, at most {NOISE_MAX_COILS}")
    m, mask_ny = _raw_noise_mask(noise_mask, t, nx, ny, k.device)
    low = _chol_pairs(chol, c, k.device)
    if out is None:
        res = torch.empty_like(k)
    elif out is raw:
        if k is not x:
            raise CineHipError("add_noise_raw: in place needs contiguous raw data")
        res = k
    else:
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == raw.dtype and out.is_contiguous() and out.shape == raw.shape):
            raise CineHipError("add_noise_raw: out must be a contiguous GPU tensor of the raw data's shape and dtype")
        res = torch.view_as_real(out) if cplx else out
    if replica_dev is not None and not (isinstance(replica_dev, torch.Tensor) and replica_dev.is_cuda and replica_dev.dtype == torch.int64
                                        and replica_dev.numel() == 1):
        raise CineHipError("add_noise_raw: replica_dev must be a one-element int64 GPU tensor")
    check(lib().cine_noise_add_raw(k.data_ptr(), res.data_ptr(), ops._p(m), mask_ny, ops._p(low), float(scale), _as_long(seed), int(replica),
                                   ops._p(replica_dev), int(point0), t, nx, ny, c, ops._stream()), "cine_noise_add_raw")
    if out is not None:
        return out
    return torch.view_as_complex(res) if cplx else res


def _as_long(seed: int) -> int:
    """Any Python integer as the C long of the same low 64 bits."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s - (1 << 64) if s >> 63 else s


class ReplicaStats:
    """Running mean and variance of the replicas, float64 on the device: ``add(x)`` takes the next sample (float32, ``shape``), Welford's
    update in one launch; ``finish`` returns the maps.  ``pairs``: the samples are complex (trailing pair) -- the variance is that of
    the complex value, var_re + var_im, the mean map is |mean|, and the maps drop the trailing axis."""

    def __init__(self, shape, device, pairs: bool = False):
        self.shape, self.device, self.pairs = tuple(int(v) for v in shape), torch.device(device), bool(pairs)
        if self.device.type != "cuda":
            raise CineHipError("ReplicaStats: the HIP path needs a GPU (no CPU fallback)")
        if self.pairs and (not self.shape or self.shape[-1] != 2):
            raise ValueError(f"ReplicaStats: pairs=True needs a trailing axis of 2, got {self.shape}")
        self.mean = torch.empty(self.shape, device=self.device, dtype=torch.float64)
        self.m2 = torch.empty(self.shape, device=self.device, dtype=torch.float64)
        if self.mean.numel() < 1:
            raise ValueError(f"ReplicaStats: empty shape {self.shape}")
        self.count = 0

    def add(self, x: torch.Tensor) -> None:
        _no_grad_inputs("ReplicaStats.add", x=x)
        x = ops._dev(x, "replica")
        if tuple(x.shape) != self.shape or x.device != self.device:
            raise CineHipError(f"ReplicaStats.add: sample {tuple(x.shape)} on {x.device}, expected {self.shape} on {self.device}")
        check(lib().cine_replica_accum(x.data_ptr(), self.mean.data_ptr(), self.m2.data_ptr(), x.numel(), self.count + 1, ops._stream()),
              "cine_replica_accum")
        self.count += 1

    def finish(self, ref_std: Optional[torch.Tensor] = None, accel: Optional[float] = None) -> NoiseMaps:
        """NoiseMaps(mean, std, snr, g, replicas) as float32 maps: std = sqrt(m2 / (N - 1)), snr = |mean| / std (0 where std is 0), and
        with ``ref_std`` (the std map of the fully sampled acquisition) and ``accel`` (R), g = std / (ref_std sqrt(R)) (0 where
        ref_std is 0); g is None without them.  At least two samples."""
        if self.count < 2:
            raise CineHipError(f"ReplicaStats.finish: {self.count} samples, at least 2")
        shape = self.shape[:-1] if self.pairs else self.shape
        if (ref_std is None) != (accel is None):
            raise ValueError("ReplicaStats.finish: ref_std and accel go together")
        if ref_std is not None:
            ref_std = ops._dev(ref_std, "ref_std")
            if tuple(ref_std.shape) != shape or ref_std.device != self.device:
                raise CineHipError(f"ReplicaStats.finish: ref_std {tuple(ref_std.shape)}, expected {shape} on {self.device}")
            if not float(accel) > 0.0:
                raise ValueError(f"ReplicaStats.finish: accel = {accel!r}")
        outs = [torch.empty(shape, device=self.device, dtype=torch.float32) for _ in range(4 if ref_std is not None else 3)]
        check(lib().cine_replica_finish(self.mean.data_ptr(), self.m2.data_ptr(), self.mean.numel(), self.count, int(self.pairs),
                                        ops._p(ref_std), 0.0 if accel is None else float(accel), outs[0].data_ptr(), outs[1].data_ptr(),
                                        outs[2].data_ptr(), outs[3].data_ptr() if ref_std is not None else None, ops._stream()),
              "cine_replica_finish")
        return NoiseMaps(outs[0], outs[1], outs[2], outs[3] if ref_std is not None else None, self.count)


def pseudo_replica(model, masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: Optional[torch.Tensor] = None, *,
                   chol: Optional[torch.Tensor] = None, scale: float = 1.0, replicas: int = 64, seed: int = 0, pipeline=None,
                   output: Optional[str] = None, **forward_kwargs) -> NoiseMaps:
    """The noise maps of ``model`` at this slice: replica r is ``model(add_noise(masked_kspace, mask, chol, scale=scale, seed=seed,
    replica=r), mask[, sens_maps])``, r = 0 .. replicas - 1, accumulated in that order.

    Without ``pipeline`` a loop on the current stream; ``output`` ("magnitude" / "complex") and ``forward_kwargs`` are handed to the
    model's forward, and "complex" results (trailing pair) are accumulated as complex values (``ReplicaStats(pairs=True)``).  With
    ``pipeline``, a ``SlicePipeline`` built on ``model`` with nothing pending, the replicas go through ``submit(..., noise=NoiseSpec)``
    and are accumulated as ``results()`` hands them out; the pipeline calls ``forward(mk, mask[, sens])`` only, so ``output`` and
    ``forward_kwargs`` must be left out.  The two ways give bit-identical maps.  ``sens_maps`` may be "espirit" with a pipeline.
    The mean map is the mean of the NOISY reconstructions; for magnitude outputs at low SNR it carries the Rician bias (not corrected)."""
    replicas = int(replicas)
    if replicas < 2:
        raise ValueError(f"pseudo_replica: replicas = {replicas}, at least 2")
    if output not in (None, "magnitude", "complex"):
        raise ValueError(f"pseudo_replica: output {output!r}")
    stats = None

    def take(o):
        nonlocal stats
        if not isinstance(o, torch.Tensor):
            raise CineHipError(f"pseudo_replica: the reconstruction returned {type(o).__name__}, not a tensor")
        if stats is None:
            stats = ReplicaStats(o.shape, o.device, pairs=output == "complex")
        stats.add(o)

    if pipeline is None:
        kw = dict(forward_kwargs)
        if output is not None:
            kw["output"] = output
        with torch.no_grad():
            for r in range(replicas):
                mk = add_noise(masked_kspace, mask, chol, scale=scale, seed=seed, replica=r)
                take(model(mk, mask, **kw) if sens_maps is None else model(mk, mask, sens_maps, **kw))
        return stats.finish()
    if pipeline.model is not model:
        raise CineHipError("pseudo_replica: the pipeline was built on another model")
    if output is not None or forward_kwargs:
        raise CineHipError("pseudo_replica: a pipeline calls forward(masked_kspace, mask[, sens_maps]) only; leave output= and the "
                           "forward keywords out, or run without pipeline=")
    if pipeline.zero_filled or pipeline.out != "device":
        raise CineHipError("pseudo_replica: the pipeline must hand out device tensors without the zero-filled image")
    if pipeline.pending():
        raise CineHipError(f"pseudo_replica: the pipeline has {pipeline.pending()} slices pending; take them first")
    for r in range(replicas):
        pipeline.submit(masked_kspace, mask, sens_maps, noise=NoiseSpec(chol, scale, seed, r))
        for _, o in pipeline.results():
            take(o)
    for _, o in pipeline.drain():
        take(o)
    return stats.finish()


def pseudo_replica_raw(model, raw: torch.Tensor, mask: torch.Tensor, sens_maps: Optional[torch.Tensor] = None, *,
                       chol: Optional[torch.Tensor] = None, scale: float = 1.0, replicas: int = 64, seed: int = 0,
                       noise_mask: Optional[torch.Tensor] = None, pipeline=None, output: Optional[str] = None, **front_end) -> NoiseMaps:
    """The noise maps of a RAW scan's slice through the front-end and ``model``: replica r is
    ``model(frontend.prepare_masked_slice(add_noise_raw(raw[:n], chol, noise_mask=noise_mask, scale=scale, seed=seed, replica=r), mask,
    **front_end), mask[, sens_maps])``, r = 0 .. replicas - 1, accumulated in that order; n = min(n_slices, t) kept frames.  The noise
    enters where a receiver's does, so whitening, coil compression (with ``virtual_coils=`` every replica's matrix is computed from its
    own noisy data), crop, filter and mask colour it as they colour the scan's own.  With ``chol`` from the scan's noise pre-scan
    (``noise_cholesky(noise=...)``) ``scale=1`` means "the scan's noise once more"; the front-end's ``scaling=`` is applied behind it.

    ``front_end``: the keywords of ``frontend.prepare_masked_slice`` / ``SlicePipeline.submit_raw`` (``crop_shape``, ``n_slices`` or
    ``n_frames``, ``filter_size``, ``scaling``, ``coil_matrix``, ``apply_mask``, ``virtual_coils``, ``cc_region``, ``whitener``).
    ``noise_mask``: see ``add_noise_raw``, on the kept frames; None for fully sampled raw masked retrospectively.  ``raw`` is moved to
    the device once (a host array handed to ``submit_raw`` would be copied again for every replica).  Without ``pipeline`` a loop on
    the current stream with ``output`` handed to the model; with ``pipeline`` the replicas go through ``submit_raw(..., noise=)`` under
    the rules of ``pseudo_replica`` (no ``output``, nothing pending, device results), and ``sens_maps`` may be "espirit": every replica
    then calibrates from its own noisy data.  The two ways give bit-identical maps."""
    from . import frontend
    replicas = int(replicas)
    if replicas < 2:
        raise ValueError(f"pseudo_replica_raw: replicas = {replicas}, at least 2")
    if output not in (None, "magnitude", "complex"):
        raise ValueError(f"pseudo_replica_raw: output {output!r}")
    fe = dict(front_end)
    if "n_frames" in fe and "n_slices" in fe:
        raise ValueError("pseudo_replica_raw: n_frames and n_slices name the same setting; pass one")
    n_keep = int(fe.pop("n_frames", fe.pop("n_slices", 15)))
    unknown = set(fe) - {"crop_shape", "filter_size", "scaling", "coil_matrix", "apply_mask", "virtual_coils", "cc_region", "whitener"}
    if unknown:
        raise TypeError(f"pseudo_replica_raw: unknown front-end keywords {sorted(unknown)}")
    if not torch.cuda.is_available():
        raise CineHipError("pseudo_replica_raw: no GPU (the HIP path has no CPU fallback)")
    dev = pipeline.device if pipeline is not None else torch.device("cuda", torch.cuda.current_device())
    if not isinstance(raw, torch.Tensor):
        raw = torch.from_numpy(raw)
    if raw.dim() < 4 or raw.shape[0] < 1 or n_keep < 1:
        raise ValueError("Invalid shapes.")
    kept = frontend._raw_pairs(raw[:min(n_keep, raw.shape[0])].to(dev), "pseudo_replica_raw")     # once: the replicas start from device memory
    stats = None

    def take(o):
        nonlocal stats
        if not isinstance(o, torch.Tensor):
            raise CineHipError(f"pseudo_replica_raw: the reconstruction returned {type(o).__name__}, not a tensor")
        if stats is None:
            stats = ReplicaStats(o.shape, o.device, pairs=output == "complex")
        stats.add(o)

    if pipeline is None:
        if isinstance(sens_maps, str):
            raise CineHipError('pseudo_replica_raw: sens_maps="espirit" is calibrated in flight: pass pipeline=')
        kw = {} if output is None else {"output": output}
        noisy = torch.empty_like(kept)
        with torch.no_grad():
            for r in range(replicas):
                add_noise_raw(kept, chol, noise_mask=noise_mask, scale=scale, seed=seed, replica=r, out=noisy)
                mk = frontend.prepare_masked_slice(noisy, mask, n_slices=n_keep, **fe)
                take(model(mk, mask, **kw) if sens_maps is None else model(mk, mask, sens_maps, **kw))
        return stats.finish()
    if pipeline.model is not model:
        raise CineHipError("pseudo_replica_raw: the pipeline was built on another model")
    if output is not None:
        raise CineHipError("pseudo_replica_raw: a pipeline calls forward(masked_kspace, mask[, sens_maps]) only; leave output= out, or "
                           "run without pipeline=")
    if pipeline.zero_filled or pipeline.out != "device":
        raise CineHipError("pseudo_replica_raw: the pipeline must hand out device tensors without the zero-filled image")
    if pipeline.pending():
        raise CineHipError(f"pseudo_replica_raw: the pipeline has {pipeline.pending()} slices pending; take them first")
    for r in range(replicas):
        pipeline.submit_raw(kept, mask, sens_maps, tag=("replica", r), n_frames=n_keep, noise=NoiseSpec(chol, scale, seed, r),
                            noise_mask=noise_mask, **fe)
        for _, o in pipeline.results():
            take(o)
    for _, o in pipeline.drain():
        take(o)
    return stats.finish()


def g_factor(std_accel: torch.Tensor, std_full: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """g = std_accel / (std_full sqrt(R)) per pixel, 0 where std_full is 0: the noise amplification of the accelerated reconstruction
    beyond the sqrt(R) of measuring less.  ``std_accel``, ``std_full``: the std maps of ``pseudo_replica`` with the scan's mask and with
    the full one; R = (points) / (sampled points) of ``mask`` (read by the host).  Runs cine_replica_finish on std_accel^2 as a
    two-sample sum of squares, which reproduces std_accel exactly."""
    if not isinstance(mask, torch.Tensor) or mask.numel() < 1:
        raise ValueError("g_factor: mask must be a non-empty tensor")
    n_on = int((mask != 0).sum())
    if n_on < 1:
        raise ValueError("g_factor: the mask samples nothing")
    a = ops._dev(std_accel, "std_accel")
    st = ReplicaStats(a.shape, a.device)
    st.mean.zero_()
    st.m2.copy_(a.double() ** 2)
    st.count = 2
    return st.finish(ref_std=std_full, accel=mask.numel() / n_on).g
