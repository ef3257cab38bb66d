"""GRAPPA and TGRAPPA: the reconstruction a scanner runs for accelerated cine, as a baseline beside ``cine_hip.classical``.

Unlike the solvers there it is not iterative, works coil by coil in k-space, needs no sensitivity maps, and has one regularisation
number.  Every frame must sample a LATTICE: rows ``off + accel * j`` for one offset ``off`` per frame (plus, optionally, an ACS block or
stray extra rows, which are kept and never written).  For each missing row of type ``m = (y - off) mod accel`` a ``ky x kx`` kernel
predicts every coil from the ``ky`` nearest lattice rows of all coils (Griswold et al., MRM 47:1202, 2002):

    out[f, q, y, x] = sum_{j, dx, k} W[m - 1][(j, dx, k)][q] * in[f, k, y - m - base + j * accel, x + dx - kx // 2]

The kernels ``W`` are fitted by regularised least squares on a calibration array: the ACS block (``calib="acs"``), or -- TGRAPPA, Breuer
et al., MRM 53:981, 2005 -- the temporal average of an interleaved acquisition, which is fully sampled although no frame is
(``calib="tgrappa"``).  ``G = P^H P`` of the calibration patches is formed in float64 (``cine_grappa_gram``),
``(G_ss + lam * trace(G_ss) / ns * I) W = G_st`` is solved in float64 on the device (``cine_grappa_weights``) and the kernels are applied
on the fp32 matrix cores (``cine_grappa_apply``); the contract of all three is in ``include/cine_hip.h``.

The result is a filled multi-coil k-space: ``output="kspace"`` hands it out (an input for ``frontend.espirit_maps`` on a larger
calibration region, for VarNet's sensitivity network or for the self-supervised loss), ``"magnitude"`` is its root-sum-of-squares image or,
with ``sens_maps``, ``|sum_c conj(S_c) x_c|``.  ``Grappa`` is an ``nn.Module`` with the models' ``forward`` signature: nothing in it is read
by the host, it can be captured into a graph and goes through ``SlicePipeline.submit`` / ``submit_raw`` like a network, and
``cine_hip.noise.pseudo_replica`` gives its noise map.

The reference's ``EquispacedMaskFunc`` (``synth.EquispacedMaskFunc``) spaces its rows by a non-integer step and rounds: its masks are no
lattice.  ``lattice_mask`` makes masks that are.

Not built: irregular (variable-density) row masks, k-t GRAPPA with temporal source points, through-time calibration per frame,
image-domain application, and a g-factor from the weights (``noise.pseudo_replica`` measures one).
"""
import threading
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import CineHipError, check, lib

__all__ = ["lattice_mask", "plan_lattice", "calibration_data", "grappa_weights", "grappa_apply", "lattice_offsets", "grappa", "Grappa",
           "RESIDUAL_MAX"]

MAX_COILS, MAX_AUG = 32, 1152
RESIDUAL_MAX = 1e-8        # check=True: above this relative residual the float64 solve has diverged (a backward-stable one sits near 1e-15)


# ------------------------------------------------------------------ host logic
def lattice_mask(t: int, h: int, accel: int, acs: int = 0, interleave: bool = True) -> torch.Tensor:
    """A (1, t, 1, h, 1, 1) uint8 row mask: frame f acquires the rows ``(f mod accel if interleave else 0) + accel * j`` and the central
    ``acs`` rows ``[h // 2 - acs // 2, h // 2 - acs // 2 + acs)`` (the block of ``synth.RandomMaskFunc``)."""
    t, h, accel, acs = int(t), int(h), int(accel), int(acs)
    if t < 1 or h < 1 or accel < 1 or acs < 0 or acs > h:
        raise ValueError(f"lattice_mask: t = {t}, h = {h}, accel = {accel}, acs = {acs}")
    m = np.zeros((t, h), np.uint8)
    for f in range(t):
        m[f, (f % accel if interleave else 0)::accel] = 1
    if acs:
        lo = h // 2 - acs // 2
        m[:, lo:lo + acs] = 1
    return torch.from_numpy(m.reshape(1, t, 1, h, 1, 1))


def _host_rows(mask) -> np.ndarray:
    """A (t, h) or (b, t, 1, h, 1, 1) mask (torch or numpy, any numeric dtype) as a boolean numpy array of the same leading shape + (h,)."""
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    if m.ndim == 6 and m.shape[2] == 1 and m.shape[4] == 1 and m.shape[5] == 1:
        m = m.reshape(m.shape[0], m.shape[1], m.shape[3])
    elif m.ndim != 2:
        raise ValueError(f"mask {m.shape}: expected (t, h) or a row mask (b, t, 1, h, 1, 1)")
    return m != 0


def plan_lattice(mask, accel: int) -> np.ndarray:
    """The lattice offset of every frame of a (t, h) mask -> (t,) int32, or of a row mask (b, t, 1, h, 1, 1) -> (b, t): the lowest residue
    r in [0, accel) such that the rows r, r + accel, ... are all acquired (0 for a fully sampled frame).  Raises ``ValueError`` naming the
    first frame that has none.  The host twin of ``cine_grappa_offsets``."""
    accel = _accel(accel)
    m = _host_rows(mask)
    flat = m.reshape(-1, m.shape[-1])
    off = np.full(flat.shape[0], -1, np.int32)
    for f in range(flat.shape[0]):
        for r in range(accel):
            if flat[f, r::accel].all():
                off[f] = r
                break
        if off[f] < 0:
            where = f"frame {f}" if m.ndim == 2 else f"frame {f % m.shape[1]} of batch element {f // m.shape[1]}"
            raise ValueError(f"plan_lattice: {where} samples no lattice of step {accel}: for no offset r are the rows r, r + {accel}, ... all "
                             f"acquired (acquired rows: {np.flatnonzero(flat[f]).tolist()})")
    return off.reshape(m.shape[:-1])


def _accel(accel) -> int:
    if int(accel) != accel or not 2 <= int(accel) <= 8:
        raise ValueError(f"accel = {accel!r}: an integer 2 .. 8")
    return int(accel)


def _kernel(kernel) -> Tuple[int, int]:
    try:
        ky, kx = (int(v) for v in kernel)
    except (TypeError, ValueError):
        raise ValueError(f"kernel = {kernel!r}: expected (ky, kx)") from None
    if ky not in (2, 4) or kx not in (3, 5, 7):
        raise ValueError(f"kernel = {kernel!r}: ky in {{2, 4}} source rows and kx in {{3, 5, 7}} columns")
    return ky, kx


def _geometry(c: int, accel: int, ky: int, kx: int):
    """(ns, n_aug, span) within the limits of the kernels."""
    ns, n_aug = ky * kx * c, ky * kx * c + (accel - 1) * c
    if c < 1 or c > MAX_COILS or n_aug > MAX_AUG:
        raise ValueError(f"grappa: {c} coils with a {ky} x {kx} kernel at accel {accel}: at most {MAX_COILS} coils and "
                         f"ns + (accel - 1) * c = {n_aug} <= {MAX_AUG}")
    return ns, n_aug, (ky - 1) * accel + 1


def _lam(lam) -> float:
    lam = float(lam)
    if not (lam > 0.0 and np.isfinite(lam)):
        raise ValueError(f"lam = {lam!r}: must be positive and finite")
    return lam


def _calib_rows(h: int, calib: str, acs, calib_rows: int) -> Tuple[int, int]:
    """The rows [lo, hi) of the calibration block."""
    if calib not in ("auto", "acs", "tgrappa"):
        raise ValueError(f"calib = {calib!r}: 'auto', 'acs' or 'tgrappa'")
    if calib == "auto":
        calib = "acs" if acs is not None else "tgrappa"
    if calib == "acs":
        try:
            lo, hi = (int(v) for v in acs)
        except (TypeError, ValueError):
            raise ValueError(f"calib='acs' needs the rows acs=(lo, hi), got {acs!r}") from None
        if not 0 <= lo < hi <= h:
            raise ValueError(f"acs = {acs!r}: rows [lo, hi) within [0, {h})")
        return lo, hi
    n = min(int(calib_rows), h)
    if n < 1:
        raise ValueError(f"calib_rows = {calib_rows!r}")
    lo = h // 2 - n // 2
    return lo, lo + n


# ------------------------------------------------------------------ device steps
_WS = {}
_WS_LOCK = threading.Lock()


def _workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    """Scratch of the calibration entry points: one buffer per (device, stream), grown on demand; a captured graph gets a buffer of its
    own pool instead, static over replays."""
    nbytes = max(int(nbytes), 16)
    if ops._capturing():
        return torch.empty(nbytes, device=device, dtype=torch.uint8)
    key = (device.index, ops._stream())
    with _WS_LOCK:
        ws = _WS.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = _WS[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return ws


def release_workspaces() -> None:
    """Drop the cached scratch buffers."""
    with _WS_LOCK:
        _WS.clear()


def lattice_offsets(mask: torch.Tensor, accel: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """mask (b, t, 1, h, 1, 1) uint8 on the GPU -> (offsets (b, t) int32, status (b, t) int32) by ``cine_grappa_offsets``: the rule of
    ``plan_lattice``, with offset -1 and status 1 for a frame without a lattice.  No host read."""
    mask = ops._dev(mask, "mask", torch.uint8)
    b, t, h = mask.shape[0], mask.shape[1], mask.shape[3]
    if mask.numel() != b * t * h:
        raise ValueError(f"mask shape {tuple(mask.shape)}: expected a row mask (b, t, 1, h, 1, 1)")
    off = torch.empty((b, t), device=mask.device, dtype=torch.int32)
    status = torch.empty((b, t), device=mask.device, dtype=torch.int32)
    check(lib().cine_grappa_offsets(mask.data_ptr(), off.data_ptr(), status.data_ptr(), b * t, h, _accel(accel), ops._stream()),
          "cine_grappa_offsets")
    return off, status


def calibration_data(masked_kspace: torch.Tensor, mask: torch.Tensor, calib: str = "auto", acs: Optional[Sequence[int]] = None,
                     calib_rows: int = 32) -> torch.Tensor:
    """The calibration array (b, c, hc, w, 2) of masked k-space (b, t, c, h, w, 2) under the row mask (b, t, 1, h, 1, 1): per row the
    average over the frames that acquired it (rows nobody acquired stay zero), restricted to the central ``min(calib_rows, h)`` rows
    (``"tgrappa"``) or to the rows ``acs=(lo, hi)`` (``"acs"``); ``"auto"`` is ``"acs"`` when ``acs`` is given.  Plain torch ops on the
    tensors' device, nothing read by the host; whether every row of the block was acquired by some frame is the caller's to check
    (``grappa`` does, from the host copy of the mask)."""
    if masked_kspace.dim() != 6 or masked_kspace.shape[-1] != 2:
        raise ValueError(f"masked_kspace {tuple(masked_kspace.shape)}: expected (b, t, c, h, w, 2)")
    h = masked_kspace.shape[3]
    lo, hi = _calib_rows(h, calib, acs, calib_rows)
    m = (mask != 0)[:, :, :, lo:hi]                                  # (b, t, 1, hc, 1, 1)
    k = masked_kspace[:, :, :, lo:hi]
    total = torch.where(m, k, torch.zeros((), dtype=k.dtype, device=k.device)).sum(dim=1)
    count = m.to(k.dtype).sum(dim=1).clamp_(min=1.0)
    return (total / count).contiguous()


def grappa_weights(cal: torch.Tensor, accel: int, kernel=(2, 5), lam: float = 1e-4) -> Tuple[torch.Tensor, torch.Tensor]:
    """cal (c, hc, w, 2) float32 on the GPU -> (weights (accel - 1, ns, c, 2) float32, info (4,) float64): ``cine_grappa_gram`` and
    ``cine_grappa_weights``.  info: the relative residual of the float64 solve, tau, the calibration fit
    sqrt(trace(G_tt - W^H G_st) / trace(G_tt)), trace(G_ss).  No host read."""
    accel, (ky, kx), lam = _accel(accel), _kernel(kernel), _lam(lam)
    cal = ops._dev(cal, "grappa_weights cal")
    if cal.dim() != 4 or cal.shape[-1] != 2:
        raise ValueError(f"cal {tuple(cal.shape)}: expected (c, hc, w, 2)")
    c, hc, w, _ = cal.shape
    ns, n_aug, span = _geometry(c, accel, ky, kx)
    if hc < span or w < kx:
        raise ValueError(f"grappa_weights: the {hc} x {w} calibration array is smaller than the {span} x {kx} window of a {ky} x {kx} kernel "
                         f"at accel {accel}")
    dev = cal.device
    gram = torch.empty((n_aug, n_aug), device=dev, dtype=torch.complex128)
    weights = torch.empty((accel - 1, ns, c, 2), device=dev, dtype=torch.float32)
    info = torch.empty(4, device=dev, dtype=torch.float64)
    nb_gram = lib().cine_grappa_gram_ws_bytes(c, hc, w, accel, ky, kx)
    nb_solve = lib().cine_grappa_weights_ws_bytes(c, accel, ky, kx)
    ws = _workspace(max(nb_gram, nb_solve), dev)
    check(lib().cine_grappa_gram(cal.data_ptr(), gram.data_ptr(), ws.data_ptr(), nb_gram, c, hc, w, accel, ky, kx, ops._stream()),
          "cine_grappa_gram")
    check(lib().cine_grappa_weights(gram.data_ptr(), weights.data_ptr(), info.data_ptr(), ws.data_ptr(), nb_solve, c, accel, ky, kx, lam,
                                    ops._stream()), "cine_grappa_weights")
    return weights, info


def grappa_apply(kspace: torch.Tensor, weights: torch.Tensor, mask: torch.Tensor, offsets: torch.Tensor, accel: int, kernel=(2, 5),
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kspace (t, c, h, w, 2), weights (accel - 1, ns, c, 2), mask (t, h) uint8, offsets (t,) int32, all on the GPU -> the filled k-space
    (``cine_grappa_apply``).  ``out=kspace`` fills in place.  Rows that are acquired, and frames whose offset is -1, keep their bits."""
    accel, (ky, kx) = _accel(accel), _kernel(kernel)
    kspace = ops._dev(kspace, "grappa_apply kspace")
    weights = ops._dev(weights, "grappa_apply weights")
    mask = ops._dev(mask, "mask", torch.uint8)
    offsets = ops._dev(offsets, "offsets", torch.int32)
    t, c, h, w, _ = kspace.shape
    ns, _, _ = _geometry(c, accel, ky, kx)
    if tuple(weights.shape) != (accel - 1, ns, c, 2) or mask.numel() != t * h or offsets.numel() != t:
        raise ValueError(f"grappa_apply: weights {tuple(weights.shape)}, mask {tuple(mask.shape)}, offsets {tuple(offsets.shape)} for k-space "
                         f"{tuple(kspace.shape)}: expected {(accel - 1, ns, c, 2)}, {(t, h)}, {(t,)}")
    if out is None:
        out = torch.empty_like(kspace)
    elif out.shape != kspace.shape or out.dtype != kspace.dtype or not out.is_contiguous() or out.device != kspace.device:
        raise ValueError("grappa_apply: out must be a contiguous tensor like kspace")
    check(lib().cine_grappa_apply(kspace.data_ptr(), weights.data_ptr(), mask.data_ptr(), offsets.data_ptr(), out.data_ptr(), t, c, h, w,
                                  accel, ky, kx, ops._stream()), "cine_grappa_apply")
    return out


# ------------------------------------------------------------------ the reconstruction
def _settings(accel, kernel, lam, calib, acs, calib_rows, output, sens_maps):
    accel, (ky, kx), lam = _accel(accel), _kernel(kernel), _lam(lam)
    if calib not in ("auto", "acs", "tgrappa"):
        raise ValueError(f"calib = {calib!r}: 'auto', 'acs' or 'tgrappa'")
    if calib == "acs" and acs is None:
        raise ValueError("calib='acs' needs the rows acs=(lo, hi)")
    if output not in ("kspace", "magnitude", "complex"):
        raise ValueError(f"output={output!r}: expected 'kspace', 'magnitude' or 'complex'")
    if output == "complex" and sens_maps is None:
        raise ValueError("output='complex' needs sens_maps: without maps there is no coil-combined complex image (take output='kspace')")
    return accel, ky, kx, lam


def _run(masked_kspace, mask, sens_maps, accel, ky, kx, lam, calib, acs, calib_rows, output):
    """The launch sequence shared by ``grappa`` and ``Grappa.forward``: (result, info (b, 4), offsets (b, t), status (b, t))."""
    b, t, c, h, w, _ = masked_kspace.shape
    offsets, status = lattice_offsets(mask, accel)
    cal = calibration_data(masked_kspace, mask, calib, acs, calib_rows)
    filled = torch.empty_like(masked_kspace)
    infos = []
    for i in range(b):
        weights, info = grappa_weights(cal[i], accel, (ky, kx), lam)
        grappa_apply(masked_kspace[i], weights, mask[i].view(t, h), offsets[i], accel, (ky, kx), out=filled[i])
        infos.append(info)
    info = torch.stack(infos)
    if output == "kspace":
        res = filled
    elif sens_maps is None:
        res = ops.zero_filled_rss(filled, destroy_input=True)
    elif output == "magnitude":
        res = ops.sens_reduce(filled, sens_maps, magnitude=True, destroy_input=True)
    else:
        res = ops.sens_reduce(filled, sens_maps, destroy_input=True).squeeze(2)
    return res, info, offsets, status


def _inputs(what, masked_kspace, mask, sens_maps, accel, ky, kx, calib, acs, calib_rows):
    """Shapes against the limits (host only), then the tensors on the device: (masked_kspace, mask as uint8 row mask)."""
    if not isinstance(masked_kspace, torch.Tensor) or masked_kspace.dim() != 6 or masked_kspace.shape[-1] != 2:
        raise ValueError(f"{what}: masked_kspace must be a (b, t, c, h, w, 2) tensor")
    b, t, c, h, w, _ = masked_kspace.shape
    _, _, span = _geometry(c, accel, ky, kx)
    lo, hi = _calib_rows(h, calib, acs, calib_rows)
    if hi - lo < span or w < kx:
        raise ValueError(f"{what}: the calibration block of {hi - lo} rows x {w} columns is smaller than the {span} x {kx} window of a "
                         f"{ky} x {kx} kernel at accel {accel}")
    if not all(isinstance(v, torch.Tensor) and v.is_cuda for v in (masked_kspace, mask) + (() if sens_maps is None else (sens_maps,))):
        raise CineHipError(f"{what}: masked_kspace, mask and sens_maps must be GPU tensors (the HIP path has no CPU fallback)")
    mask = ops.as_mask_u8(mask, masked_kspace)
    if not ops.is_row_mask(mask, masked_kspace):
        raise ValueError(f"{what}: mask {tuple(mask.shape)} is no row mask (b, t, 1, h, 1, 1) for k-space {tuple(masked_kspace.shape)}")
    return ops._dev(masked_kspace, "masked_kspace"), mask, (lo, hi)


def grappa(masked_kspace: torch.Tensor, mask: torch.Tensor, accel: int, kernel=(2, 5), lam: float = 1e-4, calib: str = "auto",
           acs: Optional[Sequence[int]] = None, calib_rows: int = 32, sens_maps: Optional[torch.Tensor] = None, output: str = "magnitude",
           check: bool = True, record: bool = False):
    """GRAPPA / TGRAPPA of ``masked_kspace`` (b, t, c, h, w, 2) under the row mask ``mask`` (b, t, 1, h, 1, 1), every frame of which samples
    a lattice of step ``accel`` (2 .. 8).  Each batch element is calibrated on its own.

    ``kernel``: (ky, kx), ky in {2, 4} source rows and kx in {3, 5, 7} columns.  ``lam``: the Tikhonov weight as a fraction of the mean
    eigenvalue of the source Gram matrix; the condition number of the system is at most ns / lam.
    ``calib``: "tgrappa" calibrates on the central ``min(calib_rows, h)`` rows of the temporal average (per row, over the frames that
    acquired it), "acs" on its rows ``acs=(lo, hi)``, "auto" is "acs" when ``acs`` is given.
    ``output``: "kspace" (b, t, c, h, w, 2), the filled k-space; "magnitude" (b, t, h, w), its root-sum-of-squares image, or with
    ``sens_maps`` (b, 1, c, h, w, 2) ``|sum_c conj(S_c) x_c|``; "complex" (b, t, h, w, 2), the latter in front of the magnitude (needs maps).
    ``check``: read the solve's residual and raise ``CineHipError`` when it is not finite or above ``RESIDUAL_MAX`` (a NaN in the data, a
    diverged iteration; not a grade of accuracy).  ``record``: also return info (b, 4) float64 (``grappa_weights``) and offsets (b, t).
    Raises ``ValueError`` for settings and shapes outside the limits and for a frame without a lattice or a calibration row that no
    frame acquired, ``CineHipError`` for CPU tensors (no fallback) and inputs that require grad.  Not differentiable."""
    accel, ky, kx, lam = _settings(accel, kernel, lam, calib, acs, calib_rows, output, sens_maps)
    from .classical import _no_grad_inputs
    _no_grad_inputs("grappa", masked_kspace=masked_kspace, sens_maps=sens_maps)
    with torch.no_grad():
        masked_kspace, mask, (lo, hi) = _inputs("grappa", masked_kspace, mask, sens_maps, accel, ky, kx, calib, acs, calib_rows)
        rows = _host_rows(mask)                                      # (b, t, h): the mask on the host, to fail early
        plan_lattice(mask, accel)
        for i in range(rows.shape[0]):
            empty = np.flatnonzero(~rows[i, :, lo:hi].any(axis=0))
            if empty.size:
                raise ValueError(f"grappa: row {lo + int(empty[0])} of the calibration block [{lo}, {hi}) of batch element {i} was acquired by "
                                 f"no frame")
        res, info, offsets, _ = _run(masked_kspace, mask, sens_maps, accel, ky, kx, lam, calib, acs, calib_rows, output)
        if check:
            resid = info[:, 0].cpu().numpy()
            if not np.all(np.isfinite(resid)) or float(resid.max()) > RESIDUAL_MAX:
                raise CineHipError(f"grappa: the float64 solve of the kernels left the relative residuals {resid.tolist()} "
                                   f"(not finite, or above {RESIDUAL_MAX:g}): a NaN in the calibration data, or lam = {lam:g} too small")
    return (res, info, offsets) if record else res


class Grappa(nn.Module):
    """``grappa`` as a module with the models' ``forward`` signature and no parameters: ``SlicePipeline(Grappa(accel=4).eval())``
    reconstructs slices in flight, raw input included.  The lattice offsets come from ``cine_grappa_offsets`` and nothing is read by the
    host, so ``forward`` can be captured; there is no ``check`` -- frames without a lattice are left as they are and a failed solve shows
    in ``last_info``: the device tensors ``info`` (b, 4), ``offsets`` (b, t) and ``status`` (b, t) of the last call."""

    def __init__(self, accel: int, kernel=(2, 5), lam: float = 1e-4, calib: str = "auto", acs: Optional[Sequence[int]] = None,
                 calib_rows: int = 32):
        super().__init__()
        self.accel, self.ky, self.kx, self.lam = _settings(accel, kernel, lam, calib, acs, calib_rows, "magnitude", None)
        self.kernel = (self.ky, self.kx)
        self.calib, self.acs, self.calib_rows = calib, (None if acs is None else tuple(int(v) for v in acs)), int(calib_rows)
        self.last_info = None

    def forward(self, masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: Optional[torch.Tensor] = None,
                output: str = "magnitude") -> torch.Tensor:
        _settings(self.accel, self.kernel, self.lam, self.calib, self.acs, self.calib_rows, output, sens_maps)
        with torch.no_grad():
            masked_kspace, mask, _ = _inputs("Grappa", masked_kspace, mask, sens_maps, self.accel, self.ky, self.kx, self.calib, self.acs,
                                             self.calib_rows)
            res, info, offsets, status = _run(masked_kspace, mask, sens_maps, self.accel, self.ky, self.kx, self.lam, self.calib, self.acs,
                                              self.calib_rows, output)
        self.last_info = {"info": info, "offsets": offsets, "status": status}
        return res
