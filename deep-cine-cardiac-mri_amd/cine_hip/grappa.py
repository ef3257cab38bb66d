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
lattice.  ``lattice_mask`` makes masks that are; ``accel=None`` takes the others:

UNEVENLY SPACED ROWS (``accel=None``).  A frame is a list of gaps: two consecutive acquired rows ``G >= 2`` apart, filled from those two
rows (``ky = 2`` only) with the lattice kernels fitted for step ``G``; the rows in front of the first and behind the last acquired row are
ends, filled with the step ``max(neighbouring spacing, rows + 1)`` from one row and a zero row outside the frame.  ``plan_gaps`` states
the rule on the host, ``cine_grappa_gaps`` lists the gaps on the device, ``grappa_weights_gaps`` fits one set of kernels per step (one Gram
matrix and one solve each, through the lattice entry points) and ``cine_grappa_apply_gaps`` applies them.  On a pure lattice of step 2 .. 8
this gives the bits of the lattice path; next to an ACS block it predicts from the nearer rows.  Steps above 8 are out of reach: rows in
such a gap stay as they are and are counted (``unfilled``).  The reference's equispaced masks have steps {2 .. 6} at acceleration 4
(7 at 32 rows), {2, 3, 4} at 3, {2, 3} at 2, and 11 - 12 at acceleration 8, which is NOT supported.  Gaussian-density masks
(``synth.RandomMaskFunc``) are not what this is for either: at acceleration 4 some 61 % of their missing rows lie in gaps above 8; the
proximal baselines of ``cine_hip.classical`` (k-t SPARSE-SENSE, L+S, TV, LLR) are the tools for those.

ANALYTIC NOISE MAPS.  On a lattice the reconstruction is linear and shift-invariant, so its noise map has a closed form (Breuer et al.,
MRM 62:739, 2009): the ``accel - 1`` kernels are one convolution kernel, its transform is a ``c x c`` matrix ``Wimg`` per pixel
(``grappa_image_weights``), and a linear coil combination ``p`` has the noise variance ``p Wimg Psi Wimg^H p^H``.
``grappa_gfactor_from_weights`` gives g and the standard deviation from a set of weights in one launch of ``cine_grappa_gfactor``,
which never writes ``Wimg`` out; ``grappa_noise_maps`` and ``Grappa.noise_maps`` calibrate as ``grappa`` does and hand out the maps
for ``p = conj(S)`` or per coil.  The conventions are those of ``cine_hip.noise``: noise ``scale^2 Psi`` on every acquired sample
(``add_noise``), ``std`` the standard deviation of the complex pixel (``ReplicaStats(pairs=True)``), ``g = std_accel / (std_full
sqrt(R))`` (``noise.g_factor``); ``noise.pseudo_replica`` measures the same maps with ``2 x replicas`` reconstructions and a sampling
error of ``1 / sqrt(2 N)``.  What the closed form leaves out: the kernels treat rows and columns outside the frame as zero where the
formula wraps around (a little less noise near the edges, visible on small matrices); ACS rows are kept as acquired where the formula
knows the lattice only (the map is that of the lattice everywhere); ``h`` need not be a multiple of ``accel`` and the formula uses
``accel``; and the weights count as fixed -- the noise of a calibration that is refitted on every noisy replica is not in it.
Unevenly spaced rows (``accel=None``) are not shift-invariant and have no such map.

Not built: gaps above 8 rows (the equispaced masks at acceleration 8), ``ky = 4`` on uneven masks, masks that vary along w, a batched
Gram / solve over the steps (one pair per step runs in sequence), k-t GRAPPA with temporal source points, through-time calibration per
frame, image-domain application of the weights to the data, noise maps that know the ACS block or the zero boundary, and noise maps of
the gap path.
"""
import collections
import ctypes
import threading
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import CineHipError, check, lib

__all__ = ["lattice_mask", "plan_lattice", "calibration_data", "grappa_weights", "grappa_apply", "lattice_offsets", "grappa", "Grappa",
           "RESIDUAL_MAX", "plan_gaps", "gap_table", "grappa_weights_gaps", "grappa_apply_gaps", "MAX_GAP", "GfactorMaps",
           "grappa_image_weights", "grappa_gfactor_from_weights", "grappa_noise_maps"]

GfactorMaps = collections.namedtuple("GfactorMaps", "g std")

MAX_COILS, MAX_AUG = 32, 1152
MAX_GAP = 8                # the largest step a gap can have: the lattice kernels exist for 2 .. 8
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


def _max_gap(max_gap) -> int:
    if int(max_gap) != max_gap or not 2 <= int(max_gap) <= MAX_GAP:
        raise ValueError(f"max_gap = {max_gap!r}: an integer 2 .. {MAX_GAP}")
    return int(max_gap)


def _gap_sizes(gaps, max_gap: int) -> Tuple[int, ...]:
    """The steps with weights as a sorted tuple of distinct integers 2 .. max_gap."""
    try:
        given = list(gaps)
        sizes = sorted({int(g) for g in given})
        ok = bool(sizes) and len(sizes) == len(given) and all(int(g) == g for g in given) and sizes[0] >= 2 and sizes[-1] <= max_gap
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"gaps = {gaps!r}: expected distinct integers 2 .. {max_gap} (max_gap), at least one")
    return tuple(sizes)


def _plan_frame(row: np.ndarray, max_gap: int, allowed) -> Tuple[list, list]:
    """One frame (h,) bool -> ([(lo, G), ...] in ascending lo, the rows that stay unfilled)."""
    h = row.shape[0]
    a = np.flatnonzero(row).tolist()
    if not a:
        return [], list(range(h))
    n = len(a)
    cand = []                                                        # (lo, G, its target rows inside the frame)
    if a[0] > 0:
        nb = a[1] - a[0] if n >= 2 and a[1] - a[0] >= 2 else 0
        G = max(nb, a[0] + 1)
        cand.append((a[0] - G, G, list(range(0, a[0]))))
    for i in range(n - 1):
        G = a[i + 1] - a[i]
        if G >= 2:
            cand.append((a[i], G, list(range(a[i] + 1, a[i + 1]))))
    if a[-1] < h - 1:
        nb = a[-1] - a[-2] if n >= 2 and a[-1] - a[-2] >= 2 else 0
        G = max(nb, h - a[-1])
        cand.append((a[-1], G, list(range(a[-1] + 1, h))))
    gaps, unfilled = [], []
    for lo, G, rows in cand:
        if G <= max_gap and G in allowed:
            gaps.append((lo, G))
        else:
            unfilled.extend(rows)
    return gaps, unfilled


def plan_gaps(mask, max_gap: int = MAX_GAP, allowed=None):
    """The gaps of every frame of a (t, h) mask, or of a row mask (b, t, 1, h, 1, 1), by the rule of ``cine_grappa_gaps``
    (include/cine_hip.h), whose host twin this is.  Per frame, with a_0 < ... < a_{n-1} the acquired rows: consecutive rows G >= 2 apart
    are the gap (a_i, G); the e > 0 rows in front of a_0 are the gap (a_0 - G, G) with G = max(nb, e + 1), nb the spacing a_1 - a_0 if
    there is one and it is >= 2, else 0; the rows behind a_{n-1} likewise, (a_{n-1}, G).  A gap with G > max_gap or G not in ``allowed``
    (default: every step 2 .. max_gap) is left out and its rows count as unfilled; an empty frame has no gap and h unfilled rows.
    Returns (gaps, sizes, unfilled): the list per frame of (lo, G) in ascending lo (nested per batch element for a row mask), the sorted
    tuple of the steps that occur among them, and the unfilled rows per frame as int32 (t,) or (b, t)."""
    max_gap = _max_gap(max_gap)
    allowed = set(range(2, max_gap + 1)) if allowed is None else set(_gap_sizes(allowed, MAX_GAP))
    m = _host_rows(mask)
    flat = m.reshape(-1, m.shape[-1])
    per_frame = [_plan_frame(flat[f], max_gap, allowed) for f in range(flat.shape[0])]
    gaps = [g for g, _ in per_frame]
    sizes = tuple(sorted({G for g in gaps for _, G in g}))
    unfilled = np.array([len(u) for _, u in per_frame], np.int32).reshape(m.shape[:-1])
    if m.ndim == 3:
        t = m.shape[1]
        gaps = [gaps[i * t:(i + 1) * t] for i in range(m.shape[0])]
    return gaps, sizes, unfilled


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


def _fit(cal: torch.Tensor, accel: int, ky: int, kx: int, lam: float, weights: torch.Tensor, info: torch.Tensor) -> None:
    """``cine_grappa_gram`` and ``cine_grappa_weights`` of cal (c, hc, w, 2) into ``weights`` (accel - 1, ns, c, 2) and ``info`` (4,)."""
    c, hc, w, _ = cal.shape
    ns, n_aug, span = _geometry(c, accel, ky, kx)
    if hc < span or w < kx:
        raise ValueError(f"grappa_weights: the {hc} x {w} calibration array is smaller than the {span} x {kx} window of a {ky} x {kx} kernel "
                         f"at accel {accel}")
    gram = torch.empty((n_aug, n_aug), device=cal.device, dtype=torch.complex128)
    nb_gram = lib().cine_grappa_gram_ws_bytes(c, hc, w, accel, ky, kx)
    nb_solve = lib().cine_grappa_weights_ws_bytes(c, accel, ky, kx)
    ws = _workspace(max(nb_gram, nb_solve), cal.device)
    check(lib().cine_grappa_gram(cal.data_ptr(), gram.data_ptr(), ws.data_ptr(), nb_gram, c, hc, w, accel, ky, kx, ops._stream()),
          "cine_grappa_gram")
    check(lib().cine_grappa_weights(gram.data_ptr(), weights.data_ptr(), info.data_ptr(), ws.data_ptr(), nb_solve, c, accel, ky, kx, lam,
                                    ops._stream()), "cine_grappa_weights")


def grappa_weights(cal: torch.Tensor, accel: int, kernel=(2, 5), lam: float = 1e-4) -> Tuple[torch.Tensor, torch.Tensor]:
    """cal (c, hc, w, 2) float32 on the GPU -> (weights (accel - 1, ns, c, 2) float32, info (4,) float64): ``cine_grappa_gram`` and
    ``cine_grappa_weights``.  info: the relative residual of the float64 solve, tau, the calibration fit
    sqrt(trace(G_tt - W^H G_st) / trace(G_tt)), trace(G_ss).  No host read."""
    accel, (ky, kx), lam = _accel(accel), _kernel(kernel), _lam(lam)
    cal = ops._dev(cal, "grappa_weights cal")
    if cal.dim() != 4 or cal.shape[-1] != 2:
        raise ValueError(f"cal {tuple(cal.shape)}: expected (c, hc, w, 2)")
    c = cal.shape[0]
    ns, _, _ = _geometry(c, accel, ky, kx)
    weights = torch.empty((accel - 1, ns, c, 2), device=cal.device, dtype=torch.float32)
    info = torch.empty(4, device=cal.device, dtype=torch.float64)
    _fit(cal, accel, ky, kx, lam, weights, info)
    return weights, info


def _kernel_gaps(kernel) -> int:
    ky, kx = _kernel(kernel)
    if ky != 2:
        raise ValueError(f"kernel = {kernel!r}: on unevenly spaced rows (accel=None) only ky = 2 source rows, the two acquired neighbours of "
                         f"a gap; four need equal spacing on both sides")
    return kx


def _woff(gaps: Sequence[int], ns: int, c: int):
    """The 9 host ints of ``cine_grappa_apply_gaps``: the offset of the block of step G in complex elements, blocks in ascending G."""
    woff, row = [-1] * 9, 0
    for G in gaps:
        woff[G] = row * ns * c
        row += G - 1
    return (ctypes.c_int * 9)(*woff), row


def gap_table(mask: torch.Tensor, gaps: Sequence[int], max_gap: int = MAX_GAP) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """mask (b, t, 1, h, 1, 1) (or (t, h)) uint8 on the GPU -> (table (b, t, cap, 2) int32 of (lo, G), count (b, t), unfilled (b, t)) by
    ``cine_grappa_gaps``: the rule of ``plan_gaps`` with ``allowed = gaps``; entries from count on are (0, 0).  No host read."""
    max_gap = _max_gap(max_gap)
    sizes = _gap_sizes(gaps, max_gap)
    mask = ops._dev(mask, "mask", torch.uint8)
    if mask.dim() == 2:
        lead, h = (mask.shape[0],), mask.shape[1]
    elif mask.dim() == 6 and mask.numel() == mask.shape[0] * mask.shape[1] * mask.shape[3]:
        lead, h = (mask.shape[0], mask.shape[1]), mask.shape[3]
    else:
        raise ValueError(f"mask shape {tuple(mask.shape)}: expected (t, h) or a row mask (b, t, 1, h, 1, 1)")
    n = int(np.prod(lead))
    cap = lib().cine_grappa_gaps_cap(h)
    table = torch.empty(lead + (cap, 2), device=mask.device, dtype=torch.int32)
    count = torch.empty(lead, device=mask.device, dtype=torch.int32)
    unfilled = torch.empty(lead, device=mask.device, dtype=torch.int32)
    bits = sum(1 << g for g in sizes)
    check(lib().cine_grappa_gaps(mask.data_ptr(), table.data_ptr(), count.data_ptr(), unfilled.data_ptr(), n, h, max_gap, bits, ops._stream()),
          "cine_grappa_gaps")
    return table, count, unfilled


def grappa_weights_gaps(cal: torch.Tensor, gaps: Sequence[int], kernel=(2, 5), lam: float = 1e-4) -> Tuple[torch.Tensor, torch.Tensor]:
    """cal (c, hc, w, 2) float32 on the GPU -> (weights (sum of G - 1, ns, c, 2) float32, info (len(gaps), 4) float64): for every step G of
    ``gaps`` in ascending order the lattice fit ``grappa_weights(cal, G, (2, kx), lam)``, one Gram matrix and one solve each, written
    into consecutive slices of one buffer; row i of info is that fit's.  hc must be at least max(gaps) + 1.  No host read."""
    kx, lam = _kernel_gaps(kernel), _lam(lam)
    sizes = _gap_sizes(gaps, MAX_GAP)
    cal = ops._dev(cal, "grappa_weights_gaps cal")
    if cal.dim() != 4 or cal.shape[-1] != 2:
        raise ValueError(f"cal {tuple(cal.shape)}: expected (c, hc, w, 2)")
    c = cal.shape[0]
    ns, _, _ = _geometry(c, sizes[-1], 2, kx)
    weights = torch.empty((sum(G - 1 for G in sizes), ns, c, 2), device=cal.device, dtype=torch.float32)
    info = torch.empty((len(sizes), 4), device=cal.device, dtype=torch.float64)
    row = 0
    for i, G in enumerate(sizes):
        _fit(cal, G, 2, kx, lam, weights[row:row + G - 1], info[i])
        row += G - 1
    return weights, info


def grappa_apply_gaps(kspace: torch.Tensor, weights: torch.Tensor, gaps: Sequence[int], mask: torch.Tensor, table: torch.Tensor,
                      count: torch.Tensor, kernel=(2, 5), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kspace (t, c, h, w, 2), weights of ``grappa_weights_gaps(cal, gaps, kernel)``, mask (t, h) uint8, table (t, cap, 2) and count (t,)
    of ``gap_table``, all on the GPU -> the filled k-space (``cine_grappa_apply_gaps``).  ``out=kspace`` fills in place.  Acquired rows,
    rows of no listed gap and empty frames keep their bits."""
    kx = _kernel_gaps(kernel)
    sizes = _gap_sizes(gaps, MAX_GAP)
    kspace = ops._dev(kspace, "grappa_apply_gaps kspace")
    weights = ops._dev(weights, "grappa_apply_gaps weights")
    mask = ops._dev(mask, "mask", torch.uint8)
    table = ops._dev(table, "table", torch.int32)
    count = ops._dev(count, "count", torch.int32)
    t, c, h, w, _ = kspace.shape
    ns, _, _ = _geometry(c, sizes[-1], 2, kx)
    woff, rows = _woff(sizes, ns, c)
    cap = table.shape[-2] if table.dim() >= 2 else 0
    if (tuple(weights.shape) != (rows, ns, c, 2) or mask.numel() != t * h or count.numel() != t or cap < 1
            or table.numel() != t * cap * 2 or table.shape[-1] != 2):
        raise ValueError(f"grappa_apply_gaps: weights {tuple(weights.shape)}, mask {tuple(mask.shape)}, table {tuple(table.shape)}, count "
                         f"{tuple(count.shape)} for k-space {tuple(kspace.shape)} and gaps {sizes}: expected {(rows, ns, c, 2)}, {(t, h)}, "
                         f"(t, cap, 2), {(t,)}")
    if out is None:
        out = torch.empty_like(kspace)
    elif out.shape != kspace.shape or out.dtype != kspace.dtype or not out.is_contiguous() or out.device != kspace.device:
        raise ValueError("grappa_apply_gaps: out must be a contiguous tensor like kspace")
    check(lib().cine_grappa_apply_gaps(kspace.data_ptr(), weights.data_ptr(), woff, mask.data_ptr(), table.data_ptr(), count.data_ptr(),
                                       out.data_ptr(), t, c, h, w, cap, kx, ops._stream()), "cine_grappa_apply_gaps")
    return out


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


# ------------------------------------------------------------------ analytic noise maps
def _weights_for_maps(what, weights, accel, kernel, h, w):
    """(accel, ky, kx, c, h, w) with every shape checked, before anything asks for a device."""
    accel, (ky, kx) = _accel(accel), _kernel(kernel)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"{what}: h = {h}, w = {w}")
    if not isinstance(weights, torch.Tensor):
        raise TypeError(f"{what} weights: expected a tensor")
    if weights.dim() != 4 or weights.shape[-1] != 2 or weights.shape[0] != accel - 1 or weights.shape[2] < 1 \
            or weights.shape[1] != ky * kx * weights.shape[2]:
        raise ValueError(f"{what}: weights {tuple(weights.shape)}: expected ({accel - 1}, {ky} x {kx} x c, c, 2) for accel {accel} and a "
                         f"{ky} x {kx} kernel (grappa_weights)")
    c = weights.shape[2]
    _geometry(c, accel, ky, kx)
    return accel, ky, kx, c, h, w


def grappa_image_weights(weights: torch.Tensor, accel: int, kernel, h: int, w: int) -> torch.Tensor:
    """weights (accel - 1, ns, c, 2) of ``grappa_weights`` -> the image-domain weights (c, c, h, w, 2) of an h x w frame
    (``cine_grappa_image_weights``): ``out[q, k]`` is the map that coil image k contributes to coil image q,
    ``ifft2c(reconstruction)[q] = sum_k out[q, k] * ifft2c(zero-filled lattice)[k]`` up to the zero boundary of the k-space kernels.
    c^2 h w complex numbers (72 MB at 15 coils, 200 x 200): for a look at the weights or a check; the noise maps do not need it."""
    from .classical import _no_grad_inputs
    _no_grad_inputs("grappa_image_weights", weights=weights)
    accel, ky, kx, c, h, w = _weights_for_maps("grappa_image_weights", weights, accel, kernel, h, w)
    weights = ops._dev(weights, "grappa_image_weights weights")
    out = torch.empty((c, c, h, w, 2), device=weights.device, dtype=torch.float32)
    check(lib().cine_grappa_image_weights(weights.data_ptr(), out.data_ptr(), c, h, w, accel, ky, kx, ops._stream()),
          "cine_grappa_image_weights")
    return out


def grappa_gfactor_from_weights(weights: torch.Tensor, accel: int, kernel, h: int, w: int, chol: Optional[torch.Tensor] = None,
                                coef: Optional[torch.Tensor] = None, scale: float = 1.0) -> GfactorMaps:
    """The analytic noise maps of the lattice reconstruction with these weights on an h x w frame, ``GfactorMaps(g, std)``, one launch of
    ``cine_grappa_gfactor``; no host read.

    ``chol``: L (c, c) complex64 of ``noise.noise_cholesky`` (noise covariance ``scale^2 L L^H`` on every acquired sample, what
    ``noise.add_noise`` adds), None: white.  ``coef``: the coefficients p (n, c, h, w, 2) of the linear combination ``sum_q p_q x_q`` of
    the coil images whose noise is asked for -- ``conj(S)`` for the combination with sensitivity maps -- or None: every coil image on
    its own.  The maps are float32 (n, h, w) with ``coef`` and (c, h, w) without: ``std = scale * sqrt(p Wimg Psi Wimg^H p^H / accel)``,
    the standard deviation of the complex pixel, and ``g = std_accel / (std_full * sqrt(accel))``, 0 where ``p Psi p^H`` is 0.
    A root-sum-of-squares image is not linear in the data; to first order its noise is that of the combination with the image's own
    phase, ``coef = conj(x_q) / rss`` per pixel from the reconstructed coil images x_q (``x = ops.fft2c(filled[i, f], inverse=True)`` of one frame,
    ``coef = x * x.new_tensor([1.0, -1.0]) / (x ** 2).sum((0, -1)).sqrt()[None, ..., None]``), passed here with n = 1."""
    from .classical import _no_grad_inputs
    from .noise import _chol_pairs
    _no_grad_inputs("grappa_gfactor_from_weights", weights=weights, chol=chol, coef=coef)
    accel, ky, kx, c, h, w = _weights_for_maps("grappa_gfactor_from_weights", weights, accel, kernel, h, w)
    low = _chol_pairs(chol, c, weights.device)                       # its type and shape first, then where it is
    weights = ops._dev(weights, "grappa_gfactor_from_weights weights")
    n = c
    if coef is not None:
        coef = ops._dev(coef, "grappa_gfactor_from_weights coef")
        if coef.dim() != 5 or tuple(coef.shape[1:]) != (c, h, w, 2) or coef.shape[0] < 1:
            raise ValueError(f"grappa_gfactor_from_weights: coef {tuple(coef.shape)}: expected (n, {c}, {h}, {w}, 2)")
        if coef.device != weights.device:
            raise CineHipError(f"grappa_gfactor_from_weights: coef is on {coef.device}, the weights on {weights.device}")
        n = coef.shape[0]
    g = torch.empty((n, h, w), device=weights.device, dtype=torch.float32)
    amp = torch.empty((n, h, w), device=weights.device, dtype=torch.float32)
    check(lib().cine_grappa_gfactor(weights.data_ptr(), ops._p(low), ops._p(coef), g.data_ptr(), amp.data_ptr(), n if coef is not None else 1,
                                    c, h, w, accel, ky, kx, ops._stream()), "cine_grappa_gfactor")
    return GfactorMaps(g, amp.mul_(float(scale) / float(np.sqrt(accel))))


def _run_noise_maps(masked_kspace, mask, sens_maps, chol, scale, accel, ky, kx, lam, calib, acs, calib_rows):
    """The launch sequence shared by ``grappa_noise_maps`` and ``Grappa.noise_maps``: (GfactorMaps, info (b, 4))."""
    b, t, c, h, w, _ = masked_kspace.shape
    cal = calibration_data(masked_kspace, mask, calib, acs, calib_rows)
    coef = None
    if sens_maps is not None:
        sens_maps = ops._dev(sens_maps, "sens_maps")
        if tuple(sens_maps.shape) != (b, 1, c, h, w, 2):
            raise ValueError(f"sens_maps shape {tuple(sens_maps.shape)} does not match k-space {tuple(masked_kspace.shape)}")
        coef = sens_maps.clone()                                     # p = conj(S), (b, 1, c, h, w, 2); no host data: capturable
        coef[..., 1].neg_()
    gs, stds, infos = [], [], []
    for i in range(b):
        weights, info = grappa_weights(cal[i], accel, (ky, kx), lam)
        maps = grappa_gfactor_from_weights(weights, accel, (ky, kx), h, w, chol, None if coef is None else coef[i], scale)
        gs.append(maps.g if coef is None else maps.g[0])
        stds.append(maps.std if coef is None else maps.std[0])
        infos.append(info)
    return GfactorMaps(torch.stack(gs), torch.stack(stds)), torch.stack(infos)


def grappa_noise_maps(masked_kspace: torch.Tensor, mask: torch.Tensor, accel: int, kernel=(2, 5), lam: float = 1e-4, calib: str = "auto",
                      acs: Optional[Sequence[int]] = None, calib_rows: int = 32, sens_maps: Optional[torch.Tensor] = None,
                      chol: Optional[torch.Tensor] = None, scale: float = 1.0, check: bool = True):
    """The analytic noise maps of ``grappa(masked_kspace, mask, accel, ...)``: ``(GfactorMaps(g, std), info)``.  The kernels are fitted
    exactly as ``grappa`` fits them (the same checks, calibration data and ``grappa_weights``, per batch element), then
    ``grappa_gfactor_from_weights`` turns each set into maps: (b, h, w) for the combination ``sum_c conj(S_c) x_c`` with ``sens_maps``
    (b, 1, c, h, w, 2), else per coil (b, c, h, w).  ``chol``, ``scale``: the noise, as ``noise.add_noise`` takes it.  ``info`` (b, 4)
    and ``check`` as in ``grappa``.  The maps hold for every frame (they do not depend on a frame's lattice offset) and for the
    lattice alone: see the module docstring for what the closed form leaves out, and ``grappa_gfactor_from_weights`` for the map of a
    root-sum-of-squares image.  ``accel=None`` raises ``ValueError``: unevenly spaced rows are not shift-invariant."""
    if accel is None:
        raise ValueError("grappa_noise_maps: accel=None (unevenly spaced rows) has no analytic noise map: the reconstruction is not "
                         "shift-invariant; noise.pseudo_replica measures one")
    accel, ky, kx, lam = _settings(accel, kernel, lam, calib, acs, calib_rows, "magnitude", sens_maps)
    from .classical import _no_grad_inputs
    _no_grad_inputs("grappa_noise_maps", masked_kspace=masked_kspace, sens_maps=sens_maps, chol=chol)
    with torch.no_grad():
        masked_kspace, mask, (lo, hi) = _inputs("grappa_noise_maps", masked_kspace, mask, sens_maps, accel, ky, kx, calib, acs, calib_rows)
        rows = _host_rows(mask)
        plan_lattice(mask, accel)
        for i in range(rows.shape[0]):
            empty = np.flatnonzero(~rows[i, :, lo:hi].any(axis=0))
            if empty.size:
                raise ValueError(f"grappa_noise_maps: row {lo + int(empty[0])} of the calibration block [{lo}, {hi}) of batch element {i} was "
                                 f"acquired by no frame")
        maps, info = _run_noise_maps(masked_kspace, mask, sens_maps, chol, scale, accel, ky, kx, lam, calib, acs, calib_rows)
        if check:
            _check_residuals(info, lam)
    return maps, info


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


def _settings_gaps(gaps, max_gap, kernel, lam, calib, acs, calib_rows, output, sens_maps):
    """The settings of the gap path: (steps or "auto", max_gap, kx, lam).  The lattice settings are checked with the step 2."""
    max_gap = _max_gap(max_gap)
    _, _, _, lam = _settings(2, kernel, lam, calib, acs, calib_rows, output, sens_maps)
    kx = _kernel_gaps(kernel)
    if not (isinstance(gaps, str) and gaps == "auto"):
        gaps = _gap_sizes(gaps, max_gap)
    return gaps, max_gap, kx, lam


def _run_gaps(masked_kspace, mask, sens_maps, sizes, max_gap, kx, lam, calib, acs, calib_rows, output):
    """The launch sequence of the gap path, shared by ``grappa`` and ``Grappa.forward``: (result, info (b, len(sizes), 4), count (b, t),
    unfilled (b, t))."""
    b, t, c, h, w, _ = masked_kspace.shape
    table, count, unfilled = gap_table(mask, sizes, max_gap)
    cal = calibration_data(masked_kspace, mask, calib, acs, calib_rows)
    filled = torch.empty_like(masked_kspace)
    infos = []
    for i in range(b):
        weights, info = grappa_weights_gaps(cal[i], sizes, (2, kx), lam)
        grappa_apply_gaps(masked_kspace[i], weights, sizes, mask[i].view(t, h), table[i], count[i], (2, kx), out=filled[i])
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
    return res, info, count, unfilled


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


def grappa(masked_kspace: torch.Tensor, mask: torch.Tensor, accel: Optional[int] = None, kernel=(2, 5), lam: float = 1e-4,
           calib: str = "auto", acs: Optional[Sequence[int]] = None, calib_rows: int = 32, sens_maps: Optional[torch.Tensor] = None,
           output: str = "magnitude", check: bool = True, record: bool = False, gaps="auto", max_gap: int = MAX_GAP,
           max_unfilled: float = 0.0):
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
    frame acquired, ``CineHipError`` for CPU tensors (no fallback) and inputs that require grad.  Not differentiable.

    ``accel=None``: unevenly spaced rows (the module docstring; ``gaps``, ``max_gap`` and ``max_unfilled`` are read in this case only).
    Every frame is filled gap by gap from the two acquired neighbours, so ``kernel[0]`` must be 2.  ``gaps``: the steps to fit kernels
    for, "auto" for those that occur in the mask (read on the host, as the lattice path reads it); ``max_gap`` (<= 8): larger gaps stay
    unfilled.  ``max_unfilled``: the share of a batch element's missing rows that may stay unfilled; above it ``ValueError`` names the
    first such frame and row.  The calibration block needs at least max(gaps) + 1 rows.  ``record``: also return info
    (b, len(gaps), 4), the steps as a tuple and the unfilled rows (b, t) int32."""
    if accel is None:
        return _grappa_gaps(masked_kspace, mask, kernel, lam, calib, acs, calib_rows, sens_maps, output, check, record, gaps, max_gap,
                            max_unfilled)
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


def _check_residuals(info, lam):
    resid = info[..., 0].cpu().numpy()
    if not np.all(np.isfinite(resid)) or float(resid.max()) > RESIDUAL_MAX:
        raise CineHipError(f"grappa: the float64 solve of the kernels left the relative residuals {resid.tolist()} "
                           f"(not finite, or above {RESIDUAL_MAX:g}): a NaN in the calibration data, or lam = {lam:g} too small")


def _grappa_gaps(masked_kspace, mask, kernel, lam, calib, acs, calib_rows, sens_maps, output, check, record, gaps, max_gap, max_unfilled):
    """``grappa(accel=None)``."""
    gaps, max_gap, kx, lam = _settings_gaps(gaps, max_gap, kernel, lam, calib, acs, calib_rows, output, sens_maps)
    max_unfilled = float(max_unfilled)
    if not 0.0 <= max_unfilled <= 1.0:
        raise ValueError(f"max_unfilled = {max_unfilled!r}: a share in [0, 1]")
    from .classical import _no_grad_inputs
    _no_grad_inputs("grappa", masked_kspace=masked_kspace, sens_maps=sens_maps)
    with torch.no_grad():
        if not isinstance(mask, torch.Tensor):
            raise CineHipError("grappa: masked_kspace, mask and sens_maps must be GPU tensors (the HIP path has no CPU fallback)")
        rows = _host_rows(mask)                                      # the mask on the host, to choose the steps and to fail early
        if rows.ndim != 3:
            raise ValueError(f"grappa: mask {tuple(mask.shape)} is no row mask (b, t, 1, h, 1, 1)")
        sizes = plan_gaps(rows.reshape(-1, rows.shape[-1]), max_gap)[1] if gaps == "auto" else gaps
        if not sizes:                                                # nothing to fill within reach: one step keeps the launch sequence whole
            sizes = (2,)
        for i in range(rows.shape[0]):
            missing = int((~rows[i]).sum())
            left = [(f, _plan_frame(rows[i, f], max_gap, set(sizes))[1]) for f in range(rows.shape[1])]
            n_left = sum(len(u) for _, u in left)
            if missing and n_left > max_unfilled * missing:
                f, u = next((f, u) for f, u in left if u)
                raise ValueError(f"grappa: {n_left} of the {missing} missing rows of batch element {i} would stay unfilled (max_unfilled = "
                                 f"{max_unfilled:g}): the first is row {u[0]} of frame {f}, in a gap above max_gap = {max_gap} or of a step "
                                 f"not in gaps = {tuple(sizes)}")
        masked_kspace, mask, (lo, hi) = _inputs("grappa", masked_kspace, mask, sens_maps, sizes[-1], 2, kx, calib, acs, calib_rows)
        for i in range(rows.shape[0]):
            empty = np.flatnonzero(~rows[i, :, lo:hi].any(axis=0))
            if empty.size:
                raise ValueError(f"grappa: row {lo + int(empty[0])} of the calibration block [{lo}, {hi}) of batch element {i} was acquired by "
                                 f"no frame")
        res, info, _, unfilled = _run_gaps(masked_kspace, mask, sens_maps, sizes, max_gap, kx, lam, calib, acs, calib_rows, output)
        if check:
            _check_residuals(info, lam)
    return (res, info, tuple(sizes), unfilled) if record else res


class Grappa(nn.Module):
    """``grappa`` as a module with the models' ``forward`` signature and no parameters: ``SlicePipeline(Grappa(accel=4).eval())``
    reconstructs slices in flight, raw input included.  The lattice offsets come from ``cine_grappa_offsets`` and nothing is read by the
    host, so ``forward`` can be captured; there is no ``check`` -- frames without a lattice are left as they are and a failed solve shows
    in ``last_info``: the device tensors ``info`` (b, 4), ``offsets`` (b, t) and ``status`` (b, t) of the last call.

    ``accel=None``: unevenly spaced rows, with kernels for the steps ``gaps`` -- explicit, because ``forward`` reads nothing on the host;
    the default is what the reference's equispaced masks have at acceleration 4.  The gap table comes from ``cine_grappa_gaps``; rows in
    gaps of other steps, or above ``max_gap``, are left as they are.  ``last_info`` then holds ``info`` (b, len(gaps), 4), ``count``
    (b, t), the gaps listed per frame, and ``unfilled`` (b, t), the rows left."""

    def __init__(self, accel: Optional[int] = None, kernel=(2, 5), lam: float = 1e-4, calib: str = "auto",
                 acs: Optional[Sequence[int]] = None, calib_rows: int = 32, gaps: Sequence[int] = (2, 3, 4, 5, 6), max_gap: int = MAX_GAP):
        super().__init__()
        self.calib, self.acs, self.calib_rows = calib, (None if acs is None else tuple(int(v) for v in acs)), int(calib_rows)
        self.last_info = None
        self.accel = None
        if accel is None:
            if isinstance(gaps, str):
                raise ValueError(f"Grappa: gaps = {gaps!r}: the steps must be explicit, forward reads nothing on the host")
            self.gaps, self.max_gap, self.kx, self.lam = _settings_gaps(gaps, max_gap, kernel, lam, calib, acs, calib_rows, "magnitude", None)
            self.ky, self.kernel = 2, (2, self.kx)
            return
        self.accel, self.ky, self.kx, self.lam = _settings(accel, kernel, lam, calib, acs, calib_rows, "magnitude", None)
        self.kernel = (self.ky, self.kx)

    def forward(self, masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: Optional[torch.Tensor] = None,
                output: str = "magnitude") -> torch.Tensor:
        if self.accel is None:
            _settings_gaps(self.gaps, self.max_gap, self.kernel, self.lam, self.calib, self.acs, self.calib_rows, output, sens_maps)
            with torch.no_grad():
                masked_kspace, mask, _ = _inputs("Grappa", masked_kspace, mask, sens_maps, self.gaps[-1], 2, self.kx, self.calib, self.acs,
                                                 self.calib_rows)
                res, info, count, unfilled = _run_gaps(masked_kspace, mask, sens_maps, self.gaps, self.max_gap, self.kx, self.lam, self.calib,
                                                       self.acs, self.calib_rows, output)
            self.last_info = {"info": info, "count": count, "unfilled": unfilled}
            return res
        _settings(self.accel, self.kernel, self.lam, self.calib, self.acs, self.calib_rows, output, sens_maps)
        with torch.no_grad():
            masked_kspace, mask, _ = _inputs("Grappa", masked_kspace, mask, sens_maps, self.accel, self.ky, self.kx, self.calib, self.acs,
                                             self.calib_rows)
            res, info, offsets, status = _run(masked_kspace, mask, sens_maps, self.accel, self.ky, self.kx, self.lam, self.calib, self.acs,
                                              self.calib_rows, output)
        self.last_info = {"info": info, "offsets": offsets, "status": status}
        return res

    def noise_maps(self, masked_kspace: torch.Tensor, mask: torch.Tensor, sens_maps: Optional[torch.Tensor] = None,
                   chol: Optional[torch.Tensor] = None, scale: float = 1.0) -> GfactorMaps:
        """The analytic noise maps of this reconstruction, ``GfactorMaps(g, std)`` as ``grappa_noise_maps`` returns them, with nothing
        read by the host (capturable; there is no ``check``): the fit's ``info`` (b, 4) is in ``last_info``.  ``accel=None`` raises
        ``ValueError``: unevenly spaced rows are not shift-invariant."""
        if self.accel is None:
            raise ValueError("Grappa.noise_maps: accel=None (unevenly spaced rows) has no analytic noise map: the reconstruction is not "
                             "shift-invariant; noise.pseudo_replica measures one")
        from .classical import _no_grad_inputs
        _no_grad_inputs("Grappa.noise_maps", masked_kspace=masked_kspace, sens_maps=sens_maps, chol=chol)
        with torch.no_grad():
            masked_kspace, mask, _ = _inputs("Grappa.noise_maps", masked_kspace, mask, sens_maps, self.accel, self.ky, self.kx, self.calib,
                                             self.acs, self.calib_rows)
            maps, info = _run_noise_maps(masked_kspace, mask, sens_maps, chol, scale, self.accel, self.ky, self.kx, self.lam, self.calib,
                                         self.acs, self.calib_rows)
        self.last_info = {"info": info}
        return maps
