"""Retrospective cardiac gating: the acquisition list of a scan -> the raw (t, x, y, coil) array the front-end starts from.

    plan = plan_gating(pe_index, trigger_ms, rr_ms, n_frames=15, nx=416, mode="linear", reject=(0.8, 1.2))    # host, once per slice
    raw = gate_readouts(lines_on_device, plan)                    # (n_frames, nx, ny, coil), one launch (cine_gate_readouts)
    pipe.submit_readouts(lines, plan, mask, ...)                  # the same inside a SlicePipeline: only what was acquired is copied

A scanner delivers readouts, not frames: readout i holds the phase-encode line ``pe_index[i]`` (along x, the axis of the reference's row
mask, subsample.py:147-150), taken ``trigger_ms[i]`` after the last R-wave of a beat ``rr_ms[i]`` long.  Its cardiac phase is
``phi = trigger_ms / rr_ms``.  ``plan_gating`` sorts the readouts into ``n_frames`` cardiac phases on the host and writes the result down
as a sparse matrix in CSR form, one row per output line (frame, x): ``out[f, x] = sum_j weight[j] * lines[index[j]]``.  The device applies
it (``csrc/gating_kernels.hip``); the readout at (frame, x) is the contiguous span ``raw[frame, x, :, :]`` of ny * coil samples.

Not built: respiratory gating, self-gating from the data, reading ISMRMRD files, temporal interpolation of higher order than linear.
"""
from typing import Optional

import numpy as np
import torch

from . import ops
from ._lib import CineHipError, check, lib

MODES = ("nearest", "linear")


class GatingPlan:
    """A gating matrix in CSR form, validated: ``row_ptr`` (n_frames * nx + 1) int32, ``index`` int32 into the ``n_lines`` readouts of
    the acquisition list, ``weight`` float32; row ``f * nx + x`` is the output line (f, x).  ``acquired``: uint8 (n_frames, nx), 1 where
    the row has an entry -- the k-t sampling pattern of the gated scan.  ``info``: what ``plan_gating`` counted.  The device trusts
    these arrays (cine_gate_readouts reads ``lines[index[j]]`` unchecked), so they are checked here, once, and ``CineHipError`` names
    what is wrong: a ``row_ptr`` that is not non-decreasing from 0 to the entry count, an index outside [0, n_lines), a weight that is
    not finite.  Treat a plan as immutable: ``to(device)`` caches the device copies."""

    def __init__(self, n_frames: int, nx: int, n_lines: int, row_ptr, index, weight, info: Optional[dict] = None):
        for name, v in (("n_frames", n_frames), ("nx", nx)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise CineHipError(f"GatingPlan: {name} must be a positive integer, got {v!r}")
        if isinstance(n_lines, bool) or not isinstance(n_lines, (int, np.integer)) or n_lines < 0:
            raise CineHipError(f"GatingPlan: n_lines must be a non-negative integer, got {n_lines!r}")
        self.n_frames, self.nx, self.n_lines = int(n_frames), int(nx), int(n_lines)
        rows = self.n_frames * self.nx
        rp, ix, w = np.asarray(row_ptr), np.asarray(index), np.asarray(weight)
        if rp.ndim != 1 or ix.ndim != 1 or w.ndim != 1 or rp.dtype.kind not in "iu" or ix.dtype.kind not in "iu" or w.dtype.kind != "f":
            raise CineHipError("GatingPlan: row_ptr and index must be one-dimensional integer arrays, weight a one-dimensional float array")
        if rp.shape[0] != rows + 1:
            raise CineHipError(f"GatingPlan: row_ptr has {rp.shape[0]} entries, {rows + 1} = n_frames * nx + 1 expected")
        if ix.shape[0] != w.shape[0] or ix.shape[0] >= 2 ** 31:
            raise CineHipError(f"GatingPlan: {ix.shape[0]} indices and {w.shape[0]} weights (one each per entry, fewer than 2^31)")
        rp64 = rp.astype(np.int64)
        if rp64[0] != 0 or rp64[-1] != ix.shape[0] or bool((np.diff(rp64) < 0).any()):
            raise CineHipError(f"GatingPlan: row_ptr must be non-decreasing from 0 to the entry count {ix.shape[0]} "
                               f"(it runs from {int(rp64[0])} to {int(rp64[-1])})")
        if ix.shape[0] and not (0 <= int(ix.min()) and int(ix.max()) < self.n_lines):
            raise CineHipError(f"GatingPlan: index outside [0, {self.n_lines}): min {int(ix.min())}, max {int(ix.max())}")
        w32 = w.astype(np.float32)                                           # the one rounding of a float64 weight
        if not bool(np.isfinite(w32).all()):
            raise CineHipError("GatingPlan: a weight is not finite")
        self.row_ptr = np.ascontiguousarray(rp64.astype(np.int32))
        self.index = np.ascontiguousarray(ix.astype(np.int32))
        self.weight = np.ascontiguousarray(w32)
        self.acquired = (np.diff(rp64) > 0).astype(np.uint8).reshape(self.n_frames, self.nx)
        self.info = dict(info or {})
        self._dev = {}
        self._host = None

    @property
    def rows(self) -> int:
        return self.n_frames * self.nx

    @property
    def entries(self) -> int:
        return int(self.index.shape[0])

    def host_tensors(self):
        """(row_ptr, index, weight) as torch tensors on the host, index and weight with one element at least; pinned when there is a GPU
        (a SlicePipeline then copies them straight from here)."""
        if self._host is None:
            pin = torch.cuda.is_available()
            ts = []
            for a in (self.row_ptr, self.index, self.weight):
                t = torch.zeros(max(a.shape[0], 1), dtype=torch.from_numpy(a).dtype)
                t[:a.shape[0]] = torch.from_numpy(a)
                ts.append(t.pin_memory() if pin else t)
            self._host = tuple(ts)
        return self._host

    def to(self, device):
        """(row_ptr, index, weight) on ``device``, copied once and kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = tuple(t.to(device) for t in self.host_tensors())
        return self._dev[device]

    def __repr__(self):
        return (f"GatingPlan(n_frames={self.n_frames}, nx={self.nx}, n_lines={self.n_lines}, entries={self.entries}, "
                f"acquired={int(self.acquired.sum())}/{self.rows})")


def plan_gating(pe_index, trigger_ms, rr_ms, n_frames: int, nx: int, mode: str = "nearest", reject=None) -> GatingPlan:
    """The gating matrix of an acquisition list.  Host code (numpy); needs no GPU.

    Per readout: ``pe_index`` in [0, nx), ``trigger_ms`` since the R-wave, ``rr_ms`` the length of its beat (a scalar serves all);
    ``phi = trigger_ms / rr_ms`` in float64.  Dropped, in this order of precedence and counted in ``plan.info``: with ``reject=(lo, hi)``
    every readout whose ``rr_ms`` lies outside ``[lo, hi] x median(rr_ms)`` (arrhythmic beats; the median over all readouts) --
    ``dropped_reject``; an index outside [0, nx) -- ``dropped_index``; ``phi`` outside [0, 1) or not finite -- ``dropped_phase``.
    The dropped readouts keep their place in ``lines``: ``index`` refers to the acquisition list as given.

    ``mode="nearest"``: frame ``floor(phi * n_frames)``; a cell holds the mean of its readouts, weights 1 / k in acquisition order;
    a cell without a readout stays empty (a k-t pattern, ``plan.acquired``).
    ``mode="linear"``: per x the readouts of identical phase form one node (equal shares), the nodes are sorted by phase, and frame f
    with centre ``theta = (f + 0.5) / n_frames`` takes its two cyclic neighbours ``phi_a <= theta < phi_b`` (the last node at
    ``phi - 1`` in front of the first, the first at ``phi + 1`` behind the last) with ``w_a = (phi_b - theta) / (phi_b - phi_a)``,
    ``w_b = 1 - w_a``, a's readouts in front of b's; a neighbour of weight exactly 0 is left out.  An x with one node gives it to every
    frame with weight 1; an x with none stays empty in every frame.
    Weights are formed in float64 and rounded once to float32."""
    if mode not in MODES:
        raise CineHipError(f"plan_gating: mode {mode!r}; expected one of {MODES}")
    for name, v in (("n_frames", n_frames), ("nx", nx)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise CineHipError(f"plan_gating: {name} must be a positive integer, got {v!r}")
    n_frames, nx = int(n_frames), int(nx)
    pe = np.asarray(pe_index)
    if pe.ndim != 1 or pe.dtype.kind not in "iu":
        raise CineHipError("plan_gating: pe_index must be a one-dimensional integer array")
    n = pe.shape[0]
    pe = pe.astype(np.int64)
    trig = np.asarray(trigger_ms, dtype=np.float64)
    rr = np.asarray(rr_ms, dtype=np.float64)
    if trig.shape != (n,) or rr.shape not in ((), (n,)):
        raise CineHipError(f"plan_gating: {n} readouts, trigger_ms of shape {trig.shape}, rr_ms of shape {rr.shape}; expected one value "
                           "per readout (rr_ms may be a scalar)")
    rr = np.broadcast_to(rr, (n,))
    keep = np.ones(n, dtype=bool)
    info = {"n_lines": n, "mode": mode, "dropped_reject": 0}
    if reject is not None:
        try:
            lo, hi = (float(v) for v in reject)
        except (TypeError, ValueError):
            raise CineHipError(f"plan_gating: reject must be (lo, hi), got {reject!r}") from None
        if not 0 <= lo <= hi:
            raise CineHipError(f"plan_gating: reject (lo, hi) = ({lo}, {hi}); expected 0 <= lo <= hi")
        if n:
            med = float(np.median(rr))
            bad = ~((rr >= lo * med) & (rr <= hi * med))
            info["dropped_reject"] = int(bad.sum())
            info["rr_median_ms"] = med
            keep &= ~bad
    bad = keep & ~((pe >= 0) & (pe < nx))
    info["dropped_index"] = int(bad.sum())
    keep &= ~bad
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = trig / rr
    bad = keep & ~((phi >= 0.0) & (phi < 1.0))                               # a NaN fails both comparisons
    info["dropped_phase"] = int(bad.sum())
    keep &= ~bad
    used = np.flatnonzero(keep)                                              # acquisition order
    info["used"] = int(used.shape[0])
    rows = n_frames * nx
    if mode == "nearest":
        f = np.minimum(np.floor(phi[used] * n_frames).astype(np.int64), n_frames - 1)
        row = f * nx + pe[used]
        order = np.argsort(row, kind="stable")                               # by row, acquisition order inside a row
        count = np.bincount(row, minlength=rows)
        row_ptr = np.concatenate(([0], np.cumsum(count)))
        index = used[order]
        weight = 1.0 / count[row[order]].astype(np.float64)
    else:
        theta = (np.arange(n_frames, dtype=np.float64) + 0.5) / n_frames
        per_row = [None] * rows                                              # (indices, weights) of row f * nx + x
        by_x = np.argsort(pe[used], kind="stable")
        starts = np.searchsorted(pe[used][by_x], np.arange(nx + 1))
        for x in range(nx):
            mem = used[by_x[starts[x]:starts[x + 1]]]                        # this line's readouts, acquisition order
            if not mem.shape[0]:
                continue
            nodes, inv = np.unique(phi[mem], return_inverse=True)            # sorted phases; identical ones merged
            members = [mem[inv == k] for k in range(nodes.shape[0])]
            m = nodes.shape[0]
            if m == 1:
                one = (members[0], np.full(members[0].shape[0], 1.0 / members[0].shape[0]))
                for fr in range(n_frames):
                    per_row[fr * nx + x] = one
                continue
            pos = np.searchsorted(nodes, theta, side="right") - 1            # the last node at or in front of theta, -1: none
            for fr in range(n_frames):
                a = int(pos[fr])
                b = a + 1
                pa = nodes[a] if a >= 0 else nodes[m - 1] - 1.0
                pb = nodes[b] if b < m else nodes[0] + 1.0
                a, b = a % m, b % m
                wa = (pb - theta[fr]) / (pb - pa)
                wb = 1.0 - wa
                idx = [members[k] for k, wk in ((a, wa), (b, wb)) if wk != 0.0]
                wts = [np.full(members[k].shape[0], wk / members[k].shape[0]) for k, wk in ((a, wa), (b, wb)) if wk != 0.0]
                per_row[fr * nx + x] = (np.concatenate(idx), np.concatenate(wts))
        count = np.array([0 if e is None else e[0].shape[0] for e in per_row], dtype=np.int64)
        row_ptr = np.concatenate(([0], np.cumsum(count)))
        filled = [e for e in per_row if e is not None]
        index = np.concatenate([e[0] for e in filled]) if filled else np.zeros(0, dtype=np.int64)
        weight = np.concatenate([e[1] for e in filled]) if filled else np.zeros(0, dtype=np.float64)
    info["entries"] = int(index.shape[0])
    info["empty_rows"] = int((np.diff(row_ptr) == 0).sum())
    return GatingPlan(n_frames, nx, n, row_ptr, index.astype(np.int64), weight.astype(np.float64), info)


def _line_pairs(lines: torch.Tensor, what: str) -> torch.Tensor:
    """Device readouts (n_lines, ny, coil) complex64 or (n_lines, ny, coil, 2) float32, contiguous, as float32 pairs."""
    if not isinstance(lines, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor")
    if lines.is_complex():
        if lines.dtype != torch.complex64:
            raise CineHipError(f"{what}: lines are {lines.dtype}; expected complex64 or float32 pairs")
        if not lines.is_contiguous():
            raise CineHipError(f"{what}: lines must be contiguous")
        lines = torch.view_as_real(lines)
    if lines.dtype != torch.float32 or lines.dim() != 4 or lines.shape[-1] != 2:
        raise CineHipError(f"{what}: lines {tuple(lines.shape)} {lines.dtype}; expected (n_lines, ny, coil) complex64 or "
                           "(n_lines, ny, coil, 2) float32")
    return ops._dev(lines, "lines")


def gate_into(lines: torch.Tensor, row_ptr: torch.Tensor, index: torch.Tensor, weight: torch.Tensor, n_lines: int,
              out: torch.Tensor) -> None:
    """cine_gate_readouts on the current stream: float32 pairs ``lines`` (>= n_lines, ny, coil, 2) and ``out`` (n_frames, nx, ny, coil, 2),
    the CSR arrays on the device.  No check beyond the library's: ``gate_readouts`` and the pipeline call it with a plan's arrays."""
    t, nx, ny, c, _ = out.shape
    check(lib().cine_gate_readouts(lines.data_ptr(), out.data_ptr(), row_ptr.data_ptr(), index.data_ptr(), weight.data_ptr(), int(n_lines),
                                   t * nx, ny * c, ops._stream()), "cine_gate_readouts")


def gate_readouts(lines: torch.Tensor, plan: GatingPlan, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gated raw array ``(n_frames, nx, ny, coil)`` of the readouts ``lines`` -- (n_lines, ny, coil) complex64 or (n_lines, ny, coil, 2)
    float32 on the GPU, contiguous, in the order the plan was made for -- in the input's form: row (f, x) is
    ``sum_j weight[j] * lines[index[j]]`` over the plan's entries of the row, in their order, the first term a product and every further
    one an ``fmaf``; rows without an entry are zeros.  One launch; every element of the result is written.  ``out``: the result's place
    (same form, contiguous).  Not differentiable."""
    if not isinstance(plan, GatingPlan):
        raise CineHipError(f"gate_readouts: plan: expected a GatingPlan (plan_gating), got {type(plan).__name__}")
    cplx = isinstance(lines, torch.Tensor) and lines.is_complex()
    if isinstance(lines, torch.Tensor) and lines.requires_grad:
        raise CineHipError("gate_readouts: not differentiable; detach the readouts")
    k = _line_pairs(lines, "gate_readouts")
    if k.shape[0] != plan.n_lines:
        raise CineHipError(f"gate_readouts: {k.shape[0]} readouts, the plan was made for {plan.n_lines}")
    _, ny, c, _ = k.shape
    if ny < 1 or c < 1:
        raise CineHipError(f"gate_readouts: lines {tuple(lines.shape)}: empty readouts")
    shape = (plan.n_frames, plan.nx, ny, c)
    if out is None:
        res = torch.empty(shape + (2,), device=k.device, dtype=torch.float32)
    else:
        if not (isinstance(out, torch.Tensor) and out.device == k.device and out.dtype == lines.dtype and out.is_contiguous()
                and tuple(out.shape) == (shape if cplx else shape + (2,))):
            raise CineHipError(f"gate_readouts: out must be a contiguous {lines.dtype} tensor {shape if cplx else shape + (2,)} on the "
                               "readouts' device")
        res = torch.view_as_real(out) if cplx else out
    src = k if k.numel() else torch.empty(2, device=k.device, dtype=torch.float32)      # no readouts: a non-null pointer
    gate_into(src, *plan.to(k.device), plan.n_lines, res)
    if out is not None:
        return out
    return torch.view_as_complex(res) if cplx else res


def readouts_from_raw(raw, acquired, rr_ms: float = 1000.0):
    """The inverse, for retrospective experiments and tests: the lines of a binned ``raw`` (t, x, y, coil) array (numpy or torch, any
    device) at the acquired (t, x) -- ``acquired`` (t, nx), non-zero where a line was taken -- as an acquisition list
    ``(lines, pe_index, trigger_ms, rr_ms)``: frame by frame, x ascending, every trigger at its frame's centre ``(f + 0.5) / t * rr_ms``
    of a beat ``rr_ms`` long.  ``lines`` is of raw's kind.  ``gate_readouts(lines, plan_gating(pe_index, trigger_ms, rr_ms, t, nx))``
    is then ``raw`` with its unacquired lines zeroed, bit for bit (one entry of weight 1.0 per acquired line)."""
    acq = acquired.detach().cpu().numpy() if isinstance(acquired, torch.Tensor) else np.asarray(acquired)
    if not isinstance(raw, (np.ndarray, torch.Tensor)) or raw.ndim < 4:
        raise CineHipError("readouts_from_raw: raw: expected a (t, x, y, coil) numpy array or torch tensor")
    t, nx = int(raw.shape[0]), int(raw.shape[1])
    if acq.shape != (t, nx):
        raise CineHipError(f"readouts_from_raw: acquired {acq.shape}; expected ({t}, {nx}) for raw {tuple(raw.shape)}")
    if not float(rr_ms) > 0:
        raise CineHipError(f"readouts_from_raw: rr_ms = {rr_ms!r} must be positive")
    f, x = np.nonzero(acq)                                                   # row-major: frame by frame, x ascending
    if isinstance(raw, torch.Tensor):
        lines = raw[torch.from_numpy(f).to(raw.device), torch.from_numpy(x).to(raw.device)].contiguous()
    else:
        lines = np.ascontiguousarray(raw[f, x])
    trigger = (f.astype(np.float64) + 0.5) / t * float(rr_ms)
    return lines, x.astype(np.int64), trigger, np.full(f.shape[0], float(rr_ms), dtype=np.float64)
