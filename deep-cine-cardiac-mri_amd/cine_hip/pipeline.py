"""SlicePipeline: many cine slices in flight through a reconstruction model, from the public API.

    pipe = SlicePipeline(model, slots=10)                   # model: any reconstruction.models model, eval(), on the GPU
    for i, (mk, mask) in enumerate(slices):
        pipe.submit(mk, mask, tag=i)                        # returns at once unless 2 x slots slices are pending
        for tag, out in pipe.results():                     # finished slices, in submission order
            ...
    for tag, out in pipe.drain():                           # the rest
        ...
    pipe.close()                                            # (or: with SlicePipeline(...) as pipe)

The scheme is the one the benchmark times.  Slice k goes to slot k mod S.  A slot is a stream of its own with two input buffer
sets and one captured hipGraph per set; slice k reads set (k // S) & 1 of its slot.  The inputs of slice k are copied into
that set on ONE copy stream, after the done-event of slice k - 2S, the set's previous reader.  The replay waits for the
copy's ready-event, then the output is copied out of the graph's static output into a tensor of the caller's own, and the
slice's done-event is recorded behind it.  ``submit`` blocks only when 2S slices are pending, and then waits for the
OLDEST slice alone.  So the copy stream never waits for a replay still in flight: slice k - 2S has been retired on the
host before slice k's copy is issued.

Every U-Net pass runs on the slot's stream (``ops.branches(1)``): the other slices fill the chip, and side streams would
compete with the slot streams for hardware queues.  The pipeline creates no side streams.  Its streams come from a pool made
once per device (``pipeline_streams``).  Set GPU_MAX_HW_QUEUES to at least slots + 1 before the first GPU call of the process
(importing ``cine_hip`` sets 16 when it is unset and the runtime is not up yet).

Inputs (``submit``): k-space as complex64 (b, t, c, h, w) or float32 (b, t, c, h, w, 2), a torch tensor or a numpy array.
  * pinned host tensor: copied to HBM asynchronously, straight from the caller's memory.  Do not modify it until its slice
    has finished (the pipeline keeps a reference until then).
  * pageable host tensor or numpy array: copied by the host into a pinned ring of two staging buffers that the pipeline owns,
    then asynchronously to HBM.  That host copy is one memcpy of the slice (72 MB for 15 coils x 15 frames x 200 x 200)
    inside ``submit``, on torch's intra-op threads; it bounds the rate only when it takes longer than a slice's share of the
    GPU (tools/pipeline_rate.py measures both).
  * device tensor: copied device to device on the copy stream, ordered after the caller's current stream.
The mask follows the k-space's place; host masks may be any numeric 0 / 1 mask that broadcasts like the reference's
(converted on the host), device masks must be uint8 or bool.  ``sens_maps`` (b, 1, c, h, w, 2) is required by CineNet /
CineNet_RNN, optional for VarNet, and not accepted by the other models.

``sens_maps="espirit"`` (the same three models): the maps are calibrated IN FLIGHT, per slice, as the reference does with
``bart ecalib -r 15`` on the time-averaged masked k-space (data/transforms.py:425-432).  Inside the slot's graph, behind the front-end of
a raw set and for every batch element, ``frontend.espirit_maps(frontend.time_average(mk[i]), r=ecalib_r, method="sign",
sign_iters=sign_iters)`` writes a static (b, 1, c, h, w, 2) buffer that the model reads: the result is bit for bit
``model(mk, mask, maps)`` with those maps computed eagerly.  The projector of the calibration comes from a matrix sign function
(Newton-Schulz steps on the float64 matrix cores) instead of an eigen-decomposition, so nothing waits for the host.  The residual
max |X^2 - I| of every slice's sign matrix is copied to pinned memory with the outputs; ``results`` / ``drain`` raise ``CineHipError``
naming the slice's tag when it exceeds 1e-6 (an eigenvalue of the Gram matrix sits at the threshold: raise ``sign_iters``) -- no silent
wrong maps.  ``("espirit", ecalib_r, kernel, thresh, crop, sign_iters)`` stands for the sens shape in the set key (``espirit_key``).
With ``coil_matrix=`` the calibration runs on the V virtual coils.  A mask that varies along w is served with VarNet this way too
(the sensitivity network is not run).

The model is called as ``model(mk, mask)`` or ``model(mk, mask, sens)``, without ``acs=``: the ACS window is found on the
device (``ops.acs_window_dev``) and a graph captured with one slice's mask gives any other slice's result.  That window is
read from row masks only; a mask that varies along w with a model that runs its sensitivity network raises ``CineHipError``.
With ``sens_maps`` such a mask is served like a row mask, by ``submit`` and ``submit_raw`` alike (the front-end masks with
``cine_apply_mask2d``, the models run their image-space operators with both line passes, ``ops.GENERAL_MASK_FUSED``).

Outputs (``results`` / ``drain``): ``(tag, out)`` in submission order; ``out`` is ``recon`` or, with ``zero_filled=True``,
``(recon, zero_filled)`` (reference run_inference.py:64-67, computed inside the same graph by ``cine_zero_filled_rss``).
They are fresh device tensors (``out="device"``, marked as used on the stream that is current when they are handed out) or
pinned host tensors (``out="host"``); no later replay writes to them.

Shapes: the graphs, buffers and events form one SET keyed by the input shapes and dtypes.  Only one set is alive: a submit
with a new key drains the pending slices (their results stay queued), frees the old set and builds a new one (one eager
forward per slot stream, then two captures per slot).

Raw input (``submit_raw``): the raw k-space ``(t, x, y, coil)`` of a slice, complex64 or float32 pairs, from the same four places.  Only
``raw[:min(n_frames, t)]`` -- a contiguous prefix -- is copied, on the copy stream, into a raw buffer of the slice's (slot, parity); the
graph of that (slot, parity) then holds ``frontend.prepare_masked_slice`` (scaling, inverse transform, crop, Gaussian filter, forward
transform, masking, written into the static k-space buffer) AND the model's forward that reads it.  Same events, same schedule, same
streams.  The set key of raw input is ``raw_set_key(...)``: kind, kept raw shape, crop, filter, scaling, apply_mask, mask shape, sens
shape; ``submit`` and ``submit_raw`` may alternate, a change of kind is a change of key.  With ``coil_matrix=A`` (V, coil) the matrix is
copied with the raw data and ``compress_coils`` runs eagerly on the slot's stream in front of the replay, into a static (T, x, y, V)
buffer the graph starts from: the coil count is not part of the key, scans with different coil counts and one V share a set, and the
raw buffers (plain byte buffers then) are replaced by larger ones, after a drain, when a larger scan arrives.  ``2 * slots`` raw
buffers are checked against ``torch.cuda.mem_get_info`` before they are allocated.  A raw slice's copy is long (5.5 ms for 311 MB):
on a hardware queue shared with slot streams it waits behind whole replays, so the ``slots + 1`` queues above matter more here.

``submit_raw(..., virtual_coils=V, cc_region=24)``: every slice is compressed with the matrix of ITS OWN calibration block, as
``prepare_slice(..., virtual_coils=V)`` does, without leaving the pipeline.  In front of the replay, where ``compress_coils`` runs for
``coil_matrix=``, the slot's stream runs ``frontend.coil_gram`` into a static buffer of the (slot, parity), cine_coil_matrix (the
eigenvectors by a Jacobi eigensolver in LDS, ``frontend.coil_matrix_from_gram(..., method="jacobi")``: no host read) into the buffer
the copied matrix of ``coil_matrix=`` would occupy, and ``compress_coils``.  The result is bit for bit
``model(prepare_masked_slice(raw, mask, ..., coil_matrix=A), mask)`` with ``A = coil_matrix_from_gram(coil_gram(raw, n_frames,
cc_region), V, method="jacobi")[0]``.  ``(V, cc_region)`` is part of the set key and the coil count is not, so scans with different
coil counts and one V share a set; the Gram workspaces grow like the raw buffers, after a drain.  At most 64 coils (the eigensolver's
LDS) and V <= 32; scans with more coils take ``coil_matrix=``.  The eigensolver's record of every slice -- the residual
max |off-diagonal| / max |diagonal| it reached, its sweeps, the kept share sum(lam[:V]) / sum(lam), lam[0] -- is copied to pinned
memory with the outputs: ``results`` / ``drain`` raise ``CineHipError`` naming the slice's tag when the residual is not finite or
exceeds the solver's own stopping bar 1e-14 (its sweep cap was hit, or the raw data hold a NaN), and file the record of every slice they
hand out under ``pipe.last_coil_info[tag]`` (``CoilInfo(residual, sweeps, kept, lam0)``; the last ``COIL_INFO_KEPT`` slices).

``submit_raw(..., whitener=W)``: noise pre-whitening with the scan's whitener W (coil, coil) complex128 from
``frontend.noise_whitener`` -- numpy, pinned or device memory.  With ``virtual_coils=V`` W is copied with the raw data into a static buffer
of the (slot, parity) and the slot's stream runs cine_coil_matrix_whitened where it ran cine_coil_matrix: the matrix is that of the
whitened calibration block composed with W, ``compress_coils`` whitens and compresses in its one pass, and the result is bit for bit
``model(prepare_masked_slice(raw, mask, ..., coil_matrix=A), mask)`` with ``A = coil_matrix_from_gram(coil_gram(raw, n_frames,
cc_region), V, method="jacobi", whitener=W)[0]``.  The set key ends with ``("virtual", V, cc_region, "whitened")``; the coil count stays
out of it, and ``last_coil_info`` and the residual check hold for the whitened Gram matrix.  ``whitener`` alone is
``coil_matrix=W.to(torch.complex64)`` (at most 32 coils); together with ``coil_matrix=`` it raises.  ``sens_maps="espirit"`` then
calibrates on the whitened virtual coils.

``submit(..., noise=noise.NoiseSpec(chol, scale, seed, replica))``: one pseudo replica (``cine_hip.noise``).  The slot's stream runs
cine_noise_add in place on the slot's copy of the k-space, between the wait for the copy and the replay, so the result is bit for bit
``model(noise.add_noise(masked_kspace, mask, chol, scale=scale, seed=seed, replica=replica), mask[, sens_maps])``.  The spec is not part of
the set key and no graph holds it: replicas and plain slices share one set, and ``noise=None`` is the path as it was.
``submit_raw(..., noise=NoiseSpec, noise_mask=None)``: the replica of a raw scan.  cine_noise_add_raw runs in place on the slot's copy of
the raw data, behind the wait for the copy and in front of the coil compression and the graph, so the noise passes through whitening, compression
(``virtual_coils=``: the matrix of the noisy slice), crop, filter, mask and calibration as a scan's own does.  ``noise_mask`` (the acquired
samples; for prospectively undersampled raw) is an input like the others, with a per-slot buffer that is made on first use.

``submit_readouts(lines, plan, mask, ...)``: the slice from its ACQUISITION LIST (``cine_hip.gating``): the readouts (n_lines, y, coil) that
were acquired and a ``GatingPlan``, the sparse matrix that sorts them into cardiac phases.  Only the readouts and the plan's three CSR arrays
are copied, on the copy stream, into buffers of the (slot, parity); the slot's stream runs cine_gate_readouts into the slot's raw buffer
behind the wait for the copy, in front of cine_noise_add_raw and the coil compression, and everything downstream is ``submit_raw``'s path:
the result is bit for bit ``submit_raw(gating.gate_readouts(lines, plan), mask, apply_mask=False, n_frames=plan.n_frames, ...)``.  The set
key is that call's key, so both may alternate on one set; the readout count and the entry count are not part of it -- the gating
buffers are made when a set first serves readouts and replaced by larger ones, after a drain, like the raw buffers.

``graphs=False`` is the explicit eager mode: same slots, streams, buffers, copies and events, with the launch sequence
enqueued on the slot's stream for every slice.  A failure raises ``CineHipError``; nothing falls back to eager launches.

Not thread-safe: one pipeline is driven from one thread.  One pipeline per GPU (``device=``) for several GPUs.
"""
import collections
import inspect
import math
from typing import Optional

import numpy as np
import torch

from . import frontend, ops
from ._lib import CineHipError


class SliceSchedule:
    """The slot / parity / event bookkeeping of a SlicePipeline, without a GPU.

    Slice k runs in slot k mod S on buffer set (k // S) & 1 of that slot.  ``copy_after`` of a step is the slice whose
    done-event the copy into that buffer set waits for (its previous reader), or None for the set's first use.  At most
    ``2 * slots`` slices are in flight: ``must_retire`` names the slice the host has to wait for before the next submit."""

    Step = collections.namedtuple("Step", "index slot parity copy_after")

    def __init__(self, slots: int):
        if isinstance(slots, bool) or not isinstance(slots, int) or slots < 1:
            raise ValueError(f"slots: a positive integer, got {slots!r}")
        self.slots = slots
        self.capacity = 2 * slots
        self.next_index = 0
        self.inflight = collections.deque()        # submitted, not yet known to be finished (oldest first)
        self.finished = collections.deque()        # known to be finished, not yet handed out (oldest first)
        self._last_reader = {}                     # (slot, parity) -> index of the last slice that read the set

    def place(self, k: int):
        return k % self.slots, (k // self.slots) & 1

    def must_retire(self) -> Optional[int]:
        """The oldest in-flight slice if the pipeline is full (the next submit has to wait for it), else None."""
        return self.inflight[0] if len(self.inflight) >= self.capacity else None

    def submit(self) -> "SliceSchedule.Step":
        if len(self.inflight) >= self.capacity:
            raise RuntimeError("SliceSchedule: full; retire the oldest slice first")
        k = self.next_index
        slot, parity = self.place(k)
        after = self._last_reader.get((slot, parity))
        if after is not None and after in self.inflight:
            raise RuntimeError(f"SliceSchedule: slice {k} would overwrite the inputs of slice {after}, still in flight")
        self._last_reader[(slot, parity)] = k
        self.next_index = k + 1
        self.inflight.append(k)
        return self.Step(k, slot, parity, after)

    def retire_oldest(self) -> int:
        k = self.inflight.popleft()
        self.finished.append(k)
        return k

    def take_finished(self) -> Optional[int]:
        return self.finished.popleft() if self.finished else None

    def new_buffers(self) -> None:
        """The buffer sets were replaced (new shapes, after a drain): no set has a previous reader."""
        if self.inflight:
            raise RuntimeError("SliceSchedule: buffers replaced with slices in flight")
        self._last_reader.clear()

    def pending(self) -> int:
        return len(self.inflight) + len(self.finished)


_STREAMS = {}


def pipeline_streams(device: torch.device, slots: int):
    """(slot streams, copy stream) of a device, from a pool created ONCE per process and device, like bench.py's
    ``bench_streams``: torch hands out streams from a fixed pool of 32 per device and the runtime maps them onto
    GPU_MAX_HW_QUEUES hardware queues as they are first used, so all of them are created and used at the first call,
    before a side stream or a later pipeline claims a queue.  Pipelines on one device share the pool (a stream is an
    in-order queue; every cross-stream edge of a pipeline is an event of its own)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    pool = _STREAMS.setdefault(idx, {"copy": None, "slots": []})
    with torch.cuda.device(idx):
        if pool["copy"] is None:
            pool["copy"] = _used_stream(idx)
        while len(pool["slots"]) < max(slots, 12):
            pool["slots"].append(_used_stream(idx))
    return pool["slots"][:slots], pool["copy"]


def _used_stream(idx: int) -> "torch.cuda.Stream":
    st = torch.cuda.Stream(device=idx)
    with torch.cuda.stream(st):
        torch.empty(1, device=torch.device("cuda", idx)).zero_()       # first use = the moment the runtime gives the stream its queue
    return st


def _forward_params(model: torch.nn.Module):
    """(takes sens_maps, needs sens_maps) from the model's forward signature."""
    try:
        p = inspect.signature(model.forward).parameters.get("sens_maps")
    except (TypeError, ValueError):                     # pragma: no cover
        p = None
    return p is not None, p is not None and p.default is inspect.Parameter.empty


def _pairs(x, name: str):
    """A float32 (..., 2) torch view of x (complex64 or float32 (..., 2); torch tensor or numpy array) and its kind:
    'device', 'pinned' or 'pageable'."""
    if isinstance(x, np.ndarray):
        if x.dtype == np.complex64:
            x = np.ascontiguousarray(x).view(np.float32).reshape(x.shape + (2,))
        elif x.dtype != np.float32:
            raise CineHipError(f"{name}: numpy dtype {x.dtype}; expected complex64 or float32 (..., 2)")
        x = torch.from_numpy(x)
    elif not isinstance(x, torch.Tensor):
        raise CineHipError(f"{name}: expected a torch tensor or a numpy array, got {type(x).__name__}")
    if x.dtype == torch.complex64:
        x = torch.view_as_real(x if x.is_contiguous() else x.contiguous())
    if x.dtype != torch.float32:
        raise CineHipError(f"{name}: dtype {x.dtype}; expected complex64 or float32 (..., 2)")
    if x.dim() < 1 or x.shape[-1] != 2:
        raise CineHipError(f"{name}: shape {tuple(x.shape)} is not complex64 data or float32 (..., 2)")
    if x.is_cuda:
        return x, "device"
    return x, ("pinned" if x.is_pinned() and x.is_contiguous() else "pageable")


def _mask_shape(mask_shape, ks_shape):
    """The shape ``ops.as_mask_u8`` brings a mask into: (b, t, 1, h, 1, 1) row mask or (b, t, 1, h, w, 1) general mask."""
    b, t, _, h, w, _ = ks_shape
    m = tuple(mask_shape)
    if len(m) != 6 or m[2] != 1 or m[5] != 1 or m[3] != h or m[0] not in (1, b) or m[1] not in (1, t) or m[4] not in (1, w):
        raise CineHipError(f"mask {m} does not broadcast against k-space {tuple(ks_shape)} as (b|1, t|1, 1, h, w|1, 1)")
    return (b, t, 1, h, m[4], 1)


def _check_mask(mask, ks_shape):
    """(mask as given or canonical host uint8, kind, the shape its buffer has)."""
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(mask)
    if not isinstance(mask, torch.Tensor):
        raise CineHipError(f"mask: expected a torch tensor or a numpy array, got {type(mask).__name__}")
    want = _mask_shape(mask.shape, ks_shape)
    if mask.is_cuda:
        if mask.dtype not in (torch.uint8, torch.bool):
            raise CineHipError(f"mask: a device mask must be uint8 or bool (got {mask.dtype}); pass other dtypes from the host")
        return mask, "device", want
    m = mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)
    m = m.expand(want)
    canonical = m.is_contiguous() and m.is_pinned()
    return (m, "pinned", want) if canonical else (m.contiguous(), "pageable", want)


ESPIRIT_KERNEL, ESPIRIT_THRESH, ESPIRIT_CROP = 6, 1e-3, 0.8      # ecalib's defaults, as frontend.espirit_maps has them
ESPIRIT_RESIDUAL_MAX = 1e-6     # max |X^2 - I| of the sign matrix above which the projector is not one at float32 resolution


def espirit_key(ecalib_r: int = 15, sign_iters: int = 60):
    """What stands for the sens shape in a set key when the maps are calibrated in flight (``sens_maps="espirit"``)."""
    r, it = int(ecalib_r), int(sign_iters)
    if r < ESPIRIT_KERNEL or it < 1:
        raise CineHipError(f"sens_maps='espirit': ecalib_r must be at least the kernel size {ESPIRIT_KERNEL} and sign_iters at least 1, "
                           f"got {ecalib_r!r}, {sign_iters!r}")
    return ("espirit", r, ESPIRIT_KERNEL, ESPIRIT_THRESH, ESPIRIT_CROP, it)


def _check_sens(pipe, sens_maps, ks_shape, general: bool):
    """(float32 pairs, "espirit" or None; kind or None)."""
    b, _, c, h, w, _ = ks_shape
    if isinstance(sens_maps, str):
        if sens_maps != "espirit":
            raise CineHipError(f"sens_maps: {sens_maps!r} is not a tensor, None or 'espirit'")
        if not pipe._takes_sens:
            raise CineHipError(f"{type(pipe.model).__name__} takes no sens_maps")
        if c > 32 or h < 2 * ESPIRIT_KERNEL - 1 or w < 2 * ESPIRIT_KERNEL - 1:
            raise CineHipError(f"sens_maps='espirit': at most 32 coils and an image of at least {2 * ESPIRIT_KERNEL - 1} x "
                               f"{2 * ESPIRIT_KERNEL - 1}, got {c} coils, {h} x {w}")
        return "espirit", None
    if sens_maps is not None:
        if not pipe._takes_sens:
            raise CineHipError(f"{type(pipe.model).__name__} takes no sens_maps")
        s, kind = _pairs(sens_maps, "sens_maps")
        if tuple(s.shape) != (b, 1, c, h, w, 2):
            raise CineHipError(f"sens_maps: shape {tuple(s.shape)}; expected {(b, 1, c, h, w, 2)} for this k-space")
        return s, kind
    if pipe._needs_sens:
        raise CineHipError(f"{type(pipe.model).__name__} needs sens_maps")
    if general:
        raise CineHipError("the mask varies along w: the ACS window of the sensitivity network is found on the device from row masks "
                           "only; pass sens_maps (VarNet) or use a row mask (b|1, t|1, 1, h, 1, 1)")
    return None, None


def _same_device(pipe, named):
    for name, x in named:
        if x is not None and x.is_cuda and x.device != pipe.device:
            raise CineHipError(f"{name} is on {x.device}, the pipeline's device is {pipe.device}")


def _check_noise(pipe, spec, c: int):
    """``submit(..., noise=)`` / ``submit_raw(..., noise=)`` validated for data of c coils: a noise.NoiseSpec with its factor as float32
    pairs on the pipeline's device, or None."""
    if spec is None:
        return None
    from . import noise as N
    if not isinstance(spec, N.NoiseSpec):
        raise CineHipError(f"noise: expected a cine_hip.noise.NoiseSpec(chol, scale, seed, replica), got {type(spec).__name__}")
    if c > N.NOISE_MAX_COILS:
        raise CineHipError(f"noise: {c} coils, at most {N.NOISE_MAX_COILS}")
    if isinstance(spec.replica, bool) or not isinstance(spec.replica, int) or not 0 <= spec.replica < 1 << 32:
        raise CineHipError(f"noise: replica {spec.replica!r} is not an integer in [0, 2^32)")
    return spec._replace(chol=N._chol_pairs(spec.chol, c, pipe.device), scale=float(spec.scale), seed=int(spec.seed))


class _Source:
    """One slice's validated inputs: torch views in their original place, the canonical mask, the set key."""
    raw = None                                      # no front-end in this set's graphs
    input_names = ("mk", "mask", "sens")

    def __init__(self, pipe, masked_kspace, mask, sens_maps, ecalib_r=15, sign_iters=60, noise=None):
        c = masked_kspace.shape[2] if isinstance(masked_kspace, torch.Tensor) and masked_kspace.dim() >= 5 else 0
        self.noise = _check_noise(pipe, noise, c)                            # not part of the key: the graphs do not hold it
        mk, self.mk_kind = _pairs(masked_kspace, "masked_kspace")
        if mk.dim() != 6:
            raise CineHipError(f"masked_kspace: shape {tuple(mk.shape)}; expected (b, t, c, h, w, 2) or complex (b, t, c, h, w)")
        self.mk = mk
        self.mk_shape = tuple(mk.shape)
        self.mask, self.mask_kind, self.mask_shape = _check_mask(mask, mk.shape)
        self.sens, self.sens_kind = _check_sens(pipe, sens_maps, mk.shape, self.mask_shape[4] > 1)
        self.espirit = None
        if isinstance(self.sens, str):                                       # calibrated in flight: nothing to copy in
            self.sens, self.espirit = None, espirit_key(ecalib_r, sign_iters)
        _same_device(pipe, (("masked_kspace", self.mk), ("mask", self.mask), ("sens_maps", self.sens)))
        self.key = (tuple(mk.shape), self.mask_shape, self.espirit or (None if self.sens is None else tuple(self.sens.shape)))

    def alloc(self, pipe):
        dev = pipe.device
        b = {"mk": torch.empty(self.mk_shape, device=dev, dtype=torch.float32),
             "mask": torch.empty(self.mask_shape, device=dev, dtype=torch.uint8),
             "sens": None if self.sens is None else torch.empty(self.sens.shape, device=dev, dtype=torch.float32)}
        _alloc_espirit(b, self, dev)
        return b

    def items(self, b):
        """(name, destination in buffer set b, source, kind) of every input the copy stream moves."""
        it = [("mk", b["mk"], self.mk, self.mk_kind), ("mask", b["mask"], self.mask, self.mask_kind)]
        if self.sens is not None:
            it.append(("sens", b["sens"], self.sens, self.sens_kind))
        return it


def _alloc_espirit(b, src, dev) -> None:
    """The static maps the calibration writes and the model reads, and the residual of every batch element's sign iteration."""
    if src.espirit is not None:
        n, _, c, h, w, _ = src.mk_shape
        b["sens"] = torch.empty((n, 1, c, h, w, 2), device=dev, dtype=torch.float32)
        b["resid"] = torch.empty(n, device=dev, dtype=torch.float64)


_CC_MAX_COILS, _CC_MAX_VIRTUAL = 128, 32            # the limits of cine_coil_compress (include/cine_hip.h)
_CM_MAX_COILS = frontend.COIL_MATRIX_MAX_COILS      # the limit of cine_coil_matrix
COIL_RESIDUAL_MAX = 1e-14       # kLsJacobiTol (csrc/ls_jacobi.h): the eigensolver's own stopping test, missed only at its sweep cap
COIL_INFO_KEPT = 4096           # records SlicePipeline.last_coil_info holds
CoilInfo = collections.namedtuple("CoilInfo", "residual sweeps kept lam0")


def raw_set_key(raw_shape, n_frames, crop_shape, filter_size, scaling, apply_mask, mask_shape, sens_shape, coil_matrix_shape=None,
                espirit=None, virtual_coils=None, whitened=False):
    """The key of the graph set that serves a ``submit_raw`` call, from shapes and settings alone: kind, kept raw shape, virtual coils,
    crop, filter, scaling, apply_mask, mask shape, sens shape.  With a coil matrix the raw coil count is NOT part of it: the compression
    runs in front of the graph, so scans with different coil counts and one V share a set.  ``espirit``: ``espirit_key(ecalib_r,
    sign_iters)`` for ``sens_maps="espirit"``; it takes the place of the sens shape.  ``virtual_coils``: ``(V, cc_region)`` for
    ``submit_raw(..., virtual_coils=V, cc_region=...)``; the key then ends with ``("virtual", V, cc_region)`` and, as with a coil matrix,
    leaves the coil count out.  Without it the key is what it was.  ``whitened``: ``submit_raw(..., virtual_coils=V, whitener=W)``; the
    marker then reads ``("virtual", V, cc_region, "whitened")`` (another launch sequence in front of the graph).  A whitener without
    ``virtual_coils`` is a coil matrix: describe it by ``coil_matrix_shape``."""
    t, nx, ny, c = (int(v) for v in tuple(raw_shape)[:4])
    n = min(int(n_frames), t)
    if n < 1 or nx < 1 or ny < 1 or c < 1:
        raise ValueError("Invalid shapes.")
    if virtual_coils is not None and coil_matrix_shape is not None:
        raise ValueError("raw_set_key: virtual_coils or coil_matrix_shape, not both")
    if whitened and virtual_coils is None:
        raise ValueError("raw_set_key: whitened marks a virtual_coils set; a whitener alone is a coil matrix (coil_matrix_shape)")
    kept = (n, nx, ny, c) if coil_matrix_shape is None and virtual_coils is None else (n, nx, ny)
    v = None if coil_matrix_shape is None else int(tuple(coil_matrix_shape)[0])
    tail = ()
    if virtual_coils is not None:
        v, region = (int(q) for q in virtual_coils)
        tail = (("virtual", v, region) + (("whitened",) if whitened else ()),)
    return ("raw", kept, v, (int(crop_shape[0]), int(crop_shape[1])), tuple(float(f) for f in filter_size), float(scaling),
            bool(apply_mask), tuple(int(m) for m in mask_shape),
            tuple(espirit) if espirit is not None else None if sens_shape is None else tuple(int(m) for m in sens_shape)) + tail


class _RawSource:
    """One raw slice's validated inputs (``submit_raw``): the kept frames of the raw data in their original place, mask, sens, the coil
    matrix, the front-end's settings, the set key."""
    input_names = ("raw", "mask", "sens", "cmat", "wh")

    def __init__(self, pipe, raw, mask, sens_maps, crop_shape, n_frames, filter_size, scaling, coil_matrix, apply_mask, ecalib_r=15,
                 sign_iters=60, virtual_coils=None, cc_region=24, whitener=None, noise=None, noise_mask=None, gate=None):
        self.gate = None                                # submit_readouts: (lines as pairs, their kind, the plan, its host tensors)
        if gate is not None:
            raw = _check_readouts(self, *gate)          # the gated array's shape on the meta device: the slot's stream writes the data
            n_frames = raw.shape[0]
            if noise is not None and noise_mask is None:
                noise_mask = gate[1].acquired           # the lines the gating filled
        if not isinstance(raw, (np.ndarray, torch.Tensor)):
            raise CineHipError(f"raw: expected a torch tensor or a numpy array, got {type(raw).__name__}")
        if raw.ndim < 4 or raw.shape[0] < 1 or int(n_frames) < 1:
            raise ValueError("Invalid shapes.")
        x, self.raw_kind = _pairs(raw[:min(int(n_frames), raw.shape[0])], "raw")     # the frame axis is the slowest: a contiguous prefix
        if x.dim() != 5:
            raise CineHipError(f"raw: shape {tuple(x.shape)}; expected (t, x, y, coil) complex64 or (t, x, y, coil, 2) float32")
        self.raw = x
        n, nx, ny, c, _ = x.shape
        self.n, self.c = n, c
        # a pseudo replica: noise on the slot's copy of the raw data, in front of everything; neither is part of the key
        self.noise = _check_noise(pipe, noise, c)
        self.nmask, self.nmask_kind = _check_noise_mask(noise_mask, self.noise, n, nx, ny)
        self.nmask_shape = None if self.nmask is None else (n,) + tuple(self.nmask.shape[1:])
        self.nmask_nbytes = n * nx * ny                                      # the slot's buffer serves either layout
        self.crop = (int(crop_shape[0]), int(crop_shape[1]))
        if not (0 < self.crop[0] <= nx and 0 < self.crop[1] <= ny):
            raise ValueError("Invalid shapes.")                              # transforms.py:206-207
        self.filter = tuple(float(f) for f in filter_size)
        if len(self.filter) != 4:
            raise CineHipError("filter_size: one sigma per axis of (t, coil, x, y)")
        self.scaling, self.apply_mask = float(scaling), bool(apply_mask)
        self.cmat, self.cmat_kind = None, None
        self.vc, self.cc_region = None, None                                 # virtual_coils=: the matrix is computed in flight
        self.wh, self.wh_kind = None, None                                   # whitener= with virtual_coils=: W (c, c, 2) float64 pairs
        if whitener is not None:
            if coil_matrix is not None:
                raise CineHipError("whitener and coil_matrix: a given matrix is applied as it is; fold the whitener into it, "
                                   "frontend.coil_matrix_from_gram(..., whitener=W), and pass that matrix alone")
            w, kind = _whitener_pairs(whitener, c)
            if virtual_coils is None:                                        # the whitener alone: a (c, c) coil matrix
                if c > _CC_MAX_VIRTUAL:
                    raise CineHipError(f"whitener alone keeps all {c} channels, the compression writes at most {_CC_MAX_VIRTUAL}: pass "
                                       "virtual_coils= as well (the whitener is then folded into every slice's matrix)")
                coil_matrix = torch.view_as_complex(w).to(torch.complex64)
            else:
                self.wh, self.wh_kind = w, kind
        if virtual_coils is not None:
            if coil_matrix is not None:
                raise CineHipError("virtual_coils computes every slice's own matrix, coil_matrix brings one: pass one of the two")
            if isinstance(virtual_coils, bool) or not isinstance(virtual_coils, (int, np.integer)) or isinstance(cc_region, bool) \
                    or not isinstance(cc_region, (int, np.integer)) or cc_region < 0:
                raise CineHipError(f"virtual_coils and cc_region must be integers, cc_region >= 0; got {virtual_coils!r}, {cc_region!r}")
            if c > _CM_MAX_COILS:
                raise CineHipError(f"virtual_coils: this scan has {c} coils, the in-flight eigensolver takes at most {_CM_MAX_COILS}; "
                                   f"compute one matrix per scan (frontend.coil_compression_matrix) and pass it as coil_matrix= (up to "
                                   f"{_CC_MAX_COILS} coils)")
            if not 1 <= virtual_coils <= min(c, _CC_MAX_VIRTUAL):
                raise CineHipError(f"virtual_coils = {virtual_coils}: 1 <= V <= {min(c, _CC_MAX_VIRTUAL)} for this scan's {c} coils (at most "
                                   f"{_CC_MAX_VIRTUAL} virtual coils)")
            self.vc, self.cc_region = int(virtual_coils), int(cc_region)
        if coil_matrix is not None:
            a, self.cmat_kind = _pairs(coil_matrix, "coil_matrix")
            if a.dim() != 3 or a.shape[1] != c:
                raise CineHipError(f"coil_matrix: shape {tuple(a.shape[:-1])}; expected (V, {c}) for this scan's {c} coils")
            if not (1 <= a.shape[0] <= min(c, _CC_MAX_VIRTUAL) and c <= _CC_MAX_COILS):
                raise CineHipError(f"coil_matrix (V, coil) = {tuple(a.shape[:-1])}: 1 <= V <= coil, at most {_CC_MAX_VIRTUAL} virtual and "
                                   f"{_CC_MAX_COILS} physical coils")
            self.cmat = a
        self.v = self.vc if self.vc is not None else None if self.cmat is None else self.cmat.shape[0]
        self.cmat_shape = None if self.v is None else (self.v, c, 2)
        self.mk_shape = (1, n, self.v or c, self.crop[0], self.crop[1], 2)
        self.mask, self.mask_kind, self.mask_shape = _check_mask(mask, self.mk_shape)
        # a mask that varies along w: the rules of ``submit`` (the sensitivity network's ACS window needs a row mask)
        self.sens, self.sens_kind = _check_sens(pipe, sens_maps, self.mk_shape, self.mask_shape[4] > 1)
        self.espirit = None
        if isinstance(self.sens, str):                                       # calibrated in flight, on the V virtual coils with a coil matrix
            self.sens, self.espirit = None, espirit_key(ecalib_r, sign_iters)
        _same_device(pipe, (("raw", self.raw), ("mask", self.mask), ("sens_maps", self.sens), ("coil_matrix", self.cmat),
                            ("whitener", self.wh), ("noise_mask", self.nmask)))
        self.raw_nbytes = x.numel() * 4
        if self.gate is not None:
            _same_device(pipe, (("lines", self.gate[0]),))
        self.gram_nbytes = 0                                                 # asked of the library when a buffer is needed (_submit, alloc)
        self.key = raw_set_key((n, nx, ny, c), n, self.crop, self.filter, self.scaling, self.apply_mask, self.mask_shape,
                               None if self.sens is None else self.sens.shape, None if self.cmat is None else self.cmat.shape, self.espirit,
                               None if self.vc is None else (self.vc, self.cc_region), self.wh is not None)

    def gram_bytes(self) -> int:
        """Workspace of this slice's coil_gram (virtual_coils=), 0 otherwise."""
        if self.vc is not None and not self.gram_nbytes:
            n, nx, ny, c, _ = self.raw.shape
            self.gram_nbytes = max(frontend.coil_gram_ws_bytes(n, nx, ny, c, self.cc_region), 16)
        return self.gram_nbytes

    def alloc(self, pipe):
        """raw: a byte buffer (with a coil matrix it may be replaced by a larger one later: no graph holds its address).  cc: what the
        eager compression writes and the graph reads.  mk: written and read inside the graph.  virtual_coils=: gram, lam and cinfo for
        the largest coil count cine_coil_matrix takes, gws (coil_gram's workspace) replaced by a larger one like raw; wh, the copied
        whitener, for that coil count too."""
        dev = pipe.device
        n, nx, ny = self.raw.shape[:3]
        b = {"raw": torch.empty(self.raw_nbytes, device=dev, dtype=torch.uint8),
             "cmat": None if self.v is None else torch.empty(self.v * _CC_MAX_COILS * 8, device=dev, dtype=torch.uint8),
             "cc": None if self.v is None else torch.empty((n, nx, ny, self.v, 2), device=dev, dtype=torch.float32),
             "mk": torch.empty(self.mk_shape, device=dev, dtype=torch.float32),
             "mask": torch.empty(self.mask_shape, device=dev, dtype=torch.uint8),
             "sens": None if self.sens is None else torch.empty(self.sens.shape, device=dev, dtype=torch.float32)}
        b["front"] = b["cc"] if self.v is not None else self.raw_view(b)
        b["wh"] = None if self.wh is None else torch.empty(_CM_MAX_COILS * _CM_MAX_COILS, device=dev, dtype=torch.complex128)
        if self.vc is not None:
            b["gram"] = torch.empty(_CM_MAX_COILS * _CM_MAX_COILS, device=dev, dtype=torch.complex128)
            b["lam"] = torch.empty(_CM_MAX_COILS, device=dev, dtype=torch.float64)
            b["cinfo"] = torch.empty((1, frontend.COIL_MATRIX_INFO), device=dev, dtype=torch.float64)
            b["gws"] = torch.empty(self.gram_bytes(), device=dev, dtype=torch.uint8)
        _alloc_espirit(b, self, dev)
        return b

    def raw_view(self, b):
        return b["raw"][:self.raw_nbytes].view(torch.float32).view(self.raw.shape)

    def cmat_view(self, b):
        v, c, _ = self.cmat_shape
        return b["cmat"][:v * c * 8].view(torch.float32).view(self.cmat_shape)

    def wh_view(self, b):
        c = self.c
        return b["wh"][:c * c].view(c, c)

    def nmask_view(self, b):
        return b["nmask"][:math.prod(self.nmask_shape)].view(self.nmask_shape)

    def gate_views(self, b):
        """(lines, row_ptr, index, weight) of this slice in the gating buffers of set b."""
        lines, _, plan, host = self.gate
        return (b["lines"][:max(lines.numel(), 2) * 4].view(torch.float32), b["rptr"][:host[0].numel()], b["gidx"][:host[1].numel()],
                b["gw"][:host[2].numel()])

    def items(self, b):
        if self.gate is None:
            it = [("raw", self.raw_view(b), self.raw, self.raw_kind)]
        else:                                            # the readouts and the plan in place of the binned array
            lines, kind, _, host = self.gate
            lv, rp, gi, gw = self.gate_views(b)
            it = [("lines", lv[:lines.numel()].view(lines.shape), lines, kind)] if lines.numel() else []
            it += [("rptr", rp, host[0], "pinned"), ("gidx", gi, host[1], "pinned"), ("gw", gw, host[2], "pinned")]
        it.append(("mask", b["mask"], self.mask, self.mask_kind))
        if self.nmask is not None:
            it.append(("nmask", self.nmask_view(b), self.nmask, self.nmask_kind))
        if self.sens is not None:
            it.append(("sens", b["sens"], self.sens, self.sens_kind))
        if self.cmat is not None:
            it.append(("cmat", self.cmat_view(b), self.cmat, self.cmat_kind))
        if self.wh is not None:
            it.append(("wh", torch.view_as_real(self.wh_view(b)), self.wh, self.wh_kind))
        return it


def _check_readouts(src, lines, plan):
    """``submit_readouts``'s readouts against its plan.  Files (lines as float32 pairs, their kind, the plan, its host tensors) under
    ``src.gate`` and returns a tensor without storage of the gated array's shape (n_frames, nx, ny, coil, 2)."""
    from . import gating
    if not isinstance(plan, gating.GatingPlan):
        raise CineHipError(f"plan: expected a cine_hip.gating.GatingPlan (gating.plan_gating), got {type(plan).__name__}")
    x, kind = _pairs(lines, "lines")
    if x.dim() != 4 or x.shape[1] < 1 or x.shape[2] < 1:
        raise CineHipError(f"lines: shape {tuple(x.shape)}; expected (n_lines, y, coil) complex64 or (n_lines, y, coil, 2) float32")
    if x.shape[0] != plan.n_lines:
        raise CineHipError(f"lines: {x.shape[0]} readouts, the plan was made for {plan.n_lines}")
    if kind == "device" and not x.is_contiguous():
        x = x.contiguous()
    src.gate = (x, kind, plan, plan.host_tensors())
    src.input_names = ("lines", "rptr", "gidx", "gw") + _RawSource.input_names[1:]       # what a new set copies to its other buffer sets
    return torch.empty((plan.n_frames, plan.nx, x.shape[1], x.shape[2], 2), dtype=torch.float32, device="meta")


def _gate_capacity(src):
    """(bytes of readouts, CSR entries, row pointers) the gating buffers must hold for this slice; the last is fixed by the set key."""
    lines, _, _, host = src.gate
    return max(lines.numel(), 2) * 4, host[1].numel(), host[0].numel()


def _check_noise_mask(noise_mask, spec, n: int, nx: int, ny: int):
    """``submit_raw(..., noise_mask=)`` against the kept frames: (the mask as given or a host uint8 one, its kind), or (None, None).
    uint8 or bool, (n | 1, nx) for acquired lines or (n | 1, nx, ny); a leading 1 is expanded by the copy."""
    if noise_mask is None:
        return None, None
    if spec is None:
        raise CineHipError("noise_mask: says where noise= is added; without noise= there is nothing to mask")
    m = torch.from_numpy(noise_mask) if isinstance(noise_mask, np.ndarray) else noise_mask
    if not isinstance(m, torch.Tensor):
        raise CineHipError(f"noise_mask: expected a torch tensor or a numpy array, got {type(noise_mask).__name__}")
    if m.dtype not in (torch.uint8, torch.bool):
        raise CineHipError(f"noise_mask: dtype {m.dtype}; expected uint8 or bool")
    shape = tuple(m.shape)
    if not (m.dim() in (2, 3) and shape[0] in (1, n) and shape[1:] in ((nx,), (nx, ny))):
        raise CineHipError(f"noise_mask: shape {shape}; expected ({n} | 1, {nx}) or ({n} | 1, {nx}, {ny}) for the {n} kept frames of raw "
                           f"data (t, x, y) = ({n}, {nx}, {ny})")
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    if m.is_cuda:
        return m, "device"
    m = m.expand((n,) + shape[1:])
    canonical = m.is_contiguous() and m.is_pinned()
    return (m, "pinned") if canonical else (m.contiguous(), "pageable")


def _whitener_pairs(whitener, c: int):
    """A whitener (c, c) complex128 -- torch tensor or numpy array, device, pinned or pageable -- as float64 (c, c, 2) pairs, and its kind."""
    if isinstance(whitener, np.ndarray):
        if whitener.dtype != np.complex128:
            raise CineHipError(f"whitener: numpy dtype {whitener.dtype}; expected complex128 (frontend.noise_whitener)")
        whitener = torch.from_numpy(np.ascontiguousarray(whitener))
    elif not isinstance(whitener, torch.Tensor):
        raise CineHipError(f"whitener: expected a torch tensor or a numpy array, got {type(whitener).__name__}")
    if whitener.dtype != torch.complex128:
        raise CineHipError(f"whitener: dtype {whitener.dtype}; expected complex128 (frontend.noise_whitener)")
    if tuple(whitener.shape) != (c, c):
        raise CineHipError(f"whitener: shape {tuple(whitener.shape)}; expected ({c}, {c}) for this scan's {c} coils")
    w = torch.view_as_real(whitener if whitener.is_contiguous() else whitener.contiguous())
    if w.is_cuda:
        return w, "device"
    return w, ("pinned" if w.is_pinned() else "pageable")


def _settings_only(src: "_RawSource"):
    """The front-end's settings of a raw set, without the tensors of the slice that built it."""
    return collections.namedtuple("RawSettings", "crop n filter scaling apply_mask")(src.crop, src.n, src.filter, src.scaling, src.apply_mask)


class SliceHandle:
    """What ``submit`` returns: the slice's index (submission order), its tag, slot and buffer parity."""
    __slots__ = ("index", "tag", "slot", "parity", "_event")

    def __init__(self, index, tag, slot, parity, event):
        self.index, self.tag, self.slot, self.parity, self._event = index, tag, slot, parity, event

    def __repr__(self):
        return f"SliceHandle(index={self.index}, tag={self.tag!r}, slot={self.slot}, parity={self.parity})"


class _Set:
    """Buffers, graphs and events of one input key."""

    def __init__(self, key):
        self.key = key
        self.bufs = {}          # (slot, parity) -> {"mk", "mask", "sens"} (+ "raw", "cmat", "cc", "front", "wh" in a raw set; "gram", "gws", "lam", "cinfo" with virtual_coils=; "lines", "rptr", "gidx", "gw" once it serves readouts)
        self.raw = None         # the front-end's settings when the graphs start from raw data (the _RawSource that built the set)
        self.raw_bytes = 0      # capacity of each raw byte buffer
        self.gram_bytes = 0     # capacity of each Gram workspace (virtual_coils=)
        self.gate_cap = (0, 0)  # capacity of the gating buffers (submit_readouts): bytes of readouts, CSR entries; 0: none yet
        self.espirit = None     # espirit_key(...) when the graphs calibrate the maps themselves (sens_maps="espirit")
        self.graphs = {}        # (slot, parity) -> (graph, static outputs)
        self.ready = {}         # (slot, parity) -> event recorded on the copy stream behind the copy into the set
        self.done = {}          # (slot, parity) -> event recorded on the slot stream behind the output copy of the set's reader
        self.stage = None       # pinned ring of two staging sets for pageable inputs (lazily)
        self.stage_ev = None
        self.stage_next = 0


class SlicePipeline:
    """S slices in flight through ``model`` on one GPU (see the module docstring)."""

    def __init__(self, model: torch.nn.Module, slots: int = 10, device=None, graphs: bool = True, out: str = "device",
                 zero_filled: bool = False):
        if not isinstance(model, torch.nn.Module):
            raise CineHipError("SlicePipeline: model must be a torch.nn.Module of reconstruction.models")
        if model.training:
            raise CineHipError("SlicePipeline: the model is in training mode; call model.eval() (the pipeline is for inference)")
        if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= 31:
            raise CineHipError(f"SlicePipeline: slots must be an integer in 1..31, got {slots!r}")
        if out not in ("device", "host"):
            raise CineHipError(f"SlicePipeline: out must be 'device' or 'host', got {out!r}")
        if not torch.cuda.is_available():
            raise CineHipError("SlicePipeline: no GPU (the HIP path has no CPU fallback)")
        pdev = next((p.device for p in model.parameters()), None)
        if device is None:
            device = pdev if pdev is not None else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise CineHipError(f"SlicePipeline: device {device} is not a GPU")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if pdev is not None and pdev != device:
            raise CineHipError(f"SlicePipeline: the model's parameters are on {pdev}, the pipeline's device is {device}; move the model first")
        self.model, self.slots, self.device, self.graphs, self.out, self.zero_filled = model, slots, device, bool(graphs), out, bool(zero_filled)
        self._takes_sens, self._needs_sens = _forward_params(model)
        self._sched = SliceSchedule(slots)
        # index -> [handle, outputs, inputs kept alive until the slice is done, ESPIRiT residuals (pinned) or None, the coil eigensolver's
        # record (pinned) or None]
        self._recs = {}
        self.last_coil_info = collections.OrderedDict()      # tag -> CoilInfo of the slices handed out (virtual_coils=), the last COIL_INFO_KEPT
        self._set = None
        self._closed = False
        self._builds = 0
        self.streams, self.copy_stream = pipeline_streams(device, slots)

    # ---- public ----------------------------------------------------------------------------------------------------------
    def submit(self, masked_kspace, mask, sens_maps=None, tag=None, *, ecalib_r: int = 15, sign_iters: int = 60,
               noise=None) -> SliceHandle:
        """Enqueue one slice.  Returns at once, unless 2 x slots slices are pending: then it waits for the oldest one.
        ``sens_maps="espirit"``: the maps of every batch element are calibrated inside the slot's graph from the time average of its masked
        k-space, ``frontend.espirit_maps(frontend.time_average(mk[i]), r=ecalib_r, method="sign", sign_iters=sign_iters)`` (the
        reference's ``bart ecalib -r 15``, data/transforms.py:425-432).
        ``noise=noise.NoiseSpec(chol, scale, seed, replica)``: one pseudo replica -- the slot's stream runs cine_noise_add in place on
        the slot's copy of the k-space, between the copy and the replay, so the slice is reconstructed from
        ``noise.add_noise(masked_kspace, mask, chol, scale=scale, seed=seed, replica=replica)``, bit for bit.  The spec is not part of
        the set key; ``noise=None`` takes the path it always took.  It describes noise on the PREPARED k-space; noise where a
        receiver's enters, in front of the crop and the filter that colour it, is ``submit_raw(..., noise=)``."""
        if self._closed:
            raise CineHipError("SlicePipeline: submit after close()")
        return self._submit(_Source(self, masked_kspace, mask, sens_maps, ecalib_r, sign_iters, noise), tag)

    def submit_raw(self, raw, mask, sens_maps=None, tag=None, *, crop_shape=(200, 200), n_frames: int = 15,
                   filter_size=(0.7, 0.0, 0.3, 0.3), scaling: float = 1e6, coil_matrix=None, apply_mask: bool = True,
                   ecalib_r: int = 15, sign_iters: int = 60, virtual_coils: Optional[int] = None, cc_region: int = 24,
                   whitener=None, noise=None, noise_mask=None) -> SliceHandle:
        """Enqueue one slice from its RAW k-space (t, x, y, coil) -- complex64 or float32 pairs, in any of the four places ``submit`` takes
        its input from.  Only ``raw[:min(n_frames, t)]`` is copied to the device.  ``frontend.prepare_masked_slice`` and the model run on
        the slot's stream inside the slot's graph; see the module docstring.  ``mask``: the mask on the crop grid, a row mask or one that varies along w under the
        rules of ``submit`` (the sensitivity network needs a row mask: pass ``sens_maps``); ``sens_maps``
        (1, 1, C, X, Y, 2) on the crop grid (on the V virtual coils with ``coil_matrix`` (V, coil)), or ``"espirit"``: calibrated in the
        graph, behind the front-end, from the masked k-space it wrote (``ecalib_r``, ``sign_iters`` as in ``submit``).
        ``virtual_coils=V`` (with ``cc_region``, and without ``coil_matrix``): the slice is compressed to V virtual coils with the matrix
        of its own kept frames, computed on the slot's stream (at most 64 coils, V <= 32; see the module docstring).  The kept share of
        the slice is ``pipe.last_coil_info[tag].kept`` once ``results`` / ``drain`` have handed it out; ``tag`` must then be hashable.
        ``whitener=W`` (coil, coil) complex128 from ``frontend.noise_whitener`` on the scan's noise samples, from numpy, pinned or device
        memory: noise pre-whitening.  With ``virtual_coils=V`` it is folded into every slice's matrix on the slot's stream
        (cine_coil_matrix_whitened); alone it is ``coil_matrix=W.to(torch.complex64)``; with ``coil_matrix`` it raises.
        ``noise=noise.NoiseSpec(chol, scale, seed, replica)``: one pseudo replica with the noise where a receiver's enters -- the slot's
        stream runs cine_noise_add_raw in place on the slot's copy of the raw data, behind the wait for the copy and in front of
        everything else, so with ``virtual_coils=`` the Gram matrix and the (whitened) matrix are computed from the noisy slice, as a
        scanner would compute them.  The result is ``model(frontend.prepare_masked_slice(noise.add_noise_raw(raw[:n], chol,
        noise_mask=noise_mask, scale=scale, seed=seed, replica=replica), mask, <the same front-end arguments>), mask[, sens_maps])``,
        bit for bit; the caller's array is never written.  ``noise_mask``: the acquired samples, uint8 or bool (n | 1, x) or
        (n | 1, x, y) on the n kept frames, from any of the places an input may lie in -- None for fully sampled raw that is masked
        retrospectively (``apply_mask=True``), needed for prospectively undersampled raw (``apply_mask=False``), whose unacquired lines
        hold zeros and carry no noise.  Neither is part of the set key; ``noise=None`` takes the path it always took."""
        if self._closed:
            raise CineHipError("SlicePipeline: submit_raw after close()")
        src = _RawSource(self, raw, mask, sens_maps, crop_shape, n_frames, filter_size, scaling, coil_matrix, apply_mask,
                         ecalib_r, sign_iters, virtual_coils, cc_region, whitener, noise, noise_mask)
        if src.vc is not None:
            try:
                hash(tag)
            except TypeError:
                raise CineHipError(f"virtual_coils: tag {tag!r} is not hashable (last_coil_info is keyed by it)") from None
        return self._submit(src, tag)

    def submit_readouts(self, lines, plan, mask, sens_maps=None, tag=None, *, crop_shape=(200, 200),
                        filter_size=(0.7, 0.0, 0.3, 0.3), scaling: float = 1e6, coil_matrix=None, ecalib_r: int = 15, sign_iters: int = 60,
                        virtual_coils: Optional[int] = None, cc_region: int = 24, whitener=None, noise=None, noise_mask=None) -> SliceHandle:
        """Enqueue one slice from its ACQUISITION LIST: ``lines`` (n_lines, y, coil) complex64 or float32 pairs, the readouts in the order
        ``plan`` (``gating.plan_gating``) was made for, in any of the four places ``submit_raw`` takes its input from.  Only the readouts
        and the plan's CSR arrays are copied to the device; the slot's stream gates them (cine_gate_readouts) into the slot's raw buffer
        behind the wait for the copy and in front of everything ``submit_raw`` runs there.  The result is, bit for bit,
        ``submit_raw(gating.gate_readouts(lines, plan), mask, sens_maps, apply_mask=False, n_frames=plan.n_frames, <the same keywords>)``
        -- gated data are prospectively undersampled, so ``mask`` (the plan's pattern on the crop grid, for the model's data consistency)
        is not applied by the front-end.  The keywords are ``submit_raw``'s.  With ``noise=``, ``noise_mask`` defaults to
        ``plan.acquired``: the lines the gating filled carry noise, the empty ones stay zero.  The set key is that ``submit_raw``
        call's; ``n_lines`` and the plan's entry count are not part of it, and ``set_builds`` does not move when they change."""
        if self._closed:
            raise CineHipError("SlicePipeline: submit_readouts after close()")
        src = _RawSource(self, None, mask, sens_maps, crop_shape, 0, filter_size, scaling, coil_matrix, False, ecalib_r, sign_iters,
                         virtual_coils, cc_region, whitener, noise, noise_mask, gate=(lines, plan))
        if src.vc is not None:
            try:
                hash(tag)
            except TypeError:
                raise CineHipError(f"virtual_coils: tag {tag!r} is not hashable (last_coil_info is keyed by it)") from None
        return self._submit(src, tag)

    @property
    def set_builds(self) -> int:
        """How many graph sets this pipeline has built so far (one per change of the set key)."""
        return self._builds

    def _submit(self, src, tag) -> SliceHandle:
        with torch.cuda.device(self.device):
            if self._set is None or self._set.key != src.key:
                self._retire_all()
                self._set = None                               # one set alive: the old graphs and buffers go first
                self._sched.new_buffers()
                self._set = self._build(src)
            elif src.raw is not None and (src.raw_nbytes > self._set.raw_bytes or src.gram_bytes() > self._set.gram_bytes):
                # a scan with more coils than any before it (coil_matrix or virtual_coils given)
                self._grow_raw(max(src.raw_nbytes, self._set.raw_bytes), max(src.gram_bytes(), self._set.gram_bytes))
            if src.raw is not None and src.gate is not None:
                need, have = _gate_capacity(src), self._set.gate_cap
                if need[0] > have[0] or need[1] > have[1]:                  # the set's first readouts, or more of them than before
                    self._grow_gate(max(need[0], have[0]), max(need[1], have[1]), need[2])
            k0 = self._sched.must_retire()
            if k0 is not None:
                self._recs[k0][0]._event.synchronize()
                self._sched.retire_oldest()
            step = self._sched.submit()
            key = (step.slot, step.parity)
            ev_done = self._set.done[key]
            h = SliceHandle(step.index, step.index if tag is None else tag, step.slot, step.parity, ev_done)
            try:
                keep = self._copy_in(src, key, wait_done=step.copy_after is not None)
                outs, resid, cinfo = self._launch(key, src)
            except Exception:
                self._recs[step.index] = [h, None, None, None, None]
                raise
            self._recs[step.index] = [h, outs, keep, resid, cinfo]
            return h

    def results(self, block: bool = False):
        """Finished slices as (tag, out), in submission order; stops at the first unfinished one unless ``block``."""
        while True:
            k = self._sched.take_finished()
            if k is None:
                if not self._sched.inflight:
                    return
                k0 = self._sched.inflight[0]
                ev = self._recs[k0][0]._event
                if block:
                    ev.synchronize()
                elif not ev.query():
                    return
                self._sched.retire_oldest()
                continue
            h, outs, _, resid, cinfo = self._recs.pop(k)
            if outs is None:
                continue                  # a submit that raised: nothing was launched for it
            if resid is not None and not bool((resid <= ESPIRIT_RESIDUAL_MAX).all()):       # pinned host memory, the slice is done
                raise CineHipError(f"SlicePipeline: slice {h.tag!r}: the in-flight ESPIRiT calibration did not converge (max |X^2 - I| = "
                                   f"{float(resid.max()):.3e} > {ESPIRIT_RESIDUAL_MAX:g}): an eigenvalue of the calibration Gram matrix "
                                   "sits at the threshold; raise sign_iters")
            if cinfo is not None:                                                           # pinned host memory, the slice is done
                rec = CoilInfo(float(cinfo[0, 0]), int(cinfo[0, 1]), float(cinfo[0, 2]), float(cinfo[0, 3]))
                if not rec.residual <= COIL_RESIDUAL_MAX:                                   # a NaN fails the comparison too
                    raise CineHipError(f"SlicePipeline: slice {h.tag!r}: the in-flight coil compression's eigensolver stopped at "
                                       f"max |off-diagonal| / max |diagonal| = {rec.residual:.3e} after {rec.sweeps} sweeps (bar "
                                       f"{COIL_RESIDUAL_MAX:g}): its sweep cap was reached or the raw data hold a NaN")
                self.last_coil_info[h.tag] = rec
                self.last_coil_info.move_to_end(h.tag)
                while len(self.last_coil_info) > COIL_INFO_KEPT:
                    self.last_coil_info.popitem(last=False)
            if self.out == "device":
                cur = torch.cuda.current_stream(self.device)
                for o in outs:
                    o.record_stream(cur)
            yield h.tag, (outs if self.zero_filled else outs[0])

    def drain(self):
        """Every pending slice as (tag, out), in submission order (waits for them)."""
        return self.results(block=True)

    def pending(self) -> int:
        """Slices submitted and not yet handed out."""
        return self._sched.pending()

    def close(self) -> None:
        """Wait for the slices in flight and free the graphs and buffers.  Results not yet taken are dropped."""
        if self._closed:
            return
        try:
            self._retire_all()
        finally:
            self._closed = True
            self._recs.clear()
            self._set = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- internals -------------------------------------------------------------------------------------------------------
    def _retire_all(self):
        while self._sched.inflight:
            self._recs[self._sched.inflight[0]][0]._event.synchronize()
            self._sched.retire_oldest()

    def _forward(self, b):
        if b["sens"] is not None:
            return self.model(b["mk"], b["mask"], b["sens"])
        return self.model(b["mk"], b["mask"])

    def _run(self, b):
        """The slice's launch sequence on the current stream: the model's forward (+ the zero-filled image)."""
        with torch.no_grad(), ops.branches(1):
            o = self._forward(b)
            if not isinstance(o, torch.Tensor):
                raise CineHipError(f"SlicePipeline: {type(self.model).__name__}.forward returned {type(o).__name__}, not a tensor")
            return (o, ops.zero_filled_rss(b["mk"])) if self.zero_filled else (o,)

    def _pre(self, b, src, noise: bool = False) -> None:
        """What runs eagerly on the slot's stream in front of the graph: for readouts (submit_readouts) the gating into the slot's raw
        buffer; with ``noise`` the replica's noise on the raw data (_launch; setting up a set runs without); with a coil matrix, the
        compression of this scan's raw data (any coil count) into the static (T, x, y, V) buffer the graph starts from; with
        virtual_coils= the Gram matrix and the matrix of this slice in front of it (with whitener= the whitened matrix, from the
        copied whitener)."""
        if src.raw is not None and src.gate is not None:
            from . import gating
            gating.gate_into(*src.gate_views(b), src.gate[2].n_lines, src.raw_view(b))
        if noise and src.noise is not None and src.raw is not None:          # a raw replica: in place on the slot's raw data, in front of the rest
            from . import noise as N
            ns = src.noise
            rv = src.raw_view(b)
            N.add_noise_raw(rv, ns.chol, noise_mask=None if src.nmask is None else src.nmask_view(b), scale=ns.scale, seed=ns.seed,
                            replica=ns.replica, out=rv)
        if src.raw is not None and src.v is not None:
            with torch.no_grad():
                if src.vc is not None:                       # this slice's own matrix, where coil_matrix= has the copied one
                    c = src.c
                    g = frontend.coil_gram(src.raw_view(b), src.n, src.cc_region, out=b["gram"][:c * c].view(c, c), ws=b["gws"])
                    frontend._coil_matrix_jacobi(g[None], src.vc, src.cmat_view(b)[None], b["lam"][:c][None], b["cinfo"],
                                                 whitener=None if src.wh is None else src.wh_view(b))
                frontend.compress_coils(src.raw_view(b), torch.view_as_complex(src.cmat_view(b)), src.n, out=b["cc"])

    def _body(self, b):
        """The slice's launch sequence on the current stream, the part a graph holds: the front-end of a raw set, the model's forward
        (+ the zero-filled image)."""
        r = self._set.raw
        if r is not None:
            with torch.no_grad():
                frontend.prepare_masked_slice(b["front"], b["mask"], r.crop, r.n, r.filter, r.scaling, None, r.apply_mask, out=b["mk"])
        e = self._set.espirit
        if e is not None:
            with torch.no_grad():
                for i in range(b["mk"].shape[0]):
                    maps, _, resid = frontend.espirit_maps(frontend.time_average(b["mk"][i]), r=e[1], k=e[2], thresh=e[3], crop=e[4],
                                                           method="sign", sign_iters=e[5], return_residual=True)
                    b["sens"][i, 0].copy_(maps)
                    b["resid"][i:i + 1].copy_(resid)
        return self._run(b)

    def _raw_memory(self, nbytes: int) -> None:
        """2 x slots raw buffers of nbytes each have to fit into the free memory the driver reports: no silent fallback."""
        need = 2 * self.slots * nbytes
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > free:
            raise CineHipError(f"SlicePipeline: {2 * self.slots} raw buffers of {nbytes} bytes need {need} bytes, {free} are free on "
                               f"{self.device}; slots={int(free // (2 * nbytes))} would fit")

    def _grow_raw(self, nbytes: int, gram_bytes: int = 0) -> None:
        """Larger raw byte buffers (and Gram workspaces) for every (slot, parity).  Only a set with a coil matrix or virtual_coils= gets
        here: its graphs start from the compressed buffer, so nothing has to be captured again."""
        self._retire_all()
        st = self._set
        for b in st.bufs.values():
            b["raw"] = None
            if gram_bytes:
                b["gws"] = None
        self._raw_memory(nbytes + gram_bytes)
        try:
            for b in st.bufs.values():
                b["raw"] = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
                if gram_bytes:
                    b["gws"] = torch.empty(gram_bytes, device=self.device, dtype=torch.uint8)
        except Exception as e:
            self._set = None
            raise CineHipError(f"SlicePipeline: allocating raw buffers of {nbytes} bytes failed: {type(e).__name__}: {e}") from e
        st.raw_bytes, st.gram_bytes = nbytes, gram_bytes
        self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))        # as in _build: new memory of the caller's stream

    def _grow_gate(self, line_bytes: int, entries: int, rows1: int) -> None:
        """Gating buffers for every (slot, parity): readouts, row_ptr (rows1 = n_frames * nx + 1), index, weight.  No graph holds them
        (the gate runs in front of the replay), so like _grow_raw this drains and allocates, and nothing is captured again."""
        self._retire_all()
        st = self._set
        for b in st.bufs.values():
            b["lines"] = b["rptr"] = b["gidx"] = b["gw"] = None
        self._raw_memory(line_bytes + 4 * rows1 + 8 * entries)
        try:
            for b in st.bufs.values():
                b["lines"] = torch.empty(line_bytes, device=self.device, dtype=torch.uint8)
                b["rptr"] = torch.empty(rows1, device=self.device, dtype=torch.int32)
                b["gidx"] = torch.empty(entries, device=self.device, dtype=torch.int32)
                b["gw"] = torch.empty(entries, device=self.device, dtype=torch.float32)
        except Exception as e:
            self._set = None
            raise CineHipError(f"SlicePipeline: allocating gating buffers of {line_bytes} bytes failed: {type(e).__name__}: {e}") from e
        st.gate_cap = (line_bytes, entries)
        self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))        # as in _build: new memory of the caller's stream

    def _build(self, src) -> _Set:
        """Buffers for every (slot, parity), filled with this slice's inputs; with graphs, one eager forward per slot stream
        (per-stream caches are filled outside capture) and one capture per buffer set."""
        S, dev = self.slots, self.device
        self._builds += 1
        st = _Set(src.key)
        try:
            if src.raw is not None:
                self._raw_memory(src.raw_nbytes + src.gram_bytes())
                st.raw, st.raw_bytes = _settings_only(src), src.raw_nbytes     # the settings, not the first slice's data
                st.gram_bytes = src.gram_bytes()
            st.espirit = src.espirit
            for i in range(S):
                for p in (0, 1):
                    st.bufs[(i, p)] = src.alloc(self)
                    st.ready[(i, p)] = torch.cuda.Event()
                    st.done[(i, p)] = torch.cuda.Event()
            self._set = st
            if src.raw is not None and src.gate is not None:
                self._grow_gate(*_gate_capacity(src))
            # the new buffers come from the pool of the caller's stream: whatever that stream still has to run on the memory they
            # took over (an eager forward just before the first submit) goes first
            self.copy_stream.wait_stream(torch.cuda.current_stream(dev))
            self._copy_in(src, (0, 0), wait_done=False)
            with torch.cuda.stream(self.copy_stream):
                b0 = st.bufs[(0, 0)]
                for key, b in st.bufs.items():
                    if key != (0, 0):
                        for name in src.input_names:
                            if b[name] is not None and not (name == "sens" and src.espirit is not None):
                                b[name].copy_(b0[name])
            self.copy_stream.synchronize()
            if self.graphs:
                for i in range(S):
                    s = self.streams[i]
                    s.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(s):
                        for p in (0, 1):
                            self._pre(st.bufs[(i, p)], src)
                        self._body(st.bufs[(i, 0)])                # warm this stream's caches outside capture
                    s.synchronize()
                    for p in (0, 1):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, stream=s):
                            o = self._body(st.bufs[(i, p)])
                        st.graphs[(i, p)] = (g, o)
                torch.cuda.synchronize(dev)
        except CineHipError:
            self._set = None
            raise
        except Exception as e:
            self._set = None
            raise CineHipError(f"SlicePipeline: setting up {type(self.model).__name__} for inputs {src.key} failed: {type(e).__name__}: {e}") from e
        return st

    def _staging(self, items):
        """The next of the two pinned staging sets for pageable inputs (waits until the copy out of it has finished): a view of the
        destination's shape for every pageable item."""
        st = self._set
        if st.stage is None:
            st.stage = [{}, {}]
            st.stage_ev = [None, None]
        r = st.stage_next
        st.stage_next ^= 1
        if st.stage_ev[r] is not None:
            st.stage_ev[r].synchronize()
        views = {}
        for name, dst, _, kind in items:
            if kind == "pageable":
                nbytes = dst.numel() * dst.element_size()
                buf = st.stage[r].get(name)
                if buf is None or buf.numel() < nbytes:
                    buf = st.stage[r][name] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                views[name] = buf[:nbytes].view(dst.dtype).view(dst.shape)
        return r, views

    def _copy_in(self, src, key, wait_done: bool):
        """The slice's inputs into buffer set `key` on the copy stream, after the set's previous reader; records the set's
        ready-event.  Returns what has to stay alive until the slice is done."""
        st = self._set
        cs = self.copy_stream
        keep = []
        b = st.bufs[key]
        if getattr(src, "nmask", None) is not None and b.get("nmask") is None:
            # the mask of a raw replica: no graph holds it, so the buffer is made when a slot first needs one; like the set's other
            # buffers it comes from the pool of the caller's stream
            b["nmask"] = torch.empty(src.nmask_nbytes, device=self.device, dtype=torch.uint8)
            cs.wait_stream(torch.cuda.current_stream(self.device))
        items = src.items(b)
        stage = None
        if any(kind == "pageable" for _, _, _, kind in items):
            r, stage = self._staging(items)
            for name, _, x, kind in items:
                if kind == "pageable":
                    stage[name].copy_(x)                           # the host memcpy of a pageable input
        if any(kind == "device" for _, _, _, kind in items):
            cs.wait_stream(torch.cuda.current_stream(self.device))
        if wait_done:
            cs.wait_event(st.done[key])
        with torch.cuda.stream(cs):
            for name, dst, x, kind in items:
                if kind == "pageable":
                    dst.copy_(stage[name], non_blocking=True)
                elif kind == "device":
                    dst.copy_(x.expand(dst.shape) if name in ("mask", "nmask") else x, non_blocking=True)
                    x.record_stream(cs)
                    keep.append(x)
                else:
                    dst.copy_(x, non_blocking=True)
                    keep.append(x)
            st.ready[key].record(cs)
            if stage is not None:
                ev = torch.cuda.Event()
                ev.record(cs)
                st.stage_ev[r] = ev
        return keep

    def _launch(self, key, src):
        """Slice on set `key`: on the slot's stream, wait for its inputs, replay (or launch), copy the outputs out, record done."""
        st = self._set
        s = self.streams[key[0]]
        with torch.cuda.stream(s):
            s.wait_event(st.ready[key])
            self._pre(st.bufs[key], src, noise=True)
            if src.noise is not None and src.raw is None:                    # a pseudo replica: in place on the slot's k-space, in front of the replay
                from . import noise as N
                b, ns = st.bufs[key], src.noise
                N.add_noise(b["mk"], b["mask"], ns.chol, scale=ns.scale, seed=ns.seed, replica=ns.replica, out=b["mk"])
            if self.graphs:
                g, static = st.graphs[key]
                g.replay()
                if self.out == "host":
                    outs = tuple(torch.empty(o.shape, dtype=o.dtype, pin_memory=True).copy_(o, non_blocking=True) for o in static)
                else:
                    outs = tuple(torch.empty_like(o).copy_(o, non_blocking=True) for o in static)
            else:
                try:
                    outs = self._body(st.bufs[key])
                except CineHipError:
                    raise
                except Exception as e:
                    raise CineHipError(f"SlicePipeline: eager forward failed: {type(e).__name__}: {e}") from e
                if self.out == "host":
                    outs = tuple(torch.empty(o.shape, dtype=o.dtype, pin_memory=True).copy_(o, non_blocking=True) for o in outs)
            resid = None
            if st.espirit is not None:          # with the outputs, on the slot's stream: read by results() once the slice is done
                resid = torch.empty(st.bufs[key]["resid"].shape, dtype=torch.float64, pin_memory=True).copy_(st.bufs[key]["resid"], non_blocking=True)
            cinfo = None
            if src.raw is not None and src.vc is not None:      # the eigensolver's record of this slice, the same way
                cinfo = torch.empty(st.bufs[key]["cinfo"].shape, dtype=torch.float64, pin_memory=True).copy_(st.bufs[key]["cinfo"], non_blocking=True)
            st.done[key].record(s)
        return outs, resid, cinfo
