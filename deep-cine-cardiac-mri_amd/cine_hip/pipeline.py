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

The model is called as ``model(mk, mask)`` or ``model(mk, mask, sens)``, without ``acs=``: the ACS window is found on the
device (``ops.acs_window_dev``) and a graph captured with one slice's mask gives any other slice's result.  That window is
read from row masks only; a mask that varies along w with a model that runs its sensitivity network raises ``CineHipError``.

Outputs (``results`` / ``drain``): ``(tag, out)`` in submission order; ``out`` is ``recon`` or, with ``zero_filled=True``,
``(recon, zero_filled)`` (reference run_inference.py:64-67, computed inside the same graph by ``cine_zero_filled_rss``).
They are fresh device tensors (``out="device"``, marked as used on the stream that is current when they are handed out) or
pinned host tensors (``out="host"``); no later replay writes to them.

Shapes: the graphs, buffers and events form one SET keyed by the input shapes and dtypes.  Only one set is alive: a submit
with a new key drains the pending slices (their results stay queued), frees the old set and builds a new one (one eager
forward per slot stream, then two captures per slot).

``graphs=False`` is the explicit eager mode: same slots, streams, buffers, copies and events, with the launch sequence
enqueued on the slot's stream for every slice.  A failure raises ``CineHipError``; nothing falls back to eager launches.

Not thread-safe: one pipeline is driven from one thread.  One pipeline per GPU (``device=``) for several GPUs.
"""
import collections
import inspect
from typing import Optional

import numpy as np
import torch

from . import ops
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


class _Source:
    """One slice's validated inputs: torch views in their original place, the canonical mask, the set key."""

    def __init__(self, pipe, masked_kspace, mask, sens_maps):
        mk, self.mk_kind = _pairs(masked_kspace, "masked_kspace")
        if mk.dim() != 6:
            raise CineHipError(f"masked_kspace: shape {tuple(mk.shape)}; expected (b, t, c, h, w, 2) or complex (b, t, c, h, w)")
        self.mk = mk
        b, t, c, h, w, _ = mk.shape
        if isinstance(mask, np.ndarray):
            mask = torch.from_numpy(mask)
        if not isinstance(mask, torch.Tensor):
            raise CineHipError(f"mask: expected a torch tensor or a numpy array, got {type(mask).__name__}")
        want = _mask_shape(mask.shape, mk.shape)
        if mask.is_cuda:
            if mask.dtype not in (torch.uint8, torch.bool):
                raise CineHipError(f"mask: a device mask must be uint8 or bool (got {mask.dtype}); pass other dtypes from the host")
            self.mask, self.mask_kind = mask, "device"
        else:
            m = mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)
            m = m.expand(want)
            canonical = m.is_contiguous() and m.is_pinned()
            self.mask, self.mask_kind = (m, "pinned") if canonical else (m.contiguous(), "pageable")
        self.mask_shape = want
        general = want[4] > 1
        self.sens, self.sens_kind = None, None
        if sens_maps is not None:
            if not pipe._takes_sens:
                raise CineHipError(f"{type(pipe.model).__name__} takes no sens_maps")
            s, self.sens_kind = _pairs(sens_maps, "sens_maps")
            if tuple(s.shape) != (b, 1, c, h, w, 2):
                raise CineHipError(f"sens_maps: shape {tuple(s.shape)}; expected {(b, 1, c, h, w, 2)} for this k-space")
            self.sens = s
        elif pipe._needs_sens:
            raise CineHipError(f"{type(pipe.model).__name__} needs sens_maps")
        elif general:
            raise CineHipError("the mask varies along w: the ACS window of the sensitivity network is found on the device from row masks "
                               "only; pass sens_maps (VarNet) or use a row mask (b|1, t|1, 1, h, 1, 1)")
        for name, x in (("masked_kspace", self.mk), ("mask", self.mask), ("sens_maps", self.sens)):
            if x is not None and x.is_cuda and x.device != pipe.device:
                raise CineHipError(f"{name} is on {x.device}, the pipeline's device is {pipe.device}")
        self.key = (tuple(mk.shape), want, None if self.sens is None else tuple(self.sens.shape))


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
        self.bufs = {}          # (slot, parity) -> {"mk", "mask", "sens"}
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
        self._recs = {}           # index -> [handle, outputs, inputs kept alive until the slice is done]
        self._set = None
        self._closed = False
        self.streams, self.copy_stream = pipeline_streams(device, slots)

    # ---- public ----------------------------------------------------------------------------------------------------------
    def submit(self, masked_kspace, mask, sens_maps=None, tag=None) -> SliceHandle:
        """Enqueue one slice.  Returns at once, unless 2 x slots slices are pending: then it waits for the oldest one."""
        if self._closed:
            raise CineHipError("SlicePipeline: submit after close()")
        src = _Source(self, masked_kspace, mask, sens_maps)
        with torch.cuda.device(self.device):
            if self._set is None or self._set.key != src.key:
                self._retire_all()
                self._set = None                               # one set alive: the old graphs and buffers go first
                self._sched.new_buffers()
                self._set = self._build(src)
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
                outs = self._launch(key)
            except Exception:
                self._recs[step.index] = [h, None, None]
                raise
            self._recs[step.index] = [h, outs, keep]
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
            h, outs, _ = self._recs.pop(k)
            if outs is None:
                continue                  # a submit that raised: nothing was launched for it
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

    def _build(self, src: _Source) -> _Set:
        """Buffers for every (slot, parity), filled with this slice's inputs; with graphs, one eager forward per slot stream
        (per-stream caches are filled outside capture) and one capture per buffer set."""
        S, dev = self.slots, self.device
        st = _Set(src.key)
        try:
            for i in range(S):
                for p in (0, 1):
                    st.bufs[(i, p)] = {"mk": torch.empty(src.mk.shape, device=dev, dtype=torch.float32),
                                       "mask": torch.empty(src.mask_shape, device=dev, dtype=torch.uint8),
                                       "sens": None if src.sens is None else torch.empty(src.sens.shape, device=dev, dtype=torch.float32)}
                    st.ready[(i, p)] = torch.cuda.Event()
                    st.done[(i, p)] = torch.cuda.Event()
            self._set = st
            self._copy_in(src, (0, 0), wait_done=False)
            with torch.cuda.stream(self.copy_stream):
                b0 = st.bufs[(0, 0)]
                for key, b in st.bufs.items():
                    if key != (0, 0):
                        for name in ("mk", "mask", "sens"):
                            if b[name] is not None:
                                b[name].copy_(b0[name])
            self.copy_stream.synchronize()
            if self.graphs:
                for i in range(S):
                    s = self.streams[i]
                    s.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(s):
                        self._run(st.bufs[(i, 0)])                 # warm this stream's caches outside capture
                    s.synchronize()
                    for p in (0, 1):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, stream=s):
                            o = self._run(st.bufs[(i, p)])
                        st.graphs[(i, p)] = (g, o)
                torch.cuda.synchronize(dev)
        except CineHipError:
            self._set = None
            raise
        except Exception as e:
            self._set = None
            raise CineHipError(f"SlicePipeline: setting up {type(self.model).__name__} for inputs {src.key} failed: {type(e).__name__}: {e}") from e
        return st

    def _staging(self, src: _Source):
        """The next of the two pinned staging sets for pageable inputs (waits until the copy out of it has finished)."""
        st = self._set
        if st.stage is None:
            def pinned(shape, dtype):
                return torch.empty(shape, dtype=dtype, pin_memory=True)
            st.stage = [{"mk": pinned(src.mk.shape, torch.float32), "mask": pinned(src.mask_shape, torch.uint8),
                         "sens": None if src.sens is None else pinned(src.sens.shape, torch.float32)} for _ in range(2)]
            st.stage_ev = [None, None]
        r = st.stage_next
        st.stage_next ^= 1
        if st.stage_ev[r] is not None:
            st.stage_ev[r].synchronize()
        return r, st.stage[r]

    def _copy_in(self, src: _Source, key, wait_done: bool):
        """The slice's inputs into buffer set `key` on the copy stream, after the set's previous reader; records the set's
        ready-event.  Returns what has to stay alive until the slice is done."""
        st = self._set
        b = st.bufs[key]
        cs = self.copy_stream
        keep = []
        items = [("mk", src.mk, src.mk_kind), ("mask", src.mask, src.mask_kind)]
        if src.sens is not None:
            items.append(("sens", src.sens, src.sens_kind))
        stage = None
        if any(kind == "pageable" for _, _, kind in items):
            r, stage = self._staging(src)
            for name, x, kind in items:
                if kind == "pageable":
                    stage[name].copy_(x)                           # the host memcpy of a pageable input
        if any(kind == "device" for _, _, kind in items):
            cs.wait_stream(torch.cuda.current_stream(self.device))
        if wait_done:
            cs.wait_event(st.done[key])
        with torch.cuda.stream(cs):
            for name, x, kind in items:
                if kind == "pageable":
                    b[name].copy_(stage[name], non_blocking=True)
                elif kind == "device":
                    b[name].copy_(x.expand(b[name].shape) if name == "mask" else x, non_blocking=True)
                    x.record_stream(cs)
                    keep.append(x)
                else:
                    b[name].copy_(x, non_blocking=True)
                    keep.append(x)
            st.ready[key].record(cs)
            if stage is not None:
                ev = torch.cuda.Event()
                ev.record(cs)
                st.stage_ev[r] = ev
        return keep

    def _launch(self, key):
        """Slice on set `key`: on the slot's stream, wait for its inputs, replay (or launch), copy the outputs out, record done."""
        st = self._set
        s = self.streams[key[0]]
        with torch.cuda.stream(s):
            s.wait_event(st.ready[key])
            if self.graphs:
                g, static = st.graphs[key]
                g.replay()
                if self.out == "host":
                    outs = tuple(torch.empty(o.shape, dtype=o.dtype, pin_memory=True).copy_(o, non_blocking=True) for o in static)
                else:
                    outs = tuple(torch.empty_like(o).copy_(o, non_blocking=True) for o in static)
            else:
                try:
                    outs = self._run(st.bufs[key])
                except CineHipError:
                    raise
                except Exception as e:
                    raise CineHipError(f"SlicePipeline: eager forward failed: {type(e).__name__}: {e}") from e
                if self.out == "host":
                    outs = tuple(torch.empty(o.shape, dtype=o.dtype, pin_memory=True).copy_(o, non_blocking=True) for o in outs)
            st.done[key].record(s)
        return outs
