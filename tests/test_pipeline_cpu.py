"""SlicePipeline without a GPU: the slot / parity / event schedule, the ordering of results, and argument checks."""
import random

import numpy as np
import pytest
import torch

from cine_hip._lib import CineHipError
from cine_hip.pipeline import SlicePipeline, SliceSchedule, _forward_params, _mask_shape, _pairs, _Source


def _run(S, N, finish_order_seed=None):
    """Drive a schedule the way SlicePipeline does: retire the oldest slice when full, then submit.  Returns the steps and,
    per step, the set of slices retired before its copy was issued."""
    sch = SliceSchedule(S)
    steps, retired_before = [], []
    retired = set()
    for _ in range(N):
        k0 = sch.must_retire()
        if k0 is not None:
            assert sch.retire_oldest() == k0
            retired.add(k0)
        steps.append(sch.submit())
        retired_before.append(set(retired))
        if finish_order_seed is not None and random.Random(finish_order_seed + len(steps)).random() < 0.3 and sch.inflight:
            retired.add(sch.retire_oldest())
    return sch, steps, retired_before


@pytest.mark.parametrize("S", [1, 2, 3, 7, 10])
def test_slice_k_goes_to_slot_k_mod_S_with_parity(S):
    _, steps, _ = _run(S, 5 * S + 3)
    for k, st in enumerate(steps):
        assert st.index == k
        assert st.slot == k % S
        assert st.parity == (k // S) & 1


@pytest.mark.parametrize("S", [1, 3, 10])
def test_copy_waits_for_the_previous_reader_of_its_buffer_set(S):
    _, steps, retired_before = _run(S, 6 * S + 1, finish_order_seed=S)
    last = {}
    for st, retired in zip(steps, retired_before):
        prev = last.get((st.slot, st.parity))
        assert st.copy_after == prev                       # the copy is ordered after the set's previous reader's done-event ...
        if prev is not None:
            assert prev == st.index - 2 * S
            assert prev in retired                         # ... which the host has already seen finish: the copy stream never waits on a replay in flight
        last[(st.slot, st.parity)] = st.index


@pytest.mark.parametrize("S", [1, 3, 4])
def test_at_most_two_rounds_in_flight(S):
    sch = SliceSchedule(S)
    for _ in range(2 * S):
        assert sch.must_retire() is None
        sch.submit()
    assert sch.must_retire() == 0
    with pytest.raises(RuntimeError):
        sch.submit()
    sch.retire_oldest()
    assert sch.submit().index == 2 * S


@pytest.mark.parametrize("S,N", [(3, 7), (4, 10), (10, 23), (1, 5)])
def test_results_in_submission_order(S, N):
    """GPU events finish in any order across slots; results are handed out in submission order (N not a multiple of S)."""
    rng = random.Random(N)
    sch = SliceSchedule(S)
    finished_on_gpu = set()
    out = []

    def collect(block):
        while True:
            k = sch.take_finished()
            if k is None:
                if not sch.inflight:
                    return
                if block or sch.inflight[0] in finished_on_gpu:
                    sch.retire_oldest()
                    continue
                return
            out.append(k)

    for _ in range(N):
        if sch.must_retire() is not None:
            sch.retire_oldest()
        sch.submit()
        for k in list(sch.inflight):
            if rng.random() < 0.5:
                finished_on_gpu.add(k)
        collect(block=False)
    collect(block=True)
    assert out == list(range(N))
    assert sch.pending() == 0


def test_new_buffers_only_when_drained():
    sch = SliceSchedule(2)
    sch.submit()
    with pytest.raises(RuntimeError):
        sch.new_buffers()
    sch.retire_oldest()
    sch.new_buffers()
    st = sch.submit()
    assert st.index == 1 and st.copy_after is None
    for _ in range(3):
        sch.submit()
    assert sch.inflight[-1] == 4
    sch.retire_oldest()
    assert sch.submit().copy_after == 1                   # first use after the new buffers: set (1, 0) -> slice 1, then slice 5


@pytest.mark.parametrize("bad", [0, -1, 1.5, True, "3", None])
def test_schedule_rejects_bad_slot_counts(bad):
    with pytest.raises(ValueError):
        SliceSchedule(bad)


def _tiny_varnet():
    import reconstruction.models as M
    return M.VarNet(1, 4, 2, 4, 2, "XF")


@pytest.mark.parametrize("kw", [dict(slots=0), dict(slots=32), dict(slots=2.0), dict(slots=True), dict(out="disk"), dict(out=None)])
def test_pipeline_rejects_bad_arguments(kw):
    with pytest.raises(CineHipError):
        SlicePipeline(_tiny_varnet().eval(), **kw)


def test_pipeline_rejects_training_mode_and_non_modules():
    with pytest.raises(CineHipError, match="training"):
        SlicePipeline(_tiny_varnet().train())
    with pytest.raises(CineHipError):
        SlicePipeline(lambda mk, mask: mk)


def test_sens_maps_arguments_of_every_model():
    import reconstruction.models as M
    assert _forward_params(M.VarNet(1, 4, 2, 4, 2, "XF")) == (True, False)
    assert _forward_params(M.CineNet(1, 2, 4, 2, "3D")) == (True, True)
    assert _forward_params(M.CineNet_RNN(1, 2, 4)) == (True, True)
    assert _forward_params(M.VarNet_RNN(1, 4, 2, 4)) == (False, False)
    xpd = M.XPDNet(num_cascades=1, sens_chans=4, sens_pools=2, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[1, 1],
                   first_conv_n_filters=8, n_primal=2, dynamic_type="XT")
    assert _forward_params(xpd) == (False, False)


def test_input_forms():
    c = (np.random.RandomState(0).standard_normal((1, 3, 2, 8, 6)) + 1j).astype(np.complex64)
    x, kind = _pairs(c, "k")
    assert kind == "pageable" and x.dtype == torch.float32 and tuple(x.shape) == (1, 3, 2, 8, 6, 2)
    assert np.array_equal(x[..., 0].numpy(), c.real) and np.array_equal(x[..., 1].numpy(), c.imag)
    x, kind = _pairs(torch.from_numpy(c), "k")
    assert kind == "pageable" and tuple(x.shape) == (1, 3, 2, 8, 6, 2)
    x, kind = _pairs(torch.zeros(1, 3, 2, 8, 6, 2), "k")
    assert kind == "pageable"
    for bad in (np.zeros((1, 3, 2, 8, 6, 2)), torch.zeros(1, 3, 2, 8, 6, 3), torch.zeros(4, dtype=torch.int32), [1.0, 2.0]):
        with pytest.raises(CineHipError):
            _pairs(bad, "k")


def test_mask_shapes():
    ks = (2, 3, 4, 8, 6, 2)
    assert _mask_shape((1, 1, 1, 8, 1, 1), ks) == (2, 3, 1, 8, 1, 1)
    assert _mask_shape((2, 3, 1, 8, 6, 1), ks) == (2, 3, 1, 8, 6, 1)
    for bad in ((1, 1, 1, 7, 1, 1), (3, 1, 1, 8, 1, 1), (1, 1, 1, 8, 5, 1), (1, 1, 8, 1, 1), (1, 1, 2, 8, 1, 1)):
        with pytest.raises(CineHipError):
            _mask_shape(bad, ks)


class _Stand:
    """The attributes of a SlicePipeline that input validation reads."""

    def __init__(self, model, takes, needs):
        self.model, self._takes_sens, self._needs_sens, self.device = model, takes, needs, torch.device("cuda", 0)


def test_source_validation():
    mk = torch.zeros(1, 3, 2, 8, 6, 2)
    row = torch.zeros(1, 3, 1, 8, 1, 1, dtype=torch.uint8)
    general = torch.zeros(1, 3, 1, 8, 6, 1)
    sens = torch.zeros(1, 1, 2, 8, 6, 2)
    varnet, cinenet, xpd = _Stand("VarNet", True, False), _Stand("CineNet", True, True), _Stand("XPDNet", False, False)
    src = _Source(varnet, mk, row.float() * 3, None)                      # float host masks are converted on the host, like as_mask_u8
    assert src.mask.dtype == torch.uint8 and src.mask_kind == "pageable" and src.key == ((1, 3, 2, 8, 6, 2), (1, 3, 1, 8, 1, 1), None)
    src = _Source(varnet, mk, torch.ones(1, 1, 1, 8, 1, 1), None)
    assert tuple(src.mask.shape) == (1, 3, 1, 8, 1, 1) and int(src.mask.sum()) == 24
    with pytest.raises(CineHipError, match="varies along w"):
        _Source(varnet, mk, general, None)                                 # the sensitivity network would need a host read of the mask
    with pytest.raises(CineHipError, match="varies along w"):
        _Source(xpd, mk, general, None)
    assert _Source(varnet, mk, general, sens).mask_shape == (1, 3, 1, 8, 6, 1)
    assert _Source(cinenet, mk, general, sens).key[2] == (1, 1, 2, 8, 6, 2)
    with pytest.raises(CineHipError, match="needs sens_maps"):
        _Source(cinenet, mk, row, None)
    with pytest.raises(CineHipError, match="takes no sens_maps"):
        _Source(xpd, mk, row, sens)
    with pytest.raises(CineHipError, match="sens_maps: shape"):
        _Source(varnet, mk, row, torch.zeros(1, 1, 3, 8, 6, 2))
    with pytest.raises(CineHipError, match="masked_kspace: shape"):
        _Source(varnet, mk[0], row, None)
    with pytest.raises(CineHipError):
        _Source(varnet, mk, "mask", None)
