"""The packed-weight cache (cine_hip.ops.PackCache) on host tensors with a fake builder, and the table of pack kinds (ops._KINDS) against
include/cine_hip.h.  No GPU and no library call: the capture query of ops (``_capturing``), which needs a device, is substituted."""
import gc
import re
import weakref

import pytest
import torch

from cine_hip import _lib, ops
from cine_hip._lib import CineHipError

HEADER = open(_lib.HEADER_PATH).read()


class Builder:
    """Returns a fresh tensor per call as (tensors to keep, value) and counts the calls."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        t = torch.full((4,), float(self.calls))
        return [t], t


@pytest.fixture
def capture(monkeypatch):
    state = {"on": False}
    monkeypatch.setattr(ops, "_capturing", lambda: state["on"])
    return state


def test_builder_runs_once_per_miss_and_never_on_a_hit(capture):
    p, q = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    cache, build = ops.PackCache("fake packs"), Builder()
    first = cache.get([p, q], build)
    assert build.calls == 1 and cache.fills == 1
    for _ in range(3):
        assert cache.get([p, q], build) is first
    assert build.calls == 1 and cache.fills == 1


def test_misses_on_inplace_update_moved_parameter_and_moved_epoch(capture, monkeypatch):
    p, q = torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))
    cache, build = ops.PackCache("fake packs"), Builder()
    seen = [cache.get([p, q], build)]

    def miss():
        v = cache.get([p, q], build)
        assert all(v is not s for s in seen) and cache.get([p, q], build) is v
        seen.append(v)
        assert build.calls == len(seen) == cache.fills
    p.mul_(2.0)                                    # in place: Tensor._version moves
    miss()
    q.data = torch.zeros(2)                        # moved: another address (the version stays)
    miss()
    monkeypatch.setattr(ops, "_cache_epoch", ops.cache_epoch() + 1)     # what the end of a training_capture() does
    miss()


def test_a_miss_during_capture_raises_and_builds_nothing(capture):
    p = torch.nn.Parameter(torch.ones(3))
    cache, build = ops.PackCache("fake packs"), Builder()
    capture["on"] = True
    with pytest.raises(CineHipError, match="fake packs would be created during hipGraph capture"):
        cache.get([p], build)
    assert build.calls == 0 and cache.fills == 0
    capture["on"] = False
    v = cache.get([p], build)
    capture["on"] = True
    assert cache.get([p], build) is v              # a hit is served under capture
    p.mul_(2.0)
    with pytest.raises(CineHipError):
        cache.get([p], build)
    assert build.calls == 1


def _superseded(captured_in_between: bool, capture):
    """Fill, (hand the value out under capture,) update the parameter in place, fill again: a weak reference to the first fill's tensor."""
    p = torch.nn.Parameter(torch.ones(3))
    cache, build = ops.PackCache("fake packs"), Builder()
    ref = weakref.ref(cache.get([p], build))
    if captured_in_between:
        capture["on"] = True
        cache.get([p], build)
        capture["on"] = False
    p.mul_(2.0)
    cache.get([p], build)
    gc.collect()
    assert build.calls == 2
    return cache, ref


def test_a_value_handed_out_under_capture_survives_the_next_miss_until_release_old(capture):
    cache, ref = _superseded(True, capture)
    assert ref() is not None and float(ref()[0]) == 1.0     # a graph captured then still reads it
    cache.release_old()
    gc.collect()
    assert ref() is None


def test_without_a_capture_the_superseded_tensors_are_dropped(capture):
    _, ref = _superseded(False, capture)
    assert ref() is None


def test_copies_start_empty(capture):
    import copy
    p = torch.nn.Parameter(torch.ones(3))
    cache, build = ops.PackCache("fake packs"), Builder()
    cache.get([p], build)
    twin = copy.deepcopy(cache)
    assert twin.what == "fake packs" and twin.fills == 0
    twin.get([p], build)
    assert build.calls == 2


# ------------------------------------------------------------------ the table of pack kinds
def test_every_kind_names_two_entries_of_the_header():
    sigs = _lib.parse_header(HEADER)
    assert sorted(ops._KINDS) == sorted(["c3", "tc", "c1", "c27", "tc3", "c3d", "tcd", "c1d"])
    for name, k in ops._KINDS.items():
        assert k.floats_fn in sigs and k.pack_fn in sigs, name
        assert k.floats_fn.endswith("_packed_floats") and k.pack_fn.startswith("cine_pack_")
    packs = [k.pack_fn for k in ops._KINDS.values()]
    assert len(set(packs)) == len(packs)


def test_op_numbers_are_those_of_the_header_comment():
    comment = re.search(r"/\*((?:(?!\*/).)*)\*/\s*size_t cine_pack_desc_bytes", HEADER, flags=re.S).group(1)
    documented = {fn: int(op) for op, fn in re.findall(r"\b(\d) = (cine_pack_[a-z0-9_]+)", comment)}
    assert sorted(documented.values()) == [0, 1, 2, 3, 4, 5]
    table = {k.pack_fn: k.op for k in ops._KINDS.values() if k.op is not None}
    assert table == documented
    assert len(set(table.values())) == len(table)
    assert [k.op for k in ops._KINDS.values() if k.op is not None] == [0, 1, 2, 3, 4, 5]      # rows in the header's order
    assert ops._KINDS["c27"].op is None and ops._KINDS["tc3"].op is None


def test_leading_dimensions_are_in_the_order_of_the_prototypes():
    for name, k in ops._KINDS.items():
        for fn, lead in ((k.pack_fn, 2), (k.floats_fn, 0)):
            args = re.search(r"\b%s\(([^)]*)\)" % fn, HEADER).group(1).split(",")
            names = tuple(a.split()[-1].lstrip("*") for a in args[lead:lead + 2])
            assert names == k.dims, (name, fn, names)
