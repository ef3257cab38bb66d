"""SlicePipeline.submit_raw(..., whitener=W): noise pre-whitening in flight, folded into every slice's own compression matrix.

The identity under test: the pipeline's output is, bit for bit, ``model(prepare_masked_slice(raw, mask, ..., coil_matrix=A), mask)`` with
``A = coil_matrix_from_gram(coil_gram(raw, n_frames, region), V, method="jacobi", whitener=W)[0]`` -- the public pieces, run one after
the other.  Shapes, model and raw data are those of tests/test_raw_pipeline_virtual_coils.py; the whiteners are those of the designed
covariances of tests/whitening_ref.py (condition number 100)."""
import numpy as np
import pytest
import torch

from test_raw_pipeline_virtual_coils import CROP, FRAMES, FS, RAW, V, _raw, _row_mask, _same
from whitening_ref import designed_cov, whitener_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    import reconstruction.models as M
    from cine_hip import synth
    n = M.VarNet_RNN(2, 4, 2, 6)
    synth.fill_parameters_(n, 9, keep=("lambda",))
    return n.to(dev).eval()


def _whitener(c, seed=5):
    """W (c, c) complex128 on the host, float64 numpy."""
    return torch.from_numpy(whitener_ref(designed_cov(c, seed))[0])


def _matrix(raw, w, dev, v=V, region=24):
    from cine_hip import frontend as FE
    return FE.coil_matrix_from_gram(FE.coil_gram(raw.to(dev), FRAMES, region), v, method="jacobi", whitener=w.to(dev))[0]


def _sequential(net, raw, mask, w, dev, v=V):
    from cine_hip import frontend as FE
    with torch.no_grad():
        mk = FE.prepare_masked_slice(raw.to(dev), mask.to(dev), CROP, FRAMES, FS, 1e6, coil_matrix=_matrix(raw, w, dev, v))
        return net(mk, mask.to(dev)).clone()


@pytest.fixture(scope="module")
def scans(net, dev):
    """13 slices of 12 coils (4 S + 1 for S = 3), one whitener, and their sequential forwards, computed once."""
    raws = [_raw(12, 100 + j) for j in range(13)]
    masks = [_row_mask(j) for j in range(13)]
    w = _whitener(12)
    want = [_sequential(net, r, m, w, dev) for r, m in zip(raws, masks)]
    assert all(bool(torch.isfinite(x).all()) for x in want) and not torch.equal(want[0], want[1])
    return raws, masks, w, want


# ------------------------------------------------------------------ 1. the identity, with graphs and without, S = 1 and S = 3
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("S", [1, 3])
def test_submit_raw_whitened_matches_the_sequential_forward(net, scans, dev, S, graphs):
    from cine_hip.pipeline import SlicePipeline
    raws, masks, w, want = scans
    ws = (w.to(dev), w.pin_memory(), w.numpy())                       # the whitener from all three places too
    n = 4 * S + 1
    got, order = {}, []
    with SlicePipeline(net, slots=S, graphs=graphs) as pipe:
        for j in range(n):
            raw = (raws[j].to(dev), raws[j].pin_memory(), raws[j].numpy())[j % 3]
            h = pipe.submit_raw(raw, masks[j], tag=f"s{j}", crop_shape=CROP, n_frames=FRAMES, virtual_coils=V, whitener=ws[(j + j // 3) % 3])
            assert (h.index, h.slot) == (j, j % S)
            for tag, out in pipe.results():
                order.append(tag); got[tag] = out
        for tag, out in pipe.drain():
            order.append(tag); got[tag] = out
        assert pipe.pending() == 0 and pipe.set_builds == 1
        infos = dict(pipe.last_coil_info)
    assert order == [f"s{j}" for j in range(n)]
    for j in range(n):
        assert _same(got[f"s{j}"], want[j]), (S, graphs, j, float((got[f"s{j}"] - want[j]).abs().max()))
        rec = infos[f"s{j}"]
        assert rec.residual <= 1e-14 and 0 < rec.sweeps < 40 and 0 < rec.kept <= 1 and rec.lam0 > 0


# ------------------------------------------------------------------ 2. 20 and 30 coils, one V, one graph set
def test_mixed_coil_counts_share_one_whitened_graph_set(net, dev):
    from cine_hip.pipeline import SlicePipeline
    plan = [(20, 1), (30, 2), (20, 3), (30, 4), (20, 5)]              # the larger scan arrives second: the buffers grow
    raws = [_raw(c, seed) for c, seed in plan]
    masks = [_row_mask(seed) for _, seed in plan]
    wh = {20: _whitener(20, 6), 30: _whitener(30, 7)}
    want = [_sequential(net, r, m, wh[c], dev) for r, m, (c, _) in zip(raws, masks, plan)]
    with SlicePipeline(net, slots=2) as pipe:
        for j, (r, m) in enumerate(zip(raws, masks)):
            pipe.submit_raw(r.pin_memory(), m, tag=j, crop_shape=CROP, n_frames=FRAMES, virtual_coils=V, whitener=wh[plan[j][0]])
        got = list(pipe.drain())
        assert pipe.set_builds == 1
    assert [t for t, _ in got] == list(range(len(plan)))
    for j, o in got:
        assert _same(o, want[j]), j


# ------------------------------------------------------------------ 3. whitened and unwhitened: two sets, two results; the whitener alone
def test_whitened_and_unwhitened_submissions_build_two_sets(net, scans, dev):
    from cine_hip import frontend as FE
    from cine_hip.pipeline import SlicePipeline
    raws, masks, w, want = scans
    with torch.no_grad():
        a = FE.coil_matrix_from_gram(FE.coil_gram(raws[0].to(dev), FRAMES, 24), V, method="jacobi")[0]
        plain = net(FE.prepare_masked_slice(raws[0].to(dev), masks[0].to(dev), CROP, FRAMES, FS, 1e6, coil_matrix=a), masks[0].to(dev)).clone()
        w64 = w.to(dev).to(torch.complex64)
        alone = net(FE.prepare_masked_slice(raws[0].to(dev), masks[0].to(dev), CROP, FRAMES, FS, 1e6, coil_matrix=w64), masks[0].to(dev)).clone()
        full = _sequential(net, raws[0], masks[0], w, dev, v=12)
    kw = dict(crop_shape=CROP, n_frames=FRAMES)
    with SlicePipeline(net, slots=2) as pipe:
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="whitened", virtual_coils=V, whitener=w, **kw)
        assert pipe.set_builds == 1
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="plain", virtual_coils=V, **kw)
        assert pipe.set_builds == 2
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="alone", whitener=w, **kw)         # = coil_matrix=W.to(complex64)
        assert pipe.set_builds == 3
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="alone again", coil_matrix=w.to(torch.complex64), **kw)
        assert pipe.set_builds == 3
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="V = c", virtual_coils=12, whitener=w.to(dev), **kw)
        got = dict(pipe.drain())
        assert "alone" not in pipe.last_coil_info and "whitened" in pipe.last_coil_info
    assert _same(got["whitened"], want[0]) and _same(got["plain"], plain) and not _same(got["whitened"], got["plain"])
    assert _same(got["alone"], alone) and _same(got["alone again"], alone)
    assert _same(got["V = c"], full) and not _same(full, alone)


# ------------------------------------------------------------------ 4. ESPIRiT on the whitened virtual coils
def test_espirit_on_the_whitened_virtual_coils(dev):
    import test_espirit_sign as E
    from cine_hip import frontend as FE
    from cine_hip.pipeline import SlicePipeline
    model = E._net("cinenet", dev)
    w = _whitener(E.C, 8).to(dev)
    raws = [E._raw(50 + j).to(dev) for j in range(3)]
    masks = [E._row_mask(j).to(dev) for j in range(3)]
    want = []
    for raw, mask in zip(raws, masks):
        with torch.no_grad():
            a = FE.coil_matrix_from_gram(FE.coil_gram(raw, E.T, 24), 4, method="jacobi", whitener=w)[0]
            mk = FE.prepare_masked_slice(raw, mask, E.CROP, E.T, E.FS, 1e6, coil_matrix=a)
        want.append(E._eager(model, mk, mask))
    assert not torch.equal(want[0], want[1]) and all(torch.isfinite(x).all() for x in want)
    with SlicePipeline(model, slots=2) as pipe:
        for j in range(3):
            pipe.submit_raw(raws[j], masks[j], "espirit", tag=j, crop_shape=E.CROP, n_frames=E.T, ecalib_r=E.ECALIB_R, virtual_coils=4,
                            whitener=w)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    for j in range(3):
        assert torch.equal(got[j], want[j]), j


# ------------------------------------------------------------------ 5. refusals, before anything is enqueued
def test_refusals_leave_nothing_pending(net, scans, dev):
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    raws, masks, w, want = scans
    kw = dict(crop_shape=CROP, n_frames=FRAMES)
    a = _matrix(raws[0], w, dev)
    with SlicePipeline(net, slots=2) as pipe:
        pipe.submit_raw(raws[0].to(dev), masks[0], tag=0, virtual_coils=V, whitener=w, **kw)
        before = (pipe.pending(), pipe.set_builds)
        for extra in ({}, {"virtual_coils": V}):
            with pytest.raises(CineHipError, match=r"coil_matrix_from_gram\(\.\.\., whitener=W\)"):
                pipe.submit_raw(raws[1].to(dev), masks[1], coil_matrix=a, whitener=w, **extra, **kw)
        with pytest.raises(CineHipError, match="shape"):
            pipe.submit_raw(raws[1].to(dev), masks[1], virtual_coils=V, whitener=w[:11, :11], **kw)
        with pytest.raises(CineHipError, match="complex128"):
            pipe.submit_raw(raws[1].to(dev), masks[1], virtual_coils=V, whitener=w.to(torch.complex64), **kw)
        with pytest.raises(CineHipError, match="virtual_coils="):
            pipe.submit_raw(torch.zeros(RAW + (40,), dtype=torch.complex64), masks[1], whitener=torch.eye(40, dtype=torch.complex128), **kw)
        with pytest.raises(CineHipError, match="at most 64.*coil_matrix="):
            pipe.submit_raw(torch.zeros(RAW + (65,), dtype=torch.complex64), masks[1], virtual_coils=V,
                            whitener=torch.eye(65, dtype=torch.complex128), **kw)
        assert (pipe.pending(), pipe.set_builds) == before
        pipe.submit_raw(raws[1].to(dev), masks[1], tag=1, virtual_coils=V, whitener=w, **kw)   # usable after every refusal
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    assert _same(got[0], want[0]) and _same(got[1], want[1])


# ------------------------------------------------------------------ 6. no side streams, no host synchronisation
def test_submit_raw_whitened_does_not_wait_for_the_device(net, scans, dev):
    from cine_hip import ops
    from cine_hip.pipeline import SlicePipeline
    raws, masks, w, want = scans
    ws = (w.pin_memory(), w.to(dev))
    with SlicePipeline(net, slots=3) as pipe:
        ins = [(raws[j].pin_memory(), masks[j].pin_memory()) for j in range(8)]
        for j in range(4):
            pipe.submit_raw(*ins[j], tag=j, crop_shape=CROP, n_frames=FRAMES, virtual_coils=V, whitener=ws[j % 2])
        ids = {s.cuda_stream for s in pipe.streams + [pipe.copy_stream]}
        assert not [k for k in ops._SIDE_STREAMS if k[1] in ids]
        got = dict(pipe.drain())
        torch.cuda.set_sync_debug_mode("error")                                      # warm from here on: a blocking torch call would raise
        try:
            for j in range(4, 8):
                pipe.submit_raw(*ins[j], tag=j, crop_shape=CROP, n_frames=FRAMES, virtual_coils=V, whitener=ws[j % 2])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        got.update(pipe.drain())
    assert sorted(got) == list(range(8))
    assert all(_same(got[j], want[j]) for j in range(8))
