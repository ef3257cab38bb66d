"""SlicePipeline.submit_raw(..., virtual_coils=V): every slice compressed with the matrix of its own calibration block, in flight.

The identity under test: the pipeline's output is, bit for bit, ``model(prepare_masked_slice(raw, mask, ..., coil_matrix=A), mask)`` with
``A = coil_matrix_from_gram(coil_gram(raw, n_frames, region), V, method="jacobi")[0]`` -- the public pieces, run one after the other.
The raw data are the designed inputs of tests/test_coil_compress.py (a known spectrum in a seeded unitary basis), scaled to the
amplitude of a k-space."""
import numpy as np
import pytest
import torch

from test_coil_compress import assert_gaps, designed_raw, gram_ref, matrix_ref

pytestmark = pytest.mark.gpu

FS = (0.7, 0.0, 0.3, 0.3)
RAW, CROP, FRAMES, V = (6, 30, 28), (24, 20), 5, 6           # 6 frames in the file, 5 kept
AMP = np.float32(1e-6)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _raw(c, seed):
    return torch.from_numpy(designed_raw(*RAW, c, seed=seed) * AMP)


def _row_mask(seed, t=FRAMES, X=CROP[0]):
    rs = np.random.RandomState(1000 + seed)
    m = (rs.uniform(size=(1, t, 1, X, 1, 1)) < 0.3).astype(np.uint8)
    half = 1 + seed % 3
    m[:, :, :, X // 2 - half:X // 2 + half] = 1
    return torch.from_numpy(m)


@pytest.fixture(scope="module")
def net(dev):
    import reconstruction.models as M
    from cine_hip import synth
    n = M.VarNet_RNN(2, 4, 2, 6)
    synth.fill_parameters_(n, 9, keep=("lambda",))
    return n.to(dev).eval()


def _matrix(raw, dev, v=V, region=24, frames=FRAMES):
    from cine_hip import frontend as FE
    return FE.coil_matrix_from_gram(FE.coil_gram(raw.to(dev), frames, region), v, method="jacobi")[0]


def _sequential(net, raw, mask, dev, a=None, v=V, region=24):
    from cine_hip import frontend as FE
    with torch.no_grad():
        a = _matrix(raw, dev, v, region) if a is None else a
        mk = FE.prepare_masked_slice(raw.to(dev), mask.to(dev), CROP, FRAMES, FS, 1e6, coil_matrix=a)
        return net(mk, mask.to(dev)).clone()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


@pytest.fixture(scope="module")
def scans(net, dev):
    """13 slices of 12 coils (4 S + 1 for S = 3) and their sequential forwards, computed once."""
    raws = [_raw(12, 100 + j) for j in range(13)]
    masks = [_row_mask(j) for j in range(13)]
    want = [_sequential(net, r, m, dev) for r, m in zip(raws, masks)]
    assert all(bool(torch.isfinite(w).all()) for w in want) and not torch.equal(want[0], want[1])
    return raws, masks, want


# ------------------------------------------------------------------ 1. the identity, with graphs and without, S = 1 and S = 3
@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("S", [1, 3])
def test_submit_raw_virtual_coils_matches_the_sequential_forward(net, scans, dev, S, graphs):
    from cine_hip.pipeline import SlicePipeline
    raws, masks, want = scans
    n = 4 * S + 1
    got, order = {}, []
    with SlicePipeline(net, slots=S, graphs=graphs) as pipe:
        for j in range(n):
            raw = (raws[j].to(dev), raws[j].pin_memory(), raws[j].numpy())[j % 3]     # from all three places
            h = pipe.submit_raw(raw, masks[j], tag=f"s{j}", crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
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
def test_mixed_coil_counts_share_one_graph_set(net, dev):
    from cine_hip.pipeline import SlicePipeline
    plan = [(20, 1), (30, 2), (20, 3), (30, 4), (20, 5), (30, 6), (20, 7)]           # the larger scan arrives second: the buffers grow
    raws = [_raw(c, seed) for c, seed in plan]
    masks = [_row_mask(seed) for _, seed in plan]
    want = [_sequential(net, r, m, dev) for r, m in zip(raws, masks)]
    with SlicePipeline(net, slots=2) as pipe:
        for j, (r, m) in enumerate(zip(raws, masks)):
            pipe.submit_raw(r.pin_memory(), m, tag=j, crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
        got = list(pipe.drain())
        assert pipe.set_builds == 1
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="other V", crop_shape=CROP, n_frames=FRAMES, virtual_coils=V + 1)
        assert pipe.set_builds == 2                                                  # V is part of the key
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="other region", crop_shape=CROP, n_frames=FRAMES, virtual_coils=V + 1, cc_region=12)
        assert pipe.set_builds == 3                                                  # and so is the region
        assert len(list(pipe.drain())) == 2
    assert [t for t, _ in got] == list(range(len(plan)))
    for j, o in got:
        assert _same(o, want[j]), j


# ------------------------------------------------------------------ 3. each slice gets its own matrix
def test_each_slice_gets_its_own_matrix(net, dev):
    """Two slices from designed inputs of two seeds (two unitary bases: two dominant subspaces).  In flight each is compressed with its
    own matrix; the matrix of the first applied to the second gives other data, and another reconstruction."""
    from cine_hip import frontend as FE
    from cine_hip.pipeline import SlicePipeline
    raws, mask = [_raw(12, 31), _raw(12, 32)], _row_mask(3)
    for r in raws:
        assert_gaps(matrix_ref(gram_ref(r.numpy(), FRAMES, 24), V)[1], V)
    mats = [_matrix(r, dev) for r in raws]
    p0, p1 = (m.conj().transpose(0, 1) @ m for m in mats)
    assert float((p0 - p1).abs().max()) > 0.1                                        # the subspaces differ
    own = FE.compress_coils(raws[1].to(dev), mats[1], FRAMES)
    shared = FE.compress_coils(raws[1].to(dev), mats[0], FRAMES)
    assert float(own.abs().pow(2).sum()) > 1.5 * float(shared.abs().pow(2).sum())    # the foreign matrix misses this slice's energy
    want_own = [_sequential(net, r, mask, dev) for r in raws]
    want_shared = _sequential(net, raws[1], mask, dev, a=mats[0])
    assert not torch.equal(want_own[1], want_shared)
    with SlicePipeline(net, slots=2) as pipe:
        for j, r in enumerate(raws):
            pipe.submit_raw(r.to(dev), mask.to(dev), tag=j, crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
        got = dict(pipe.drain())
    assert _same(got[0], want_own[0]) and _same(got[1], want_own[1]) and not _same(got[1], want_shared)


# ------------------------------------------------------------------ 4. ESPIRiT and a mask that varies along w, on the V virtual coils
@pytest.mark.parametrize("kind,general", [("cinenet", False), ("varnet", True)], ids=["cinenet-row", "varnet-general"])
def test_espirit_on_the_virtual_coils(dev, kind, general):
    import test_espirit_sign as E
    from cine_hip import frontend as FE
    from cine_hip.pipeline import SlicePipeline
    model = E._net(kind, dev)
    raws = [E._raw(50 + j).to(dev) for j in range(3)]
    masks = [(E._general_mask(20 + j) if general else E._row_mask(j)).to(dev) for j in range(3)]
    want = []
    for raw, mask in zip(raws, masks):
        with torch.no_grad():
            a = FE.coil_matrix_from_gram(FE.coil_gram(raw, E.T, 24), 4, method="jacobi")[0]
            mk = FE.prepare_masked_slice(raw, mask, E.CROP, E.T, E.FS, 1e6, coil_matrix=a)
        want.append(E._eager(model, mk, mask))
    assert not torch.equal(want[0], want[1]) and all(torch.isfinite(w).all() for w in want)
    with SlicePipeline(model, slots=2) as pipe:
        for j in range(3):
            pipe.submit_raw(raws[j], masks[j], "espirit", tag=j, crop_shape=E.CROP, n_frames=E.T, ecalib_r=E.ECALIB_R, virtual_coils=4)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    for j in range(3):
        assert torch.equal(got[j], want[j]), j


# ------------------------------------------------------------------ 5. the kept share
def test_kept_share_is_the_float64_eigenvalue_share(net, dev):
    from cine_hip.pipeline import SlicePipeline
    raws = [_raw(12, 4), _raw(20, 1)]
    want = []
    for r in raws:
        lam = matrix_ref(gram_ref(r.numpy(), FRAMES, 0), V)[1]                       # the whole matrix as the region
        assert_gaps(lam, V)
        want.append(lam[:V].sum() / lam.sum())
    with SlicePipeline(net, slots=2) as pipe:
        for j, r in enumerate(raws):
            pipe.submit_raw(r.pin_memory(), _row_mask(j), tag=("scan", j), crop_shape=CROP, n_frames=FRAMES, virtual_coils=V, cc_region=0)
        assert not pipe.last_coil_info                                               # filed when the slice is handed out
        got = list(pipe.drain())
        for j in range(2):
            rec = pipe.last_coil_info[("scan", j)]
            print(f"slice {j}: kept {rec.kept:.12f}, float64 eigenvalue share {want[j]:.12f}, residual {rec.residual:.2e}, sweeps {rec.sweeps}")
            assert abs(rec.kept - want[j]) <= 1e-9
    assert len(got) == 2


# ------------------------------------------------------------------ 6. a NaN in the raw data
def test_a_nan_slice_is_reported_by_tag_and_its_neighbours_come_out_right(net, scans, dev):
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    raws, masks, want = scans
    bad = raws[1].clone()
    bad[2, 15, 14, 3] = complex(float("nan"), 0.0)                                   # inside the calibration block
    got = {}
    with SlicePipeline(net, slots=2) as pipe:
        pipe.submit_raw(raws[0].pin_memory(), masks[0], tag="before", crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
        pipe.submit_raw(bad.pin_memory(), masks[1], tag="slice-nan", crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
        pipe.submit_raw(raws[2].pin_memory(), masks[2], tag="after", crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
        with pytest.raises(CineHipError, match="slice-nan.*NaN"):
            for tag, out in pipe.drain():
                got[tag] = out
        for tag, out in pipe.drain():
            got[tag] = out
        assert pipe.pending() == 0 and "slice-nan" not in pipe.last_coil_info
    assert sorted(got) == ["after", "before"]
    assert _same(got["before"], want[0]) and _same(got["after"], want[2])


# ------------------------------------------------------------------ 7. refusals, before anything is enqueued
def test_refusals_leave_nothing_pending(net, scans, dev):
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    raws, masks, want = scans
    kw = dict(crop_shape=CROP, n_frames=FRAMES)
    a = _matrix(raws[0], dev)
    wide = torch.zeros(RAW + (65,), dtype=torch.complex64)
    with SlicePipeline(net, slots=2) as pipe:
        pipe.submit_raw(raws[0].to(dev), masks[0], tag=0, virtual_coils=V, **kw)
        before = (pipe.pending(), pipe.set_builds)
        with pytest.raises(CineHipError, match="one of the two"):
            pipe.submit_raw(raws[1].to(dev), masks[1], virtual_coils=V, coil_matrix=a, **kw)
        for v in (0, 13, -1, 2.5, True):
            with pytest.raises(CineHipError, match="virtual_coils"):
                pipe.submit_raw(raws[1].to(dev), masks[1], virtual_coils=v, **kw)
        with pytest.raises(CineHipError, match="at most 32"):
            pipe.submit_raw(torch.zeros(RAW + (40,), dtype=torch.complex64), masks[1], virtual_coils=33, **kw)
        with pytest.raises(CineHipError, match="cc_region"):
            pipe.submit_raw(raws[1].to(dev), masks[1], virtual_coils=V, cc_region=-1, **kw)
        with pytest.raises(CineHipError, match="at most 64.*coil_matrix="):
            pipe.submit_raw(wide, masks[1], virtual_coils=V, **kw)
        with pytest.raises(CineHipError, match="hashable"):
            pipe.submit_raw(raws[1].to(dev), masks[1], tag=[1], virtual_coils=V, **kw)
        assert (pipe.pending(), pipe.set_builds) == before
        pipe.submit_raw(raws[1].to(dev), masks[1], tag=1, virtual_coils=V, **kw)     # usable after every refusal
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    assert _same(got[0], want[0]) and _same(got[1], want[1])


# ------------------------------------------------------------------ 8. no side streams, no host synchronisation
def test_submit_raw_virtual_coils_does_not_wait_for_the_device(net, scans, dev):
    from cine_hip import ops
    from cine_hip.pipeline import SlicePipeline
    raws, masks, want = scans
    with SlicePipeline(net, slots=3) as pipe:
        ins = [(raws[j].pin_memory(), masks[j].pin_memory()) for j in range(8)]
        for j in range(4):
            pipe.submit_raw(*ins[j], tag=j, crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
        ids = {s.cuda_stream for s in pipe.streams + [pipe.copy_stream]}
        assert not [k for k in ops._SIDE_STREAMS if k[1] in ids]
        got = dict(pipe.drain())
        torch.cuda.set_sync_debug_mode("error")                                      # warm from here on: a blocking torch call would raise
        try:
            for j in range(4, 8):
                pipe.submit_raw(*ins[j], tag=j, crop_shape=CROP, n_frames=FRAMES, virtual_coils=V)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        got.update(pipe.drain())
    assert sorted(got) == list(range(8))
    assert all(_same(got[j], want[j]) for j in range(8))
