"""Retrospective gating on the device: gating.gate_readouts against the float64 restatement of the kernel test for both modes, the
readouts_from_raw round trip, and SlicePipeline.submit_readouts against the composition it stands for,
``submit_raw(gate_readouts(lines_on_device, plan), mask, apply_mask=False, n_frames=plan.n_frames, ...)``, bit for bit."""
import numpy as np
import pytest
import torch

from gating_reference import check_gated
from kernel_sweep import same_bits

pytestmark = pytest.mark.gpu

FS = (0.7, 0.0, 0.3, 0.3)
SCALE, SEED = 0.5, 1234


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def acquisition(n, nx, ny, c, seed, amp=1e-6):
    """n readouts of a scan with beats of 850 - 1150 ms, 24 readouts per beat: (lines complex64 (n, ny, c), pe_index, trigger_ms, rr_ms).
    The centre lines are taken in every beat."""
    rs = np.random.RandomState(seed)
    beat = np.arange(n) // 24
    rr = (850.0 + 300.0 * rs.uniform(size=beat.max() + 1))[beat]
    trig = (np.arange(n) % 24 + rs.uniform(size=n)) / 24.0 * rr
    pe = rs.randint(0, nx, size=n)
    pe[::6] = nx // 2 + (np.arange(n)[::6] // 6) % 2 - 1
    lines = (amp * (rs.standard_normal((n, ny, c)) + 1j * rs.standard_normal((n, ny, c)))).astype(np.complex64)
    return lines, pe.astype(np.int64), trig, rr


def row_mask(t, X, seed):
    rs = np.random.RandomState(1000 + seed)
    m = (rs.uniform(size=(1, t, 1, X, 1, 1)) < 0.3).astype(np.uint8)
    m[:, :, :, X // 2 - 2:X // 2 + 2] = 1
    return torch.from_numpy(m)


def sens_maps(c, X, Y, seed):
    """(1, 1, c, X, Y, 2) float32: smooth random maps of unit root-sum-of-squares."""
    rs = np.random.RandomState(2000 + seed)
    x, y = np.meshgrid(np.linspace(-1, 1, X), np.linspace(-1, 1, Y), indexing="ij")
    a = rs.standard_normal((c, 3)) + 1j * rs.standard_normal((c, 3))
    s = a[:, 0, None, None] + a[:, 1, None, None] * x[None] + a[:, 2, None, None] * y[None]
    s = s / np.sqrt((np.abs(s) ** 2).sum(axis=0, keepdims=True))
    return torch.from_numpy(np.stack([s.real, s.imag], axis=-1).astype(np.float32))[None, None]


def places(x, k, dev):
    """A numpy array from the three places an input may lie in."""
    t = torch.from_numpy(x)
    return (t.to(dev), t.pin_memory(), x)[k % 3]


# ------------------------------------------------------------------ 1. gate_readouts against float64
@pytest.mark.parametrize("mode", ["nearest", "linear"])
def test_gate_readouts_against_the_kernel_tests_reference(dev, mode):
    from cine_hip import gating as G
    T, nx, ny, c = 5, 24, 7, 3
    lines, pe, trig, rr = acquisition(150, nx, ny, c, seed=3, amp=1.0)
    plan = G.plan_gating(pe, trig, rr, T, nx, mode=mode, reject=(0.9, 1.1))
    assert plan.info["dropped_reject"] > 0 and plan.info["empty_rows"] == int((plan.acquired == 0).sum())
    got = G.gate_readouts(torch.from_numpy(lines).to(dev), plan)
    assert got.shape == (T, nx, ny, c) and got.dtype == torch.complex64
    pairs = np.ascontiguousarray(lines).view(np.float32).reshape(150, ny * c, 2)
    out = torch.view_as_real(got).cpu().numpy().reshape(T * nx, ny * c, 2)
    worst = check_gated(out, pairs, plan.row_ptr, plan.index, plan.weight, mode)
    print(f"{mode}: {plan.entries} entries, worst error {worst:.3f} of its bar")
    # float32 pairs in, an output of the caller's own
    mine = torch.full((T, nx, ny, c, 2), float("nan"), device=dev)
    assert G.gate_readouts(torch.view_as_real(torch.from_numpy(lines)).to(dev), plan, out=mine) is mine
    assert same_bits(mine, torch.view_as_real(got))
    assert np.array_equal(plan.acquired != 0, np.abs(got.cpu().numpy()).sum(axis=(2, 3)) != 0)


def test_gate_readouts_refusals(dev):
    from cine_hip import gating as G
    from cine_hip._lib import CineHipError
    lines, pe, trig, rr = acquisition(48, 6, 4, 2, seed=1)
    plan = G.plan_gating(pe, trig, rr, 3, 6)
    ld = torch.from_numpy(lines).to(dev)
    with pytest.raises(CineHipError, match="47 readouts, the plan was made for 48"):
        G.gate_readouts(ld[:47], plan)
    with pytest.raises(CineHipError, match="no CPU fallback"):
        G.gate_readouts(torch.from_numpy(lines), plan)
    with pytest.raises(CineHipError, match="GatingPlan"):
        G.gate_readouts(ld, (plan.row_ptr, plan.index, plan.weight))
    with pytest.raises(CineHipError, match="out must be"):
        G.gate_readouts(ld, plan, out=torch.empty((3, 6, 4, 2, 2), device=dev))


# ------------------------------------------------------------------ 2. the round trip
@pytest.mark.parametrize("shape", [(4, 20, 14, 4), (3, 7, 5, 3), (1, 1, 1, 1)])
def test_round_trip_returns_raw_with_its_unacquired_lines_zeroed(dev, shape):
    from cine_hip import gating as G
    t, nx, ny, c = shape
    rs = np.random.RandomState(sum(shape))
    raw = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    acq = (rs.uniform(size=(t, nx)) < 0.4).astype(np.uint8)
    acq[0, 0] = 1
    zeroed = raw.copy()
    zeroed[acq == 0] = 0                                                       # +0, as the kernel writes an empty row (raw * 0 would keep signs)
    want = torch.view_as_real(torch.from_numpy(zeroed))
    for src in (raw, torch.from_numpy(raw).to(dev)):                           # host and device raw
        lines, pe, trig, rr = G.readouts_from_raw(src, acq)
        assert isinstance(lines, torch.Tensor) == isinstance(src, torch.Tensor)              # of raw's kind, and in raw's place
        ld = lines if isinstance(lines, torch.Tensor) else torch.from_numpy(lines).to(dev)
        assert ld.device == dev
        got = G.gate_readouts(ld, G.plan_gating(pe, trig, rr, t, nx, mode="nearest"))
        assert same_bits(torch.view_as_real(got).cpu(), want)


# ------------------------------------------------------------------ 3. submit_readouts == submit_raw of the gated array
def _varnet_rnn():
    import reconstruction.models as M
    from cine_hip import synth
    net = M.VarNet_RNN(2, 4, 2, 6)                                             # the smallest network of tests/test_raw_pipeline.py
    synth.fill_parameters_(net, 9, keep=("lambda",))
    return net


def _kt():
    from cine_hip.classical import KtSparseSense
    return KtSparseSense(iters=3)


def _whiten_noise(dev, c):
    from cine_hip import noise as N
    rs = np.random.RandomState(5)
    low = np.tril(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c))) * 1e-7
    low[np.diag_indices(c)] = np.abs(np.diag(low)) + 1e-7
    return N.NoiseSpec(torch.from_numpy(low.astype(np.complex64)).to(dev), SCALE, SEED, 2)


# name -> (model, gated shape (T, x, y, c), crop, coils behind the front-end, wants sens, gating mode, keywords(dev))
CONFIGS = {
    "kt_sparse_sense": (_kt, (4, 20, 14, 4), (16, 12), 4, True, "linear", lambda dev: {}),
    "varnet_rnn_line": (_varnet_rnn, (5, 30, 28, 3), (24, 20), 3, False, "nearest", lambda dev: {}),
    "window": (_kt, (3, 401, 6, 3), (16, 6), 3, True, "nearest", lambda dev: {}),
    "virtual_coils": (_kt, (4, 20, 14, 4), (16, 12), 3, True, "linear", lambda dev: {"virtual_coils": 3}),
    "noise": (_kt, (4, 20, 14, 4), (16, 12), 4, True, "nearest", lambda dev: {"noise": _whiten_noise(dev, 4)}),
}


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_submit_readouts_equals_submit_raw_of_the_gated_array(dev, name, graphs):
    from cine_hip import gating as G, ops
    from cine_hip.pipeline import SlicePipeline
    make, (T, nx, ny, c), crop, v, wants_sens, mode, keywords = CONFIGS[name]
    assert (ops.fft_line_supported(nx) and ops.fft_line_supported(ny)) == (name != "window")
    model = make().to(dev).eval()
    kw = dict(crop_shape=crop, **keywords(dev))
    mask = row_mask(T, crop[0], 3).to(dev)
    sens = sens_maps(v, crop[0], crop[1], 4).to(dev) if wants_sens else None
    # five slices: the readout count shrinks, then grows past the first (the gating buffers grow, nothing is built again)
    counts = [6 * nx, 4 * nx, 9 * nx, 9 * nx + 1, 5 * nx]
    scans = [acquisition(n, nx, ny, c, seed=10 + j) for j, n in enumerate(counts)]
    plans = [G.plan_gating(pe, trig, rr, T, nx, mode=mode, reject=(0.8, 1.25)) for _, pe, trig, rr in scans]
    assert all(0 < int(p.acquired.sum()) for p in plans) and (mode == "linear" or any(int(p.acquired.sum()) < T * nx for p in plans))
    with SlicePipeline(model, slots=2, graphs=graphs) as pipe:
        for j, ((lines, _, _, _), plan) in enumerate(zip(scans, plans)):
            pipe.submit_readouts(places(lines, j, dev), plan, mask, sens, tag=("readouts", j), **kw)
            gated = G.gate_readouts(torch.from_numpy(lines).to(dev), plan)
            extra = {"noise_mask": plan.acquired} if name == "noise" else {}   # what submit_readouts takes when none is given
            pipe.submit_raw(gated, mask, sens, tag=("raw", j), apply_mask=False, n_frames=plan.n_frames, **kw, **extra)
            if name == "noise" and j == 0:                                     # ... and that mask matters: noise on every line differs
                pipe.submit_raw(gated, mask, sens, tag="everywhere", apply_mask=False, n_frames=plan.n_frames, **kw)
                pipe.submit_readouts(lines, plan, mask, sens, tag="given", noise_mask=torch.from_numpy(plan.acquired).bool(), **kw)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1                                            # one key for both calls; n_lines and the entry count are not in it
    for j in range(len(scans)):
        a, b = got[("readouts", j)], got[("raw", j)]
        assert bool(torch.isfinite(b).all()) and same_bits(a, b), (name, j, float((a - b).abs().max()))
    assert not same_bits(got[("raw", 1)], got[("raw", 2)])
    if name == "noise":
        assert not same_bits(got["everywhere"], got[("raw", 0)]) and same_bits(got["given"], got[("raw", 0)])


def test_different_readout_counts_leave_set_builds_at_one(dev):
    from cine_hip import gating as G
    from cine_hip.pipeline import SlicePipeline
    T, nx, ny, c, crop = 4, 20, 14, 4, (16, 12)
    model = _kt().to(dev).eval()
    mask, sens = row_mask(T, crop[0], 3).to(dev), sens_maps(c, crop[0], crop[1], 4).to(dev)
    outs = []
    with SlicePipeline(model, slots=3) as pipe:
        for j, (n, mode) in enumerate([(60, "nearest"), (200, "linear")]):     # more readouts and more entries per row
            lines, pe, trig, rr = acquisition(n, nx, ny, c, seed=40 + j)
            plan = G.plan_gating(pe, trig, rr, T, nx, mode=mode)
            pipe.submit_readouts(torch.from_numpy(lines).pin_memory(), plan, mask, sens, tag=j, crop_shape=crop)
            assert pipe.set_builds == 1
            with torch.no_grad():
                from cine_hip import frontend as FE
                mk = FE.prepare_masked_slice(G.gate_readouts(torch.from_numpy(lines).to(dev), plan), mask, crop, T, FS, 1e6, apply_mask=False)
                outs.append(model(mk, mask, sens).clone())
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    assert same_bits(got[0], outs[0]) and same_bits(got[1], outs[1])           # and equal to the sequential forward


def test_lines_from_numpy_pinned_and_device_memory_give_the_same_bits(dev):
    from cine_hip import gating as G
    from cine_hip.pipeline import SlicePipeline
    T, nx, ny, c, crop = 4, 20, 14, 4, (16, 12)
    model = _kt().to(dev).eval()
    mask, sens = row_mask(T, crop[0], 3).to(dev), sens_maps(c, crop[0], crop[1], 4).to(dev)
    lines, pe, trig, rr = acquisition(130, nx, ny, c, seed=8)
    plan = G.plan_gating(pe, trig, rr, T, nx, mode="linear")
    keep = lines.copy()
    forms = {"numpy": lines, "pairs": np.ascontiguousarray(lines).view(np.float32).reshape(lines.shape + (2,)),
             "pinned": torch.from_numpy(lines).pin_memory(), "pageable": torch.from_numpy(lines), "device": torch.from_numpy(lines).to(dev)}
    with SlicePipeline(model, slots=2) as pipe:
        for k in range(2):                                                     # twice: every (slot, parity) sees every form
            for form, x in forms.items():
                pipe.submit_readouts(x, plan, mask, sens, tag=(form, k), crop_shape=crop)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    first = got[("numpy", 0)]
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    for tag, o in got.items():
        assert same_bits(o, first), tag
    assert np.array_equal(lines, keep)


def test_submit_readouts_refusals(dev):
    from cine_hip import gating as G
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    T, nx, ny, c, crop = 4, 20, 14, 4, (16, 12)
    mask, sens = row_mask(T, crop[0], 3).to(dev), sens_maps(c, crop[0], crop[1], 4).to(dev)
    lines, pe, trig, rr = acquisition(60, nx, ny, c, seed=2)
    plan = G.plan_gating(pe, trig, rr, T, nx)
    with SlicePipeline(_kt().to(dev).eval(), slots=1) as pipe:
        with pytest.raises(CineHipError, match="59 readouts, the plan was made for 60"):
            pipe.submit_readouts(lines[:59], plan, mask, sens, crop_shape=crop)
        with pytest.raises(CineHipError, match="GatingPlan"):
            pipe.submit_readouts(lines, None, mask, sens, crop_shape=crop)
        with pytest.raises(CineHipError, match="lines: shape"):
            pipe.submit_readouts(lines[:, :, 0], plan, mask, sens, crop_shape=crop)
        with pytest.raises(TypeError):
            pipe.submit_readouts(lines, plan, mask, sens, crop_shape=crop, apply_mask=True)
        assert pipe.set_builds == 0 and pipe.pending() == 0
        pipe.submit_readouts(lines, plan, mask, sens, crop_shape=crop)         # usable after every refusal
        assert len(list(pipe.drain())) == 1
