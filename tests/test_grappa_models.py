"""cine_hip.grappa on the GPU: ``grappa`` end to end against the float64 reference (tests/grappa_reference.py) within the model-level
bar max |delta| / peak <= 1e-4, its ``check`` and ``output`` keywords, and ``Grappa`` captured into a graph and through ``SlicePipeline``
(k-space input and raw input) bit for bit against the eager calls."""
import numpy as np
import pytest
import torch

import grappa_reference as ref

pytestmark = pytest.mark.gpu

MODEL_BAR = 1e-4
# t, c, h, w, R, (ky, kx), ACS lines
CASES = [(6, 8, 48, 40, 3, (2, 5), 0), (8, 8, 48, 40, 4, (2, 5), 0), (5, 6, 30, 22, 2, (2, 3), 0), (6, 8, 48, 40, 3, (2, 5), 12)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def pairs(z):
    return torch.from_numpy(np.stack((z.real, z.imag), -1).astype(np.float32))


def problem(case, dev):
    """(masked k-space (1, t, c, h, w, 2), mask (1, t, 1, h, 1, 1), keywords of the calibration) on the device, and the numpy pair."""
    t, c, h, w, R, kernel, acs = case
    _, mask, mk = ref.phantom_slice(t, c, h, w, R, acs=acs)
    lo = h // 2 - acs // 2
    kw = {"acs": (lo, lo + acs)} if acs else {"calib": "tgrappa", "calib_rows": h}
    return pairs(mk)[None].to(dev), torch.from_numpy(mask.reshape(1, t, 1, h, 1, 1)).to(dev), kw, mk, mask


@pytest.mark.parametrize("case", CASES, ids=lambda s: "t%d-c%d-%dx%d-R%d-k%dx%d-acs%d" % (s[:5] + s[5] + s[6:]))
def test_grappa_against_the_reference(dev, case):
    from cine_hip import grappa as G
    t, c, h, w, R, kernel, acs = case
    d_mk, d_mask, kw, mk, mask = problem(case, dev)
    want, info_ref, off_ref = ref.grappa(mk, mask, R, kernel, 1e-4, **kw)
    filled, info, off = G.grappa(d_mk, d_mask, R, kernel=kernel, lam=1e-4, output="kspace", record=True, **kw)
    assert tuple(filled.shape) == (1, t, c, h, w, 2) and tuple(info.shape) == (1, 4) and off.cpu().tolist() == [off_ref.tolist()]
    got = filled[0].cpu().numpy().astype(np.float64)
    got = got[..., 0] + 1j * got[..., 1]
    e_k = float(np.abs(got - want).max() / np.abs(want).max())
    acquired = mask.astype(bool)
    assert (got[acquired.nonzero()[0], :, acquired.nonzero()[1]] == mk[acquired.nonzero()[0], :, acquired.nonzero()[1]]).all()
    img = G.grappa(d_mk, d_mask, R, kernel=kernel, lam=1e-4, **kw)
    assert tuple(img.shape) == (1, t, h, w)
    rss = ref.rss(want)
    e_i = float(np.abs(img[0].cpu().numpy() - rss).max() / rss.max())
    print(f"k-space {e_k:.3e}, RSS image {e_i:.3e} of the peak (bar {MODEL_BAR:g}); info {info.cpu().tolist()}, reference {info_ref.tolist()}")
    assert e_k <= MODEL_BAR and e_i <= MODEL_BAR
    assert float(info[0, 0]) <= G.RESIDUAL_MAX
    mod = G.Grappa(accel=R, kernel=kernel, lam=1e-4, **kw).eval()
    assert torch.equal(mod(d_mk, d_mask), img) and torch.equal(mod(d_mk, d_mask, output="kspace"), filled)
    assert mod.last_info["status"].cpu().tolist() == [[0] * t] and torch.equal(mod.last_info["offsets"], off)


def test_check_raises_on_a_nan_in_the_calibration_block(dev):
    from cine_hip import grappa as G
    from cine_hip._lib import CineHipError
    case = CASES[2]
    t, c, h, w, R, kernel, _ = case
    d_mk, d_mask, kw, _, mask = problem(case, dev)
    bad = d_mk.clone()
    bad[0, 0, 1, int(np.flatnonzero(mask[0])[len(np.flatnonzero(mask[0])) // 2]), 3, 0] = float("nan")
    with pytest.raises(CineHipError, match="residual"):
        G.grappa(bad, d_mask, R, kernel=kernel, **kw)
    out, info, _ = G.grappa(bad, d_mask, R, kernel=kernel, check=False, record=True, **kw)       # unchecked: the NaN is reported, not raised
    assert bool(torch.isnan(info[0, 0]))
    holes = d_mask.clone()
    holes[0, 1, 0, int(np.flatnonzero(mask[1])[1]), 0, 0] = 0                                    # frame 1 loses a lattice row
    with pytest.raises(ValueError, match="frame 1"):
        G.grappa(d_mk, holes, R, kernel=kernel, **kw)
    with pytest.raises(ValueError, match="acquired by no frame"):                                # only frame 0's rows: TGRAPPA has holes
        G.grappa(d_mk, d_mask[:, :1].expand(1, t, 1, h, 1, 1).contiguous(), R, kernel=kernel, **kw)


def test_output_keyword(dev):
    from cine_hip import grappa as G, ops, synth
    case = CASES[2]
    t, c, h, w, R, kernel, _ = case
    d_mk, d_mask, kw, _, _ = problem(case, dev)
    with pytest.raises(ValueError, match="sens_maps"):
        G.grappa(d_mk, d_mask, R, kernel=kernel, output="complex", **kw)
    maps = pairs(synth.coil_maps(c, h, w))[None, None].to(dev)
    filled = G.grappa(d_mk, d_mask, R, kernel=kernel, output="kspace", **kw)
    mag = G.grappa(d_mk, d_mask, R, kernel=kernel, sens_maps=maps, **kw)
    cx = G.grappa(d_mk, d_mask, R, kernel=kernel, sens_maps=maps, output="complex", **kw)
    assert tuple(mag.shape) == (1, t, h, w) and tuple(cx.shape) == (1, t, h, w, 2)
    assert torch.equal(mag, ops.sens_reduce(filled, maps, magnitude=True))
    assert torch.equal(cx, ops.sens_reduce(filled, maps).squeeze(2))
    assert torch.equal(G.grappa(d_mk, d_mask, R, kernel=kernel, **kw), ops.zero_filled_rss(filled))


def test_grappa_is_capturable(dev):
    """Captured and replayed twice: the eager bits.  The process keeps its default number of hardware queues."""
    from cine_hip import grappa as G
    from cine_hip.pipeline import pipeline_streams
    case = CASES[0]
    t, c, h, w, R, kernel, _ = case
    d_mk, d_mask, kw, _, _ = problem(case, dev)
    model = G.Grappa(accel=R, kernel=kernel, **kw).eval()
    want = model(d_mk, d_mask).clone()
    s = pipeline_streams(dev, 1)[0][0]                                     # a stream of the pipelines' pool: the test creates none of its own
    with torch.cuda.stream(s):
        warm = model(d_mk, d_mask).clone()
    s.synchronize()
    assert torch.equal(warm, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = model(d_mk, d_mask)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    assert model.last_info["status"].cpu().tolist() == [[0] * t] and float(model.last_info["info"][0, 0]) <= G.RESIDUAL_MAX


def test_pipeline_submit_and_submit_raw(dev):
    from cine_hip import frontend as FE, grappa as G
    from cine_hip.pipeline import SlicePipeline
    t, c, h, w, R = 6, 8, 48, 40, 3
    model = G.Grappa(accel=R).eval()
    full = ref.phantom_slice(t, c, h, w, R)[0]
    ins = []
    for j in range(3):                                                     # three slices whose frames start the interleave at offset j
        mask = ref.lattice_mask(t, h, R, offsets=[(f + j) % R for f in range(t)])
        d = pairs((1.0 + 0.25 * j) * full * mask[:, None, :, None])[None].to(dev)
        ins.append((d, torch.from_numpy(mask.reshape(1, t, 1, h, 1, 1)).to(dev)))
    want = [model(*a).clone() for a in ins]
    assert not torch.equal(want[0], want[1]) and all(bool(torch.isfinite(v).all()) for v in want)
    with SlicePipeline(model, slots=2) as pipe:
        assert pipe.graphs
        for j, a in enumerate(ins):
            pipe.submit(*a, tag=j)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    for j in range(3):
        assert torch.equal(got[j], want[j]), j

    T, C, N = 5, 6, 64
    raw_shape, crop, fs = (T, 72, 68, C), (N, N), (0.7, 0.0, 0.3, 0.3)
    rs = np.random.RandomState(50)
    x, y = np.arange(72)[:, None] - 36, np.arange(68)[None, :] - 34
    wgt = np.exp(-(x * x / (2.0 * 9.0 ** 2) + y * y / (2.0 * 8.5 ** 2))) + 0.02
    z = rs.standard_normal(raw_shape) + 1j * rs.standard_normal(raw_shape)
    raw = torch.from_numpy((1e-6 * z * wgt[None, :, :, None]).astype(np.complex64)).to(dev)
    mask = G.lattice_mask(T, N, R).to(dev)
    with torch.no_grad():
        want_raw = model(FE.prepare_masked_slice(raw, mask, crop, T, fs, 1e6), mask).clone()
    with SlicePipeline(model, slots=2) as pipe:
        pipe.submit_raw(raw, mask, tag="raw", crop_shape=crop, n_frames=T, apply_mask=True)
        got = dict(pipe.drain())
    assert bool(torch.isfinite(want_raw).all()) and float(want_raw.max()) > 0 and torch.equal(got["raw"], want_raw)
