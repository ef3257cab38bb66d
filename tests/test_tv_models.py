"""cine_hip.classical's total-variation baseline on the GPU: total_variation / TotalVariation eagerly, and TotalVariation through
SlicePipeline with graphs -- k-space input, and raw input with the maps calibrated in flight (sens_maps="espirit") -- bit for bit against
the eager calls."""
import numpy as np
import pytest
import torch

import kt_reference as K
import tv_reference as R
from kernel_sweep import BAR_CAP

pytestmark = pytest.mark.gpu
SHAPE = (1, 5, 3, 24, 20)
ITERS = 30


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def inputs(dev, layout="row", shape=SHAPE):
    p = K.problem(shape, layout)
    return p, p["masked_kspace"].to(dev), p["mask"].to(dev), p["sens_maps"].to(dev)


@pytest.mark.parametrize("layout", ["row", "plane"])
def test_module_function_outputs_and_explicit_settings(dev, layout):
    from cine_hip import classical, dc, ops
    p, mk, mask, sens = inputs(dev, layout)
    b, t, c, h, w = SHAPE
    x = classical.total_variation(mk, mask, sens, iters=ITERS)
    assert x.shape == (b, t, h, w) and bool(torch.isfinite(x).all())
    assert torch.equal(classical.TotalVariation(iters=ITERS).eval()(mk, mask, sens), x)                   # the module is the function
    assert torch.equal(classical.total_variation(mk, mask.float(), sens, iters=ITERS), x)                 # any numeric 0 / 1 mask
    xc = classical.total_variation(mk, mask, sens, iters=ITERS, output="complex")
    assert xc.shape == (b, t, h, w, 2) and torch.equal(ops.complex_abs(xc), x)
    assert torch.equal(classical.TotalVariation(iters=ITERS).eval()(mk, mask, sens, output="complex"), xc)
    # tv_peaks against the yardstick, then the defaults computed by hand and passed as absolute device values
    zf = dc.Acquisition(mk, ops.as_mask_u8(mask, mk), sens).zero_filled()
    for periodic in (True, False):
        peak_t, peak_s = classical.tv_peaks(zf, periodic)
        want_t, want_s = R.peaks(p["zf"], periodic)
        assert peak_t.shape == peak_s.shape == (1,) and peak_t.is_cuda
        assert abs(float(peak_t) - want_t) <= 1e-5 * want_t and abs(float(peak_s) - want_s) <= 1e-5 * want_s
    peak_t, peak_s = classical.tv_peaks(zf, True)
    step = classical.default_step(sens)
    sigma = (24.0 * step).reciprocal()
    lam_t, lam_s = 0.02 * peak_t, 0.01 * peak_s
    assert torch.equal(classical.total_variation(mk, mask, sens, iters=ITERS, lam_t=lam_t, lam_s=lam_s, step=step, sigma=sigma), x)
    assert torch.equal(classical.TotalVariation(iters=ITERS, lam_t=lam_t, lam_s=lam_s, step=step, sigma=sigma).eval()(mk, mask, sens), x)
    assert torch.equal(classical.total_variation(mk, mask, sens, iters=ITERS, step=float(step), sigma=float(sigma)), x)   # floats are the values
    assert torch.equal(classical.total_variation(mk, mask, sens, iters=ITERS, lam_t=lam_t), x)             # a fraction and a weight mixed
    # record and dual: the documented shapes and order
    x2, dual, rec = classical.total_variation(mk, mask, sens, iters=7, record=True, dual=True, output="complex")
    assert x2.shape == (b, t, h, w, 2) and dual.shape == (3, b, t, h, w, 2) and rec.shape == (7, 4) and bool((rec > 0).all())
    x3, rec3 = classical.total_variation(mk, mask, sens, iters=7, record=True, output="complex")
    x4, dual4 = classical.total_variation(mk, mask, sens, iters=7, dual=True, output="complex")
    assert torch.equal(x3, x2) and torch.equal(x4, x2) and torch.equal(rec3, rec) and torch.equal(dual4, dual)
    mag_t, mag_s = (dual[0] ** 2).sum(-1).sqrt(), ((dual[1] ** 2).sum(-1) + (dual[2] ** 2).sum(-1)).sqrt()
    assert float(mag_t.max()) <= float(lam_t) * (1 + 1e-5) and float(mag_s.max()) <= float(lam_s) * (1 + 1e-5)        # the dual lies in its balls
    # one term off: its dual planes are zeros, its record column too, and the result differs
    xt, dual_t, rec_t = classical.total_variation(mk, mask, sens, iters=7, lam_s=0.0, record=True, dual=True, output="complex")
    xs, dual_s, rec_s = classical.total_variation(mk, mask, sens, iters=7, lam_t=0.0, record=True, dual=True, output="complex")
    assert not dual_t[1:].any() and bool(dual_t[0].any()) and not rec_t[:, 3].any() and bool((rec_t[:, :3] > 0).all())
    assert not dual_s[0].any() and bool(dual_s[1:].any()) and not rec_s[:, 2].any()
    assert not torch.equal(xt, x2) and not torch.equal(xs, x2)
    assert not torch.equal(classical.total_variation(mk, mask, sens, iters=7, periodic=False, output="complex"), x2)
    # against the float64 iteration with the same settings
    tau = K.default_step(p["s"])
    want_t, want_s = R.peaks(p["zf"], True)
    want, _, _ = R.solve(p["zf"], p["s"], p["m"], tau, R.default_sigma(tau, 3), 0.02 * want_t, 0.01 * want_s, ITERS)
    err = float(np.abs(K.to_complex(xc) - want).max() / np.abs(want).max())
    print(f"total_variation {layout}: {err:.3e} of the float64 peak (bar {BAR_CAP:.0e})")
    assert err <= BAR_CAP


def test_the_reconstruction_beats_the_zero_filled_image(dev):
    """The yardstick's own figure is 0.51 of the zero-filled NRMSE after 30 iterations on this problem (test_tv_cpu.py asserts <= 0.6)."""
    from cine_hip import classical
    p, mk, mask, sens = inputs(dev)
    truth = p["target"].numpy()
    got = K.nrmse(classical.total_variation(mk, mask, sens, iters=ITERS).cpu().numpy(), truth)
    zero_filled = K.nrmse(np.abs(p["zf"]), truth)
    print(f"NRMSE against the phantom: TV {got:.3f}, zero-filled {zero_filled:.3f} ({got / zero_filled:.2f} of it)")
    assert got <= 0.6 * zero_filled


def test_pipeline_submit(dev):
    """Slots 2, graphs: four slices over two masks; every output equals the eager call."""
    from cine_hip import classical
    from cine_hip.pipeline import SlicePipeline
    model = classical.TotalVariation(iters=10).eval()
    for layout in ("row", "plane"):
        probs = [K.problem(SHAPE, layout, seed=s) for s in (0, 3)]
        ins = []
        for j in range(4):
            q = probs[j % 2]
            ins.append(((q["masked_kspace"] * (1.0 + 0.25 * j)).to(dev), q["mask"].to(dev), q["sens_maps"].to(dev)))
        want = [model(*a).clone() for a in ins]
        assert not torch.equal(want[0], want[1]) and all(bool(torch.isfinite(v).all()) for v in want)
        with SlicePipeline(model, slots=2) as pipe:
            assert pipe.graphs
            for j, a in enumerate(ins):
                pipe.submit(*a, tag=j)
            got = dict(pipe.drain())
            assert pipe.set_builds == 1
        for j in range(4):
            assert torch.equal(got[j], want[j]), (layout, j)


def test_pipeline_submit_raw_with_espirit_maps_in_flight(dev):
    """Raw scans in, maps calibrated in flight, at the shape of test_espirit_sign.py's raw-pipeline tests."""
    from cine_hip import classical, frontend as FE, ops
    from cine_hip.pipeline import SlicePipeline
    T, C, N, r = 5, 6, 64, 12
    raw_shape, crop, fs = (T, 72, 68, C), (N, N), (0.7, 0.0, 0.3, 0.3)
    model = classical.TotalVariation(iters=10).eval()
    raws, masks = [], []
    for j in range(2):
        rs = np.random.RandomState(50 + j)
        t, nx, ny, c = raw_shape
        x, y = np.arange(nx)[:, None] - nx // 2, np.arange(ny)[None, :] - ny // 2
        wgt = np.exp(-(x * x / (2.0 * (nx / 8.0) ** 2) + y * y / (2.0 * (ny / 8.0) ** 2))) + 0.02
        z = rs.standard_normal(raw_shape) + 1j * rs.standard_normal(raw_shape)
        raws.append(torch.from_numpy((1e-6 * z * wgt[None, :, :, None]).astype(np.complex64)).to(dev))
        m = (np.random.RandomState(1000 + j).uniform(size=(1, T, 1, N, 1, 1)) < 0.3).astype(np.uint8)
        m[:, :, :, N // 2 - 5:N // 2 + 5] = 1
        masks.append(torch.from_numpy(m).to(dev))
    want = []
    with torch.no_grad(), ops.branches(1):
        for raw, mask in zip(raws, masks):
            mk = FE.prepare_masked_slice(raw, mask, crop, T, fs, 1e6)
            maps = torch.stack([FE.espirit_maps(FE.time_average(mk[i]), r=r, method="sign")[0] for i in range(mk.shape[0])])[:, None]
            want.append(model(mk, mask, maps).clone())
    with SlicePipeline(model, slots=2) as pipe:
        for j in range(2):
            pipe.submit_raw(raws[j], masks[j], "espirit", tag=j, crop_shape=crop, n_frames=T, ecalib_r=r)
        got = dict(pipe.drain())
    assert not torch.equal(want[0], want[1])
    for j in range(2):
        assert bool(torch.isfinite(want[j]).all()) and torch.equal(got[j], want[j]), j
