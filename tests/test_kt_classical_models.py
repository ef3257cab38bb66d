"""cine_hip.classical on the GPU: kt_sparse_sense / KtSparseSense eagerly, and KtSparseSense through SlicePipeline with graphs -- k-space
input, maps calibrated in flight (sens_maps="espirit") and raw input -- bit for bit against the eager calls."""
import numpy as np
import pytest
import torch

import kt_reference as R
from kernel_sweep import BAR_CAP

pytestmark = pytest.mark.gpu
SHAPE = (1, 5, 3, 24, 20)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def inputs(dev, layout="row", shape=SHAPE):
    p = R.problem(shape, layout)
    return p, p["masked_kspace"].to(dev), p["mask"].to(dev), p["sens_maps"].to(dev)


@pytest.mark.parametrize("layout", ["row", "plane"])
def test_module_function_outputs_and_explicit_settings(dev, layout):
    from cine_hip import classical, dc, ops
    p, mk, mask, sens = inputs(dev, layout)
    b, t, c, h, w = SHAPE
    x = classical.kt_sparse_sense(mk, mask, sens)
    assert x.shape == (b, t, h, w) and bool(torch.isfinite(x).all())
    assert torch.equal(classical.KtSparseSense().eval()(mk, mask, sens), x)                       # the module is the function
    assert torch.equal(classical.kt_sparse_sense(mk, mask.float(), sens), x)                      # any numeric 0 / 1 mask, as the models take
    xc = classical.kt_sparse_sense(mk, mask, sens, output="complex")
    assert xc.shape == (b, t, h, w, 2) and torch.equal(ops.complex_abs(xc), x)
    assert torch.equal(classical.KtSparseSense().eval()(mk, mask, sens, output="complex"), xc)
    # the defaults computed by hand and passed as absolute device values
    step = 1.0 / (sens * sens).sum(dim=(2, 5)).amax().reshape(1)
    zf = dc.Acquisition(mk, mask, sens).zero_filled()                                              # A^H M y
    xf = ops.fft1c(zf.reshape(b, t, h * w, 2).permute(0, 2, 1, 3).contiguous())
    lam = 0.02 * (xf * xf).sum(dim=-1).amax().sqrt().reshape(1)
    assert abs(float(step) - R.default_step(p["s"])) <= 1e-6 * R.default_step(p["s"])
    peak = np.abs(R.fft1c(p["zf"], 1)).max()
    assert abs(float(lam) - 0.02 * peak) <= 1e-5 * 0.02 * peak
    assert torch.equal(classical.kt_sparse_sense(mk, mask, sens, step=step, lam=lam), x)
    assert torch.equal(classical.KtSparseSense(step=step, lam=lam).eval()(mk, mask, sens), x)
    assert torch.equal(classical.kt_sparse_sense(mk, mask, sens, step=float(step)), x)            # a float step is the value itself
    x2, rec = classical.kt_sparse_sense(mk, mask, sens, iters=7, record=True, penalise_dc=False)
    assert rec.shape == (7, 4) and bool((rec[:, :3] > 0).all()) and not torch.equal(x2, x)
    # against the float64 iteration with the same settings
    want, _ = R.fista(p["zf"], p["s"], p["m"], R.default_step(p["s"]), 0.02 * peak, 30, True)
    err = float(np.abs(R.to_complex(xc) - want).max() / np.abs(want).max())
    print(f"kt_sparse_sense {layout}: {err:.3e} of the float64 peak (bar {BAR_CAP:.0e})")
    assert err <= BAR_CAP


def test_the_reconstruction_beats_the_zero_filled_image(dev):
    from cine_hip import classical
    p, mk, mask, sens = inputs(dev)
    truth = p["target"].numpy()
    got = R.nrmse(classical.kt_sparse_sense(mk, mask, sens).cpu().numpy(), truth)
    zero_filled = R.nrmse(np.abs(p["zf"]), truth)
    print(f"NRMSE against the phantom: k-t SPARSE-SENSE {got:.3f}, zero-filled {zero_filled:.3f}")
    assert got < zero_filled


def _drain(pipe):
    return dict(pipe.drain())


def test_pipeline_four_slices_two_masks(dev):
    """Slots 2, graphs: slices alternate between two masks (and differ in their data); every output equals the eager call."""
    from cine_hip import classical
    from cine_hip.pipeline import SlicePipeline
    model = classical.KtSparseSense(iters=8).eval()
    for layout in ("row", "plane"):
        probs = [R.problem(SHAPE, layout, seed=s) for s in (0, 3)]
        assert not torch.equal(probs[0]["mask"], probs[1]["mask"])
        ins = []
        for j in range(4):
            q = probs[j % 2]
            ins.append(((q["masked_kspace"] * (1.0 + 0.25 * j)).to(dev), q["mask"].to(dev), q["sens_maps"].to(dev)))
        want = [model(*a).clone() for a in ins]
        assert not torch.equal(want[0], want[1])
        with SlicePipeline(model, slots=2) as pipe:
            assert pipe.graphs
            for j, a in enumerate(ins):
                pipe.submit(*a, tag=j)
            got = _drain(pipe)
            assert pipe.set_builds == 1
        for j in range(4):
            assert torch.equal(got[j], want[j]), (layout, j)


def test_pipeline_espirit_maps_in_flight(dev):
    from cine_hip import classical, frontend as FE, ops, synth
    from cine_hip.pipeline import SlicePipeline
    T, C, N, r = 5, 6, 64, 12
    model = classical.KtSparseSense(iters=5).eval()
    exs = [synth.make_cine_slice(T, C, N, N, accel=4, center_lines=10, seed=10 + j) for j in range(2)]
    ins = [(ex["masked_kspace"].to(dev), ex["mask"].to(torch.uint8).to(dev)) for ex in exs]
    want = []
    with torch.no_grad(), ops.branches(1):
        for mk, mask in ins:
            maps = torch.stack([FE.espirit_maps(FE.time_average(mk[i]), r=r, method="sign")[0] for i in range(mk.shape[0])])[:, None]
            want.append(model(mk, mask, maps).clone())
    with SlicePipeline(model, slots=2) as pipe:
        for j, (mk, mask) in enumerate(ins):
            pipe.submit(mk, mask, "espirit", tag=j, ecalib_r=r)
        got = _drain(pipe)
    for j in range(2):
        assert bool(torch.isfinite(want[j]).all()) and torch.equal(got[j], want[j]), j


def test_pipeline_submit_raw(dev):
    from cine_hip import classical, frontend as FE, synth
    from cine_hip.pipeline import SlicePipeline
    raw_shape, crop, frames, fs = (7, 30, 28, 3), (24, 20), 5, (0.7, 0.0, 0.3, 0.3)
    model = classical.KtSparseSense(iters=5).eval()
    sens = synth.make_cine_slice(frames, 3, crop[0], crop[1], accel=4, center_lines=4, seed=70)["sens_maps"].contiguous().to(dev)
    raws, masks = [], []
    for j in range(2):
        rs = np.random.RandomState(50 + j)
        t, nx, ny, c = raw_shape
        x, y = np.arange(nx)[:, None] - nx // 2, np.arange(ny)[None, :] - ny // 2
        wgt = np.exp(-(x * x / (2.0 * (nx / 8.0) ** 2) + y * y / (2.0 * (ny / 8.0) ** 2))) + 0.02
        z = rs.standard_normal(raw_shape) + 1j * rs.standard_normal(raw_shape)
        raws.append(torch.from_numpy((1e-6 * z * wgt[None, :, :, None]).astype(np.complex64)).to(dev))
        m = (np.random.RandomState(1000 + j).uniform(size=(1, frames, 1, crop[0], 1, 1)) < 0.3).astype(np.uint8)
        m[:, :, :, crop[0] // 2 - 2:crop[0] // 2 + 2] = 1
        masks.append(torch.from_numpy(m).to(dev))
    want = []
    with torch.no_grad():
        for raw, mask in zip(raws, masks):
            want.append(model(FE.prepare_masked_slice(raw, mask, crop, frames, fs, 1e6), mask, sens).clone())
    with SlicePipeline(model, slots=2) as pipe:
        for j in range(2):
            pipe.submit_raw(raws[j], masks[j], sens, tag=j, crop_shape=crop, n_frames=frames)
        got = _drain(pipe)
    assert not torch.equal(want[0], want[1])
    for j in range(2):
        assert torch.equal(got[j], want[j]), j
