"""cine_hip.classical's locally low-rank baseline on the GPU: locally_low_rank / LocallyLowRank eagerly, and LocallyLowRank through
SlicePipeline with graphs -- k-space input, and raw input with the maps calibrated in flight (sens_maps="espirit") -- bit for bit against
the eager calls."""
import numpy as np
import pytest
import torch

import kt_reference as R
import llr_reference as LLR
from kernel_sweep import BAR_CAP

pytestmark = pytest.mark.gpu
SHAPE, LAYOUT = LLR.FIXTURES[1]                    # (2, 15, 4, 32, 28), a mask that varies along w


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def inputs(dev, shape=SHAPE, layout=LAYOUT, seed=0):
    p = R.problem(shape, layout, seed)
    return p, p["masked_kspace"].to(dev), p["mask"].to(dev), p["sens_maps"].to(dev)


def test_the_reconstruction_beats_the_zero_filled_image_and_matches_the_float64_solve(dev):
    from cine_hip import classical, dc, ops
    p, mk, mask, sens = inputs(dev)
    b, t, c, h, w = SHAPE
    truth = p["target"].numpy()
    x = classical.locally_low_rank(mk, mask, sens)                                                          # 30 iterations, 8 x 8, seed-0 shifts
    assert x.shape == (b, t, h, w) and bool(torch.isfinite(x).all())
    got, zero_filled = R.nrmse(x.cpu().numpy(), truth), R.nrmse(np.abs(p["zf"]), truth)
    print(f"NRMSE against the phantom: LLR {got:.3f}, zero-filled {zero_filled:.3f} ({got / zero_filled:.2f} of it; the float64 yardstick 0.50)")
    assert got <= 0.6 * zero_filled                                                                         # the condition of test_llr_cpu.py
    assert torch.equal(classical.LocallyLowRank().eval()(mk, mask, sens), x)                                # the module is the function
    assert torch.equal(classical.locally_low_rank(mk, mask.float(), sens), x)                               # any numeric 0 / 1 mask
    assert torch.equal(classical.locally_low_rank(mk, mask, sens, shifts=classical.llr_shifts(LLR.ITERS, LLR.BLOCK, 0)), x)
    xc = classical.locally_low_rank(mk, mask, sens, output="complex")
    assert xc.shape == (b, t, h, w, 2) and torch.equal(ops.complex_abs(xc), x)
    fixed = classical.locally_low_rank(mk, mask, sens, shifts=None)
    assert torch.equal(classical.locally_low_rank(mk, mask, sens, shifts="fixed"), fixed) and not torch.equal(fixed, x)
    # the defaults computed on the host in float64 and passed as absolute device values: within the float32 solve's bar of the yardstick
    _, _, step, thresh = LLR.settings(SHAPE, LAYOUT)
    zf = dc.Acquisition(mk, ops.as_mask_u8(mask, mk), sens).zero_filled()
    ref = LLR.block_sigma_max(p["zf"], LLR.BLOCK)
    assert abs(float(classical.block_sigma_max(zf, LLR.BLOCK)) - ref) <= 1e-5 * ref
    st, th = torch.tensor([step], device=dev), torch.tensor([thresh], device=dev)
    xa, rec, info = classical.locally_low_rank(mk, mask, sens, lam=th, step=st, output="complex", record=True)
    assert rec.shape == (LLR.ITERS, 4) and info.shape == (LLR.ITERS, 4) and info.dtype == torch.float64
    assert bool((rec[:, :3] > 0).all()) and float(info[:, 1].max()) <= 1e-14 and float(info[:, 2].max()) < 40
    want, _, _ = LLR.solved(SHAPE, LAYOUT)
    e = float(np.abs(R.to_complex(xa) - want).max() / np.abs(want).max())
    print(f"locally_low_rank: {e:.3e} of the float64 peak (bar {BAR_CAP:.0e})")
    assert e <= BAR_CAP
    assert float((xa - xc).abs().max() / xc.abs().max()) <= BAR_CAP                                         # the fraction formed on the device


@pytest.mark.parametrize("slots", [2, 3], ids=lambda s: f"slots{s}")
def test_pipeline_submit(dev, slots):
    """Graphs: four slices over two masks; every output equals the eager call, the replayed graphs replay the same shifts."""
    from cine_hip import classical
    from cine_hip.pipeline import SlicePipeline
    model = classical.LocallyLowRank(iters=10).eval()
    shape = (1, 5, 3, 24, 20)
    for layout in ("row", "plane"):
        probs = [R.problem(shape, layout, seed=s) for s in (0, 3)]
        ins = []
        for j in range(4):
            q = probs[j % 2]
            ins.append(((q["masked_kspace"] * (1.0 + 0.25 * j)).to(dev), q["mask"].to(dev), q["sens_maps"].to(dev)))
        want = [model(*a).clone() for a in ins]
        assert not torch.equal(want[0], want[1]) and all(bool(torch.isfinite(v).all()) for v in want)
        with SlicePipeline(model, slots=slots) as pipe:
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
    model = classical.LocallyLowRank(iters=10).eval()
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
