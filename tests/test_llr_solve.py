"""cine_llr_solve (the whole locally low-rank solve in one C call) against tests/llr_reference.py in float64: (1, 5, 3, 24, 20) with a row
mask and (2, 15, 4, 32, 28) with a mask that varies along w, 30 iterations, 8 x 8 blocks, the default step 1 / max sum |S_c|^2,
lam = 0.005 of the largest block singular value of zf -- with the seed-0 shifts and once with shifts = NULL (the fixed partition).

Bars: x within kernel_sweep.BAR_CAP = 1e-4 of the float64 peak, the bar cine_ls_solve and cine_kt_fista hold (with the default step the
iteration map is non-expansive, so float32 errors add and do not grow); the record within REC_REL = 1e-4 relative; every Jacobi residual
<= 1e-14, sweeps below the cap, the block count of each iteration's shift exact.  Equal bits for x, rec and info: the C driver against the
binding's own loop over ops.image_dc and ops.llr_prox, against ops.llr_solve, two calls of the driver, and a captured graph replayed twice."""
import ctypes

import numpy as np
import pytest
import torch

import kt_reference as R
import llr_reference as LLR
from kernel_sweep import BAR_CAP, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
ITERS, BLOCK, REC_REL = LLR.ITERS, LLR.BLOCK, 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def setup(shape, layout):
    p, zf32, step, thresh = LLR.settings(shape, layout)
    return p, torch.from_numpy(zf32), step, thresh


def host_shifts(seq):
    return None if seq is None else (ctypes.c_int * seq.size)(*[int(v) for v in seq.reshape(-1)])


def solve_call(k, p, zf, step, thresh, shape, layout, seq, iters=ITERS, record=True):
    b, t, c, h, w = shape
    mask_w = 1 if layout == "row" else w
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    st, th = k.raw(torch.tensor([step])), k.raw(torch.tensor([thresh]))
    x = k.out((b, t, h, w, 2))
    rec, info = (k.out((iters, 4)), k.out((iters, 8))) if record else (None, None)                  # info: doubles, seen as float pairs
    nbytes = L().cine_llr_solve_ws_bytes(b, t, c, h, w, mask_w, BLOCK, iters)
    ws = k.ws(nbytes)
    check(L().cine_llr_solve(x.ptr(), ptr(zi), ptr(si), None, ptr(mi), mask_w, ptr(st), ptr(th), BLOCK, host_shifts(seq), iters,
                             rec.ptr() if rec else None, info.ptr() if info else None, b, t, c, h, w, ws.ptr(), nbytes, stream()), "cine_llr_solve")
    return [x.t] + ([rec.t, info.t] if record else [])


def check_solve(dev, shape, layout, shifted, everything):
    from cine_hip import ops
    b, t, c, h, w = shape
    p, zf, step, thresh = setup(shape, layout)
    seq = LLR.shifts(ITERS, BLOCK, 0) if shifted else None
    want_x, want_rec, _ = LLR.solved(shape, layout, shifted=shifted)
    what = f"cine_llr_solve {shape} {layout} {'seed-0 shifts' if shifted else 'shifts = NULL'}"
    x, rec, info = twice(dev, 0, lambda k: solve_call(k, p, zf, step, thresh, shape, layout, seq), what)      # two solves: equal bits
    info = info.contiguous().view(torch.float64).numpy().reshape(ITERS, 4)
    ex = float(np.abs(R.to_complex(x) - want_x).max() / np.abs(want_x).max())
    er = float((np.abs(rec.double().numpy()[:, :3] - want_rec[:, :3]) / want_rec[:, :3]).max())
    print(f"{what}: x {ex:.3e} of the float64 peak (bar {BAR_CAP:.0e}), record {er:.3e} relative (bar {REC_REL:.0e}), worst Jacobi residual "
          f"{info[:, 1].max():.1e}, at most {int(info[:, 2].max())} sweeps")
    assert ex <= BAR_CAP and er <= REC_REL and not rec[:, 3].any(), what
    assert np.all(info[:, 1] <= 1e-14) and np.all(info[:, 2] < 40) and np.all(info[:, 0] > 0), info
    blocks = [b * len(LLR.blocks(h, w, BLOCK, *((0, 0) if seq is None else seq[k]))) for k in range(ITERS)]
    assert np.array_equal(info[:, 3], blocks), (info[:, 3], blocks)
    # the binding's own loop over the entry points
    zf_d, sens_d, mask_d = zf.to(dev).unsqueeze(2), p["sens_maps"].to(dev), p["mask"].to(dev)
    st, th = torch.tensor([step], device=dev), torch.tensor([thresh], device=dev)
    xk, rows, infos = zf_d, [], []
    for k in range(ITERS):
        g = ops.image_dc(xk, sens_d, zf_d, mask_d, weights=(1.0, 0.0, -1.0))
        xk, r, f = ops.llr_prox(xk, g, st, th, BLOCK, (0, 0) if seq is None else tuple(int(v) for v in seq[k]), record=True)
        rows.append(r.cpu()); infos.append(f.cpu())
    assert same_bits(xk.squeeze(2).cpu(), x), what + ": the hand-rolled loop gives other bits"
    assert same_bits(torch.stack(rows), rec) and np.array_equal(torch.stack(infos).numpy(), info), what + ": the hand-rolled loop gives other records"
    # the binding of the driver, with and without the records
    xb, rb, fb = ops.llr_solve(zf_d, sens_d, mask_d, st, th, BLOCK, ITERS, shifts=seq, record=True)
    assert xb.shape == zf_d.shape and same_bits(xb.squeeze(2).cpu(), x) and same_bits(rb.cpu(), rec) and np.array_equal(fb.cpu().numpy(), info)
    if not everything:
        return
    assert same_bits(ops.llr_solve(zf_d, sens_d, mask_d, st, th, BLOCK, ITERS, shifts=seq).squeeze(2).cpu(), x)
    k = Call(dev, 0)
    (x_only,) = solve_call(k, p, zf, step, thresh, shape, layout, seq, record=False)
    k.finish(what + " without the records")
    assert same_bits(x_only.cpu(), x)
    # captured on one stream and replayed twice: the shifts are read at capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xg, rg, _ = ops.llr_solve(zf_d, sens_d, mask_d, st, th, BLOCK, ITERS, shifts=seq, record=True)
    for _ in range(2):
        xg.zero_(); rg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(xg.squeeze(2).cpu(), x) and same_bits(rg.cpu(), rec), what + ": the replayed graph gives other bits"


@pytest.mark.parametrize("shape,layout", LLR.FIXTURES, ids=["row", "plane"])
def test_solve_with_seeded_shifts_vs_float64_and_the_hand_rolled_loop(dev, shape, layout):
    check_solve(dev, shape, layout, shifted=True, everything=True)


@pytest.mark.parametrize("shape,layout", LLR.FIXTURES, ids=["row", "plane"])
def test_solve_with_a_fixed_partition_vs_float64_and_the_hand_rolled_loop(dev, shape, layout):
    check_solve(dev, shape, layout, shifted=False, everything=False)


def test_one_iteration_is_one_gradient_step_and_one_prox(dev):
    shape, layout = LLR.FIXTURES[0]
    p, zf, step, thresh = setup(shape, layout)
    seq = np.array([[3, 5]], dtype=np.int32)
    x, rec, info = twice(dev, 0, lambda k: solve_call(k, p, zf, step, thresh, shape, layout, seq, iters=1), "cine_llr_solve")
    z64 = R.to_complex(zf)
    want_x, want_rec, _ = LLR.prox(z64, R.gradient(z64, p["s"], p["m"], z64), step, thresh, BLOCK, 3, 5)
    assert float(np.abs(R.to_complex(x) - want_x).max() / np.abs(want_x).max()) <= BAR_CAP
    assert rec.shape == (1, 4) and float((np.abs(rec[0].double().numpy()[:3] - want_rec[:3]) / want_rec[:3]).max()) <= REC_REL


def test_refusals_come_before_anything_is_written(dev):
    shape, layout = LLR.FIXTURES[0]
    b, t, c, h, w = shape
    p, zf, step, thresh = setup(shape, layout)
    k = Call(dev, 0)
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    st, th = k.raw(torch.tensor([step])), k.raw(torch.tensor([thresh]))
    x, rec, info = k.out((b, t, h, w, 2)), k.out((3, 4)), k.out((3, 8))
    need = L().cine_llr_solve_ws_bytes(b, t, c, h, w, 1, BLOCK, 3)
    assert need > L().cine_llr_solve_ws_bytes(b, t, c, h, w, 1, BLOCK, 2) > zf.numel() * 4 and L().cine_llr_solve_ws_bytes(b, t, c, h, w, 1, BLOCK, 0) == 0
    ws = k.ws(need)
    good = (ctypes.c_int * 6)(1, 2, 0, 0, 7, 7)
    base = dict(x=x.ptr(), zf=ptr(zi), sens=ptr(si), mask=ptr(mi), mask_w=1, step=ptr(st), thresh=ptr(th), block=BLOCK, shifts=good, iters=3,
                rec=rec.ptr(), info=info.ptr(), b=b, t=t, c=c, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_llr_solve(a["x"], a["zf"], a["sens"], None, a["mask"], a["mask_w"], a["step"], a["thresh"], a["block"], a["shifts"],
                                          a["iters"], a["rec"], a["info"], a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"], a["nbytes"], stream())
    refused(call(iters=0), EINVAL, k, "cine_llr_solve iters = 0")
    refused(call(t=1), EUNSUPPORTED, k, "cine_llr_solve t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_llr_solve t = 65")
    refused(call(block=17), EUNSUPPORTED, k, "cine_llr_solve block = 17")
    refused(call(block=1), EUNSUPPORTED, k, "cine_llr_solve block = 1")
    refused(call(h=401, nbytes=1 << 30), EUNSUPPORTED, k, "cine_llr_solve h = 401 (the operator's refusal)")
    for n in ("x", "zf", "sens", "mask", "step", "thresh", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_llr_solve {n} = NULL")
    refused(call(shifts=(ctypes.c_int * 6)(1, 2, 0, 0, 7, 8)), EINVAL, k, "cine_llr_solve a bad entry in the last row of shifts")
    refused(call(shifts=(ctypes.c_int * 6)(-1, 2, 0, 0, 7, 7)), EINVAL, k, "cine_llr_solve a negative shift")
    refused(call(c=0), EINVAL, k, "cine_llr_solve c = 0")
    refused(call(mask_w=2), EINVAL, k, "cine_llr_solve mask_w = 2")
    refused(call(x=base["zf"]), EINVAL, k, "cine_llr_solve x aliases zf")
    refused(call(rec=base["x"]), EINVAL, k, "cine_llr_solve rec aliases x")
    refused(call(info=base["rec"]), EINVAL, k, "cine_llr_solve info aliases rec")
    refused(call(ws=base["ws"] + 8), EINVAL, k, "cine_llr_solve ws off a 16-byte boundary")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_llr_solve a workspace one byte short")
    check(call()(), "cine_llr_solve")
    k.finish("cine_llr_solve")
    assert bool(torch.isfinite(x.t).all()) and bool(torch.isfinite(rec.t).all()) and bool(torch.isfinite(info.t.view(torch.float64)).all())
