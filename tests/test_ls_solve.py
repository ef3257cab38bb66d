"""cine_ls_solve (the whole low-rank plus sparse solve in one C call) against tests/ls_reference.py in float64: (1, 5, 3, 24, 20) with a row
mask and (2, 15, 4, 32, 28) with a mask that varies along w, 30 iterations, the default step 0.5 / max sum |S_c|^2, lam_l = 0.01 sigma_max,
lam_s = 0.01 max |F_t zf|.

Bars: x within kernel_sweep.BAR_CAP = 1e-4 of the float64 peak, the bar cine_kt_fista holds (with the default step the iteration map is
non-expansive, so float32 errors add and do not grow); the record, the nuclear norm in column 3 included, within REC_REL = 1e-4 relative;
every Jacobi residual <= 1e-14.  Equal bits for x, L, S and the record: the C driver against the binding's own loop over ops.image_dc,
ops.casorati_gram, ops.svt_weight and ops.ls_prox, against ops.ls_solve, two calls of the driver, and a captured graph replayed twice."""
import numpy as np
import pytest
import torch

import kt_reference as R
import ls_reference as LS
from kernel_sweep import BAR_CAP, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
ITERS, REC_REL = LS.ITERS, 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def setup(shape, layout):
    p, zf32, step, thl, ths = LS.settings(shape, layout)
    return p, torch.from_numpy(zf32), step, thl, ths


def solve_call(k, p, zf, step, thl, ths, shape, layout, iters=ITERS, components=True, record=True):
    b, t, c, h, w = shape
    mask_w = 1 if layout == "row" else w
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    st, tl, ts = k.raw(torch.tensor([step])), k.raw(torch.tensor([thl])), k.raw(torch.tensor([ths]))
    x = k.out((b, t, h, w, 2))
    lo, so = (k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2))) if components else (None, None)
    rec, resid = (k.out((iters, 4)), k.out((iters, 2))) if record else (None, None)                 # resid: doubles, seen as float pairs
    nbytes = L().cine_ls_solve_ws_bytes(b, t, c, h, w, mask_w, iters)
    ws = k.ws(nbytes)
    check(L().cine_ls_solve(x.ptr(), lo.ptr() if lo else None, so.ptr() if so else None, ptr(zi), ptr(si), None, ptr(mi), mask_w, ptr(st), ptr(tl),
                            ptr(ts), iters, rec.ptr() if rec else None, resid.ptr() if resid else None, b, t, c, h, w, ws.ptr(), nbytes, stream()),
          "cine_ls_solve")
    return [x.t] + ([lo.t, so.t] if components else []) + ([rec.t, resid.t] if record else [])


@pytest.mark.parametrize("shape,layout", LS.FIXTURES, ids=["row", "plane"])
def test_solve_vs_float64_and_the_hand_rolled_loop(dev, shape, layout):
    from cine_hip import ops
    b, t, c, h, w = shape
    p, zf, step, thl, ths = setup(shape, layout)
    want_l, want_s, want_rec, _ = LS.solved(shape, layout)
    what = f"cine_ls_solve {shape} {layout}"
    x, lo, so, rec, resid = twice(dev, 0, lambda k: solve_call(k, p, zf, step, thl, ths, shape, layout), what)          # two solves: equal bits
    resid = resid.contiguous().view(torch.float64).numpy().reshape(ITERS)
    peak = np.abs(want_l + want_s).max()
    ex = float(np.abs(R.to_complex(x) - (want_l + want_s)).max() / peak)
    el, es = float(np.abs(R.to_complex(lo) - want_l).max() / peak), float(np.abs(R.to_complex(so) - want_s).max() / peak)
    er = float((np.abs(rec.double().numpy() - want_rec) / want_rec).max())
    print(f"{what}: x {ex:.3e}, L {el:.3e}, S {es:.3e} of the float64 peak (bar {BAR_CAP:.0e}), record {er:.3e} relative (bar {REC_REL:.0e}), "
          f"worst Jacobi residual {resid.max():.1e}")
    assert max(ex, el, es) <= BAR_CAP and er <= REC_REL, what
    assert np.all(resid <= 1e-14), resid
    # the binding's own loop over the entry points
    zf_d, sens_d, mask_d = zf.to(dev).unsqueeze(2), p["sens_maps"].to(dev), p["mask"].to(dev)
    st, tl, ts = (torch.tensor([v], device=dev) for v in (step, thl, ths))
    lk, sk, xk = zf_d, torch.zeros_like(zf_d), zf_d
    rows = []
    for _ in range(ITERS):
        g = ops.image_dc(xk, sens_d, zf_d, mask_d, weights=(1.0, 0.0, -1.0))
        wgt, info = ops.svt_weight(ops.casorati_gram(lk, g, st), tl, st)
        lk, sk, xk, r = ops.ls_prox(lk, sk, g, wgt, st, ts, record=True)
        nuc = 0.0
        for v in info[:, 1].tolist():                   # the batch in order, in double, as the record kernel adds them
            nuc += v
        rows.append(torch.cat((r[:3].cpu(), torch.tensor([nuc], dtype=torch.float64).float())))
    assert same_bits(xk.squeeze(2).cpu(), x) and same_bits(lk.squeeze(2).cpu(), lo) and same_bits(sk.squeeze(2).cpu(), so), \
        what + ": the hand-rolled loop gives other bits"
    assert same_bits(torch.stack(rows), rec), what + ": the hand-rolled loop gives another record"
    # the binding of the driver, with and without the extras
    xb, lb, sb, rb, qb = ops.ls_solve(zf_d, sens_d, mask_d, st, tl, ts, ITERS, components=True, record=True)
    assert xb.shape == zf_d.shape and same_bits(xb.squeeze(2).cpu(), x) and same_bits(lb.squeeze(2).cpu(), lo) and same_bits(sb.squeeze(2).cpu(), so)
    assert same_bits(rb.cpu(), rec) and np.array_equal(qb.cpu().numpy(), resid)
    assert same_bits(ops.ls_solve(zf_d, sens_d, mask_d, st, tl, ts, ITERS).squeeze(2).cpu(), x)
    k = Call(dev, 0)
    (x_only,) = solve_call(k, p, zf, step, thl, ths, shape, layout, components=False, record=False)
    k.finish(what + " without components and record")
    assert same_bits(x_only.cpu(), x)
    # captured on one stream and replayed twice
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        xg, rg, _ = ops.ls_solve(zf_d, sens_d, mask_d, st, tl, ts, ITERS, record=True)
    for _ in range(2):
        xg.zero_(); rg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(xg.squeeze(2).cpu(), x) and same_bits(rg.cpu(), rec), what + ": the replayed graph gives other bits"


def test_one_iteration_is_one_gradient_step_and_one_prox(dev):
    shape, layout = LS.FIXTURES[0]
    p, zf, step, thl, ths = setup(shape, layout)
    x, lo, so, rec, _ = twice(dev, 0, lambda k: solve_call(k, p, zf, step, thl, ths, shape, layout, iters=1), "cine_ls_solve")
    z64 = R.to_complex(zf)
    want_l, want_s, want_rec = LS.ls_iteration(z64, np.zeros_like(z64), z64, p["s"], p["m"], step, thl, ths)
    peak = np.abs(want_l + want_s).max()
    assert float(np.abs(R.to_complex(lo) - want_l).max() / peak) <= BAR_CAP and float(np.abs(R.to_complex(so) - want_s).max() / peak) <= BAR_CAP
    assert rec.shape == (1, 4) and float((np.abs(rec[0].double().numpy() - want_rec) / want_rec).max()) <= REC_REL
    assert same_bits(lo + so, x)                                               # x is the float32 sum of the components


def test_refusals_come_before_anything_is_written(dev):
    shape, layout = LS.FIXTURES[0]
    b, t, c, h, w = shape
    p, zf, step, thl, ths = setup(shape, layout)
    k = Call(dev, 0)
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    st, tl, ts = k.raw(torch.tensor([step])), k.raw(torch.tensor([thl])), k.raw(torch.tensor([ths]))
    x, lo, so, rec, resid = k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2)), k.out((3, 4)), k.out((3, 2))
    need = L().cine_ls_solve_ws_bytes(b, t, c, h, w, 1, 3)
    assert need > L().cine_ls_solve_ws_bytes(b, t, c, h, w, 1, 2) > 3 * zf.numel() * 4 and L().cine_ls_solve_ws_bytes(b, t, c, h, w, 1, 0) == 0
    ws = k.ws(need)
    base = dict(x=x.ptr(), l=lo.ptr(), s=so.ptr(), zf=ptr(zi), sens=ptr(si), mask=ptr(mi), mask_w=1, step=ptr(st), thresh_l=ptr(tl), thresh_s=ptr(ts),
                iters=3, rec=rec.ptr(), resid=resid.ptr(), b=b, t=t, c=c, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_ls_solve(a["x"], a["l"], a["s"], a["zf"], a["sens"], None, a["mask"], a["mask_w"], a["step"], a["thresh_l"],
                                         a["thresh_s"], a["iters"], a["rec"], a["resid"], a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"],
                                         a["nbytes"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_ls_solve t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_ls_solve t = 65")
    refused(call(h=401, nbytes=1 << 30), EUNSUPPORTED, k, "cine_ls_solve h = 401 (the operator's refusal)")
    for n in ("x", "zf", "sens", "mask", "step", "thresh_l", "thresh_s", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_ls_solve {n} = NULL")
    refused(call(rec=None), EINVAL, k, "cine_ls_solve resid without rec")
    refused(call(iters=0), EINVAL, k, "cine_ls_solve iters = 0")
    refused(call(c=0), EINVAL, k, "cine_ls_solve c = 0")
    refused(call(mask_w=2), EINVAL, k, "cine_ls_solve mask_w = 2")
    refused(call(x=base["zf"]), EINVAL, k, "cine_ls_solve x aliases zf")
    refused(call(l=base["x"]), EINVAL, k, "cine_ls_solve l aliases x")
    refused(call(s=base["l"]), EINVAL, k, "cine_ls_solve s aliases l")
    refused(call(rec=base["x"]), EINVAL, k, "cine_ls_solve rec aliases x")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_ls_solve a workspace one byte short")
    check(call()(), "cine_ls_solve")
    k.finish("cine_ls_solve")
    assert bool(torch.isfinite(x.t).all()) and bool(torch.isfinite(rec.t).all())
