"""cine_tv_solve (the whole spatio-temporal TV solve in one C call) against tests/tv_reference.py in float64, 30 iterations.

Shapes (b, t, c, h, w): (1, 5, 3, 24, 20) with a row mask and with a plane mask; (1, 7, 4, 21, 17), odd sizes that divide no tile, plane
mask; (2, 3, 9, 200, 12), the h == 200 operator and b > 1, row mask, with and without the tiled maps.  terms 3 everywhere, 1 and 2 on the
first shape, periodic off once.  The fixture is kt_reference.problem; tau = default_step, sigma = 1 / (2 tau B), lam_t = 0.02 max |D_t zf|,
lam_s = 0.01 max |(D_h, D_w) zf|, each rounded to float32 once.

Bars: x within kernel_sweep.BAR_CAP = 1e-4 of the float64 peak (the project's whole-model bar; the sibling FISTA measured 3.4e-6 for a
float32 restatement of its iterations, so expect that order), the record within REC_REL = 1e-4 relative, the final dual within BAR_CAP of
max(lam_t, lam_s), the radius of the larger ball.  Equal bits, record and dual included: the C driver against the binding's own loop of
ops.image_dc + ops.tv_pd_step, against ops.tv_solve, two calls of the driver, and a call with and without rec / p_out."""
import numpy as np
import pytest
import torch

import kt_reference as K
import tv_reference as R
from kernel_sweep import BAR_CAP, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
ITERS, LAM_T, LAM_S, REC_REL = 30, 0.02, 0.01, 1e-4
CASES = [((1, 5, 3, 24, 20), "row", False, 3, True), ((1, 5, 3, 24, 20), "plane", False, 3, True), ((1, 7, 4, 21, 17), "plane", False, 3, True),
         ((2, 3, 9, 200, 12), "row", False, 3, True), ((2, 3, 9, 200, 12), "row", True, 3, True),
         ((1, 5, 3, 24, 20), "row", False, 1, True), ((1, 5, 3, 24, 20), "row", False, 2, True), ((1, 5, 3, 24, 20), "plane", False, 3, False)]


def case_id(c):
    shape, layout, tiled, terms, periodic = c
    return "x".join(map(str, shape)) + f"-{layout}-tiled{int(tiled)}-terms{terms}-periodic{int(periodic)}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


_SETUP, _REF = {}, {}


def setup(shape, layout, terms=3, periodic=True):
    """The float32 operands of the solve (zf from the float64 adjoint, rounded once; the four scalars as float32 values), shared by the cases."""
    key = (shape, layout, terms, periodic)
    if key not in _SETUP:
        p = K.problem(shape, layout)
        zf = torch.from_numpy(K.to_pairs(p["zf"]).astype(np.float32))
        f32 = lambda v: float(np.float32(v))
        tau = f32(K.default_step(p["s"]))
        sigma = f32(R.default_sigma(tau, terms))
        peak_t, peak_s = R.peaks(p["zf"], periodic)
        _SETUP[key] = (p, zf, (tau, sigma, f32(LAM_T * peak_t), f32(LAM_S * peak_s)))
    return _SETUP[key]


def reference(shape, layout, terms, periodic, iters=ITERS):
    key = (shape, layout, terms, periodic, iters)
    if key not in _REF:
        p, zf, (tau, sigma, lam_t, lam_s) = setup(shape, layout, terms, periodic)
        _REF[key] = R.solve(K.to_complex(zf), p["s"], p["m"], tau, sigma, lam_t, lam_s, iters, periodic, terms)
    return _REF[key]


def solve_call(k, p, zf, scal, terms, periodic, shape, layout, tiled, iters=ITERS, record=True, dual=True):
    b, t, c, h, w = shape
    mask_w = 1 if layout == "row" else w
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    sc = [k.raw(torch.tensor([v], dtype=torch.float32)) for v in scal]
    x = k.out((b, t, h, w, 2))
    rec = k.out((iters, 4)) if record else None
    po = k.out((3, b, t, h, w, 2)) if dual else None
    nbytes = L().cine_tv_solve_ws_bytes(b, t, c, h, w, mask_w, iters)
    ws = k.ws(nbytes)
    check(L().cine_tv_solve(x.ptr(), ptr(zi), ptr(si), ptr(tiled), ptr(mi), mask_w, ptr(sc[0]), ptr(sc[1]), ptr(sc[2]), ptr(sc[3]), terms,
                            int(periodic), iters, rec.ptr() if record else None, po.ptr() if dual else None, b, t, c, h, w, ws.ptr(), nbytes,
                            stream()), "cine_tv_solve")
    return [x.t] + ([rec.t] if record else []) + ([po.t] if dual else [])


def rec_err(rec, want_rec, terms):
    """The worst relative error of the record; the column of a term that is off is 0 exactly on both sides."""
    cols = [0, 1] + ([2] if terms & 1 else []) + ([3] if terms & 2 else [])
    off = [q for q in (2, 3) if q not in cols]
    assert not rec[:, off].any() and not want_rec[:, off].any()
    return float((np.abs(rec[:, cols].double().numpy() - want_rec[:, cols]) / want_rec[:, cols]).max())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_solve_vs_float64_and_the_hand_rolled_loop(dev, case):
    from cine_hip import ops
    shape, layout, tiled, terms, periodic = case
    b, t, c, h, w = shape
    p, zf, scal = setup(shape, layout, terms, periodic)
    tau, sigma, lam_t, lam_s = scal
    want_x, want_p, want_rec = reference(shape, layout, terms, periodic)
    sens_d = p["sens_maps"].to(dev)
    tiled_d = ops.sens_tile_pack(sens_d) if tiled else None
    assert (tiled_d is not None) == tiled
    what = f"cine_tv_solve {case_id(case)}"
    x, rec, dual = twice(dev, 0, lambda k: solve_call(k, p, zf, scal, terms, periodic, shape, layout, tiled_d), what)     # two calls: equal bits
    ex = float(np.abs(K.to_complex(x) - want_x).max() / np.abs(want_x).max())
    er = rec_err(rec, want_rec, terms)
    radius = max(lam_t if terms & 1 else 0.0, lam_s if terms & 2 else 0.0)
    ep = float(np.abs(K.to_complex(dual) - want_p).max() / radius)
    print(f"{what}: x {ex:.3e} of the float64 peak (bar {BAR_CAP:.0e}), record {er:.3e} relative (bar {REC_REL:.0e}), dual {ep:.3e} of the "
          f"larger radius (bar {BAR_CAP:.0e})")
    assert ex <= BAR_CAP and er <= REC_REL and ep <= BAR_CAP
    if not terms & 1:
        assert not dual[0].any()                                                      # the planes of a term that is off: zeros
    if not terms & 2:
        assert not dual[1:].any()
    # the binding's own loop over the two entry points, and the binding of the driver
    zf_d, mask_d = zf.to(dev).unsqueeze(2), p["mask"].to(dev)
    sc = [torch.tensor([v], device=dev) for v in scal]
    xk, pk = zf_d, torch.zeros((3,) + tuple(zf_d.shape), device=dev)
    rows = []
    for k in range(ITERS):
        g = ops.image_dc(xk, sens_d, zf_d, mask_d, weights=(1.0, 0.0, -1.0), sens_tiled=tiled_d)
        xk, pk, r = ops.tv_pd_step(xk, g, pk, *sc, terms=terms, periodic=periodic, record=True)
        rows.append(r)
    assert same_bits(xk.squeeze(2).cpu(), x) and same_bits(torch.stack(rows).cpu(), rec) and same_bits(pk.squeeze(3).cpu(), dual), \
        what + ": the hand-rolled loop gives other bits"
    xb, pb, rb = ops.tv_solve(zf_d, sens_d, mask_d, *sc, ITERS, terms=terms, periodic=periodic, sens_tiled=tiled_d, record=True, dual=True)
    assert xb.shape == zf_d.shape and pb.shape == (3,) + tuple(zf_d.shape)
    assert same_bits(xb.squeeze(2).cpu(), x) and same_bits(rb.cpu(), rec) and same_bits(pb.squeeze(3).cpu(), dual)
    assert same_bits(ops.tv_solve(zf_d, sens_d, mask_d, *sc, ITERS, terms=terms, periodic=periodic, sens_tiled=tiled_d).squeeze(2).cpu(), x)
    for record, with_dual in ((False, False), (True, False), (False, True)):
        k = Call(dev, 0)
        outs = solve_call(k, p, zf, scal, terms, periodic, shape, layout, tiled_d, record=record, dual=with_dual)
        k.finish(what + f" record {int(record)} dual {int(with_dual)}")
        assert same_bits(outs[0].cpu(), x), what + ": other bits without rec / p_out"
        assert not record or same_bits(outs[1].cpu(), rec)
        assert not with_dual or same_bits(outs[-1].cpu(), dual)


def test_an_even_number_of_iterations_ends_in_x_too(dev):
    """The iterates alternate between x and the workspace: 1, 2 and 3 iterations against the yardstick and the hand-rolled loop's bits."""
    from cine_hip import ops
    shape, layout = (1, 5, 3, 24, 20), "row"
    p, zf, scal = setup(shape, layout)
    zf_d, mask_d, sens_d = zf.to(dev).unsqueeze(2), p["mask"].to(dev), p["sens_maps"].to(dev)
    sc = [torch.tensor([v], device=dev) for v in scal]
    xk, pk = zf_d, torch.zeros((3,) + tuple(zf_d.shape), device=dev)
    for iters in (1, 2, 3):
        x, dual = twice(dev, 0, lambda k: solve_call(k, p, zf, scal, 3, True, shape, layout, None, iters=iters, record=False), "cine_tv_solve")
        want_x, _, _ = reference(shape, layout, 3, True, iters)
        assert float(np.abs(K.to_complex(x) - want_x).max() / np.abs(want_x).max()) <= BAR_CAP
        xk, pk = ops.tv_pd_step(xk, ops.image_dc(xk, sens_d, zf_d, mask_d, weights=(1.0, 0.0, -1.0)), pk, *sc)
        assert same_bits(xk.squeeze(2).cpu(), x) and same_bits(pk.squeeze(3).cpu(), dual), iters


def test_one_iteration_is_one_gradient_step_and_one_projection(dev):
    shape, layout = (1, 5, 3, 24, 20), "row"
    p, zf, scal = setup(shape, layout)
    tau, sigma, lam_t, lam_s = scal
    x, rec, dual = twice(dev, 0, lambda k: solve_call(k, p, zf, scal, 3, True, shape, layout, None, iters=1), "cine_tv_solve")
    z64 = K.to_complex(zf)
    want_x = z64 - tau * K.gradient(z64, p["s"], p["m"], z64)
    want_p = R.project(sigma * R.D(2.0 * want_x - z64), lam_t, lam_s)
    assert float(np.abs(K.to_complex(x) - want_x).max() / np.abs(want_x).max()) <= BAR_CAP
    assert float(np.abs(K.to_complex(dual) - want_p).max() / max(lam_t, lam_s)) <= BAR_CAP
    want_rec = R.record(want_x, z64)
    assert rec.shape == (1, 4) and float((np.abs(rec[0].double().numpy() - want_rec) / want_rec).max()) <= REC_REL


def test_refusals_come_before_anything_is_written(dev):
    shape, layout = (1, 5, 3, 24, 20), "row"
    b, t, c, h, w = shape
    p, zf, scal = setup(shape, layout)
    k = Call(dev, 0)
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    sc = [k.raw(torch.tensor([v], dtype=torch.float32)) for v in scal]
    x, rec, po = k.out((b, t, h, w, 2)), k.out((3, 4)), k.out((3, b, t, h, w, 2))
    need = L().cine_tv_solve_ws_bytes(b, t, c, h, w, 1, 3)
    assert need > L().cine_tv_solve_ws_bytes(b, t, c, h, w, 1, 2) > 8 * zf.numel() * 4 and L().cine_tv_solve_ws_bytes(b, t, c, h, w, 1, 0) == 0
    ws = k.ws(need)
    base = dict(x=x.ptr(), zf=ptr(zi), sens=ptr(si), mask=ptr(mi), mask_w=1, tau=ptr(sc[0]), sigma=ptr(sc[1]), lam_t=ptr(sc[2]), lam_s=ptr(sc[3]),
                terms=3, iters=3, rec=rec.ptr(), p_out=po.ptr(), b=b, t=t, c=c, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_tv_solve(a["x"], a["zf"], a["sens"], None, a["mask"], a["mask_w"], a["tau"], a["sigma"], a["lam_t"], a["lam_s"],
                                         a["terms"], 1, a["iters"], a["rec"], a["p_out"], a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"],
                                         a["nbytes"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_tv_solve t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_tv_solve t = 65")
    refused(call(h=401, nbytes=1 << 30), EUNSUPPORTED, k, "cine_tv_solve h = 401 (the operator's refusal)")
    for n in ("x", "zf", "sens", "mask", "tau", "sigma", "lam_t", "lam_s", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_tv_solve {n} = NULL")
    refused(call(iters=0), EINVAL, k, "cine_tv_solve iters = 0")
    refused(call(c=0), EINVAL, k, "cine_tv_solve c = 0")
    refused(call(mask_w=2), EINVAL, k, "cine_tv_solve mask_w = 2")
    refused(call(terms=0), EINVAL, k, "cine_tv_solve terms = 0")
    refused(call(terms=4), EINVAL, k, "cine_tv_solve terms = 4")
    refused(call(x=base["zf"]), EINVAL, k, "cine_tv_solve x aliases zf")
    refused(call(rec=base["x"]), EINVAL, k, "cine_tv_solve rec aliases x")
    refused(call(p_out=base["x"]), EINVAL, k, "cine_tv_solve p_out aliases x")
    refused(call(p_out=base["zf"]), EINVAL, k, "cine_tv_solve p_out aliases zf")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_tv_solve a workspace one byte short")
    check(call()(), "cine_tv_solve")
    k.finish("cine_tv_solve")
    assert bool(torch.isfinite(x.t).all()) and bool(torch.isfinite(rec.t).all()) and bool(torch.isfinite(po.t).all())
