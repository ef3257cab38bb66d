"""cine_kt_fista (the whole k-t SPARSE-SENSE solve in one C call) against tests/kt_reference.py in float64, 30 iterations.

Shapes (b, t, c, h, w): (1, 5, 3, 24, 20) with a row mask and with a plane mask; (1, 7, 4, 21, 17), direct-DFT odd lengths, plane mask;
(2, 3, 9, 200, 12), the h == 200 operator, row mask, with and without the tiled maps.  penalise_dc on and off.  The fixture is
kt_reference.problem: RSS-normalised smooth maps, the moving-disc phantom, 1 % noise, about one row in three plus a centre block.

Bars: x within kernel_sweep.BAR_CAP = 1e-4 of the float64 peak (the project's whole-model bar; a float32 numpy restatement of the same
iterations stays within 3.4e-6 of float64 on such shapes, so the bar leaves a factor of 30), the record within REC_REL = 1e-4 relative.
Equal bits, record included: the C driver against the binding's own loop of ops.image_dc + ops.kt_prox, against ops.kt_fista, and two calls
of the driver."""
import numpy as np
import pytest
import torch

import kt_reference as R
from kernel_sweep import BAR_CAP, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
ITERS, LAM, REC_REL = 30, 0.02, 1e-4
CASES = [((1, 5, 3, 24, 20), "row", False), ((1, 5, 3, 24, 20), "plane", False), ((1, 7, 4, 21, 17), "plane", False),
         ((2, 3, 9, 200, 12), "row", False), ((2, 3, 9, 200, 12), "row", True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


_SETUP, _REF = {}, {}


def setup(shape, layout):
    """The float32 operands of the solve (zf from the float64 adjoint, rounded once; step and threshold as float32 values), per shape and
    layout, shared by the cases."""
    key = (shape, layout)
    if key not in _SETUP:
        p = R.problem(shape, layout)
        zf = torch.from_numpy(R.to_pairs(p["zf"]).astype(np.float32))
        step = float(np.float32(R.default_step(p["s"])))
        thresh = float(np.float32(LAM * np.abs(R.fft1c(p["zf"], 1)).max()))
        _SETUP[key] = (p, zf, step, thresh)
    return _SETUP[key]


def reference(shape, layout, pdc):
    key = (shape, layout, pdc)
    if key not in _REF:
        p, zf, step, thresh = setup(shape, layout)
        _REF[key] = R.fista(R.to_complex(zf), p["s"], p["m"], step, thresh, ITERS, pdc)
    return _REF[key]


def fista_call(k, p, zf, step, thresh, pdc, shape, layout, tiled, iters=ITERS, record=True):
    b, t, c, h, w = shape
    mask_w = 1 if layout == "row" else w
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    st, th = k.raw(torch.tensor([step])), k.raw(torch.tensor([thresh]))
    x = k.out((b, t, h, w, 2))
    rec = k.out((iters, 4)) if record else None
    nbytes = L().cine_kt_fista_ws_bytes(b, t, c, h, w, mask_w, iters)
    ws = k.ws(nbytes)
    check(L().cine_kt_fista(x.ptr(), ptr(zi), ptr(si), ptr(tiled), ptr(mi), mask_w, ptr(st), ptr(th), iters, int(pdc), rec.ptr() if record else None,
                            b, t, c, h, w, ws.ptr(), nbytes, stream()), "cine_kt_fista")
    return [x.t] + ([rec.t] if record else [])


@pytest.mark.parametrize("pdc", [True, False], ids=["dc", "nodc"])
@pytest.mark.parametrize("shape,layout,tiled", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_fista_vs_float64_and_the_hand_rolled_loop(dev, shape, layout, tiled, pdc):
    from cine_hip import classical, ops
    b, t, c, h, w = shape
    p, zf, step, thresh = setup(shape, layout)
    want_x, want_rec = reference(shape, layout, pdc)
    sens_d = p["sens_maps"].to(dev)
    tiled_d = ops.sens_tile_pack(sens_d) if tiled else None
    assert (tiled_d is not None) == tiled
    what = f"cine_kt_fista {shape} {layout} tiled {int(tiled)} penalise_dc {int(pdc)}"
    x, rec = twice(dev, 0, lambda k: fista_call(k, p, zf, step, thresh, pdc, shape, layout, tiled_d), what)        # two calls: equal bits
    ex = float(np.abs(R.to_complex(x) - want_x).max() / np.abs(want_x).max())
    er = float((np.abs(rec[:, :3].double().numpy() - want_rec) / want_rec).max())
    print(f"{what}: x {ex:.3e} of the float64 peak (bar {BAR_CAP:.0e}), record {er:.3e} relative (bar {REC_REL:.0e})")
    assert ex <= BAR_CAP and er <= REC_REL and not rec[:, 3].any()
    # the binding's own loop over the two entry points, and the binding of the driver
    zf_d, mask_d = zf.to(dev).unsqueeze(2), p["mask"].to(dev)
    st, th = torch.tensor([step], device=dev), torch.tensor([thresh], device=dev)
    betas = classical.fista_momentum(ITERS)
    xk = zk = zf_d
    rows = []
    for k in range(ITERS):
        g = ops.image_dc(zk, sens_d, zf_d, mask_d, weights=(1.0, 0.0, -1.0), sens_tiled=tiled_d)
        xk, zk, r = ops.kt_prox(zk, g, xk, st, th, float(betas[k]), penalise_dc=pdc, record=True)
        rows.append(r)
    assert same_bits(xk.squeeze(2).cpu(), x) and same_bits(torch.stack(rows).cpu(), rec), what + ": the hand-rolled loop gives other bits"
    xb, rb = ops.kt_fista(zf_d, sens_d, mask_d, st, th, ITERS, penalise_dc=pdc, sens_tiled=tiled_d, record=True)
    assert xb.shape == zf_d.shape and same_bits(xb.squeeze(2).cpu(), x) and same_bits(rb.cpu(), rec)
    k = Call(dev, 0)
    (x_only,) = fista_call(k, p, zf, step, thresh, pdc, shape, layout, tiled_d, record=False)
    k.finish(what + " without a record")
    assert same_bits(x_only.cpu(), x)


def test_one_iteration_is_one_gradient_step_and_one_prox(dev):
    shape, layout = (1, 5, 3, 24, 20), "row"
    p, zf, step, thresh = setup(shape, layout)
    x, rec = twice(dev, 0, lambda k: fista_call(k, p, zf, step, thresh, True, shape, layout, None, iters=1), "cine_kt_fista")
    z64 = R.to_complex(zf)
    want, _, want_rec = R.prox(z64, R.gradient(z64, p["s"], p["m"], z64), z64, step, thresh, 0.0, True)
    assert float(np.abs(R.to_complex(x) - want).max() / np.abs(want).max()) <= BAR_CAP
    assert rec.shape == (1, 4) and float((np.abs(rec[0, :3].double().numpy() - want_rec) / want_rec).max()) <= REC_REL


def test_refusals_come_before_anything_is_written(dev):
    shape, layout = (1, 5, 3, 24, 20), "row"
    b, t, c, h, w = shape
    p, zf, step, thresh = setup(shape, layout)
    k = Call(dev, 0)
    zi, si, mi = k.inp(zf), k.inp(p["sens_maps"]), k.raw(p["mask"])
    st, th = k.raw(torch.tensor([step])), k.raw(torch.tensor([thresh]))
    x, rec = k.out((b, t, h, w, 2)), k.out((3, 4))
    need = L().cine_kt_fista_ws_bytes(b, t, c, h, w, 1, 3)
    assert need > L().cine_kt_fista_ws_bytes(b, t, c, h, w, 1, 2) > 2 * zf.numel() * 4 and L().cine_kt_fista_ws_bytes(b, t, c, h, w, 1, 0) == 0
    ws = k.ws(need)
    base = dict(x=x.ptr(), zf=ptr(zi), sens=ptr(si), mask=ptr(mi), mask_w=1, step=ptr(st), thresh=ptr(th), iters=3, rec=rec.ptr(),
                b=b, t=t, c=c, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_kt_fista(a["x"], a["zf"], a["sens"], None, a["mask"], a["mask_w"], a["step"], a["thresh"], a["iters"], 1, a["rec"],
                                         a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"], a["nbytes"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_kt_fista t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_kt_fista t = 65")
    refused(call(h=401, nbytes=1 << 30), EUNSUPPORTED, k, "cine_kt_fista h = 401 (the operator's refusal)")
    for n in ("x", "zf", "sens", "mask", "step", "thresh", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_kt_fista {n} = NULL")
    refused(call(iters=0), EINVAL, k, "cine_kt_fista iters = 0")
    refused(call(c=0), EINVAL, k, "cine_kt_fista c = 0")
    refused(call(mask_w=2), EINVAL, k, "cine_kt_fista mask_w = 2")
    refused(call(x=base["zf"]), EINVAL, k, "cine_kt_fista x aliases zf")
    refused(call(rec=base["x"]), EINVAL, k, "cine_kt_fista rec aliases x")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_kt_fista a workspace one byte short")
    check(call()(), "cine_kt_fista")
    k.finish("cine_kt_fista")
    assert bool(torch.isfinite(x.t).all()) and bool(torch.isfinite(rec.t).all())
