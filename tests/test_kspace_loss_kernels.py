"""cine_kspace_loss / cine_kspace_loss_grad (the self-supervised k-space loss on held-out samples) through the C ABI, shape by shape against
float64 autograd of the loss formula on the oracle's sens_expand.

Shapes (b, t, c, h, w): a 2 x 3 image, the direct DFT at odd lengths, mixed radix, the h == 200 one-kernel column pass with 9 coils, the
w == 200 row kernels.  Each with a row mask and a plane mask: all ones, about 40 %, a single point (for a row mask a single row).

The fixture has no kink: y = u + d with u the float64 prediction and every real component of d of magnitude in [0.51, 1.5] with a random sign,
rounded to float32, so no component of the residual is within 0.5 of zero (asserted on the float64 residual) and float32 rounding cannot flip
a sign.

Bars (tests/test_general_mask_training.py holds the residual operator these kernels extend to the same ones): the loss and the four sums within
LAM_REL = 1e-4 relative of float64; the image gradient and the maps' gradient within RESID = 5e-5 of the float64 peak."""
import pytest
import torch

from conftest import rel_err, rnd
from kernel_sweep import EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
D_KSPACE_LOSS = 32
LAM_REL, RESID = 1e-4, 5e-5
GLOSS = 0.7                                      # the incoming scalar gradient
SHAPES = [(1, 1, 1, 2, 3), (1, 2, 2, 21, 17), (1, 3, 3, 24, 20), (2, 2, 9, 200, 12), (1, 1, 2, 12, 200)]
LAYOUTS = ["row", "plane"]
KINDS = ["ones", "frac", "single"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def chunks(b, t, c):
    """Column-pass launches per call: the image batch is cut at the grid limit in multiples of c."""
    return -(-(b * t * c) // (32768 // c * c))


def make_lam(kind, layout, b, t, h, w, seed):
    ww = 1 if layout == "row" else w
    if kind == "ones":
        return torch.ones(b, t, 1, h, ww, 1, dtype=torch.uint8)
    if kind == "frac":
        g = torch.Generator().manual_seed(seed)
        m = (torch.rand(b, t, 1, h, ww, 1, generator=g) < 0.4).to(torch.uint8)
        m[0, 0, 0, 0, 0, 0] = 1
        return m
    m = torch.zeros(b, t, 1, h, ww, 1, dtype=torch.uint8)
    m[b - 1, t - 1, 0, h // 2, ww // 2, 0] = 1
    return m


_FIX, _REF = {}, {}


def fixture(shape):
    """Image, maps (float32), the float64 prediction u and the kink-free measurement y (float32), once per shape."""
    if shape not in _FIX:
        from oracle import varnet_ref as V
        b, t, c, h, w = shape
        x, s = rnd(1, b, t, 1, h, w, 2), rnd(2, b, 1, c, h, w, 2)
        u = V.VarNetBlock.sens_expand(x.double(), s.double())
        g = torch.Generator().manual_seed(3)
        mag = 0.51 + 0.99 * torch.rand(u.shape, generator=g, dtype=torch.float64)
        sign = torch.where(torch.rand(u.shape, generator=g) < 0.5, -1.0, 1.0).double()
        y = (u + sign * mag).float()
        r = u - y.double()
        assert float(r.abs().min()) >= 0.5, "the fixture has a residual component within 0.5 of zero"
        _FIX[shape] = (x, s, y)
    return _FIX[shape]


def loss_formula(u, y, lam):
    """The loss and its four sums in the tensors' own precision; lam broadcasts."""
    r, v = lam * (u - y), lam * y
    r2, r1, y2, y1 = (r * r).sum(), r.abs().sum(), (v * v).sum(), v.abs().sum()
    return 0.5 * r2.sqrt() / y2.sqrt() + 0.5 * r1 / y1, (r2, r1, y2, y1)


def reference(shape, layout, kind):
    key = (shape, layout, kind)
    if key not in _REF:
        from oracle import varnet_ref as V
        x, s, y = fixture(shape)
        b, t, c, h, w = shape
        lam = make_lam(kind, layout, b, t, h, w, 7)
        with torch.enable_grad():
            x64, s64 = x.double().requires_grad_(True), s.double().requires_grad_(True)
            loss, sums = loss_formula(V.VarNetBlock.sens_expand(x64, s64), y.double(), lam.double())
            gx, gs = torch.autograd.grad(GLOSS * loss, (x64, s64))
        _REF[key] = (lam, float(loss), [float(v) for v in sums], gx, gs)
    return _REF[key]


def forward_call(k, x, s, y, plane, shape):
    b, t, c, h, w = shape
    xi, si, yi, mi = k.inp(x), k.inp(s), k.inp(y), k.raw(plane)
    rec = k.out((8,))
    nbytes = L().cine_kspace_loss_ws_bytes(b, t, c, h, w)
    assert nbytes == L().cine_image_dc_general_ws_bytes(b, t, c, h, w) > 0
    ws = k.ws(nbytes)
    check(L().cine_kspace_loss(ptr(xi), ptr(si), ptr(yi), ptr(mi), rec.ptr(), b, t, c, h, w, ws.ptr(), nbytes, stream()), "cine_kspace_loss")
    return (xi, si, yi, mi), rec, nbytes


def both_passes(k, x, s, y, plane, shape):
    """Forward, then backward with both outputs, on fresh operands of Call k -> [rec, gimg, part]."""
    b, t, c, h, w = shape
    (xi, si, yi, mi), rec, nbytes = forward_call(k, x, s, y, plane, shape)
    gl = k.raw(torch.tensor([GLOSS]))
    gimg, part = k.out((b, t, 1, h, w, 2)), k.out((b, t, c, h, w, 2))
    ws = k.ws(nbytes)
    check(L().cine_kspace_loss_grad(ptr(xi), ptr(si), ptr(yi), ptr(mi), rec.ptr(), ptr(gl), gimg.ptr(), part.ptr(), b, t, c, h, w,
                                    ws.ptr(), nbytes, stream()), "cine_kspace_loss_grad")
    return [rec.t, gimg.t, part.t]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradients_vs_float64(dev, shape, layout, kind):
    from cine_hip import ops
    b, t, c, h, w = shape
    x, s, y = fixture(shape)
    lam, want_loss, want_sums, want_gx, want_gs = reference(shape, layout, kind)
    plane = lam.expand(b, t, 1, h, w, 1).contiguous()
    L().cine_diag_counter(D_KSPACE_LOSS, 1)
    rec, gimg, part = twice(dev, 2, lambda k: both_passes(k, x, s, y, plane, shape), "cine_kspace_loss")        # two calls: identical bits
    assert L().cine_diag_counter(D_KSPACE_LOSS, 1) == 2 * 2 * chunks(b, t, c)              # forward and backward, each call twice
    errs = {n: abs(float(rec[i]) - v) / abs(v) for i, (n, v) in enumerate(zip(("sum r^2", "sum |r|", "sum y^2", "sum |y|"), want_sums))}
    errs["loss"] = abs(float(rec[4]) - want_loss) / abs(want_loss)
    gs = part.double().sum(dim=1, keepdim=True)                                              # the frames added (cine_coil_accum's job)
    gerrs = {"image gradient": rel_err(gimg, want_gx), "maps' gradient": rel_err(gs, want_gs)}
    print(f"{shape} {layout} {kind}: " + ", ".join(f"{n} {e:.3e}" for n, e in errs.items()) + f" relative (bar {LAM_REL:.0e}); " +
          ", ".join(f"{n} {e:.3e}" for n, e in gerrs.items()) + f" of the float64 peak (bar {RESID:.0e})")
    assert all(e < LAM_REL for e in errs.values()), errs
    assert all(e < RESID for e in gerrs.values()), gerrs
    # the binding with the mask in its own layout (a row mask is expanded to planes there): the same bits, and cine_coil_accum's sum
    d = [v.to(dev) for v in (x, s, y, lam)]
    rec_b = ops.kspace_loss_forward(*d)
    gimg_b, part_b = ops.kspace_loss_backward(*d, rec_b, torch.tensor([GLOSS], device=dev), want_image=True, want_sens=True)
    assert same_bits(rec_b.cpu(), rec) and same_bits(gimg_b.cpu(), gimg) and same_bits(part_b.cpu(), part)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_counter_advances_in_forward_and_in_backward(dev, shape):
    b, t, c, h, w = shape
    x, s, y = fixture(shape)
    plane = make_lam("frac", "plane", b, t, h, w, 7)
    L().cine_diag_counter(D_KSPACE_LOSS, 1)
    k = Call(dev, 0)
    (xi, si, yi, mi), rec, nbytes = forward_call(k, x, s, y, plane, shape)
    assert L().cine_diag_counter(D_KSPACE_LOSS, 1) == chunks(b, t, c)
    gl, gimg, ws = k.raw(torch.tensor([GLOSS])), k.out((b, t, 1, h, w, 2)), k.ws(nbytes)
    check(L().cine_kspace_loss_grad(ptr(xi), ptr(si), ptr(yi), ptr(mi), rec.ptr(), ptr(gl), gimg.ptr(), None, b, t, c, h, w,
                                    ws.ptr(), nbytes, stream()), "cine_kspace_loss_grad")
    assert L().cine_diag_counter(D_KSPACE_LOSS, 1) == chunks(b, t, c)
    k.finish("cine_kspace_loss_grad")
    assert L().cine_diag_counter(16, 0) == -1 and L().cine_diag_counter(31, 0) == -1 and L().cine_diag_counter(33, 0) == -1


@pytest.mark.parametrize("kind", ["frac", "single"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_measurement_is_read_on_the_loss_mask_only(dev, shape, kind):
    """NaN in y outside the mask changes no bit of any output."""
    b, t, c, h, w = shape
    x, s, y = fixture(shape)
    plane = make_lam(kind, "plane", b, t, h, w, 7)
    poisoned = torch.where(plane.bool().expand(b, t, c, h, w, 2), y, torch.full_like(y, float("nan")))
    assert bool(torch.isnan(poisoned).any())
    clean = twice(dev, 0, lambda k: both_passes(k, x, s, y, plane, shape), "cine_kspace_loss")
    dirty = twice(dev, 0, lambda k: both_passes(k, x, s, poisoned, plane, shape), "cine_kspace_loss")
    for a, bb in zip(clean, dirty):
        assert not bool(torch.isnan(bb).any()) and same_bits(a, bb)


def test_an_empty_mask_gives_what_the_expression_gives(dev):
    shape = (1, 3, 3, 24, 20)
    b, t, c, h, w = shape
    x, s, y = fixture(shape)
    plane = torch.zeros(b, t, 1, h, w, 1, dtype=torch.uint8)
    k = Call(dev, 0)
    _, rec, _ = forward_call(k, x, s, y, plane, shape)
    k.finish("cine_kspace_loss")
    want, _ = loss_formula(torch.zeros(4), torch.ones(4), torch.zeros(4))
    assert bool(torch.isnan(want)) and bool(torch.isnan(rec.t[4])) and float(rec.t[:4].abs().max()) == 0.0


def test_refusals_come_before_anything_is_written(dev):
    shape = (1, 3, 3, 24, 20)
    b, t, c, h, w = shape
    x, s, y = fixture(shape)
    plane = make_lam("frac", "plane", b, t, h, w, 7)
    k = Call(dev, 0)
    xi, si, yi, mi, gl = k.inp(x), k.inp(s), k.inp(y), k.raw(plane), k.raw(torch.tensor([GLOSS]))
    rec, gimg, part = k.out((8,)), k.out((b, t, 1, h, w, 2)), k.out((b, t, c, h, w, 2))
    recin = k.inp(torch.ones(8))
    need = L().cine_kspace_loss_ws_bytes(b, t, c, h, w)
    ws = k.ws(need)
    base = dict(img=ptr(xi), sens=ptr(si), kspace=ptr(yi), mask=ptr(mi), rec=rec.ptr(), b=b, t=t, c=c, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def fwd(**kw):
        a = {**base, **kw}
        return lambda: L().cine_kspace_loss(a["img"], a["sens"], a["kspace"], a["mask"], a["rec"], a["b"], a["t"], a["c"], a["h"], a["w"],
                                            a["ws"], a["nbytes"], stream())
    gbase = {**base, "rec": ptr(recin), "gloss": ptr(gl), "gimg": gimg.ptr(), "part": part.ptr()}

    def bwd(**kw):
        a = {**gbase, **kw}
        return lambda: L().cine_kspace_loss_grad(a["img"], a["sens"], a["kspace"], a["mask"], a["rec"], a["gloss"], a["gimg"], a["part"],
                                                 a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"], a["nbytes"], stream())
    for name, call, nulls in (("cine_kspace_loss", fwd, ("img", "sens", "kspace", "mask", "rec", "ws")),
                              ("cine_kspace_loss_grad", bwd, ("img", "sens", "kspace", "mask", "rec", "gloss", "ws"))):
        refused(call(h=401), EUNSUPPORTED, k, f"{name} h = 401")
        refused(call(w=401), EUNSUPPORTED, k, f"{name} w = 401")
        for n in nulls:
            refused(call(**{n: None}), EINVAL, k, f"{name} {n} = NULL")
        refused(call(nbytes=need - 1), EWORKSPACE, k, f"{name} a workspace one byte short")
        refused(call(c=32769), EINVAL, k, f"{name} c = 32769")
        refused(call(b=65536, t=1), EUNSUPPORTED, k, f"{name} b*t > 65535")
        refused(call(h=1, w=9), EUNSUPPORTED, k, f"{name} h = 1 with a one-point tile")
    refused(bwd(gimg=None, part=None), EINVAL, k, "cine_kspace_loss_grad both outputs NULL")
    for n in ("img", "sens", "kspace"):
        refused(fwd(rec=base[n]), EINVAL, k, f"cine_kspace_loss rec aliases {n}")
        refused(bwd(gimg=base[n]), EINVAL, k, f"cine_kspace_loss_grad gimg aliases {n}")
        refused(bwd(part=base[n]), EINVAL, k, f"cine_kspace_loss_grad part aliases {n}")
    refused(fwd(rec=base["ws"]), EINVAL, k, "cine_kspace_loss rec aliases ws")
    refused(bwd(gimg=base["ws"]), EINVAL, k, "cine_kspace_loss_grad gimg aliases ws")
    refused(bwd(part=gimg.ptr()), EINVAL, k, "cine_kspace_loss_grad part aliases gimg")
    assert L().cine_kspace_loss_ws_bytes(1, 1, 1, 1, 9) == 0 and L().cine_kspace_loss_ws_bytes(1, 1, 1, 1, 8) == 64
