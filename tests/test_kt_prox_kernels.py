"""cine_kt_prox (the second half of one k-t FISTA iteration, one launch) through the C ABI, shape by shape against tests/kt_reference.py in
float64, with the kernel_sweep harness: guarded outputs, an exact-size workspace with a sentinel tail, two calls with equal bits, refusals
that write nothing.

Frames t: 2 (smallest), 5 and 15 (odd: the DC bin t // 2 and (t + 1) // 2 differ), 16 (even), 64 (the limit; the whole LDS tile).  Pixels
h * w: 1, and P - 1, P, P + 1, 2 P + 3 around the kernel's pixel tile P = ops.kt_prox_pixels().  Batch 2 once.  Per shape every combination of
threshold (0: the result is v = z - step g itself; above every |F_t v|: zero, or the temporal mean with penalise_dc off; the median of
|F_t v|), momentum (0, 0.7) and penalise_dc.  In place (znew == z, xnew == xprev) gives the bits of out of place.

Bars: xnew and znew within kernel_sweep.BAR = 1e-5 of the float64 peak (the map is 1-Lipschitz and continuous at the kink, so the fixture
needs no margin around it); a result that is zero in float64 is zero exactly.  The three sums within SUM_REL = 1e-4 relative, the bar
test_kspace_loss_kernels.py holds for its sums."""
import numpy as np
import pytest
import torch

import kt_reference as R
from conftest import rnd
from kernel_sweep import BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
SUM_REL = 1e-4
STEP = 0.9
FRAMES = [2, 5, 15, 16, 64]
TILE = 64                                        # asserted against the binding's constant below; only the ids are made from it
PIXELS = {"1": (1, 1), "P-1": (7, 9), "P": (8, 8), "P+1": (5, 13), "2P+3": (131, 1)}
THRESHOLDS = ["zero", "above", "median"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def test_the_pixel_sizes_sit_around_the_kernels_tile(dev):
    from cine_hip import ops
    P = ops.kt_prox_pixels()
    assert P == TILE == L().cine_kt_prox_pixels()
    assert [h * w for h, w in PIXELS.values()] == [1, P - 1, P, P + 1, 2 * P + 3]
    assert L().cine_kt_prox_ws_bytes(2, 5, 5, 13) == 2 * 2 * 16 and L().cine_kt_prox_ws_bytes(1, 64, 8, 8) == 16
    assert L().cine_kt_prox_ws_bytes(0, 5, 5, 13) == 0


def operands(shape, seed):
    b, t, h, w = shape
    return rnd(seed, b, t, h, w, 2), rnd(seed + 1, b, t, h, w, 2), rnd(seed + 2, b, t, h, w, 2)


def threshold_for(kind, z, g, penalise_dc):
    """thresh (a float32 value) with step * thresh at the wanted place among |F_t v|."""
    step = float(np.float32(STEP))
    c = np.abs(R.fft1c(R.to_complex(z) - step * R.to_complex(g), 1))
    th = {"zero": 0.0, "above": 1.5 * c.max(), "median": float(np.median(c))}[kind]
    return float(np.float32(th / step))


def prox_call(k, z, g, xp, thresh, beta, pdc, shape, inplace=False, record=True):
    b, t, h, w = shape
    si, ti, gi = k.raw(torch.tensor([STEP])), k.raw(torch.tensor([thresh])), k.inp(g)
    if inplace:
        zo, xo = k.out((b, t, h, w, 2), fill=z), k.out((b, t, h, w, 2), fill=xp)
        zi, xi = zo.t, xo.t
    else:
        zi, xi = k.inp(z), k.inp(xp)
        xo, zo = k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2))
    rec = k.out((4,)) if record else None
    nbytes = L().cine_kt_prox_ws_bytes(b, t, h, w) if record else 0
    assert not record or nbytes == -(-h * w // TILE) * b * 16
    ws = k.ws(nbytes)
    check(L().cine_kt_prox(ptr(zi), ptr(gi), ptr(xi), ptr(si), ptr(ti), beta, int(pdc), xo.ptr(), zo.ptr(), rec.ptr() if record else None,
                           b, t, h, w, ws.ptr() if ws else None, nbytes, stream()), "cine_kt_prox")
    return [xo.t, zo.t] + ([rec.t] if record else [])


def peak_err(got, want):
    """max |got - want| over the float64 peak of want; a float64 zero must be met exactly."""
    got = R.to_complex(got)
    peak = np.abs(want).max()
    if peak == 0.0:
        assert not got.any(), "a result that is zero in float64 is not zero"
        return 0.0
    return float(np.abs(got - want).max() / peak)


def check_case(dev, shape, seed):
    z, g, xp = operands(shape, seed)
    t = shape[1]
    z64, g64, xp64 = R.to_complex(z), R.to_complex(g), R.to_complex(xp)
    step = float(np.float32(STEP))
    worst = {}
    for kind in THRESHOLDS:
        for pdc in (True, False):
            thresh = threshold_for(kind, z, g, pdc)
            for beta in (0.0, 0.7):
                what = f"cine_kt_prox {shape} {kind} beta {beta} penalise_dc {int(pdc)}"
                xnew, znew, rec = twice(dev, 2, lambda k: prox_call(k, z, g, xp, thresh, beta, pdc, shape), what)
                want_x, want_z, want_rec = R.prox(z64, g64, xp64, step, thresh, float(np.float32(beta)), pdc)
                v = z64 - step * g64
                if kind == "zero":
                    assert np.allclose(want_x, v, rtol=0, atol=1e-12)                         # the yardstick: no threshold, the result is v
                elif kind == "above":
                    mean = v.mean(axis=1, keepdims=True) * np.ones((1, t, 1, 1))
                    assert np.allclose(want_x, 0 if pdc else mean, rtol=0, atol=1e-12)        # zero, or the temporal mean
                ex, ez = peak_err(xnew, want_x), peak_err(znew, want_z)
                es = []
                floor = 1e-12 * np.array([(np.abs(v) ** 2).sum(), (np.abs(v) ** 2).sum(), np.abs(R.fft1c(v, 1)).sum()])
                for q in range(3):
                    if want_rec[q] < floor[q]:                  # zero but for float64 rounding (the inverse and forward transform of one bin)
                        assert float(rec[q]) == 0.0, (what, q, float(rec[q]))
                        es.append(0.0)
                    else:
                        es.append(abs(float(rec[q]) - want_rec[q]) / want_rec[q])
                assert float(rec[3]) == 0.0
                print(f"{what}: xnew {ex:.2e}, znew {ez:.2e} of the float64 peak (bar {BAR:.0e}); sums {es[0]:.2e} {es[1]:.2e} {es[2]:.2e} relative "
                      f"(bar {SUM_REL:.0e})")
                assert ex <= BAR and ez <= BAR, (what, ex, ez)
                assert max(es) <= SUM_REL, (what, es)
                # in place, and without the record: the same bits
                k = Call(dev, 2)
                xi, zi, ri = prox_call(k, z, g, xp, thresh, beta, pdc, shape, inplace=True)
                k.finish(what + " in place")
                assert same_bits(xi.cpu(), xnew) and same_bits(zi.cpu(), znew) and same_bits(ri.cpu(), rec), what + ": in place gives other bits"
                k = Call(dev, 0)
                xn, zn = prox_call(k, z, g, xp, thresh, beta, pdc, shape, record=False)
                k.finish(what + " without a record")
                assert same_bits(xn.cpu(), xnew) and same_bits(zn.cpu(), znew), what + ": other bits without the record"
                worst[what] = max(ex, ez)
    return worst


@pytest.mark.parametrize("pix", list(PIXELS), ids=lambda p: f"pix{p}")
@pytest.mark.parametrize("t", FRAMES, ids=lambda t: f"t{t}")
def test_prox_vs_float64(dev, t, pix):
    h, w = PIXELS[pix]
    check_case(dev, (1, t, h, w), seed=1000 * t + h * w)


def test_prox_vs_float64_batch_two(dev):
    check_case(dev, (2, 5, 5, 13), seed=77)


def test_z_and_xprev_may_be_one_tensor(dev):
    """The first iteration of the solve: z == xprev == zf, read only; and with znew on top of it."""
    shape = (1, 5, 5, 13)
    z, g, _ = operands(shape, 5)
    thresh = threshold_for("median", z, g, True)
    want = twice(dev, 0, lambda k: prox_call(k, z, g, z, thresh, 0.7, True, shape), "cine_kt_prox")
    for inplace in (False, True):
        k = Call(dev, 0)
        b, t, h, w = shape
        si, ti, gi = k.raw(torch.tensor([STEP])), k.raw(torch.tensor([thresh])), k.inp(g)
        if inplace:
            zo, xo = k.out((b, t, h, w, 2), fill=z), k.out((b, t, h, w, 2))
            zi = zo.t
        else:
            zi, xo, zo = k.inp(z), k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2))
        check(L().cine_kt_prox(ptr(zi), ptr(gi), ptr(zi), ptr(si), ptr(ti), 0.7, 1, xo.ptr(), zo.ptr(), None, b, t, h, w, None, 0, stream()),
              "cine_kt_prox")
        k.finish("cine_kt_prox z == xprev")
        assert same_bits(xo.t.cpu(), want[0]) and same_bits(zo.t.cpu(), want[1]), inplace


def test_the_binding_gives_the_bits_of_the_c_call(dev):
    from cine_hip import ops
    shape = (2, 5, 5, 13)
    z, g, xp = operands(shape, 9)
    thresh = threshold_for("median", z, g, False)
    want = twice(dev, 0, lambda k: prox_call(k, z, g, xp, thresh, 0.7, False, shape), "cine_kt_prox")
    zd, gd, xd = z.to(dev), g.to(dev), xp.to(dev)
    st, th = torch.tensor([STEP], device=dev), torch.tensor([thresh], device=dev)
    xnew, znew, rec = ops.kt_prox(zd, gd, xd, st, th, 0.7, penalise_dc=False, record=True)
    assert same_bits(xnew.cpu(), want[0]) and same_bits(znew.cpu(), want[1]) and same_bits(rec.cpu(), want[2])
    z2, x2 = zd.clone(), xd.clone()
    a, bb = ops.kt_prox(z2, gd, x2, st, th, 0.7, penalise_dc=False, xnew=x2, znew=z2)               # in place through the binding
    assert a.data_ptr() == x2.data_ptr() and bb.data_ptr() == z2.data_ptr()
    assert same_bits(x2.cpu(), want[0]) and same_bits(z2.cpu(), want[1])
    xnew6, _ = ops.kt_prox(zd.unsqueeze(2), gd.unsqueeze(2), xd.unsqueeze(2), st, th, 0.7, penalise_dc=False)
    assert xnew6.shape == (2, 5, 1, 5, 13, 2) and same_bits(xnew6.squeeze(2).cpu(), want[0])


def test_refusals_come_before_anything_is_written(dev):
    shape = (1, 5, 5, 13)
    b, t, h, w = shape
    z, g, xp = operands(shape, 3)
    k = Call(dev, 0)
    zi, gi, xi = k.inp(z), k.inp(g), k.inp(xp)
    si, ti = k.raw(torch.tensor([STEP])), k.raw(torch.tensor([0.5]))
    xo, zo, rec = k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2)), k.out((4,))
    need = L().cine_kt_prox_ws_bytes(b, t, h, w)
    ws = k.ws(need)
    base = dict(z=ptr(zi), g=ptr(gi), xprev=ptr(xi), step=ptr(si), thresh=ptr(ti), xnew=xo.ptr(), znew=zo.ptr(), rec=rec.ptr(), b=b, t=t, h=h, w=w,
                ws=ws.ptr(), nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_kt_prox(a["z"], a["g"], a["xprev"], a["step"], a["thresh"], 0.5, 1, a["xnew"], a["znew"], a["rec"],
                                        a["b"], a["t"], a["h"], a["w"], a["ws"], a["nbytes"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_kt_prox t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_kt_prox t = 65")
    refused(call(b=65536), EUNSUPPORTED, k, "cine_kt_prox b = 65536")
    for n in ("z", "g", "xprev", "step", "thresh", "xnew", "znew", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_kt_prox {n} = NULL")
    for n in ("b", "t", "h", "w"):
        refused(call(**{n: 0}), EINVAL, k, f"cine_kt_prox {n} = 0")
    refused(call(g=base["z"]), EINVAL, k, "cine_kt_prox z passed as g")
    refused(call(xnew=base["znew"]), EINVAL, k, "cine_kt_prox xnew aliases znew")
    refused(call(xnew=base["g"]), EINVAL, k, "cine_kt_prox xnew aliases g")
    refused(call(znew=base["g"]), EINVAL, k, "cine_kt_prox znew aliases g")
    refused(call(xnew=base["z"]), EINVAL, k, "cine_kt_prox xnew aliases z")
    refused(call(znew=base["xprev"]), EINVAL, k, "cine_kt_prox znew aliases xprev")
    refused(call(rec=base["xnew"]), EINVAL, k, "cine_kt_prox rec aliases xnew")
    refused(call(rec=base["ws"]), EINVAL, k, "cine_kt_prox rec aliases ws")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_kt_prox a workspace one byte short")
    check(call()(), "cine_kt_prox")                                                          # and the same operands are accepted as they stand
    k.finish("cine_kt_prox")
    assert bool(torch.isfinite(xo.t).all()) and bool(torch.isfinite(rec.t).all())
