"""cine_tv_pd_step (everything after the gradient of one Condat-Vu iteration of spatio-temporal TV, one launch) through the C ABI, shape by
shape against tests/tv_reference.py in float64, with the kernel_sweep harness: guarded outputs, an exact-size workspace with a sentinel
tail, two calls with equal bits, refusals that write nothing.

Shapes (b, t, h, w): the image sizes of the solver's cases -- (1, 5, 24, 20), (1, 7, 21, 17) (odd, no multiple of the tile), (2, 3, 200, 12)
-- and (1, 2, 1, 9), (1, 2, 9, 1) (a length-1 spatial axis), (2, 64, th + 1, tw + 1) (the frame limit, and one pixel past a tile seam in
both directions), (1, 3, 2 th, 2 tw) (exact tile multiples), with (th, tw) = cine_tv_pd_tile().  Per shape terms 1, 2, 3 and periodic 0, 1,
with lam_t and lam_s at the median of |p + sigma D (2 xnew - x)| in float64, so that about half of the points lie inside their ball.  The
planes of a term that is off hold NaN in p and keep their fill in pnew: they are neither read nor written.

Bars: xnew and pnew within kernel_sweep.BAR = 1e-5 of their float64 peaks (the step is affine, the projection 1-Lipschitz and continuous
on the sphere, so the fixture needs no margin around it), the record within SUM_REL = 1e-4 relative, 0 exactly for a term that is off.
The operators as the kernel applies them: with x = g = 0 and tau = 1 xnew is -D^H p, with p = 0, tau = 0, sigma = 1 and a huge lam pnew is
D x; <D x, p> = <x, D^H p> on those device results to 1e-5 -- the test that catches a wrong seam or boundary rule."""
import numpy as np
import pytest
import torch

import kt_reference as K
import tv_reference as R
from conftest import rnd
from kernel_sweep import BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, NAN, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
SUM_REL = 1e-4
TAU, SIGMA = 0.7, 0.4
SHAPES = {"solve-24x20": (1, 5, 24, 20), "solve-21x17": (1, 7, 21, 17), "solve-200x12": (2, 3, 200, 12), "h1": (1, 2, 1, 9), "w1": (1, 2, 9, 1),
          "seam": (2, 64, "th+1", "tw+1"), "multiple": (1, 3, "2th", "2tw")}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def tile():
    import ctypes
    th, tw = ctypes.c_int(0), ctypes.c_int(0)
    check(L().cine_tv_pd_tile(ctypes.byref(th), ctypes.byref(tw)), "cine_tv_pd_tile")
    return th.value, tw.value


def resolve(shape):
    th, tw = tile()
    names = {"th+1": th + 1, "tw+1": tw + 1, "2th": 2 * th, "2tw": 2 * tw}
    return tuple(names.get(v, v) for v in shape)


def test_the_tile_and_the_workspace_size(dev):
    from cine_hip import ops
    th, tw = tile()
    assert (th, tw) == ops.tv_pd_tile() and th >= 1 and tw >= 1
    assert L().cine_tv_pd_tile(None, None) == EINVAL
    one = L().cine_tv_pd_ws_bytes(1, 2, th, tw)
    assert one > 0 and one % 16 == 0                                                  # whole records of 4 floats
    assert L().cine_tv_pd_ws_bytes(1, 2, th + 1, tw) == 2 * one == L().cine_tv_pd_ws_bytes(1, 2, th, tw + 1) == L().cine_tv_pd_ws_bytes(2, 2, th, tw)
    assert L().cine_tv_pd_ws_bytes(1, 2, 2 * th, 2 * tw) == 4 * one
    assert L().cine_tv_pd_ws_bytes(0, 2, th, tw) == 0


def operands(shape, seed, terms):
    """x, g (b, t, h, w, 2) and p (3, b, t, h, w, 2) with NaN in the planes of a term that is off."""
    b, t, h, w = shape
    x, g, p = rnd(seed, b, t, h, w, 2), rnd(seed + 1, b, t, h, w, 2), rnd(seed + 2, 3, b, t, h, w, 2)
    if not terms & 1:
        p[0] = NAN
    if not terms & 2:
        p[1:] = NAN
    return x, g, p


def dual64(p, terms):
    """p as complex128 with zeros where the term is off (the yardstick never looks at them either)."""
    q = p.clone()
    if not terms & 1:
        q[0] = 0
    if not terms & 2:
        q[1:] = 0
    return K.to_complex(q)


def step_call(k, x, g, p, scal, terms, periodic, shape, record=True):
    b, t, h, w = shape
    xi, gi, pi = k.inp(x), k.inp(g), k.inp(p)
    sc = [k.raw(torch.tensor([v], dtype=torch.float32)) for v in scal]                # tau, sigma, lam_t, lam_s
    xo, po = k.out((b, t, h, w, 2)), k.out((3, b, t, h, w, 2))
    rec = k.out((4,)) if record else None
    nbytes = L().cine_tv_pd_ws_bytes(b, t, h, w) if record else 0
    ws = k.ws(nbytes)
    check(L().cine_tv_pd_step(ptr(xi), ptr(gi), ptr(pi), ptr(sc[0]), ptr(sc[1]), ptr(sc[2]), ptr(sc[3]), terms, int(periodic), xo.ptr(), po.ptr(),
                              rec.ptr() if record else None, b, t, h, w, ws.ptr() if ws else None, nbytes, stream()), "cine_tv_pd_step")
    return [xo.t, po.t] + ([rec.t] if record else [])


def on_planes(terms):
    return ([0] if terms & 1 else []) + ([1, 2] if terms & 2 else [])


def check_off_planes_keep_their_fill(pnew, terms, what):
    for q in range(3):
        if q not in on_planes(terms):
            assert bool(torch.isnan(pnew[q]).all()), f"{what}: plane {q} of a term that is off was written"


def check_case(dev, shape, seed):
    f32 = lambda v: float(np.float32(v))
    tau, sigma = f32(TAU), f32(SIGMA)
    for terms in (1, 2, 3):
        x, g, p = operands(shape, seed, terms)
        x64, g64, p64 = K.to_complex(x), K.to_complex(g), dual64(p, terms)
        for periodic in (True, False):
            what = f"cine_tv_pd_step {shape} terms {terms} periodic {int(periodic)}"
            xn64 = x64 - tau * (g64 + R.DH(p64, periodic, terms))
            v = p64 + sigma * R.D(2.0 * xn64 - x64, periodic, terms)
            mag_t, mag_s = np.abs(v[0]), np.sqrt(np.abs(v[1]) ** 2 + np.abs(v[2]) ** 2)
            lam_t, lam_s = f32(np.median(mag_t)) if terms & 1 else 1.0, f32(np.median(mag_s)) if terms & 2 else 1.0
            if terms & 1:
                assert (mag_t < lam_t).any() and (mag_t > lam_t).any(), what                     # the fixture: points inside and outside the ball
            if terms & 2:
                assert (mag_s < lam_s).any() and (mag_s > lam_s).any(), what
            want_x, want_p, want_rec = R.step(x64, g64, p64, tau, sigma, lam_t, lam_s, periodic, terms)
            assert np.array_equal(want_x, xn64)
            xnew, pnew, rec = twice(dev, 2, lambda k: step_call(k, x, g, p, (tau, sigma, lam_t, lam_s), terms, periodic, shape), what)
            check_off_planes_keep_their_fill(pnew, terms, what)
            on = on_planes(terms)
            ex = float(np.abs(K.to_complex(xnew) - want_x).max() / np.abs(want_x).max())
            ep = float(np.abs(K.to_complex(pnew[on]) - want_p[on]).max() / np.abs(want_p[on]).max())
            es = []
            for q in range(4):
                if (q == 2 and not terms & 1) or (q == 3 and not terms & 2) or want_rec[q] == 0.0:
                    assert float(rec[q]) == 0.0, (what, q, float(rec[q]))                        # a term that is off, or a length-1 axis alone
                    es.append(0.0)
                else:
                    es.append(abs(float(rec[q]) - want_rec[q]) / want_rec[q])
            print(f"{what}: xnew {ex:.2e}, pnew {ep:.2e} of the float64 peak (bar {BAR:.0e}); sums " + " ".join(f"{e:.2e}" for e in es) +
                  f" relative (bar {SUM_REL:.0e})")
            assert ex <= BAR and ep <= BAR, (what, ex, ep)
            assert max(es) <= SUM_REL, (what, es)
            k = Call(dev, 0)                                                                      # without the record: the same bits
            xn, pn = step_call(k, x, g, p, (tau, sigma, lam_t, lam_s), terms, periodic, shape, record=False)
            k.finish(what + " without a record")
            assert same_bits(xn.cpu(), xnew) and same_bits(pn.cpu()[on], pnew[on]), what + ": other bits without the record"


@pytest.mark.parametrize("name", list(SHAPES))
def test_step_vs_float64(dev, name):
    shape = resolve(SHAPES[name])
    check_case(dev, shape, seed=100 + 7 * len(name) + sum(shape))


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_kernels_d_and_dh_are_adjoint(dev, name):
    """-D^H p and D x read off the kernel; <D x, p> = <x, D^H p> with float64 sums on the host."""
    shape = resolve(SHAPES[name])
    b, t, h, w = shape
    x, _, p = operands(shape, 900 + sum(shape), 3)
    zero_x, zero_p = torch.zeros_like(x), torch.zeros_like(p)
    for periodic in (True, False):
        for terms in (1, 2, 3):
            what = f"cine_tv_pd_step {shape} terms {terms} periodic {int(periodic)} as an operator"
            k = Call(dev, 0)
            dhp, _ = step_call(k, zero_x, zero_x, p, (1.0, 0.0, 1e30, 1e30), terms, periodic, shape, record=False)       # xnew = -D^H p
            k.finish(what)
            k = Call(dev, 0)
            xn, dx = step_call(k, x, zero_x, zero_p, (0.0, 1.0, 1e30, 1e30), terms, periodic, shape, record=False)       # pnew = D (2 x - x)
            k.finish(what)
            assert same_bits(xn.cpu(), x)                                                                               # tau = 0: xnew is x
            on = on_planes(terms)
            dhp64, dx64 = -K.to_complex(dhp.cpu()), K.to_complex(dx.cpu()[on])
            x64, p64 = K.to_complex(x), K.to_complex(p)
            lhs, rhs = np.vdot(p64[on], dx64), np.vdot(dhp64, x64)
            scale = np.linalg.norm(x64) * np.linalg.norm(p64[on])
            print(f"{what}: <D x, p> - <x, D^H p> = {abs(lhs - rhs) / scale:.2e} of |x| |p| (bar 1e-5)")
            assert abs(lhs - rhs) <= 1e-5 * scale, (what, lhs, rhs)
            # and each of them is the yardstick's (differences of float32 values are exact or rounded once)
            want_d = R.D(x64, periodic, terms)[on]
            assert np.abs(dx64 - want_d).max() <= 1e-6 * np.abs(x64).max(), what
            want_dh = R.DH(dual64(p, 3), periodic, terms)
            assert np.abs(dhp64 - want_dh).max() <= 1e-6 * 6 * np.abs(p64).max(), what


def test_the_binding_gives_the_bits_of_the_c_call(dev):
    from cine_hip import ops
    shape = (2, 3, 11, 37)
    f32 = lambda v: float(np.float32(v))
    scal = (f32(TAU), f32(SIGMA), f32(0.9), f32(1.3))
    for terms in (3, 1):
        x, g, p = operands(shape, 9, terms)
        want = twice(dev, 0, lambda k: step_call(k, x, g, p, scal, terms, True, shape), "cine_tv_pd_step")
        xd, gd, pd = x.to(dev), g.to(dev), p.to(dev)
        sc = [torch.tensor([v], device=dev) for v in scal]
        xnew, pnew, rec = ops.tv_pd_step(xd, gd, pd, *sc, terms=terms, periodic=True, record=True)
        on = on_planes(terms)
        assert same_bits(xnew.cpu(), want[0]) and same_bits(pnew.cpu()[on], want[1][on]) and same_bits(rec.cpu(), want[2])
        if terms == 1:
            assert not pnew[1:].any()                                                 # a pnew made by the binding: zeros where the term is off
            xnew1, _ = ops.tv_pd_step(xd, gd, pd, sc[0], sc[1], sc[2], None, terms=1)  # the lam of a term that is off may be None
            assert same_bits(xnew1.cpu(), want[0])
        x6, p6 = ops.tv_pd_step(xd.unsqueeze(2), gd.unsqueeze(2), pd.unsqueeze(3), *sc, terms=terms)
        assert x6.shape == (2, 3, 1, 11, 37, 2) and p6.shape == (3, 2, 3, 1, 11, 37, 2) and same_bits(x6.squeeze(2).cpu(), want[0])
    with pytest.raises(ValueError):
        ops.tv_pd_step(xd, gd, pd, *sc, terms=0)
    from cine_hip._lib import CineHipError
    with pytest.raises(CineHipError, match="alias"):
        ops.tv_pd_step(xd, gd, pd, *sc, xnew=xd)


def test_refusals_come_before_anything_is_written(dev):
    shape = (1, 5, 9, 35)
    b, t, h, w = shape
    x, g, p = operands(shape, 3, 3)
    k = Call(dev, 0)
    xi, gi, pi = k.inp(x), k.inp(g), k.inp(p)
    sc = [k.raw(torch.tensor([v], dtype=torch.float32)) for v in (TAU, SIGMA, 0.9, 1.3)]
    xo, po, rec = k.out((b, t, h, w, 2)), k.out((3, b, t, h, w, 2)), k.out((4,))
    need = L().cine_tv_pd_ws_bytes(b, t, h, w)
    ws = k.ws(need)
    base = dict(x=ptr(xi), g=ptr(gi), p=ptr(pi), tau=ptr(sc[0]), sigma=ptr(sc[1]), lam_t=ptr(sc[2]), lam_s=ptr(sc[3]), terms=3, xnew=xo.ptr(),
                pnew=po.ptr(), rec=rec.ptr(), b=b, t=t, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_tv_pd_step(a["x"], a["g"], a["p"], a["tau"], a["sigma"], a["lam_t"], a["lam_s"], a["terms"], 1, a["xnew"], a["pnew"],
                                           a["rec"], a["b"], a["t"], a["h"], a["w"], a["ws"], a["nbytes"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_tv_pd_step t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_tv_pd_step t = 65")
    refused(call(b=65536), EUNSUPPORTED, k, "cine_tv_pd_step b = 65536")
    for n in ("x", "g", "p", "tau", "sigma", "lam_t", "lam_s", "xnew", "pnew", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_tv_pd_step {n} = NULL")
    for n in ("b", "t", "h", "w"):
        refused(call(**{n: 0}), EINVAL, k, f"cine_tv_pd_step {n} = 0")
    refused(call(xnew=base["x"]), EINVAL, k, "cine_tv_pd_step xnew aliases x")
    refused(call(pnew=base["p"]), EINVAL, k, "cine_tv_pd_step pnew aliases p")
    refused(call(xnew=base["g"]), EINVAL, k, "cine_tv_pd_step xnew aliases g")
    refused(call(xnew=base["p"]), EINVAL, k, "cine_tv_pd_step xnew aliases p")
    refused(call(pnew=base["x"]), EINVAL, k, "cine_tv_pd_step pnew aliases x")
    refused(call(pnew=base["g"]), EINVAL, k, "cine_tv_pd_step pnew aliases g")
    refused(call(pnew=base["xnew"]), EINVAL, k, "cine_tv_pd_step pnew aliases xnew")
    refused(call(rec=base["xnew"]), EINVAL, k, "cine_tv_pd_step rec aliases xnew")
    refused(call(rec=base["ws"]), EINVAL, k, "cine_tv_pd_step rec aliases ws")
    refused(call(terms=0), EINVAL, k, "cine_tv_pd_step terms = 0")
    refused(call(terms=4), EINVAL, k, "cine_tv_pd_step terms = 4")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_tv_pd_step a workspace one byte short")
    check(call()(), "cine_tv_pd_step")                                                # and the same operands are accepted as they stand
    k.finish("cine_tv_pd_step")
    assert bool(torch.isfinite(xo.t).all()) and bool(torch.isfinite(po.t).all()) and bool(torch.isfinite(rec.t).all())
