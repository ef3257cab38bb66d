"""cine_grappa_image_weights and cine_grappa_gfactor through ctypes against float64 (tests/grappa_gfactor_reference.py), the contract of
include/cine_hip.h.  The bars are derived there, not tuned: one rounding per fmaf of every chain (row offsets, Cholesky factor, column
offsets, coils), 8 * 2^-24 for each phase factor (one rounded division in the argument, sincospif to 2 ulp), the sum of squares and the
root; every component of every output must lie within its own bound.  The worst fraction met is printed."""
import numpy as np
import pytest
import torch

import grappa_gfactor_reference as gref
from kernel_sweep import EINVAL, EUNSUPPORTED, Call, L, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu

# c, h, w, R, ky, kx
SHAPES = [(1, 4, 3, 2, 2, 3),          # the smallest
          (3, 13, 10, 3, 2, 5),        # odd sizes, h no multiple of R
          (4, 24, 16, 4, 4, 7),        # ky = 4, the widest kernel
          (32, 8, 66, 2, 2, 3),        # the coil limit, w just over one wave
          (5, 7, 130, 8, 2, 3)]        # R = 8, two full lane tiles and a remainder
IDS = ["c%d-%dx%d-R%d-k%dx%d" % s for s in SHAPES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def pairs(z):
    z = np.asarray(z)
    return torch.from_numpy(np.stack((z.real, z.imag), -1).astype(np.float32))


def crandn(rs, *shape):
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)


_CASES = {}


def case(shape):
    """Per shape, once: random complex64 weights, a Cholesky factor of a random positive-definite matrix with NaN above the diagonal
    (the entry reads the lower triangle only) and three coefficient sets, one pixel of each all zero."""
    if shape not in _CASES:
        c, h, w, R, ky, kx = shape
        rs = np.random.RandomState(sum(a * b for a, b in zip(shape, (1, 3, 5, 7, 11, 13))))
        ns = ky * kx * c
        W = (crandn(rs, R - 1, ns, c) / np.sqrt(ns)).astype(np.complex64)
        M = crandn(rs, c, c).astype(np.complex128)
        low = np.linalg.cholesky(M @ M.conj().T / c + 0.25 * np.eye(c)).astype(np.complex64)
        chol = np.where(np.tril(np.ones((c, c), bool)), low, np.complex64(complex(np.nan, np.nan)))
        coef = crandn(rs, 3, c, h, w)
        zero = (h // 2, w - 1)
        coef[:, :, zero[0], zero[1]] = 0
        for a in (W, low, chol, coef):
            a.setflags(write=False)
        _CASES[shape] = {"W": W, "low": low, "chol": chol, "coef": coef, "zero": zero}
    return _CASES[shape]


# ================================================================== image weights
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_image_weights_against_float64(dev, shape):
    c, h, w, R, ky, kx = shape
    W = case(shape)["W"]

    def body(k):
        d_w = k.inp(pairs(W))
        out = k.out((c, c, h, w, 2))
        assert L().cine_grappa_image_weights(d_w.data_ptr(), out.ptr(), c, h, w, R, ky, kx, stream()) == 0, L().cine_last_error()
        return [out.t]

    got = twice(dev, 0, body, "cine_grappa_image_weights")[0].numpy().astype(np.float64)    # guards intact, the same bits on a second call
    want = gref.image_weights(W, c, R, ky, kx, h, w)
    bound = gref.image_weights_bound(W, c, R, ky, kx)[:, :, None, None]
    e_re, e_im = np.abs(got[..., 0] - want.real), np.abs(got[..., 1] - want.imag)
    worst = max(float((e_re / bound).max()), float((e_im / bound).max()))
    print(f"image weights {IDS[SHAPES.index(shape)]}: worst error {worst:.3f} of its bound")
    assert np.isfinite(got).all() and (e_re <= bound).all() and (e_im <= bound).all()


# ================================================================== g-factor
def call_gfactor(k, shape, W, chol, coef, want_g=True, want_amp=True):
    c, h, w, R, ky, kx = shape
    n = 1 if coef is None else coef.shape[0]
    maps = c if coef is None else n
    d_w = k.inp(pairs(W))
    d_l = None if chol is None else k.inp_among_nan(pairs(chol))
    d_c = None if coef is None else k.inp_among_nan(pairs(coef))
    g = k.out((maps, h, w)) if want_g else None
    amp = k.out((maps, h, w)) if want_amp else None
    code = L().cine_grappa_gfactor(d_w.data_ptr(), None if d_l is None else d_l.data_ptr(), None if d_c is None else d_c.data_ptr(),
                                   None if g is None else g.ptr(), None if amp is None else amp.ptr(), n, c, h, w, R, ky, kx, stream())
    assert code == 0, L().cine_last_error()
    return [o.t for o in (g, amp) if o is not None]


@pytest.mark.parametrize("with_chol", [False, True], ids=["white", "chol"])
@pytest.mark.parametrize("n", [0, 1, 3], ids=["per-coil", "n1", "n3"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gfactor_against_float64(dev, shape, n, with_chol):
    c, h, w, R, ky, kx = shape
    cs = case(shape)
    W, coef = cs["W"], (cs["coef"][:n] if n else None)
    chol = cs["chol"] if with_chol else None
    what = "cine_grappa_gfactor"
    got_g, got_amp = twice(dev, 0, lambda k: call_gfactor(k, shape, W, chol, coef), what)
    only_g = twice(dev, 0, lambda k: call_gfactor(k, shape, W, chol, coef, want_amp=False), what + " without amp")[0]
    only_amp = twice(dev, 0, lambda k: call_gfactor(k, shape, W, chol, coef, want_g=False), what + " without g")[0]
    assert same_bits(only_g, got_g) and same_bits(only_amp, got_amp), "a null output changes the other one's bits"

    g, amp, g_b, amp_b = gref.gfactor(W, c, R, ky, kx, h, w, chol=cs["low"] if with_chol else None, coef=coef, bound=True)
    got_g, got_amp = got_g.numpy().astype(np.float64), got_amp.numpy().astype(np.float64)
    assert got_g.shape == g.shape and np.isfinite(got_g).all() and np.isfinite(got_amp).all()
    e_g, e_a = np.abs(got_g - g), np.abs(got_amp - amp)
    live = g_b > 0
    worst = max(float((e_g[live] / g_b[live]).max()), float((e_a[amp_b > 0] / amp_b[amp_b > 0]).max()))
    print(f"gfactor {IDS[SHAPES.index(shape)]} n {n} chol {with_chol}: g in [{g[live].min():.3f}, {g.max():.3f}], worst error {worst:.3f} of "
          f"its bound")
    assert (e_g <= g_b).all() and (e_a <= amp_b).all()
    if n:
        y, x = cs["zero"]
        assert (got_g[:, y, x] == 0).all() and (got_amp[:, y, x] == 0).all()           # p = 0: no combination, g = 0 by definition
        assert (got_g.reshape(n, -1)[:, :y * w + x] > 0).all()


# ================================================================== refusals
def test_refusals(dev):
    shape = SHAPES[1]
    c, h, w, R, ky, kx = shape
    cs = case(shape)
    lib = L()
    k = Call(dev, 0)
    d_w = k.inp(pairs(cs["W"]))
    d_l = k.inp(pairs(cs["low"]))
    d_c = k.inp(pairs(cs["coef"][:1]))
    g, amp = k.out((1, h, w)), k.out((1, h, w))
    wimg = k.out((c, c, h, w, 2))
    names = ["weights", "chol", "coef", "g", "amp", "n", "c", "h", "w", "R", "ky", "kx"]
    good = [d_w.data_ptr(), d_l.data_ptr(), d_c.data_ptr(), g.ptr(), amp.ptr(), 1, c, h, w, R, ky, kx]

    def bad(want, what, **kw):
        args = [kw.get(nm, v) for nm, v in zip(names, good)]
        refused(lambda: lib.cine_grappa_gfactor(*args, stream()), want, k, f"cine_grappa_gfactor {what}")

    bad(EINVAL, "null weights", weights=None)
    bad(EINVAL, "neither g nor amp", g=None, amp=None)
    bad(EINVAL, "weights off their alignment", weights=d_w.data_ptr() + 4)
    bad(EINVAL, "chol off its alignment", chol=d_l.data_ptr() + 4)
    bad(EINVAL, "coef off its alignment", coef=d_c.data_ptr() + 4)
    bad(EINVAL, "g off its alignment", g=g.ptr() + 2)
    bad(EINVAL, "amp off its alignment", amp=amp.ptr() + 1)
    bad(EINVAL, "g is amp", amp=g.ptr())
    bad(EINVAL, "g overlaps amp", amp=g.ptr() + 4 * (h * w - 1))
    bad(EINVAL, "g is coef", g=d_c.data_ptr())
    bad(EINVAL, "amp inside coef", amp=d_c.data_ptr() + 8 * (c * h * w - 1))
    bad(EINVAL, "g is the weights", g=d_w.data_ptr())
    bad(EINVAL, "amp is chol", amp=d_l.data_ptr())
    for nm in ("n", "c", "h", "w"):
        bad(EINVAL, f"{nm} = 0", **{nm: 0})
    bad(EINVAL, "R = 1", R=1)
    bad(EINVAL, "R = 9", R=9)
    bad(EINVAL, "ky = 3", ky=3)
    bad(EINVAL, "kx = 4", kx=4)
    bad(EUNSUPPORTED, "33 coils", c=33)
    bad(EUNSUPPORTED, "h above 2^20", h=(1 << 20) + 1)
    bad(EUNSUPPORTED, "w above 2^20", w=(1 << 20) + 1)

    inames = ["weights", "out", "c", "h", "w", "R", "ky", "kx"]
    igood = [d_w.data_ptr(), wimg.ptr(), c, h, w, R, ky, kx]

    def ibad(want, what, **kw):
        args = [kw.get(nm, v) for nm, v in zip(inames, igood)]
        refused(lambda: lib.cine_grappa_image_weights(*args, stream()), want, k, f"cine_grappa_image_weights {what}")

    ibad(EINVAL, "null weights", weights=None)
    ibad(EINVAL, "null out", out=None)
    ibad(EINVAL, "weights off their alignment", weights=d_w.data_ptr() + 4)
    ibad(EINVAL, "out off its alignment", out=wimg.ptr() + 4)
    ibad(EINVAL, "out is the weights", out=d_w.data_ptr())
    ibad(EINVAL, "out ends inside the weights", weights=wimg.ptr() + 8 * (c * c * h * w - 1))
    for nm in ("c", "h", "w"):
        ibad(EINVAL, f"{nm} = 0", **{nm: 0})
    ibad(EINVAL, "R = 1", R=1)
    ibad(EINVAL, "R = 9", R=9)
    ibad(EINVAL, "ky = 3", ky=3)
    ibad(EINVAL, "kx = 4", kx=4)
    ibad(EUNSUPPORTED, "33 coils", c=33)
    ibad(EUNSUPPORTED, "h above 2^20", h=(1 << 20) + 1)

    assert lib.cine_grappa_gfactor(*good, stream()) == 0, lib.cine_last_error()          # and both calls work after every refusal
    assert lib.cine_grappa_image_weights(*igood, stream()) == 0, lib.cine_last_error()
    k.finish("the calls after the refusals")
    want_g, want_amp = gref.gfactor(cs["W"], c, R, ky, kx, h, w, chol=cs["low"], coef=cs["coef"][:1])
    assert np.abs(g.t.cpu().numpy() - want_g).max() <= 1e-4 * want_g.max() and np.abs(amp.t.cpu().numpy() - want_amp).max() <= 1e-4 * want_amp.max()
    assert bool(torch.isfinite(wimg.t).all())
