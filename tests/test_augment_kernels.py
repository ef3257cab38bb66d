"""cine_affine_warp through ctypes against float64 (tests/augment_reference.py, itself held against grid_sample in test_augment_cpu.py).

The sweep: (h, w) in {(1,1), (1,7), (2,3), (5,8), (17,33), (64,64), (70,130)} -- a tile is 8 rows x 32 columns, so the last two cross tile
edges in both directions -- x (frames, inner) in {(1,1), (3,2), (4,5)} x both modes x both borders x the maps of
augment_reference.matrices (identity, both flips, the quarter turn on square planes, an integer shift, shifts of 2.5 / -3.7 and 3.7 / 2.5
image sizes, a rotation by 37 degrees, an anisotropic scale with shear, the all-zero matrix) x every t_shift with and without t_reverse
x in / out on a 16-byte boundary and 8 bytes past one.  EVERY output component of every case is compared.

The bar, with u = 2^-24 (float32 unit roundoff) and the sum over the taps of the output's footprint that count:

    |got - ref| <= C u sum_k |x_k|,    C = 8 bilinear, 24 bicubic.

Where C comes from.  The float64 coordinate is good to 1e-9 pixels at worst (|coordinate| < 2^24); its fraction f in [0, 1) is rounded to
float32 once, |df| <= u / 2.
  bilinear   w1 = f: u / 2.  w0 = 1 - f: df plus one rounding of a value <= 1: u.  A tap's weight wy wx is never formed; its error is
             <= |dwy| |wx| + |wy| |dwx| <= 2 u.  The chain rounds a tap's term at most twice in the row sum and twice in the column
             sum: 4 u |w| <= 4 u.  Together 6 u per tap; C = 8 leaves room for the second-order terms.
  bicubic    near(x) = ((A + 2) x - (A + 3)) x^2 + 1 on [0, 1], evaluated as fmaf(fmaf(1.25, x, -2.25) x, x, 1): the inner fmaf
             (|.| <= 2.25, ulp 2^-22) 2 u, the product (|.| <= 2.25) its own 2 u plus the inherited 2 u, the last fmaf (|.| <= 1) u / 2
             plus 4 u: 4.5 u; the argument (f, or 1 - f with its rounding) is off by <= u and |near'| <= 1.35: 6 u in all.
             far(x) = ((A x - 5 A) x + 8 A) x - 4 A on [1, 2], three fmafs: 2 u (|.| <= 3), then 2 * 2 u + 2 u = 6 u (|.| <= 3.75), then
             2 * 6 u + (a rounding of |.| <= 0.112) = 12.1 u; the argument 1 + f or 2 - f is off by <= 1.5 u and |far'| <= 0.75: 13.2 u.
             |near| <= 1, |far| <= 0.112, so a tap's weight is off by <= 13.2 u * 1 + 0.112 * 6 u < 14 u (far x near), 12 u (near x
             near), 3 u (far x far).  The chain rounds a term at most four times in the row sum and four times in the column sum:
             8 u |w| <= 8 u.  Together 22 u per tap; C = 24.
Both are worst cases over every rounding at once; the sweep prints the worst ratio it meets (DESIGN.md section 3 "Augmentation" has it).
A wrong tap, a reflection off by one or a swapped axis is wrong by order |x|, five orders above the bar."""
import numpy as np
import pytest
import torch

import augment_reference as R
from kernel_sweep import EINVAL, EUNSUPPORTED, GUARD, GUARD_VALUE, L, same_bits, stream

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (2, 3), (5, 8), (17, 33), (64, 64), (70, 130)]
FRAMES_INNER = [(1, 1), (3, 2), (4, 5)]
PLANES = max(f * i for f, i in FRAMES_INNER)
OFFSETS = (0, 2)                                                             # floats past a 16-byte boundary


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


class Placed:
    """A float32 device tensor of `shape` `off` floats past a 16-byte boundary, between guard floats."""

    def __init__(self, shape, off, dev, values=None):
        self.n = int(np.prod(shape))
        self.lo = 4 * ((GUARD + 3) // 4) + off
        self.buf = torch.full((self.lo + self.n + GUARD,), GUARD_VALUE, device=dev)
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        assert (self.t.data_ptr() - 4 * off) % 16 == 0 and self.t.data_ptr() % 8 == 0
        if values is not None:
            self.t.copy_(values)

    def broken(self):
        """A device bool: a guard float changed."""
        return (self.buf[:self.lo] != GUARD_VALUE).any() | (self.buf[self.lo + self.n:] != GUARD_VALUE).any()


def call(x, out, m, mode, border, t_shift=0, t_reverse=0):
    frames, inner, h, w, _ = x.shape
    (ayy, ayx, by), (axy, axx, bx) = m
    return L().cine_affine_warp(x.data_ptr(), out.data_ptr(), frames, inner, h, w, ayy, ayx, by, axy, axx, bx, mode, border, t_shift,
                                t_reverse, stream())


def bits_differ(a, b):
    return (a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).any()


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_affine_warp_against_float64(dev, hw):
    h, w = hw
    x_all = np.random.RandomState(1000 * h + w).standard_normal((PLANES, h, w, 2)).astype(np.float32)
    ins, outs = {}, {}
    for frames, inner in FRAMES_INNER:
        for off in OFFSETS:
            shape = (frames, inner, h, w, 2)
            ins[frames, inner, off] = Placed(shape, off, dev, torch.from_numpy(x_all[:frames * inner].reshape(shape)))
            outs[frames, inner, off] = Placed(shape, off, dev)
    worst = {0: (0.0, None), 1: (0.0, None)}
    for name, m in R.matrices(h, w).items():
        for mode in (0, 1):
            for border in (0, 1):
                ref, foot = R.warp_planes(x_all, m, mode, border)
                ref_d = torch.from_numpy(ref).to(dev)
                bar_d = torch.from_numpy(foot * R.U).to(dev)
                cases, ratios, flags = [], [], []
                for frames, inner in FRAMES_INNER:
                    shape = (frames, inner, h, w, 2)
                    r_fi, b_fi = ref_d[:frames * inner].view(shape), bar_d[:frames * inner].view(shape)
                    for t_shift in range(frames):
                        for t_reverse in (0, 1):
                            g = torch.from_numpy(R.frame_map(frames, t_shift, bool(t_reverse))).to(dev)
                            first = None
                            for off in OFFSETS:
                                xi, xo = ins[frames, inner, off], outs[frames, inner, off]
                                xo.t.fill_(float("nan"))
                                assert call(xi.t, xo.t, m, mode, border, t_shift, t_reverse) == 0, L().cine_last_error()
                                got = xo.t.clone()
                                err = (got.double() - r_fi[g]).abs()
                                ratios.append((err / b_fi[g].clamp_min(1e-300)).max())   # no tap counts: the bar is 0 and so must the error be
                                bad = xo.broken() | xi.broken()
                                xo.t.fill_(float("inf"))                                 # what out held does not matter; the same bits again
                                assert call(xi.t, xo.t, m, mode, border, t_shift, t_reverse) == 0
                                bad = bad | bits_differ(xo.t, got)
                                if first is None:
                                    first = got
                                else:
                                    bad = bad | bits_differ(got, first)                  # the other placement: the same bits
                                flags.append(bad)
                                cases.append(f"{h}x{w} {name} mode {mode} border {border} frames {frames} inner {inner} t_shift {t_shift} "
                                             f"t_reverse {t_reverse} offset {off}")
                ratios, flags = torch.stack(ratios).cpu().numpy(), torch.stack(flags).cpu().numpy()
                for case, ratio, bad in zip(cases, ratios, flags):
                    assert not bad, f"{case}: a guard float changed, or a second call / the other placement gave other bits"
                    assert ratio <= R.C_BAR[mode], f"{case}: worst |got - ref| = {ratio:.3g} u sum |taps|, the bar is {R.C_BAR[mode]:g}"
                k = int(np.argmax(ratios))
                if ratios[k] > worst[mode][0]:
                    worst[mode] = (float(ratios[k]), cases[k])
    for (frames, inner, off), xi in ins.items():
        shape = (frames, inner, h, w, 2)
        assert same_bits(xi.t.cpu(), torch.from_numpy(x_all[:frames * inner].reshape(shape))), "in was written"
    for mode in (0, 1):
        print(f"{h}x{w} {('bilinear', 'bicubic')[mode]}: worst error {worst[mode][0]:.3f} u sum|taps| (bar {R.C_BAR[mode]:g}) at {worst[mode][1]}")


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 8), (64, 64), (70, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_affine_warp_bit_for_bit_cases(dev, hw):
    h, w = hw
    frames, inner = 4, 3
    x = torch.from_numpy(np.random.RandomState(77 * h + w).standard_normal((frames, inner, h, w, 2)).astype(np.float32)).to(dev)
    ms = R.matrices(h, w)
    out = torch.empty_like(x)

    def run(m, mode, border, t_shift=0, t_reverse=0):
        out.fill_(float("nan"))
        assert call(x, out, m, mode, border, t_shift, t_reverse) == 0, L().cine_last_error()
        return out.clone()

    for mode in (0, 1):
        for border in (0, 1):
            what = f"{h}x{w} mode {mode} border {border}"
            assert same_bits(run(ms["identity"], mode, border), x), f"{what}: identity"
            assert same_bits(run(ms["flip_h"], mode, border), torch.flip(x, (3,))), f"{what}: flip_h"
            assert same_bits(run(ms["flip_v"], mode, border), torch.flip(x, (2,))), f"{what}: flip_v"
            if h == w:
                for k in (1, 2, 3):
                    q = np.linalg.matrix_power(np.array([[0.0, 1.0], [-1.0, 0.0]]), k) + 0.0
                    m = ((q[0, 0], q[0, 1], 0.0), (q[1, 0], q[1, 1], 0.0))
                    assert same_bits(run(m, mode, border), torch.rot90(x, k, (2, 3))), f"{what}: {k} quarter turns"
            for s in range(frames):
                assert same_bits(run(ms["identity"], mode, border, s, 0), torch.roll(x, -s, 0)), f"{what}: t_shift {s}"
                assert same_bits(run(ms["identity"], mode, border, s, 1), torch.roll(torch.flip(x, (0,)), s + 1, 0)), f"{what}: t_shift {s} reversed"
            assert same_bits(run(ms["flip_h"], mode, border, 1, 1), torch.roll(torch.flip(x, (0, 3)), 2, 0)), f"{what}: flip_h with the frames reversed"
        # integer shifts under reflection: indexing a symmetrically padded copy (pads of several image sizes: repeated reflection)
        for sy, sx in ((2, -3), (-1, 1), (3 * h + 1, -2 * w - 2)):
            py, px = abs(sy) + 1, abs(sx) + 1
            pad = torch.from_numpy(np.pad(x.cpu().numpy(), ((0, 0), (0, 0), (py, py), (px, px), (0, 0)), mode="symmetric")).to(dev)
            want = pad[:, :, py + sy:py + sy + h, px + sx:px + sx + w]
            got = run(((1.0, 0.0, float(sy)), (0.0, 1.0, float(sx))), mode, 1)
            assert same_bits(got, want), f"{h}x{w} mode {mode}: integer shift ({sy}, {sx}) under reflection"
            # under border 0 the same shift is the zero-padded copy (zeros where no tap counts)
            zpad = torch.zeros_like(pad)
            zpad[:, :, py:py + h, px:px + w] = x
            got0 = run(((1.0, 0.0, float(sy)), (0.0, 1.0, float(sx))), mode, 0)
            assert torch.equal(got0, zpad[:, :, py + sy:py + sy + h, px + sx:px + sx + w]), f"{h}x{w} mode {mode}: integer shift, zero border"


def test_affine_warp_is_capturable(dev):
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((3, 2, 17, 33, 2)).astype(np.float32)).to(dev)
    m = R.matrices(17, 33)["rot37"]
    out = torch.full_like(x, float("nan"))
    assert call(x, out, m, 1, 1, 2, 1) == 0
    torch.cuda.synchronize()
    want = out.clone()
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        assert call(x, out, m, 1, 1, 2, 1) == 0
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, want)


def test_affine_warp_refusals_leave_out_untouched(dev):
    frames, inner, h, w = 3, 2, 5, 8
    shape = (frames, inner, h, w, 2)
    xi = Placed(shape, 0, dev, torch.from_numpy(np.random.RandomState(9).standard_normal(shape).astype(np.float32)))
    xo = Placed(shape, 0, dev)
    xo.t.fill_(float("nan"))
    lib = L()
    ip, op = xi.t.data_ptr(), xo.t.data_ptr()
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]

    def refused(want, args, word):
        assert lib.cine_scale(None, 1, 1.0, None) == EINVAL                   # another entry point's message, to be replaced
        assert lib.cine_affine_warp(*args, stream()) == want, args
        msg = lib.cine_last_error()
        assert msg.startswith(b"cine_affine_warp") and word in msg, msg
        torch.cuda.synchronize()
        assert bool(torch.isnan(xo.t).all()) and not bool(xo.broken()) and not bool(xi.broken()), "a refused call wrote"

    good = [ip, op, frames, inner, h, w] + ident + [1, 1, 0, 0]
    sub = lambda k, v: good[:k] + [v] + good[k + 1:]
    refused(EINVAL, sub(0, None), b"null")
    refused(EINVAL, sub(1, None), b"null")
    for k in (2, 3, 4, 5):                                                    # frames, inner, h, w below 1
        refused(EINVAL, sub(k, 0), b"Invalid shapes")
        refused(EINVAL, sub(k, -2), b"Invalid shapes")
    refused(EUNSUPPORTED, sub(4, 4097), b"at most 4096")
    refused(EUNSUPPORTED, sub(5, 4097), b"at most 4096")
    for v in (-1, 2):
        refused(EINVAL, sub(12, v), b"mode")
        refused(EINVAL, sub(13, v), b"border")
    for k in (6, 7, 9, 10):                                                   # the linear part
        for v in (float("nan"), float("inf"), -float("inf"), 1024.5, -1025.0):
            refused(EINVAL, sub(k, v), b"matrix entry")
    for k in (8, 11):                                                         # the offsets
        for v in (float("nan"), float("inf"), 2.0 ** 20 + 1.0, -(2.0 ** 20) - 0.5):
            refused(EINVAL, sub(k, v), b"offset")
    refused(EINVAL, sub(14, -1), b"t_shift")
    refused(EINVAL, sub(14, frames), b"t_shift")
    refused(EINVAL, sub(0, ip + 4), b"8-byte aligned")
    refused(EINVAL, sub(1, op + 4), b"8-byte aligned")
    nbytes = 8 * frames * inner * h * w
    refused(EINVAL, sub(0, op), b"overlaps")                                  # in place
    refused(EINVAL, sub(0, op + nbytes - 8), b"overlaps")                     # in begins in out's last element
    refused(EINVAL, sub(0, op - nbytes + 8), b"overlaps")                     # in ends in out's first element
    refused(EINVAL, [ip, op, 2 ** 31 - 1, 2 ** 31 - 1, 4096, 4096] + good[6:], b"overflow")
    refused(EUNSUPPORTED, [op + 2 ** 44, op, 2 ** 31 - 1, 1, 8, 64] + good[6:], b"grid limit")     # refused before the launch: the sizes stand for no memory
    # the limits themselves pass, and the call works after every refusal
    assert lib.cine_affine_warp(*(good[:6] + [1024.0, -1024.0, 2.0 ** 20, 0.0, 0.0, -(2.0 ** 20)] + good[12:]), stream()) == 0, lib.cine_last_error()
    assert lib.cine_affine_warp(*good, stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(xo.t, xi.t) and not bool(xo.broken())
