"""cine_llr_prox through the C ABI, shape by shape against tests/llr_reference.py in float64 (numpy.linalg.svd per block), with the
kernel_sweep harness: guarded outputs, an exact-size workspace with a sentinel tail, two calls with equal bits, refusals that write nothing.

Shapes, the smallest at which the kernel can go wrong.  Block 8 with t in 2, 5, 15, 16, 64 over (h, w, shift) = (1, 1, (0, 0)) one clipped
block of one pixel, (7, 9, (0, 0)) a clipped block and a one-pixel-wide sliver, (8, 8, (0, 0)) the exact fit, (8, 8, (3, 5)) four clipped
blocks, (9, 17, (7, 1)) and (19, 13, (0, 7)) slivers beside whole blocks -- blocks with fewer pixels than frames among them, and at t = 64
the layout in which a block is staged tile by tile.  Blocks 2, 3, 4, 16 at t in 5, 15 with (h, w) = (2 block + 3, block + 1) and shift
(block - 1, 1).  t = 64 with block 16 at 35 x 19, the largest LDS layout.  Batch 2 once.

Bars.  xnew within kernel_sweep.BAR = 1e-5 of the float64 peak (the bar cine_ls_prox holds by the same route; the prox is 1-Lipschitz, so
no margin round a kink is needed); rec within SUM_REL = 1e-4 relative; info: sigma_max within 1e-10 relative of the float64 value on the
same float32 v, residual <= 1e-14, sweeps below the cap of 40, the block count exact.
The first sum, sum |xnew - x|^2, cannot be known better than the differences it squares: where xnew = x in exact arithmetic (threshold 0
without g) the yardstick itself returns only its rounding, 1e-29, and a relative bar means nothing.  So that sum alone also passes within
DIFF_FLOOR = N (BAR peak)^2, N the number of complex samples: the value it takes when every sample is off by xnew's own bar.  Measured
in that case on the MI355X: xnew 1.4e-7 of the peak; every other case holds the plain relative bar."""
import numpy as np
import pytest
import torch

import kt_reference as R
import llr_reference as LLR
from conftest import rnd
from kernel_sweep import BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
SUM_REL = 1e-4
STEP = 0.45
MAX_SWEEPS = 40
OFF = 2                                                            # storage offset of every float pointer: 8-byte aligned, not 16
FRAMES = [2, 5, 15, 16, 64]
PLACES = [(1, 1, (0, 0)), (7, 9, (0, 0)), (8, 8, (0, 0)), (8, 8, (3, 5)), (9, 17, (7, 1)), (19, 13, (0, 7))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def f64(t):
    """A float32 CPU tensor holding doubles -> float64 numpy."""
    return t.contiguous().view(torch.float64).numpy()


def prox_call(k, x, g, shape, block, shift, thresh, step=STEP, inplace=False, image=True, rec=True, info=True):
    """One cine_llr_prox call on fresh operands -> [xnew], [rec], [info as float pairs].  step None: no step pointer."""
    b, t, h, w = shape
    gi = k.inp(g)
    si = k.raw(torch.tensor([step])) if step is not None else None
    ti = k.raw(torch.tensor([thresh]))
    if inplace:
        xo = k.out((b, t, h, w, 2), fill=x)
        xi = xo.t
    else:
        xi = k.inp(x)
        xo = k.out((b, t, h, w, 2)) if image else None
    ro = k.out((4,)) if rec else None
    io = k.out((8,)) if info else None
    nbytes = L().cine_llr_prox_ws_bytes(b, t, h, w, block, shift[0], shift[1]) if rec or info else 0
    nblk = len(LLR.blocks(h, w, block, *shift)) * b
    assert not (rec or info) or nbytes == (1 + nblk) * 64
    ws = k.ws(nbytes)
    check(L().cine_llr_prox(ptr(xi), ptr(gi), ptr(si), ptr(ti), block, shift[0], shift[1], xo.ptr() if xo else None, ro.ptr() if ro else None,
                            io.ptr() if io else None, b, t, h, w, ws.ptr() if ws else None, nbytes, stream()), "cine_llr_prox")
    return ([xo.t] if xo else []) + ([ro.t] if ro else []) + ([io.t] if io else [])


def reference(x, g, step, thresh, block, shift):
    """The yardstick on the float32 v the kernel forms -> (xnew, rec, sigma_max, blocks): float64 SVD per block."""
    x64 = R.to_complex(x)
    if g is None:
        v = x64
    else:
        v = R.to_complex(R.to_pairs(x64 - float(np.float32(step)) * R.to_complex(g)).astype(np.float32))
    theta = float(np.float32(thresh)) if step is None else float(np.float32(step) * np.float32(thresh))
    xnew, nuc, smax = LLR.block_svt(v, theta, block, *shift)
    rec = np.array([(np.abs(xnew - x64) ** 2).sum(), (np.abs(xnew) ** 2).sum(), nuc])
    return xnew, rec, smax, len(LLR.blocks(x.shape[2], x.shape[3], block, *shift)) * x.shape[0]


def peak_err(got, want):
    peak = np.abs(want).max()
    return float(np.abs(R.to_complex(got) - want).max() / peak) if peak > 0 else float(np.abs(R.to_complex(got)).max())


def judge(what, outs, want):
    """outs = (xnew, rec, info) on the CPU against want = reference(...): asserts the bars of the docstring."""
    xnew, rec, info = outs
    want_x, want_rec, want_smax, want_blocks = want
    info = f64(info)
    ex = peak_err(xnew, want_x)
    floor = want_x.size * (BAR * np.abs(want_x).max()) ** 2                        # DIFF_FLOOR of the docstring, for the first sum only
    er = [abs(float(rec[q]) - want_rec[q]) / want_rec[q] if want_rec[q] > 0 else abs(float(rec[q])) for q in range(3)]
    if abs(float(rec[0]) - want_rec[0]) <= floor:
        print(f"{what}: sum |xnew - x|^2 = {float(rec[0]):.2e} against {want_rec[0]:.2e}, within N (BAR peak)^2 = {floor:.2e}")
        er[0] = min(er[0], SUM_REL)
    es = abs(info[0] - want_smax) / want_smax if want_smax > 0 else abs(info[0])
    print(f"{what}: xnew {ex:.2e} of the float64 peak (bar {BAR:.0e}); sums {er[0]:.2e} {er[1]:.2e} {er[2]:.2e} relative (bar {SUM_REL:.0e}); "
          f"sigma_max {es:.1e} relative (bar 1e-10), residual {info[1]:.1e}, {int(info[2])} sweeps, {int(info[3])} blocks")
    assert ex <= BAR, what
    assert max(er) <= SUM_REL and float(rec[3]) == 0.0, (what, er)
    assert es <= 1e-10 and info[1] <= 1e-14 and 0 <= info[2] < MAX_SWEEPS and info[2] == int(info[2]) and info[3] == want_blocks, (what, info)


def check_prox(dev, shape, block, shift, seed, frac=0.3):
    b, t, h, w = shape
    x, g = rnd(seed, b, t, h, w, 2), rnd(seed + 1, b, t, h, w, 2)
    v = R.to_complex(x) - float(np.float32(STEP)) * R.to_complex(g)
    thresh = float(np.float32(frac * LLR.block_svt(v, 0.0, block, *shift)[2] / STEP))
    what = f"cine_llr_prox {shape} block {block} shift {shift}"
    outs = twice(dev, OFF, lambda k: prox_call(k, x, g, shape, block, shift, thresh), what)
    judge(what, outs, reference(x, g, STEP, thresh, block, shift))
    k = Call(dev, OFF)
    xi, ri, ii = prox_call(k, x, g, shape, block, shift, thresh, inplace=True)
    k.finish(what + " in place")
    assert same_bits(xi.cpu(), outs[0]) and same_bits(ri.cpu(), outs[1]) and same_bits(ii.cpu(), outs[2]), what + ": in place gives other bits"
    k = Call(dev, 0)
    (xn,) = prox_call(k, x, g, shape, block, shift, thresh, rec=False, info=False)
    k.finish(what + " without records")
    assert same_bits(xn.cpu(), outs[0]), what + ": other bits without the records (and at another storage offset)"


@pytest.mark.parametrize("place", PLACES, ids=lambda p: f"{p[0]}x{p[1]}s{p[2][0]}{p[2][1]}")
@pytest.mark.parametrize("t", FRAMES, ids=lambda t: f"t{t}")
def test_block_8_vs_float64(dev, t, place):
    h, w, shift = place
    check_prox(dev, (1, t, h, w), 8, shift, seed=3000 * t + 37 * h + w + shift[0])


@pytest.mark.parametrize("block", [2, 3, 4, 16], ids=lambda v: f"block{v}")
@pytest.mark.parametrize("t", [5, 15], ids=lambda t: f"t{t}")
def test_other_blocks_vs_float64(dev, t, block):
    check_prox(dev, (1, t, 2 * block + 3, block + 1), block, (block - 1, 1), seed=500 * t + block)


def test_the_largest_lds_layout_vs_float64(dev):
    check_prox(dev, (1, 64, 35, 19), 16, (0, 0), seed=64)


def test_batch_two_vs_float64(dev):
    check_prox(dev, (2, 5, 9, 17), 8, (7, 1), seed=77)


def special_image(seed=11):
    """(1, 15, 19, 13), block 8, no shift: block (0, 0) all zero, block (1, 0) of rank 1 (one frame repeated), the others random."""
    x = rnd(seed, 1, 15, 19, 13, 2)
    x[:, :, 0:8, 0:8] = 0.0
    x[:, :, 8:16, 0:8] = x[:, 0:1, 8:16, 0:8].clone()
    return x


def test_special_inputs(dev):
    shape, block, shift = (1, 15, 19, 13), 8, (0, 0)
    x = special_image()
    x64 = R.to_complex(x)
    smax = LLR.block_sigma_max(x64, block)
    rank1 = np.linalg.svd(x64[0, :, 8:16, 0:8].reshape(15, -1), compute_uv=False)
    assert rank1[1] <= 1e-12 * rank1[0]
    # g = NULL and no step: v = x, theta = thresh.  Threshold 0: xnew = v; a mid threshold; above every sigma_max: exactly 0
    for name, thresh in (("0", 0.0), ("mid", float(np.float32(0.3 * smax))), ("above", float(np.float32(1.001 * smax)))):
        what = f"cine_llr_prox special blocks, g = NULL, threshold {name}"
        outs = twice(dev, OFF, lambda k: prox_call(k, x, None, shape, block, shift, thresh, step=None), what)
        want = reference(x, None, None, thresh, block, shift)
        judge(what, outs, want)
        got = R.to_complex(outs[0])
        assert not got[0, :, 0:8, 0:8].any(), what + ": the zero block is not exactly zero"
        if name == "0":
            assert np.abs(got - x64).max() <= BAR * np.abs(x64).max(), what + ": xnew is not v"
        if name == "above":
            assert not outs[0].any() and float(outs[1][1]) == 0.0 and float(outs[1][2]) == 0.0, what + ": xnew is not exactly 0"
        if name == "mid":                                       # the rank-1 block keeps its one singular value, lowered by the threshold
            blk = np.linalg.svd(got[0, :, 8:16, 0:8].reshape(15, -1), compute_uv=False)
            assert abs(blk[0] - (rank1[0] - thresh)) <= 1e-5 * rank1[0] and blk[1] <= 1e-5 * rank1[0]
    # g = NULL with a step: theta = step * thresh
    thresh = float(np.float32(0.3 * smax / STEP))
    what = "cine_llr_prox special blocks, g = NULL with a step"
    outs = twice(dev, OFF, lambda k: prox_call(k, x, None, shape, block, shift, thresh), what)
    judge(what, outs, reference(x, None, STEP, thresh, block, shift))
    # xnew = NULL: nothing but rec and info is written, and they hold the bits of the call with an image
    k = Call(dev, OFF)
    ro, io = prox_call(k, x, None, shape, block, shift, thresh, image=False)
    k.finish(what + ", xnew = NULL")
    assert same_bits(ro.cpu(), outs[1]) and same_bits(io.cpu(), outs[2])
    k = Call(dev, OFF)
    (io2,) = prox_call(k, x, None, shape, block, shift, thresh, image=False, rec=False)
    k.finish(what + ", info alone")
    assert same_bits(io2.cpu(), outs[2])


def test_the_binding_gives_the_bits_of_the_c_call(dev):
    from cine_hip import classical, ops
    shape, block, shift = (2, 15, 9, 17), 8, (7, 1)
    b, t, h, w = shape
    x, g = rnd(5, b, t, h, w, 2), rnd(6, b, t, h, w, 2)
    thresh = 0.7
    want = twice(dev, 0, lambda k: prox_call(k, x, g, shape, block, shift, thresh), "cine_llr_prox")
    xd, gd = x.to(dev), g.to(dev)
    st, th = torch.tensor([STEP], device=dev), torch.tensor([thresh], device=dev)
    xn, rec, info = ops.llr_prox(xd, gd, st, th, block, shift, record=True)
    assert xn.shape == xd.shape and same_bits(xn.cpu(), want[0]) and same_bits(rec.cpu(), want[1])
    assert info.dtype == torch.float64 and np.array_equal(info.cpu().numpy(), f64(want[2]))
    assert same_bits(ops.llr_prox(xd.unsqueeze(2), gd.unsqueeze(2), st, th, block, shift).squeeze(2).cpu(), want[0])      # (b, t, 1, h, w, 2)
    x2 = xd.clone()
    out = ops.llr_prox(x2, gd, st, th, block, shift, xnew=x2)                                  # in place through the binding
    assert out.data_ptr() == x2.data_ptr() and same_bits(x2.cpu(), want[0])
    rec2, info2 = ops.llr_prox(xd, gd, st, th, block, shift, image=False)
    assert same_bits(rec2.cpu(), want[1]) and torch.equal(info2, info)
    # block_sigma_max: info[0] of the unshifted partition with no threshold, one device float
    got = classical.block_sigma_max(xd, block)
    ref = LLR.block_sigma_max(R.to_complex(x), block)
    assert got.shape == (1,) and got.dtype == torch.float32 and abs(float(got) - ref) <= 1e-6 * ref
    with pytest.raises(ValueError, match="shift"):
        ops.llr_prox(xd, gd, st, th, block, (8, 0))
    with pytest.raises(ValueError, match="block"):
        ops.llr_prox(xd, gd, st, th, 17)


def test_refusals_come_before_anything_is_written(dev):
    shape, block = (1, 5, 9, 17), 8
    b, t, h, w = shape
    x, g = rnd(3, b, t, h, w, 2), rnd(4, b, t, h, w, 2)
    k = Call(dev, OFF)
    xi, gi, si, ti = k.inp(x), k.inp(g), k.raw(torch.tensor([STEP])), k.raw(torch.tensor([0.5]))
    xo, ro, io = k.out((b, t, h, w, 2)), k.out((4,)), k.out((8,))
    need = L().cine_llr_prox_ws_bytes(b, t, h, w, block, 7, 1)
    ws = k.ws(need)
    base = dict(x=ptr(xi), g=ptr(gi), step=ptr(si), thresh=ptr(ti), block=block, sh=7, sw=1, xnew=xo.ptr(), rec=ro.ptr(), info=io.ptr(),
                b=b, t=t, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_llr_prox(a["x"], a["g"], a["step"], a["thresh"], a["block"], a["sh"], a["sw"], a["xnew"], a["rec"], a["info"],
                                         a["b"], a["t"], a["h"], a["w"], a["ws"], a["nbytes"], stream())
    for kw, want in ((dict(t=1), EUNSUPPORTED), (dict(t=65), EUNSUPPORTED), (dict(block=1, sh=0, sw=0), EUNSUPPORTED),
                     (dict(block=17), EUNSUPPORTED), (dict(b=65536), EUNSUPPORTED), (dict(sh=-1), EINVAL), (dict(sh=8), EINVAL),
                     (dict(sw=8), EINVAL), (dict(x=None), EINVAL), (dict(thresh=None), EINVAL), (dict(step=None), EINVAL), (dict(ws=None), EINVAL),
                     (dict(b=0), EINVAL), (dict(t=0), EINVAL), (dict(h=0), EINVAL), (dict(w=0), EINVAL), (dict(ws=base["ws"] + 8), EINVAL),
                     (dict(info=base["info"] + 4), EINVAL), (dict(xnew=base["g"]), EINVAL), (dict(rec=base["xnew"]), EINVAL),
                     (dict(info=base["rec"]), EINVAL), (dict(ws=base["x"]), EINVAL), (dict(nbytes=need - 1), EWORKSPACE)):
        refused(call(**kw), want, k, f"cine_llr_prox {kw}")
    check(call()(), "cine_llr_prox")
    k.finish("cine_llr_prox")
    assert bool(torch.isfinite(xo.t).all()) and bool(torch.isfinite(ro.t).all()) and bool(torch.isfinite(io.t.view(torch.float64)).all())
