"""cine_ssim_loss / cine_ssim_loss_bwd, cine_image_metrics and the small helpers of ew_kernels.hip through the C ABI, shape by shape.

The SSIM kernels are compared with the centred float64 yardstick of tests/ssim_reference.py (test_loss_metric_cpu.py measures the yardstick's
own uncertainty: below 1e-12 of every quantity) on uniform noise AND on image-like inputs: a piecewise-constant phantom whose reconstruction
lies within sigma = 1e-2, 1e-3 or 1e-4 of its target, and one with a frame a thousand times darker than the others.  Noise alone cannot
show a loss of precision: each of its windows has a variance far above C2 = (0.03 L)^2, so nothing in S or in its derivatives cancels.

Bars.  Loss: 2e-6 absolute (a float32 scalar of order 1).  Gradient: BAR = 1e-5 on the relative L2 error and on max |error| / max |reference|,
the second so that a local error on a plateau cannot hide in the norm.  cine_image_metrics computes in float64 and differs from the yardstick
in the order of its sums only: SSIM (mean and every frame) and PSNR 1e-8 absolute, NMSE and MSE 1e-12 relative.  The helpers use the unfused
IEEE operations of the reference's tensor expressions: bit for bit the same expression in float32 torch on the CPU, and within BAR of float64.

Shapes.  The loss kernels work in tiles of 16 x 16 windows and end in a 64-lane reduction over the tiles: Ho = h - win + 1 and Wo take 1
(h == win), 15, 16, 17 and 33, one case has 17 x 4 tiles.  The metric kernel works in tiles of 32 x 32: the valid extent takes 1, 31, 32, 33.

Every case: an exact-size workspace prefilled with 0xFF, guards intact, inputs unchanged, two calls with the same bits, and the same bits with
every float pointer at a storage offset of 0, 1 and 3 floats (0 and 2 floats for complex operands, which ask for 8-byte alignment)."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_reference as R
from conftest import rel_err
from kernel_sweep import (BAR, EINVAL, EWORKSPACE, Call, GuardedF64, L, Workspace, Worst, at_offsets, case_id, check, hash_case, ptr, refused,
                          same_bits, stream, sweep)

pytestmark = pytest.mark.gpu
WORST = Worst()
_record = WORST.record
OFFS = (0, 1, 3)                               # storage offsets in floats of plain float arrays
OFFS_C = (0, 2)                                # and of complex operands
K1, K2 = 0.01, 0.03
LOSS_ABS, SSIM_ABS, PSNR_ABS, SUM_REL = 2e-6, 1e-8, 1e-8, 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def make_pair(kind, t, h, w, seed):
    """(target, reconstruction) of one of the input kinds."""
    if kind == "noise":
        return R.noise_pair(t, h, w, seed)
    if kind == "dark":
        return R.phantom_pair(t, h, w, 1e-3, dark_frame=t - 1, seed=seed)
    return R.phantom_pair(t, h, w, {"ph2": 1e-2, "ph3": 1e-3, "ph4": 1e-4}[kind], seed=seed)


# ================================================================== cine_ssim_loss + cine_ssim_loss_bwd
LOSS_AXES = dict(win=[3, 4, 7, 11], ho=[1, 15, 16, 17, 33], wo=[1, 15, 16, 17, 33], t=[1, 2, 5], inp=["noise", "ph2", "ph3", "ph4", "dark"],
                 gl=[1.0, 3.0, -0.5])
LOSS_CASES = sweep(11, LOSS_AXES, 20) + [
    dict(win=7, ho=264, wo=54, t=1, inp="ph4", gl=1.0),          # 270 x 60: 17 x 4 = 68 tiles, the lane-strided final reduction wraps
    dict(win=7, ho=34, wo=30, t=1, inp="ph4", gl=1.0),           # 40 x 36, sigma 1e-4: where a float32 rounding of the saved derivatives shows most
    dict(win=7, ho=34, wo=30, t=2, inp="ph3", gl=3.0),
    dict(win=7, ho=34, wo=30, t=2, inp="noise", gl=1.0),
    dict(win=11, ho=1, wo=1, t=1, inp="ph4", gl=-0.5),           # one window, the largest one
]


def loss_body(dev, tgt, rec, win, gl):
    t, h, w = rec.shape

    def body(k):
        x, y = k.inp(rec), k.inp(tgt)
        loss, gx, gx_moved = k.out((1,)), k.out((t, h, w)), k.out((t, h, w))
        need = L().cine_ssim_loss_ws_bytes(t, h, w, win)
        assert need > 0
        ws = k.ws(need)
        check(L().cine_ssim_loss(ptr(x), ptr(y), t, h, w, win, K1, K2, loss.ptr(), ws.ptr(), need, stream()), "cine_ssim_loss")
        kept = ws.buf[:need].clone()
        g = k.raw(torch.tensor([gl], dtype=torch.float32))
        check(L().cine_ssim_loss_bwd(ptr(x), ptr(y), t, h, w, win, ptr(g), ws.ptr(), need, gx.ptr(), stream()), "cine_ssim_loss_bwd")
        assert torch.equal(ws.buf[:need], kept), "cine_ssim_loss_bwd wrote into the workspace it only reads"
        moved = Workspace(need, dev, past256=8)                                   # the same bytes at another address, another alignment
        moved.buf[:need] = kept
        k.wss.append(moved)
        check(L().cine_ssim_loss_bwd(ptr(x), ptr(y), t, h, w, win, ptr(g), moved.ptr(), need, gx_moved.ptr(), stream()), "cine_ssim_loss_bwd")
        return [loss.t, gx.t, gx_moved.t]
    return body


@pytest.mark.parametrize("c", LOSS_CASES, ids=case_id)
def test_ssim_loss_and_gradient_vs_float64(dev, c):
    win, t, h, w = c["win"], c["t"], c["ho"] + c["win"] - 1, c["wo"] + c["win"] - 1
    tgt, rec = make_pair(c["inp"], t, h, w, hash_case(c))
    want_loss, want_g = R.ssim_loss_grad(rec, tgt, win, K1, K2, c["gl"])
    loss, gx, gx_moved = at_offsets(dev, OFFS, loss_body(dev, tgt, rec, win, c["gl"]), "cine_ssim_loss")
    assert same_bits(gx, gx_moved), "cine_ssim_loss_bwd depends on where the workspace lies, not only on its bytes"
    d = gx.double() - want_g
    e_loss, e_l2, e_max = abs(float(loss) - want_loss), float(d.norm() / want_g.norm()), float(d.abs().max() / want_g.abs().max())
    print(f"{case_id(c)}: loss {want_loss:.3e}, error {e_loss:.2e} (bar {LOSS_ABS:.0e}); gradient relative L2 {e_l2:.2e}, max {e_max:.2e} (bar {BAR:.0e})")
    _record("cine_ssim_loss", e_loss, LOSS_ABS, case_id(c))
    _record("cine_ssim_loss_bwd (L2)", e_l2, BAR, case_id(c))
    _record("cine_ssim_loss_bwd (max)", e_max, BAR, case_id(c))


def test_ssim_loss_refusals_come_before_anything_is_written(dev):
    t, h, w, win = 2, 20, 18, 7
    tgt, rec = R.phantom_pair(t, h, w, 1e-3)
    k = Call(dev, 0)
    x, y, g = k.inp(rec), k.inp(tgt), k.raw(torch.tensor([1.0]))
    loss, gx = k.out((1,)), k.out((t, h, w))
    need = L().cine_ssim_loss_ws_bytes(t, h, w, win)
    ws = k.ws(need)
    base = dict(x=ptr(x), y=ptr(y), g=ptr(g), loss=loss.ptr(), gx=gx.ptr(), ws=ws.ptr(), t=t, h=h, w=w, win=win, nbytes=need)

    def fwd(**kw):
        a = {**base, **kw}
        return lambda: L().cine_ssim_loss(a["x"], a["y"], a["t"], a["h"], a["w"], a["win"], K1, K2, a["loss"], a["ws"], a["nbytes"], stream())

    def bwd(**kw):
        a = {**base, **kw}
        return lambda: L().cine_ssim_loss_bwd(a["x"], a["y"], a["t"], a["h"], a["w"], a["win"], a["g"], a["ws"], a["nbytes"], a["gx"], stream())
    for name, call, nulls in (("cine_ssim_loss", fwd, ("x", "y", "loss", "ws")), ("cine_ssim_loss_bwd", bwd, ("x", "y", "g", "ws", "gx"))):
        for n in nulls:
            refused(call(**{n: None}), EINVAL, k, f"{name} {n} = NULL")
        for bad in (dict(win=1), dict(win=1, h=1, w=1), dict(win=0), dict(win=12), dict(t=0), dict(h=6), dict(w=6)):
            refused(call(**bad), EINVAL, k, f"{name} {bad}")
        refused(call(nbytes=need - 1), EWORKSPACE, k, f"{name} a workspace one byte short")
    refused(fwd(t=65536), EINVAL, k, "cine_ssim_loss t = 65536")
    assert torch.equal(ws.buf[:need], torch.full_like(ws.buf[:need], 0xFF)), "a refused call wrote into the workspace"
    assert L().cine_ssim_loss_ws_bytes(t, h, w, 1) == 0 and L().cine_ssim_loss_ws_bytes(t, h, w, 12) == 0


def test_the_wrappers_refuse_a_window_of_one_pixel(dev):
    from cine_hip import ops
    from reconstruction.utils import SSIMLoss
    tgt, rec = (v.to(dev) for v in R.phantom_pair(2, 12, 12, 1e-3))
    with pytest.raises(ValueError):
        ops.image_metrics(tgt, rec, win_size=1)
    module = SSIMLoss().to(dev)
    module.win_size = 1                                                          # (SSIMLoss(win_size=1) itself divides by zero, as the reference's does)
    with pytest.raises(ValueError):
        module(rec[None, None], tgt[None, None])


# ================================================================== cine_image_metrics
def metric_sizes(vy, vx, win, crop):
    """(hg, wg, hp, wp) with a common crop of (vy + win - 1, vx + win - 1); the size differences are odd: // 2 floors."""
    ch, cw = vy + win - 1, vx + win - 1
    return {"gt": (ch + 3, cw + 5, ch, cw), "pred": (ch, cw, ch + 5, cw + 3), "mixed": (ch + 3, cw, ch, cw + 5)}[crop]


def embed(img, hh, ww, rs, bright=None):
    """img (t, ch, cw) in the centre of (t, hh, ww) -- from = (size - crop) // 2 -- with noise below the image's peak around it.  bright: that value
    is put into a corner of frame 0, outside the crop."""
    t, ch, cw = img.shape
    out = torch.from_numpy(rs.uniform(0, 0.9, size=(t, hh, ww)).astype(np.float32))
    fy, fx = (hh - ch) // 2, (ww - cw) // 2
    out[:, fy:fy + ch, fx:fx + cw] = img
    if bright is not None:
        assert fy > 0 or fx > 0, "the corner lies inside the crop"
        out[0, 0, 0] = bright
    return out


METRIC_AXES = dict(vy=[1, 31, 32, 33], vx=[1, 31, 32, 33], win=[3, 7, 11], t=[1, 4], mode=[0, 1, 2], crop=["gt", "pred", "mixed"],
                   inp=["noise", "ph3", "ph4", "dark"], bright=[False])
METRIC_CASES = sweep(12, METRIC_AXES, 16) + [
    # the maximum of frame 0 of gt lies outside the crop: the data range and the peak of the PSNR come from the cropped region
    dict(vy=31, vx=33, win=7, t=4, mode=0, crop="gt", inp="ph3", bright=True),
    dict(vy=33, vx=32, win=3, t=4, mode=1, crop="mixed", inp="noise", bright=True),
    dict(vy=32, vx=1, win=11, t=1, mode=0, crop="mixed", inp="ph4", bright=True),
    dict(vy=33, vx=33, win=7, t=4, mode=2, crop="gt", inp="ph2", bright=True),
]
MAXVAL = 2.5                                   # mode 2: not the data's maximum (1 on the phantom, 1.5 on noise)


@pytest.mark.parametrize("c", METRIC_CASES, ids=case_id)
def test_image_metrics_vs_float64(dev, c):
    win, t, mode = c["win"], c["t"], c["mode"]
    hg, wg, hp, wp = metric_sizes(c["vy"], c["vx"], win, c["crop"])
    ch, cw = min(hg, hp), min(wg, wp)
    rs = np.random.RandomState(hash_case(c))
    tgt, rec = make_pair(c["inp"], t, ch, cw, hash_case(c))
    gt, pred = embed(tgt, hg, wg, rs, 3.0 if c["bright"] else None), embed(rec, hp, wp, rs)
    if c["bright"]:
        assert float(gt.max()) == 3.0 > float(tgt.max())
    want = R.image_metrics(gt.numpy(), pred.numpy(), win, K1, K2, mode, MAXVAL)

    def body(k):
        g, p = k.inp(gt), k.inp(pred)
        out = GuardedF64(4 + t, dev)
        k.outs.append(out)
        need = L().cine_image_metrics_ws_bytes(t, hg, wg, hp, wp, win)
        assert need > 0
        ws = k.ws(need)
        check(L().cine_image_metrics(ptr(g), ptr(p), t, hg, wg, hp, wp, win, K1, K2, mode, MAXVAL if mode == 2 else 0.0, out.ptr(), ws.ptr(), need,
                                     stream()), "cine_image_metrics")
        return [out.t]
    got, = at_offsets(dev, OFFS, body, "cine_image_metrics")
    got = got.numpy()
    errs = dict(ssim=abs(got[0] - want["ssim"]), frames=float(np.abs(got[4:] - want["ssim_frames"]).max()), psnr=abs(got[2] - want["psnr"]),
                nmse=abs(got[1] - want["nmse"]) / want["nmse"], mse=abs(got[3] - want["mse"]) / want["mse"])
    print(f"{case_id(c)}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    _record("cine_image_metrics ssim", errs["ssim"], SSIM_ABS, case_id(c))
    _record("cine_image_metrics frames", errs["frames"], SSIM_ABS, case_id(c))
    _record("cine_image_metrics psnr", errs["psnr"], PSNR_ABS, case_id(c))
    _record("cine_image_metrics nmse", errs["nmse"], SUM_REL, case_id(c))
    _record("cine_image_metrics mse", errs["mse"], SUM_REL, case_id(c))


def test_image_metrics_refusals_come_before_anything_is_written(dev):
    t, hg, wg, hp, wp, win = 2, 20, 18, 22, 17, 7
    rs = np.random.RandomState(3)
    tgt, rec = R.phantom_pair(t, 20, 17, 1e-3)
    k = Call(dev, 0)
    g, p = k.inp(embed(tgt, hg, wg, rs)), k.inp(embed(rec, hp, wp, rs))
    out = GuardedF64(4 + t, dev)
    k.outs.append(out)
    need = L().cine_image_metrics_ws_bytes(t, hg, wg, hp, wp, win)
    ws = k.ws(need)
    base = dict(gt=ptr(g), pred=ptr(p), out=out.ptr(), ws=ws.ptr(), t=t, hg=hg, wg=wg, hp=hp, wp=wp, win=win, mode=0, nbytes=need)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L().cine_image_metrics(a["gt"], a["pred"], a["t"], a["hg"], a["wg"], a["hp"], a["wp"], a["win"], K1, K2, a["mode"], 0.0,
                                              a["out"], a["ws"], a["nbytes"], stream())
    for n in ("gt", "pred", "out", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_image_metrics {n} = NULL")
    for bad in (dict(win=1), dict(win=1, hg=1, wg=1, hp=1, wp=1), dict(win=0), dict(win=4), dict(win=10), dict(win=13), dict(mode=-1), dict(mode=3),
                dict(t=0), dict(t=65536), dict(hg=6), dict(wp=6), dict(hp=0)):
        refused(call(**bad), EINVAL, k, f"cine_image_metrics {bad}")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_image_metrics a workspace one byte short")
    assert torch.equal(ws.buf[:need], torch.full_like(ws.buf[:need], 0xFF)), "a refused call wrote into the workspace"


# ================================================================== the helpers of ew_kernels.hip
def cplx(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape + (2,)).astype(np.float32))


def strides_of(shape, full):
    """Strides in complex elements of a contiguous tensor of `shape` seen as `full`: 0 where it broadcasts."""
    st, acc = [0] * len(shape), 1
    for d in reversed(range(len(shape))):
        st[d] = 0 if shape[d] == 1 and full[d] != 1 else acc
        acc *= shape[d]
    return st


def mul32(a, b):
    """complex_mul (utils/math.py) in the tensors' own precision, one unfused operation after the other."""
    return torch.stack((a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]), dim=-1)


MUL_CASES = [  # (out shape, x shape, y shape)
    ((), (), ()), ((5,), (5,), (5,)), ((3, 4), (1, 4), (3, 4)), ((2, 3, 5), (2, 3, 5), (2, 1, 5)), ((2, 3, 4, 5), (2, 1, 4, 1), (1, 3, 1, 5)),
    ((2, 3, 2, 3, 7), (2, 3, 2, 3, 7), (1, 1, 1, 1, 7)), ((2, 3, 2, 3, 2, 3), (2, 1, 2, 1, 2, 3), (2, 3, 1, 3, 1, 3)),
    ((3, 1, 5, 2, 1, 7), (3, 1, 5, 1, 1, 7), (1, 1, 5, 2, 1, 7)), ((4, 300), (1, 1), (4, 300)), ((3, 257), (3, 257), (3, 257)),
    ((2, 3, 4), (1, 3, 1), (1, 1, 4)),                         # the first dimension broadcasts on both operands
]


def run_complex_mul(dev, offs, full, xs, ys, x, y, what="cine_complex_mul"):
    nd = len(full)
    shape = (ctypes.c_int * max(nd, 1))(*full)
    xst, yst = (ctypes.c_long * max(nd, 1))(*strides_of(xs, full)), (ctypes.c_long * max(nd, 1))(*strides_of(ys, full))

    def body(k):
        a, b = k.inp(x), k.inp(y)
        o = k.out(tuple(full) + (2,))
        check(L().cine_complex_mul(ptr(a), ptr(b), o.ptr(), nd, shape, xst, yst, stream()), what)
        return [o.t]
    return at_offsets(dev, offs, body, what)[0]


@pytest.mark.parametrize("full,xs,ys", MUL_CASES, ids=lambda s: "x".join(map(str, s)) or "scalar")
def test_complex_mul_broadcasts_bit_for_bit(dev, full, xs, ys):
    x, y = cplx(1, *xs), cplx(2, *ys)
    got = run_complex_mul(dev, OFFS_C, full, xs, ys, x, y)
    assert same_bits(got, mul32(x, y).expand(tuple(full) + (2,)).contiguous()), "cine_complex_mul: not the bits of the float32 expression"
    _record("cine_complex_mul", rel_err(got, mul32(x.double(), y.double()).expand(tuple(full) + (2,))), BAR, str(full))


def test_complex_mul_beyond_one_grid_and_its_refusals(dev):
    """More than 16384 x 256 elements: the grid-stride loop goes round; y broadcasts along the first dimension."""
    full, xs, ys = (3, 1_400_003), (3, 1_400_003), (1, 1_400_003)
    assert full[0] * full[1] > 16384 * 256
    x, y = cplx(3, *xs), cplx(4, *ys)
    got = run_complex_mul(dev, (2,), full, xs, ys, x, y)
    assert same_bits(got, mul32(x, y))
    _record("cine_complex_mul", rel_err(got, mul32(x.double(), y.double())), BAR, str(full))
    k = Call(dev, 0)
    a, b, o = k.inp(cplx(5, 2, 3)), k.inp(cplx(6, 2, 3)), k.out((2, 3, 2))
    ones7, st7 = (ctypes.c_int * 7)(2, 3, 1, 1, 1, 1, 1), (ctypes.c_long * 7)(3, 1, 0, 0, 0, 0, 0)
    shape, st, empty = (ctypes.c_int * 2)(2, 3), (ctypes.c_long * 2)(3, 1), (ctypes.c_int * 2)(2, 0)
    refused(lambda: L().cine_complex_mul(ptr(a), ptr(b), o.ptr(), 7, ones7, st7, st7, stream()), EINVAL, k, "cine_complex_mul ndim = 7")
    refused(lambda: L().cine_complex_mul(ptr(a), ptr(b), o.ptr(), -1, shape, st, st, stream()), EINVAL, k, "cine_complex_mul ndim = -1")
    refused(lambda: L().cine_complex_mul(ptr(a), ptr(b), o.ptr(), 2, empty, st, st, stream()), EINVAL, k, "cine_complex_mul an empty dimension")
    for i in range(6):
        args = [ptr(a), ptr(b), o.ptr(), shape, st, st]
        args[i] = None
        refused(lambda: L().cine_complex_mul(args[0], args[1], args[2], 2, args[3], args[4], args[5], stream()), EINVAL, k, f"cine_complex_mul argument {i} NULL")


@pytest.mark.parametrize("n", [1, 255, 256, 1001])
def test_complex_conj_and_abs_sq_bit_for_bit(dev, n):
    x = cplx(n, n)
    x[0, 1] = 0.0                                                                # conj gives -0 here

    def body(k):
        a = k.inp(x)
        c, s = k.out((n, 2)), k.out((n,))
        check(L().cine_complex_conj(ptr(a), c.ptr(), n, stream()), "cine_complex_conj")
        check(L().cine_complex_abs_sq(ptr(a), s.ptr(), n, stream()), "cine_complex_abs_sq")
        return [c.t, s.t]
    c, s = at_offsets(dev, OFFS_C, body, "cine_complex_conj")
    assert same_bits(c, torch.stack((x[..., 0], -x[..., 1]), dim=-1)) and same_bits(s, x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1])
    _record("cine_complex_abs_sq", rel_err(s, (x.double() ** 2).sum(-1)), BAR, f"n{n}")
    k = Call(dev, 0)
    a, o = k.inp(x), k.out((n, 2))
    for name in ("cine_complex_conj", "cine_complex_abs_sq"):
        f = getattr(L(), name)
        refused(lambda: f(None, o.ptr(), n, stream()), EINVAL, k, f"{name} x = NULL")
        refused(lambda: f(ptr(a), None, n, stream()), EINVAL, k, f"{name} out = NULL")
        refused(lambda: f(ptr(a), o.ptr(), 0, stream()), EINVAL, k, f"{name} n = 0")


@pytest.mark.parametrize("inner", [1, 7, 200])
@pytest.mark.parametrize("kk", [1, 2, 15])
@pytest.mark.parametrize("is_complex", [0, 1], ids=["real", "complex"])
def test_rss_bit_for_bit(dev, is_complex, kk, inner):
    outer = 3
    x = cplx(kk * 1000 + inner, outer, kk, inner) if is_complex else cplx(kk * 1000 + inner, outer, kk, inner)[..., 0].contiguous()

    def ref(v):
        s = torch.zeros(outer, inner, dtype=v.dtype)
        for j in range(kk):                                                      # k ascending, one rounding per operation
            s = s + ((v[:, j, :, 0] * v[:, j, :, 0] + v[:, j, :, 1] * v[:, j, :, 1]) if is_complex else v[:, j] * v[:, j])
        # the correctly rounded root, as the kernel's sqrtf is: the float64 root of a float32 rounds to it (53 >= 2 * 24 + 2 bits), while torch's
        # vectorised float32 sqrt on the CPU is an ulp off on about 0.7 % of its arguments
        return s.double().sqrt().to(v.dtype)

    def body(k):
        a = k.inp(x)
        o = k.out((outer, inner))
        check(L().cine_rss(ptr(a), o.ptr(), outer, kk, inner, is_complex, stream()), "cine_rss")
        return [o.t]
    got, = at_offsets(dev, OFFS_C if is_complex else OFFS, body, "cine_rss")
    assert same_bits(got, ref(x)), "cine_rss: not the bits of the float32 expression"
    _record("cine_rss", rel_err(got, ref(x.double())), BAR, f"complex{is_complex}-k{kk}-inner{inner}")


@pytest.mark.parametrize("inner", [1, 2, 5])
@pytest.mark.parametrize("n", [7, 8])
def test_roll_every_shift(dev, n, inner):
    outer = 3
    x = cplx(n * 10 + inner, outer, n, inner)[..., 0].contiguous()
    for shift in (0, 1, n // 2, (n + 1) // 2, -1, n, n + 3, -(2 * n + 1)):
        def body(k):
            a = k.inp(x)
            o = k.out((outer, n, inner))
            check(L().cine_roll(ptr(a), o.ptr(), outer, n, inner, shift, stream()), "cine_roll")
            return [o.t]
        got, = at_offsets(dev, OFFS, body, "cine_roll")
        assert same_bits(got, torch.roll(x, shift, dims=1)), f"cine_roll: shift {shift} of {n}"
    k = Call(dev, 0)
    a, o = k.inp(x), k.out((outer, n, inner))
    refused(lambda: L().cine_roll(ptr(a), ptr(a), outer, n, inner, 1, stream()), EINVAL, k, "cine_roll in place")
    refused(lambda: L().cine_roll(None, o.ptr(), outer, n, inner, 1, stream()), EINVAL, k, "cine_roll x = NULL")
    refused(lambda: L().cine_roll(ptr(a), None, outer, n, inner, 1, stream()), EINVAL, k, "cine_roll out = NULL")
    refused(lambda: L().cine_roll(ptr(a), o.ptr(), outer, 0, inner, 1, stream()), EINVAL, k, "cine_roll n = 0")


@pytest.mark.parametrize("top,left,bottom,right", [(0, 0, 0, 0), (2, 3, 0, 0), (0, 0, 3, 1), (1, 2, 2, 5)], ids=["none", "top-left", "bottom-right", "all"])
def test_pad2d_pads_with_plus_zero(dev, top, left, bottom, right):
    planes, h, w = 3, 9, 13
    hp, wp = h + top + bottom, w + left + right
    x = cplx(top * 7 + right, planes, h, w)[..., 0].contiguous()
    x[0, 0, 0] = -0.0
    want = torch.zeros(planes, hp, wp)
    want[:, top:top + h, left:left + w] = x

    def body(k):
        a = k.inp(x)
        o = k.out((planes, hp, wp))
        check(L().cine_pad2d(ptr(a), o.ptr(), planes, h, w, top, left, hp, wp, stream()), "cine_pad2d")
        return [o.t]
    got, = at_offsets(dev, OFFS, body, "cine_pad2d")
    assert same_bits(got, want), "cine_pad2d: the frame is not +0 or the image moved"
    k = Call(dev, 0)
    a, o = k.inp(x), k.out((planes, hp, wp))
    refused(lambda: L().cine_pad2d(ptr(a), o.ptr(), planes, h, w, top + 1, left, h + top, wp + 1, stream()), EINVAL, k, "cine_pad2d an output smaller than h + top")
    refused(lambda: L().cine_pad2d(ptr(a), o.ptr(), planes, h, w, top, left + 1, hp, w + left, stream()), EINVAL, k, "cine_pad2d an output smaller than w + left")
    refused(lambda: L().cine_pad2d(ptr(a), o.ptr(), planes, h, w, -1, left, hp, wp, stream()), EINVAL, k, "cine_pad2d top = -1")
    refused(lambda: L().cine_pad2d(None, o.ptr(), planes, h, w, top, left, hp, wp, stream()), EINVAL, k, "cine_pad2d x = NULL")
    refused(lambda: L().cine_pad2d(ptr(a), None, planes, h, w, top, left, hp, wp, stream()), EINVAL, k, "cine_pad2d out = NULL")
