"""cine_image_dc_general, cine_normal_op_general and cine_apply_mask2d -- the image-space data consistency and the masking step for sampling
masks that vary along w -- through the C ABI, shape by shape against float64.

Reference: the composition the header names, sens_reduce(DC(sens_expand(img))) with the mask applied point by point in k-space, in float64
on the CPU with oracle.centered_fft.  Bar: kernel_sweep.BAR (1e-5 of the reference's peak).  Every call runs on guarded operands at two
storage offsets, twice (the same bits), with a workspace of exactly the size asked for in front of a sentinel.

Shapes, the smallest that reach each code path: h = 200 (the one-kernel column pass, 16 columns per workgroup: w below, at and above 16 and
a ragged third workgroup), w = 200 (the 200-point row engine) with a mixed-radix and a direct column length, mixed-radix and direct lengths on
either axis including the largest of each (512, 397) and 480 along w; 1 - 17 coils (17 exceeds the lines of a workgroup on both engines).
Counter 15 of cine_diag_counter proves the mask-plane column pass ran: one count per column chunk."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from kernel_sweep import (BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L as _L, Worst, at_offsets as _at_offsets, case_id, check as _check,
                          hash_case, ptr as _p, refused as _refused, same_bits, stream as _stream, sweep)
from oracle import centered_fft as cf

gpu = pytest.mark.gpu
WORST = Worst()
_record = WORST.record
BOTH = (0, 2)
D_MASK2D = 15

SHAPES = [(200, 1), (200, 15), (200, 16), (200, 17), (200, 33),          # h = 200 fast path
          (7, 200), (24, 200),                                          # w = 200 row engine
          (24, 20), (96, 10), (512, 3), (12, 480),                      # mixed radix
          (17, 9), (7, 13), (397, 2)]                                   # direct DFT
MASKS = ["random40", "ones", "zeros", "checker_w", "per_frame", "centre_point", "origin_point", "cols_equal"]
WEIGHTS = ["soft-3", "soft0", "soft4", "w100", "w10m1", "w_odd"]
LAMS = {"soft-3": -3.0, "soft0": float(np.log(np.e - 1.0)), "soft4": 4.0}
FIXED = {"w100": (1.0, 0.0, 0.0), "w10m1": (1.0, 0.0, -1.0), "w_odd": (0.25, 2.0, 0.5)}


def _cases():
    cs = sweep(20241, {"hw": SHAPES, "c": [1, 3, 8, 17], "bt": [(1, 1), (2, 3)], "mask": MASKS, "weights": WEIGHTS,
                       "zf": [True, False], "magnitude": [0, 1]}, 2 * len(SHAPES))
    for c in cs:
        c["h"], c["w"] = c.pop("hw")
        c["b"], c["t"] = c.pop("bt")
        if c["weights"] == "w10m1":
            c["zf"] = True                       # XPDNet's backward image: the - zf term is the point
    return cs


CASES = _cases()


def make_mask(seed, b, t, h, w, kind):
    """uint8 (b, t, h, w)."""
    rs = np.random.RandomState(seed)
    m = np.zeros((b, t, h, w), np.uint8)
    if kind == "random40":
        m[:] = rs.rand(1, 1, h, w) < 0.4
        m[:, :, max(h // 2 - 2, 0):h // 2 + 2, max(w // 2 - 2, 0):w // 2 + 2] = 1
    elif kind == "ones":
        m[:] = 1
    elif kind == "checker_w":
        m[..., ::2] = 1
    elif kind == "per_frame":
        m[:] = rs.rand(b, t, h, w) < rs.uniform(0.2, 0.8, (b, t, 1, 1))
    elif kind == "centre_point":
        m[:, :, h // 2, w // 2] = 1
    elif kind == "origin_point":
        m[:, :, 0, 0] = 1
    elif kind == "cols_equal":
        m[:] = (rs.rand(b, t, h, 1) < 0.4)
    else:
        assert kind == "zeros"
    return torch.from_numpy(m)


def _rand(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def softplus64(lam):
    return float(torch.log1p(torch.exp(torch.tensor(float(np.float32(lam)), dtype=torch.float64))))


def ref_weighted(img, S, mask, w1, w0):
    """sum_c conj(S_c) IFFT2[(mask ? w1 : w0) FFT2(S_c img)] in float64: img (b, t, h, w, 2), S (b, c, h, w, 2), mask (b, t, h, w)."""
    x = torch.view_as_complex(img.double().contiguous())
    s = torch.view_as_complex(S.double().contiguous())
    k = cf.fft2c(torch.view_as_real(s[:, None] * x[:, :, None]))                     # (b, t, c, h, w, 2)
    wgt = torch.where(mask.bool()[:, :, None, :, :, None], torch.tensor(w1, dtype=torch.float64), torch.tensor(w0, dtype=torch.float64))
    y = torch.view_as_complex(cf.ifft2c(k * wgt).contiguous())
    return torch.view_as_real((s.conj()[:, None] * y).sum(2))


def ref_general(img, S, mask, zf, weights):
    if weights in LAMS:
        v = softplus64(LAMS[weights])
        w1, w0, beta = 1.0 / (1.0 + v), 1.0, v / (1.0 + v)
    else:
        w1, w0, beta = (float(np.float32(x)) for x in FIXED[weights])
    out = ref_weighted(img, S, mask, w1, w0)
    return out if zf is None else out + beta * zf.double()


def data(c, seed):
    b, t, C, h, w = c["b"], c["t"], c["c"], c["h"], c["w"]
    img, S = _rand(seed, b, t, h, w, 2), _rand(seed + 1, b, C, h, w, 2)
    zf = _rand(seed + 2, b, t, h, w, 2) if c["zf"] else None
    return img, S, zf, make_mask(seed + 3, b, t, h, w, c["mask"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def chunks(b, t, c):
    """Column-pass launches of one call: the images go in chunks of whole frames, at most 32 768 images each."""
    step = 32768 // c * c
    return -(-b * t * c // step)


def run_general(dev, c, img, S, zf, mask, offs=BOTH):
    L = _L()
    b, t, C, h, w, mag = c["b"], c["t"], c["c"], c["h"], c["w"], c["magnitude"]
    lam = LAMS.get(c["weights"])
    wts = FIXED.get(c["weights"], (7.0, 7.0, 7.0))            # ignored with lambda_dev
    nb = L.cine_image_dc_general_ws_bytes(b, t, C, h, w)
    assert nb == b * t * C * h * w * 8

    def body(kk):
        imgd, Sd, zfd, md, lamd = kk.inp(img), kk.inp(S), kk.inp(zf), kk.raw(mask), kk.lam(lam)
        o, ws = kk.out((b, t, h, w) if mag else (b, t, h, w, 2)), kk.ws(nb)
        _check(L.cine_image_dc_general(imgd.data_ptr(), Sd.data_ptr(), _p(zfd), md.data_ptr(), _p(lamd), *wts, o.ptr(), b, t, C, h, w, mag,
                                       ws.ptr(), nb, _stream()), "cine_image_dc_general")
        return [o.t]
    L.cine_diag_counter(D_MASK2D, 1)
    got, = _at_offsets(dev, offs, body, "cine_image_dc_general")
    assert L.cine_diag_counter(D_MASK2D, 1) == 2 * len(offs) * chunks(b, t, C)
    return got


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_image_dc_general_sweep(dev, c):
    L = _L()
    img, S, zf, mask = data(c, hash_case(c))
    ref = ref_general(img, S, mask, zf, c["weights"])
    want = torch.view_as_complex(ref.contiguous()).abs() if c["magnitude"] else ref
    got = run_general(dev, c, img, S, zf, mask)
    path = "200" if c["h"] == 200 else "generic"
    _record(f"cine_image_dc_general ({path})", rel_err(got, want), BAR, c)
    if c["mask"] == "cols_equal":
        # the same pattern as a row mask through cine_image_dc: both within BAR of the one reference
        b, t, C, h, w, mag = c["b"], c["t"], c["c"], c["h"], c["w"], c["magnitude"]
        lam = LAMS.get(c["weights"])
        wts = FIXED.get(c["weights"], (7.0, 7.0, 7.0))
        nb = L.cine_image_dc_ws_bytes(b, t, C, h, w)
        kk = Call(dev, 0)
        imgd, Sd, zfd, md, lamd = kk.inp(img), kk.inp(S), kk.inp(zf), kk.raw(mask[..., 0].contiguous()), kk.lam(lam)
        o, ws = kk.out((b, t, h, w) if mag else (b, t, h, w, 2)), kk.ws(nb)
        _check(L.cine_image_dc(imgd.data_ptr(), Sd.data_ptr(), _p(zfd), md.data_ptr(), _p(lamd), *wts, o.ptr(), b, t, C, h, w, mag,
                               ws.ptr() if ws else None, nb, _stream()), "cine_image_dc")
        kk.finish("cine_image_dc")
        _record(f"cine_image_dc on the row mask ({path})", rel_err(o.t.cpu(), want), BAR, c)


def test_the_cases_reach_every_path():
    assert {(c["h"], c["w"]) for c in CASES} == set(SHAPES)
    for axis, vals in (("c", [1, 3, 8, 17]), ("mask", MASKS), ("weights", WEIGHTS), ("zf", [True, False]), ("magnitude", [0, 1])):
        assert {c[axis] for c in CASES} == set(vals), axis
    assert {(c["b"], c["t"]) for c in CASES} == {(1, 1), (2, 3)}


@gpu
@pytest.mark.parametrize("h,w", [(200, 17), (9, 7), (24, 20)])
@pytest.mark.parametrize("kind", ["centre_point", "origin_point"])
def test_single_point_masks_at_odd_and_even_lengths(dev, h, w, kind):
    """One sampled point: a shift that is off by one at an odd length moves it to a neighbour, and the result is a different plane wave."""
    c = dict(b=1, t=2, c=3, h=h, w=w, mask=kind, weights="w100", zf=False, magnitude=0)
    img, S, zf, mask = data(c, 77 + h + w)
    got = run_general(dev, c, img, S, zf, mask, offs=(0,))
    _record("cine_image_dc_general (single point)", rel_err(got, ref_general(img, S, mask, zf, "w100")), BAR, c)


@gpu
def test_image_dc_general_across_the_column_chunks(dev):
    """36 000 images of 4 x 2 in three frames: the column pass goes in two launches, the second from frame 2 on with that frame's mask."""
    c = dict(b=1, t=3, c=12000, h=4, w=2, mask="per_frame", weights="soft0", zf=True, magnitude=0)
    img, S, zf, _ = data(c, 5)
    mask = torch.zeros((1, 3, 4, 2), dtype=torch.uint8)
    mask[0, 0, :, 0] = 1
    mask[0, 1, 1::2] = 1
    mask[0, 2, 0, 1] = 1
    assert chunks(1, 3, 12000) == 2
    got = run_general(dev, c, img, S, zf, mask, offs=(0,))
    _record("cine_image_dc_general (chunks)", rel_err(got, ref_general(img, S, mask, zf, "soft0")), BAR, c)


@gpu
@pytest.mark.parametrize("b,t,C,h,w,lam", [(1, 2, 6, 200, 17, 0.3), (2, 3, 3, 24, 20, -3.0), (1, 1, 17, 7, 13, 4.0), (1, 2, 2, 12, 200, 0.0)])
def test_normal_op_general(dev, b, t, C, h, w, lam):
    """A^H M A x + softplus(lambda) x."""
    L = _L()
    c = dict(b=b, t=t, c=C, h=h, w=w, mask="random40", zf=False)
    img, S, _, mask = data(c, 31 + h)
    want = ref_weighted(img, S, mask, 1.0, 0.0) + softplus64(lam) * img.double()
    nb = L.cine_image_dc_general_ws_bytes(b, t, C, h, w)

    def body(kk):
        imgd, Sd, md, lamd = kk.inp(img), kk.inp(S), kk.raw(mask), kk.lam(lam)
        o, ws = kk.out((b, t, h, w, 2)), kk.ws(nb)
        _check(L.cine_normal_op_general(imgd.data_ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), b, t, C, h, w,
                                        ws.ptr(), nb, _stream()), "cine_normal_op_general")
        return [o.t]
    L.cine_diag_counter(D_MASK2D, 1)
    got, = _at_offsets(dev, BOTH, body, "cine_normal_op_general")
    assert L.cine_diag_counter(D_MASK2D, 1) == 4
    _record("cine_normal_op_general", rel_err(got, want), BAR, c)


@gpu
@pytest.mark.parametrize("bt,C,h,w", [(1, 1, 1, 1), (3, 2, 7, 5), (2, 17, 200, 33), (6, 3, 24, 20)])
def test_apply_mask2d_is_the_torch_expression_bit_for_bit(dev, bt, C, h, w):
    L = _L()
    k = _rand(bt + h, bt, C, h, w, 2)
    k.view(-1)[::3] = -0.0
    k.view(-1)[1::7] *= -1.0
    mask = torch.from_numpy((np.random.RandomState(h).rand(bt, 1, h, w, 1) < 0.5).astype(np.uint8))
    want = k * mask + 0.0
    assert bool((want.view(torch.int32) != (k * mask).view(torch.int32)).any())          # the + 0.0 matters: there are -0.0 products

    def body(alias):
        def run(kk):
            if alias:
                o = kk.out(k.shape, fill=k)
                src = o.t
            else:
                src, o = kk.inp(k), kk.out(k.shape)
            md = kk.raw(mask)
            _check(L.cine_apply_mask2d(src.data_ptr(), md.data_ptr(), o.ptr(), bt, C, h, w, _stream()), "cine_apply_mask2d")
            return [o.t]
        return run
    for alias in (False, True):
        got, = _at_offsets(dev, BOTH, body(alias), "cine_apply_mask2d")
        assert same_bits(got, want), (alias, bt, C, h, w)


@gpu
def test_refusals_write_nothing(dev):
    L = _L()
    b, t, C, h, w = 1, 2, 3, 8, 6
    c = dict(b=b, t=t, c=C, h=h, w=w, mask="random40", zf=True)
    img, S, zf, mask = data(c, 3)
    nb = L.cine_image_dc_general_ws_bytes(b, t, C, h, w)

    def operands(hh=h, ww=w, nbytes=nb):
        kk = Call(dev, 0)
        imgd = kk.inp(_rand(1, b, t, hh, ww, 2)) if (hh, ww) != (h, w) else kk.inp(img)
        Sd = kk.inp(_rand(2, b, C, hh, ww, 2)) if (hh, ww) != (h, w) else kk.inp(S)
        zfd = kk.inp(_rand(3, b, t, hh, ww, 2)) if (hh, ww) != (h, w) else kk.inp(zf)
        md = kk.raw(torch.ones((b, t, hh, ww), dtype=torch.uint8)) if (hh, ww) != (h, w) else kk.raw(mask)
        return kk, imgd, Sd, zfd, md, kk.lam(0.5), kk.out((b, t, hh, ww, 2)), kk.ws(nbytes)

    def dc(i, s, z, m, lam, o, ws, nbytes, hh=h, ww=w):
        return lambda: L.cine_image_dc_general(i, s, z, m, lam, 1.0, 0.0, 0.0, o, b, t, C, hh, ww, 0, ws, nbytes, _stream())

    def nop(i, s, m, lam, o, ws, nbytes):
        return lambda: L.cine_normal_op_general(i, s, m, lam, o, b, t, C, h, w, ws, nbytes, _stream())

    for drop in ("img", "sens", "mask", "out", "ws"):
        kk, imgd, Sd, zfd, md, lamd, o, ws = operands()
        a = dict(img=imgd.data_ptr(), sens=Sd.data_ptr(), mask=md.data_ptr(), out=o.ptr(), ws=ws.ptr())
        a[drop] = None
        _refused(dc(a["img"], a["sens"], zfd.data_ptr(), a["mask"], lamd.data_ptr(), a["out"], a["ws"], nb), EINVAL, kk,
                 f"cine_image_dc_general without {drop}")
        _refused(nop(a["img"], a["sens"], a["mask"], lamd.data_ptr(), a["out"], a["ws"], nb), EINVAL, kk, f"cine_normal_op_general without {drop}")
    kk, imgd, Sd, zfd, md, lamd, o, ws = operands()
    _refused(nop(imgd.data_ptr(), Sd.data_ptr(), md.data_ptr(), None, o.ptr(), ws.ptr(), nb), EINVAL, kk, "cine_normal_op_general without lambda")
    # out aliasing img
    kk = Call(dev, 0)
    Sd, md, lamd, io, ws = kk.inp(S), kk.raw(mask), kk.lam(0.5), kk.out((b, t, h, w, 2), fill=img), kk.ws(nb)
    _refused(dc(io.ptr(), Sd.data_ptr(), None, md.data_ptr(), lamd.data_ptr(), io.ptr(), ws.ptr(), nb), EINVAL, kk, "cine_image_dc_general in place")
    _refused(nop(io.ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), io.ptr(), ws.ptr(), nb), EINVAL, kk, "cine_normal_op_general in place")
    # workspace one byte short
    kk, imgd, Sd, zfd, md, lamd, o, ws = operands(nbytes=nb - 1)
    _refused(dc(imgd.data_ptr(), Sd.data_ptr(), zfd.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), ws.ptr(), nb - 1), EWORKSPACE, kk,
             "cine_image_dc_general with a short workspace")
    _refused(nop(imgd.data_ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), ws.ptr(), nb - 1), EWORKSPACE, kk,
             "cine_normal_op_general with a short workspace")
    assert bool((ws.buf[:ws.nbytes] == 0xFF).all()), "the workspace was written before the refusal"
    # a length no engine takes, on either axis
    for hh, ww in ((401, 2), (2, 401)):
        n2 = L.cine_image_dc_general_ws_bytes(b, t, C, hh, ww)
        kk, imgd, Sd, zfd, md, lamd, o, ws = operands(hh, ww, n2)
        _refused(dc(imgd.data_ptr(), Sd.data_ptr(), zfd.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), ws.ptr(), n2, hh, ww), EUNSUPPORTED, kk,
                 f"cine_image_dc_general at {hh} x {ww}")
        assert bool((ws.buf[:ws.nbytes] == 0xFF).all())
    # b * t above the grid limit
    kk, imgd, Sd, zfd, md, lamd, o, ws = operands()
    _refused(lambda: L.cine_image_dc_general(imgd.data_ptr(), Sd.data_ptr(), None, md.data_ptr(), None, 1.0, 0.0, 0.0, o.ptr(), 256, 256, 1, 1, 1, 0,
                                             ws.ptr(), 1 << 40, _stream()), EUNSUPPORTED, kk, "cine_image_dc_general with b * t = 65536")
    # cine_apply_mask2d
    kk = Call(dev, 0)
    kd, md, o = kk.inp(_rand(4, 2, 3, 4, 5, 2)), kk.raw(torch.ones((2, 4, 5), dtype=torch.uint8)), kk.out((2, 3, 4, 5, 2))
    for a in ((None, md.data_ptr(), o.ptr()), (kd.data_ptr(), None, o.ptr()), (kd.data_ptr(), md.data_ptr(), None)):
        _refused(lambda: L.cine_apply_mask2d(*a, 2, 3, 4, 5, _stream()), EINVAL, kk, "cine_apply_mask2d with a null pointer")
    _refused(lambda: L.cine_apply_mask2d(kd.data_ptr(), md.data_ptr(), o.ptr(), 2, 3, 0, 5, _stream()), EINVAL, kk, "cine_apply_mask2d with h = 0")
    assert L.cine_diag_counter(99, 0) == -1
