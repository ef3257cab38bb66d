"""cine_image_dc_general_sens_grad -- the maps' gradient of the image-space data consistency for sampling masks that vary along w -- followed by
cine_coil_accum(NULL, part), through the C ABI, shape by shape against float64.

Reference: float64 autograd on the CPU of the composition the header names, out = sum_c conj(S_c) IFFT2[(mask ? w1 : w0) FFT2(S_c img)]
(ref_weighted of test_general_mask_kernels.py, restated here with one copy of the maps per frame, so that autograd returns the per-frame
`part`), under d loss = Re(conj(g) d out).  Both `part` and the frame sum are held to kernel_sweep.BAR (1e-5 of the reference's peak).
Every call runs on guarded operands at two storage offsets, twice (the same bits), with a workspace of exactly the size asked for in front
of a sentinel.

Shapes, the smallest that reach each path: h = 200 (the one-kernel column pass, 16 columns per workgroup) below and above 16 columns,
w = 200 (the 200-point row engine and its per-coil epilogue), a mixed-radix pair and two direct-DFT pairs; 1, 3 and 17 coils (17 exceeds the
lines of a workgroup on both engines: the seeded cases bring it to the generic row engine, a pinned case to the 200-point one).  Counter 15 of
cine_diag_counter proves the mask-plane column pass ran: one count per operand and column chunk."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from kernel_sweep import (BAR, EUNSUPPORTED, Call, L as _L, Worst, at_offsets as _at_offsets, case_id, check as _check, hash_case, ptr as _p,
                          refused as _refused, stream as _stream, sweep)
from oracle import centered_fft as cf

gpu = pytest.mark.gpu
WORST = Worst()
_record = WORST.record
BOTH = (0, 2)
D_MASK2D = 15
ME = "cine_image_dc_general_sens_grad"

SHAPES = [(200, 15), (200, 17),          # h = 200 fast column kernel below and above 16 columns
          (24, 200),                     # 200-point row engine
          (24, 20),                      # mixed radix
          (17, 9), (7, 13)]              # direct DFT
COILS = [1, 3, 17]
MASKS = ["random40", "per_frame", "cols_equal", "zeros", "ones"]
WEIGHTS = ["soft0", "soft4", "w10m1", "w_odd"]
LAMS = {"soft0": float(np.log(np.e - 1.0)), "soft4": 4.0}
FIXED = {"w10m1": (1.0, 0.0), "w_odd": (0.25, 2.0)}


def _cases():
    cs = sweep(20251, {"hw": SHAPES, "c": COILS, "bt": [(1, 1), (2, 3)], "mask": MASKS, "weights": WEIGHTS}, 2 * len(SHAPES))
    # pinned beside the seeded ones: 17 coils on the 200-point row engine, two coil chunks (16 + 1) through its per-coil epilogue, which writes
    # and then accumulates at the chunk's own coil offset
    cs.append({"hw": (24, 200), "c": 17, "bt": (2, 3), "mask": "per_frame", "weights": "soft0"})
    for c in cs:
        c["h"], c["w"] = c.pop("hw")
        c["b"], c["t"] = c.pop("bt")
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
    elif kind == "per_frame":
        m[:] = rs.rand(b, t, h, w) < rs.uniform(0.2, 0.8, (b, t, 1, 1))
    elif kind == "cols_equal":
        m[:] = (rs.rand(b, t, h, 1) < 0.4)
    else:
        assert kind == "zeros"
    return torch.from_numpy(m)


def _rand(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def softplus64(lam):
    return float(torch.log1p(torch.exp(torch.tensor(float(np.float32(lam)), dtype=torch.float64))))


def weights64(name):
    if name in LAMS:
        return 1.0 / (1.0 + softplus64(LAMS[name])), 1.0
    return tuple(float(np.float32(x)) for x in FIXED[name])


def ref_weighted(img, S_bt, mask, w1, w0):
    """sum_c conj(S_c) IFFT2[(mask ? w1 : w0) FFT2(S_c img)] in float64: img (b, t, h, w, 2), S_bt (b, t, c, h, w, 2) -- the maps, one copy
    per frame --, mask (b, t, h, w)."""
    x = torch.view_as_complex(img.double().contiguous())
    s = torch.view_as_complex(S_bt)
    k = cf.fft2c(torch.view_as_real(s * x[:, :, None]))                              # (b, t, c, h, w, 2)
    wgt = torch.where(mask.bool()[:, :, None, :, :, None], torch.tensor(w1, dtype=torch.float64), torch.tensor(w0, dtype=torch.float64))
    y = torch.view_as_complex(cf.ifft2c(k * wgt).contiguous())
    return torch.view_as_real((s.conj() * y).sum(2))


def ref_part(img, g, S, mask, w1, w0):
    """d [sum Re(conj(g) out)] / d S per frame, (b, t, c, h, w, 2), by float64 autograd."""
    t = img.shape[1]
    S_bt = S.double()[:, None].expand(-1, t, -1, -1, -1, -1).contiguous().requires_grad_(True)
    with torch.enable_grad():
        out = ref_weighted(img, S_bt, mask, w1, w0)
        part, = torch.autograd.grad((out * g.double()).sum(), S_bt)
    return part


def data(c, seed):
    b, t, C, h, w = c["b"], c["t"], c["c"], c["h"], c["w"]
    return _rand(seed, b, t, h, w, 2), _rand(seed + 1, b, t, h, w, 2), _rand(seed + 2, b, C, h, w, 2), make_mask(seed + 3, b, t, h, w, c["mask"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def chunks(b, t, c):
    """Column-pass launches per operand: the images go in chunks of whole frames, at most 32 768 images each."""
    step = 32768 // c * c
    return -(-b * t * c // step)


def run_grad(dev, c, img, g, S, mask, offs=BOTH):
    L = _L()
    b, t, C, h, w = c["b"], c["t"], c["c"], c["h"], c["w"]
    lam = LAMS.get(c["weights"])
    wts = FIXED.get(c["weights"], (7.0, 7.0))                 # ignored with lambda_dev
    nb = L.cine_image_dc_general_sens_grad_ws_bytes(b, t, C, h, w)
    assert nb == b * t * C * h * w * 8

    def body(kk):
        imgd, gd, Sd, md, lamd = kk.inp(img), kk.inp(g), kk.inp(S), kk.raw(mask), kk.lam(lam)
        part, gs, ws = kk.out((b, t, C, h, w, 2)), kk.out((b, C, h, w, 2)), kk.ws(nb)
        _check(L.cine_image_dc_general_sens_grad(imgd.data_ptr(), gd.data_ptr(), Sd.data_ptr(), md.data_ptr(), _p(lamd), *wts, part.ptr(),
                                                 b, t, C, h, w, ws.ptr(), nb, _stream()), ME)
        _check(L.cine_coil_accum(None, part.ptr(), gs.ptr(), b, t, C, h, w, 0, _stream()), "cine_coil_accum")
        return [part.t, gs.t]
    L.cine_diag_counter(D_MASK2D, 1)
    part, gs = _at_offsets(dev, offs, body, ME)
    assert L.cine_diag_counter(D_MASK2D, 1) == 2 * 2 * len(offs) * chunks(b, t, C)          # two operands per call, each call twice per offset
    return part, gs


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_general_sens_grad_sweep(dev, c):
    img, g, S, mask = data(c, hash_case(c))
    want = ref_part(img, g, S, mask, *weights64(c["weights"]))
    part, gs = run_grad(dev, c, img, g, S, mask)
    path = "200" if c["h"] == 200 else "generic"
    _record(f"{ME} ({path})", rel_err(part, want), BAR, c)
    _record(f"{ME} + cine_coil_accum ({path})", rel_err(gs, want.sum(1)), BAR, c)


def test_the_cases_reach_every_path():
    assert {(c["h"], c["w"]) for c in CASES} == set(SHAPES)
    for axis, vals in (("c", COILS), ("mask", MASKS), ("weights", WEIGHTS)):
        assert {c[axis] for c in CASES} == set(vals), axis
    assert {(c["b"], c["t"]) for c in CASES} == {(1, 1), (2, 3)}
    # more than one coil chunk on each row engine (16 lines per workgroup at w = 200, 8 at any other length)
    assert any(c["c"] == 17 and c["w"] == 200 for c in CASES) and any(c["c"] == 17 and c["w"] != 200 for c in CASES)
    assert any(c["c"] == 17 and c["w"] == 200 and (c["b"], c["t"]) == (2, 3) for c in CASES)


@gpu
def test_an_unsupported_length_is_refused_with_nothing_written(dev):
    L = _L()
    b, t, C, h, w = 1, 2, 3, 401, 2
    nb = L.cine_image_dc_general_sens_grad_ws_bytes(b, t, C, h, w)
    kk = Call(dev, 0)
    imgd, gd, Sd = kk.inp(_rand(1, b, t, h, w, 2)), kk.inp(_rand(2, b, t, h, w, 2)), kk.inp(_rand(3, b, C, h, w, 2))
    md, lamd, part, ws = kk.raw(torch.ones((b, t, h, w), dtype=torch.uint8)), kk.lam(0.5), kk.out((b, t, C, h, w, 2)), kk.ws(nb)
    L.cine_diag_counter(D_MASK2D, 1)
    _refused(lambda: L.cine_image_dc_general_sens_grad(imgd.data_ptr(), gd.data_ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), 1.0, 0.0,
                                                       part.ptr(), b, t, C, h, w, ws.ptr(), nb, _stream()), EUNSUPPORTED, kk, f"{ME} at h = 401")
    assert bool((ws.buf[:ws.nbytes] == 0xFF).all()), "the workspace was written before the refusal"
    assert L.cine_diag_counter(D_MASK2D, 1) == 0
