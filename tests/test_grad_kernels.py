"""The backward entry points of include/cine_hip.h called one by one, shape by shape, against float64 references on the CPU.

Entry points: cine_conv3x3_wgrad, cine_conv1x1_wgrad, cine_conv3x3_dgrad, cine_conv3x3_dgrad_gated, cine_conv1x1_dgrad,
cine_tconv2x2_dgrad, cine_in_lrelu_bwd and cine_relu_mask.  The seeded case lists walk the shapes where grad_kernels.hip changes
its code path: the weight gradient's row block (cout 16 / 32 / 64 / 128), its tile width (W 16 / 8 / 4 / 2), the vectorised
staging (W a multiple of the piece width, 16-byte aligned pointers), the lean plane kernel against the general one, the K split;
the four paths of the InstanceNorm + LeakyReLU backward; the float4 body and scalar tail of the ReLU mask.

Every case checks
  * the error: conftest.rel_err (max |d| / peak) against float64 at a bar of 1e-5.  Above ~1e5 summed terms the bar is twice the
    error of torch's own float32 CPU result against the same reference, 1e-5 at least and 1e-4 at most;
  * the header's semantics: weight and bias gradients ACCUMULATE into random prefills, input gradients OVERWRITE a NaN prefill;
  * that nothing is written outside the output (guard floats on both sides) or past the workspace size the library reports
    (a sentinel tail behind it);
  * determinism: a second identical call gives the same bits (fixed-order reductions, no atomics).
Subsets run again on views at storage offset 1 or 2 floats: pointers that are not 16-byte aligned, so the vectorised staging
must be skipped, and the result must meet the same bar.

The InstanceNorm backward is only comparable away from LeakyReLU's kink: its inputs come from kink_free_planes, which keeps every
normalised value at least KINK_MARGIN from zero in float64 (else float32 and float64 can fall on opposite sides of the kink and the
comparison measures rounding, not the kernel).  The reference helpers and that generator are checked on the CPU by the tests
without the gpu mark.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from kernel_sweep import BAR, BAR_CAP, LONG_REDUCTION, Guarded, Workspace, Worst, _bar, cap_samples, case_id, hash_case, sweep, view_at

KINK_MARGIN = 1e-3
EPS = 1e-5
D_WGRAD_PLANE, D_WGRAD_GENERAL = 0, 1          # cine_diag_counter (csrc/common.h: Diag)


# ================================================================== float64 references (CPU)
def ref_conv3x3_wgrad(x, g):
    """(gw, gb) of y = conv2d(x, W, b, padding=1): x (n, cin, h, w), g = d loss / d y (n, cout, h, w)."""
    x, g = x.double(), g.double()
    gw = torch.nn.grad.conv2d_weight(x, (g.shape[1], x.shape[1], 3, 3), g, padding=1)
    return gw, g.sum((0, 2, 3))


def ref_conv1x1_wgrad(x, g):
    """(gw (cout, cin), gb) of y = conv2d(x, W[..., None, None], b)."""
    x, g = x.double(), g.double()
    return torch.einsum("nihw,nohw->oi", x, g), g.sum((0, 2, 3))


def _per_set(n, set_split, w1, w2, fn):
    """fn(sample range, weights) over samples [0, set_split) with w1 and [set_split, n) with w2, concatenated."""
    parts = []
    if set_split > 0:
        parts.append(fn(slice(0, set_split), w1))
    if set_split < n:
        parts.append(fn(slice(set_split, n), w2))
    return torch.cat(parts)


def ref_conv3x3_dgrad(gy, w1, w2=None, set_split=None):
    """d loss / d x of y = conv2d(x, W, padding=1) from gy (n, cout, h, w); W (cout, cin, 3, 3); samples >= set_split use w2."""
    gy = gy.double()
    n, _, h, w = gy.shape
    set_split = n if set_split is None else set_split
    return _per_set(n, set_split, w1, w2, lambda s, W: torch.nn.grad.conv2d_input(
        (gy[s].shape[0], W.shape[1], h, w), W.double(), gy[s], padding=1))


def ref_conv1x1_dgrad(gy, w1, w2=None, set_split=None):
    """d loss / d x of y = conv2d(x, W[..., None, None]) from gy (n, cout, h, w); W (cout, cin)."""
    gy = gy.double()
    n = gy.shape[0]
    set_split = n if set_split is None else set_split
    return _per_set(n, set_split, w1, w2, lambda s, W: torch.einsum("nohw,oi->nihw", gy[s], W.double()))


def ref_tconv2x2_dgrad(gy, w1, w2=None, set_split=None):
    """d loss / d x of y = conv_transpose2d(x, W, stride=2) from gy (n, cout, 2h, 2w); W (cin, cout, 2, 2).  The adjoint of
    the k2 s2 transpose convolution is the k2 s2 convolution with the same weight."""
    gy = gy.double()
    n = gy.shape[0]
    set_split = n if set_split is None else set_split
    return _per_set(n, set_split, w1, w2, lambda s, W: F.conv2d(gy[s], W.double(), stride=2))


def ref_in_lrelu_bwd(x, g, slope, eps=EPS):
    """d loss / d x of y = LeakyReLU(InstanceNorm(x)) (no affine, biased variance) from g = d loss / d y, closed form:
    rstd (g' - mean(g') - xhat mean(g' xhat)) per (sample, channel) plane with g' = g LeakyReLU'(xhat)."""
    x, g = x.double(), g.double()
    dims = tuple(range(2, x.dim()))
    mean = x.mean(dims, keepdim=True)
    rstd = ((x - mean).pow(2).mean(dims, keepdim=True) + eps).rsqrt()
    xh = (x - mean) * rstd
    gp = torch.where(xh > 0, g, g * slope)
    return rstd * (gp - gp.mean(dims, keepdim=True) - xh * (gp * xh).mean(dims, keepdim=True))


def normalised(x, eps=EPS):
    """InstanceNorm(x) in float64 (biased variance), per (sample, channel) plane."""
    x = x.double()
    dims = tuple(range(2, x.dim()))
    mean = x.mean(dims, keepdim=True)
    return (x - mean) * ((x - mean).pow(2).mean(dims, keepdim=True) + eps).rsqrt()


def kink_margin(x, eps=EPS):
    """The smallest |InstanceNorm(x)| in float64 (how far the float32 tensor x stays from LeakyReLU's kink)."""
    return float(normalised(x, eps).abs().min())


def kink_free_planes(seed, shape, scale=1.7, shift=0.3, gap=0.05, margin=KINK_MARGIN, tries=64):
    """A float32 tensor of `shape` (n, c, ...) whose normalised values all lie at least `margin` from zero, checked in float64.
    Values are drawn standard normal and pushed `gap` away from zero before the affine map; when a draw still lands inside the
    margin (a plane's mean moves the zero), it is redrawn with the next seed -- deterministically."""
    for k in range(tries):
        z = np.random.RandomState(seed + 7919 * k).standard_normal(shape)
        z = np.sign(z) * (np.abs(z) + gap)
        x = torch.from_numpy((z * scale + shift).astype(np.float32))
        if kink_margin(x) >= margin:
            return x
    raise AssertionError(f"kink_free_planes: no draw of {shape} keeps {margin} from the kink in {tries} tries")


# ================================================================== case lists
WGRAD3_AXES = dict(cout=[1, 8, 16, 17, 32, 33, 64, 65, 128, 130], c0=[1, 2, 3, 16, 17, 20], c1=[0, 0, 3, 5, 7],
                   w=[1, 2, 3, 4, 5, 8, 9, 16, 17, 33], h=[1, 2, 7, 13, 26, 52, 208], n=list(range(1, 16)), gb=[False, True])
_WG3 = sweep(101, WGRAD3_AXES, 30)
for _c in _WG3:
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"], 8000)
_WG3 += [dict(cout=32, c0=16, c1=5, w=16, h=26, n=3, gb=True),          # plane kernel with the concatenated second source
         dict(cout=130, c0=20, c1=7, w=33, h=13, n=5, gb=True),         # every ragged edge at once: general kernel
         dict(cout=16, c0=2, c1=0, w=8, h=52, n=4, gb=False)]
WGRAD3_CASES = _WG3
WGRAD3_FULL = [dict(cout=16, c0=2, c1=0, w=16, h=208, n=400, gb=True),     # cfg 2, U-Net level 0: many K chunks, plane kernel
               dict(cout=16, c0=16, c1=0, w=16, h=208, n=400, gb=True),
               dict(cout=16, c0=2, c1=0, w=200, h=200, n=15, gb=True)]      # one 200 x 200 cine slice of 15 frames

WGRAD1_AXES = dict(WGRAD3_AXES, cin=[1, 2, 3, 16, 17, 20, 23])
del WGRAD1_AXES["c0"], WGRAD1_AXES["c1"]
_WG1 = sweep(202, WGRAD1_AXES, 20)
for _c in _WG1:
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"], 8000)
WGRAD1_CASES = _WG1 + [dict(cout=2, cin=16, w=24, h=7 * 24, n=2, gb=True)]   # a 3-D U-Net's final 1x1x1 conv: (d h, w) = (7 * 24, 24)

DGRAD_AXES = dict(cout=[1, 8, 16, 17, 32, 33, 64, 65, 128, 130], cin=[1, 2, 3, 16, 17, 20, 23], w=[1, 2, 3, 4, 5, 8, 9, 16, 17, 33],
           h=[1, 2, 7, 13, 26, 52, 208], n=list(range(2, 16)), split=["none", "mid", "n"])
DGRAD3_CASES = sweep(303, DGRAD_AXES, 20)
DGRAD1_CASES = sweep(404, DGRAD_AXES, 14)
TCONV_AXES = dict(cout=[1, 8, 16, 17, 32, 33, 64], cin=[1, 2, 3, 16, 17, 20, 32, 128], w=[1, 2, 3, 4, 5, 8, 9, 16, 17],
                  h=[1, 2, 7, 13, 26, 52, 104], n=list(range(2, 16)), split=["none", "mid", "n"])
TCONV_CASES = sweep(505, TCONV_AXES, 14)
for _c in DGRAD3_CASES + DGRAD1_CASES + TCONV_CASES:
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"], 8000)
    _c["n"] = max(_c["n"], 2) if _c["split"] == "mid" else _c["n"]
GATED_CASES = [dict(cout=c, cin=ci, w=w, h=h, n=n, addend=a, gate=g)
               for (c, ci, w, h, n), (a, g) in itertools.product(
                   [(5, 5, 7, 9, 4), (16, 16, 16, 26, 3), (33, 20, 17, 13, 2)], itertools.product((False, True), repeat=2))]

# (n, c, h, w, records, slope, path): records "one" = ops.instnorm_partials; "k" = that many contiguous chunk records per plane
# merged by the kernel; "conv" = the records of a real cine_conv3x3_in output (one per tile).  The path is what the dispatch of
# grad_kernels.hip: launch_in_lrelu_bwd_split / inbwd_fast.hip: launch_in_lrelu_bwd_fast takes for an ALIGNED call.
IN_BWD_CASES = [
    (3, 5, 13, 4, "one", 0.2, "fast-wave"),            # w % 4 == 0, plane <= 1024: fast kernel, one wave per plane
    (2, 3, 52, 64, "4", 0.2, "fast-block"),            # plane 3328 <= 4096: fast kernel, one workgroup per plane
    (2, 3, 52, 32, "conv", 0.0, "fast-block"),       # two tiles: two records per plane
    (4, 3, 7, 9, "one", 0.2, "small"),                 # w odd: general kernel, one wave per plane
    (5, 2, 1, 3, "one", 0.0, "small"),                 # (planes of 1 or 2 elements normalise to constants: no gradient to compare)
    (2, 3, 45, 33, "3", 0.2, "plane"),                 # 1485 elements, w odd: one workgroup per plane
    (1, 2, 80, 64, "conv", 0.2, "plane"),              # 5120 > 4096 elements: one workgroup per plane
    (1, 2, 200, 200, "5", 0.2, "split-vec"),           # 40 000 > 32 768 elements: chunked two-pass split, float4 pieces
    (2, 3, 211, 199, "one", 0.0, "split"),             # odd width: chunked split, scalar pieces, ragged last chunk
    (1, 2, 200, 200, "one", 0.2, "plane-nows"),        # the split shape without a workspace: one workgroup per plane
]
RELU_MASK_N = [1, 2, 3, 5, 1023, 4096, 4097, 70_001, 70_002]


# ================================================================== CPU checks of the references and the generator
def test_in_lrelu_reference_closed_form_vs_autograd():
    for seed, shape, slope in ((1, (2, 3, 7, 9), 0.2), (2, (1, 2, 16, 4), 0.0), (3, (2, 1, 3, 5, 4), 0.2)):
        x = kink_free_planes(seed, shape)
        g = torch.from_numpy(np.random.RandomState(seed + 50).standard_normal(shape))
        x64 = x.double().requires_grad_(True)
        with torch.enable_grad():
            F.leaky_relu(F.instance_norm(x64, eps=EPS), slope).backward(g)
        assert rel_err(ref_in_lrelu_bwd(x, g, slope), x64.grad) < 1e-12, shape


def test_conv_references_vs_autograd():
    rs = np.random.RandomState(9)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))                 # noqa: E731
    n, cin, cout, h, w = 4, 3, 5, 7, 6
    x, W, W2, b = t(n, cin, h, w), t(cout, cin, 3, 3), t(cout, cin, 3, 3), t(cout)
    gy = t(n, cout, h, w)
    for w2, split in ((None, None), (W2, 1), (W2, 0), (W2, n)):
        xr, Wr, W2r, br = (a.clone().requires_grad_(True) for a in (x, W, W2, b))
        s = n if split is None else split
        with torch.enable_grad():
            y = torch.cat([F.conv2d(xr[:s], Wr, br, padding=1), F.conv2d(xr[s:], Wr if w2 is None else W2r, br, padding=1)])
            y.backward(gy)
        assert rel_err(ref_conv3x3_dgrad(gy, W, w2, split), xr.grad) < 1e-12
        if w2 is None:
            gw, gb = ref_conv3x3_wgrad(x, gy)
            assert rel_err(gw, Wr.grad) < 1e-12 and rel_err(gb, br.grad) < 1e-12
    W1, W12 = t(cout, cin), t(cout, cin)
    xr, Wr = x.clone().requires_grad_(True), W1.clone().requires_grad_(True)
    with torch.enable_grad():
        F.conv2d(xr, Wr[:, :, None, None]).backward(gy)
    assert rel_err(ref_conv1x1_dgrad(gy, W1), xr.grad) < 1e-12
    assert rel_err(ref_conv1x1_wgrad(x, gy)[0], Wr.grad) < 1e-12
    two = ref_conv1x1_dgrad(gy, W1, W12, 3)
    assert rel_err(two[3:], ref_conv1x1_dgrad(gy[3:], W12)) < 1e-12 and rel_err(two[:3], ref_conv1x1_dgrad(gy[:3], W1)) < 1e-12
    Wt = t(cin, cout, 2, 2)
    xr = t(n, cin, h, w).requires_grad_(True)
    gt = t(n, cout, 2 * h, 2 * w)
    with torch.enable_grad():
        F.conv_transpose2d(xr, Wt, stride=2).backward(gt)
    assert rel_err(ref_tconv2x2_dgrad(gt, Wt), xr.grad) < 1e-12


def test_kink_free_generator_keeps_its_margin():
    for i, (n, c, h, w, _, _, _) in enumerate(IN_BWD_CASES):
        x = kink_free_planes(700 + i, (n, c, h, w))
        assert x.dtype == torch.float32 and kink_margin(x) >= KINK_MARGIN
        assert torch.equal(x, kink_free_planes(700 + i, (n, c, h, w)))         # deterministic
    # a draw that does land on the kink is redrawn, not accepted: a plane of three values can always be normalised to ~0 in its middle
    assert kink_margin(torch.tensor([[[0.0, 1.0, 2.0]]])) < KINK_MARGIN
    x = kink_free_planes(5, (64, 1, 3))
    assert kink_margin(x) >= KINK_MARGIN
    z = _near_constant_plane(3)
    assert kink_margin(z) >= KINK_MARGIN and float(z.double().var(unbiased=False)) < 1e-2 * EPS


def test_sweeps_cover_every_branch_value():
    """The seeded lists reach every value of every axis but the sample count (capped to keep the references fast), both wgrad
    kernels (also with a second source), every in_lrelu path and every residue of the ReLU mask's tail."""
    for cases, axes in ((WGRAD3_CASES, WGRAD3_AXES), (WGRAD1_CASES, WGRAD1_AXES), (DGRAD3_CASES, DGRAD_AXES),
                        (DGRAD1_CASES, DGRAD_AXES), (TCONV_CASES, TCONV_AXES)):
        for a, vals in axes.items():
            if a != "n":
                assert {c[a] for c in cases} >= set(vals), a
    assert {wgrad3_route(c, 0) for c in WGRAD3_CASES} == {"plane", "general"}
    assert any(wgrad3_route(c, 0) == "plane" and c["c1"] > 0 for c in WGRAD3_CASES)
    assert any(c["cout"] > 128 and c["w"] > 16 and c["c1"] > 0 for c in WGRAD3_CASES)
    assert {p for *_, p in IN_BWD_CASES} == {"fast-wave", "fast-block", "small", "plane", "split", "split-vec", "plane-nows"}
    assert {0.0, 0.2} <= {s for _, _, _, _, _, s, _ in IN_BWD_CASES} and {"one", "conv"} < {r for _, _, _, _, r, _, _ in IN_BWD_CASES}
    assert {n % 4 for n in RELU_MASK_N} == {0, 1, 2, 3}


def wgrad3_route(c, off):
    """Which 3x3 weight-gradient kernel grad_kernels.hip: launch_wg_cfg takes for a case of the stand-alone entry point: the lean
    plane kernel needs W equal to the tile width (2, 4, 8 or 16), 16-byte aligned input and gradient, and a 16-channel first source
    when there is a second one."""
    return "plane" if c["w"] in (2, 4, 8, 16) and off == 0 and (c["c1"] == 0 or c["c0"] % 16 == 0) else "general"


def _near_constant_plane(seed):
    """One (1, 1, 24, 20) plane whose variance is far below eps: 0.25 + 1e-4 z, z pushed 0.1 away from zero."""
    z = np.random.RandomState(seed).standard_normal((1, 1, 24, 20))
    z = np.sign(z) * (np.abs(z) + 0.1)
    return torch.from_numpy((0.25 + 1e-4 * z).astype(np.float32))


# ================================================================== GPU harness
gpu = pytest.mark.gpu
WORST = Worst()     # entry point -> (worst error / bar, case)
_record = WORST.record


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def _L():
    from cine_hip._lib import lib
    return lib()


def _check(code, what):
    from cine_hip._lib import check
    check(code, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


_view = view_at


# ================================================================== weight gradients
def _run_wgrad(taps, c, off, dev, seed):
    """One weight-gradient case on views at storage offset `off`; returns (gw, gb, route) after every per-case check."""
    L = _L()
    cin = c["c0"] + c.get("c1", 0) if taps == 9 else c["cin"]
    n, cout, h, w = c["n"], c["cout"], c["h"], c["w"]
    x = _rand(seed, n, cin, h, w)
    g = _rand(seed + 1, n, cout, h, w)
    gw_shape = (cout, cin, 3, 3) if taps == 9 else (cout, cin)
    pre_w, pre_b = _rand(seed + 2, *gw_shape), _rand(seed + 3, cout)
    if taps == 9:
        ref_w, ref_b = ref_conv3x3_wgrad(x, g)
        nb = L.cine_conv3x3_wgrad_ws_bytes(cout, cin, n)
    else:
        ref_w, ref_b = ref_conv1x1_wgrad(x, g)
        nb = L.cine_conv1x1_wgrad_ws_bytes(cout, cin, n)
    # prefill at the gradient's own scale: an addition that dropped it, or a reduction that assigned, is off by the whole prefill
    pre_w *= float(ref_w.abs().max()) + 1.0
    pre_b *= float(ref_b.abs().max()) + 1.0
    x0 = _view(x[:, :c["c0"]] if taps == 9 else x, off, dev)
    x1 = _view(x[:, c["c0"]:], off, dev) if taps == 9 and c["c1"] else None
    gd = _view(g, off, dev)
    outs = []
    for rep in range(2):
        gw = Guarded(gw_shape, off, dev, pre_w)
        gb = Guarded((cout,), off, dev, pre_b) if c["gb"] else None
        ws = Workspace(nb, dev)
        counts = [L.cine_diag_counter(k, 0) for k in (D_WGRAD_PLANE, D_WGRAD_GENERAL)]
        if taps == 9:
            _check(L.cine_conv3x3_wgrad(x0.data_ptr(), c["c0"], None if x1 is None else x1.data_ptr(), c["c1"], gd.data_ptr(), gw.ptr(),
                                        gb.ptr() if gb else None, n, cout, h, w, ws.ptr(), nb, _stream()), "cine_conv3x3_wgrad")
        else:
            _check(L.cine_conv1x1_wgrad(x0.data_ptr(), cin, gd.data_ptr(), gw.ptr(), gb.ptr() if gb else None, n, cout, h, w,
                                        ws.ptr(), nb, _stream()), "cine_conv1x1_wgrad")
        torch.cuda.synchronize()
        counts = [L.cine_diag_counter(k, 0) - v for k, v in zip((D_WGRAD_PLANE, D_WGRAD_GENERAL), counts)]
        route = {(1, 0): "plane", (0, 1): "general", (0, 0): None}.get(tuple(counts), counts)
        assert ws.intact(), f"workspace tail overwritten {c}"
        assert gw.intact() and (gb is None or gb.intact()), f"write outside gw / gb {c}"
        outs.append((gw.t.clone(), gb.t.clone() if gb else None, route))
    (gw1, gb1, route), (gw2, gb2, route2) = outs
    assert torch.equal(gw1, gw2) and (gb1 is None or torch.equal(gb1, gb2)), f"not deterministic {c}"
    assert route == route2
    k = n * h * w
    e32 = 0.0
    if k > LONG_REDUCTION:
        if taps == 9:
            e32 = rel_err(torch.nn.grad.conv2d_weight(x, (cout, cin, 3, 3), g, padding=1), ref_w)
        else:
            e32 = rel_err(torch.einsum("nihw,nohw->oi", x, g), ref_w)
    name = "cine_conv3x3_wgrad" if taps == 9 else "cine_conv1x1_wgrad"
    _record(name, rel_err(gw1.cpu().double() - pre_w.double(), ref_w), _bar(e32, k), (c, off))
    if gb1 is not None:
        _record(name + " (gb)", rel_err(gb1.cpu().double() - pre_b.double(), ref_b), _bar(0.0, k) if k <= LONG_REDUCTION else
                min(BAR_CAP, max(BAR, 2 * rel_err(g.sum((0, 2, 3)), ref_b))), (c, off))
    return gw1, gb1, route


@gpu
@pytest.mark.parametrize("c", WGRAD3_CASES, ids=case_id)
def test_conv3x3_wgrad_sweep(dev, c):
    """cine_conv3x3_wgrad at an aligned base; the kernel it took (cine_diag_counter) is the one the dispatch rule names, and a case
    the lean plane kernel takes gives the same bits through the general kernel (cine_set_conv_plane bit 4)."""
    from cine_hip import ops
    gw, gb, route = _run_wgrad(9, c, 0, dev, seed=hash_case(c))
    assert route == wgrad3_route(c, 0), (c, route)
    if route == "plane":
        try:
            ops.set_conv_plane(7 | 16)
            gw2, gb2, route2 = _run_wgrad(9, c, 0, dev, seed=hash_case(c))
        finally:
            ops.set_conv_plane(7)
        assert route2 == "general"
        assert torch.equal(gw, gw2) and (gb is None or torch.equal(gb, gb2)), c


@gpu
@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("c", WGRAD3_CASES[::3], ids=case_id)
def test_conv3x3_wgrad_unaligned(dev, c, off):
    """Inputs, output gradient and gw / gb as views at storage offset 1 or 2 floats: no vectorised staging, no plane kernel."""
    _, _, route = _run_wgrad(9, c, off, dev, seed=hash_case(c))
    assert route == "general", (c, route)


@gpu
@pytest.mark.parametrize("c", WGRAD3_FULL, ids=case_id)
def test_conv3x3_wgrad_full_size(dev, c):
    """Full-size layers: K = n h w > 1e5 summed terms, split into the most partial chunks the workspace takes."""
    _, _, route = _run_wgrad(9, c, 0, dev, seed=hash_case(c))
    assert route == wgrad3_route(c, 0)


@gpu
def test_conv3x3_wgrad_sweep_reaches_both_kernels(dev):
    """cine_diag_counter proof that the sweep's cases reach both the lean plane kernel and the general kernel."""
    L = _L()
    base = [L.cine_diag_counter(k, 0) for k in (D_WGRAD_PLANE, D_WGRAD_GENERAL)]
    for c in WGRAD3_CASES:
        cin = c["c0"] + c["c1"]
        x = torch.zeros(c["n"], cin, c["h"], c["w"], device=dev)
        g = torch.zeros(c["n"], c["cout"], c["h"], c["w"], device=dev)
        gw = torch.zeros(c["cout"], cin, 3, 3, device=dev)
        nb = L.cine_conv3x3_wgrad_ws_bytes(c["cout"], cin, c["n"])
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        x1 = x[:, c["c0"]:].contiguous() if c["c1"] else None
        x0 = x[:, :c["c0"]].contiguous()
        _check(L.cine_conv3x3_wgrad(x0.data_ptr(), c["c0"], None if x1 is None else x1.data_ptr(), c["c1"], g.data_ptr(), gw.data_ptr(),
                                    None, c["n"], c["cout"], c["h"], c["w"], ws.data_ptr(), nb, _stream()), "cine_conv3x3_wgrad")
    torch.cuda.synchronize()
    plane, general = (L.cine_diag_counter(k, 0) - b for k, b in zip((D_WGRAD_PLANE, D_WGRAD_GENERAL), base))
    print(f"\nwgrad sweep: {plane} launches on wgrad_plane_kernel, {general} on wgrad_mfma_kernel")
    assert plane == sum(wgrad3_route(c, 0) == "plane" for c in WGRAD3_CASES) and plane > 0
    assert general == len(WGRAD3_CASES) - plane and general > 0


@gpu
@pytest.mark.parametrize("c", WGRAD1_CASES, ids=case_id)
def test_conv1x1_wgrad_sweep(dev, c):
    _run_wgrad(1, c, 0, dev, seed=hash_case(c))


@gpu
@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("c", WGRAD1_CASES[::4], ids=case_id)
def test_conv1x1_wgrad_unaligned(dev, c, off):
    _run_wgrad(1, c, off, dev, seed=hash_case(c))


# ================================================================== input gradients
def _split_of(c):
    return {"none": None, "mid": max(1, c["n"] // 2), "n": c["n"]}[c["split"]]


def _run_dgrad(kind, c, off, dev, seed):
    from cine_hip import ops
    L = _L()
    n, cout, cin, h, w = c["n"], c["cout"], c["cin"], c["h"], c["w"]
    if kind == "c3":
        wshape, gshape, pack, fn, ref = (cout, cin, 3, 3), (n, cout, h, w), "c3d", L.cine_conv3x3_dgrad, ref_conv3x3_dgrad
    elif kind == "c1":
        wshape, gshape, pack, fn, ref = (cout, cin), (n, cout, h, w), "c1d", L.cine_conv1x1_dgrad, ref_conv1x1_dgrad
    else:
        wshape, gshape, pack, fn, ref = (cin, cout, 2, 2), (n, cout, 2 * h, 2 * w), "tcd", L.cine_tconv2x2_dgrad, ref_tconv2x2_dgrad
    W1 = _rand(seed, *wshape) / (cout * (9 if kind == "c3" else 1)) ** 0.5
    W2 = _rand(seed + 1, *wshape) / (cout * (9 if kind == "c3" else 1)) ** 0.5
    gy = _rand(seed + 2, *gshape)
    s = _split_of(c)
    two = s is not None
    want = ref(gy, W1, W2 if two else None, s)
    wp1, wp2 = ops._pack(pack, W1.to(dev)), ops._pack(pack, W2.to(dev))
    gyd = _view(gy, off, dev)
    outs = []
    for rep in range(2):
        gx = Guarded((n, cin, h, w), off, dev, torch.full((n, cin, h, w), float("nan")))
        if kind == "tc":
            _check(fn(gyd.data_ptr(), wp1.data_ptr(), wp2.data_ptr() if two else None, s if two else n, gx.ptr(), n, cin, cout, h, w, _stream()), kind)
        else:
            _check(fn(gyd.data_ptr(), wp1.data_ptr(), wp2.data_ptr() if two else None, s if two else n, gx.ptr(), n, cout, cin, h, w, _stream()), kind)
        torch.cuda.synchronize()
        assert gx.intact(), f"write outside gx {c}"
        outs.append(gx.t.clone())
    assert torch.equal(outs[0], outs[1]), f"not deterministic {c}"
    assert not torch.isnan(outs[0]).any(), f"gx not fully written {c}"
    name = {"c3": "cine_conv3x3_dgrad", "c1": "cine_conv1x1_dgrad", "tc": "cine_tconv2x2_dgrad"}[kind]
    _record(name, rel_err(outs[0].cpu(), want), BAR, (c, off))


@gpu
@pytest.mark.parametrize("c", DGRAD3_CASES, ids=case_id)
def test_conv3x3_dgrad_sweep(dev, c):
    """Two weight sets with 0 < set_split < n ("mid"), set_split == n ("n": the second set unused) and one set ("none")."""
    _run_dgrad("c3", c, 0, dev, hash_case(c))


@gpu
@pytest.mark.parametrize("c", DGRAD1_CASES, ids=case_id)
def test_conv1x1_dgrad_sweep(dev, c):
    _run_dgrad("c1", c, 0, dev, hash_case(c))


@gpu
@pytest.mark.parametrize("c", TCONV_CASES, ids=case_id)
def test_tconv2x2_dgrad_sweep(dev, c):
    _run_dgrad("tc", c, 0, dev, hash_case(c))


@gpu
@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("kind,c", [("c3", c) for c in DGRAD3_CASES[::4]] + [("c1", c) for c in DGRAD1_CASES[::4]] +
                         [("tc", c) for c in TCONV_CASES[::4]], ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_dgrad_unaligned(dev, kind, c, off):
    _run_dgrad(kind, c, off, dev, hash_case(c))


@gpu
@pytest.mark.parametrize("c", GATED_CASES, ids=case_id)
def test_conv3x3_dgrad_gated(dev, c):
    """gx = gate > 0 ? conv(gy) + addend : 0, gate and addend each present or NULL; the gate is a ReLU output with exact zeros."""
    from cine_hip import ops
    L = _L()
    n, cout, cin, h, w = c["n"], c["cout"], c["cin"], c["h"], c["w"]
    seed = hash_case(c)
    W = _rand(seed, cout, cin, 3, 3) / (9 * cout) ** 0.5
    gy = _rand(seed + 1, n, cout, h, w)
    addend = _rand(seed + 2, n, cin, h, w) if c["addend"] else None
    gate = F.relu(_rand(seed + 3, n, cin, h, w)) if c["gate"] else None
    assert gate is None or (gate == 0).any()
    want = ref_conv3x3_dgrad(gy, W)
    if addend is not None:
        want = want + addend.double()
    if gate is not None:
        want = torch.where(gate > 0, want, torch.zeros_like(want))
    wp = ops._pack("c3d", W.to(dev))
    for off in (0, 1):
        gyd = _view(gy, off, dev)
        ad = _view(addend, off, dev) if addend is not None else None
        gt = _view(gate, off, dev) if gate is not None else None
        outs = []
        for rep in range(2):
            gx = Guarded((n, cin, h, w), off, dev, torch.full((n, cin, h, w), float("nan")))
            _check(L.cine_conv3x3_dgrad_gated(gyd.data_ptr(), wp.data_ptr(), None if ad is None else ad.data_ptr(),
                                              None if gt is None else gt.data_ptr(), gx.ptr(), n, cout, cin, h, w, _stream()),
                   "cine_conv3x3_dgrad_gated")
            torch.cuda.synchronize()
            assert gx.intact()
            outs.append(gx.t.clone())
        assert torch.equal(outs[0], outs[1])
        got = outs[0].cpu()
        if gate is not None:
            assert bool((got[gate == 0] == 0).all()), "masked entries must be exact zeros"
        _record("cine_conv3x3_dgrad_gated", rel_err(got, want), BAR, (c, off))


# ================================================================== InstanceNorm + LeakyReLU backward
def _records(x, how, dev):
    """Statistics records (n, c, np, 3) of x on the device, and the raw tensor they describe."""
    from cine_hip import ops
    n, c, h, w = x.shape
    xd = x.to(dev)
    if how == "one":
        return xd, ops.instnorm_partials(xd)
    if how == "conv":
        # a real conv output with one record per output tile: the identity 3x3 conv (centre tap 1) of the kink-free x
        Wid = torch.zeros(c, c, 3, 3)
        Wid[range(c), range(c), 1, 1] = 1.0
        y, part = ops.conv3x3_in([(xd, None, 0)], ops.pack_conv3x3(Wid.to(dev)), c, h, w)
        assert part.shape[2] > 1, part.shape
        return y, part
    k = int(how)
    pe = h * w
    assert pe % k == 0
    part = ops.instnorm_partials(xd.view(n, c * k, pe // k)).view(n, c, k, 3)
    return xd, part


def _run_in_bwd(x, g, how, slope, off, dev, with_ws=True):
    L = _L()
    n, c, h, w = x.shape
    r, part = _records(x, how, dev)
    rd, gd = _view(r, off, dev), _view(g, off, dev)
    nb = L.cine_in_lrelu_bwd_ws_bytes(n, c, h, w) if with_ws else 0
    outs = []
    for rep in range(2):
        gr = Guarded((n, c, h, w), off, dev, torch.full((n, c, h, w), float("nan")))
        ws = Workspace(nb, dev)
        _check(L.cine_in_lrelu_bwd(rd.data_ptr(), part.data_ptr(), part.shape[2], gd.data_ptr(), gr.ptr(), n, c, h, w, EPS, slope,
                                   ws.ptr() if with_ws else None, nb, _stream()), "cine_in_lrelu_bwd")
        torch.cuda.synchronize()
        assert gr.intact() and ws.intact()
        outs.append(gr.t.clone())
    assert torch.equal(outs[0], outs[1])
    assert not torch.isnan(outs[0]).any()
    return outs[0].cpu(), r.cpu(), part.shape[2], nb


@gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("case", IN_BWD_CASES, ids=lambda t: f"{t[6]}-{t[0]}x{t[1]}x{t[2]}x{t[3]}-rec{t[4]}-s{t[5]}")
def test_in_lrelu_bwd_paths(dev, case, off):
    """Each path of cine_in_lrelu_bwd (the id names the one an aligned call takes; at offset 1 the fast kernels and float4 pieces
    are skipped) against the closed form in float64, kink-free inputs, records merged across np > 1 tiles or chunks."""
    n, c, h, w, how, slope, path = case
    seed = 900 + IN_BWD_CASES.index(case)
    x = kink_free_planes(seed, (n, c, h, w))
    assert kink_margin(x) >= KINK_MARGIN
    g = _rand(seed + 1, n, c, h, w)
    got, r, np_, nb = _run_in_bwd(x, g, how, slope, off, dev, with_ws=path != "plane-nows")
    assert (nb > 0) == path.startswith("split"), (path, nb)
    assert how == "one" or np_ > 1
    assert kink_margin(r) >= KINK_MARGIN            # a conv output is x itself up to rounding: still off the kink
    _record("cine_in_lrelu_bwd", rel_err(got, ref_in_lrelu_bwd(r, g, slope)), BAR, (case, off))


@gpu
@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_in_lrelu_bwd_near_constant_plane(dev, slope):
    """A plane whose variance (~1e-8) is far below eps: rstd ~ 1 / sqrt(eps), the result ~300 times the incoming gradient."""
    x = _near_constant_plane(3)
    assert kink_margin(x) >= KINK_MARGIN
    g = _rand(4, *x.shape)
    for off in (0, 1):
        got, _, _, _ = _run_in_bwd(x, g, "one", slope, off, dev)
        _record("cine_in_lrelu_bwd", rel_err(got, ref_in_lrelu_bwd(x, g, slope)), BAR, ("near-constant", slope, off))


# ================================================================== ReLU mask
@gpu
@pytest.mark.parametrize("off", [0, 1, 2])
@pytest.mark.parametrize("n", RELU_MASK_N)
def test_relu_mask(dev, n, off):
    """g *= (y > 0) in place, bit for bit: the float4 body plus the scalar tail (n % 4 != 0) when aligned, the scalar kernel when not."""
    L = _L()
    g = _rand(n, n)
    y = F.relu(_rand(n + 1, n))
    y[::7] = -0.0
    gd = Guarded((n,), off, dev, g)
    yd = _view(y, off, dev)
    _check(L.cine_relu_mask(gd.ptr(), yd.data_ptr(), n, _stream()), "cine_relu_mask")
    torch.cuda.synchronize()
    assert gd.intact()
    assert torch.equal(gd.t.cpu(), torch.where(y > 0, g, torch.zeros_like(g)))
