"""The forward convolution entry points of include/cine_hip.h called one by one, shape by shape, against float64 references on the CPU.

Entry points: cine_conv3x3_in / _ex / _ex2, cine_crnn_step / _step2, cine_tconv2x2_in, cine_conv1x1_bias, cine_conv3d_in,
cine_tconv3d_in, cine_conv1x1x1_bias, cine_pool3d_act and cine_instnorm_partials / _finalize / _merge / _lrelu_apply.  The seeded case
lists cross the shapes where conv_kernels.hip's dispatcher changes route: the tile width (W 2 / 4 / 8 / 16), the lean plane kernels
(W equal to the tile width), the 16-wide column-tile kernel (W > 16, W % 4 == 0), the coarse K-split kernel, the padded row counts
(<= 16 / 32 / 64 / > 64), ragged last tiles, the 4-channel first-layer chunk, the record counts of the statistics merge (<= 4 / 8 / 16),
a NULL statistics output, two weight sets, the volume tile rules and the vectorised against the element-wise staging.

Every case checks
  * the error against float64 (max |d| / peak) at a bar of 1e-5: forward reductions stay far below 1e5 summed terms;
  * overwrite semantics: y, the statistics records and a storing accum overwrite a NaN prefill; an adding accum adds onto a random
    prefill at the output's scale;
  * guard floats on both sides of every output, the record buffer sized at exactly cine_conv_stat_partials[3d] records per plane;
  * the records: finite, positive integer counts that add up to the plane's pixels, and -- merged on the host in float64 (Chan) -- the
    mean and M2 of the kernel's own y (RECORD_MEAN_BAR, RECORD_M2_BAR: a record that drops one pixel of a 200 x 200 plane fails);
  * determinism: a second identical call gives the same bits;
  * the route: cine_diag_counter (counters 4 .. 12) names exactly one route per launch.  A case on a lean kernel (plane, transpose
    plane, column tiles) runs again with its cine_set_conv_plane bit cleared: a general route, the same bits.
Subsets run again with sources, outputs, addend and accum at storage offsets of 1, 2 and 3 floats, where every 16-byte check fails.

The references follow the header: InstanceNorm (biased variance, the call's eps) + LeakyReLU (the call's slope) from the exact source,
the avg-pool with floors, the Haar DWT / IWT of oracle/xpdnet_ref.py, zero outside a source's extent.  CPU tests check them against
torch modules and check that the case lists reach every axis value.
"""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from kernel_sweep import BAR, Guarded, Worst, cap_samples, case_id, hash_case, sweep, view_at
from oracle.xpdnet_ref import DWT, IWT

ROUTES = ("plane", "tconv_plane", "wide", "wide_v3", "coarse", "stream1x1", "pair", "general_vec", "general_elem")
D_FIRST = 4                                     # cine_diag_counter index of "plane" (csrc/common.h: Diag D_CONV_PLANE ..)
D_POOL3D_VEC, D_POOL3D_SCALAR = 13, 14          # cine_pool3d_act on pool3d_act_kernel<true> / <false>
LEAN = {"plane": 1, "tconv_plane": 2, "wide": 4, "wide_v3": 4}     # route -> its cine_set_conv_plane bit
GENERAL = {"general_vec", "general_elem", "pair"}
RECORD_MEAN_BAR = 2e-6                          # |merged mean - mean(y)| / (|mean(y)| + std(y))
RECORD_M2_BAR = 1e-5                            # |merged M2 - M2(y)| / M2(y)
CINE_EINVAL = -1
MAC_BUDGET = 150_000_000                        # multiply-adds of one float64 reference (cap_samples)
NAN = float("nan")


# ================================================================== float64 references (CPU)
def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def in_act(x, eps, slope):
    """LeakyReLU(InstanceNorm(x)) in float64 per (sample, channel) over all trailing dims, biased variance."""
    x = x.double()
    dims = tuple(range(2, x.dim()))
    mean = x.mean(dims, keepdim=True)
    var = (x - mean).pow(2).mean(dims, keepdim=True)
    return lrelu((x - mean) / torch.sqrt(var + eps), slope)


def fit(t, size):
    """t (n, c, *extent) cropped or zero-padded at the far end to `size`: a source reads as zero outside its extent."""
    out = t.new_zeros(tuple(t.shape[:2]) + tuple(size))
    sl = (slice(None), slice(None)) + tuple(slice(0, min(a, b)) for a, b in zip(t.shape[2:], size))
    out[sl] = t[sl]
    return out


def src_input(x, mode, eps, slope, size):
    """What one source contributes to the convolution input, float64, at the output extent `size`: mode 0 as is, 1 act, 2 act then
    2x avg-pool (floors), 3 Haar DWT, 4 Haar IWT; bit 3 (| 8) on modes 3 / 4: of act(x)."""
    base, raw = mode & 7, bool(mode & 8)
    if base in (1, 2) or raw:
        a = in_act(x, eps, slope)
    else:
        a = x.double()
    if base == 2:
        a = F.avg_pool2d(a, 2) if a.dim() == 4 else F.avg_pool3d(a, 2)
    elif base == 3:
        a = DWT()(a[..., :a.shape[-2] // 2 * 2, :a.shape[-1] // 2 * 2])
    elif base == 4:
        a = IWT()(a)
    return fit(a, size)


def conv_input(c, srcs, size):
    """The convolution input of a case: the sources' contributions concatenated, or added (add_src1)."""
    parts = [src_input(x, m, c["eps"], c["slope"], size) for x, m in srcs]
    if len(parts) == 2 and c.get("add"):
        return parts[0] + parts[1]
    return torch.cat(parts, 1)


def _per_set(n, split, fn):
    out = []
    if split > 0:
        out.append(fn(slice(0, split), 0))
    if split < n:
        out.append(fn(slice(split, n), 1))
    return torch.cat(out)


def _conv3d_by_slices(x, W, b, chunk=3):
    """conv3d(x, W, b, padding=1) computed a few output slices at a time (bounded im2col memory on full-size volumes)."""
    xp = F.pad(x, (0, 0, 0, 0, 1, 1))
    outs = [F.conv3d(xp[:, :, z:z + chunk + 2], W, b, padding=(0, 1, 1)) for z in range(0, x.shape[2], chunk)]
    return torch.cat(outs, 2)


def ref_conv(inp, ws, bs, split, addend=None, relu=False, kind="conv"):
    """y = conv(inp; ws[set]) + bs[set] (+ addend, then ReLU), samples >= split on set 1.  kind: "conv" (3x3 / 3x3x3 pad 1 or 1x1 /
    1x1x1 from the weight's shape) or "tconv" (k2 s2 transpose conv, 2-D or 3-D)."""
    inp = inp.double()
    n = inp.shape[0]

    def one(s, k):
        W = ws[k].double()
        b = None if bs is None or bs[k] is None else bs[k].double()
        if kind == "tconv":
            f = F.conv_transpose2d if W.dim() == 4 else F.conv_transpose3d
            return f(inp[s], W, b, stride=2)
        if W.dim() == 5 and W.shape[-1] == 3:
            return _conv3d_by_slices(inp[s], W, b)
        f = F.conv2d if W.dim() == 4 else F.conv3d
        return f(inp[s], W, b, padding=W.shape[-1] // 2)
    y = _per_set(n, split, one)
    if addend is not None:
        y = y + addend.double()
    return torch.relu(y) if relu else y


def records(x, k):
    """k contiguous-chunk statistics records {count, mean, M2} per (sample, channel) plane of x, float64 -> float32 (n, c, k, 3)."""
    n, c = x.shape[:2]
    flat = x.double().reshape(n, c, -1)
    pe = flat.shape[2]
    out = torch.zeros(n, c, k, 3, dtype=torch.float64)
    for i, idx in enumerate(np.array_split(np.arange(pe), k)):
        ch = flat[:, :, idx[0]:idx[-1] + 1]
        m = ch.mean(2)
        out[:, :, i, 0] = len(idx)
        out[:, :, i, 1] = m
        out[:, :, i, 2] = (ch - m[..., None]).pow(2).sum(2)
    return out.float()


def merge_records(p):
    """Chan's merge of records (..., np, 3) in float64 -> (count, mean, M2)."""
    p = p.double()
    cnt = p[..., 0].sum(-1)
    mean = (p[..., 0] * p[..., 1]).sum(-1) / cnt
    m2 = (p[..., 2] + p[..., 0] * (p[..., 1] - mean[..., None]).pow(2)).sum(-1)
    return cnt, mean, m2


def record_errors(part, y):
    """(worst |d mean| / (|mean| + std), worst |d M2| / M2) over the planes of y (n, c, ...) against its records (n, c, np, 3)."""
    _, mean, m2 = merge_records(part)
    yy = y.double().reshape(y.shape[0], y.shape[1], -1)
    ym = yy.mean(-1)
    ym2 = (yy - ym[..., None]).pow(2).sum(-1)
    scale = ym.abs() + (ym2 / yy.shape[-1]).sqrt()
    dmean = torch.where(scale > 0, (mean - ym).abs() / scale.clamp_min(1e-30), (mean - ym).abs())
    dm2 = torch.where(ym2 > 0, (m2 - ym2).abs() / ym2.clamp_min(1e-30), (m2 - ym2).abs())
    return float(dmean.max()), float(dm2.max())


# ================================================================== mirrors of the dispatch rules (csrc/conv_kernels.hip)
def cdiv(a, b):
    return -(-a // b)


def rows16(r):
    return cdiv(r, 16) * 16


def coarse_shape2d(rowsp, h, w):
    return w > 16 and rowsp > 32 and 32 + 2 * (w + 2) <= 192 and h * (w + 1) <= 4096


def _regular_nf(rowsp, frags):
    if rowsp <= 16:
        return 52
    if rowsp <= 32:
        return 26
    return 13 if rowsp <= 64 or frags > 8 else 4


def vol_small_tiles(rowsp, h, w, d):
    tw = 16 if w > 8 else 8 if w > 4 else 4 if w > 2 else 2
    frags = cdiv(h * tw, 16) * cdiv(w, tw)
    th = _regular_nf(rowsp, frags) * 16 // tw
    return cdiv(w, tw) * cdiv(h, th) * d * cdiv(rowsp, rowsp if rowsp <= 64 else 128) < 128


def coarse_shape(rowsp, h, w, d):
    return w > 8 and rowsp > 32 and vol_small_tiles(rowsp, h, w, d) and 32 + 2 * (w + 2) <= 192


def conv3d_v3_ok(c, ext0, ext1):
    """conv3d_v3_ok for a volume case (sources described by their mode and (d, h, w) extent)."""
    d, h, w = c["d"], c["h"], c["w"]

    def ok(mode, ext):
        if ext is None:
            return True
        if mode == 2:
            return ext[2] in (2 * w, 2 * w + 1) and ext[1] >= 2 * h
        return ext[2] == w and ext[1] <= h
    if not (w > 8 and ok(c["mode0"], ext0) and ok(c["mode1"], ext1) and (ext1 is None or c["c0"] % 8 == 0)):
        return False
    return not vol_small_tiles(rows16(c["cout"]), h, w, d) or rows16(c["cout"]) > 32


def unaligned_routes_2d(rowsp, h, w, ypart, fast_src):
    """The route of a 2-D 3x3 launch whose pointers all fail the 16-byte checks: the coarse kernel on its shapes (its element-wise
    staging only with a statistics record to keep in step), else the general kernel's element-wise staging."""
    if coarse_shape2d(rowsp, h, w) and (fast_src or ypart):
        return {"coarse"}
    return {"general_elem"}


def plane_exts(c):
    """(h, w) extents of a 2-D case's two sources (None: no second source)."""
    h, w = c["h"], c["w"]

    def ext(mode, kind):
        if mode == 2:
            if kind == "odd":
                return (2 * h + 1, 2 * w + 1)
            return (2 * max(1, h - 1), 2 * max(1, w - 2)) if kind == "short" else (2 * h, 2 * w)
        return (max(1, h - 1), max(1, w - 2)) if kind == "short" else (h, w)
    return ext(c["mode0"], c["ext"]), (ext(c["mode1"], "same") if c["c1"] else None)


def vol_exts(c):
    """(d, h, w) extents of a volume case's two sources (None: no second source); "shallow": an up volume one slice short."""
    d, h, w = c["d"], c["h"], c["w"]

    def ext(mode, kind):
        if mode == 2:
            return (2 * d + 1, 2 * h + 1, 2 * w + 1) if kind == "odd" else (2 * d, 2 * h, 2 * w)
        if kind == "short":
            return (d, max(1, h - 1), max(1, w - 2))
        if kind == "shallow":
            return (max(1, d - 1), h, w)
        return (d, h, w)
    return ext(c["mode0"], c["ext"]), (ext(c["mode1"], "same") if c["c1"] else None)


# ================================================================== case lists
W_AXIS = [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 20, 33, 52, 78, 80, 200]
H_AXIS = [1, 2, 7, 13, 26, 27, 52, 53, 104, 208]
COUT_AXIS = [1, 8, 16, 17, 32, 33, 64, 65, 128, 130]
CIN_AXIS = [1, 2, 3, 4, 7, 8, 9, 16, 17, 20]
REC_AXIS = [1, 4, 5, 8, 9, 16, 17, 64]
SLOPES = [0.0, 0.2, 1.0]
EPSS = [1e-5, 1e-3]
SPLITS = ["none", "zero", "mid", "n"]

CONV_AXES = dict(entry=["in", "ex", "ex2"], w=W_AXIS, h=H_AXIS, cout=COUT_AXIS, c0=CIN_AXIS, c1=[0, 0, 3, 8, 9, 16],
                 mode0=[0, 1, 2], mode1=[0, 1, 2], ext=["same", "same", "short", "odd"], rec=REC_AXIS, party=[True, True, False],
                 n=list(range(1, 17)), split=SPLITS, slope=SLOPES, eps=EPSS, bias=[False, True], addend=[False, True], relu=[False, True])


def _conv_macs(c, cin, taps=9):
    return c["h"] * c["w"] * c.get("d", 1) * cin * c["cout"] * taps


def _fix_conv(c, cap=True):
    """A swept 3x3 case made a valid call of its entry point: cine_conv3x3_in has no epilogue, cine_conv3x3_ex one weight set."""
    if c["entry"] == "in":
        c.update(bias=False, addend=False, relu=False)
    if c["entry"] == "ex":
        c["split"] = "none"
    if c["entry"] == "ex2" and c["split"] == "none":
        c["split"] = "mid"
    if cap:
        c["n"] = cap_samples(c["n"], _conv_macs(c, c["c0"] + c["c1"]) + 1, MAC_BUDGET)
    if c["split"] == "mid":
        c["n"] = max(c["n"], 2)
    return c


def _c3(cap=True, **kw):
    base = dict(entry="in", c1=0, mode1=0, ext="same", rec=1, party=True, split="none", slope=0.2, eps=1e-5, bias=False, addend=False,
                relu=False)
    base.update(kw)
    return _fix_conv(base, cap)


# Hand-placed cases carry the route they must take at an aligned base (PINNED, asserted by the sweep tests).
CONV_PINNED = [
    # the lean plane kernel: W equal to the tile width, plane modes 0 / 1 / 2, two sources, the 4-channel first-layer chunk
    (_c3(w=16, h=208, cout=16, c0=16, mode0=1, n=3, split="mid", eps=1e-3), "plane"),
    (_c3(w=8, h=104, cout=32, c0=16, c1=16, mode0=1, mode1=1, rec=5, n=2, slope=0.0), "plane"),
    (_c3(w=4, h=52, cout=64, c0=32, mode0=2, rec=9, n=2, split="zero", slope=1.0, eps=1e-3), "plane"),
    (_c3(w=16, h=13, cout=16, c0=2, mode0=0, n=4, split="n"), "plane"),
    # the column-tile kernel with a concatenated normalised second source
    (_c3(w=20, h=27, cout=16, c0=8, c1=8, mode0=1, mode1=1, rec=17, n=2, eps=1e-3), "wide"),
    # the 16-row small-MT tiles (few planes, no records): a ragged 18-channel input, which the column-tile kernel takes on its 52- and
    # 40-row shapes only -- the general kernel's vectorised staging with bias, addend and ReLU
    (_c3(entry="ex", w=80, h=53, cout=16, c0=16, c1=2, mode0=0, party=False, n=3, bias=True, addend=True, relu=True), "general_vec"),
    # the 40-row tiles (dispatch_tw, CINE_NO_MT10): the CRNN cells' all-frame conv over cat(hidden 16, image 2) of 15 frames of 200 x 200
    (_c3(cap=False, entry="ex", w=200, h=200, cout=16, c0=16, c1=2, mode0=0, party=False, n=15, bias=True, addend=True, relu=True), "wide"),
    # the coarse kernel: two sources with a ragged first one, a pooled source of odd extent
    (_c3(w=26, h=26, cout=64, c0=9, c1=7, mode0=1, rec=4, n=3, split="mid", eps=1e-3), "coarse"),
    (_c3(entry="ex2", w=33, h=13, cout=65, c0=16, mode0=2, ext="odd", rec=16, n=3, split="mid", slope=0.0, bias=True), "coarse"),
]
CONV_CASES = [_fix_conv(c) for c in sweep(1001, CONV_AXES, 56)] + [c for c, _ in CONV_PINNED]

WAV_AXES = dict(mode0=[3, 11, 4, 12], w=[2, 4, 8, 9, 16, 17, 20, 26, 50], h=[2, 4, 7, 8, 13, 26, 50], cq=[1, 2, 4, 8, 16],
                add=[False, True], mode1=[0, 1], cout=[1, 8, 16, 17, 32, 64], bias=[False, True], relu=[False, True], rec=REC_AXIS,
                party=[True, False], n=list(range(1, 9)), slope=SLOPES, eps=EPSS, split=["none", "mid"])
WAV_PINNED = [
    # the plane kernel's Haar DWT on load (TW 8) and its IWT + added skip (TW 16)
    (dict(mode0=11, w=8, h=16, cq=8, add=False, mode1=1, cout=16, bias=True, relu=False, rec=1, party=True, n=2, slope=0.2, eps=1e-3,
          split="mid"), "plane"),
    (dict(mode0=12, w=16, h=26, cq=16, add=True, mode1=1, cout=16, bias=True, relu=False, rec=4, party=True, n=2, slope=0.2, eps=1e-5,
          split="none"), "plane"),
    # a DWT whose 32 output rows have no plane shape at TW 16: the general kernel's wavelet staging
    (dict(mode0=11, w=16, h=16, cq=8, add=False, mode1=1, cout=32, bias=True, relu=False, rec=1, party=True, n=2, slope=0.2, eps=1e-3,
          split="mid"), "general_vec"),
]
WAV_CASES = sweep(1002, WAV_AXES, 20) + [c for c, _ in WAV_PINNED]
for _c in WAV_CASES:
    if _c["mode0"] & 7 == 4:                                # an IWT output has even extents
        _c["h"], _c["w"] = _c["h"] + _c["h"] % 2, _c["w"] + _c["w"] % 2
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"] * 8 * _c["cq"] * _c["cout"] * 9 + 1, MAC_BUDGET)
    _c["n"] = max(_c["n"], 2) if _c["split"] == "mid" else _c["n"]

CRNN_AXES = dict(c=[1, 2, 8, 16, 17], w=[1, 3, 4, 8, 9, 16, 17, 20, 33, 200], h=[1, 2, 7, 13, 27, 53, 200], n=[1, 2, 3, 4, 7],
                 relu=[False, True], accum=["none", "add"])
CRNN_CASES = sweep(1003, CRNN_AXES, 12)
CRNN2_CASES = []
for _i, (_sf, _sb, _xb, _relu) in enumerate(itertools.product((0, 1), (0, 1), (False, True), (False, True))):
    _c = sweep(1004 + _i, dict(c=[1, 2, 8, 16, 17], w=[3, 8, 16, 20, 33, 200], h=[2, 7, 13, 53, 200], n=[1, 2, 3]), 1)[0]
    _c.update(store_f=_sf, store_b=_sb, xb=_xb, relu=_relu)
    CRNN2_CASES.append(_c)
# both sets in one pair launch on planes the column-tile kernel does not take (W <= 16): the general kernel's pair form
CRNN2_PINNED = [(dict(c=8, w=9, h=13, n=2, store_f=1, store_b=0, xb=True, relu=True), "pair")]
CRNN2_CASES += [c for c, _ in CRNN2_PINNED]
for _c in CRNN_CASES + CRNN2_CASES:
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"] * _c["c"] * _c["c"] * 9 + 1, MAC_BUDGET)

TCONV_AXES = dict(cin=[1, 2, 3, 4, 7, 8, 9, 16, 17, 20, 32, 64, 128], cout=[1, 8, 16, 17, 32, 33, 64], w=[1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 33],
                  h=[1, 2, 7, 13, 26, 27, 52, 53, 104], mode=[0, 1], rec=REC_AXIS, n=list(range(1, 17)), split=SPLITS, slope=SLOPES, eps=EPSS)
TCONV_PINNED = [(dict(cin=32, cout=16, w=8, h=104, mode=1, rec=1, n=4, split="mid", slope=0.2, eps=1e-3), "tconv_plane"),   # the three
                (dict(cin=64, cout=32, w=4, h=52, mode=1, rec=1, n=4, split="mid", slope=0.2, eps=1e-5), "tconv_plane"),    # plane kernels
                (dict(cin=128, cout=64, w=2, h=26, mode=1, rec=4, n=4, split="none", slope=0.0, eps=1e-3), "tconv_plane")]
TCONV_CASES = sweep(1005, TCONV_AXES, 24) + [c for c, _ in TCONV_PINNED]
for _c in TCONV_CASES:
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"] * _c["cin"] * _c["cout"] * 4 + 1, MAC_BUDGET)
    _c["n"] = max(_c["n"], 2) if _c["split"] == "mid" else _c["n"]
TCONV_PLANE_SHAPES = {(32, 16, 8), (64, 32, 4), (128, 64, 2)}      # (cin, cout, W) of tconv_plane_kernel

C1_AXES = dict(cin=[1, 2, 3, 4, 7, 8, 9, 16, 17, 20, 33], cout=[1, 2, 3, 4, 8, 17, 33, 65], w=[1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 200],
               h=[1, 2, 7, 13, 26, 52, 200], mode=[0, 1], rec=REC_AXIS, n=list(range(1, 17)), split=SPLITS, slope=SLOPES, eps=EPSS)
C1_PINNED = [(dict(cin=16, cout=2, w=16, h=208, mode=1, rec=1, n=6, split="mid", slope=0.2, eps=1e-5), "stream1x1"),   # U-Net final
             (dict(cin=16, cout=4, w=200, h=200, mode=0, rec=1, n=2, split="zero", slope=0.2, eps=1e-5), "stream1x1")]
C1_CASES = sweep(1006, C1_AXES, 22) + [c for c, _ in C1_PINNED]
for _c in C1_CASES:
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"] * _c["cin"] * _c["cout"] + 1, MAC_BUDGET)
    _c["n"] = max(_c["n"], 2) if _c["split"] == "mid" else _c["n"]

VW_AXIS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 25, 33, 50]
VOL_AXES = dict(d=[1, 2, 3, 5, 7, 15], h=[1, 2, 3, 7, 13, 25, 26, 50], w=VW_AXIS, cout=[1, 8, 16, 17, 32, 33, 64, 65, 128],
                c0=[1, 2, 3, 8, 9, 16, 17], c1=[0, 0, 3, 8, 16], mode0=[0, 1, 2], mode1=[0, 1, 2], ext=["same", "same", "short", "odd", "shallow"],
                rec=REC_AXIS, party=[True, True, False], n=[1, 2, 3], slope=SLOPES, eps=EPSS, bias=[False, True], addend=[False, True],
                relu=[False, True])
VOL_PINNED = [
    # the coarse kernel, pooled on load from an odd 7 x 101 x 101 source
    (dict(d=3, h=50, w=50, cout=64, c0=32, c1=0, mode0=2, mode1=0, ext="odd", rec=64, party=True, n=1, slope=0.2, eps=1e-3,
          bias=False, addend=False, relu=False), "coarse"),
    # the V3 column tiles with an up volume one slice shallower than its skip (unet3d.hip's up path: 14 slices under 15)
    (dict(d=15, h=104, w=80, cout=16, c0=16, c1=16, mode0=1, mode1=1, ext="shallow", rec=9, party=True, n=1, slope=0.2, eps=1e-3,
          bias=False, addend=False, relu=False), "wide_v3"),
    # the same on a small-tile level of <= 32 rows (no V3 form): the 27-tap configurations
    (dict(d=7, h=20, w=20, cout=32, c0=16, c1=16, mode0=1, mode1=1, ext="shallow", rec=9, party=True, n=1, slope=0.2, eps=1e-5,
          bias=False, addend=False, relu=False), "general_vec"),
    (dict(d=5, h=9, w=17, cout=16, c0=8, c1=0, mode0=0, mode1=0, ext="same", rec=1, party=False, n=2, slope=0.2, eps=1e-5,
          bias=True, addend=True, relu=True), "general_vec"),
]
VOL_CASES = sweep(1007, VOL_AXES, 30) + [c for c, _ in VOL_PINNED]
for _c in VOL_CASES:
    _c["n"] = cap_samples(_c["n"], _conv_macs(_c, _c["c0"] + _c["c1"], 27) + 1, MAC_BUDGET)

TVOL_AXES = dict(d=[1, 2, 3, 5, 7, 15], h=[1, 2, 3, 7, 13, 25, 50], w=VW_AXIS, cin=[1, 2, 3, 8, 9, 16, 17, 32, 64], cout=[1, 2, 8, 16, 17, 32],
                 mode=[0, 1], rec=REC_AXIS, n=[1, 2, 3], slope=SLOPES, eps=EPSS)
TVOL_CASES = sweep(1008, TVOL_AXES, 16)
C111_CASES = sweep(1009, TVOL_AXES, 14)
for _c in TVOL_CASES + C111_CASES:
    _c["n"] = cap_samples(_c["n"], _c["d"] * _c["h"] * _c["w"] * _c["cin"] * _c["cout"] * 8 + 1, MAC_BUDGET)

POOL_CASES = [  # (planes, d, h, w, records, slope, eps, off): w % 8 == 0 and aligned -> the float4 kernel, else the scalar one (asserted)
    (5, 2, 2, 8, 1, 0.2, 1e-5, 0), (3, 3, 5, 16, 4, 0.0, 1e-3, 0), (2, 15, 200, 200, 64, 0.2, 1e-5, 0), (7, 5, 7, 9, 5, 1.0, 1e-3, 0),
    (4, 7, 13, 33, 9, 0.2, 1e-5, 0), (3, 3, 4, 16, 17, 0.2, 1e-3, 1), (1, 2, 3, 2, 1, 0.0, 1e-5, 2), (6, 5, 9, 24, 8, 0.2, 1e-3, 3)]
PARTIALS_CASES = [(8, 8192), (5, 8193), (9, 1), (7, 3), (3, 200 * 200), (13, 64)]     # (planes, elements per plane)

# Full-size layers: (name, kind, case, the route profiles/r06_rocprofv3_kernel_stats_{isolated,cfg4}.csv show for the layer)
FULL_LAYERS = [
    ("cfg2 U-Net level 0 first conv", "conv", _c3(w=16, h=208, cout=16, c0=2, mode0=0, n=8, split="mid"), "plane"),
    ("cfg2 U-Net level 0", "conv", _c3(w=16, h=208, cout=16, c0=16, mode0=1, n=8, split="mid"), "plane"),
    ("cfg2 U-Net level 1 pooled", "conv", _c3(w=8, h=104, cout=32, c0=16, mode0=2, n=8, split="mid"), "plane"),
    ("cfg2 U-Net level 2", "conv", _c3(w=4, h=52, cout=64, c0=64, mode0=1, n=8, split="mid"), "plane"),
    ("cfg2 U-Net level 3", "conv", _c3(w=2, h=26, cout=128, c0=128, mode0=1, n=8, split="mid"), "plane"),
    ("cfg2 U-Net up level 0", "conv", _c3(w=16, h=208, cout=16, c0=16, c1=16, mode0=1, mode1=1, rec=4, n=4, split="mid"), "plane"),
    ("cfg2 tconv 32 to 16", "tconv", dict(cin=32, cout=16, w=8, h=104, mode=1, rec=1, n=8, split="mid", slope=0.2, eps=1e-5), "tconv_plane"),
    ("cfg2 final 1x1", "c1", dict(cin=16, cout=2, w=16, h=208, mode=1, rec=1, n=8, split="mid", slope=0.2, eps=1e-5), "stream1x1"),
    ("sensitivity net 208 x 208 level", "conv", _c3(w=208, h=208, cout=8, c0=8, mode0=1, n=2), "wide"),
    ("sensitivity net 26 x 26 x 64 level", "conv", _c3(cap=False, w=26, h=26, cout=64, c0=64, mode0=1, n=15), "coarse"),
    ("CRNN cell 200 x 200", "crnn", dict(c=16, w=200, h=200, n=1, relu=True, accum="add"), "wide"),
    ("cfg4 level 0 15 x 200 x 200", "vol", dict(d=15, h=200, w=200, cout=16, c0=16, c1=0, mode0=1, mode1=0, ext="same", rec=1, party=True,
                                                n=1, slope=0.2, eps=1e-5, bias=False, addend=False, relu=False), "wide_v3"),
    ("cfg4 level 1 7 x 100 x 100", "vol", dict(d=7, h=100, w=100, cout=32, c0=16, c1=0, mode0=0, mode1=0, ext="same", rec=1, party=True,
                                               n=1, slope=0.2, eps=1e-5, bias=False, addend=False, relu=False), "wide_v3"),
    ("cfg4 level 2 pooled on load", "vol", dict(d=3, h=50, w=50, cout=64, c0=32, c1=0, mode0=2, mode1=0, ext="same", rec=1, party=True,
                                                n=1, slope=0.2, eps=1e-5, bias=False, addend=False, relu=False), "coarse"),
    ("cfg4 level 3", "vol", dict(d=1, h=25, w=25, cout=128, c0=128, c1=0, mode0=1, mode1=0, ext="same", rec=1, party=True,
                                 n=1, slope=0.2, eps=1e-5, bias=False, addend=False, relu=False), "coarse"),
    ("cfg4 tconv 32 to 16", "tvol", dict(d=7, h=100, w=100, cin=32, cout=16, mode=1, rec=1, n=1, slope=0.2, eps=1e-5), "general_vec"),
    ("cfg4 final 1x1x1", "c111", dict(d=15, h=200, w=200, cin=16, cout=2, mode=1, rec=1, n=1, slope=0.2, eps=1e-5), "general_vec"),
]
FULL_POOL = (16, 15, 200, 200, 1, 0.2, 1e-5, 0)         # cfg 4's pooled level-1 input: pool3d_act_kernel<true>


@functools.lru_cache(maxsize=None)
def pinned():
    """(kind, case id) -> the route a hand-placed case must take at an aligned base (after the sample caps above)."""
    pins = {}
    for kind, lst in (("conv", CONV_PINNED), ("crnn2", CRNN2_PINNED), ("tconv", TCONV_PINNED), ("c1", C1_PINNED), ("vol", VOL_PINNED)):
        for c, route in lst:
            pins[(kind, case_id(c))] = route
    for c, route in WAV_PINNED:
        pins[("conv", case_id(_wav_case(c)))] = route
    return pins


def forty_row_tiles(c):
    """dispatch_tw's 40-row rule for a 2-D 3x3 case: <= 16 rows, no records, wider than 16, not the small-MT shape, and 40-row tiles at four
    workgroups per CU take fewer resident rounds x rows than 52-row tiles at three."""
    n, h, w = c["n"], c["h"], c["w"]
    frags = cdiv(h * 16, 16) * cdiv(w, 16)
    if rows16(c["cout"]) > 16 or c["party"] or w <= 16 or n * cdiv(frags, 52) < 200:
        return False
    w13, w10 = n * cdiv(w, 16) * cdiv(h, 52), n * cdiv(w, 16) * cdiv(h, 40)
    return cdiv(w10, 1024) * 40 < cdiv(w13, 768) * 39


# ================================================================== CPU checks of the references and the case lists
def test_references_vs_torch_modules():
    rs = np.random.RandomState(3)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))                 # noqa: E731
    x = t(2, 3, 9, 11) * 1.5 + 0.3
    for eps, slope in ((1e-5, 0.2), (1e-3, 0.0), (1e-5, 1.0)):
        want = F.leaky_relu(F.instance_norm(x, eps=eps), slope)
        assert rel_err(in_act(x, eps, slope), want) < 1e-12
        assert rel_err(src_input(x, 2, eps, slope, (4, 5)), F.avg_pool2d(want, 2)) < 1e-12
        assert rel_err(src_input(x, 11, eps, slope, (4, 5)), DWT()(want[..., :8, :10])) < 1e-12
    v = t(2, 3, 5, 7, 9)
    assert rel_err(src_input(v, 2, 1e-5, 0.2, (2, 3, 4)), F.avg_pool3d(F.leaky_relu(F.instance_norm(v, eps=1e-5), 0.2), 2)) < 1e-12
    # a source shorter than the output reads as zero beyond its extent; a longer one is cut
    s = src_input(x, 0, 1e-5, 0.2, (12, 6))
    assert torch.equal(s[:, :, :9, :6], x[..., :6]) and bool((s[:, :, 9:] == 0).all())
    # the IWT inverts the DWT
    e = t(1, 2, 6, 8)
    assert rel_err(src_input(src_input(e, 3, 1e-5, 0.2, (3, 4)), 4, 1e-5, 0.2, (6, 8)), e) < 1e-12
    # the conv reference against torch's modules: two sets, bias, addend, ReLU; transpose convs; the sliced 3-D conv
    inp, W1, W2, b1, b2, ad = t(4, 3, 6, 5), t(5, 3, 3, 3), t(5, 3, 3, 3), t(5), t(5), t(4, 5, 6, 5)
    got = ref_conv(inp, (W1, W2), (b1, b2), 1, ad, True)
    want = torch.relu(torch.cat([F.conv2d(inp[:1], W1, b1, padding=1), F.conv2d(inp[1:], W2, b2, padding=1)]) + ad)
    assert rel_err(got, want) < 1e-12
    Wt = t(3, 5, 2, 2)
    assert rel_err(ref_conv(inp, (Wt, Wt), None, 4, kind="tconv"), F.conv_transpose2d(inp, Wt, stride=2)) < 1e-12
    v3, W3, b3 = t(2, 3, 7, 5, 4), t(4, 3, 3, 3, 3), t(4)
    assert rel_err(ref_conv(v3, (W3, W3), (b3, b3), 2), F.conv3d(v3, W3, b3, padding=1)) < 1e-12
    Wt3 = t(3, 5, 2, 2, 2)
    assert rel_err(ref_conv(v3, (Wt3, Wt3), None, 2, kind="tconv"), F.conv_transpose3d(v3, Wt3, stride=2)) < 1e-12


def test_records_merge_to_plane_statistics():
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((2, 3, 7, 9)) * 2 + 1)
    flat = x.reshape(2, 3, -1)
    for k in (1, 4, 5, 17, 63):
        cnt, mean, m2 = merge_records(records(x, k))
        assert bool((cnt == 63).all())
        assert rel_err(mean, flat.mean(-1)) < 1e-6 and rel_err(m2, (flat - flat.mean(-1, keepdim=True)).pow(2).sum(-1)) < 1e-6
    # the bars catch a record whose mean and M2 omit one pixel of a 200 x 200 plane that its count still includes
    y = torch.from_numpy(np.random.RandomState(5).standard_normal((1, 1, 200, 200)))
    assert max(record_errors(records(y, 169), y)) < 0.1 * RECORD_MEAN_BAR
    chunks = np.array_split(np.arange(40_000), 169)
    caught = 0
    for i in range(0, 169, 12):
        p = records(y, 169).double()
        part = y.reshape(-1)[chunks[i][0]:chunks[i][-1]]          # chunk i without its last pixel
        p[0, 0, i, 1] = part.mean()
        p[0, 0, i, 2] = (part - part.mean()).pow(2).sum()
        dmean, dm2 = record_errors(p, y)
        caught += dmean > RECORD_MEAN_BAR or dm2 > RECORD_M2_BAR
    assert caught == len(range(0, 169, 12)), caught


def test_sweeps_cover_every_axis_value():
    """Every value of every axis is reached (the sample counts are capped); the volume and plane rules; every crnn_step2 combination."""
    for cases, axes, skip in ((CONV_CASES, CONV_AXES, {"n"}), (WAV_CASES, WAV_AXES, {"n", "h", "w"}), (CRNN_CASES, CRNN_AXES, {"n"}),
                              (TCONV_CASES, TCONV_AXES, {"n"}), (C1_CASES, C1_AXES, {"n"}), (VOL_CASES, VOL_AXES, {"n"}),
                              (TVOL_CASES, TVOL_AXES, {"n"}), (C111_CASES, TVOL_AXES, {"n"})):
        for a, vals in axes.items():
            if a not in skip:
                assert {c[a] for c in cases} >= set(vals), a
    assert {c["n"] for c in CONV_CASES + TCONV_CASES + C1_CASES} >= {1, 16}
    assert any(c["c1"] > 0 and c["c0"] % 8 for c in CONV_CASES)
    assert {(c["store_f"], c["store_b"], c["xb"], c["relu"]) for c in CRNN2_CASES} == \
        set(itertools.product((0, 1), (0, 1), (False, True), (False, True)))
    assert {4 * c["cout"] for c in TCONV_CASES} >= {128, 256}
    assert {(c["cin"], c["cout"], c["w"]) for c in TCONV_CASES} >= TCONV_PLANE_SHAPES
    assert {c["w"] > 8 for c in VOL_CASES} == {False, True} and {c["w"] > 8 for c in TVOL_CASES} == {False, True}
    vols = [(rows16(c["cout"]), c["h"], c["w"], c["d"]) for c in VOL_CASES]
    assert any(coarse_shape(*v) for v in vols) and any(vol_small_tiles(*v) and not coarse_shape(*v) for v in vols)
    assert any(conv3d_v3_ok(c, *vol_exts(c)) for c in VOL_CASES) and any(not conv3d_v3_ok(c, *vol_exts(c)) for c in VOL_CASES)
    assert any(c["mode0"] == 2 and c["ext"] == "odd" for c in VOL_CASES) and any(c["c1"] and c["ext"] == "shallow" for c in VOL_CASES)
    assert any(coarse_shape2d(rows16(c["cout"]), c["h"], c["w"]) for c in CONV_CASES)
    assert {p % 4 for p, *_ in POOL_CASES} >= {1, 2, 3} and {w % 8 == 0 for _, _, _, w, *_ in POOL_CASES} == {False, True}
    assert any(d % 2 and h % 2 and w % 2 for _, d, h, w, *_ in POOL_CASES)
    assert {pe for _, pe in PARTIALS_CASES} >= {8192, 8193} and any(p % 4 for p, _ in PARTIALS_CASES)
    assert {r for _, _, _, r in FULL_LAYERS} == set(ROUTES) - {"pair", "general_elem"}
    # every hand-placed case names its route; with the unaligned tests' general_elem they name every route
    hand = len(CONV_PINNED) + len(WAV_PINNED) + len(CRNN2_PINNED) + len(TCONV_PINNED) + len(C1_PINNED) + len(VOL_PINNED)
    assert len(pinned()) == hand and set(pinned().values()) | {"general_elem"} == set(ROUTES)
    # the mirrored dispatch rules agree with the pins they can decide
    assert [forty_row_tiles(c) for c, _ in CONV_PINNED].count(True) == 1
    assert forty_row_tiles(next(c for c, _ in CONV_PINNED if c["w"] == 200))
    for c, route in VOL_PINNED:
        assert route in vol_routes(c), (c, route)
    assert any(c["c1"] and c["ext"] == "shallow" and conv3d_v3_ok(c, *vol_exts(c)) for c, _ in VOL_PINNED)


# ================================================================== GPU harness
gpu = pytest.mark.gpu
WORST = Worst()
ROUTE_LOG = {}          # entry point -> {route: launches}
CASE_LOG = {}           # route -> cases that took it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()
    if ROUTE_LOG:
        print("\nlaunches per route:")
        for k in sorted(ROUTE_LOG):
            print(f"  {k:28s} " + ", ".join(f"{r} {v}" for r, v in sorted(ROUTE_LOG[k].items())))
        print("cases per route: " + ", ".join(f"{r} {len(CASE_LOG.get(r, ()))}" for r in ROUTES))


def _L():
    from cine_hip._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed % 2_147_483_000).standard_normal(shape).astype(np.float32))


def _src(seed, shape):
    return _rand(seed, *shape) * 1.3 + 0.3


def _p(t):
    return None if t is None else t.data_ptr()


def _counts(L):
    return [L.cine_diag_counter(D_FIRST + i, 0) for i in range(len(ROUTES))]


def _launch(what, call, outs, launches=1):
    """Run call() once; returns the route it took, after checking the return code, the guards and one route per launch."""
    L = _L()
    before = _counts(L)
    code = call()
    torch.cuda.synchronize()
    after = _counts(L)
    if code != 0:
        raise AssertionError(f"{what} failed ({code}): {L.cine_last_error().decode(errors='replace')}")
    for name, g in outs.items():
        assert g.intact(), f"{what}: write outside {name}"
    delta = {r: a - b for r, a, b in zip(ROUTES, after, before) if a != b}
    assert sum(delta.values()) == launches and len(delta) == 1, (what, delta)
    route = next(iter(delta))
    log = ROUTE_LOG.setdefault(what, {})
    log[route] = log.get(route, 0) + launches
    return route


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run(what, call, make_outs, case, launches=1, exact=True):
    """call(outs) twice on fresh outputs: the same bits and route; a lean-kernel route runs a third time with its cine_set_conv_plane bit
    cleared, which must take a general route and give the same bits -- or, with exact=False, outputs the caller checks against float64
    as well (returned under "general:<name>").  Returns ({name: cpu tensor}, route)."""
    from cine_hip import ops
    res = []
    for rep in range(2):
        outs = make_outs()
        route = _launch(what, lambda: call(outs), outs, launches)
        res.append(({k: g.t.cpu() for k, g in outs.items()}, route))
    (o1, r1), (o2, r2) = res
    assert r1 == r2, (what, r1, r2)
    for k in o1:
        assert _same_bits(o1[k], o2[k]), f"{what}: {k} not deterministic"
    CASE_LOG.setdefault(r1, set()).add((what, case))
    if r1 in LEAN:
        outs = make_outs()
        try:
            ops.set_conv_plane(7 & ~LEAN[r1])
            r3 = _launch(what, lambda: call(outs), outs, launches)
        finally:
            ops.set_conv_plane(7)
        assert r3 in GENERAL, (what, r1, r3)
        for k in list(o1):
            if exact:
                assert _same_bits(o1[k], outs[k].t.cpu()), f"{what}: {k} differs between {r1} and {r3}"
            else:
                o1["general:" + k] = outs[k].t.cpu()
    return o1, r1


def _check_pin(kind, c, off, route):
    """A hand-placed case at an aligned base takes the route it is placed for."""
    want = pinned().get((kind, case_id(c)))
    assert off != 0 or want is None or route == want, (kind, case_id(c), route, want)


def _check_y(what, y, want, case):
    assert not torch.isnan(y).any(), f"{what}: y not fully written {case}"
    WORST.record(what, rel_err(y, want), BAR, case)


def _check_records(what, part, y, pixels, case):
    assert bool(torch.isfinite(part).all()), f"{what}: non-finite record {case}"
    cnt = part[..., 0].double()
    assert bool((cnt > 0).all()) and bool((cnt == cnt.round()).all()), f"{what}: bad counts {case}"
    assert bool((cnt.sum(-1) == pixels).all()), f"{what}: counts do not add up to {pixels} {case}"
    dmean, dm2 = record_errors(part, y)
    WORST.record(what + " (records mean)", dmean, RECORD_MEAN_BAR, case)
    WORST.record(what + " (records M2)", dm2, RECORD_M2_BAR, case)


def _split_of(split, n):
    return {"none": None, "zero": 0, "mid": max(1, n // 2), "n": n}[split]


# ================================================================== 3x3 convolutions (cine_conv3x3_in / _ex / _ex2)
def _conv_data(c, seed):
    n, h, w, cout = c["n"], c["h"], c["w"], c["cout"]
    e0, e1 = plane_exts(c)
    x0 = _src(seed, (n, c["c0"]) + e0)
    x1 = _src(seed + 1, (n, c["c1"]) + e1) if c["c1"] else None
    p0 = records(x0, min(c["rec"], e0[0] * e0[1])) if c["mode0"] else None
    p1 = records(x1, min(c["rec"], e1[0] * e1[1])) if x1 is not None and c["mode1"] else None
    srcs = [(x0, c["mode0"])] + ([(x1, c["mode1"])] if x1 is not None else [])
    return _conv_finish(c, seed, dict(x0=x0, x1=x1, p0=p0, p1=p1, e0=e0, e1=e1), conv_input(c, srcs, (h, w)))


def _conv_finish(c, seed, d, inp):
    n, h, w, cout = c["n"], c["h"], c["w"], c["cout"]
    cin = inp.shape[1]
    W1 = _rand(seed + 2, cout, cin, 3, 3) / (9 * cin) ** 0.5
    W2 = _rand(seed + 3, cout, cin, 3, 3) / (9 * cin) ** 0.5
    b1 = _rand(seed + 4, cout) if c["bias"] else None
    b2 = _rand(seed + 5, cout) if c["bias"] else None
    addend = _rand(seed + 6, n, cout, h, w) if c["addend"] else None
    split = _split_of(c["split"], n)
    want = ref_conv(inp, (W1, W2), (b1, b2), n if split is None else split, addend, c["relu"])
    d.update(W1=W1, W2=W2, b1=b1, b2=b2, addend=addend, split=split, want=want)
    return d


def _run_conv(c, off, dev, seed, data=None):
    """One 3x3 case on views at storage offset `off`; returns (y, records, route) after every per-case check."""
    from cine_hip import ops
    L = _L()
    d = data or _conv_data(c, seed)
    n, h, w, cout = c["n"], c["h"], c["w"], c["cout"]
    x0, x1 = view_at(d["x0"], off, dev), (view_at(d["x1"], off, dev) if d["x1"] is not None else None)
    p0 = d["p0"].to(dev) if d["p0"] is not None else None
    p1 = d["p1"].to(dev) if d["p1"] is not None else None
    wp1, wp2 = ops.pack_conv3x3(d["W1"].to(dev)), ops.pack_conv3x3(d["W2"].to(dev))
    b1 = d["b1"].to(dev) if d["b1"] is not None else None
    b2 = d["b2"].to(dev) if d["b2"] is not None else None
    ad = view_at(d["addend"], off, dev) if d["addend"] is not None else None
    nrec = L.cine_conv_stat_partials(cout, h, w, 0)
    np0, np1 = (0 if p0 is None else p0.shape[2]), (0 if p1 is None else p1.shape[2])
    e0, e1 = d["e0"], d["e1"] or (0, 0)
    c1, split, add = c["c1"], d["split"], int(bool(c.get("add")))

    def outs():
        o = {"y": Guarded((n, cout, h, w), off, dev, torch.full((n, cout, h, w), NAN))}
        if c["party"]:
            o["part"] = Guarded((n, cout, nrec, 3), off, dev, torch.full((n, cout, nrec, 3), NAN))
        return o

    def call(o):
        a0 = (x0.data_ptr(), _p(p0), np0, x0.shape[1], c["mode0"], e0[0], e0[1], _p(x1), _p(p1), np1, c1, c["mode1"] if c1 else 0, e1[0], e1[1])
        y, py = o["y"].ptr(), (o["part"].ptr() if "part" in o else None)
        if c["entry"] == "in":
            return L.cine_conv3x3_in(*a0, wp1.data_ptr(), None if split is None else wp2.data_ptr(), split or 0, y, py, n, cout, h, w,
                                     c["eps"], c["slope"], _stream())
        if c["entry"] == "ex":
            return L.cine_conv3x3_ex(*a0, add, wp1.data_ptr(), _p(b1), _p(ad), int(c["relu"]), y, py, n, cout, h, w, c["eps"], c["slope"],
                                     _stream())
        return L.cine_conv3x3_ex2(*a0, add, wp1.data_ptr(), _p(b1), wp2.data_ptr(), _p(b2), split, _p(ad), int(c["relu"]), y, py, n, cout,
                                  h, w, c["eps"], c["slope"], _stream())
    what = "cine_conv3x3_" + c["entry"]
    # the plane kernel's Haar DWT on load regroups each K chunk as two source channels x four bands (the general kernel: eight source
    # channels of one band): the same sums in another order, so both routes are held to float64 instead of to each other's bits
    o, route = _run(what, call, outs, case_id(c), exact=c["mode0"] & 7 != 3)
    _check_pin("conv", c, off, route)
    for pre in ("", "general:") if "general:y" in o else ("",):
        _check_y(what, o[pre + "y"], d["want"], (case_id(c), off, pre))
        if c["party"]:
            _check_records(what, o[pre + "part"], o[pre + "y"], h * w, (case_id(c), off, pre))
    return o["y"], o.get("part"), route


@gpu
@pytest.mark.parametrize("c", CONV_CASES, ids=case_id)
def test_conv3x3_sweep(dev, c):
    _run_conv(c, 0, dev, hash_case(c))


@gpu
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("c", CONV_CASES[::5], ids=case_id)
def test_conv3x3_unaligned(dev, c, off):
    """Sources, addend and outputs at storage offset 1 .. 3 floats: every 16-byte check fails."""
    _, _, route = _run_conv(c, off, dev, hash_case(c))
    assert route in unaligned_routes_2d(rows16(c["cout"]), c["h"], c["w"], c["party"], True), (c, route)


# ---------------------------------------------------------------- Haar DWT / IWT sources (cine_conv3x3_ex / _ex2)
def _wav_case(c):
    """A wavelet case as a 3x3 case: mode 3 reads 4 cq channels from a (2h, 2w) source of cq, mode 4 cq channels from an (h/2, w/2) source
    of 4 cq; an added skip has as many channels as the transform gives."""
    dwt = c["mode0"] & 7 == 3
    cin = 4 * c["cq"] if dwt else c["cq"]
    return dict(entry="ex2" if c["split"] == "mid" else "ex", w=c["w"], h=c["h"], cout=c["cout"], c0=c["cq"] if dwt else 4 * c["cq"],
                c1=cin if c["add"] else 0, mode0=c["mode0"], mode1=c["mode1"], ext="same", rec=c["rec"], party=c["party"], n=c["n"],
                split=c["split"], slope=c["slope"], eps=c["eps"], bias=c["bias"], addend=False, relu=c["relu"], add=c["add"])


def _wav_data(cc, seed):
    n, h, w = cc["n"], cc["h"], cc["w"]
    e0 = (2 * h, 2 * w) if cc["mode0"] & 7 == 3 else (h // 2, w // 2)
    x0 = _src(seed, (n, cc["c0"]) + e0)
    x1 = _src(seed + 1, (n, cc["c1"], h, w)) if cc["c1"] else None
    p0 = records(x0, min(cc["rec"], e0[0] * e0[1])) if cc["mode0"] & 8 else None
    p1 = records(x1, min(cc["rec"], h * w)) if x1 is not None and cc["mode1"] else None
    srcs = [(x0, cc["mode0"])] + ([(x1, cc["mode1"])] if x1 is not None else [])
    d = dict(x0=x0, x1=x1, p0=p0, p1=p1, e0=e0, e1=(h, w) if x1 is not None else None)
    return _conv_finish(cc, seed, d, conv_input(cc, srcs, (h, w)))


@gpu
@pytest.mark.parametrize("c", WAV_CASES, ids=case_id)
def test_conv3x3_wavelet_sources(dev, c):
    """Haar DWT / IWT sources, raw (bit 3: normalised on load) or as is, concatenated or with an added skip; every fourth case again at
    storage offset 1."""
    cc = _wav_case(c)
    seed = hash_case(c)
    data = _wav_data(cc, seed)
    _run_conv(cc, 0, dev, seed, data)
    if WAV_CASES.index(c) % 4 == 0:
        _, _, route = _run_conv(cc, 1, dev, seed, data)
        assert route in unaligned_routes_2d(rows16(cc["cout"]), cc["h"], cc["w"], cc["party"], False), (c, route)


# ================================================================== CRNN steps
def _run_crnn(c, off, dev, seed):
    from cine_hip import ops
    L = _L()
    n, ch, h, w = c["n"], c["c"], c["h"], c["w"]
    x, ad = _rand(seed, n, ch, h, w), _rand(seed + 1, n, ch, h, w)
    W = _rand(seed + 2, ch, ch, 3, 3) / (9 * ch) ** 0.5
    y_ref = ref_conv(x, (W, W), None, n, ad, c["relu"])
    pre = _rand(seed + 3, n, ch, h, w) * (float(y_ref.abs().max()) + 1.0)
    wp = ops.pack_conv3x3(W.to(dev))
    xd, add = view_at(x, off, dev), view_at(ad, off, dev)

    def outs():
        o = {"y": Guarded((n, ch, h, w), off, dev, torch.full((n, ch, h, w), NAN))}
        if c["accum"] == "add":
            o["accum"] = Guarded((n, ch, h, w), off, dev, pre)
        return o

    def call(o):
        return L.cine_crnn_step(xd.data_ptr(), wp.data_ptr(), add.data_ptr(), o["y"].ptr(), o["accum"].ptr() if "accum" in o else None,
                                n, ch, h, w, int(c["relu"]), _stream())
    o, route = _run("cine_crnn_step", call, outs, case_id(c))
    _check_y("cine_crnn_step", o["y"], y_ref, (case_id(c), off))
    if "accum" in o:
        WORST.record("cine_crnn_step (accum)", rel_err(o["accum"].double() - pre.double(), y_ref), BAR, (case_id(c), off))
    return route


@gpu
@pytest.mark.parametrize("c", CRNN_CASES, ids=case_id)
def test_crnn_step_sweep(dev, c):
    _run_crnn(c, 0, dev, hash_case(c))


@gpu
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("c", CRNN_CASES[::3], ids=case_id)
def test_crnn_step_unaligned(dev, c, off):
    assert _run_crnn(c, off, dev, hash_case(c)) == "general_elem", c


def _pair_config(c):
    """crnn_step2 with both sets in ONE pair launch (crnn_step2_impl: <= 16 padded rows, few 52-row tiles)."""
    tw = 16 if c["w"] > 8 else 8 if c["w"] > 4 else 4 if c["w"] > 2 else 2
    frags = cdiv(c["h"] * tw, 16) * cdiv(c["w"], tw)
    return rows16(c["c"]) <= 16 and 2 * c["n"] * cdiv(frags, 52) < 200


def _run_crnn2(c, off, dev, seed):
    from cine_hip import ops
    L = _L()
    n, ch, h, w = c["n"], c["c"], c["h"], c["w"]
    W = _rand(seed, ch, ch, 3, 3) / (9 * ch) ** 0.5
    wp = ops.pack_conv3x3(W.to(dev))
    sets = ["f", "b"] if c["xb"] else ["f"]
    data = {}
    for i, s in enumerate(sets):
        x, ad = _rand(seed + 10 * i + 1, n, ch, h, w), _rand(seed + 10 * i + 2, n, ch, h, w)
        y = ref_conv(x, (W, W), None, n, ad, c["relu"])
        store = c["store_" + s]
        pre = torch.full((n, ch, h, w), NAN) if store else _rand(seed + 10 * i + 3, n, ch, h, w) * (float(y.abs().max()) + 1.0)
        data[s] = (view_at(x, off, dev), view_at(ad, off, dev), y, pre, store)

    def outs():
        o = {}
        for s in sets:
            o["y_" + s] = Guarded((n, ch, h, w), off, dev, torch.full((n, ch, h, w), NAN))
            o["accum_" + s] = Guarded((n, ch, h, w), off, dev, data[s][3])
        return o

    def call(o):
        xf, af, _, _, sf = data["f"]
        if c["xb"]:
            xb, ab, _, _, sb = data["b"]
            return L.cine_crnn_step2(xf.data_ptr(), af.data_ptr(), o["y_f"].ptr(), o["accum_f"].ptr(), sf, xb.data_ptr(), ab.data_ptr(),
                                     o["y_b"].ptr(), o["accum_b"].ptr(), sb, wp.data_ptr(), n, ch, h, w, int(c["relu"]), _stream())
        return L.cine_crnn_step2(xf.data_ptr(), af.data_ptr(), o["y_f"].ptr(), o["accum_f"].ptr(), sf, None, None, None, None, 0,
                                 wp.data_ptr(), n, ch, h, w, int(c["relu"]), _stream())
    launches = 2 if c["xb"] and not _pair_config(c) else 1
    o, route = _run("cine_crnn_step2", call, outs, case_id(c), launches)
    _check_pin("crnn2", c, off, route)
    for s in sets:
        _, _, y, pre, store = data[s]
        _check_y("cine_crnn_step2", o["y_" + s], y, (case_id(c), s, off))
        acc = o["accum_" + s].double() if store else o["accum_" + s].double() - pre.double()
        assert not torch.isnan(acc).any(), (c, s)
        WORST.record("cine_crnn_step2 (accum)", rel_err(acc, y), BAR, (case_id(c), s, off))
    return route


@gpu
@pytest.mark.parametrize("c", CRNN2_CASES, ids=case_id)
def test_crnn_step2_every_combination(dev, c):
    """store_f / store_b (overwrite a NaN prefill or add onto a random one), x_b NULL or given, ReLU or none."""
    route = _run_crnn2(c, 0, dev, hash_case(c))
    if c["xb"] and _pair_config(c):
        assert route in {"pair", "wide"}, (c, route)


@gpu
@pytest.mark.parametrize("off", [1, 2])
@pytest.mark.parametrize("c", CRNN2_CASES[1::4], ids=case_id)
def test_crnn_step2_unaligned(dev, c, off):
    route = _run_crnn2(c, off, dev, hash_case(c))
    assert route == ("pair" if c["xb"] and _pair_config(c) else "general_elem"), (c, route)


# ================================================================== transpose conv and 1x1 conv (2-D)
def _run_tconv(c, off, dev, seed):
    from cine_hip import ops
    L = _L()
    n, cin, cout, h, w = c["n"], c["cin"], c["cout"], c["h"], c["w"]
    x = _src(seed, (n, cin, h, w))
    p = records(x, min(c["rec"], h * w)) if c["mode"] else None
    W1, W2 = _rand(seed + 1, cin, cout, 2, 2) / cin ** 0.5, _rand(seed + 2, cin, cout, 2, 2) / cin ** 0.5
    split = _split_of(c["split"], n)
    want = ref_conv(src_input(x, c["mode"], c["eps"], c["slope"], (h, w)), (W1, W2), None, n if split is None else split, kind="tconv")
    wp1, wp2 = ops.pack_tconv2x2(W1.to(dev)), ops.pack_tconv2x2(W2.to(dev))
    xd, pd = view_at(x, off, dev), (p.to(dev) if p is not None else None)
    nrec = L.cine_conv_stat_partials(cout, h, w, 1)

    def outs():
        return {"y": Guarded((n, cout, 2 * h, 2 * w), off, dev, torch.full((n, cout, 2 * h, 2 * w), NAN)),
                "part": Guarded((n, cout, nrec, 3), off, dev, torch.full((n, cout, nrec, 3), NAN))}

    def call(o):
        return L.cine_tconv2x2_in(xd.data_ptr(), _p(pd), 0 if pd is None else pd.shape[2], c["mode"], wp1.data_ptr(),
                                  None if split is None else wp2.data_ptr(), split or 0, o["y"].ptr(), o["part"].ptr(), n, cin, cout, h, w,
                                  c["eps"], c["slope"], _stream())
    o, route = _run("cine_tconv2x2_in", call, outs, case_id(c))
    _check_pin("tconv", c, off, route)
    _check_y("cine_tconv2x2_in", o["y"], want, (case_id(c), off))
    _check_records("cine_tconv2x2_in", o["part"], o["y"], 4 * h * w, (case_id(c), off))
    return route


@gpu
@pytest.mark.parametrize("c", TCONV_CASES, ids=case_id)
def test_tconv2x2_sweep(dev, c):
    route = _run_tconv(c, 0, dev, hash_case(c))
    if (c["cin"], c["cout"], c["w"]) in TCONV_PLANE_SHAPES and c["h"] % 2 == 0:
        assert route == "tconv_plane", (c, route)


@gpu
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("c", TCONV_CASES[::5], ids=case_id)
def test_tconv2x2_unaligned(dev, c, off):
    assert _run_tconv(c, off, dev, hash_case(c)) == "general_elem", c


def _run_c1(c, off, dev, seed):
    from cine_hip import ops
    L = _L()
    n, cin, cout, h, w = c["n"], c["cin"], c["cout"], c["h"], c["w"]
    x = _src(seed, (n, cin, h, w))
    p = records(x, min(c["rec"], h * w)) if c["mode"] else None
    W1, W2 = _rand(seed + 1, cout, cin) / cin ** 0.5, _rand(seed + 2, cout, cin) / cin ** 0.5
    b1, b2 = _rand(seed + 3, cout), _rand(seed + 4, cout)
    split = _split_of(c["split"], n)
    want = ref_conv(src_input(x, c["mode"], c["eps"], c["slope"], (h, w)), (W1[..., None, None], W2[..., None, None]), (b1, b2),
                    n if split is None else split)
    wp1, wp2 = ops.pack_conv1x1(W1.to(dev)), ops.pack_conv1x1(W2.to(dev))
    b1d, b2d = b1.to(dev), b2.to(dev)
    xd, pd = view_at(x, off, dev), (p.to(dev) if p is not None else None)

    def outs():
        return {"y": Guarded((n, cout, h, w), off, dev, torch.full((n, cout, h, w), NAN))}

    def call(o):
        two = split is not None
        return L.cine_conv1x1_bias(xd.data_ptr(), _p(pd), 0 if pd is None else pd.shape[2], c["mode"], wp1.data_ptr(), b1d.data_ptr(),
                                   wp2.data_ptr() if two else None, b2d.data_ptr() if two else None, split if two else n, o["y"].ptr(),
                                   n, cin, cout, h, w, c["eps"], c["slope"], _stream())
    stream = cout <= 4 and (h * w) % 4 == 0 and off == 0          # conv1x1_stream_kernel: <= 4 outputs, float4 pixel groups, aligned
    launches = 2 if not stream and split is not None and 0 < split < n else 1
    o, route = _run("cine_conv1x1_bias", call, outs, case_id(c), launches)
    _check_pin("c1", c, off, route)
    _check_y("cine_conv1x1_bias", o["y"], want, (case_id(c), off))
    assert (route == "stream1x1") == stream, (c, route)
    return route


@gpu
@pytest.mark.parametrize("c", C1_CASES, ids=case_id)
def test_conv1x1_bias_sweep(dev, c):
    _run_c1(c, 0, dev, hash_case(c))


@gpu
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("c", C1_CASES[::4], ids=case_id)
def test_conv1x1_bias_unaligned(dev, c, off):
    assert _run_c1(c, off, dev, hash_case(c)) == "general_elem", c


# ================================================================== volumes
def _run_vol(c, off, dev, seed):
    from cine_hip import ops
    L = _L()
    n, d, h, w, cout = c["n"], c["d"], c["h"], c["w"], c["cout"]
    e0, e1 = vol_exts(c)
    x0 = _src(seed, (n, c["c0"]) + e0)
    x1 = _src(seed + 1, (n, c["c1"]) + e1) if c["c1"] else None
    p0 = records(x0, min(c["rec"], int(np.prod(e0)))) if c["mode0"] else None
    p1 = records(x1, min(c["rec"], int(np.prod(e1)))) if x1 is not None and c["mode1"] else None
    srcs = [(x0, c["mode0"])] + ([(x1, c["mode1"])] if x1 is not None else [])
    inp = conv_input(c, srcs, (d, h, w))
    cin = inp.shape[1]
    W = _rand(seed + 2, cout, cin, 3, 3, 3) / (27 * cin) ** 0.5
    b = _rand(seed + 3, cout) if c["bias"] else None
    ad = _rand(seed + 4, n, cout, d, h, w) if c["addend"] else None
    want = ref_conv(inp, (W, W), (b, b), n, ad, c["relu"])
    del inp
    wp = ops._pack("c27", W.to(dev))
    x0d, x1d = view_at(x0, off, dev), (view_at(x1, off, dev) if x1 is not None else None)
    p0d, p1d = (p0.to(dev) if p0 is not None else None), (p1.to(dev) if p1 is not None else None)
    bd, add = (b.to(dev) if b is not None else None), (view_at(ad, off, dev) if ad is not None else None)
    nrec = L.cine_conv_stat_partials3d(cout, d, h, w, 0)
    e1 = e1 or (0, 0, 0)

    def outs():
        o = {"y": Guarded((n, cout, d, h, w), off, dev, torch.full((n, cout, d, h, w), NAN))}
        if c["party"]:
            o["part"] = Guarded((n, cout, nrec, 3), off, dev, torch.full((n, cout, nrec, 3), NAN))
        return o

    def call(o):
        return L.cine_conv3d_in(x0d.data_ptr(), _p(p0d), 0 if p0d is None else p0d.shape[2], c["c0"], c["mode0"], *e0,
                                _p(x1d), _p(p1d), 0 if p1d is None else p1d.shape[2], c["c1"], c["mode1"] if c["c1"] else 0, *e1,
                                wp.data_ptr(), _p(bd), _p(add), int(c["relu"]), o["y"].ptr(), o["part"].ptr() if "part" in o else None,
                                n, cout, d, h, w, c["eps"], c["slope"], _stream())
    o, route = _run("cine_conv3d_in", call, outs, case_id(c))
    _check_pin("vol", c, off, route)
    _check_y("cine_conv3d_in", o["y"], want, (case_id(c), off))
    if c["party"]:
        _check_records("cine_conv3d_in", o["part"], o["y"], d * h * w, (case_id(c), off))
    return route


def vol_routes(c):
    """The routes cine_conv3d_in can take for a case whatever its alignment: the coarse kernel on its shapes, the V3 form (column-tile
    kernel, or the general kernel's vectorised staging) where conv3d_v3_ok, else the 27-tap configurations (vectorised row pieces, but
    element-wise staging on 2-wide tiles)."""
    if coarse_shape(rows16(c["cout"]), c["h"], c["w"], c["d"]):
        return {"coarse"}
    if conv3d_v3_ok(c, *vol_exts(c)):
        return {"wide_v3", "general_vec"}
    return {"general_vec"} if c["w"] > 2 else {"general_elem"}


@gpu
@pytest.mark.parametrize("c", VOL_CASES, ids=case_id)
def test_conv3d_sweep(dev, c):
    route = _run_vol(c, 0, dev, hash_case(c))
    assert route in vol_routes(c), (c, route)


@gpu
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("c", VOL_CASES[::6], ids=case_id)
def test_conv3d_unaligned(dev, c, off):
    """Volumes stage rows with 4-byte aligned loads: misaligned pointers keep the V3 and 27-tap vectorised staging and lose the
    column-tile kernel."""
    route = _run_vol(c, off, dev, hash_case(c))
    assert route in vol_routes(c) - {"wide_v3"}, (c, route)


def _run_tvol(c, off, dev, seed, tconv):
    from cine_hip import ops
    L = _L()
    n, d, h, w, cin, cout = c["n"], c["d"], c["h"], c["w"], c["cin"], c["cout"]
    x = _src(seed, (n, cin, d, h, w))
    p = records(x, min(c["rec"], d * h * w)) if c["mode"] else None
    inp = src_input(x, c["mode"], c["eps"], c["slope"], (d, h, w))
    if tconv:
        W = _rand(seed + 1, cin, cout, 2, 2, 2) / cin ** 0.5
        want = ref_conv(inp, (W, W), None, n, kind="tconv")
        wp = ops._pack("tc3", W.to(dev))
        yshape = (n, cout, 2 * d, 2 * h, 2 * w)
        nrec = L.cine_conv_stat_partials3d(cout, d, h, w, 1)
    else:
        W = _rand(seed + 1, cout, cin) / cin ** 0.5
        b = _rand(seed + 2, cout)
        want = ref_conv(inp, (W[..., None, None, None],) * 2, (b, b), n)
        wp = ops.pack_conv1x1(W.to(dev))
        bd = b.to(dev)
        yshape = (n, cout, d, h, w)
    xd, pd = view_at(x, off, dev), (p.to(dev) if p is not None else None)
    npx = 0 if pd is None else pd.shape[2]

    def outs():
        o = {"y": Guarded(yshape, off, dev, torch.full(yshape, NAN))}
        if tconv:
            o["part"] = Guarded((n, cout, nrec, 3), off, dev, torch.full((n, cout, nrec, 3), NAN))
        return o

    def call(o):
        if tconv:
            return L.cine_tconv3d_in(xd.data_ptr(), _p(pd), npx, c["mode"], wp.data_ptr(), o["y"].ptr(), o["part"].ptr(), n, cin, cout, d, h, w,
                                     c["eps"], c["slope"], _stream())
        return L.cine_conv1x1x1_bias(xd.data_ptr(), _p(pd), npx, c["mode"], wp.data_ptr(), bd.data_ptr(), o["y"].ptr(), n, cin, cout, d, h, w,
                                     c["eps"], c["slope"], _stream())
    what = "cine_tconv3d_in" if tconv else "cine_conv1x1x1_bias"
    o, route = _run(what, call, outs, case_id(c))
    _check_y(what, o["y"], want, (case_id(c), off))
    if tconv:
        _check_records(what, o["part"], o["y"], 8 * d * h * w, (case_id(c), off))
    # vol1x1_fast_ok: W > 8 -> the 16-wide configurations with volume addressing and vectorised staging (no 16-byte check)
    assert route == ("general_vec" if w > 8 else "general_elem"), (c, route)
    return route


@gpu
@pytest.mark.parametrize("c", TVOL_CASES, ids=case_id)
def test_tconv3d_sweep(dev, c):
    _run_tvol(c, 0, dev, hash_case(c), True)


@gpu
@pytest.mark.parametrize("c", C111_CASES, ids=case_id)
def test_conv1x1x1_bias_sweep(dev, c):
    _run_tvol(c, 0, dev, hash_case(c), False)


@gpu
@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("kind,c", [("tconv", c) for c in TVOL_CASES[::5]] + [("c111", c) for c in C111_CASES[::5]],
                         ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_vol1x1_unaligned(dev, kind, c, off):
    _run_tvol(c, off, dev, hash_case(c), kind == "tconv")


# ================================================================== statistics kernels
@gpu
@pytest.mark.parametrize("case", POOL_CASES + [FULL_POOL], ids=lambda t: "x".join(map(str, t)))
def test_pool3d_act(dev, case):
    """cine_pool3d_act against avg_pool3d(LeakyReLU(InstanceNorm3d(x)), 2) in float64 with floors; NaN prefill, guards, repeat bits."""
    L = _L()
    planes, d, h, w, k, slope, eps, off = case
    x = _src(hash_case(dict(p=planes, d=d, h=h, w=w)), (1, planes, d, h, w))
    p = records(x, k)[0]
    want = src_input(x, 2, eps, slope, (d // 2, h // 2, w // 2))[0]
    xd, pd = view_at(x[0], off, dev), p.to(dev)
    shp = (planes, d // 2, h // 2, w // 2)
    vec = w % 8 == 0 and off == 0               # the float4 kernel: rows of whole 8-float pieces, 16-byte aligned x and y
    ys = []
    for rep in range(2):
        y = Guarded(shp, off, dev, torch.full(shp, NAN))
        before = [L.cine_diag_counter(k_, 0) for k_ in (D_POOL3D_VEC, D_POOL3D_SCALAR)]
        assert L.cine_pool3d_act(xd.data_ptr(), pd.data_ptr(), k, y.ptr(), planes, d, h, w, eps, slope, _stream()) == 0
        torch.cuda.synchronize()
        moved = [L.cine_diag_counter(k_, 0) - b for k_, b in zip((D_POOL3D_VEC, D_POOL3D_SCALAR), before)]
        assert moved == ([1, 0] if vec else [0, 1]), (case, moved)
        assert y.intact()
        ys.append(y.t.cpu())
    assert _same_bits(ys[0], ys[1])
    _check_y("cine_pool3d_act", ys[0], want, case)


@gpu
@pytest.mark.parametrize("planes,pe", PARTIALS_CASES)
def test_instnorm_kernels(dev, planes, pe):
    """cine_instnorm_partials (wave kernel <= 8192 elements, block kernel above), _finalize, _merge and _lrelu_apply against float64."""
    L = _L()
    x = _src(planes * 100_003 + pe, (1, planes, pe))
    xd = x[0].to(dev)
    part = Guarded((planes, 1, 3), 0, dev, torch.full((planes, 1, 3), NAN))
    assert L.cine_instnorm_partials(xd.data_ptr(), part.ptr(), planes, pe, _stream()) == 0
    torch.cuda.synchronize()
    assert part.intact()
    _check_records("cine_instnorm_partials", part.t.cpu()[None], x, pe, (planes, pe))
    x64 = x[0].double()
    mean, var = x64.mean(-1), x64.var(-1, unbiased=False)
    for k, eps, slope in ((1, 1e-5, 0.2), (5, 1e-3, 0.0), (17, 1e-5, 1.0), (64, 1e-3, 0.2)):
        k = min(k, pe)
        rec = records(x, k)[0].to(dev)
        st = Guarded((planes, 2), 0, dev, torch.full((planes, 2), NAN))
        mg = Guarded((planes, 3), 0, dev, torch.full((planes, 3), NAN))
        y = Guarded((planes, pe), 1, dev, torch.full((planes, pe), NAN))
        assert L.cine_instnorm_finalize(rec.data_ptr(), st.ptr(), planes, k, eps, _stream()) == 0
        assert L.cine_instnorm_merge(rec.data_ptr(), mg.ptr(), planes, k, _stream()) == 0
        assert L.cine_instnorm_lrelu_apply(xd.data_ptr(), rec.data_ptr(), k, y.ptr(), planes, pe, eps, slope, _stream()) == 0
        torch.cuda.synchronize()
        assert st.intact() and mg.intact() and y.intact()
        WORST.record("cine_instnorm_finalize", rel_err(st.t.cpu(), torch.stack([mean, (var + eps).rsqrt()], -1)), BAR, (planes, pe, k))
        _check_records("cine_instnorm_merge", mg.t.cpu()[None, :, None], x, pe, (planes, pe, k))
        # (error relative to the terms x * rstd the kernel forms: a one-element plane normalises to exactly 0, which the
        # x * rstd - mean * rstd form meets only to their rounding)
        want = in_act(x, eps, slope)[0]
        got = y.t.cpu()
        assert not torch.isnan(got).any()
        scale = max(float(want.abs().max()), float((x64.abs() * (var + eps).rsqrt()[:, None]).max()))
        WORST.record("cine_instnorm_lrelu_apply", float((got - want).abs().max()) / scale, BAR, (planes, pe, k, eps, slope))


# ================================================================== full-size layers and routes
@gpu
@pytest.mark.parametrize("layer", FULL_LAYERS, ids=lambda t: t[0].replace(" ", "_"))
def test_full_size_layer_route(dev, layer):
    """The production layer shapes take the kernel the committed rocprofv3 profiles show for them, and meet the bar: a dispatch change
    that moves a hot layer onto another kernel fails here."""
    name, kind, c, expect = layer
    seed = hash_case(c)
    if kind == "conv":
        route = _run_conv(c, 0, dev, seed)[2]
    elif kind == "tconv":
        route = _run_tconv(c, 0, dev, seed)
    elif kind == "c1":
        route = _run_c1(c, 0, dev, seed)
    elif kind == "crnn":
        route = _run_crnn(c, 0, dev, seed)
    elif kind == "vol":
        route = _run_vol(c, 0, dev, seed)
    else:
        route = _run_tvol(c, 0, dev, seed, kind == "tvol")
    assert route == expect, (name, route)


@gpu
def test_sweep_reaches_every_route(dev):
    """Every forward-convolution route counter moves, on its own: one hand-placed case per route (the same cases the sweeps pin),
    with every per-case check, independent of which other tests ran before."""
    by = {}                                   # route -> its cheapest pinned case
    for (kind, cid), route in sorted(pinned().items(), key=lambda kv: _pin_cost(kv[0]), reverse=True):
        by[route] = (kind, _pinned_case(kind, cid))
    seen = set()
    for route, (kind, c) in sorted(by.items()):
        seed = hash_case(c)
        if kind == "conv":
            got = _run_conv(c, 0, dev, seed, _wav_data(c, seed) if c["mode0"] >= 3 else None)[2]
        elif kind == "crnn2":
            got = _run_crnn2(c, 0, dev, seed)
        elif kind == "tconv":
            got = _run_tconv(c, 0, dev, seed)
        elif kind == "c1":
            got = _run_c1(c, 0, dev, seed)
        else:
            got = _run_vol(c, 0, dev, seed)
        assert got == route, (kind, c, got)
        seen.add(got)
    c = min((c for c, r in CONV_PINNED if r == "plane"), key=lambda c: _conv_macs(c, c["c0"] + c["c1"]) * c["n"])
    seen.add(_run_conv(c, 1, dev, hash_case(c))[2])          # the same pointers 4 bytes past alignment: the element-wise staging
    assert seen == set(ROUTES), set(ROUTES) - seen


def _pinned_case(kind, cid):
    lists = {"conv": [c for c, _ in CONV_PINNED] + [_wav_case(c) for c, _ in WAV_PINNED], "crnn2": [c for c, _ in CRNN2_PINNED],
             "tconv": [c for c, _ in TCONV_PINNED], "c1": [c for c, _ in C1_PINNED], "vol": [c for c, _ in VOL_PINNED]}
    return next(c for c in lists[kind] if case_id(c) == cid)


def _pin_cost(key):
    """Multiply-adds of a pinned case's float64 reference: the cheapest case of each route represents it."""
    c = _pinned_case(*key)
    if key[0] == "vol":
        return _conv_macs(c, c["c0"] + c["c1"], 27) * c["n"]
    if key[0] in ("tconv", "c1"):
        return c["h"] * c["w"] * c["cin"] * c["cout"] * c["n"]
    if key[0] == "crnn2":
        return c["h"] * c["w"] * c["c"] * c["c"] * c["n"]
    return _conv_macs(c, c["c0"] + c["c1"]) * c["n"]


# ================================================================== argument validation
def _einval(call, g, fill):
    L = _L()
    before = _counts(L)
    code = call()
    torch.cuda.synchronize()
    assert code == CINE_EINVAL, code
    assert _counts(L) == before, "a rejected call launched"
    assert g.intact() and bool((g.t == fill).all()), "a rejected call wrote its output"
    assert L.cine_last_error().decode(), "no error message"


@gpu
def test_bad_arguments_are_rejected(dev):
    """CINE_EINVAL, nothing launched or written, an error message: slopes outside [0, 1], bad modes, an IWT source of 4k + 2 channels,
    added sources of different channel counts, n > 65535.  Every buffer is real and sized for what a call without the check would read
    and write, so that a missing check launches on valid memory."""
    from cine_hip import ops
    L = _L()
    s = _stream()
    n, c, h, w = 2, 8, 8, 8
    x = torch.randn(n, c, h, w, device=dev)
    part = ops.instnorm_partials(x)
    wp = ops.pack_conv3x3(torch.randn(c, 4 * c, 3, 3, device=dev))       # room for a space-to-depth (mode 5) source of 4 c channels
    wt = ops.pack_tconv2x2(torch.randn(c, c, 2, 2, device=dev))
    w1 = ops.pack_conv1x1(torch.randn(c, c, device=dev))
    w27 = ops._pack("c27", torch.randn(c, c, 3, 3, 3, device=dev))
    b = torch.zeros(c, device=dev)
    y = Guarded((n, c, 2 * h, 2 * w), 0, dev, torch.full((n, c, 2 * h, 2 * w), 7.0))
    py = torch.empty(n, c, 64, 3, device=dev)

    def c3(slope=0.2, mode0=1, c0=c, h0=h, w0=w, x1=None, c1=0, add=0):
        return lambda: L.cine_conv3x3_ex(x.data_ptr(), part.data_ptr(), 1, c0, mode0, h0, w0, _p(x1), part.data_ptr(), 1, c1, 0, h, w, add,
                                         wp.data_ptr(), None, None, 0, y.ptr(), py.data_ptr(), n, c, h, w, 1e-5, slope, s)
    for slope in (-0.1, 1.5, NAN):
        _einval(c3(slope=slope), y, 7.0)
    _einval(c3(mode0=5), y, 7.0)
    _einval(c3(mode0=4, c0=6, h0=4, w0=4), y, 7.0)                        # IWT of 6 channels
    _einval(c3(x1=x, c1=4, add=1), y, 7.0)                                # 8 channels + 4 channels, added
    _einval(lambda: L.cine_tconv2x2_in(x.data_ptr(), part.data_ptr(), 1, 2, wt.data_ptr(), None, 0, y.ptr(), py.data_ptr(), n, c, c, h, w,
                                       1e-5, 0.2, s), y, 7.0)
    _einval(lambda: L.cine_tconv2x2_in(x.data_ptr(), part.data_ptr(), 1, 1, wt.data_ptr(), None, 0, y.ptr(), py.data_ptr(), n, c, c, h, w,
                                       1e-5, -1.0, s), y, 7.0)
    _einval(lambda: L.cine_conv1x1_bias(x.data_ptr(), part.data_ptr(), 1, 2, w1.data_ptr(), b.data_ptr(), None, None, n, y.ptr(), n, c, c,
                                        h, w, 1e-5, 0.2, s), y, 7.0)
    xv = x.view(n, c, 2, h // 2, w)
    _einval(lambda: L.cine_conv3d_in(xv.data_ptr(), part.data_ptr(), 1, c, 3, 2, h // 2, w, None, None, 0, 0, 0, 0, 0, 0, w27.data_ptr(),
                                     None, None, 0, y.ptr(), py.data_ptr(), n, c, 2, h // 2, w, 1e-5, 0.2, s), y, 7.0)
    _einval(lambda: L.cine_conv3d_in(xv.data_ptr(), part.data_ptr(), 1, c, 1, 2, h // 2, w, None, None, 0, 0, 0, 0, 0, 0, w27.data_ptr(),
                                     None, None, 0, y.ptr(), py.data_ptr(), n, c, 2, h // 2, w, 1e-5, 2.0, s), y, 7.0)
    _einval(lambda: L.cine_tconv3d_in(xv.data_ptr(), part.data_ptr(), 1, 2, w27.data_ptr(), y.ptr(), py.data_ptr(), n, c, 1, 2, h // 2, w,
                                      1e-5, 0.2, s), y, 7.0)
    _einval(lambda: L.cine_conv1x1x1_bias(xv.data_ptr(), part.data_ptr(), 1, 2, w1.data_ptr(), b.data_ptr(), y.ptr(), n, c, c, 2, h // 2, w,
                                          1e-5, 0.2, s), y, 7.0)
    _einval(lambda: L.cine_pool3d_act(xv.data_ptr(), part.data_ptr(), 1, y.ptr(), n * c, 2, h // 2, w, 1e-5, 1.01, s), y, 7.0)
    # n = 65536 one-pixel planes of one channel, every buffer sized for all of them
    big = 65536
    xb = torch.randn(big, 1, 1, 1, device=dev)
    pb = ops.instnorm_partials(xb.view(big, 1, 1, 1))
    wb = ops.pack_conv3x3(torch.randn(1, 1, 3, 3, device=dev))
    w1b = ops.pack_conv1x1(torch.randn(1, 1, device=dev))
    yb = Guarded((big, 1, 1, 1), 0, dev, torch.full((big, 1, 1, 1), 7.0))
    pyb = torch.empty(big, 1, L.cine_conv_stat_partials(1, 1, 1, 0), 3, device=dev)
    _einval(lambda: L.cine_conv3x3_in(xb.data_ptr(), pb.data_ptr(), 1, 1, 1, 1, 1, None, None, 0, 0, 0, 0, 0, wb.data_ptr(), None, 0,
                                      yb.ptr(), pyb.data_ptr(), big, 1, 1, 1, 1e-5, 0.2, s), yb, 7.0)
    _einval(lambda: L.cine_conv1x1_bias(xb.data_ptr(), pb.data_ptr(), 1, 1, w1b.data_ptr(), b.data_ptr(), None, None, big, yb.ptr(), big, 1,
                                        1, 1, 1, 1e-5, 0.2, s), yb, 7.0)
    _einval(lambda: L.cine_conv3d_in(xb.data_ptr(), pb.data_ptr(), 1, 1, 1, 1, 1, 1, None, None, 0, 0, 0, 0, 0, 0,
                                     ops._pack("c27", torch.randn(1, 1, 3, 3, 3, device=dev)).data_ptr(), None, None, 0, yb.ptr(),
                                     pyb.data_ptr(), big, 1, 1, 1, 1, 1e-5, 0.2, s), yb, 7.0)
