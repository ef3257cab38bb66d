"""The yardstick of the U-Net launch-sequence sweep (test_unet_sequences.py on the GPU, test_unet_sequences_cpu.py without one):
oracle/regularisers.Unet (2-D, and dims = 3) in float64 under autograd, on seeded inputs and synth.fill_parameters_ weights, for one network or
two with n / 2 samples each, with the LeakyReLU slope set on every module and optionally fixed Dropout multipliers in the oracle's Dropout
slots; the same oracle in float32 on the CPU, whose error against float64 sets each tensor's bar; the case table; the pointer arrays
cine_unet2d_* / cine_unet3d_* take, built through the C ABI's pack entry points alone from what include/cine_hip.h says; and the calls.
A plain module, not a conftest."""
import copy
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import torch

from kernel_sweep import BAR, BAR_CAP

SLOPE = 0.2
KMERGE = 12                 # csrc/unet.hip kMergeMin: a 2-D inference layer with this many records per plane has them merged once
# id -> (n, in, out, chans, pools, h, w).  What each case is there for; the record counts are asserted through cine_conv_stat_partials by
# test_unet_sequences_cpu.py::test_record_counts_of_the_table
CASES = {
    # odd extent at every pool; the up-path zero pad on both axes at every level
    "odd-every-level": (1, 2, 2, 5, 3, 23, 19),
    # chans 1, in = out = 1; the 2-channel concat gradient
    "one-channel": (2, 1, 1, 1, 2, 21, 11),
    # ragged 16-channel chunks; in != out != 2
    "ragged-18": (1, 3, 5, 18, 2, 27, 13),
    # in_ch > 16 (the max(in_ch, 16) sizing of the backward's gradient buffers); out_ch 17; ragged last 16-pixel tile
    "wide-in": (1, 20, 17, 4, 1, 9, 33),
    # level-0 conv 12 records and its transpose conv 12, both merged; level 1 (48 x 28: 3) unmerged: a merged and an unmerged producer feed one concat
    "merge-l0": (2, 2, 2, 4, 2, 56, 96),
    # the same with odd sizes: up 56 x 98 under skip 57 x 99
    "merge-odd": (1, 2, 2, 4, 2, 57, 99),
    # 32-row tiling
    "merge-32rows": (1, 2, 2, 20, 1, 54, 98),
    # conv_plane.hip widths 16 / 8 / 4 / 2; n = 3 for uneven branch cuts
    "plane16": (3, 2, 2, 16, 3, 40, 16),
    # level 2 = 64 rows on 26 x 26: conv_coarse.hip's record count; level 0 merges
    "coarse2d": (1, 2, 2, 16, 2, 104, 104),
    # pools = 6; odd at four levels; bottleneck 3 x 5 (a bottleneck of <= 6 elements leaves the float32 oracle itself past BAR_CAP / 2)
    "six-pools": (1, 2, 2, 1, 6, 200, 330),
    # both ends of the accepted slope range run on this shape
    "slope": (2, 2, 2, 5, 2, 21, 11),
}
# id -> (n, in, out, chans, pools, d, h, w)
CASES3 = {
    # odd extents on all three axes: the depth crop and the in-plane crop of the zero-padded transpose-conv output
    "odd3d": (1, 2, 2, 4, 2, 5, 13, 11),
    # two samples, in != out, chans 3
    "two3d": (2, 3, 1, 3, 1, 7, 9, 11),
    # 180 records per channel at level 0; rows of whole float4 pieces
    "wide3d": (1, 2, 2, 2, 1, 6, 40, 36),
    # level 1 (32 channels on 2 x 6 x 20) gets its pooled input materialised, level 2 (64 channels on 1 x 3 x 10) runs on conv_coarse.hip, which pools
    # on load: both routes of cine_conv3d_pools_on_load in one network.  (6 x 24 x 24, the shape first written down for this case, never pools on
    # load: its 64-channel level is 6 wide and conv_coarse.hip takes volumes wider than 8 only.)
    "coarse3d": (1, 2, 2, 16, 2, 4, 12, 40),
    # three pools; depth 9 -> 4 -> 2 -> 1
    "three3d": (1, 2, 2, 2, 3, 9, 17, 24),
}
ALL = {**CASES, **CASES3}
SEEDS = {k: 300 + 7 * i for i, k in enumerate(ALL)}
DROP_P = 0.25
# (case, slope, sets, drop, n): every run of the sweep.  n None = the table's
RUNS = ([(k, SLOPE, 1, False, None) for k in ALL if k != "slope"] + [("slope", 0.0, 1, False, None), ("slope", 1.0, 1, False, None)]
        + [("odd-every-level", SLOPE, 2, False, 2), ("plane16", SLOPE, 2, False, 6), ("merge-l0", SLOPE, 2, False, None)]
        + [("odd-every-level", SLOPE, 1, True, None), ("merge-l0", SLOPE, 2, True, None), ("odd3d", SLOPE, 1, True, None)])


def run_id(r):
    k, slope, sets, drop, n = r
    return k + (f"-slope{slope:g}" if slope != SLOPE else "") + ("-2sets" if sets == 2 else "") + ("-drop" if drop else "") + (f"-n{n}" if n else "")


def is3d(case):
    return case in CASES3


def rel_l2(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def bar(e32):
    """The bar of one tensor of one run: twice the error of the float32 oracle against the float64 one, BAR at least and BAR_CAP at most
    (test_unet_sequences_cpu.py asserts that the cap never decides)."""
    return min(BAR_CAP, max(BAR, 2 * e32))


# ================================================================== the layer plan, restated from reference unet.py:73-125
def levels(case):
    """Per level 0..pools: (channels, extents) with extents (h, w) or (d, h, w)."""
    t = ALL[case]
    chans, pools, ext = t[3], t[4], t[5:]
    return [(chans << l, tuple(e >> l for e in ext)) for l in range(pools + 1)]


def conv_channels(case):
    """Output channels of the 4 pools + 2 3x3 convs in launch order (down path and bottleneck, then the up path from the coarsest level): the
    order of the Dropout multipliers' (n, ch) blocks."""
    lv = levels(case)
    P = len(lv) - 1
    return [lv[j // 2][0] for j in range(2 * P + 2)] + [lv[P - 1 - u][0] for u in range(P) for _ in range(2)]


def conv_slot(case, j):
    """The pointer-array slot of 3x3 conv j (launch order)."""
    P = ALL[case][4]
    if j < 2 * P + 2:
        return j
    u, k = divmod(j - 2 * P - 2, 2)
    return 2 * P + 2 + 3 * u + 1 + k


def drop_floats(case, n):
    return n * sum(conv_channels(case))


def kept_tensors(case, n):
    """(floats, channels, level, is_tconv) of every tensor the training forward keeps: per level two convs (down / bottleneck), per up level the
    transpose-conv output (twice the extents of the level below) and two convs."""
    lv = levels(case)
    P = len(lv) - 1
    out = []
    for l, (c, ext) in enumerate(lv):
        out += [(n * c * int(np.prod(ext)), c, l, False)] * 2
    for l in range(P):
        c, ext = lv[l]
        up = int(np.prod([2 * e for e in lv[l + 1][1]]))
        out += [(n * c * up, c, l, True)] + [(n * c * int(np.prod(ext)), c, l, False)] * 2
    return out


def records(L, case, l, tconv):
    """Statistics records per (sample, channel) of a conv output at level l / of the transpose conv that produces level l's `up` from level l + 1."""
    lv = levels(case)
    c = lv[l][0]
    ext = lv[l + 1][1] if tconv else lv[l][1]
    if is3d(case):
        return L.cine_conv_stat_partials3d(c, *ext, int(tconv))
    return L.cine_conv_stat_partials(c, *ext, int(tconv))


def merges(L, case):
    """True when a layer of the 2-D inference layout has its records merged once (and so is summed in another order than the training layout's)."""
    P = ALL[case][4]
    if is3d(case):
        return False
    return max([records(L, case, l, False) for l in range(P + 1)] + [records(L, case, l, True) for l in range(P)]) >= KMERGE


# ================================================================== the oracle
class Mult(torch.nn.Module):
    """Fixed Dropout multipliers (n, ch) in a Dropout2d / Dropout3d slot."""

    def __init__(self, m, dims):
        super().__init__()
        self.register_buffer("m", m.reshape(m.shape + (1,) * dims))

    def forward(self, v):
        return v * self.m


def blocks(net):
    """The ConvBlocks in launch order."""
    P = net.num_pool_layers
    return list(net.down_sample_layers) + [net.conv] + [net.up_conv[i] if i < P - 1 else net.up_conv[i][0] for i in range(P)]


def slots(net):
    """(kind, parameter) of one network in the order of the pointer arrays (include/cine_hip.h, cine_unet2d_forward): per down level and the
    bottleneck two 3x3 convs; per up level from the coarsest the transpose conv and two 3x3 convs; the final 1x1 conv's weight, then its bias."""
    seq = []
    for blk in list(net.down_sample_layers) + [net.conv]:
        seq += [("conv", blk.layers[0].weight), ("conv", blk.layers[4].weight)]
    for tc, blk in zip(net.up_transpose_conv, blocks(net)[net.num_pool_layers + 1:]):
        seq += [("tconv", tc.layers[0].weight), ("conv", blk.layers[0].weight), ("conv", blk.layers[4].weight)]
    fin = net.up_conv[-1][1]
    return seq + [("final", fin.weight), ("bias", fin.bias)]


def make_net(case, seed, slope=SLOPE):
    from cine_hip import synth
    from oracle import regularisers as O
    t = ALL[case]
    net = O.Unet(chans=t[3], num_pool_layers=t[4], in_chans=t[1], out_chans=t[2], drop_prob=0.0, dims=3 if is3d(case) else 2)
    synth.fill_parameters_(net, seed, keep=())
    for m in net.modules():
        if isinstance(m, torch.nn.LeakyReLU):
            m.negative_slope = slope
    return net.eval()


def make_multipliers(case, n, seed):
    """Multipliers 0, 1 and 1 / (1 - p) in cine_unet2d_forward_branches' layout; the first plane of the first conv is dropped."""
    rs = np.random.RandomState(seed)
    vals = np.array([0.0, 1.0, 1.0 / (1.0 - DROP_P)], dtype=np.float32)
    m = vals[rs.choice(3, size=drop_floats(case, n), p=[0.25, 0.25, 0.5])]
    m[0] = 0.0
    assert all((m == v).any() for v in vals)
    return torch.from_numpy(m)


def with_multipliers(net, case, mult, n, rows):
    """A copy of the network with Mult modules holding rows `rows` of every conv's (n, ch) block."""
    net = copy.deepcopy(net)
    dims = 3 if is3d(case) else 2
    off, chs = 0, conv_channels(case)
    for bi, blk in enumerate(blocks(net)):
        for k, slot in enumerate((3, 7)):
            ch = chs[2 * bi + k]
            assert blk.layers[0 if k == 0 else 4].out_channels == ch
            blk.layers[slot] = Mult(mult[off:off + n * ch].view(n, ch)[rows].clone(), dims)
            off += n * ch
    assert off == mult.numel()
    return net


def _run(nets, x, gy, dtype):
    """y, gx and per network the slot gradients of sum(y gy), y = cat(net_k(x[k n / sets : (k + 1) n / sets])), in `dtype` on the CPU."""
    nets = [copy.deepcopy(nt).to(dtype) for nt in nets]
    xr = x.to(dtype).requires_grad_(True)
    per = x.shape[0] // len(nets)
    with torch.enable_grad():
        y = torch.cat([nt(xr[k * per:(k + 1) * per]) for k, nt in enumerate(nets)])
        (y * gy.to(dtype)).sum().backward()
    return y.detach(), xr.grad, [[p.grad for _, p in slots(nt)] for nt in nets]


@functools.lru_cache(maxsize=None)
def reference(case, slope=SLOPE, sets=1, drop=False, n=None):
    """One run of the sweep, computed once per process and shared (treat every tensor as read-only): float32 x, gy and networks, the float64
    results y, gx, grads[net][slot], e32 = the float32 oracle's relative L2 error against each of them (same nesting), and the Dropout
    multipliers `mult` (None without)."""
    t = ALL[case]
    n = t[0] if n is None else n
    assert n % sets == 0
    cin, cout, ext = t[1], t[2], t[5:]
    seed = SEEDS[case]
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((n, cin) + ext).astype(np.float32))
    gy = torch.from_numpy(rs.standard_normal((n, cout) + ext).astype(np.float32))
    nets = [make_net(case, seed + 1 + k, slope) for k in range(sets)]
    mult = make_multipliers(case, n, seed + 5) if drop else None
    per = n // sets
    onets = nets if mult is None else [with_multipliers(nt, case, mult, n, slice(k * per, (k + 1) * per)) for k, nt in enumerate(nets)]
    y, gx, grads = _run(onets, x, gy, torch.float64)
    y32, gx32, grads32 = _run(onets, x, gy, torch.float32)
    e32 = SimpleNamespace(y=rel_l2(y32, y), gx=rel_l2(gx32, gx),
                          grads=[[rel_l2(a, b) for a, b in zip(g32, g64)] for g32, g64 in zip(grads32, grads)])
    return SimpleNamespace(case=case, slope=slope, sets=sets, x=x, gy=gy, nets=nets, y=y, gx=gx, grads=grads, e32=e32, mult=mult, n=n)


# ================================================================== the C ABI's operands
def flip_transpose(w):
    """A 3x3x3 weight with its taps flipped and (cout, cin) transposed: what cine_unet3d_backward's wdgrad packs with cine_pack_conv3d."""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


def pack_plan(net):
    """Per slot: ((forward pack entry point, view of the weight, n1, n2), (input-gradient pack entry point, view, n1, n2) | None), as
    include/cine_hip.h states them; the bias slot is (None, None): the parameter at its own address, NULL in the dgrad list."""
    three = getattr(net, "dims", 2) == 3
    ident = lambda w: w                                                         # noqa: E731
    plan = []
    for kind, p in slots(net):
        a, b = (int(p.shape[0]), int(p.shape[1])) if p.dim() > 1 else (0, 0)
        if kind == "bias":
            plan.append((None, None))
        elif not three:
            stem = {"conv": "conv3x3", "tconv": "tconv2x2", "final": "conv1x1"}[kind]
            plan.append(((f"cine_pack_{stem}", ident, a, b), (f"cine_pack_{stem}_dgrad", ident, a, b)))
        elif kind == "conv":                 # (cout, cin, 3, 3, 3); dgrad: the forward kernel on the flipped, transposed weight (cin rows)
            plan.append((("cine_pack_conv3d", ident, a, b), ("cine_pack_conv3d", flip_transpose, b, a)))
        elif kind == "tconv":                # (cin, cout, 2, 2, 2); dgrad: a 1x1x1 conv with cin rows over the 8 cout space-to-depth channels
            plan.append((("cine_pack_tconv3d", ident, a, b), ("cine_pack_conv1x1", lambda w: w.reshape(w.shape[0], -1), a, 8 * b)))
        else:                                # (out_ch, chans, 1, 1, 1); dgrad: the transposed matrix (chans rows)
            plan.append((("cine_pack_conv1x1", ident, a, b), ("cine_pack_conv1x1", lambda w: w.reshape(w.shape[0], -1).t().contiguous(), b, a)))
    return plan


def floats_fn(L, pack_name):
    stem = pack_name[len("cine_pack_"):]
    return getattr(L, f"cine_{stem}_packed_floats")


def ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


class DeviceNet:
    """One network's pointer lists on `dev`: `weights` and `wdgrad` (Python lists of addresses, None in wdgrad's bias slot)."""

    def __init__(self, net, dev):
        from cine_hip._lib import lib, check
        L = lib()
        st = torch.cuda.current_stream().cuda_stream
        self.params = [p for _, p in slots(net)]
        self.keep, self.weights, self.wdgrad = [], [], []
        for (kind, p), (fwd, dg) in zip(slots(net), pack_plan(net)):
            src = p.detach().float().to(dev).contiguous()
            self.keep.append(src)
            if fwd is None:
                self.weights.append(src.data_ptr()); self.wdgrad.append(None)
                continue
            for (name, view, n1, n2), dst in ((fwd, self.weights), (dg, self.wdgrad)):
                wv = view(src).contiguous()
                out = torch.zeros(floats_fn(L, name)(n1, n2), device=dev)
                check(getattr(L, name)(wv.data_ptr(), out.data_ptr(), n1, n2, st), name)
                self.keep += [wv, out]
                dst.append(out.data_ptr())
        torch.cuda.synchronize()

    def __len__(self):
        return len(self.params)


def dims(case, **over):
    """The scalar arguments of one call: the case's, with overrides."""
    t = ALL[case]
    a = dict(n=t[0], cin=t[1], cout=t[2], chans=t[3], pools=t[4], slope=SLOPE, nsets=1, three=is3d(case))
    a.update(dict(zip(("d", "h", "w") if is3d(case) else ("h", "w"), t[5:])))
    a.update(over)
    return SimpleNamespace(**a)


def _shape(a):
    return (a.n, a.d, a.h, a.w) if a.three else (a.n, a.h, a.w)


def ws_sizes(L, a):
    """(inference, training, backward) workspace bytes of a call's dims."""
    t = _shape(a) + (a.cin, a.cout, a.chans, a.pools)
    if a.three:
        return L.cine_unet3d_ws_bytes(*t), L.cine_unet3d_train_ws_bytes(*t), L.cine_unet3d_backward_ws_bytes(*t)
    return L.cine_unet2d_ws_bytes(*t), L.cine_unet2d_train_ws_bytes(*t), L.cine_unet2d_backward_ws_bytes(*t)


def branch_ws(L, a, nbranch, train):
    return L.cine_unet2d_branch_ws_bytes(a.n, a.h, a.w, a.cin, a.cout, a.chans, a.pools, a.nsets, nbranch, train)


def call_forward(L, a, x, y, weights, ws, ws_bytes, stream, train=False, drop=None, use_drop_entry=False):
    """cine_unet2d_forward / _forward_train, cine_unet3d_forward / _forward_train / _forward_train_drop."""
    tail = (a.cin, a.cout, a.chans, a.pools, a.slope, ws, ws_bytes)
    if a.three:
        if drop is not None or use_drop_entry:
            return L.cine_unet3d_forward_train_drop(x, y, weights, *_shape(a), *tail, drop, stream)
        return (L.cine_unet3d_forward_train if train else L.cine_unet3d_forward)(x, y, weights, *_shape(a), *tail, stream)
    return (L.cine_unet2d_forward_train if train else L.cine_unet2d_forward)(x, y, weights, a.nsets, *_shape(a), *tail, stream)


def call_branches(L, a, x, y, weights, ws, ws_bytes, stream, side, nside, train, drop):
    return L.cine_unet2d_forward_branches(x, y, weights, a.nsets, a.n, a.h, a.w, a.cin, a.cout, a.chans, a.pools, a.slope, ws, ws_bytes, stream,
                                          side, nside, train, drop)


def call_backward(L, a, x, gy, wdgrad, grads, fwd_ws, fwd_bytes, ws, ws_bytes, gx, stream, drop=None, use_drop_entry=False):
    """cine_unet2d_backward / _backward_drop, cine_unet3d_backward / _backward_drop."""
    tail = (a.cin, a.cout, a.chans, a.pools, a.slope, fwd_ws, fwd_bytes, ws, ws_bytes, gx)
    sets = () if a.three else (a.nsets,)
    stem = "cine_unet3d_backward" if a.three else "cine_unet2d_backward"
    if drop is not None or use_drop_entry:
        return getattr(L, stem + "_drop")(x, gy, wdgrad, grads, *sets, *_shape(a), *tail, drop, stream)
    return getattr(L, stem)(x, gy, wdgrad, grads, *sets, *_shape(a), *tail, stream)


EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
REFUSAL_CASE, REFUSAL_CASE3 = "slope", "odd3d"          # 2-D refusals run with two sets (n = 2)
NAN = float("nan")
# (what, overrides of the dims, code, entry points: f forward, t forward_train, r forward_branches, b backward (both forms); d the 3-D _drop forms ride
# with t and b).  Every one returns before the first launch.
REFUSALS = [
    ("slope -0.1", dict(slope=-0.1), EINVAL, "ftrb"), ("slope 1.1", dict(slope=1.1), EINVAL, "ftrb"), ("slope NaN", dict(slope=NAN), EINVAL, "ftrb"),
    ("nsets 0", dict(nsets=0), EINVAL, "ftrb2"), ("nsets 3", dict(nsets=3, n=3), EINVAL, "ftrb2"), ("n % nsets", dict(n=3), EINVAL, "ftrb2"),
    ("n 0", dict(n=0), EINVAL, "ftrb"), ("n -2", dict(n=-2), EINVAL, "ftrb"), ("h 0", dict(h=0), EINVAL, "ftrb"), ("w -1", dict(w=-1), EINVAL, "ftrb"),
    ("d 0", dict(d=0), EINVAL, "ftb3"),
    ("in_ch 0", dict(cin=0), EINVAL, "ftrb"), ("out_ch 0", dict(cout=0), EINVAL, "ftrb"), ("in_ch -1", dict(cin=-1), EINVAL, "ftrb"),
    ("out_ch -1", dict(cout=-1), EINVAL, "ftrb"), ("chans 0", dict(chans=0), EINVAL, "ftrb"),
    ("pools 0", dict(pools=0), EINVAL, "ftrb"), ("pools 7", dict(pools=7, h=256, w=256, d=256), EINVAL, "ftrb"),
    ("h >> pools == 0", dict(h=3), EUNSUPPORTED, "ftrb"), ("w >> pools == 0", dict(w=3), EUNSUPPORTED, "ftrb"),
    ("d >> pools == 0", dict(d=3), EUNSUPPORTED, "ftb3"),
    ("n 65536", dict(n=65536), EINVAL, "b"),
]
ENTRIES2, ENTRIES3 = "ftrbB", "ftTbB"
ENTRY = {(False, "f"): "cine_unet2d_forward", (False, "t"): "cine_unet2d_forward_train", (False, "r"): "cine_unet2d_forward_branches",
         (False, "b"): "cine_unet2d_backward", (False, "B"): "cine_unet2d_backward_drop",
         (True, "f"): "cine_unet3d_forward", (True, "t"): "cine_unet3d_forward_train", (True, "T"): "cine_unet3d_forward_train_drop",
         (True, "b"): "cine_unet3d_backward", (True, "B"): "cine_unet3d_backward_drop"}
# the prefix of the message each entry point leaves (the forms share their checks)
MESSAGE = {"f": "_forward", "t": "_forward", "T": "_forward", "r": "_forward", "b": "_backward", "B": "_backward"}


def applies(entries, e, three):
    """Whether a row of REFUSALS applies to entry point e of the 2-D / 3-D sequence."""
    if ("3" in entries and not three) or ("2" in entries and three):
        return False
    return {"T": "t", "B": "b"}.get(e, e) in entries


def entry_call(L, e, a, p):
    """The call of entry point e (a letter of ENTRIES2 / ENTRIES3) with dims a and the operands p: addresses x, y, gy, gx, ws / ws_bytes (inference and
    backward scratch), fwd_ws / fwd_bytes (training layout), bws / bws_bytes (branches), stream, the slot lists weights, wdgrad, grads (Python
    lists, nsets sets one after the other; None = a NULL array), side (list | None), nside, train, drop."""
    arr = {k: None if p[k] is None else ptr_array(p[k]) for k in ("weights", "wdgrad", "grads")}
    if e == "f":
        return call_forward(L, a, p["x"], p["y"], arr["weights"], p["ws"], p["ws_bytes"], p["stream"])
    if e in "tT":
        return call_forward(L, a, p["x"], p["y"], arr["weights"], p["fwd_ws"], p["fwd_bytes"], p["stream"], train=True, use_drop_entry=e == "T")
    if e == "r":
        side = None if p["side"] is None else ptr_array(p["side"])
        return call_branches(L, a, p["x"], p["y"], arr["weights"], p["bws"], p["bws_bytes"], p["stream"], side, p["nside"], p["train"], p["drop"])
    return call_backward(L, a, p["x"], p["gy"], arr["wdgrad"], arr["grads"], p["fwd_ws"], p["fwd_bytes"], p["ws"], p["ws_bytes"], p["gx"], p["stream"],
                         use_drop_entry=e == "B")


def refusal_dims(three, **over):
    """The dims the refusals start from: REFUSAL_CASE with two sets (n = 2), REFUSAL_CASE3 with its own."""
    return dims(REFUSAL_CASE3, **over) if three else dims(REFUSAL_CASE, **{"nsets": 2, **over})


def pointer_refusals(e, p, three, nptr):
    """(what, operands with one pointer or slot nulled) for entry point e: each pointer NULL, each slot of each list NULL (wdgrad's bias slots may be)."""
    fwd = e in "ftTr"
    rows = []
    for k in (("x", "y", "weights", "bws" if e == "r" else "ws" if e == "f" else "fwd_ws") if fwd else ("x", "gy", "wdgrad", "grads", "fwd_ws", "ws")):
        rows.append((f"{k} NULL", dict(p, **{k: None})))
    for k in (("weights",) if fwd else ("wdgrad", "grads")):
        for i in range(len(p[k])):
            if k == "wdgrad" and i % nptr == nptr - 1:
                continue
            lst = list(p[k]); lst[i] = None
            rows.append((f"{k}[{i}] NULL", dict(p, **{k: lst})))
    return rows


def branch_refusals(p):
    """(what, dims overrides, operand overrides, code) of cine_unet2d_forward_branches' own checks, from two sets with n = 2 ... 8."""
    s = p["stream"] if p["stream"] is not None else 0x7000
    sd = p["side"]
    return [
        ("nside -1", {}, dict(nside=-1), EINVAL),
        ("side NULL", {}, dict(side=None, nside=1), EINVAL),
        ("side[0] NULL", {}, dict(side=[None] + sd[1:], nside=1), EINVAL),
        ("side[1] NULL", dict(n=4), dict(side=[sd[0], None, sd[2]], nside=3), EINVAL),
        ("side[0] == stream", {}, dict(side=[s] + sd[1:], nside=1, stream=s), EINVAL),
        ("nbranch % nsets", dict(n=6), dict(nside=2), EINVAL),
        ("nbranch 9", dict(n=18), dict(side=sd + [sd[0] + 8], nside=8), EINVAL),
        ("n / nbranch < 1", {}, dict(nside=3), EINVAL),
        ("drop with train 0", {}, dict(nside=1, train=0, drop=0x8000), EINVAL),
        ("drop with train 2", {}, dict(nside=1, train=2, drop=0x8000), EINVAL),
    ]
