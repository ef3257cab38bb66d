"""The yardstick of the MWCNN launch-sequence sweep (test_mwcnn_sequences.py on the GPU, test_mwcnn_sequences_cpu.py without one):
oracle/xpdnet_ref.MWCNN in float64 under autograd, on seeded inputs and synth.fill_parameters_ weights, for one network or two with a
sample split; the same oracle in float32 on the CPU, whose error against float64 sets each tensor's bar; the case table; and the
pointer arrays cine_mwcnn_forward / _forward2 / _forward_train / _backward take (include/cine_hip.h: first_convs[0]; conv_blocks_per_scale[s][i]
in module order; first_convs[1] weight, bias -- all 3x3 weights packed with cine_pack_conv3x3, the input-gradient list with
cine_pack_conv3x3_dgrad and NULL in the bias slot).  A plain module, not a conftest."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import torch

from kernel_sweep import BAR, BAR_CAP

SLOPE = 0.2
# id -> (n, in, out, first, nf, nc, h, w).  The smallest shapes at which cine_mwcnn_* still change path.  Which forward conv kernel a level takes
# (conv_plane.hip: launch_conv_plane needs a plane exactly 16 / 8 / 4 / 2 wide in one of its listed tile shapes; everything else is the general
# kernel of conv_kernels.hip or, for > 32 rows on planes wider than 16, conv_coarse.hip) is stated per case and asserted by
# test_mwcnn_sequences.py::test_both_conv_kernels_run_over_the_table with the library's diagnostic counters.
CASES = {
    # no IWT + skip conv, the final conv reads scale 0 directly; planes 3 x 5: general kernel
    "one-scale": (1, 2, 2, 8, [8], [1], 6, 10),
    # today's small topology off powers of two, nc 2 next to 1; widths 20 / 10 / 5: the wide-plane kernel for the 20-wide first conv, the general
    # kernel at every other level
    "small": (3, 6, 4, 8, [8, 16], [2, 1], 12, 20),
    # XPDNet's topology on planes 16 wide, as XPDNet's own (200 x 16): widths 16 / 8 / 4 / 2 -- the PLANE kernel at 12 of its 14 convs (first conv, DWT,
    # inner, IWT + skip convs; the two 64-row convs on 10 x 4 planes have no plane shape); coarsest planes 5 x 2, odd height 5 at scale 2
    "default": (2, 12, 10, 16, [16, 32, 64], [2, 2, 2], 40, 16),
    # no channel count a multiple of 16 (or of 8: the plane kernel's whole-chunk shapes refuse), first < 16; widths 12 / 6 / 3: general kernel,
    # its 14-fragment (20 rows on 5 x 3) and 4-fragment (48 rows on 5 x 3) tiles
    "ragged": (2, 3, 5, 6, [12, 20], [1, 3], 20, 12),
    # out == first, the boundary of max(4 first, 4 out); widths 12 / 6: general kernel
    "eq": (2, 4, 8, 8, [8], [2], 8, 12),
    # 2 nc == kMaxConvs; widths 8 / 4 with <= 16 rows: tile shapes the plane kernel does not list, general kernel
    "deep-convs": (1, 2, 2, 4, [8], [4], 8, 8),
    # kMaxScales; coarsest planes 1 x 3; 4 channels everywhere: general kernel (the 16-wide level's convs have DWT / IWT sources of 4 channels).
    # 64 x 128 (coarsest 1 x 2) is no case: InstanceNorm over two elements maps them to +-1 whatever their values, the gradient through it lives on
    # eps alone, and the float32 oracle itself misses float64 by 4e-5 to 6e-4 on the coarsest weight gradients depending on the seed -- past BAR_CAP
    "six-scales": (1, 2, 2, 4, [4] * 6, [1] * 6, 64, 192),
    # weight-gradient sources of 2 * 64 * 24 * 24 = 2 * 16 * 48 * 48 = 73 728 floats >= the 65 536 of grad_kernels.hip: launch_wgrad, so the DWT source
    # of scale 0 and the IWT + skip source of the final conv are materialised first; every other case stays below
    # (test_mwcnn_sequences_cpu.py::test_materialise_threshold_has_a_case_on_each_side);
    # scale 0's last conv (64 rows on 24 x 24) runs on conv_coarse.hip with 19 statistics records per plane
    "big-source": (2, 4, 4, 16, [16], [1], 48, 48),
}
SEEDS = {k: 100 + 7 * i for i, k in enumerate(CASES)}
MATERIALISE_FLOATS = 1 << 16
# (case, slope, split) of every run of the sweep: split None = one network
RUNS = [(k, SLOPE, None) for k in CASES] + [("small", 0.0, None), ("small", 1.0, None),
                                             ("small", SLOPE, 1), ("small", SLOPE, 2), ("default", SLOPE, 1)]
TIED = ("deep-convs", (1, 2))          # slots (0, 1) and (0, 2) of deep-convs: both 8 -> 8
TIED_RUN = (TIED[0], SLOPE, 1, TIED[1], None, 2)      # reference(*TIED_RUN): set one tied, set two not, two samples split at 1


def run_id(r):
    k, slope, split = r
    return k + (f"-slope{slope:g}" if slope != SLOPE else "") + (f"-split{split}" if split is not None else "")


def kwargs(case):
    n, cin, cout, first, nf, nc, h, w = CASES[case]
    return dict(in_chans=cin, out_chans=cout, n_scales=len(nf), n_filters_per_scale=list(nf), n_convs_per_scale=list(nc),
                n_first_convs=1, first_conv_n_filters=first, res=False)


def rel_l2(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def bar(e32):
    """The bar of one tensor of one case: twice the error of the float32 oracle against the float64 one, BAR at least and BAR_CAP at most
    (kernel_sweep._bar's rule for long reductions; test_mwcnn_sequences_cpu.py asserts that the cap never decides)."""
    return min(BAR_CAP, max(BAR, 2 * e32))


def slots(net):
    """The parameters of one network in the order of the pointer arrays (what ops.MwcnnWeights._params states)."""
    seq = [net.first_convs[0].layers[0].weight]
    for blocks in net.conv_blocks_per_scale:
        seq += [blk.layers[0].weight for blk in blocks]
    return seq + [net.first_convs[-1].weight, net.first_convs[-1].bias]


def feature_floats(case, n=None):
    """The floats of every feature map the training forward keeps (first conv + every conv block's output), from the channel plan of the
    reference's mwcnn.py:110-132, restated here independently of the library."""
    n0, cin, cout, first, nf, nc, h, w = CASES[case]
    n = n0 if n is None else n
    total = n * first * h * w
    for s in range(len(nf)):
        for i in range(2 * nc[s]):
            co = nf[s]
            if i == 2 * nc[s] - 1:
                co = max(4 * first, 4 * cout) if s == 0 else 4 * nf[s - 1]
            total += n * co * (h >> (s + 1)) * (w >> (s + 1))
    return total


def conv_plan(case):
    """(ci, co, hs, ws, transformed source) of every conv block, then the final conv: what the weight gradients re-stage."""
    n, cin, cout, first, nf, nc, h, w = CASES[case]
    out = []
    for s in range(len(nf)):
        for i in range(2 * nc[s]):
            ci = co = nf[s]
            if i == 0:
                ci = 4 * (first if s == 0 else nf[s - 1])
            if i == 2 * nc[s] - 1:
                co = max(4 * first, 4 * cout) if s == 0 else 4 * nf[s - 1]
            out.append((ci, co, h >> (s + 1), w >> (s + 1), i == 0 or (i == nc[s] and s != len(nf) - 1)))
    return out + [(first, cout, h, w, True)]


def make_net(case, seed, slope=SLOPE, tie=None):
    """The float32 oracle network of a case; tie = (i, j): conv_blocks_per_scale[0][j] IS module [0][i]."""
    from cine_hip import synth
    from oracle import xpdnet_ref as X
    net = X.MWCNN(**kwargs(case))
    synth.fill_parameters_(net, seed, keep=())
    if tie is not None:
        net.conv_blocks_per_scale[0][tie[1]] = net.conv_blocks_per_scale[0][tie[0]]
    set_slope(net, slope)
    return net.eval()


def set_slope(net, slope):
    for m in net.modules():
        if isinstance(m, torch.nn.LeakyReLU):
            m.negative_slope = slope


def _run(nets, x, gy, split, dtype):
    """y, gx and per network the slot gradients of sum(y gy), y = cat(net0(x[:split]), net1(x[split:])), in `dtype` on the CPU."""
    import copy
    nets = [copy.deepcopy(nt).to(dtype) for nt in nets]
    xr = x.to(dtype).requires_grad_(True)
    with torch.enable_grad():
        if len(nets) == 1:
            y = nets[0](xr)
        else:
            y = torch.cat([nets[0](xr[:split]), nets[1](xr[split:])])
        (y * gy.to(dtype)).sum().backward()
    return y.detach(), xr.grad, [[p.grad for p in slots(nt)] for nt in nets]


@functools.lru_cache(maxsize=None)
def reference(case, slope=SLOPE, split=None, tie=None, tie2=None, n=None):
    """One run of the sweep, computed once per process and shared (treat every tensor as read-only): float32 x, gy and networks, the float64
    results y, gx, grads[net][slot], and e32 = the float32 oracle's relative L2 error against each of them (same nesting)."""
    cin, cout = CASES[case][1:3]
    h, w = CASES[case][6:]
    n = CASES[case][0] if n is None else n          # (n: another sample count than the table's -- the tied two-set run of deep-convs takes 2)
    seed = SEEDS[case]
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((n, cin, h, w)).astype(np.float32))
    gy = torch.from_numpy(rs.standard_normal((n, cout, h, w)).astype(np.float32))
    nets = [make_net(case, seed + 1, slope, tie)]
    if split is not None:
        nets.append(make_net(case, seed + 2, slope, tie2))
    y, gx, grads = _run(nets, x, gy, split, torch.float64)
    y32, gx32, grads32 = _run(nets, x, gy, split, torch.float32)
    e32 = SimpleNamespace(y=rel_l2(y32, y), gx=rel_l2(gx32, gx),
                          grads=[[rel_l2(a, b) for a, b in zip(g32, g64)] for g32, g64 in zip(grads32, grads)])
    return SimpleNamespace(case=case, slope=slope, split=split, x=x, gy=gy, nets=nets, y=y, gx=gx, grads=grads, e32=e32,
                           dims=(n,) + tuple(CASES[case][1:]))


# ================================================================== the C ABI's operands (device side)
def int_array(v):
    return (ctypes.c_int * len(v))(*v)


class DeviceNet:
    """One network's pointer arrays on `dev`: weights (cine_pack_conv3x3 of every 3x3 weight, the bias at its own address), wdgrad
    (cine_pack_conv3x3_dgrad, NULL in the bias slot) -- a parameter that sits in two slots is packed once and its pointer repeated."""

    def __init__(self, net, dev):
        from cine_hip._lib import lib, check
        L = lib()
        st = torch.cuda.current_stream().cuda_stream
        self.params = slots(net)
        self.keep, fwd, dg, seen = [], [], [], {}
        for k, p in enumerate(self.params):
            if id(p) in seen:
                f, d = seen[id(p)]
            elif p.dim() == 1:
                b = p.detach().float().to(dev).contiguous()
                self.keep.append(b)
                f, d = b.data_ptr(), None
            else:
                wt = p.detach().float().to(dev).contiguous()
                co, ci = wt.shape[:2]
                pf = torch.zeros(L.cine_conv3x3_packed_floats(co, ci), device=dev)
                pd = torch.zeros(L.cine_conv3x3_dgrad_packed_floats(co, ci), device=dev)
                check(L.cine_pack_conv3x3(wt.data_ptr(), pf.data_ptr(), co, ci, st), "cine_pack_conv3x3")
                check(L.cine_pack_conv3x3_dgrad(wt.data_ptr(), pd.data_ptr(), co, ci, st), "cine_pack_conv3x3_dgrad")
                self.keep += [wt, pf, pd]
                f, d = pf.data_ptr(), pd.data_ptr()
            seen[id(p)] = (f, d)
            fwd.append(f); dg.append(d)
        self.weights = (ctypes.c_void_p * len(fwd))(*fwd)
        self.wdgrad = (ctypes.c_void_p * len(dg))(*dg)

    def __len__(self):
        return len(self.params)


def ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


# ================================================================== calls through the C ABI
def dims(case, **over):
    """The scalar arguments of one call: the case's, with overrides (S alone changes n_scales and leaves the lists)."""
    n, cin, cout, first, nf, nc, h, w = CASES[case]
    a = dict(n=n, cin=cin, cout=cout, first=first, nf=list(nf), nc=list(nc), h=h, w=w, S=len(nf), nfc=1, res=0, slope=SLOPE)
    a.update(over)
    return SimpleNamespace(**a)


def ws_sizes(L, a):
    """(cine_mwcnn_ws_bytes, cine_mwcnn_train_ws_bytes, cine_mwcnn_backward_ws_bytes) of a call's dims."""
    t = (a.n, a.h, a.w, a.cin, a.cout, a.S, int_array(a.nf), int_array(a.nc), a.first)
    return L.cine_mwcnn_ws_bytes(*t), L.cine_mwcnn_train_ws_bytes(*t), L.cine_mwcnn_backward_ws_bytes(*t)


def call_forward(L, a, x, y, weights, ws, ws_bytes, stream):
    return L.cine_mwcnn_forward(x, y, weights, a.n, a.h, a.w, a.cin, a.cout, a.S, int_array(a.nf), int_array(a.nc), a.nfc, a.first, a.res,
                                a.slope, ws, ws_bytes, stream)


def call_forward2(L, a, x, y, weights, weights2, split, ws, ws_bytes, stream):
    return L.cine_mwcnn_forward2(x, y, weights, weights2, split, a.n, a.h, a.w, a.cin, a.cout, a.S, int_array(a.nf), int_array(a.nc), a.nfc,
                                 a.first, a.res, a.slope, ws, ws_bytes, stream)


def call_forward_train(L, a, x, y, weights, weights2, split, ws, ws_bytes, stream):
    return L.cine_mwcnn_forward_train(x, y, weights, weights2, split, a.n, a.h, a.w, a.cin, a.cout, a.S, int_array(a.nf), int_array(a.nc),
                                      a.nfc, a.first, a.res, a.slope, ws, ws_bytes, stream)


def call_backward(L, a, x, gy, wdgrad, wdgrad2, grads, grads2, split, fwd_ws, fwd_bytes, ws, ws_bytes, gx, stream):
    return L.cine_mwcnn_backward(x, gy, wdgrad, wdgrad2, grads, grads2, split, a.n, a.h, a.w, a.cin, a.cout, a.S, int_array(a.nf),
                                 int_array(a.nc), a.first, a.slope, fwd_ws, fwd_bytes, ws, ws_bytes, gx, stream)


EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
REFUSAL_CASE = "small"
# (what, overrides of the dims, the slot list nulled ("weights" / "weights2" / "grads" / "wdgrad") or None, code, the entry points it applies to:
# f forward, 2 forward2, t forward_train, b backward).  Every one returns before the first launch (csrc/mwcnn.hip checks arguments, topology,
# sizes, workspaces and pointer slots ahead of the launch sequence), so the CPU file runs them with made-up device addresses and the GPU file
# again with guarded outputs.
REFUSALS = [
    ("n_scales 0", dict(S=0), None, EUNSUPPORTED, "f2tb"),
    ("n_scales 7", dict(S=7, nf=[8] * 7, nc=[1] * 7, h=128, w=128), None, EUNSUPPORTED, "f2tb"),
    ("nc 0", dict(nc=[0, 1]), None, EUNSUPPORTED, "f2tb"),
    ("nc 5", dict(nc=[2, 5]), None, EUNSUPPORTED, "f2tb"),
    ("nf 0", dict(nf=[8, 0]), None, EUNSUPPORTED, "f2tb"),
    ("n_first_convs 2", dict(nfc=2), None, EUNSUPPORTED, "f2t"),
    ("res 1", dict(res=1), None, EUNSUPPORTED, "f2t"),
    ("h not a multiple of 4", dict(h=14), None, EINVAL, "f2tb"),
    ("w not a multiple of 4", dict(w=22), None, EINVAL, "f2tb"),
    ("slope -0.1", dict(slope=-0.1), None, EINVAL, "f2tb"),
    ("slope 1.5", dict(slope=1.5), None, EINVAL, "f2tb"),
    ("split 0", dict(split=0), None, EINVAL, "2tb"),
    ("split n", dict(split=3), None, EINVAL, "2tb"),
    ("null slot in weights", dict(), "weights", EINVAL, "f2t"),
    ("null slot in weights2", dict(), "weights2", EINVAL, "2t"),
    ("null slot in grads", dict(), "grads", EINVAL, "b"),
    ("null slot in wdgrad", dict(), "wdgrad", EINVAL, "b"),
    ("n 65536", dict(n=65536), None, EINVAL, "b"),
    ("out_ch 12 > first_filters 8", dict(cin=2, cout=12, first=8), None, EINVAL, "f2tb"),
]
ENTRY = {"f": "cine_mwcnn_forward", "2": "cine_mwcnn_forward2", "t": "cine_mwcnn_forward_train", "b": "cine_mwcnn_backward"}


def refusal_call(L, entry, over, null, p):
    """The call of one row of REFUSALS at one entry point.  p: the pointers (x, y, gy, gx, ws, ws_bytes, fwd_ws, fwd_bytes, stream, and the
    four slot lists as Python lists of addresses); forward2 / forward_train / backward run with two sets, split 1 unless overridden."""
    over = dict(over)
    split = over.pop("split", 1)
    a = dims(REFUSAL_CASE, **over)
    lists = {k: list(p[k]) for k in ("weights", "weights2", "wdgrad", "wdgrad2", "grads", "grads2")}
    if null is not None:
        lists[null][2] = None
    arr = {k: ptr_array(v) for k, v in lists.items()}
    if entry == "f":
        return call_forward(L, a, p["x"], p["y"], arr["weights"], p["ws"], p["ws_bytes"], p["stream"])
    if entry == "2":
        return call_forward2(L, a, p["x"], p["y"], arr["weights"], arr["weights2"], split, p["ws"], p["ws_bytes"], p["stream"])
    if entry == "t":
        return call_forward_train(L, a, p["x"], p["y"], arr["weights"], arr["weights2"], split, p["fwd_ws"], p["fwd_bytes"], p["stream"])
    return call_backward(L, a, p["x"], p["gy"], arr["wdgrad"], arr["wdgrad2"], arr["grads"], arr["grads2"], split, p["fwd_ws"], p["fwd_bytes"],
                         p["ws"], p["ws_bytes"], p["gx"], p["stream"])


def refusal_message_ok(msg, entry, what):
    """The message is this call's: it names the entry point (cine_mwcnn_forward2 shares cine_mwcnn_forward's checks; the topology checks of all
    four say cine_mwcnn), and the out_ch > first_filters refusal names both counts."""
    names = {"f": ("cine_mwcnn_forward:", "cine_mwcnn:"), "2": ("cine_mwcnn_forward2:", "cine_mwcnn_forward:", "cine_mwcnn:"),
             "t": ("cine_mwcnn_forward_train:", "cine_mwcnn:"), "b": ("cine_mwcnn_backward:", "cine_mwcnn:")}[entry]
    ok = msg.startswith(names)
    if what.startswith("out_ch"):
        ok = ok and "out_ch 12" in msg and "first_filters 8" in msg
    return ok
