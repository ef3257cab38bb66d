"""The yardstick of the CRNN launch-sequence sweep (test_crnn_sequences.py on the GPU, test_crnn_sequences_cpu.py without one): the literal
loops of oracle/recurrent_ref.BCRNNlayer / _CRNNBody._body in float64 under autograd, chained over cascades (cascade k's [x0..x3] is the state
of cascade k + 1; the first state is zeros and takes no gradient; out = conv4(x3) + residual as in CRNNBody.body), with every ReLU behind ONE
autograd.Function whose backward multiplies by a mask handed in; the time sweeps alone on given input terms P (what cine_bcrnn_sweep and
cine_bcrnn_sweep_bwd compute, the latter as the recursion of include/cine_hip.h); the same in float32 on the CPU, whose error against float64
sets each tensor's bar; the case table and the arithmetic of what each row reaches.  A plain module, not a conftest.

Masked ReLU.  forward relu(v); backward g * m.  m None: plain ReLU (m = v > 0).  The GPU tests hand in the DEVICE's masks (hf > 0, hb > 0,
x_k > 0): the backward is then linear and exact, so float32 and float64 can no longer disagree at isolated O(1) entries and the error is
max |d| / peak; the forward stays a true-ReLU check.  The masks are a condition, not a loophole (mask_condition): wherever a mask differs from
pre64 > 0, |pre64| <= bar * peak of that pre-activation tensor, and at most MASK_SHARE of a run's entries differ."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from conftest import rel_err
from kernel_sweep import BAR, BAR_CAP

MASK_SHARE = 1e-4
# id -> (T, ch, c, h, w, och)
CASES = {
    "cfg": (5, 2, 16, 40, 36, 2),           # CRNN-VarNet's channels; column-tile route; pair launch; odd T (T + 1 launches)
    "plane16": (4, 2, 16, 40, 16, 2),       # W equal to the tile width; even T
    "long": (15, 2, 16, 24, 16, 2),         # the workload's T on a small plane: ping-pong over many steps
    "ragged": (3, 3, 5, 9, 7, 2),           # general element-wise route, unaligned frames
    "rows32": (4, 2, 17, 12, 20, 2),        # padded rows 32: two launches per step, not a pair
    "xpd": (5, 12, 18, 24, 20, 10),         # XPDNet_RNN's channel counts (ch = 2 (n + 1), och = 2 n, 18 hidden)
    "w2": (3, 2, 16, 12, 2, 2), "w4": (3, 2, 16, 12, 4, 2), "w8": (3, 2, 16, 12, 8, 2),        # the 2-, 4- and 8-wide tile tiers
    "one": (1, 2, 16, 12, 20, 2),           # T = 1: both chains meet at once; gw_hh stays zero
    "two": (2, 2, 4, 6, 10, 2),             # T = 2: the chains cross without a middle frame
    "area-in": (2, 2, 2, 396, 208, 2),      # 2 ceil(frags / 52) = 198: the last pair shape
    "area-out": (2, 2, 2, 400, 208, 2),     # ... = 200: the first two-launch shape
}
SWEEP_ONLY = ("area-in", "area-out")                         # the sweep entry points only (no weight gradient: its float32 error passes BAR there)
BODY_CASES = ("cfg", "ragged", "rows32", "xpd", "one", "w4")
OFFSET_CASES = ("cfg", "ragged", "w4", "rows32")             # run again at storage offsets of 1, 2 and 3 floats
SEEDS = {k: 500 + 11 * i for i, k in enumerate(CASES)}
# id -> the routes (cine_diag_counter 4 .. 12, named as in test_conv_fwd_kernels.py) the launches of one sweep call take, forward or backward, at an
# aligned base with every lean kernel on.  "wide" = the 16-wide column-tile kernel of conv_plane.hip (pair launches included), the CRNN path's only
# lean route; "pair" = the general kernel's pair launch; the single launches of an odd T's middle frame and of the two-launch shapes stage by vector
# ("general_vec") or, on ragged's 7-wide rows, by element.  No case reaches "plane": a pair launch has no plane form, and the plane kernels have no
# 16-fragment tile, which the single launches of this configuration use.
ROUTES_ALIGNED = {
    "cfg": {"wide"}, "one": {"wide"},
    "plane16": {"pair"}, "two": {"pair"}, "area-in": {"pair"},
    "long": {"pair", "general_vec"}, "w2": {"pair", "general_vec"}, "w4": {"pair", "general_vec"}, "w8": {"pair", "general_vec"},
    "ragged": {"pair", "general_elem"},
    "rows32": {"general_vec"}, "xpd": {"general_vec"}, "area-out": {"general_vec"},
}
LEAN_ROUTES = {"plane": 1, "wide": 4}                        # route -> its cine_set_conv_plane bit
GENERAL_ROUTES = {"pair", "general_vec", "general_elem"}
UNALIGNED_ROUTES = {"pair", "general_elem"}                  # at a storage offset of 1 .. 3 floats no 16-byte staging and no column tiles
LEAN_CASES = tuple(k for k, v in ROUTES_ALIGNED.items() if v & set(LEAN_ROUTES))
PARAM_NAMES = (["w_ih2ih", "w_i2h", "w_h2h", "b_i2h", "b_h2h", "b_ih2ih"] + [f"{n}{k}{s}" for k in (1, 2, 3) for n, s in (("w", "x"), ("w", "h"), ("b", "x"), ("b", "h"))]
               + ["w4", "b4"])                               # CRNNBody._body_params order


def bar(e32):
    """The bar of one tensor of one run: twice the error of this reference in float32 against itself in float64 under the same masks, BAR at
    least and BAR_CAP at most (test_crnn_sequences_cpu.py asserts that the cap never decides)."""
    return min(BAR_CAP, max(BAR, 2 * e32))


# ================================================================== what a row reaches: crnn_step2_impl and cine_bcrnn_sweep restated
def cdiv(a, b):
    return -(-a // b)


def tile_width(w):
    return 16 if w > 8 else 8 if w > 4 else 4 if w > 2 else 2


def padded_rows(c):
    return cdiv(c, 16) * 16


def frags(h, w):
    tw = tile_width(w)
    return cdiv(h * tw, 16) * cdiv(w, tw)


def pair_area(h, w, n=1):
    """The figure crnn_step2_impl compares with 200."""
    return 2 * n * cdiv(frags(h, w), 52)


def pair_shape(c, h, w):
    """Both chains of a step in ONE launch (n = 1 per chain, both gated or neither)."""
    return padded_rows(c) <= 16 and pair_area(h, w) < 200


def launches(T, c, h, w):
    """Convolution launches of one cine_bcrnn_sweep / cine_bcrnn_sweep_bwd call: a pair launch per step and two single launches where the
    chains meet in the middle frame of an odd T; two launches per step outside the pair configuration."""
    return T + (T & 1) if pair_shape(c, h, w) else 2 * T


# ================================================================== the masked ReLU
class MaskedRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, m):
        ctx.save_for_backward((v > 0) if m is None else m)
        return v.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        (m,) = ctx.saved_tensors
        return g * m.to(g.dtype), None


def act(v, m, relu):
    return MaskedRelu.apply(v, m) if relu else v


# ================================================================== seeded data
def _rand(rs, *shape):
    return torch.from_numpy(rs.standard_normal(shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def body_data(case, ncasc=2):
    """float32 inputs of a chain of `ncasc` cascades (read-only): per cascade x (T, ch, h, w), residual and output gradient (T, och, h, w); the
    20 parameters in _body_params order, weights at 1 / sqrt(fan-in of the sum they enter)."""
    T, ch, c, h, w, och = CASES[case]
    rs = np.random.RandomState(SEEDS[case])
    fan = (9 * (2 * c + ch)) ** -0.5
    shapes = [(c, c, 3, 3), (c, ch, 3, 3), (c, c, 3, 3), (c,), (c,), (c,)] + [(c, c, 3, 3), (c, c, 3, 3), (c,), (c,)] * 3 + [(och, c, 3, 3), (och,)]
    params = [_rand(rs, *s) * (fan if len(s) == 4 else 0.1) for s in shapes]
    xs = [_rand(rs, T, ch, h, w) for _ in range(ncasc)]
    res = [_rand(rs, T, och, h, w) for _ in range(ncasc)]
    gouts = [_rand(rs, T, och, h, w) for _ in range(ncasc)]
    return SimpleNamespace(case=case, dims=CASES[case], params=params, xs=xs, res=res, gouts=gouts)


@functools.lru_cache(maxsize=None)
def sweep_data(case):
    """float32 operands of the sweep entry points (read-only): P, gout (T, c, h, w), W_h2h (c, c, 3, 3)."""
    T, ch, c, h, w, och = CASES[case]
    rs = np.random.RandomState(SEEDS[case] + 5)
    return SimpleNamespace(case=case, P=_rand(rs, T, c, h, w), gout=_rand(rs, T, c, h, w), W=_rand(rs, c, c, 3, 3) * 0.8 * (9 * c) ** -0.5)


def synthetic_gates(case, seed_off=0):
    """hf / hb the backward test writes itself: +0.0, -0.0, the smallest positive subnormal, negatives and positives, every kind in every frame.
    Only > 0 opens a gate: both zeros and the negatives close it, the subnormal opens it."""
    T, ch, c, h, w, och = CASES[case]
    rs = np.random.RandomState(SEEDS[case] + 9 + seed_off)
    vals = np.array([0.0, -0.0, 1e-45, -1.0, -1e-30, 2.0, 1e-30], dtype=np.float32)
    assert vals[2] > 0 and np.signbit(vals[1])
    out = []
    for _ in range(2):
        g = vals[rs.randint(0, len(vals), size=(T, c * h * w))]
        for t in range(T):
            g[t, rs.permutation(c * h * w)[:len(vals)]] = vals
        out.append(torch.from_numpy(g.reshape(T, c, h, w)))
    return out


# ================================================================== the time sweeps alone (cine_bcrnn_sweep, cine_bcrnn_sweep_bwd)
def sweep_forward(P, W, relu, dtype=torch.float64):
    """hf, hb, out and the pre-activations pre_f, pre_b (T, c, h, w): h_t = [ReLU](conv(h_prev; W) + P_t) forward and backward in time from
    zeros, out = hf + hb."""
    P, W = P.to(dtype), W.to(dtype)
    T = P.shape[0]
    zero = torch.zeros_like(P[:1])
    pre_f, pre_b = [None] * T, [None] * T
    hid = zero
    for t in range(T):
        pre_f[t] = F.conv2d(hid, W, padding=1) + P[t:t + 1]
        hid = pre_f[t].clamp_min(0) if relu else pre_f[t]
    hid = zero
    for t in range(T - 1, -1, -1):
        pre_b[t] = F.conv2d(hid, W, padding=1) + P[t:t + 1]
        hid = pre_b[t].clamp_min(0) if relu else pre_b[t]
    pre_f, pre_b = torch.cat(pre_f), torch.cat(pre_b)
    hf, hb = (pre_f.clamp_min(0), pre_b.clamp_min(0)) if relu else (pre_f, pre_b)
    return SimpleNamespace(hf=hf, hb=hb, out=hf + hb, pre_f=pre_f, pre_b=pre_b)


def sweep_backward(gout, W, gate_f, gate_b, dtype=torch.float64):
    """The recursion of the header: gf[t] = [gate_f[t]] (conv(gf[t + 1]; Wd) + gout[t]) for t = T-1 .. 0, gb[t] = [gate_b[t]] (conv(gb[t - 1]; Wd) +
    gout[t]) for t = 0 .. T-1, Wd the flipped / transposed W, gP = gf + gb.  gate_* boolean (T, c, h, w) or None (no ReLU)."""
    gout = gout.to(dtype)
    Wd = W.to(dtype).flip(2, 3).transpose(0, 1).contiguous()
    T = gout.shape[0]
    gf, gb = [None] * T, [None] * T
    prev = torch.zeros_like(gout[:1])
    for t in range(T - 1, -1, -1):
        prev = F.conv2d(prev, Wd, padding=1) + gout[t:t + 1]
        if gate_f is not None:
            prev = prev * gate_f[t:t + 1].to(dtype)
        gf[t] = prev
    prev = torch.zeros_like(gout[:1])
    for t in range(T):
        prev = F.conv2d(prev, Wd, padding=1) + gout[t:t + 1]
        if gate_b is not None:
            prev = prev * gate_b[t:t + 1].to(dtype)
        gb[t] = prev
    gf, gb = torch.cat(gf), torch.cat(gb)
    return SimpleNamespace(gf=gf, gb=gb, gP=gf + gb)


# ================================================================== the body, literally
MASK_KEYS = ("hf", "hb", "x1", "x2", "x3")


def bcrnn(x, s0, p, masks, relu):
    """oracle BCRNNlayer.forward for batch 1: the cell i2h(x_t) + h2h(hid) + ih2ih(s0_t) per frame, forward and backward in time, summed.
    Returns (x0, pre_f, pre_b)."""
    w_ih2ih, w_i2h, w_h2h, b_i2h, b_h2h, b_ih2ih = p[:6]
    T = x.shape[0]
    zero = x.new_zeros((1, w_h2h.shape[0]) + tuple(x.shape[2:]))
    m = masks or {}

    def cell(t, hid):
        return F.conv2d(x[t:t + 1], w_i2h, b_i2h, padding=1) + F.conv2d(hid, w_h2h, b_h2h, padding=1) + F.conv2d(s0[t:t + 1], w_ih2ih, b_ih2ih, padding=1)
    fwd, bwd, pre_f, pre_b = [None] * T, [None] * T, [None] * T, [None] * T
    hid = zero
    for t in range(T):
        pre_f[t] = cell(t, hid)
        hid = fwd[t] = act(pre_f[t], None if m.get("hf") is None else m["hf"][t:t + 1], relu)
    hid = zero
    for t in range(T - 1, -1, -1):
        pre_b[t] = cell(t, hid)
        hid = bwd[t] = act(pre_b[t], None if m.get("hb") is None else m["hb"][t:t + 1], relu)
    return torch.cat(fwd) + torch.cat(bwd), torch.cat(pre_f), torch.cat(pre_b)


def body(x, state, residual, p, masks, relu):
    """oracle _CRNNBody._body for batch 1 with out = conv4(x3) + residual: (out, [x0..x3], pre-activations {hf, hb, x1, x2, x3})."""
    m = masks or {}
    x0, pre_f, pre_b = bcrnn(x, state[0], p, masks, relu)
    feats, pre = [x0], {"hf": pre_f, "hb": pre_b}
    for k in (1, 2, 3):
        wx, wh, bx, bh = p[6 + 4 * (k - 1):10 + 4 * (k - 1)]
        pre[f"x{k}"] = F.conv2d(state[k], wh, bh, padding=1) + F.conv2d(feats[-1], wx, bx, padding=1)
        feats.append(act(pre[f"x{k}"], m.get(f"x{k}"), relu))
    return F.conv2d(feats[3], p[18], p[19], padding=1) + residual, feats, pre


def chain(data, dtype=torch.float64, masks=None, relu=True, grads=True):
    """The cascades of `data` chained, in `dtype` on the CPU: outs, feats and pre per cascade; with `grads` the gradients of sum_k <out_k, gout_k>
    with respect to every x (gx), every residual (gres) and the 20 shared parameters (gp).  masks: per cascade {hf, hb, x1, x2, x3} boolean
    tensors, or None (plain ReLU)."""
    T, ch, c, h, w, och = data.dims
    leaf = lambda v: v.detach().to(dtype, copy=True).requires_grad_(grads)          # noqa: E731  (a copy: `data` is shared and read-only)
    p, xs, res = [leaf(v) for v in data.params], [leaf(v) for v in data.xs], [leaf(v) for v in data.res]
    state = [torch.zeros((T, c, h, w), dtype=dtype) for _ in range(4)]
    outs, feats, pres = [], [], []
    with torch.enable_grad():
        for k in range(len(xs)):
            out, state, pre = body(xs[k], state, res[k], p, None if masks is None else masks[k], relu)
            outs.append(out); feats.append(state); pres.append(pre)
        if grads:
            torch.autograd.backward(outs, [g.to(dtype) for g in data.gouts])
    det = lambda ts: [t.detach() for t in ts]                                       # noqa: E731
    r = SimpleNamespace(outs=det(outs), feats=[det(f) for f in feats], pres=[{k: v.detach() for k, v in pr.items()} for pr in pres])
    if grads:
        r.gx, r.gres, r.gp = [v.grad for v in xs], [v.grad for v in res], [v.grad for v in p]
    return r


def own_masks(run):
    """The masks a run's own pre-activations give."""
    return [{k: pr[k] > 0 for k in MASK_KEYS} for pr in run.pres]


def chain_tensors(run):
    """name -> tensor of everything a chain run is compared on."""
    t = {}
    for k, o in enumerate(run.outs):
        t[f"out{k}"] = o
        t.update({f"x{j}_{k}": f for j, f in enumerate(run.feats[k])})
    if hasattr(run, "gx"):
        t.update({f"gx{k}": g for k, g in enumerate(run.gx)})
        t.update({f"gres{k}": g for k, g in enumerate(run.gres)})
        t.update({f"g_{n}": g for n, g in zip(PARAM_NAMES, run.gp)})
    return t


def errors(a, b):
    """rel_err (max |d| / peak) per tensor name of two namespaces' / dicts' tensors; an all-zero reference (gw_hh at T = 1) must be met exactly."""
    out = {}
    for k in b:
        out[k] = (0.0 if float(a[k].abs().max()) == 0 else float("inf")) if float(b[k].abs().max()) == 0 else rel_err(a[k], b[k])
    return out


def measured(data, masks, relu, grads=True):
    """(the float64 run under `masks`, e32 per tensor name: this reference in float32 under the same masks against it)."""
    r64, r32 = chain(data, torch.float64, masks, relu, grads), chain(data, torch.float32, masks, relu, grads)
    return r64, errors(chain_tensors(r32), chain_tensors(r64))


def pre_bars(data, relu):
    """Per cascade: (float64 pre-activations, bar of each from the float32 run's error on it).  The forward does not depend on the masks."""
    r64, r32 = chain(data, torch.float64, None, relu, False), chain(data, torch.float32, None, relu, False)
    return [(p64, {k: bar(e) for k, e in errors(p32, p64).items()}) for p32, p64 in zip(r32.pres, r64.pres)]


def mask_condition(masks, pres64, bars):
    """Where a mask differs from pre64 > 0 the pre-activation is within bar * peak of zero; at most MASK_SHARE of the entries differ.
    masks / pres64: dicts name -> tensor; bars: name -> bar of that pre-activation tensor.  Returns the number of entries that differ."""
    diff = total = 0
    for k, m in masks.items():
        pre = pres64[k]
        bad = m.cpu() != (pre > 0)
        total += bad.numel()
        n = int(bad.sum())
        if n:
            diff += n
            lim = bars[k] * float(pre.abs().max())
            worst = float(pre[bad].abs().max())
            assert worst <= lim, f"mask {k}: differs from the float64 sign at |pre| = {worst:.3e} > {lim:.3e}"
    assert diff <= MASK_SHARE * total, f"{diff} of {total} mask entries differ from the float64 signs"
    return diff
