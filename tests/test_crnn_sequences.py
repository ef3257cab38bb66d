"""The launch sequences of the convolutional-RNN body against float64 (tests/crnn_reference.py: the yardstick, the masked ReLU, the case table,
the bar): cine_bcrnn_sweep and cine_bcrnn_sweep_bwd through the C ABI, and the Python sequences on top of them -- ag.CrnnBodyFn,
ag.BcrnnFn + ag.ConvSumFn, CRNNBody.body_train / body, BCRNNlayer.forward, CRNNcell.forward.

Through the C ABI every output sits between guard floats and is pre-filled with NaN (so the first chain to reach a frame must STORE and the
second ADD), hf / hb are sized at exactly (2, c, h, w) without `keep`, inputs are proven unchanged, a second call gives the same bits, the
launches are counted with cine_diag_counter, and subsets run again at storage offsets of 1, 2 and 3 floats.  The error is max |d| / peak at the
bar min(BAR_CAP, max(BAR, 2 e32)), e32 the same reference in float32 on the CPU under the same masks.  Bit identities asserted: keep 0 == keep 1;
out == hf + hb; gP == gf + gb; a lean route == the general route; relu = 0 ignores the gates; CRNN_SIDE_LANE off == on; BCRNN_SWEEP_IN_C off == on;
the inference forward == the training forward; two backward() calls == twice one; a second step == the first."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import crnn_reference as R
from conftest import rel_err
from kernel_sweep import EINVAL, NAN, Call, Worst, at_offsets, refused, same_bits, twice

pytestmark = pytest.mark.gpu
WORST = Worst()
ROUTES = ("plane", "tconv_plane", "wide", "wide_v3", "coarse", "stream1x1", "pair", "general_vec", "general_elem")
D_SWEEP_C, D_FIRST = 3, 4                       # cine_diag_counter: cine_bcrnn_sweep calls; the first route counter (csrc/common.h Diag)
LEAN = R.LEAN_ROUTES                            # route -> its cine_set_conv_plane bit
ROUTE_LOG = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    d = torch.device("cuda:0")
    yield d
    torch.cuda.synchronize()
    if WORST:
        WORST.report()
    for k in sorted(ROUTE_LOG):
        print(f"  routes {k:36s} " + ", ".join(f"{r} {v}" for r, v in sorted(ROUTE_LOG[k].items())))


def L():
    from cine_hip._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(what, got, want, e32, case):
    assert not torch.isnan(got).any(), f"{what} {case}: not fully written"
    if float(want.abs().max()) == 0:
        assert float(got.abs().max()) == 0, f"{what} {case}: must be exactly zero"
        return
    WORST.record(what, rel_err(got.detach().cpu(), want), R.bar(e32), case)


def _counted(call, T, c, h, w, what, case, off, sweep_c=None):
    """call() with its launches counted: the code; exactly R.launches convolution launches, pair launches only on pair shapes; the routes are the
    table's (R.ROUTES_ALIGNED) at an aligned base with every lean kernel on, general ones with a lean bit cleared or at a storage offset; never
    the plane-wide kernel."""
    from cine_hip import ops
    lib = L()
    before = [lib.cine_diag_counter(D_FIRST + i, 0) for i in range(len(ROUTES))]
    calls = lib.cine_diag_counter(D_SWEEP_C, 0)
    code = call()
    assert code == 0, (what, code, lib.cine_last_error())
    delta = {r: lib.cine_diag_counter(D_FIRST + i, 0) - before[i] for i, r in enumerate(ROUTES)}
    delta = {r: v for r, v in delta.items() if v}
    assert sum(delta.values()) == R.launches(T, c, h, w), (what, delta)
    if sweep_c is not None:
        assert lib.cine_diag_counter(D_SWEEP_C, 0) - calls == sweep_c, what
    if R.pair_shape(c, h, w):
        paired = delta.get("pair", 0) + delta.get("wide", 0)
        assert paired >= T - (T & 1) and (T & 1 or paired == T), (what, delta)
        if R.tile_width(w) != 16:
            assert delta.get("pair", 0) == T - (T & 1), (what, delta)
    else:
        assert "pair" not in delta, (what, delta)
    assert "plane" not in delta, (what, case, delta)
    mask = ops.conv_plane_mask()
    if off:
        assert set(delta) <= R.UNALIGNED_ROUTES, (what, case, off, delta)
    elif mask == 7:
        assert set(delta) == R.ROUTES_ALIGNED[case], (what, case, delta)
    else:
        cleared = {r for r, bit in LEAN.items() if not mask & bit}
        assert set(delta) <= R.GENERAL_ROUTES and set(delta) == {"pair", "general_vec"} - ({"pair"} if T == 1 else set()) and cleared, (what, case, mask, delta)
    _log_routes(f"{what} {case}", delta)
    return delta


def _log_routes(key, delta):
    log = ROUTE_LOG.setdefault(key, {})
    for r, v in delta.items():
        log[r] = log.get(r, 0) + v


def _route_counts():
    return [L().cine_diag_counter(D_FIRST + i, 0) for i in range(len(ROUTES))]


def _with_lean_off(case, delta, fn, what):
    """fn(routes) again with the cine_set_conv_plane bits of the lean routes in `delta` cleared: it must leave them for general routes (_counted
    asserts that under the cleared mask; here that the rerun was counted at all).  Exactly the rows of R.LEAN_CASES take a lean route; returns None
    for the others."""
    from cine_hip import ops
    bits = sum({LEAN[r] for r in delta if r in LEAN})
    assert bool(bits) == (case in R.LEAN_CASES), (what, case, delta)
    if not bits:
        return None
    routes = {}
    try:
        ops.set_conv_plane(7 & ~bits)
        res = fn(routes)
    finally:
        ops.set_conv_plane(7)
    assert routes and not set(routes) & set(LEAN) and set(routes) <= R.GENERAL_ROUTES, (what, case, delta, routes)
    return res


# ================================================================== 1. cine_bcrnn_sweep through the C ABI
@pytest.fixture(scope="module")
def packs(dev):
    """case -> (W on the device, its forward packing, its input-gradient packing)."""
    from cine_hip import ops
    cache = {}

    def get(case):
        if case not in cache:
            W = R.sweep_data(case).W.to(dev)
            cache[case] = (W, ops.pack_conv3x3(W), ops._pack("c3d", W))
            torch.cuda.synchronize()
        return cache[case]
    return get


def _sweep(dev, case, relu, keep, off, wp, routes=None):
    """cine_bcrnn_sweep twice on fresh guarded operands at storage offset `off`: [out, hf, hb] on the CPU."""
    T, ch, c, h, w, och = R.CASES[case]
    sd = R.sweep_data(case)
    what = f"cine_bcrnn_sweep {case} relu {relu} keep {keep} off {off}"

    def body(k):
        P, zero = k.inp(sd.P), k.inp(torch.zeros(c, h, w))
        k.ins.append((wp, wp.clone()))
        hf, hb, out = k.out((T if keep else 2, c, h, w)), k.out((T if keep else 2, c, h, w)), k.out((T, c, h, w))
        d = _counted(lambda: L().cine_bcrnn_sweep(P.data_ptr(), wp.data_ptr(), zero.data_ptr(), hf.ptr(), hb.ptr(), out.ptr(), T, c, h, w, relu, keep,
                                                  _stream()), T, c, h, w, "cine_bcrnn_sweep", case, off, sweep_c=1)
        if routes is not None:
            routes.update(d)
        return [out.t, hf.t, hb.t]
    return twice(dev, off, body, what)


SWEEP_RUNS = [(case, relu) for case in R.CASES for relu in (1, 0)]


@pytest.mark.parametrize("case,relu", SWEEP_RUNS, ids=[f"{c}-relu{r}" for c, r in SWEEP_RUNS])
def test_bcrnn_sweep(dev, packs, case, relu):
    T, ch, c, h, w, och = R.CASES[case]
    sd = R.sweep_data(case)
    _, wp, _ = packs(case)
    f64, f32 = R.sweep_forward(sd.P, sd.W, relu), R.sweep_forward(sd.P, sd.W, relu, torch.float32)
    routes = {}
    out1, hf1, hb1 = _sweep(dev, case, relu, 1, 0, wp, routes)
    out0, hf0, hb0 = _sweep(dev, case, relu, 0, 0, wp)
    for name, got in (("out", out1), ("hf", hf1), ("hb", hb1)):
        _record(f"cine_bcrnn_sweep {name}", got, getattr(f64, name), rel_err(getattr(f32, name), getattr(f64, name)), (case, relu))
    assert same_bits(out0, out1), "keep 0 and keep 1 give other bits"
    assert same_bits(out1, hf1 + hb1), "out is not hf + hb"
    # the ping-pong buffers: slot (T - 1) & 1 holds the last hidden state of each chain, the other slot the one before (T = 1: never written)
    last = (T - 1) & 1
    assert same_bits(hf0[last], hf1[T - 1]) and same_bits(hb0[last], hb1[0])
    if T > 1:
        assert same_bits(hf0[last ^ 1], hf1[T - 2]) and same_bits(hb0[last ^ 1], hb1[1])
    else:
        assert bool(torch.isnan(hf0[1]).all()) and bool(torch.isnan(hb0[1]).all())
    general = _with_lean_off(case, routes, lambda rr: _sweep(dev, case, relu, 1, 0, wp, rr), "cine_bcrnn_sweep")
    assert (general is not None) == (case in R.LEAN_CASES)
    if general is not None:
        assert all(same_bits(a, b) for a, b in zip(general, (out1, hf1, hb1))), f"the general route gives other bits than {sorted(routes)}"


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("case", R.OFFSET_CASES)
def test_bcrnn_sweep_at_storage_offsets(dev, packs, case, keep):
    _, wp, _ = packs(case)
    sd = R.sweep_data(case)
    T, ch, c, h, w, och = R.CASES[case]
    what = f"cine_bcrnn_sweep {case} keep {keep}"

    def body(k):
        P, zero = k.inp(sd.P), k.inp(torch.zeros(c, h, w))
        hf, hb, out = k.out((T if keep else 2, c, h, w)), k.out((T if keep else 2, c, h, w)), k.out((T, c, h, w))
        _counted(lambda: L().cine_bcrnn_sweep(P.data_ptr(), wp.data_ptr(), zero.data_ptr(), hf.ptr(), hb.ptr(), out.ptr(), T, c, h, w, 1, keep, _stream()),
                 T, c, h, w, "cine_bcrnn_sweep (offsets)", case, k.off)
        return [out.t] + ([hf.t, hb.t] if keep else [])
    at_offsets(dev, (0, 1, 2, 3), body, what)


# ================================================================== 2. cine_bcrnn_sweep_bwd through the C ABI
def _sweep_bwd(dev, case, relu, hf, hb, off, wd, routes=None, offs=None):
    """cine_bcrnn_sweep_bwd on gates hf / hb (CPU tensors): [gf, gb, gP] on the CPU (twice; at every offset of `offs`)."""
    T, ch, c, h, w, och = R.CASES[case]
    sd = R.sweep_data(case)

    def body(k):
        gout, zero, f, b = k.inp(sd.gout), k.inp(torch.zeros(c, h, w)), k.inp(hf), k.inp(hb)
        k.ins.append((wd, wd.clone()))
        gf, gb, gP = k.out((T, c, h, w)), k.out((T, c, h, w)), k.out((T, c, h, w))
        d = _counted(lambda: L().cine_bcrnn_sweep_bwd(gout.data_ptr(), wd.data_ptr(), zero.data_ptr(), f.data_ptr(), b.data_ptr(), gf.ptr(), gb.ptr(),
                                                      gP.ptr(), T, c, h, w, relu, _stream()), T, c, h, w, "cine_bcrnn_sweep_bwd", case, k.off, sweep_c=0)
        if routes is not None:
            routes.update(d)
        return [gf.t, gb.t, gP.t]
    what = f"cine_bcrnn_sweep_bwd {case} relu {relu}"
    return at_offsets(dev, offs, body, what) if offs else twice(dev, off, body, what)


def _check_bwd(case, relu, got, hf, hb, tag):
    sd = R.sweep_data(case)
    gates = (hf > 0, hb > 0) if relu else (None, None)
    b64, b32 = R.sweep_backward(sd.gout, sd.W, *gates), R.sweep_backward(sd.gout, sd.W, *gates, dtype=torch.float32)
    for name, g in zip(("gf", "gb", "gP"), got):
        _record(f"cine_bcrnn_sweep_bwd {name} ({tag})", g, getattr(b64, name), rel_err(getattr(b32, name), getattr(b64, name)), (case, relu))
    assert same_bits(got[2], got[0] + got[1]), "gP is not gf + gb"


@pytest.mark.parametrize("case,relu", SWEEP_RUNS, ids=[f"{c}-relu{r}" for c, r in SWEEP_RUNS])
def test_bcrnn_sweep_bwd(dev, packs, case, relu):
    T, ch, c, h, w, och = R.CASES[case]
    sd = R.sweep_data(case)
    _, wp, wd = packs(case)
    # gates from a real forward; the device's signs against the float64 ones
    _, hf, hb = _sweep(dev, case, relu, 1, 0, wp)
    if relu:
        f64, f32 = R.sweep_forward(sd.P, sd.W, relu), R.sweep_forward(sd.P, sd.W, relu, torch.float32)
        bars = {"hf": R.bar(rel_err(f32.pre_f, f64.pre_f)), "hb": R.bar(rel_err(f32.pre_b, f64.pre_b))}
        n = R.mask_condition({"hf": hf > 0, "hb": hb > 0}, {"hf": f64.pre_f, "hb": f64.pre_b}, bars)
        print(f"  {case}: {n} gate entries differ from the float64 signs")
    routes = {}
    real = _sweep_bwd(dev, case, relu, hf, hb, 0, wd, routes)
    _check_bwd(case, relu, real, hf, hb, "real gates")
    general = _with_lean_off(case, routes, lambda rr: _sweep_bwd(dev, case, relu, hf, hb, 0, wd, rr), "cine_bcrnn_sweep_bwd")
    assert (general is not None) == (case in R.LEAN_CASES)
    if general is not None:
        assert all(same_bits(a, b) for a, b in zip(general, real)), f"the general route gives other bits than {sorted(routes)}"
    # gates the test writes itself: +0.0, -0.0, the smallest subnormal, negatives -- only > 0 opens
    sf, sb = R.synthetic_gates(case)
    if relu:
        synth = _sweep_bwd(dev, case, relu, sf, sb, 0, wd)
        _check_bwd(case, relu, synth, sf, sb, "synthetic gates")
        assert not same_bits(synth[2], real[2])
    else:
        # relu = 0 ignores the gates: other gates, and NaN gates, change no bit
        for f, b in ((sf, sb), (torch.full_like(hf, NAN), torch.full_like(hb, NAN))):
            other = _sweep_bwd(dev, case, relu, f, b, 0, wd)
            assert all(same_bits(a, b_) for a, b_ in zip(other, real)), "relu = 0 read the gates"


@pytest.mark.parametrize("case", R.OFFSET_CASES)
def test_bcrnn_sweep_bwd_at_storage_offsets(dev, packs, case):
    _, _, wd = packs(case)
    sf, sb = R.synthetic_gates(case, 1)
    got = _sweep_bwd(dev, case, 1, sf, sb, 0, wd, offs=(0, 1, 2, 3))
    _check_bwd(case, 1, got, sf, sb, "offsets")


# ================================================================== 3. refusals
def _refusal_operands(dev, packs, bwd):
    case = "two"
    T, ch, c, h, w, och = R.CASES[case]
    sd = R.sweep_data(case)
    _, wp, wd = packs(case)
    k = Call(dev, 0)
    p = dict(zero=k.inp(torch.zeros(c, h, w)).data_ptr(), T=T, c=c, h=h, w_=w)
    if bwd:
        p.update(gout=k.inp(sd.gout).data_ptr(), w=wd.data_ptr(), hf=k.inp(sd.P).data_ptr(), hb=k.inp(sd.P * 0.5).data_ptr())
        p.update({n: k.out((T, c, h, w)).ptr() for n in ("gf", "gb", "gP")})
    else:
        p.update(P=k.inp(sd.P).data_ptr(), w=wp.data_ptr())
        p.update({n: k.out((T, c, h, w)).ptr() for n in ("hf", "hb", "out")})
    return k, p, 4 * (T - 1) * c * h * w


FWD, BWD = ("P", "w", "zero", "hf", "hb", "out"), ("gout", "w", "zero", "hf", "hb", "gf", "gb", "gP")


def _entry(bwd, p, keep=1):
    s = (p["T"], p["c"], p["h"], p["w_"])
    if bwd:
        return L().cine_bcrnn_sweep_bwd(*[p[n] for n in BWD], *s, 1, _stream())
    return L().cine_bcrnn_sweep(*[p[n] for n in FWD], *s, 1, keep, _stream())


@pytest.mark.parametrize("bwd", [False, True], ids=["sweep", "sweep_bwd"])
def test_refusals_leave_every_output_untouched(dev, packs, bwd):
    k, p, last = _refusal_operands(dev, packs, bwd)
    name = "cine_bcrnn_sweep_bwd" if bwd else "cine_bcrnn_sweep"
    for n in (BWD if bwd else FWD):
        for keep in (0, 1):
            refused(lambda: _entry(bwd, dict(p, **{n: None}), keep), EINVAL, k, f"{name} {n} NULL", name + ":")
    for n in ("T", "c", "h", "w_"):
        for v in (0, -1):
            refused(lambda: _entry(bwd, dict(p, **{n: v})), EINVAL, k, f"{name} {n} = {v}", name + ":")
    # aliased buffers: the first step refuses them under its own name before its launch (frames 0 and T - 1)
    if bwd:
        alias = [("gb", p["zero"], 1), ("gP", p["gb"], 1), ("gf", p["zero"] - last, 1), ("gP", p["zero"] - last, 1), ("gP", p["gf"], 1)]
    else:
        alias = [("hf", p["zero"], 0), ("hf", p["zero"], 1), ("out", p["zero"], 1), ("out", p["hf"], 0), ("hb", p["hf"], 0), ("hb", p["zero"] - last, 1),
                 ("hb", p["zero"], 0)]
    for n, v, keep in alias:
        refused(lambda: _entry(bwd, dict(p, **{n: v}), keep), EINVAL, k, f"{name} {n} aliased, keep {keep}", "cine_crnn_step2:")


# ================================================================== 4. the Python sequences
def _module(data, dev):
    from reconstruction.models.recurrent_common import CRNNBody
    T, ch, c, h, w, och = data.dims

    class Body(CRNNBody):
        def __init__(self):
            super().__init__()
            self.chans = c
            self._make_body(ch, c, och)
    m = Body().to(dev)
    with torch.no_grad():
        for p, v in zip(m._body_params(), data.params):
            p.copy_(v)
    return m


def _gates(node_out, body_fn):
    """hf, hb of the cascade that produced x0 (`node_out`), from the tensors its autograd node saved."""
    saved = node_out.grad_fn.saved_tensors
    assert len(saved) == (11 if body_fn else 6)
    hf, hb = (saved[9], saved[10]) if body_fn else (saved[4], saved[5])
    # the right two tensors: x0 is their sum (one float add), which no other pair of the saved tensors is
    assert hf.shape == hb.shape == node_out.shape and same_bits(hf + hb, node_out.detach()), "the saved tensors are not (.., hf, hb)"
    return hf, hb


def _step(m, data, dev, relu, body_fn=True, side_lane=True, in_c=True, backward=True, zero_grad=True, x_grad=(True, True)):
    """Two chained cascades through CRNNBody.body_train on one set of parameters, and the backward of sum_k <out_k, gout_k>: a namespace like
    R.chain's, with the device's masks."""
    from cine_hip import autograd as ag, ops
    T, ch, c, h, w, och = data.dims
    old = (ag.CRNN_BODY_FN, ag.CRNN_SIDE_LANE, ops.BCRNN_SWEEP_IN_C)
    ag.CRNN_BODY_FN, ag.CRNN_SIDE_LANE, ops.BCRNN_SWEEP_IN_C = body_fn, side_lane, in_c
    try:
        if zero_grad:
            m.zero_grad(set_to_none=True)
        xs = [v.to(dev).view(T, 1, ch, h, w).requires_grad_(g) for v, g in zip(data.xs, x_grad)]
        res = [data.res[0].to(dev).requires_grad_(True), data.res[1].to(dev)]           # need[5] on and off
        with ops.activation(relu=relu), torch.enable_grad():
            state = m.zero_state(T, 1, h, w, xs[0])
            assert not any(s.requires_grad for s in state)
            outs, feats, masks = [], [], []
            for x, r in zip(xs, res):
                out, state = m.body_train(x, state, r)
                outs.append(out); feats.append(state)
                hf, hb = _gates(state[0], body_fn)
                masks.append({"hf": (hf > 0).cpu(), "hb": (hb > 0).cpu(), **{f"x{k}": (state[k] > 0).cpu() for k in (1, 2, 3)}})
            if backward:
                torch.autograd.backward(outs, [g.to(dev) for g in data.gouts])
        torch.cuda.synchronize()
    finally:
        ag.CRNN_BODY_FN, ag.CRNN_SIDE_LANE, ops.BCRNN_SWEEP_IN_C = old
    r = SimpleNamespace(outs=[o.detach() for o in outs], feats=[[f.detach() for f in fs] for fs in feats], masks=masks)
    if backward:
        assert res[1].grad is None
        assert all((x.grad is not None) == g for x, g in zip(xs, x_grad))
        r.gx, r.gres = [x.grad.view(T, ch, h, w) if g else None for x, g in zip(xs, x_grad)], [res[0].grad]      # (the second residual takes no gradient)
        r.gp = [p.grad for p in m._body_params()]
    return r


def _tensors(run):
    return {k: v.detach().cpu() for k, v in R.chain_tensors(run).items() if v is not None}


def _same(a, b, what, absent=()):
    """Every tensor of step b has the bits of step a's; `absent`: the tensors b must not have (an input that takes no gradient)."""
    ta, tb = _tensors(a), _tensors(b)
    assert set(ta) - set(tb) == set(absent) and set(tb) <= set(ta), (what, set(ta) ^ set(tb))
    bad = [k for k in tb if not same_bits(ta[k].float(), tb[k].float())]
    assert not bad, (what, bad)


BODY_RUNS = [(case, relu) for case in R.BODY_CASES for relu in (True, False)]
_STEPS = {}


def _steps(dev, case, relu):
    """Per run, once: the module, the step with CrnnBodyFn, the step with one node per layer, and the float64 reference under each one's masks."""
    key = (case, relu)
    if key not in _STEPS:
        data = R.body_data(case)
        m = _module(data, dev)
        before = _route_counts()
        on = _step(m, data, dev, relu, body_fn=True)
        delta = {r: a - b for r, a, b in zip(ROUTES, _route_counts(), before) if a != b}
        # the whole step (forward convs, sweeps, gated dgrads): never the plane-wide kernel; the column tiles exactly on the lean rows
        assert delta and "plane" not in delta and ("wide" in delta) == (case in R.LEAN_CASES), (case, delta)
        _log_routes(f"CrnnBodyFn step (forward and dgrads) {case}", delta)
        off = _step(m, data, dev, relu, body_fn=False)
        _STEPS[key] = (data, m, on, off)
    return _STEPS[key]


def _against_float64(data, run, relu, what, case):
    if relu:
        differ = sum(R.mask_condition(ms, pre64, bars) for (pre64, bars), ms in zip(R.pre_bars(data, relu), run.masks))
        print(f"  {what} {case}: {differ} mask entries differ from the float64 signs")
    r64, e32 = R.measured(data, run.masks if relu else None, relu)
    want = R.chain_tensors(r64)
    got = _tensors(run)
    assert set(got) == set(want) - {"gres1"}
    for k in got:
        name = "x" if k[0] == "x" else "g_w" if k.startswith("g_w") else "g_b" if k.startswith("g_b") else k.rstrip("01")
        _record(f"{what} {name}", got[k], want[k], e32[k], (case, relu, k))


@pytest.mark.parametrize("case,relu", BODY_RUNS, ids=[f"{c}-relu{int(r)}" for c, r in BODY_RUNS])
def test_crnn_body_fn_two_cascades(dev, case, relu):
    """ag.CrnnBodyFn: both outputs, both states, both input gradients, the residual's and all 20 parameter gradients."""
    data, m, on, off = _steps(dev, case, relu)
    _against_float64(data, on, relu, "CrnnBodyFn", case)
    if data.dims[0] == 1:
        assert float(on.gp[2].abs().max()) == 0


@pytest.mark.parametrize("case,relu", BODY_RUNS, ids=[f"{c}-relu{int(r)}" for c, r in BODY_RUNS])
def test_one_node_per_layer_two_cascades(dev, case, relu):
    """ag.CRNN_BODY_FN off (BcrnnFn + ConvSumFn per layer) at the same bar; the two paths agree at the bar (bits are not promised)."""
    data, m, on, off = _steps(dev, case, relu)
    _against_float64(data, off, relu, "BcrnnFn+ConvSumFn", case)
    _, e32 = R.measured(data, on.masks if relu else None, relu)
    a, b = _tensors(on), _tensors(off)
    # the two forwards are the same launches: the same masks, so every gradient is comparable
    assert all(torch.equal(x[k], y[k]) for x, y in zip(on.masks, off.masks) for k in x), "the two paths' ReLU masks differ"
    assert set(a) == set(b)
    for k in a:
        if float(a[k].abs().max()) == 0:
            assert float(b[k].abs().max()) == 0, k
        else:
            WORST.record("CrnnBodyFn vs one node per layer", rel_err(b[k], a[k]), R.bar(e32[k]), (case, relu, k))


@pytest.mark.parametrize("case", R.BODY_CASES)
def test_side_lane_and_sweep_in_c_change_no_bit(dev, case):
    data, m, on, off = _steps(dev, case, True)
    _same(on, _step(m, data, dev, True, side_lane=False), "CRNN_SIDE_LANE off")
    _same(off, _step(m, data, dev, True, body_fn=False, in_c=False), "BCRNN_SWEEP_IN_C off inside BcrnnFn")
    # determinism of the whole two-cascade step
    _same(on, _step(m, data, dev, True), "a second step")
    # an input that takes no gradient (need[0] off in that cascade's node: no i2h dgrad launch) changes no other bit, in either cascade
    _same(on, _step(m, data, dev, True, x_grad=(False, True)), "x of cascade 1 without a gradient", absent=("gx0",))
    _same(on, _step(m, data, dev, True, x_grad=(True, False)), "x of cascade 2 without a gradient", absent=("gx1",))


@pytest.mark.parametrize("case,relu", BODY_RUNS, ids=[f"{c}-relu{int(r)}" for c, r in BODY_RUNS])
def test_inference_is_the_training_forward(dev, case, relu):
    """CRNNBody.body (BCRNNlayer.forward inside, the keep = 0 sweep) chained over two cascades: against float64 at the bar, and the bits of the
    training forward (_body_packed and _train_packs pack the same concatenations; the launches are the same)."""
    from cine_hip import ops
    data, m, on, off = _steps(dev, case, relu)
    T, ch, c, h, w, och = data.dims
    lib = L()
    with ops.activation(relu=relu):
        state = m.zero_state(T, 1, h, w, data.xs[0].to(dev))
        outs, feats = [], []
        calls = lib.cine_diag_counter(D_SWEEP_C, 0)
        for x, r in zip(data.xs, data.res):
            out, state = m.body(x.to(dev).view(T, 1, ch, h, w), state, r.to(dev))
            outs.append(out); feats.append(state)
        torch.cuda.synchronize()
        assert lib.cine_diag_counter(D_SWEEP_C, 0) - calls == 2
    r64, e32 = R.measured(data, None, relu, grads=False)
    for k in range(2):
        _record("CRNNBody.body out", outs[k].cpu(), r64.outs[k], e32[f"out{k}"], (case, relu, k))
        assert same_bits(outs[k], on.outs[k]), "inference and training forward differ"
        for j in range(4):
            _record("CRNNBody.body x", feats[k][j].cpu(), r64.feats[k][j], e32[f"x{j}_{k}"], (case, relu, k, j))
            assert same_bits(feats[k][j], on.feats[k][j])


def test_accumulation_and_gradient_storage(dev):
    """Two backward() calls without zeroing give exactly twice the gradients (a + a is exact); no two parameters' .grad share storage, although
    CrnnBodyFn.backward returns one tensor for three biases and one for two, all views of one flat buffer."""
    data, m, on, off = _steps(dev, "ragged", True)
    once = _step(m, data, dev, True)
    grads = [p.grad for p in m._body_params()]
    assert all(g.is_contiguous() for g in grads)
    spans = sorted((g.data_ptr(), g.data_ptr() + 4 * g.numel()) for g in grads)
    assert all(end <= nxt for (_, end), (nxt, _) in zip(spans, spans[1:])), "two parameters' gradients overlap in memory"
    first = [g.clone() for g in grads]
    again = _step(m, data, dev, True, zero_grad=False)
    for p, f in zip(m._body_params(), first):
        assert same_bits(p.grad, f + f)
    for a, b in zip(once.gx, again.gx):
        assert same_bits(a, b)
    # writing to one bias gradient changes no other
    cell = m.bcrnn.CRNN_model
    keep = [cell.h2h.bias.grad.clone(), cell.ih2ih.bias.grad.clone(), m.conv1_h.bias.grad.clone()]
    cell.i2h.bias.grad.add_(1.0); m.conv1_x.bias.grad.add_(1.0)
    assert same_bits(cell.h2h.bias.grad, keep[0]) and same_bits(cell.ih2ih.bias.grad, keep[1]) and same_bits(m.conv1_h.bias.grad, keep[2])
    m.zero_grad(set_to_none=True)


def test_bcrnn_layer_with_batch_two_vs_the_oracle_module(dev):
    """BCRNNlayer.forward with b = 2 on `ragged`: the Python step loop with n = 2 per chain, against the oracle module in float64."""
    from oracle import recurrent_ref as O
    data, m, _, _ = _steps(dev, "ragged", True)
    T, ch, c, h, w, och = data.dims
    x = torch.stack([data.xs[0], data.xs[1]], 1)                                            # (T, 2, ch, h, w)
    hid = torch.stack([R._rand(np.random.RandomState(77 + b), T, c, h, w) for b in range(2)], 1)
    ref = O.BCRNNlayer(ch, c, 3).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in m.bcrnn.state_dict().items()})
    want = ref(x.double(), hid.double())
    want32 = ref.float()(x, hid)
    lib = L()
    calls = lib.cine_diag_counter(D_SWEEP_C, 0)
    got = m.bcrnn(x.to(dev), hid.to(dev))
    torch.cuda.synchronize()
    assert lib.cine_diag_counter(D_SWEEP_C, 0) == calls, "b = 2 must run the Python step loop"
    _record("BCRNNlayer.forward b = 2", got.cpu(), want, rel_err(want32, want), "ragged")
    # ... and with b = 1 the C sweep, against the same oracle
    got1 = m.bcrnn(x[:, :1].to(dev).contiguous(), hid[:, :1].to(dev).contiguous())
    assert lib.cine_diag_counter(D_SWEEP_C, 0) == calls + 1
    want1 = ref.double()(x[:, :1].double(), hid[:, :1].double())
    _record("BCRNNlayer.forward b = 1", got1.cpu(), want1, rel_err(ref.float()(x[:, :1], hid[:, :1]), want1), "ragged")


def test_crnn_cell_vs_the_oracle_cell(dev):
    from oracle import recurrent_ref as O
    data, m, _, _ = _steps(dev, "ragged", True)
    T, ch, c, h, w, och = data.dims
    cell = m.bcrnn.CRNN_model
    ref = O.CRNNcell(ch, c, 3).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in cell.state_dict().items()})
    rs = np.random.RandomState(91)
    x, hi, hid = data.xs[0], R._rand(rs, T, c, h, w), R._rand(rs, T, c, h, w)
    want = ref(x.double(), hi.double(), hid.double())
    want32 = ref.float()(x, hi, hid)
    got = cell(x.to(dev), hi.to(dev), hid.to(dev))
    _record("CRNNcell.forward", got.cpu(), want, rel_err(want32, want), "ragged")
