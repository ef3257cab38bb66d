"""The parts of the CRNN launch-sequence sweep that need no GPU: the yardstick of tests/crnn_reference.py against oracle/recurrent_ref (values and
gradients, two chained cascades), the masked ReLU under its own signs, the two caps of the mask condition and 2 e32 <= BAR_CAP for the float32
run of every case (so the cap of the bar never passes anything), what each row of the table is there for (tile tier, padded rows, the pair
configuration on both sides of 200, launch counts, T in {1, 2, odd, even}), the header's cine_crnn_* / cine_bcrnn_* entry points all being
called by a sweep, and the refusals that return before any launch, with made-up addresses."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import crnn_reference as R
from kernel_sweep import BAR_CAP

EINVAL = -1


def L():
    from cine_hip._lib import lib
    return lib()


def _oracle_body(data):
    from oracle import recurrent_ref as O
    T, ch, c, h, w, och = data.dims

    class Body(O._CRNNBody):
        def __init__(self):
            super().__init__()
            self.chans = c
            self._make_body(ch, c, och)
    m = Body().double()
    cell = m.bcrnn.CRNN_model
    ps = [cell.ih2ih.weight, cell.i2h.weight, cell.h2h.weight, cell.i2h.bias, cell.h2h.bias, cell.ih2ih.bias]
    for k in (1, 2, 3):
        cx, chh = getattr(m, f"conv{k}_x"), getattr(m, f"conv{k}_h")
        ps += [cx.weight, chh.weight, cx.bias, chh.bias]
    ps += [m.conv4_x.weight, m.conv4_x.bias]
    with torch.no_grad():
        for p, v in zip(ps, data.params):
            p.copy_(v.double())
    return m, ps


# ================================================================== the yardstick
@pytest.mark.parametrize("case", ["ragged", "two", "one", "rows32"])
def test_the_yardstick_is_the_oracle_chained_over_two_cascades(case):
    """m = None: oracle _CRNNBody._body (BCRNNlayer inside) as VarNet_RNN chains it -- the state of a cascade is [x0..x3] of the one before, zeros
    first -- in float64: outputs, states, and the gradients of both inputs, both residuals and all 20 shared parameters, to 1e-12."""
    data = R.body_data(case)
    T, ch, c, h, w, och = data.dims
    mine = R.chain(data)
    m, ps = _oracle_body(data)
    xs = [v.double().requires_grad_(True) for v in data.xs]
    res = [v.double().requires_grad_(True) for v in data.res]
    with torch.enable_grad():
        state = m._zero_state(T, 1, h, w, xs[0])
        outs, feats = [], []
        for x, r in zip(xs, res):
            x4, state = m._body(x.view(T, 1, ch, h, w), state)
            outs.append(x4 + r); feats.append(state)
        torch.autograd.backward(outs, [g.double() for g in data.gouts])
    want = {}
    for k in range(2):
        want[f"out{k}"] = outs[k].detach()
        want.update({f"x{j}_{k}": f.detach() for j, f in enumerate(feats[k])})
        want[f"gx{k}"], want[f"gres{k}"] = xs[k].grad, res[k].grad
    want.update({f"g_{n}": p.grad for n, p in zip(R.PARAM_NAMES, ps)})
    errs = R.errors(R.chain_tensors(mine), want)
    assert set(errs) == set(R.chain_tensors(mine)) and len(errs) == 2 * 7 + 20
    assert max(errs.values()) <= 1e-12, errs
    if T == 1:
        assert float(mine.gp[2].abs().max()) == 0            # gw_hh: every chain starts from zeros and ends at once


@pytest.mark.parametrize("relu", [True, False])
def test_the_sweeps_alone_are_the_layer_and_its_autograd(relu):
    """sweep_forward on P = i2h(x) + ih2ih(s0) + the three biases is the BCRNN layer; sweep_backward's recursion gives the gradients autograd
    gives: gf = d <hf, gout> / dP, gb = d <hb, gout> / dP, gP = d <out, gout> / dP."""
    data, sd = R.body_data("ragged"), R.sweep_data("ragged")
    p = [v.double() for v in data.params]
    x, s0 = data.xs[0].double(), data.xs[1].double()[:, :1].expand(-1, p[0].shape[1], -1, -1).contiguous()
    x0, pre_f, pre_b = R.bcrnn(x, s0, p, None, relu)
    P = F.conv2d(x, p[1], p[3], padding=1) + F.conv2d(s0, p[0], p[5], padding=1) + p[4].view(1, -1, 1, 1)
    f = R.sweep_forward(P, p[2], relu)
    assert R.rel_err(f.out, x0) <= 1e-12 and R.rel_err(f.pre_f, pre_f) <= 1e-12 and R.rel_err(f.pre_b, pre_b) <= 1e-12
    Pg = sd.P.double().requires_grad_(True)
    with torch.enable_grad():
        g = R.sweep_forward(Pg, sd.W, relu)
        gout = sd.gout.double()
        want = [torch.autograd.grad((t * gout).sum(), Pg, retain_graph=True)[0] for t in (g.hf, g.hb, g.out)]
    b = R.sweep_backward(sd.gout, sd.W, g.hf.detach() > 0 if relu else None, g.hb.detach() > 0 if relu else None)
    for got, ref in zip((b.gf, b.gb, b.gP), want):
        assert R.rel_err(got, ref) <= 1e-12


@pytest.mark.parametrize("case", ["ragged", "two"])
def test_masks_equal_to_its_own_signs_reproduce_the_plain_gradients_exactly(case):
    data = R.body_data(case)
    plain = R.chain(data)
    masked = R.chain(data, masks=R.own_masks(plain))
    a, b = R.chain_tensors(plain), R.chain_tensors(masked)
    assert all(torch.equal(a[k], b[k]) for k in a)
    # ... and a mask does change the backward (and only the backward)
    flipped = R.chain(data, masks=[{k: ~m for k, m in ms.items()} for ms in R.own_masks(plain)])
    c = R.chain_tensors(flipped)
    assert torch.equal(c["out1"], a["out1"]) and not torch.equal(c["gx0"], a["gx0"])


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", R.BODY_CASES)
def test_the_caps_hold_for_the_float32_run_of_the_body(case, relu):
    """The float32 run's masks against the float64 signs meet the mask condition; under those masks 2 e32 <= BAR_CAP for every tensor."""
    data = R.body_data(case)
    r32 = R.chain(data, torch.float32, None, relu, False)
    differ = 0
    if relu:
        for (pre64, bars), ms in zip(R.pre_bars(data, relu), R.own_masks(r32)):
            differ += R.mask_condition(ms, pre64, bars)
    r64, e32 = R.measured(data, R.own_masks(r32) if relu else None, relu)
    worst = max(e32, key=e32.get)
    print(f"{case} relu {int(relu)}: {differ} mask entries differ; e32 {min(e32.values()):.1e} .. {e32[worst]:.1e} ({worst})")
    assert all(2 * e <= BAR_CAP for e in e32.values()), e32
    for k, t in R.chain_tensors(r64).items():
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()) and (float(t.abs().max()) > 0 or (k == "g_w_h2h" and data.dims[0] == 1)), k


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("case", list(R.CASES))
def test_the_caps_hold_for_the_float32_run_of_the_sweeps(case, relu):
    sd = R.sweep_data(case)
    f64, f32 = R.sweep_forward(sd.P, sd.W, relu), R.sweep_forward(sd.P, sd.W, relu, torch.float32)
    e = {k: R.rel_err(getattr(f32, k), getattr(f64, k)) for k in ("hf", "hb", "out", "pre_f", "pre_b")}
    gates = (f32.hf > 0, f32.hb > 0) if relu else (None, None)
    differ = R.mask_condition({"hf": gates[0], "hb": gates[1]}, {"hf": f64.pre_f, "hb": f64.pre_b}, {"hf": R.bar(e["pre_f"]), "hb": R.bar(e["pre_b"])}) if relu else 0
    b64, b32 = R.sweep_backward(sd.gout, sd.W, *gates), R.sweep_backward(sd.gout, sd.W, *gates, dtype=torch.float32)
    e.update({k: R.rel_err(getattr(b32, k), getattr(b64, k)) for k in ("gf", "gb", "gP")})
    print(f"{case} relu {int(relu)}: {differ} gate entries differ; e32 " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert all(2 * v <= BAR_CAP for v in e.values()), e
    sg = R.synthetic_gates(case)
    for g in sg:
        for t in range(g.shape[0]):
            fr = g[t].flatten()
            bits = fr.view(torch.int32)
            assert bool((bits == 0).any()) and bool((bits == -2 ** 31).any()) and bool((bits == 1).any()) and bool((fr < 0).any()) and bool((fr > 1).any())
    assert bool(((sg[0] > 0) != (sg[1] > 0)).any())


# ================================================================== what the rows are there for
def test_the_table_reaches_every_axis_value_it_claims():
    C = R.CASES
    assert {R.tile_width(C[k][4]) for k in ("w2", "w4", "w8", "plane16")} == {2, 4, 8, 16} and all(C[k][4] == R.tile_width(C[k][4]) for k in ("w2", "w4", "w8", "plane16"))
    assert C["cfg"][4] > 16 and C["cfg"][4] % 4 == 0 and C["ragged"][4] % 2 == 1
    assert {k: R.padded_rows(C[k][2]) for k in ("cfg", "ragged", "rows32", "xpd")} == {"cfg": 16, "ragged": 16, "rows32": 32, "xpd": 32}
    # the frags rule of crnn_step2_impl on both sides of 200
    assert R.frags(396, 208) == 396 * 13 and R.pair_area(396, 208) == 198 and R.pair_area(400, 208) == 200
    assert R.pair_shape(*C["area-in"][2:5]) and not R.pair_shape(*C["area-out"][2:5]) and R.padded_rows(C["area-out"][2]) == 16
    two_launch = {k for k, t in C.items() if not R.pair_shape(*t[2:5])}
    assert two_launch == {"rows32", "xpd", "area-out"}
    # launch counts: T, T + 1 for odd T, 2 T outside the pair configuration
    want = {"cfg": 6, "plane16": 4, "long": 16, "ragged": 4, "rows32": 8, "xpd": 10, "w2": 4, "w4": 4, "w8": 4, "one": 2, "two": 2, "area-in": 2, "area-out": 4}
    assert {k: R.launches(t[0], *t[2:5]) for k, t in C.items()} == want
    Ts = {t[0] for t in C.values()}
    assert {1, 2, 15} <= Ts and any(T % 2 == 1 and T > 1 for T in Ts) and any(T % 2 == 0 and T > 2 for T in Ts)
    assert (C["xpd"][1], C["xpd"][5], C["xpd"][2]) == (2 * (5 + 1), 2 * 5, 18)
    assert set(R.BODY_CASES) <= set(C) - set(R.SWEEP_ONLY) and set(R.OFFSET_CASES) <= set(C)
    # the routes the GPU file asserts: every row has them; pair launches exactly on the pair shapes with a step before the crossing; the lean
    # (column-tile) rows are W > 16 with whole 16-byte rows, one of them among the body cases and one among the offset cases
    assert set(R.ROUTES_ALIGNED) == set(C) and not any("plane" in v for v in R.ROUTES_ALIGNED.values())
    for k, t in C.items():
        r = R.ROUTES_ALIGNED[k]
        assert r and r <= R.GENERAL_ROUTES | set(R.LEAN_ROUTES)
        if not R.pair_shape(*t[2:5]) or t[0] == 1:
            assert "pair" not in r, k
        elif "wide" not in r:
            assert "pair" in r, k
    assert set(R.LEAN_CASES) == {"cfg", "one"} and all(C[k][4] > 16 and C[k][4] % 4 == 0 for k in R.LEAN_CASES)
    assert set(R.LEAN_CASES) & set(R.BODY_CASES) and set(R.LEAN_CASES) & set(R.OFFSET_CASES)
    # unaligned frames: a frame of `ragged` is not a whole number of 16-byte pieces
    assert (C["ragged"][2] * C["ragged"][3] * C["ragged"][4]) % 4 != 0
    # the restated rule is the one in the source
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "deep-cine-cardiac-mri_amd", "csrc", "conv_kernels.hip")) as f:
        src = f.read()
    assert "a.rowsp <= 16 && 2L * n * ceil_div(frags, 52L) < 200 && !gate_f == !gate_b" in src
    assert "const long frags = (long)ceil_div(h * TW, 16) * ceil_div(w, TW);" in src


def test_every_crnn_entry_point_of_the_header_is_called_by_a_sweep():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "cine_hip.h")) as f:
        names = set(re.findall(r"\b(cine_b?crnn_\w+)\s*\(", f.read()))
    assert names == {"cine_crnn_step", "cine_crnn_step2", "cine_bcrnn_sweep", "cine_bcrnn_sweep_bwd"}, sorted(names)
    text = ""
    for fn in ("test_crnn_sequences.py", "test_conv_fwd_kernels.py"):
        with open(os.path.join(here, fn)) as f:
            text += f.read()
    missing = [n for n in names if not re.search(rf"\bL\(?\)?\.{n}\b|lib\.{n}\b", text)]
    assert not missing, missing


# ================================================================== refusals (all before the first launch)
FAKE = dict(P=0x10000, w=0x20000, zero=0x30000, hf=0x40000, hb=0x50000, out=0x60000, gout=0x70000, gf=0x80000, gb=0x90000, gP=0xA0000)
FWD, BWD = ("P", "w", "zero", "hf", "hb", "out"), ("gout", "w", "zero", "hf", "hb", "gf", "gb", "gP")
SIZES = dict(T=3, c=4, h=6, w_=5)


def _call(lib, bwd, ptrs, sizes, relu=1, keep=1):
    s = (sizes["T"], sizes["c"], sizes["h"], sizes["w_"])
    if bwd:
        return lib.cine_bcrnn_sweep_bwd(*[ptrs[k] for k in BWD], *s, relu, None)
    return lib.cine_bcrnn_sweep(*[ptrs[k] for k in FWD], *s, relu, keep, None)


def _refused(lib, bwd, ptrs, sizes, name, what, **kw):
    assert lib.cine_scale(None, 1, 1.0, None) == EINVAL and lib.cine_last_error().startswith(b"cine_scale")
    code = _call(lib, bwd, ptrs, sizes, **kw)
    msg = lib.cine_last_error().decode(errors="replace")
    assert code == EINVAL and msg.startswith(name), (what, code, msg)


@pytest.mark.parametrize("bwd", [False, True], ids=["sweep", "sweep_bwd"])
def test_refusals_before_any_launch(bwd):
    lib = L()
    name = "cine_bcrnn_sweep_bwd:" if bwd else "cine_bcrnn_sweep:"
    for k in (BWD if bwd else FWD):
        for keep in (0, 1):
            _refused(lib, bwd, dict(FAKE, **{k: None}), SIZES, name, f"{k} NULL", keep=keep)
    for k in SIZES:
        for v in (0, -1):
            _refused(lib, bwd, FAKE, dict(SIZES, **{k: v}), name, f"{k} = {v}")
    # aliased buffers: refused by the FIRST step (frames 0 and T - 1) under the step's name, before its launch
    last = 4 * (SIZES["T"] - 1) * SIZES["c"] * SIZES["h"] * SIZES["w_"]                # byte offset of frame T - 1
    if bwd:
        alias = [("gb", FAKE["zero"], 1), ("gP", FAKE["gb"], 1), ("gf", FAKE["zero"] - last, 1), ("gP", FAKE["zero"] - last, 1), ("gP", FAKE["gf"], 1)]
    else:
        alias = [("hf", FAKE["zero"], 0), ("hf", FAKE["zero"], 1), ("out", FAKE["zero"], 1), ("out", FAKE["hf"], 0), ("hb", FAKE["hf"], 0),
                 ("hb", FAKE["zero"] - last, 1), ("hb", FAKE["zero"], 0)]
    for a, v, keep in alias:
        _refused(lib, bwd, dict(FAKE, **{a: v}), SIZES, "cine_crnn_step2:", f"{a} = {v:#x} keep {keep}", keep=keep)
