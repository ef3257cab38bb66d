"""The whole-network launch sequences of csrc/mwcnn.hip through the C ABI -- cine_mwcnn_forward, cine_mwcnn_forward2, cine_mwcnn_forward_train,
cine_mwcnn_backward with their three *_ws_bytes queries and cine_set_side_stream -- against oracle/xpdnet_ref.MWCNN in float64 under autograd
(tests/mwcnn_reference.py: the case table, the runs, the bar).

Every call writes guarded outputs and takes a workspace of exactly the size the library reports, filled with 0xFF bytes (NaN) unless stated, with
a sentinel tail.  Per run: the forward and every gradient at the bar min(BAR_CAP, max(BAR, 2 e32)) on the relative L2 error (e32: the float32
oracle against the float64 one; the CPU file asserts the cap never decides); the bit identities the binding relies on (training forward ==
inference forward; two sets == the two one-set passes concatenated; the same network in both sets == one set; gx = NULL changes no gradient;
a side stream changes nothing; a second call gives the same bits); the accumulation contract of `grads`; inputs and the forward workspace
unchanged; no dependence on what a workspace held (0x00 against 0xFF fill), also at a base pointer 64 bytes past a 256-byte boundary;
every refusal with its outputs untouched.  The module, autograd.mwcnn and ops.mwcnn_forward under ops.branches(2) once each at `ragged`."""
import pytest
import torch

import mwcnn_reference as R
from kernel_sweep import NAN, Call, Guarded, Workspace, Worst, refused, same_bits, twice

pytestmark = pytest.mark.gpu
WORST = Worst()
D_FIRST, D_LAST = 4, 12                                               # cine_diag_counter (csrc/common.h: Diag D_CONV_PLANE .. D_CONV_GENERAL_ELEM)
ROUTES = ["plane", "tconv-plane", "wide", "wide-v3", "coarse", "conv1x1-stream", "pair", "general-vec", "general-elem"]
_NETS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    L().cine_set_side_stream(None)
    yield torch.device("cuda:0")
    L().cine_set_side_stream(None)
    if WORST:
        WORST.report()


def L():
    from cine_hip._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nets(ref, dev):
    """The packed pointer arrays of a reference's networks, made once per run."""
    key = id(ref)
    if key not in _NETS:
        _NETS[key] = (ref, [R.DeviceNet(nt, dev) for nt in ref.nets])
    return _NETS[key][1]


def _dims(ref, **over):
    return R.dims(ref.case, n=ref.dims[0], slope=ref.slope, **over)


def _forward(dev, ref, x, entry, nets, split=None, fill=0xFF, past256=None, a=None):
    """One forward call (entry: "f" cine_mwcnn_forward, "2" forward2, "t" forward_train) on x (device): (y, workspace) after the guard checks."""
    lib, a = L(), a or _dims(ref)
    a.n = x.shape[0]
    inf, train, _ = R.ws_sizes(lib, a)
    ws = Workspace(train if entry == "t" else inf, dev, past256)
    ws.buf[:ws.nbytes] = fill
    y = Guarded((a.n, a.cout, a.h, a.w), 0, dev)
    y.t.fill_(NAN)
    w2 = nets[1].weights if len(nets) > 1 else None
    if entry == "f":
        code = R.call_forward(lib, a, x.data_ptr(), y.ptr(), nets[0].weights, ws.ptr(), ws.nbytes, _stream())
    elif entry == "2":
        code = R.call_forward2(lib, a, x.data_ptr(), y.ptr(), nets[0].weights, w2, split, ws.ptr(), ws.nbytes, _stream())
    else:
        code = R.call_forward_train(lib, a, x.data_ptr(), y.ptr(), nets[0].weights, w2, split if w2 else a.n, ws.ptr(), ws.nbytes, _stream())
    assert code == 0, (R.ENTRY[entry], code, lib.cine_last_error())
    torch.cuda.synchronize()
    assert y.intact() and ws.intact(), f"{R.ENTRY[entry]}: write outside the output or past the workspace"
    return y.t, ws


def _zero_grads(nets, dev):
    out = []
    for nt in nets:
        gl = [Guarded(tuple(p.shape), 0, dev) for p in nt.params]
        for g in gl:
            g.t.zero_()
        out.append(gl)
    return out


def _backward(dev, ref, x, gy, nets, fwd_ws, split=None, grads=None, want_gx=True, fill=0xFF, past256=None):
    """One cine_mwcnn_backward call: (gx | None, grads[net][slot] as Guarded) after the guard checks; `grads` given: accumulated into."""
    lib, a = L(), _dims(ref)
    _, _, need = R.ws_sizes(lib, a)
    ws = Workspace(need, dev, past256)
    ws.buf[:ws.nbytes] = fill
    grads = grads or _zero_grads(nets, dev)
    gx = Guarded(tuple(x.shape), 0, dev) if want_gx else None
    if gx is not None:
        gx.t.fill_(NAN)
    two = len(nets) > 1
    garr = [R.ptr_array([g.ptr() for g in gl]) for gl in grads]
    code = R.call_backward(lib, a, x.data_ptr(), gy.data_ptr(), nets[0].wdgrad, nets[1].wdgrad if two else None, garr[0], garr[1] if two else None,
                           split if two else a.n, fwd_ws.ptr(), fwd_ws.nbytes, ws.ptr(), ws.nbytes, gx.ptr() if gx else None, _stream())
    assert code == 0, (code, lib.cine_last_error())
    torch.cuda.synchronize()
    assert ws.intact() and fwd_ws.intact() and (gx is None or gx.intact()) and all(g.intact() for gl in grads for g in gl), \
        "cine_mwcnn_backward: write outside an output or past a workspace"
    return (gx.t if gx else None), grads


def _record(what, got, want, e32, case):
    err, b = R.rel_l2(got.detach().cpu(), want), R.bar(e32)
    print(f"  {what:34s} {case}: error {err:.2e}, float32 oracle {e32:.2e}, bar {b:.1e}")
    WORST.record(what, err, b, case)


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


# ================================================================== every run: forward, backward, identities
@pytest.mark.parametrize("run", R.RUNS, ids=[R.run_id(r) for r in R.RUNS])
def test_forward_and_backward_vs_float64(dev, run):
    ref = R.reference(*run)
    nets, k, rid = _nets(ref, dev), ref.split, R.run_id(run)
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    x0, gy0 = x.clone(), gy.clone()
    # ---- forward
    if k is None:
        y, _ = _forward(dev, ref, x, "f", nets)
        _record("cine_mwcnn_forward", y, ref.y, ref.e32.y, rid)
    else:
        y, _ = _forward(dev, ref, x, "2", nets, k)
        _record("cine_mwcnn_forward2", y, ref.y, ref.e32.y, rid)
        parts = [_forward(dev, ref, x[lo:hi].clone(), "f", [nt])[0] for lo, hi, nt in ((0, k, nets[0]), (k, x.shape[0], nets[1]))]
        assert same_bits(y, torch.cat(parts)), "cine_mwcnn_forward2: not the bits of the two one-set passes"
        same, _ = _forward(dev, ref, x, "2", [nets[0], nets[0]], k)
        one, _ = _forward(dev, ref, x, "f", nets[:1])
        assert same_bits(same, one), "cine_mwcnn_forward2 with one network in both sets: not the bits of cine_mwcnn_forward"
    yt, fwd_ws = _forward(dev, ref, x, "t", nets, k)
    assert same_bits(yt, y), "cine_mwcnn_forward_train: y differs from the inference forward's"
    # ---- backward
    kept = fwd_ws.buf.clone()
    gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws, k)
    first = [[g.t.clone() for g in gl] for gl in grads]
    assert _finite(gx, *[g for gl in first for g in gl])
    _record("cine_mwcnn_backward gx", gx, ref.gx, ref.e32.gx, rid)
    for s, (gl, wl, el) in enumerate(zip(first, ref.grads, ref.e32.grads)):
        for i, (g, want, e32) in enumerate(zip(gl, wl, el)):
            _record("cine_mwcnn_backward bias" if want.dim() == 1 else "cine_mwcnn_backward weights", g, want, e32, f"{rid} set {s} slot {i}")
    assert same_bits(x, x0) and same_bits(gy, gy0) and torch.equal(fwd_ws.buf, kept), "cine_mwcnn_backward changed an input or the forward workspace"
    # gx = NULL: the same gradients
    _, nogx = _backward(dev, ref, x, gy, nets, fwd_ws, k, want_gx=False)
    assert all(same_bits(a.t, b) for al, bl in zip(nogx, first) for a, b in zip(al, bl)), "cine_mwcnn_backward: gx = NULL changes a gradient"
    # grads are accumulated into: a second identical call leaves twice the gradient
    gx2, grads = _backward(dev, ref, x, gy, nets, fwd_ws, k, grads=grads)
    assert same_bits(gx2, gx)
    for s, (gl, wl, el) in enumerate(zip(grads, ref.grads, ref.e32.grads)):
        for i, (g, want, e32) in enumerate(zip(gl, wl, el)):
            _record("cine_mwcnn_backward accumulated", g.t, 2 * want, e32, f"{rid} set {s} slot {i}")


def test_tied_slots_of_set_one_do_not_leak_into_set_two(dev):
    """Set one holds one packed tensor in slots (0, 1) and (0, 2) of deep-convs, set two holds two tensors there: set two's slot (0, 2) is its own
    (a lookup of the second set's pointer by the first set's pointer VALUE ran it with set two's slot (0, 1))."""
    ref = R.reference(*R.TIED_RUN)
    nets = _nets(ref, dev)
    i, j = R.TIED[1]
    assert nets[0].weights[1 + i] == nets[0].weights[1 + j] and nets[1].weights[1 + i] != nets[1].weights[1 + j]
    x = ref.x.to(dev)
    y, _ = _forward(dev, ref, x, "2", nets, ref.split)
    _record("cine_mwcnn_forward2", y, ref.y, ref.e32.y, "deep-convs tied")
    yt, _ = _forward(dev, ref, x, "t", nets, ref.split)
    assert same_bits(yt, y)


# ================================================================== workspaces
WS_CASES = [(k, R.SLOPE, None) for k in R.CASES] + [("default", R.SLOPE, 1)]


@pytest.mark.parametrize("run", WS_CASES, ids=[R.run_id(r) for r in WS_CASES])
def test_results_do_not_depend_on_what_the_workspaces_held(dev, run):
    """Exact-size workspaces filled with 0x00 and with 0xFF (NaN) bytes: the same bits, all finite -- a read of scratch the pass never wrote
    (a feature map, a statistics record, a partial sum) shows as a NaN or as other bits."""
    ref = R.reference(*run)
    nets, k = _nets(ref, dev), ref.split
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    res = []
    for fill in (0x00, 0xFF):
        y, _ = _forward(dev, ref, x, "f" if k is None else "2", nets, k, fill=fill)
        yt, fwd_ws = _forward(dev, ref, x, "t", nets, k, fill=fill)
        gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws, k, fill=fill)
        res.append([y, yt, gx] + [g.t for gl in grads for g in gl])
    assert _finite(*res[0]) and _finite(*res[1])
    for a, b in zip(*res):
        assert same_bits(a, b), "the result depends on what a workspace held"


def test_workspaces_at_64_bytes_past_a_256_byte_boundary(dev):
    ref = R.reference("small", R.SLOPE, 1)
    nets, k = _nets(ref, dev), ref.split
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    res = []
    for past in (None, 64):
        y1, _ = _forward(dev, ref, x, "f", nets[:1], past256=past)
        y2, _ = _forward(dev, ref, x, "2", nets, k, past256=past)
        yt, fwd_ws = _forward(dev, ref, x, "t", nets, k, past256=past)
        gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws, k, past256=past)
        res.append([y1, y2, yt, gx] + [g.t for gl in grads for g in gl])
    assert _finite(*res[1])
    for a, b in zip(*res):
        assert same_bits(a, b), "other bits with the workspace 64 bytes past a 256-byte boundary"


def _refusal_operands(dev, ref, nets, k):
    """A Call with guarded outputs (y, gx, every gradient of both sets: NaN / zero prefills) and the pointer table R.refusal_call takes."""
    c = Call(dev, 0)
    x, gy = c.inp(ref.x), c.inp(ref.gy)
    y, gx = c.out(ref.y.shape), c.out(ref.x.shape)
    grads = [[c.out(p.shape, fill=torch.zeros(p.shape)) for p in nt.params] for nt in nets]
    lib, a = L(), _dims(ref)
    inf, train, bwd = R.ws_sizes(lib, a)
    ws, fwd = c.ws(max(inf, bwd)), c.ws(train)
    p = dict(x=x.data_ptr(), y=y.ptr(), gy=gy.data_ptr(), gx=gx.ptr(), ws=ws.ptr(), ws_bytes=ws.nbytes, fwd_ws=fwd.ptr(), fwd_bytes=fwd.nbytes,
             stream=_stream(), weights=list(nets[0].weights), weights2=list(nets[1].weights), wdgrad=list(nets[0].wdgrad),
             wdgrad2=list(nets[1].wdgrad), grads=[g.ptr() for g in grads[0]], grads2=[g.ptr() for g in grads[1]])
    return c, p, (inf, train, bwd)


def test_refusals_leave_every_output_untouched(dev):
    """The rows of R.REFUSALS at every entry point they apply to, and workspaces 256 bytes short: the stated code, a message of the call's own,
    y / gx still NaN, the gradients still zero, guards and workspace tails intact."""
    assert R.REFUSAL_CASE == "small"
    ref = R.reference("small", R.SLOPE, 1)
    nets = _nets(ref, dev)
    c, p, (inf, train, bwd) = _refusal_operands(dev, ref, nets, 1)
    lib = L()
    for what, over, null, code, entries in R.REFUSALS:
        for e in entries:
            refused(lambda: R.refusal_call(lib, e, over, null, p), code, c, f"{R.ENTRY[e]} {what}", name="cine_mwcnn")
            msg = lib.cine_last_error().decode(errors="replace")
            assert R.refusal_message_ok(msg, e, what), (e, what, msg)
    short = [("f", dict(ws_bytes=inf - 256)), ("2", dict(ws_bytes=inf - 256)), ("t", dict(fwd_bytes=train - 256)),
             ("b", dict(fwd_bytes=train - 256, ws_bytes=bwd)), ("b", dict(fwd_bytes=train, ws_bytes=bwd - 256))]
    for e, sizes in short:
        refused(lambda: R.refusal_call(lib, e, {}, None, dict(p, **sizes)), R.EWORKSPACE, c, f"{R.ENTRY[e]} workspace 256 bytes short", name="cine_mwcnn")


# ================================================================== determinism, the side stream
def test_default_twice_gives_the_same_bits(dev):
    ref = R.reference("default", R.SLOPE, 1)
    nets = _nets(ref, dev)
    lib, a = L(), _dims(ref)
    inf, train, bwd = R.ws_sizes(lib, a)

    def body(c):
        x, gy = c.inp(ref.x), c.inp(ref.gy)
        y, yt, gx = c.out(ref.y.shape), c.out(ref.y.shape), c.out(ref.x.shape)
        grads = [[c.out(q.shape, fill=torch.zeros(q.shape)) for q in nt.params] for nt in nets]
        ws, fwd, wsb = c.ws(inf), c.ws(train), c.ws(bwd)
        assert R.call_forward2(lib, a, x.data_ptr(), y.ptr(), nets[0].weights, nets[1].weights, 1, ws.ptr(), ws.nbytes, _stream()) == 0
        assert R.call_forward_train(lib, a, x.data_ptr(), yt.ptr(), nets[0].weights, nets[1].weights, 1, fwd.ptr(), fwd.nbytes, _stream()) == 0
        torch.cuda.synchronize()
        c.ins.append((fwd.buf, fwd.buf.clone()))                            # the backward must not change the forward workspace
        garr = [R.ptr_array([g.ptr() for g in gl]) for gl in grads]
        assert R.call_backward(lib, a, x.data_ptr(), gy.data_ptr(), nets[0].wdgrad, nets[1].wdgrad, garr[0], garr[1], 1, fwd.ptr(), fwd.nbytes,
                               wsb.ptr(), wsb.nbytes, gx.ptr(), _stream()) == 0
        return [y.t, yt.t, gx.t] + [g.t for gl in grads for g in gl]
    outs = twice(dev, 0, body, "cine_mwcnn_forward2 / _forward_train / _backward at default")
    assert _finite(*outs)


def test_side_stream_changes_no_bit(dev):
    ref = R.reference("small", R.SLOPE, 1)
    nets, k = _nets(ref, dev), ref.split
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    _, fwd_ws = _forward(dev, ref, x, "t", nets, k)
    gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws, k)
    side = torch.cuda.Stream(dev)
    assert side.cuda_stream != _stream()
    try:
        assert L().cine_set_side_stream(side.cuda_stream) == 0
        gx_s, grads_s = _backward(dev, ref, x, gy, nets, fwd_ws, k)
    finally:
        assert L().cine_set_side_stream(None) == 0
    side.synchronize()
    assert same_bits(gx_s, gx) and all(same_bits(a.t, b.t) for al, bl in zip(grads_s, grads) for a, b in zip(al, bl))
    gx_n, grads_n = _backward(dev, ref, x, gy, nets, fwd_ws, k)              # and back on one stream
    assert same_bits(gx_n, gx) and all(same_bits(a.t, b.t) for al, bl in zip(grads_n, grads) for a, b in zip(al, bl))


def test_both_conv_kernels_run_over_the_table(dev):
    """Which forward conv kernel the levels of a case take, from the library's route counters (one count per launch): the plane kernel
    (conv_plane.hip) nearly every level of `default`, the general kernel (conv_kernels.hip) every level of `ragged` and all of `small` but its
    20-wide first conv (the wide-plane kernel), and scale 0's last conv of big-source runs on conv_coarse.hip -- as the case table says."""
    lib = L()

    def routes(case):
        ref = R.reference(case)
        before = [lib.cine_diag_counter(i, 0) for i in range(D_FIRST, D_LAST + 1)]
        _forward(dev, ref, ref.x.to(dev), "f", _nets(ref, dev))
        moved = [lib.cine_diag_counter(i, 0) - b for i, b in zip(range(D_FIRST, D_LAST + 1), before)]
        nconv = 2 + 2 * sum(R.CASES[case][5])
        print(f"{case}: {nconv} convs, routes {dict(zip(ROUTES, moved))}")
        assert sum(moved) == nconv
        return dict(zip(ROUTES, moved)), nconv
    r, nconv = routes("default")
    assert r["plane"] >= nconv - 2
    r, nconv = routes("small")
    assert r["plane"] == 0 and r["general-vec"] + r["general-elem"] == nconv - 1 and r["wide"] == 1
    r, nconv = routes("ragged")
    assert r["general-vec"] + r["general-elem"] == nconv
    r, nconv = routes("big-source")
    assert r["coarse"] == 1


# ================================================================== Python level, at `ragged`
def _module(ref, net, dev):
    from reconstruction.models.denoisers import MWCNN
    hip = MWCNN(**R.kwargs(ref.case))
    hip.load_state_dict(net.state_dict(), strict=True)
    return hip.to(dev)


def test_module_forward_and_backward_vs_float64(dev):
    ref = R.reference("ragged")
    hip = _module(ref, ref.nets[0], dev)
    with torch.no_grad():
        _record("MWCNN.forward (inference)", hip(ref.x.to(dev)), ref.y, ref.e32.y, "ragged")
    x = ref.x.to(dev).requires_grad_(True)
    with torch.enable_grad():
        y = hip(x)
        (y * ref.gy.to(dev)).sum().backward()
    _record("MWCNN.forward (training)", y, ref.y, ref.e32.y, "ragged")
    _record("MWCNN.backward gx", x.grad, ref.gx, ref.e32.gx, "ragged")
    for i, (p, want, e32) in enumerate(zip(R.slots(hip), ref.grads[0], ref.e32.grads[0])):
        _record("MWCNN.backward parameters", p.grad, want, e32, f"ragged slot {i}")


def test_autograd_mwcnn_two_networks_vs_float64(dev):
    from cine_hip import autograd as ag
    ref = R.reference("ragged", R.SLOPE, 1)
    mods = [_module(ref, nt, dev) for nt in ref.nets]
    x = ref.x.to(dev).requires_grad_(True)
    with torch.enable_grad():
        y = ag.mwcnn(x, mods[0].hip_weights(), mods[1].hip_weights(), ref.split)
        (y * ref.gy.to(dev)).sum().backward()
    _record("autograd.mwcnn y", y, ref.y, ref.e32.y, "ragged split 1")
    _record("autograd.mwcnn gx", x.grad, ref.gx, ref.e32.gx, "ragged split 1")
    for s, (m, wl, el) in enumerate(zip(mods, ref.grads, ref.e32.grads)):
        for i, (p, want, e32) in enumerate(zip(R.slots(m), wl, el)):
            _record("autograd.mwcnn parameters", p.grad, want, e32, f"ragged split 1 set {s} slot {i}")


def test_ops_forward_under_two_branches_has_the_one_stream_bits(dev):
    from cine_hip import ops
    ref = R.reference("ragged", R.SLOPE, 1)
    mods = [_module(ref, nt, dev) for nt in ref.nets]
    x = ref.x.to(dev)
    with torch.no_grad():
        for w2, split in ((None, 0), (mods[1].hip_weights(), ref.split)):
            one = ops.mwcnn_forward(x, mods[0].hip_weights(), w2, split)
            with ops.branches(2):
                two = ops.mwcnn_forward(x, mods[0].hip_weights(), w2, split)
            torch.cuda.synchronize()
            assert same_bits(one, two), "ops.mwcnn_forward under branches(2): other bits"
    _record("ops.mwcnn_forward (2 networks)", one, ref.y, ref.e32.y, "ragged split 1")
