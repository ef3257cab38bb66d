"""The whole-network launch sequences of csrc/unet.hip and csrc/unet3d.hip through the C ABI -- cine_unet2d_forward, _forward_train,
_forward_branches, _backward, _backward_drop, cine_unet3d_forward, _forward_train, _forward_train_drop, _backward, _backward_drop with their
size queries -- against oracle/regularisers.Unet in float64 under autograd (tests/unet_reference.py: the case table, the runs, the bar).

Every call writes guarded outputs pre-filled with NaN and takes a workspace of exactly the size the library reports, filled with 0xFF bytes
(NaN) unless stated, with a sentinel tail.  Per run: the forward and every gradient at the bar min(BAR_CAP, max(BAR, 2 e32)) on the relative L2
error (e32: the float32 oracle against the float64 one; the CPU file asserts the cap never decides); the identities the binding relies on --
bit identities where the code promises them: training forward == inference forward where no layer's records are merged (at the bar
where one is: cine_instnorm_merge sums the records in another order than the consumers' own merge); two sets == the two one-set passes
concatenated; the same network in both sets == one set; branches == one stream for every admissible count, inference and training, also
layer-interleaved; all-ones Dropout multipliers == none; gx = NULL changes no gradient; a side stream changes no bit; a second call gives the same
bits -- the accumulation contract of `grads`; inputs and the forward workspace unchanged; no dependence on what a workspace held (0x00 against 0xFF fill), also at a base
pointer 64 bytes past a 256-byte boundary; every refusal with its outputs untouched.  The module, autograd.unet2d and ops.unet2d_forward under
ops.branches(2) once each at odd-every-level."""
import pytest
import torch

import unet_reference as R
from kernel_sweep import NAN, Call, Guarded, Workspace, Worst, refused, same_bits

pytestmark = pytest.mark.gpu
WORST = Worst()
_NETS = {}
_SIDE = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    L().cine_set_side_stream(None)
    d = torch.device("cuda:0")
    _SIDE[:] = [torch.cuda.Stream(d) for _ in range(7)]
    yield d
    torch.cuda.synchronize()
    if WORST:
        WORST.report()


def L():
    from cine_hip._lib import lib
    return lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nets(ref, dev):
    """The packed pointer lists of a reference's networks, made once per run."""
    key = id(ref)
    if key not in _NETS:
        _NETS[key] = (ref, [R.DeviceNet(nt, dev) for nt in ref.nets])
    return _NETS[key][1]


def _dims(ref, nets, **over):
    return R.dims(ref.case, **{"n": ref.n, "slope": ref.slope, "nsets": len(nets), **over})


def _lists(nets, key):
    return R.ptr_array([v for nt in nets for v in getattr(nt, key)])


def _ok(code, what):
    assert code == 0, (what, code, L().cine_last_error())


def _forward(dev, ref, x, nets, train=False, drop=None, fill=0xFF, past256=None, drop_entry=False):
    """cine_unet2d_forward / _forward_train, cine_unet3d_forward / _forward_train / _forward_train_drop on x (device): (y, workspace) after the
    guard checks.  A 2-D training forward with multipliers goes through cine_unet2d_forward_branches with nside = 0 (the only 2-D entry that takes them)."""
    lib, a = L(), _dims(ref, nets, n=x.shape[0])
    inf, trn, _ = R.ws_sizes(lib, a)
    ws = Workspace(trn if train else inf, dev, past256)
    ws.buf[:ws.nbytes] = fill
    y = Guarded((a.n, a.cout) + tuple(x.shape[2:]), 0, dev)
    y.t.fill_(NAN)
    dp = None if drop is None else drop.data_ptr()
    if drop is not None and not a.three:
        code = R.call_branches(lib, a, x.data_ptr(), y.ptr(), _lists(nets, "weights"), ws.ptr(), ws.nbytes, _stream(), None, 0, 1, dp)
    else:
        code = R.call_forward(lib, a, x.data_ptr(), y.ptr(), _lists(nets, "weights"), ws.ptr(), ws.nbytes, _stream(), train, dp, drop_entry)
    _ok(code, "forward")
    torch.cuda.synchronize()
    assert y.intact() and ws.intact(), "forward: write outside the output or past the workspace"
    return y.t, ws


def _branches(dev, ref, x, nets, nside, train, drop=None, fill=0xFF, past256=None):
    """cine_unet2d_forward_branches with nside side streams: (y, workspace)."""
    lib, a = L(), _dims(ref, nets, n=x.shape[0])
    need = R.branch_ws(lib, a, nside + 1, train & 1)
    assert need > 0, (a, nside)
    ws = Workspace(need, dev, past256)
    ws.buf[:ws.nbytes] = fill
    y = Guarded((a.n, a.cout) + tuple(x.shape[2:]), 0, dev)
    y.t.fill_(NAN)
    side = R.ptr_array([s.cuda_stream for s in _SIDE[:nside]]) if nside else None
    code = R.call_branches(lib, a, x.data_ptr(), y.ptr(), _lists(nets, "weights"), ws.ptr(), ws.nbytes, _stream(), side, nside, train,
                           None if drop is None else drop.data_ptr())
    _ok(code, f"cine_unet2d_forward_branches nside {nside} train {train}")
    torch.cuda.synchronize()
    assert y.intact() and ws.intact(), "cine_unet2d_forward_branches: write outside the output or past the workspace"
    return y.t, ws


def _zero_grads(nets, dev, fill=0.0):
    return [[Guarded(tuple(p.shape), 0, dev, torch.full(tuple(p.shape), fill)) for p in nt.params] for nt in nets]


def _backward(dev, ref, x, gy, nets, fwd_ws, grads=None, want_gx=True, drop=None, fill=0xFF, past256=None, drop_entry=False):
    """One backward call: (gx | None, grads[net][slot] as Guarded) after the guard checks; `grads` given: accumulated into."""
    lib, a = L(), _dims(ref, nets, n=x.shape[0])
    need = R.ws_sizes(lib, a)[2]
    ws = Workspace(need, dev, past256)
    ws.buf[:ws.nbytes] = fill
    grads = grads or _zero_grads(nets, dev)
    gx = Guarded(tuple(x.shape), 0, dev) if want_gx else None
    if gx is not None:
        gx.t.fill_(NAN)
    garr = R.ptr_array([g.ptr() for gl in grads for g in gl])
    code = R.call_backward(lib, a, x.data_ptr(), gy.data_ptr(), _lists(nets, "wdgrad"), garr, fwd_ws.ptr(), fwd_ws.nbytes, ws.ptr(), ws.nbytes,
                           gx.ptr() if gx else None, _stream(), None if drop is None else drop.data_ptr(), drop_entry)
    _ok(code, "backward")
    torch.cuda.synchronize()
    assert ws.intact() and fwd_ws.intact() and (gx is None or gx.intact()) and all(g.intact() for gl in grads for g in gl), \
        "backward: write outside an output or past a workspace"
    return (gx.t if gx else None), grads


def _record(what, got, want, e32, case):
    err, b = R.rel_l2(got.detach().cpu(), want), R.bar(e32)
    print(f"  {what:34s} {case}: error {err:.2e}, float32 oracle {e32:.2e}, bar {b:.1e}")
    WORST.record(what, err, b, case)


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _flat(grads):
    return [g.t if isinstance(g, Guarded) else g for gl in grads for g in gl]


def _stem(ref):
    return "cine_unet3d" if R.is3d(ref.case) else "cine_unet2d"


# ================================================================== every run: forward, backward, identities, contracts
@pytest.mark.parametrize("run", R.RUNS, ids=[R.run_id(r) for r in R.RUNS])
def test_forward_and_backward_vs_float64(dev, run):
    ref = R.reference(*run)
    nets, rid, stem, three = _nets(ref, dev), R.run_id(run), _stem(ref), R.is3d(ref.case)
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    x0, gy0 = x.clone(), gy.clone()
    drop = None if ref.mult is None else ref.mult.to(dev)
    per = ref.n // ref.sets
    # ---- forward
    if drop is None:
        y, _ = _forward(dev, ref, x, nets)
        _record(f"{stem}_forward", y, ref.y, ref.e32.y, rid)
        if ref.sets == 2:
            parts = [_forward(dev, ref, x[k * per:(k + 1) * per].clone(), [nt])[0] for k, nt in enumerate(nets)]
            assert same_bits(y, torch.cat(parts)), "two sets: not the bits of the two one-set passes"
            same, _ = _forward(dev, ref, x, [nets[0], nets[0]])
            one, _ = _forward(dev, ref, x, nets[:1])
            assert same_bits(same, one), "one network in both sets: not the bits of one set"
    yt, fwd_ws = _forward(dev, ref, x, nets, train=True, drop=drop)
    _record(f"{stem}_forward_train" + ("" if drop is None else " (drop)"), yt, ref.y, ref.e32.y, rid)
    if drop is None:
        if R.merges(L(), ref.case):         # merged records are summed in another order: equal at the bar, not to the bit
            assert R.rel_l2(yt.cpu(), y.cpu()) <= R.BAR, "training forward differs from the inference forward by more than the bar"
        else:
            assert same_bits(yt, y), "training forward: y differs from the inference forward's"
    # ---- backward
    kept = fwd_ws.buf.clone()
    gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws, drop=drop)
    first = [[g.t.clone() for g in gl] for gl in grads]
    assert _finite(yt, gx, *_flat(first))
    tag = f"{stem}_backward" + ("" if drop is None else "_drop")
    _record(f"{tag} gx", gx, ref.gx, ref.e32.gx, rid)
    for s, (gl, wl, el) in enumerate(zip(first, ref.grads, ref.e32.grads)):
        for i, (g, want, e32) in enumerate(zip(gl, wl, el)):
            _record(f"{tag} bias" if want.dim() == 1 else f"{tag} weights", g, want, e32, f"{rid} set {s} slot {i}")
    assert same_bits(x, x0) and same_bits(gy, gy0) and torch.equal(fwd_ws.buf, kept), "the backward changed an input or the forward workspace"
    if drop is not None and ref.sets == 1 and ref.n == 1:        # a dropped output channel (record M2 = +inf) takes no gradient at all
        off = 0
        for j, ch in enumerate(R.conv_channels(ref.case)):
            dead = (ref.mult[off:off + ch] == 0).to(dev)
            off += ch
            g = first[0][R.conv_slot(ref.case, j)]
            assert not dead.any() or float(g[dead].abs().max()) == 0, f"conv {j}: a dropped channel has a gradient"
    # gx = NULL: the same gradients
    _, nogx = _backward(dev, ref, x, gy, nets, fwd_ws, want_gx=False, drop=drop)
    assert all(same_bits(a, b) for a, b in zip(_flat(nogx), _flat(first))), "gx = NULL changes a gradient"
    # grads are accumulated into: a second call on pre-filled gradients leaves first + pre-fill
    gx2, acc = _backward(dev, ref, x, gy, nets, fwd_ws, grads=_zero_grads(nets, dev, 0.5), drop=drop)
    assert same_bits(gx2, gx), "a second backward gives other bits"
    for s, (gl, wl, el) in enumerate(zip(acc, ref.grads, ref.e32.grads)):
        for i, (g, want, e32) in enumerate(zip(gl, wl, el)):
            _record(f"{tag} accumulated", g.t, want + 0.5, e32, f"{rid} set {s} slot {i}")


# ================================================================== Dropout: all-ones multipliers are no multipliers
@pytest.mark.parametrize("case,sets", [("odd-every-level", 1), ("merge-l0", 2), ("odd3d", 1)])
def test_all_ones_multipliers_are_no_multipliers(dev, case, sets):
    ref = R.reference(case, R.SLOPE, sets)
    nets = _nets(ref, dev)
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    ones = torch.ones(R.drop_floats(case, ref.n), device=dev)
    assert L().cine_unet2d_drop_floats(ref.n, R.ALL[case][3], R.ALL[case][4]) == ones.numel()
    y0, ws0 = _forward(dev, ref, x, nets, train=True)
    y1, ws1 = _forward(dev, ref, x, nets, train=True, drop=ones)
    assert same_bits(y0, y1) and torch.equal(ws0.buf, ws1.buf), "all-ones multipliers change the training forward"
    if R.is3d(case):
        y2, ws2 = _forward(dev, ref, x, nets, train=True, drop_entry=True)           # cine_unet3d_forward_train_drop(NULL)
        assert same_bits(y0, y2) and torch.equal(ws0.buf, ws2.buf)
    else:
        y2, ws2 = _branches(dev, ref, x, nets, 0, 1)                                # cine_unet2d_forward_branches(nside 0, train, drop NULL)
        assert same_bits(y0, y2) and torch.equal(ws0.buf, ws2.buf)
    res = [_backward(dev, ref, x, gy, nets, ws0, drop=d, drop_entry=e) for d, e in ((None, False), (ones, True), (None, True))]
    for gx, grads in res[1:]:
        assert same_bits(gx, res[0][0]) and all(same_bits(a, b) for a, b in zip(_flat(grads), _flat(res[0][1]))), "all-ones multipliers change a gradient"


# ================================================================== branches
BRANCH_RUNS = [("plane16", 1, None), ("plane16", 2, 6), ("merge-l0", 1, None), ("merge-l0", 2, None), ("odd-every-level", 2, 2)]


@pytest.mark.parametrize("case,sets,n", BRANCH_RUNS, ids=[f"{c}-{s}sets" for c, s, _ in BRANCH_RUNS])
def test_branches_have_the_one_stream_bits(dev, case, sets, n):
    """Every admissible number of side streams, inference and training, whole sequences per branch and layer-interleaved: y and -- in training
    mode -- the whole workspace equal the one-stream call's byte for byte, and the backward on it gives the same gradients."""
    ref = R.reference(case, R.SLOPE, sets, False, n)
    nets = _nets(ref, dev)
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    y, _ = _forward(dev, ref, x, nets)
    yt, fwd_ws = _forward(dev, ref, x, nets, train=True)
    y0, _ = _branches(dev, ref, x, nets, 0, 0)
    assert same_bits(y0, y), "cine_unet2d_forward_branches with nside = 0: not cine_unet2d_forward's bits"
    gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws)
    ran = []
    for nside in range(1, 8):
        nb = nside + 1
        if nb % sets or ref.n // nb < 1:
            assert R.branch_ws(L(), _dims(ref, nets), nb, 0) == 0
            continue
        ran.append(nb)
        yb, _ = _branches(dev, ref, x, nets, nside, 0)
        assert same_bits(yb, y), f"{nb} branches (inference): other bits"
        yi, _ = _branches(dev, ref, x, nets, nside, 2)
        assert same_bits(yi, y), f"{nb} branches (inference, interleaved): other bits"
        for train in (1, 3):
            ytb, wsb = _branches(dev, ref, x, nets, nside, train)
            assert same_bits(ytb, yt), f"{nb} branches (train {train}): other bits"
            assert torch.equal(wsb.buf, fwd_ws.buf), f"{nb} branches (train {train}): the training workspace differs from the one-stream call's"
        gxb, gradsb = _backward(dev, ref, x, gy, nets, wsb)
        assert same_bits(gxb, gx) and all(same_bits(a, b) for a, b in zip(_flat(gradsb), _flat(grads))), f"{nb} branches: the backward differs"
    print(f"{case} n {ref.n} sets {sets}: branch counts run {ran}")
    want = {("plane16", 1): [2, 3], ("plane16", 2): [2, 4, 6], ("merge-l0", 1): [2], ("merge-l0", 2): [2], ("odd-every-level", 2): [2]}[(case, sets)]
    assert ran == want


def test_branches_with_multipliers_have_the_one_stream_bits(dev):
    ref = R.reference("merge-l0", R.SLOPE, 2, True)
    nets = _nets(ref, dev)
    x = ref.x.to(dev)
    drop = ref.mult.to(dev)
    yt, ws = _forward(dev, ref, x, nets, train=True, drop=drop)
    yb, wsb = _branches(dev, ref, x, nets, 1, 1, drop=drop)
    assert same_bits(yb, yt) and torch.equal(wsb.buf, ws.buf)


# ================================================================== workspaces
WS_RUNS = [(k, R.SLOPE, 1, False, None) for k in R.ALL] + [("plane16", R.SLOPE, 2, False, 6)]


@pytest.mark.parametrize("run", WS_RUNS, ids=[R.run_id(r) for r in WS_RUNS])
def test_results_do_not_depend_on_what_the_workspaces_held(dev, run):
    """Exact-size workspaces filled with 0x00 and with 0xFF (NaN) bytes: the same bits, all finite -- a read of scratch the pass never wrote
    (a layer output, a statistics record, a merged record, a partial sum) shows as a NaN or as other bits."""
    ref = R.reference(*run)
    nets = _nets(ref, dev)
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    res = []
    for fill in (0x00, 0xFF):
        y, _ = _forward(dev, ref, x, nets, fill=fill)
        yt, fwd_ws = _forward(dev, ref, x, nets, train=True, fill=fill)
        gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws, fill=fill)
        out = [y, yt, gx] + _flat(grads)
        if not R.is3d(ref.case) and ref.n >= 2:
            out += [_branches(dev, ref, x, nets, 1, 0, fill=fill)[0], _branches(dev, ref, x, nets, 1, 1, fill=fill)[0]]
        res.append(out)
    assert _finite(*res[0]) and _finite(*res[1])
    for a, b in zip(*res):
        assert same_bits(a, b), "the result depends on what a workspace held"


@pytest.mark.parametrize("case,sets", [("merge-l0", 2), ("odd3d", 1)])
def test_workspaces_at_64_bytes_past_a_256_byte_boundary(dev, case, sets):
    ref = R.reference(case, R.SLOPE, sets)
    nets = _nets(ref, dev)
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    res = []
    for past in (None, 64):
        y, _ = _forward(dev, ref, x, nets, past256=past)
        yt, fwd_ws = _forward(dev, ref, x, nets, train=True, past256=past)
        gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws, past256=past)
        out = [y, yt, gx] + _flat(grads)
        if not R.is3d(case):
            out += [_branches(dev, ref, x, nets, 1, 0, past256=past)[0], _branches(dev, ref, x, nets, 1, 1, past256=past)[0]]
        res.append(out)
    assert _finite(*res[1])
    for a, b in zip(*res):
        assert same_bits(a, b), "other bits with the workspace 64 bytes past a 256-byte boundary"


@pytest.mark.parametrize("case,sets,n", [("plane16", 2, 6), ("coarse2d", 1, None), ("coarse3d", 1, None)])
def test_side_stream_changes_no_bit(dev, case, sets, n):
    """cine_set_side_stream: the weight gradients fork onto a second stream and join before the call returns -- same bits, and the same again
    back on one stream.  (The gradient chain goes on writing its scratch while they run: a scratch buffer too small for what the chain writes
    runs into the weight gradients' partial sums.)"""
    ref = R.reference(case, R.SLOPE, sets, False, n)
    nets = _nets(ref, dev)
    x, gy = ref.x.to(dev), ref.gy.to(dev)
    _, fwd_ws = _forward(dev, ref, x, nets, train=True)
    gx, grads = _backward(dev, ref, x, gy, nets, fwd_ws)
    side = _SIDE[0]
    assert side.cuda_stream != _stream()
    try:
        assert L().cine_set_side_stream(side.cuda_stream) == 0
        gx_s, grads_s = _backward(dev, ref, x, gy, nets, fwd_ws)
    finally:
        assert L().cine_set_side_stream(None) == 0
    side.synchronize()
    assert same_bits(gx_s, gx) and all(same_bits(a, b) for a, b in zip(_flat(grads_s), _flat(grads))), "a side stream changes a gradient"
    gx_n, grads_n = _backward(dev, ref, x, gy, nets, fwd_ws)
    assert same_bits(gx_n, gx) and all(same_bits(a, b) for a, b in zip(_flat(grads_n), _flat(grads)))


# ================================================================== refusals
def _refusal_operands(dev, three):
    """A Call with guarded outputs (y, gx, every gradient: NaN / zero prefills), exact workspaces and the operand table R.entry_call takes."""
    case = R.REFUSAL_CASE3 if three else R.REFUSAL_CASE
    ref = R.reference(case, 0.0, 1) if not three else R.reference(case)
    nets = _nets(ref, dev) * (1 if three else 2)
    a = R.refusal_dims(three)
    c = Call(dev, 0)
    x, gy = c.inp(ref.x), c.inp(ref.gy)
    y, gx = c.out(ref.y.shape), c.out(ref.x.shape)
    grads = [[c.out(p.shape, fill=torch.zeros(p.shape)) for p in nt.params] for nt in nets]
    inf, trn, bwd = R.ws_sizes(L(), a)
    bneed = 0 if three else max(R.branch_ws(L(), a, 2, 0), R.branch_ws(L(), a, 2, 1))
    ws, fwd = c.ws(max(inf, bwd)), c.ws(trn)
    bws = c.ws(bneed)
    p = dict(x=x.data_ptr(), y=y.ptr(), gy=gy.data_ptr(), gx=gx.ptr(), ws=ws.ptr(), ws_bytes=ws.nbytes, fwd_ws=fwd.ptr(), fwd_bytes=fwd.nbytes,
             bws=bws.ptr() if bws else None, bws_bytes=bneed, stream=_stream(), weights=[v for nt in nets for v in nt.weights],
             wdgrad=[v for nt in nets for v in nt.wdgrad], grads=[g.ptr() for gl in grads for g in gl],
             side=[s.cuda_stream for s in _SIDE], nside=1, train=0, drop=None)
    return c, a, p, (inf, trn, bwd)


@pytest.mark.parametrize("three", [False, True], ids=["2d", "3d"])
def test_refusals_leave_every_output_untouched(dev, three):
    """The rows of R.REFUSALS at every entry point they apply to, every NULL pointer and slot, the branch checks and workspaces one byte short:
    the stated code, a message of the call's own, y / gx still NaN, the gradients still zero, guards and workspace tails intact."""
    c, a0, p, (inf, trn, bwd) = _refusal_operands(dev, three)
    lib = L()
    entries = R.ENTRIES3 if three else R.ENTRIES2
    nptr = 5 * a0.pools + 4

    def go(e, a, q, code, what):
        name = R.ENTRY[(three, e)]
        refused(lambda: R.entry_call(lib, e, a, q), code, c, f"{name} {what}", name=name[:11] + R.MESSAGE[e])
    for what, over, code, ents in R.REFUSALS:
        over = {k: v for k, v in over.items() if three or k != "d"}
        for e in entries:
            if not R.applies(ents, e, three):
                continue
            q = p
            if over.get("nsets") == 3:
                q = dict(p, weights=p["weights"] + p["weights"][:nptr], wdgrad=p["wdgrad"] + p["wdgrad"][:nptr], grads=p["grads"] + p["grads"][:nptr])
            for train in ((0, 1) if e == "r" else (0,)):
                go(e, R.refusal_dims(three, **over), dict(q, train=train), code, what)
    for e in entries:
        for what, q in R.pointer_refusals(e, p, three, nptr):
            go(e, a0, q, R.EINVAL, what)
    short = [("f", dict(ws_bytes=inf - 1)), ("t", dict(fwd_bytes=trn - 1)), ("b", dict(fwd_bytes=trn - 1, ws_bytes=bwd)),
             ("b", dict(fwd_bytes=trn, ws_bytes=bwd - 1)), ("B", dict(fwd_bytes=trn - 1, ws_bytes=bwd)), ("B", dict(fwd_bytes=trn, ws_bytes=bwd - 1))]
    if three:
        short.append(("T", dict(fwd_bytes=trn - 1)))
    else:
        short += [("r", dict(bws_bytes=R.branch_ws(lib, a0, nb, tr & 1) - 1, nside=nb - 1, train=tr)) for nb in (1, 2) for tr in (0, 1, 3)]
        for train in (0, 1):
            for what, over, ops_over, code in R.branch_refusals(p):
                if over.get("n", 2) > 2:
                    continue                    # (more samples than the operands hold: the CPU file runs these rows)
                go("r", R.refusal_dims(False, **over), {**p, "train": train, **ops_over}, code, what)
    for e, sizes in short:
        go(e, a0, dict(p, **sizes), R.EWORKSPACE, f"one byte short {sizes}")


# ================================================================== Python level, at odd-every-level
def _module(ref, net, dev):
    from reconstruction.models.denoisers.unet import Unet
    t = R.ALL[ref.case]
    hip = Unet(in_chans=t[1], out_chans=t[2], chans=t[3], num_pool_layers=t[4], drop_prob=0.0, dims=3 if R.is3d(ref.case) else 2)
    hip.load_state_dict(net.state_dict(), strict=True)
    return hip.to(dev).eval()


def _hip_slots(m):
    from cine_hip import ops
    (seq,) = ops.UnetWeights([m])._params()
    return [p for _, p in seq]


@pytest.mark.parametrize("case", ["odd-every-level", "odd3d"])
def test_module_forward_and_backward_vs_float64(dev, case):
    ref = R.reference(case)
    hip = _module(ref, ref.nets[0], dev)
    with torch.no_grad():
        _record("Unet.forward (inference)", hip(ref.x.to(dev)), ref.y, ref.e32.y, case)
    x = ref.x.to(dev).requires_grad_(True)
    with torch.enable_grad():
        y = hip(x)
        (y * ref.gy.to(dev)).sum().backward()
    _record("Unet.forward (training)", y, ref.y, ref.e32.y, case)
    _record("Unet.backward gx", x.grad, ref.gx, ref.e32.gx, case)
    for i, (p, want, e32) in enumerate(zip(_hip_slots(hip), ref.grads[0], ref.e32.grads[0])):
        _record("Unet.backward parameters", p.grad, want, e32, f"{case} slot {i}")


def test_autograd_unet2d_two_networks_vs_float64(dev):
    from cine_hip import autograd as ag, ops
    ref = R.reference("odd-every-level", R.SLOPE, 2, False, 2)
    mods = [_module(ref, nt, dev) for nt in ref.nets]
    x = ref.x.to(dev).requires_grad_(True)
    with torch.enable_grad():
        y = ag.unet2d(x, ops.UnetWeights(mods))
        (y * ref.gy.to(dev)).sum().backward()
    _record("autograd.unet2d y", y, ref.y, ref.e32.y, "odd-every-level 2 sets")
    _record("autograd.unet2d gx", x.grad, ref.gx, ref.e32.gx, "odd-every-level 2 sets")
    for s, (m, wl, el) in enumerate(zip(mods, ref.grads, ref.e32.grads)):
        for i, (p, want, e32) in enumerate(zip(_hip_slots(m), wl, el)):
            _record("autograd.unet2d parameters", p.grad, want, e32, f"odd-every-level 2 sets set {s} slot {i}")


def test_ops_forward_under_two_branches_has_the_one_stream_bits(dev):
    from cine_hip import ops
    ref = R.reference("odd-every-level", R.SLOPE, 2, False, 2)
    wts = ops.UnetWeights([_module(ref, nt, dev) for nt in ref.nets])
    x = ref.x.to(dev)
    with torch.no_grad():
        one = ops.unet2d_forward(x, wts)
        with ops.branches(2):
            two = ops.unet2d_forward(x, wts)
        torch.cuda.synchronize()
    assert same_bits(one, two), "ops.unet2d_forward under branches(2): other bits"
    _record("ops.unet2d_forward (2 networks)", one, ref.y, ref.e32.y, "odd-every-level 2 sets")
