"""The parts of the MWCNN launch-sequence sweep that need no GPU: the yardstick of tests/mwcnn_reference.py itself, the three workspace-size
queries of csrc/mwcnn.hip, the order of the pointer arrays, and every refusal -- all of them return before the first launch, so they run here
with made-up device addresses (test_mwcnn_sequences.py repeats them with guarded outputs).

The bar of a compared tensor is min(BAR_CAP, max(BAR, 2 e32)), e32 the float32 oracle's relative L2 error against the float64 one.  The cap is
a condition on the case table, asserted here: 2 e32 <= BAR_CAP for every run and tensor, so the cap never passes anything."""
import pytest
import torch

import mwcnn_reference as R
from kernel_sweep import BAR_CAP


def L():
    from cine_hip._lib import lib
    return lib()


ALL_RUNS = [(k, s, sp, None, None) for k, s, sp in R.RUNS] + [R.TIED_RUN]


@pytest.mark.parametrize("run", ALL_RUNS, ids=[R.run_id(r[:3]) + ("-tied" if r[3] else "") for r in ALL_RUNS])
def test_the_cap_never_decides_a_bar(run):
    ref = R.reference(*run)
    errs = {"y": ref.e32.y, "gx": ref.e32.gx}
    for k, g in enumerate(ref.e32.grads):
        errs.update({f"grads{k}[{i}]": e for i, e in enumerate(g)})
    worst = max(errs, key=errs.get)
    print(f"{R.run_id(run[:3])}: float32 oracle vs float64, worst {worst} {errs[worst]:.2e}; y {ref.e32.y:.2e}, gx {ref.e32.gx:.2e}")
    for name, e in errs.items():
        assert 2 * e <= BAR_CAP, (name, e)
    for t in [ref.y, ref.gx] + [g for gl in ref.grads for g in gl]:
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0


def test_tied_modules_equal_copied_weights():
    """The oracle with conv_blocks_per_scale[0][2] IS [0][1] computes what an oracle with the weight copied into that slot computes, and the
    tied parameter's gradient is the sum of the two slots'."""
    case, (i, j) = R.TIED
    ref = R.reference(case, R.SLOPE, None, (i, j))
    tied = ref.nets[0]
    assert tied.conv_blocks_per_scale[0][j] is tied.conv_blocks_per_scale[0][i]
    plain = R.make_net(case, R.SEEDS[case] + 1)
    with torch.no_grad():
        plain.conv_blocks_per_scale[0][j].layers[0].weight.copy_(plain.conv_blocks_per_scale[0][i].layers[0].weight)
    assert all(torch.equal(a, b) for a, b in zip(R.slots(plain), R.slots(tied)))
    y, gx, grads = R._run([plain], ref.x, ref.gy, None, torch.float64)
    assert R.rel_l2(y, ref.y) < 1e-13 and R.rel_l2(gx, ref.gx) < 1e-13
    assert R.rel_l2(grads[0][1 + i] + grads[0][1 + j], ref.grads[0][1 + i]) < 1e-13
    untied = R.reference(case)                      # and the tying matters: the untied network of the same seed gives another result
    assert R.rel_l2(untied.y, ref.y) > 1e-3


def test_slopes_reach_the_oracle():
    a, b, c = (R.reference("small", s) for s in (0.0, R.SLOPE, 1.0))
    assert R.rel_l2(a.y, b.y) > 1e-3 and R.rel_l2(c.y, b.y) > 1e-3
    assert all(m.negative_slope == 0.0 for m in a.nets[0].modules() if isinstance(m, torch.nn.LeakyReLU))


def test_pointer_array_order_matches_the_binding():
    from cine_hip import ops
    from reconstruction.models.denoisers import MWCNN
    for case in R.CASES:
        net = MWCNN(**R.kwargs(case))
        (seq,) = ops.MwcnnWeights(net)._params()
        want = R.slots(net)
        n, cin, cout, first, nf, nc, h, w = R.CASES[case]
        assert len(seq) == len(want) == 1 + 2 * sum(nc) + 2
        assert all(p is q for (_, p), q in zip(seq, want))
        assert [k for k, _ in seq] == ["c3"] * (len(want) - 1) + ["raw"]
        ref = R.make_net(case, 1)                    # the oracle's slots have the shapes of the module's
        assert [tuple(p.shape) for p in R.slots(ref)] == [tuple(p.shape) for p in want]
        plan = R.conv_plan(case)
        assert [tuple(p.shape[:2]) for p in want[1:-1]] == [(co, ci) for ci, co, _, _, _ in plan]


def test_materialise_threshold_has_a_case_on_each_side():
    """grad_kernels.hip: launch_wgrad materialises a transformed (DWT / IWT / summed) source of n ci hs ws >= 65 536 floats whose width is a
    multiple of 4: big-source has such sources, every other case only smaller ones."""
    big = {}
    for case, (n, *_rest) in R.CASES.items():
        big[case] = max(n * ci * hs * ws for ci, co, hs, ws, tr in R.conv_plan(case) if tr)
    print(big)
    assert big["big-source"] >= R.MATERIALISE_FLOATS and R.CASES["big-source"][7] // 2 % 4 == 0
    assert all(v < R.MATERIALISE_FLOATS for k, v in big.items() if k != "big-source")


# ================================================================== workspace sizes
EXTRA_WS_SHAPES = [            # (n, in, out, first, nf, nc, h, w): XPDNet's topology on planes whose scale 0 is wider than 16
    (1, 12, 10, 16, [16, 32, 64], [2, 2, 2], 48, 48), (3, 12, 10, 16, [16, 32, 64], [2, 2, 2], 200, 16),
    (2, 12, 10, 16, [16, 32, 64], [2, 2, 2], 104, 56), (1, 4, 4, 32, [32, 16], [1, 2], 64, 64)]


def _inference_floor(lib, n, cin, cout, first, nf, nc, h, w):
    """What one inference pass must hold at least, in bytes: the first block's feature and records, every scale's skip feature and records, and
    three scratch buffers each large enough for ANY conv output of the plan with its statistics records (cine_conv_stat_partials per conv)."""
    rec = lambda c, hs, ws: n * c * lib.cine_conv_stat_partials(c, hs, ws, 0) * 3          # noqa: E731
    total = n * first * h * w + rec(first, h, w)
    feat = part = 0
    for s in range(len(nf)):
        hs, ws = h >> (s + 1), w >> (s + 1)
        total += n * nf[s] * hs * ws + rec(nf[s], hs, ws)
        for i in range(2 * nc[s]):
            co = nf[s]
            if i == 2 * nc[s] - 1:
                co = max(4 * first, 4 * cout) if s == 0 else 4 * nf[s - 1]
            feat, part = max(feat, n * co * hs * ws), max(part, rec(co, hs, ws))
    return 4 * (total + 3 * (feat + part))


@pytest.mark.parametrize("shape", [R.CASES[k] for k in R.CASES] + EXTRA_WS_SHAPES, ids=list(R.CASES) + [f"extra{i}" for i in range(len(EXTRA_WS_SHAPES))])
def test_inference_workspace_holds_every_conv_output_and_its_records(shape):
    """Before this sweep build() sized the scratch statistics from the 16-row tiling of the finest scale times 4; a 64-row conv on a 24 x 24
    plane (conv_coarse.hip: 19 records per plane against 2) wrote past them -- inside the workspace at big-source, past its end at extra0."""
    lib = L()
    n, cin, cout, first, nf, nc, h, w = shape
    got = lib.cine_mwcnn_ws_bytes(n, h, w, cin, cout, len(nf), R.int_array(nf), R.int_array(nc), first)
    assert got >= _inference_floor(lib, *shape), (got, _inference_floor(lib, *shape))


@pytest.mark.parametrize("case", list(R.CASES))
def test_workspace_sizes(case):
    lib = L()
    a = R.dims(case)
    sizes = R.ws_sizes(lib, a)
    assert all(s > 0 and s % 256 == 0 for s in sizes), sizes
    assert sizes[1] >= 4 * R.feature_floats(case)
    prev = (0, 0, 0)
    for n in (1, 2, 3, 5, 8, 64):
        cur = R.ws_sizes(lib, R.dims(case, n=n))
        assert all(c >= p and c % 256 == 0 for c, p in zip(cur, prev)), (n, cur, prev)
        assert cur[1] >= 4 * R.feature_floats(case, n)
        prev = cur
    bad = [dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(S=0), dict(S=7, nf=[8] * 7, nc=[1] * 7), dict(cin=0), dict(cout=0), dict(first=0),
           dict(cout=a.first + 1), dict(nf=[0] * a.S), dict(nc=[0] * a.S), dict(nc=[5] * a.S)]
    for over in bad:
        assert R.ws_sizes(lib, R.dims(case, **over)) == (0, 0, 0), over
    t = (a.n, a.h, a.w, a.cin, a.cout, a.S)
    for fn in (lib.cine_mwcnn_ws_bytes, lib.cine_mwcnn_train_ws_bytes, lib.cine_mwcnn_backward_ws_bytes):
        assert fn(*t, None, R.int_array(a.nc), a.first) == 0 and fn(*t, R.int_array(a.nf), None, a.first) == 0


# ================================================================== out_ch > first_filters
def test_out_wider_than_first_has_no_reference_and_is_refused():
    from oracle import xpdnet_ref as X
    from reconstruction.models.denoisers import MWCNN
    kw = dict(R.kwargs("small"), in_chans=2, out_chans=12, first_conv_n_filters=8)
    ref = X.MWCNN(**kw)                                       # the reference constructs it ...
    assert ref.conv_blocks_per_scale[0][-1].layers[0].out_channels == 48
    with pytest.raises(RuntimeError):                         # ... and its forward adds 12 channels to 8 (mwcnn.py:172)
        ref(torch.zeros(1, 2, 12, 20))
    with pytest.raises(RuntimeError):                         # (first = 1 broadcasts in the sum and fails in the final conv instead)
        X.MWCNN(**dict(kw, first_conv_n_filters=1))(torch.zeros(1, 2, 12, 20))
    hip = MWCNN(**kw)
    for grad in (False, True):
        with torch.set_grad_enabled(grad), pytest.raises(ValueError, match="out_chans 12 > first_conv_n_filters 8"):
            hip(torch.zeros(1, 2, 12, 20))
    from cine_hip._lib import CineHipError
    eq = MWCNN(**dict(kw, out_chans=8))                       # the boundary is accepted: it gets as far as asking for a device tensor
    with pytest.raises(CineHipError, match="needs a GPU tensor"):
        eq(torch.zeros(1, 2, 12, 20))
    assert R.ws_sizes(L(), R.dims("small", cin=2, cout=12, first=8)) == (0, 0, 0)


# ================================================================== refusals (all before the first launch)
def _fake_pointers():
    nslots = 1 + 2 * sum(R.CASES[R.REFUSAL_CASE][5]) + 2
    fake = lambda k: [0x10000 * (k + 1) + 256 * i for i in range(nslots)]          # noqa: E731  never dereferenced: every call is refused first
    return dict(x=0x1000, y=0x2000, gy=0x3000, gx=0x4000, ws=0x5000, ws_bytes=1 << 40, fwd_ws=0x6000, fwd_bytes=1 << 40, stream=None,
                weights=fake(0), weights2=fake(1), wdgrad=fake(2), wdgrad2=fake(3), grads=fake(4), grads2=fake(5))


REFUSAL_ROWS = [(what, over, null, code, e) for what, over, null, code, entries in R.REFUSALS for e in entries]


@pytest.mark.parametrize("what,over,null,code,entry", REFUSAL_ROWS, ids=[f"{R.ENTRY[r[4]][11:]}-{r[0].replace(' ', '_')}" for r in REFUSAL_ROWS])
def test_refusals_before_any_launch(what, over, null, code, entry):
    lib = L()
    assert lib.cine_scale(None, 1, 1.0, None) == R.EINVAL and lib.cine_last_error().startswith(b"cine_scale")
    got = R.refusal_call(lib, entry, over, null, _fake_pointers())
    msg = lib.cine_last_error().decode(errors="replace")
    assert got == code, (got, msg)
    assert R.refusal_message_ok(msg, entry, what), msg


def test_short_workspace_is_refused_before_any_launch():
    lib = L()
    p = _fake_pointers()
    a = R.dims(R.REFUSAL_CASE)
    inf, train, bwd = R.ws_sizes(lib, a)
    arr = {k: R.ptr_array(p[k]) for k in ("weights", "weights2", "wdgrad", "wdgrad2", "grads", "grads2")}
    assert R.call_forward(lib, a, p["x"], p["y"], arr["weights"], p["ws"], inf - 256, None) == R.EWORKSPACE
    assert R.call_forward2(lib, a, p["x"], p["y"], arr["weights"], arr["weights2"], 1, p["ws"], inf - 256, None) == R.EWORKSPACE
    assert R.call_forward_train(lib, a, p["x"], p["y"], arr["weights"], None, a.n, p["fwd_ws"], train - 256, None) == R.EWORKSPACE
    for fb, bb in ((train - 256, bwd), (train, bwd - 256)):
        assert R.call_backward(lib, a, p["x"], p["gy"], arr["wdgrad"], None, arr["grads"], None, a.n, p["fwd_ws"], fb, p["ws"], bb, p["gx"],
                               None) == R.EWORKSPACE
        assert lib.cine_last_error().startswith(b"cine_mwcnn_backward")
