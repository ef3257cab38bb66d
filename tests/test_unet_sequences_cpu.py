"""The parts of the U-Net launch-sequence sweep that need no GPU: the yardstick of tests/unet_reference.py itself, what each case of the table
is there for (record counts on both sides of kMergeMin, levels on both sides of cine_conv3d_pools_on_load), the order and packing of the pointer
arrays against the binding's, the size queries of csrc/unet.hip and csrc/unet3d.hip restated from the layer plan, and every refusal -- all of
them return before the first launch, so they run here with made-up device addresses (test_unet_sequences.py repeats them with guarded outputs).

The bar of a compared tensor is min(BAR_CAP, max(BAR, 2 e32)), e32 the float32 oracle's relative L2 error against the float64 one.  The cap is
a condition on the case table, asserted here: 2 e32 <= BAR_CAP for every run and tensor, so the cap never passes anything."""
import os
import re

import numpy as np
import pytest
import torch

import unet_reference as R
from kernel_sweep import BAR_CAP


def L():
    from cine_hip._lib import lib
    return lib()


# ================================================================== the yardstick
@pytest.mark.parametrize("run", R.RUNS, ids=[R.run_id(r) for r in R.RUNS])
def test_the_cap_never_decides_a_bar(run):
    ref = R.reference(*run)
    errs = {"y": ref.e32.y, "gx": ref.e32.gx}
    for k, g in enumerate(ref.e32.grads):
        errs.update({f"grads{k}[{i}]": e for i, e in enumerate(g)})
    worst = max(errs, key=errs.get)
    print(f"{R.run_id(run)}: float32 oracle vs float64, worst {worst} {errs[worst]:.2e}; y {ref.e32.y:.2e}, gx {ref.e32.gx:.2e}")
    for name, e in errs.items():
        assert 2 * e <= BAR_CAP, (name, e)
    for t in [ref.y, ref.gx] + [g for gl in ref.grads for g in gl]:
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0


def test_slopes_and_multipliers_reach_the_oracle():
    a, b, c = (R.reference("slope", s) for s in (0.0, R.SLOPE, 1.0))
    assert R.rel_l2(a.y, b.y) > 1e-3 and R.rel_l2(c.y, b.y) > 1e-3
    assert all(m.negative_slope == 0.0 for m in a.nets[0].modules() if isinstance(m, torch.nn.LeakyReLU))
    for case in ("odd-every-level", "odd3d"):
        plain, drop = R.reference(case), R.reference(case, R.SLOPE, 1, True)
        assert R.rel_l2(drop.y, plain.y) > 1e-3
        m = drop.mult
        assert m.numel() == R.drop_floats(case, drop.n) and set(m.tolist()) == {0.0, 1.0, float(np.float32(1 / (1 - R.DROP_P)))}
        # n = 1: a dropped output channel of a conv takes no gradient at all
        off = 0
        for j, ch in enumerate(R.conv_channels(case)):
            dead = m[off:off + ch] == 0
            off += ch
            g = drop.grads[0][R.conv_slot(case, j)]
            assert g.shape[0] == ch and float(g[dead].abs().max() if dead.any() else 0) == 0 and float(g[~dead].abs().max()) > 0


def test_two_sets_are_the_two_one_set_passes():
    two = R.reference("odd-every-level", R.SLOPE, 2, False, 2)
    for k, net in enumerate(two.nets):
        y, gx, grads = R._run([net], two.x[k:k + 1], two.gy[k:k + 1], torch.float64)
        assert torch.equal(y, two.y[k:k + 1]) and torch.equal(gx, two.gx[k:k + 1])
        assert all(torch.equal(a, b) for a, b in zip(grads[0], two.grads[k]))


# ================================================================== what the cases are there for
# (case, level, is_tconv) -> records per (sample, channel), derived by hand from tiles_for in csrc/conv_kernels.hip
RECORDS = {("merge-l0", 0, False): 12, ("merge-l0", 0, True): 12, ("merge-l0", 1, False): 3, ("six-pools", 0, False): 84}


def test_record_counts_of_the_table():
    lib = L()
    table = {}
    for case in R.ALL:
        P = R.ALL[case][4]
        table[case] = ([R.records(lib, case, l, False) for l in range(P + 1)], [R.records(lib, case, l, True) for l in range(P)])
        print(f"{case:16s} conv records per level {table[case][0]}, transpose-conv records per level {table[case][1]}")
        assert all(v >= 1 for v in table[case][0] + table[case][1])
    for (case, l, tc), want in RECORDS.items():
        assert table[case][int(tc)][l] == want, (case, l, tc, table[case])
    # a merged and an unmerged layer inside one network, for both kinds of producer
    for case in ("merge-l0", "merge-odd"):
        conv, tconv = table[case]
        assert max(conv) >= R.KMERGE > min(conv) and max(tconv) >= R.KMERGE > min(tconv), (case, table[case])
    assert max(table["coarse2d"][0]) >= R.KMERGE > min(table["coarse2d"][0])
    assert max(table["merge-32rows"][0]) >= R.KMERGE and R.merges(lib, "merge-32rows")
    # exactly at the threshold, and one below it somewhere in the table: kMergeMin itself is pinned
    assert any(v == R.KMERGE for case in R.CASES for v in table[case][0])
    # conv_coarse.hip's level (64 rows on 26 x 26) emits more records than the 16-row tiling of that plane would
    assert table["coarse2d"][0][2] > 4
    # cases the identities treat as unmerged really are
    for case in ("odd-every-level", "one-channel", "ragged-18", "wide-in", "plane16", "slope"):
        assert not R.merges(lib, case), (case, table[case])
    assert not any(R.merges(lib, case) for case in R.CASES3)


def test_both_sides_of_pools_on_load():
    lib = L()
    seen = set()
    for case in R.CASES3:
        for l, (c, ext) in enumerate(R.levels(case)[1:], 1):
            v = lib.cine_conv3d_pools_on_load(c, *ext)
            assert v in (0, 1)
            seen.add(v)
            print(f"{case} level {l}: {c} channels on {ext}: pools on load {v}")
    assert seen == {0, 1}


# ================================================================== pointer arrays
def _hip_net(case):
    from reconstruction.models.denoisers.unet import Unet
    t = R.ALL[case]
    return Unet(in_chans=t[1], out_chans=t[2], chans=t[3], num_pool_layers=t[4], drop_prob=0.0, dims=3 if R.is3d(case) else 2)


@pytest.mark.parametrize("case", ["odd-every-level", "wide-in", "six-pools", "odd3d", "two3d", "three3d"])
def test_pointer_array_order_and_packing_match_the_binding(case):
    from cine_hip import ops
    net = _hip_net(case)
    wts = ops.UnetWeights([net])
    (seq,) = wts._params()
    mine, plan = R.slots(net), R.pack_plan(net)
    P = R.ALL[case][4]
    assert len(seq) == len(mine) == len(plan) == 5 * P + 4
    three = R.is3d(case)
    for (kind, p), (_, q), (fwd, dg) in zip(seq, mine, plan):
        assert p is q
        if kind == "raw":
            assert fwd is None and dg is None
            continue
        k = ops._KINDS[kind]
        assert (k.pack_fn, k.floats_fn) == (fwd[0], fwd[0].replace("cine_pack_", "cine_") + "_packed_floats")
        assert (fwd[2], fwd[3]) == tuple(p.shape[:2]) and fwd[1](p) is p
        dkind, view = (wts._DGRAD_3D if three else wts._DGRAD)[kind]
        dk = ops._KINDS[dkind]
        want = p.detach() if view is None else view(p.detach())
        got = dg[1](p.detach())
        assert dk.pack_fn == dg[0] and (dg[2], dg[3]) == tuple(want.shape[:2])
        assert got.shape == want.shape and torch.equal(got, want) and got.is_contiguous()
    ref = R.make_net(case, 1)                        # the oracle's slots have the shapes of the module's
    assert [tuple(p.shape) for _, p in R.slots(ref)] == [tuple(p.shape) for _, p in mine]
    # the Dropout blocks: one per 3x3 conv, in the order of the slots that hold them
    chs = R.conv_channels(case)
    assert len(chs) == 4 * P + 2 and [mine[R.conv_slot(case, j)][1].shape[0] for j in range(len(chs))] == chs


def test_every_unet_entry_point_of_the_header_is_called_by_the_sweep():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "cine_hip.h")) as f:
        names = set(re.findall(r"\b(cine_unet[23]d_\w+)\s*\(", f.read()))
    assert len(names) == 18, sorted(names)
    text = ""
    for fn in ("unet_reference.py", "test_unet_sequences.py", "test_unet_sequences_cpu.py"):
        with open(os.path.join(here, fn)) as f:
            text += f.read()
    stems = ("cine_unet3d_backward", "cine_unet2d_backward")        # called as getattr(L, stem) and getattr(L, stem + "_drop")
    missing = [n for n in names if not re.search(rf"\bL\.{n}\b|lib\.{n}\b", text) and not n.startswith(stems)]
    assert not missing, missing


# ================================================================== size queries
EXTRA = {"cfg2-level": (2, 2, 2, 16, 3, 208, 16), "sens": (1, 2, 2, 8, 4, 208, 208)}


def _floors(lib, case, n):
    """(inference, training) floors in floats: every kept tensor with its records; three times the largest layer with the largest record block,
    plus the skips (and in 3-D the unmerged records of the widest layer, which every launch writes before the merge)."""
    three = R.is3d(case)
    kept = R.kept_tensors(case, n)
    rec = lambda c, l, tc: n * c * 3 * (1 if three else R.records(lib, case, l, tc))          # noqa: E731
    train = sum(f + rec(c, l, tc) for f, c, l, tc in kept)
    P = R.ALL[case][4]
    skips = sum(f + rec(c, l, tc) for f, c, l, tc in kept[1:2 * P:2])
    inf = 3 * (max(f for f, *_ in kept) + max(rec(c, l, tc) for _, c, l, tc in kept)) + skips
    if three:
        raw = max(n * c * 3 * R.records(lib, case, l, tc) for _, c, l, tc in kept)
        inf, train = inf + raw, train + raw
    return inf, train


@pytest.mark.parametrize("case", list(R.ALL) + list(EXTRA))
def test_workspace_sizes_hold_the_layer_plan(case):
    lib = L()
    if case in EXTRA:
        R.ALL[case] = EXTRA[case]
    try:
        prev = (0, 0, 0)
        for n in (1, 2, 3, 5, 8):
            a = R.dims(case, n=n)
            cur = R.ws_sizes(lib, a)
            inf, train = _floors(lib, case, n)
            assert all(c > 0 and c % 256 == 0 and c >= p for c, p in zip(cur, prev)), (n, cur, prev)
            assert cur[0] >= 4 * inf and cur[1] >= 4 * train, (n, cur, inf, train)
            # the backward's scratch: three gradient buffers as large as the largest layer or the input gradient, the concat gradients of every level
            lv = R.levels(case)
            big = max([n * c * int(np.prod(e)) for c, e in lv] + [n * a.cin * int(np.prod(lv[0][1]))])
            cat = sum(2 * n * c * int(np.prod(e)) for c, e in lv[:-1])
            assert cur[2] >= 4 * (3 * big + cat), (n, cur[2], big, cat)
            prev = cur
    finally:
        if case in EXTRA:
            del R.ALL[case]


@pytest.mark.parametrize("case", list(R.CASES3))
def test_3d_workspace_sizes_are_exactly_the_layer_plan(case):
    """The 3-D layouts restated buffer by buffer (every buffer rounded up to 256 bytes): the skips, three scratch buffers (or every kept tensor),
    each with one merged record per (sample, channel); the unmerged records of the layer that emits most -- a conv OR a transpose conv --; the
    pooled input of the widest level that does not pool on load.  The floors above leave the rounding slack of some 30 buffers, which hides a
    record block a few hundred bytes short."""
    lib = L()
    r256 = lambda floats: (4 * floats + 255) // 256 * 256                       # noqa: E731
    P = R.ALL[case][4]
    lv = R.levels(case)
    for n in (1, 2, 5):
        kept = R.kept_tensors(case, n)
        raw = r256(max(n * c * 3 * R.records(lib, case, l, tc) for _, c, l, tc in kept))
        pool = max([n * lv[l - 1][0] * int(np.prod(lv[l][1])) for l in range(1, P + 1) if not lib.cine_conv3d_pools_on_load(lv[l][0], *lv[l][1])] + [0])
        tail = raw + (r256(pool) if pool else 0)
        train = sum(r256(f) + r256(n * c * 3) for f, c, _, _ in kept) + tail
        skips = sum(r256(f) + r256(n * c * 3) for f, c, _, _ in kept[1:2 * P:2])
        inf = skips + 3 * (r256(max(n * c * int(np.prod(e)) for c, e in lv)) + r256(n * lv[P][0] * 3)) + tail
        got = R.ws_sizes(lib, R.dims(case, n=n))
        assert got[:2] == (inf, train), (case, n, got, inf, train)


@pytest.mark.parametrize("case", ["plane16", "merge-l0", "odd-every-level"])
def test_branch_workspace_is_the_sum_over_the_runs(case):
    lib = L()
    for n in (1, 2, 3, 6, 7, 8, 16):
        for nsets in (1, 2):
            a = R.dims(case, n=n, nsets=nsets)
            for nb in range(0, 11):
                ok = n % nsets == 0 and (nb == 1 or (2 <= nb <= 8 and nb % nsets == 0 and n // nb >= 1))
                inf, train = R.branch_ws(lib, a, nb, 0), R.branch_ws(lib, a, nb, 1)
                if not ok:
                    assert inf == 0 and train == 0, (n, nsets, nb)
                    continue
                if nb == 1:
                    runs = [n]
                else:
                    per, ns = nb // nsets, n // nsets
                    runs = [ns * (j + 1) // per - ns * j // per for _ in range(nsets) for j in range(per)]
                    runs = [r for r in runs if r > 0]
                assert sum(runs) == n
                assert inf == sum(R.ws_sizes(lib, R.dims(case, n=r))[0] for r in runs), (n, nsets, nb, runs)
                assert train == R.ws_sizes(lib, a)[1]


def test_drop_floats():
    lib = L()
    for case in R.ALL:
        t = R.ALL[case]
        for n in (1, 2, 5):
            assert lib.cine_unet2d_drop_floats(n, t[3], t[4]) == R.drop_floats(case, n)
    assert [lib.cine_unet2d_drop_floats(*t) for t in ((0, 4, 2), (1, 0, 2), (1, 4, 0), (1, 4, 7), (-1, 4, 2))] == [0] * 5


# ================================================================== refusals (all before the first launch)
def _fake(three, nsets=None):
    a = R.refusal_dims(three)
    nptr = 5 * a.pools + 4
    ns = nsets or a.nsets
    fake = lambda k: [0x100000 * (k + 1) + 256 * i for i in range(ns * nptr)]          # noqa: E731  never dereferenced: every call is refused first
    wd = fake(1)
    for s in range(ns):
        wd[s * nptr + nptr - 1] = None
    return dict(x=0x1000, y=0x2000, gy=0x3000, gx=0x4000, ws=0x5000, ws_bytes=1 << 40, fwd_ws=0x6000, fwd_bytes=1 << 40, bws=0x9000, bws_bytes=1 << 40,
                stream=None, weights=fake(0), wdgrad=wd, grads=fake(2), side=[0x7100, 0x7200, 0x7300, 0x7400, 0x7500, 0x7600, 0x7700], nside=1, train=0,
                drop=None), nptr


def _assert_refused(lib, three, e, a, p, code, what):
    assert lib.cine_scale(None, 1, 1.0, None) == R.EINVAL and lib.cine_last_error().startswith(b"cine_scale")
    got = R.entry_call(lib, e, a, p)
    msg = lib.cine_last_error().decode(errors="replace")
    name = R.ENTRY[(three, e)]
    assert got == code, (name, what, got, msg)
    assert msg.startswith(name[:11] + R.MESSAGE[e]), (name, what, msg)


ROWS = [(three, e, r) for three in (False, True) for r in R.REFUSALS for e in (R.ENTRIES3 if three else R.ENTRIES2) if R.applies(r[3], e, three)]


@pytest.mark.parametrize("three,e,row", ROWS, ids=[f"{R.ENTRY[(t, e)][5:]}-{r[0].replace(' ', '_')}" for t, e, r in ROWS])
def test_refusals_before_any_launch(three, e, row):
    what, over, code, _ = row
    lib = L()
    over = {k: v for k, v in over.items() if three or k != "d"}
    a = R.refusal_dims(three, **over)
    p, _ = _fake(three, 3 if over.get("nsets") == 3 else None)
    for train in ((0, 1, 3) if e == "r" else (0,)):
        _assert_refused(lib, three, e, a, dict(p, train=train), code, what)
    # a size query refuses what its entry point refuses
    if not any(k in over for k in ("slope", "nsets")) and what != "n % nsets":
        inf, train, bwd = R.ws_sizes(lib, a)
        if what == "n 65536":
            assert bwd == 0, (what, bwd)
        else:
            assert (inf, train, bwd) == (0, 0, 0), (what, inf, train, bwd)
    if e == "r" and what != "slope NaN" and "slope" not in over:
        assert R.branch_ws(lib, a, 2, 0) == 0 and R.branch_ws(lib, a, 2, 1) == 0 and R.branch_ws(lib, a, 1, 1) == 0, what


@pytest.mark.parametrize("three", [False, True], ids=["2d", "3d"])
def test_null_pointers_and_null_slots_are_refused(three):
    lib = L()
    a = R.refusal_dims(three)
    p, nptr = _fake(three)
    for e in (R.ENTRIES3 if three else R.ENTRIES2):
        rows = R.pointer_refusals(e, p, three, nptr)
        assert len(rows) >= 4 + (nptr * (1 if three else 2) if e in "ftTr" else (2 * nptr - 1) * (1 if three else 2))
        for what, q in rows:
            _assert_refused(lib, three, e, a, q, R.EINVAL, what)


def test_branch_refusals():
    lib = L()
    p, _ = _fake(False)
    for train in (0, 1):
        for what, over, ops_over, code in R.branch_refusals(p):
            q = dict(p, train=train)
            q.update(ops_over)
            _assert_refused(lib, False, "r", R.refusal_dims(False, **over), q, code, what)


@pytest.mark.parametrize("three", [False, True], ids=["2d", "3d"])
def test_a_workspace_one_byte_short_is_refused(three):
    lib = L()
    a = R.refusal_dims(three)
    p, _ = _fake(three)
    inf, train, bwd = R.ws_sizes(lib, a)
    assert min(inf, train, bwd) > 0
    short = [("f", dict(ws_bytes=inf - 1)), ("t", dict(fwd_bytes=train - 1)), ("b", dict(fwd_bytes=train - 1, ws_bytes=bwd)),
             ("b", dict(fwd_bytes=train, ws_bytes=bwd - 1)), ("B", dict(fwd_bytes=train - 1, ws_bytes=bwd)), ("B", dict(fwd_bytes=train, ws_bytes=bwd - 1))]
    if three:
        short.append(("T", dict(fwd_bytes=train - 1)))
    else:
        for nb in (1, 2):
            for tr in (0, 1, 3):
                short.append(("r", dict(bws_bytes=R.branch_ws(lib, a, nb, tr & 1) - 1, nside=nb - 1, train=tr)))
    for e, sizes in short:
        _assert_refused(lib, three, e, a, dict(p, **sizes), R.EWORKSPACE, f"one byte short {sizes}")
