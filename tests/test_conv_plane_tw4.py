"""The column-pure sweep of the 4-wide plane convolutions with one wave per plane tile (csrc/conv_plane.hip, <8, 1, 4, 1, 13, 4, MODE, COLP = 1>:
U-Net level 2) against the general kernel (cine_set_conv_plane(0)) and against the nine-tap sweep it replaces (mask 15): outputs and
{count, mean, M2} records bit for bit.

A canonical fragment of a 4-wide plane is 4 rows x all four columns.  The new sweep works on 12 fragments of (one column, 16 rows) for rows
0 .. 47 of a 52-row tile, keeps the thirteenth fragment (rows 48 .. 51) canonical, skips the taps that read only the zero halo column, and
transposes lane rows against registers after the last chunk.  What can go wrong is the row / column a lane reads, the taps a fragment keeps,
the rolling operand loads, the transpose, and the seam between the pure and the mixed fragment -- so the heights cross every border of that
map: 17 (one 16-row block and one row), 31 / 32 / 33, 47 / 48 / 49 (the last pure row and the first rows of the mixed fragment), 51 / 52 (the
tile, one off and exactly), 57 and 104 (two tiles, ragged and full).

Which kernel a layer takes follows conv_kernels.hip's dispatcher (regular_nf / dispatch_tw): 33 .. 64 output rows on a 4-wide plane run on
<8, 1, 4, 1, 4, 4> up to 4 fragments per plane (h <= 16), which conv_plane.hip does not have, and on <8, 1, 4, 1, 13, 4> above that (the
14-fragment rule is for 17 .. 32 output rows).  The lean kernel takes two concatenated sources only when the first is whole 8-channel chunks.
cine_diag_counter (D_CONV_PLANE) is checked against that rule for every launch.

Every kind runs with 8 and 24 conv input channels (1 and 3 chunks) and two weight sets (set_split).  The two-source kind splits 24 channels
as 8 + 16 (the lean kernel) and 8 channels as 4 + 4 (no lean shape: the general kernel under every mask, and the counter says so).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from kernel_sweep import BAR

pytestmark = pytest.mark.gpu

HEIGHTS = (17, 31, 32, 33, 47, 48, 49, 51, 52, 57, 104)
KINDS = ("plain", "norm", "concat", "pool", "relu")
D_CONV_PLANE = 4                    # cine_diag_counter id (csrc/common.h)
N, W, COUT = 3, 4, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def split(kind, cin):
    """Channels of source 0 (kind concat: the rest is source 1)."""
    return (8 if cin > 8 else 4) if kind == "concat" else cin


def lean_expected(kind, cin, h):
    frags = (W * h + 15) // 16
    if kind == "concat" and split(kind, cin) % 8 != 0:
        return False
    return frags > 4                # 64 output rows: 4-fragment tiles up to 4 fragments, 13-fragment tiles above


def pool_rows(h):
    """Source height of the pooled kind: 2 h, and 2 h + 1 (the odd row is dropped by the pool) at every other height."""
    return 2 * h + (h % 2)


def make_case(kind, cin, h, seed, zero=None):
    """(x on the CPU, weights a / b, bias)."""
    g = torch.Generator().manual_seed(seed)
    wa = torch.randn(COUT, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    wb = torch.randn(COUT, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    hs, ws = (pool_rows(h), 2 * W) if kind == "pool" else (h, W)
    x = torch.randn(N, cin, hs, ws, generator=g)
    if zero == "all":
        x.zero_()
    elif zero == "cols":
        x[..., 0] = 0.
        x[..., W - 1] = 0.
    bias = torch.randn(COUT, generator=g) if kind == "relu" else None
    return x, wa, wb, bias


def run(ops, kind, x, wa, wb, bias, h):
    """One launch on the calling thread's current mask -> (y, records or None)."""
    if kind == "relu":
        return ops.conv3x3_sum([x], ops.pack_conv3x3(wa), bias, COUT, relu=True), None
    if kind == "plain":
        srcs = [(x, None, 0)]
    elif kind == "concat":
        c0 = split(kind, x.shape[1])
        x0, x1 = x[:, :c0].contiguous(), x[:, c0:].contiguous()
        srcs = [(x0, ops.instnorm_partials(x0), 1), (x1, ops.instnorm_partials(x1), 1)]
    else:
        srcs = [(x, ops.instnorm_partials(x), {"norm": 1, "pool": 2}[kind])]
    return ops.conv3x3_in(srcs, ops.pack_conv3x3(wa), COUT, h, W, wpacked2=ops.pack_conv3x3(wb), set_split=2)


def three_ways(dev, kind, cin, h, seed, zero=None):
    """The case under masks 7 (new sweep), 15 (nine-tap sweep) and 0 (general kernel), with the route each launch took."""
    from cine_hip import ops
    from cine_hip._lib import lib
    x, wa, wb, bias = make_case(kind, cin, h, seed, zero)
    x, wa, wb = x.to(dev), wa.to(dev), wb.to(dev)
    bias = None if bias is None else bias.to(dev)
    outs = {}
    try:
        for mask in (7, 15, 0):
            ops.set_conv_plane(mask)
            before = lib().cine_diag_counter(D_CONV_PLANE, 0)
            outs[mask] = run(ops, kind, x, wa, wb, bias, h)
            took = lib().cine_diag_counter(D_CONV_PLANE, 0) - before
            want = 1 if mask != 0 and lean_expected(kind, cin, h) else 0
            assert took == want, (kind, cin, h, mask, took)
    finally:
        ops.set_conv_plane(7)
    return outs


def assert_same_bits(a, b, what):
    (ya, pa), (yb, pb) = a, b
    assert torch.equal(ya, yb) and torch.equal(bits(ya), bits(yb)), what + (float((ya - yb).abs().max()),)
    assert (pa is None) == (pb is None), what
    if pa is not None:
        assert torch.equal(pa, pb) and torch.equal(bits(pa), bits(pb)), what


@pytest.mark.parametrize("kind", KINDS)
def test_tw4_column_pure_sweep_same_bits(dev, kind):
    """New sweep == nine-tap sweep == general kernel, y and records, every height, 8 and 24 input channels (1 and 3 chunks), two weight sets."""
    for cin in (8, 24):
        for h in HEIGHTS:
            o = three_ways(dev, kind, cin, h, seed=1000 * COUT + 10 * cin + h)
            assert_same_bits(o[7], o[15], (kind, "new vs nine-tap", cin, h))
            assert_same_bits(o[7], o[0], (kind, "new vs general", cin, h))


F64_H = 57                          # two tiles: a full one (pure and mixed fragments) and a ragged one


@pytest.fixture(scope="module")
def f64_refs():
    """float64 conv2d of one case per kind (h = 57, 24 input channels), computed once."""
    from cine_hip import ops
    eps, slope = ops.IN_EPS, ops.lrelu_slope()

    def act(x):
        x = x.double()
        mean = x.mean((2, 3), keepdim=True)
        var = (x - mean).pow(2).mean((2, 3), keepdim=True)
        v = (x - mean) / torch.sqrt(var + eps)
        return torch.where(v > 0, v, v * slope)

    refs = {}
    for kind in KINDS:
        x, wa, wb, bias = make_case(kind, 24, F64_H, seed=4242)
        inp = {"plain": lambda: x.double(), "relu": lambda: x.double(), "norm": lambda: act(x), "concat": lambda: act(x),
               "pool": lambda: F.avg_pool2d(act(x), 2)}[kind]()           # InstanceNorm is per channel: the concat of two sources == one
        if kind == "relu":
            ref = torch.relu(F.conv2d(inp, wa.double(), bias.double(), padding=1))
        else:
            ref = torch.cat([F.conv2d(inp[:2], wa.double(), padding=1), F.conv2d(inp[2:], wb.double(), padding=1)])
        refs[kind] = ref
    return refs


@pytest.mark.parametrize("kind", KINDS)
def test_tw4_column_pure_sweep_against_float64(dev, f64_refs, kind):
    """max |d| / peak against float64 conv2d at the bar of tests/test_conv_fwd_kernels.py (kernel_sweep.BAR), records against y."""
    ref = f64_refs[kind]
    o = three_ways(dev, kind, 24, F64_H, seed=4242)
    y, part = o[7]
    err = rel_err(y.cpu(), ref)
    print(f"{kind}: max|d|/peak vs float64 = {err:.3e}")
    assert err < BAR, (kind, err)
    if part is not None:
        p = part.double().cpu()
        assert float(p[..., 0].sum(-1).min()) == float(p[..., 0].sum(-1).max()) == float(F64_H * W)
        mean = (p[..., 0] * p[..., 1]).sum(-1) / float(F64_H * W)
        assert float((mean - y.double().cpu().mean((2, 3))).abs().max()) < 2e-6 * max(1.0, float(ref.abs().max())), kind


@pytest.mark.parametrize("zero", ["all", "cols"])
def test_tw4_column_pure_sweep_zero_columns(dev, zero):
    """An all-zero plane and a plane that is zero in columns 0 and 3: the skipped products are then not the only zero ones, and a sum may
    stay at +0 all the way -- the bit patterns (signed zeros included) equal both other kernels'."""
    for kind in ("plain", "norm", "relu"):
        for h in (17, 52):
            o = three_ways(dev, kind, 8, h, seed=31 + h, zero=zero)
            assert_same_bits(o[7], o[15], (kind, zero, "new vs nine-tap", h))
            assert_same_bits(o[7], o[0], (kind, zero, "new vs general", h))
            if zero == "all" and kind == "plain":
                assert torch.equal(bits(o[7][0]), torch.zeros_like(bits(o[7][0]))), (kind, zero, h)        # +0 everywhere
