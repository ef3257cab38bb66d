"""The column-pure sweep of the 2-wide plane convolutions (csrc/conv_plane.hip, COLP = 1) against the general kernel
(cine_set_conv_plane(0)) and against the nine-tap sweep it replaces (mask 15): outputs and {count, mean, M2} records bit for bit.

A canonical fragment of a 2-wide plane is 8 rows x both columns; the new sweep works on (one column, 16 rows) and skips the taps that read
only the zero halo.  What can go wrong is the row / column a lane reads, the taps a fragment keeps, and the lane swaps that put the sums
back where the epilogue expects them -- so the heights cross every border of that map: 2 (one ragged fragment), 15 / 16 / 17 (one
16-row block, exactly and one off), 26 (the U-Net bottleneck), 31 / 32 / 33 (the 32-row tile with its row halo), 50 (two tiles).

Which kernel a layer takes follows conv_kernels.hip's dispatcher: 128 output rows run on <8, 2, 4, 1, 4, 2> up to 8 fragments per plane
(h <= 64), 64 rows on <8, 1, 4, 1, 4, 2> up to 4 (h <= 32); a taller 64-row layer has no plane-wide 2-wide shape and runs on the general
kernel under every mask.  cine_diag_counter (D_CONV_PLANE) is checked against that rule for every launch.

Every kind runs with 8 and 24 conv input channels (1 and 3 chunks).  For the Haar-DWT source (mode 3) those are 2 and 6 source channels,
and the lean kernel takes a DWT source in whole groups of 8 source channels only: these cases run on the general kernel under every mask
(the counter says so), and the three results are equal.  The DWT launches that DO reach the lean kernel -- 8 and 24 source channels, 32 and
96 conv input channels, 64 output rows, h <= 32 -- have a test of their own: bit for bit against the nine-tap sweep, which is the same
kernel with the same chunks, and against the general kernel at the bound that pair of kernels has always had (see there).
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from kernel_sweep import BAR
from oracle.xpdnet_ref import DWT

pytestmark = pytest.mark.gpu

HEIGHTS = (2, 15, 16, 17, 26, 31, 32, 33, 50)
KINDS = ("plain", "norm", "pool", "dwt", "relu")
D_CONV_PLANE = 4                    # cine_diag_counter id (csrc/common.h)
N = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def lean_expected(kind, cin, cout, h):
    frags = (2 * h + 15) // 16
    if kind == "dwt":
        return (cin // 4) % 8 == 0 and cout == 64 and frags <= 4        # the only 2-wide DWT shape of conv_plane.hip, whole groups of 8 source channels
    return frags <= (8 if cout == 128 else 4)


def make_case(kind, cin, cout, h, seed, zero=None):
    """(x on the CPU, weights a / b, bias).  `cin` counts the conv's input channels (kind dwt: cin / 4 source channels, four bands each)."""
    g = torch.Generator().manual_seed(seed)
    wa = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    wb = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    hs, ws = (2 * h, 4) if kind in ("pool", "dwt") else (h, 2)
    x = torch.randn(N, cin // 4 if kind == "dwt" else cin, hs, ws, generator=g)
    if zero == "all":
        x.zero_()
    elif zero == "col0":
        x[..., 0] = 0.
    bias = torch.randn(cout, generator=g) if kind == "relu" else None
    return x, wa, wb, bias


def run(ops, kind, x, wa, wb, bias, cout, h):
    """One launch on the calling thread's current mask -> (y, records or None)."""
    if kind == "relu":
        return ops.conv3x3_sum([x], ops.pack_conv3x3(wa), bias, cout, relu=True), None
    mode = {"plain": 0, "norm": 1, "pool": 2, "dwt": 3 | 8}[kind]
    part = None if kind == "plain" else ops.instnorm_partials(x)
    return ops.conv3x3_in([(x, part, mode)], ops.pack_conv3x3(wa), cout, h, 2, wpacked2=ops.pack_conv3x3(wb), set_split=2)


def three_ways(dev, kind, cin, cout, h, seed, zero=None):
    """The case under masks 7 (new sweep), 15 (nine-tap sweep) and 0 (general kernel), with the route each launch took."""
    from cine_hip import ops
    from cine_hip._lib import lib
    x, wa, wb, bias = make_case(kind, cin, cout, h, seed, zero)
    x, wa, wb = x.to(dev), wa.to(dev), wb.to(dev)
    bias = None if bias is None else bias.to(dev)
    outs = {}
    try:
        for mask in (7, 15, 0):
            ops.set_conv_plane(mask)
            before = lib().cine_diag_counter(D_CONV_PLANE, 0)
            outs[mask] = run(ops, kind, x, wa, wb, bias, cout, h)
            took = lib().cine_diag_counter(D_CONV_PLANE, 0) - before
            want = 1 if mask != 0 and lean_expected(kind, cin, cout, h) else 0
            assert took == want, (kind, cin, cout, h, mask, took)
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
def test_tw2_column_pure_sweep_same_bits(dev, kind):
    """New sweep == nine-tap sweep == general kernel, y and records, every height, 64 / 128 output rows, 8 and 24 input channels (1 and 3
    chunks), two weight sets.  (kind dwt: 2 and 6 source channels, which no lean kernel takes -- the general kernel three times.)"""
    for cout in (64, 128):
        for cin in (8, 24):
            for h in HEIGHTS:
                o = three_ways(dev, kind, cin, cout, h, seed=1000 * cout + 10 * cin + h)
                assert_same_bits(o[7], o[15], (kind, "new vs nine-tap", cin, cout, h))
                assert_same_bits(o[7], o[0], (kind, "new vs general", cin, cout, h))


DWT_REORDER_BAR = 2e-6              # max |d| / peak, lean against general kernel on a DWT source (tests/test_hip_parity.py: the same pair, the same bar)
DWT_STATS_BAR = 1e-5                # the finalised {mean, rstd} of their records (ditto)


def test_tw2_column_pure_sweep_dwt_on_the_lean_kernel(dev):
    """Haar DWT on load where the lean kernel takes it (whole groups of 8 source channels: 8 and 24, i.e. 32 and 96 conv input channels).

    Against the nine-tap sweep: y and records bit for bit -- the same kernel, chunks and order, minus the zero products.
    Against the general kernel: NOT the same bits, before this sweep as after it.  The lean kernel forms a DWT chunk from the four bands of
    two source channels, the general kernel from eight channels of one band (include/cine_hip.h, cine_set_conv_plane), so each output is the
    same 9 x 32 .. 9 x 96 products summed in another order.  Two float32 sums of K terms of one sign pattern differ by about sqrt(K) ulp of
    the partial sums: sqrt(864) x 6e-8 = 1.8e-6 of the peak at the widest case.  The bar is the one tests/test_hip_parity.py has held this
    pair of kernels to since the lean DWT chunks exist (2e-6 on y, 1e-5 on the finalised statistics), and the nine-tap sweep must show the
    SAME difference from the general kernel to the last bit, or the column-pure sweep changed something."""
    from cine_hip import ops
    for cout in (64, 128):
        for src in (8, 24):
            for h in HEIGHTS:
                o = three_ways(dev, "dwt", 4 * src, cout, h, seed=77 * cout + 10 * src + h)
                what = ("dwt", src, cout, h)
                assert_same_bits(o[7], o[15], what + ("new vs nine-tap",))
                d7 = rel_err(o[7][0], o[0][0])
                s7 = rel_err(ops.instnorm_finalize(o[7][1]), ops.instnorm_finalize(o[0][1]))
                print(f"dwt cout {cout} source channels {src} h {h}: y vs general {d7:.3e}, statistics {s7:.3e}")
                if lean_expected("dwt", 4 * src, cout, h):
                    assert d7 < DWT_REORDER_BAR and s7 < DWT_STATS_BAR, what + (d7, s7)
                else:                                   # no lean shape: the general kernel under every mask
                    assert_same_bits(o[7], o[0], what + ("new vs general",))


@pytest.fixture(scope="module")
def f64_refs():
    """float64 conv2d of one case per kind (h = 26, the bottleneck's height; 24 input channels), computed once."""
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
        cout = 64 if kind == "dwt" else 128
        cin = 32 if kind == "dwt" else 24               # dwt: 8 source channels, the lean kernel's <8, 1, 4, 1, 4, 2, 3>
        x, wa, wb, bias = make_case(kind, cin, cout, 26, seed=4242)
        inp = {"plain": lambda: x.double(), "relu": lambda: x.double(), "norm": lambda: act(x),
               "pool": lambda: F.avg_pool2d(act(x), 2), "dwt": lambda: DWT()(act(x))}[kind]()
        if kind == "relu":
            ref = torch.relu(F.conv2d(inp, wa.double(), bias.double(), padding=1))
        else:
            ref = torch.cat([F.conv2d(inp[:2], wa.double(), padding=1), F.conv2d(inp[2:], wb.double(), padding=1)])
        refs[kind] = (cin, cout, ref)
    return refs


@pytest.mark.parametrize("kind", KINDS)
def test_tw2_column_pure_sweep_against_float64(dev, f64_refs, kind):
    """max |d| / peak against float64 conv2d at the bar of tests/test_conv_fwd_kernels.py (kernel_sweep.BAR), records against y."""
    cin, cout, ref = f64_refs[kind]
    o = three_ways(dev, kind, cin, cout, 26, seed=4242)
    y, part = o[7]
    err = rel_err(y.cpu(), ref)
    print(f"{kind}: max|d|/peak vs float64 = {err:.3e}")
    assert err < BAR, (kind, err)
    if part is not None:
        p = part.double().cpu()
        assert float(p[..., 0].sum(-1).min()) == float(p[..., 0].sum(-1).max()) == 52.0
        mean = (p[..., 0] * p[..., 1]).sum(-1) / 52.0
        assert float((mean - y.double().cpu().mean((2, 3))).abs().max()) < 2e-6 * max(1.0, float(ref.abs().max())), kind


@pytest.mark.parametrize("zero", ["all", "col0"])
def test_tw2_column_pure_sweep_zero_columns(dev, zero):
    """An all-zero plane and a plane that is zero in column 0 only: the skipped products are then not the only zero ones, and a sum may
    stay at +0 all the way -- the bit patterns (signed zeros included) equal both other kernels'."""
    for kind in ("plain", "norm", "relu"):
        for h in (17, 26):
            o = three_ways(dev, kind, 8, 128, h, seed=31 + h, zero=zero)
            assert_same_bits(o[7], o[15], (kind, zero, "new vs nine-tap", h))
            assert_same_bits(o[7], o[0], (kind, zero, "new vs general", h))
            if zero == "all" and kind == "plain":
                assert torch.equal(bits(o[7][0]), torch.zeros_like(bits(o[7][0]))), (kind, zero, h)        # +0 everywhere
