"""cine_noise_add_raw (noise on the raw layout (t, nx, ny, c), coil fastest) against tests/noise_reference.py permuted to that layout, and
bit for bit against cine_noise_add on the permuted data -- the contract of include/cine_hip.h.

A workgroup owns a run of 64 consecutive flat points, so the shapes are chosen by what a run does: (2, 5, 7, 3) an odd coil count, runs
that straddle lines and frames; (1, 3, 70, 5) a line longer than a run; (3, 4, 6, 64) the coil limit (L, z and eta share the 64 KB);
(2, 9, 1, 1) ny = 1 and one coil; (1, 2, 33, 2) a ragged last run; 32 and 33 coils, between which a lane goes from 8 to 16 held
elements.  Each with white and coloured noise, without a mask, with a line mask
(t, nx) and a sample mask (t, nx, ny) -- where the shape has more than one run, a mask leaves one run fully unsampled and one partly
sampled -- at point0 = 0 and at one that makes p cross 2^32, with a negative seed, at storage offsets of 0 and 2 floats.  The bar is
kernel_sweep.BAR of the noise's peak, the bar cine_noise_add is held to: the raw data are of the noise's size, so the rounding of the
final addition (2^-24 of the sum) is far below it."""
import numpy as np
import pytest
import torch

import noise_reference as R
from kernel_sweep import BAR, EINVAL, EUNSUPPORTED, Call, L, Worst, at_offsets, check, ptr, refused, same_bits, stream

pytestmark = pytest.mark.gpu
WORST = Worst()
OFFS = (0, 2)
SEED, REPLICA, SCALE = 0x5DEECE66D1234567, 5, 0.75
RUN = 64
SHAPES = [(2, 5, 7, 3), (1, 3, 70, 5), (3, 4, 6, 64), (2, 9, 1, 1), (1, 2, 33, 2),
          (1, 2, 40, 32), (1, 2, 40, 33)]           # the two sides of the coil count at which the launch takes the kernel's wider form
MASKS = ["none", "line", "sample"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def pairs(z):
    return torch.from_numpy(np.stack([z.real, z.imag], axis=-1).astype(np.float32))


def cplx(t):
    a = t.double().numpy()
    return a[..., 0] + 1j * a[..., 1]


def run_counts(on):
    """Sampled points per run of 64 flat points, and the points per run."""
    flat = np.asarray(on, dtype=np.int64).reshape(-1)
    edges = np.arange(0, flat.size, RUN)
    return np.add.reduceat(flat, edges), np.diff(np.append(edges, flat.size))


def make_mask(rs, shape, kind):
    """uint8 (t, nx) / (t, nx, ny) / None.  Point 0 is sampled; with more than one run the last run is fully unsampled and another one
    partly sampled; with one run that run is partly sampled."""
    t, nx, ny, _ = shape
    if kind == "none":
        return None
    n = t * nx * ny
    last = (n - 1) // RUN * RUN                                               # first point of the last run
    if kind == "line":
        m = (rs.uniform(size=t * nx) < 0.5).astype(np.uint8)
        m[0] = 1
        if n > RUN:
            m[last // ny:] = 0                                                # every line that reaches into the last run
        else:
            m[-1] = 0
        m = m.reshape(t, nx)
    else:
        m = (rs.uniform(size=n) < 0.5).astype(np.uint8)
        m[0], m[1] = 1, 0
        if n > RUN:
            m[last:] = 0
        m = m.reshape(t, nx, ny)
    on, size = run_counts(sampled(m, shape))
    assert ((on > 0) & (on < size)).any(), "no partly sampled run"
    assert n <= RUN or (on == 0).any(), "no fully unsampled run"
    return m


def sampled(m, shape):
    """bool (t, nx, ny) of a mask (t, nx), (t, nx, ny) or None."""
    t, nx, ny, _ = shape
    if m is None:
        return np.ones((t, nx, ny), dtype=bool)
    return np.broadcast_to(m.reshape(t, nx, -1).astype(bool), (t, nx, ny))


def operands(seed, shape, mask, chol):
    """raw (t, nx, ny, c, 2) float32 of unit size, nonzero; the mask; L (c, c) complex64 or None."""
    rs = np.random.RandomState(seed)
    t, nx, ny, c = shape
    raw = torch.from_numpy(rs.standard_normal((t, nx, ny, c, 2)).astype(np.float32))
    return raw, make_mask(rs, shape, mask), (R.random_chol(rs, c)[0] if chol else None)


def raw_call(rd, out, md, mask_ny, ld, shape, seed=SEED, replica=REPLICA, rdev=None, point0=0, scale=SCALE):
    t, nx, ny, c = shape
    check(L().cine_noise_add_raw(ptr(rd), out, ptr(md), mask_ny, ptr(ld), scale, seed, replica, ptr(rdev), point0, t, nx, ny, c, stream()),
          "cine_noise_add_raw")


def run(dev, raw, m, low, shape, offs=OFFS, inplace=False, **kw):
    """The call on fresh guarded operands at every offset of offs (twice each, the same bits): its output on the CPU."""
    mask_ny = 1 if m is None or m.ndim == 2 else shape[2]

    def body(call):
        md = None if m is None else call.raw(torch.from_numpy(m))
        ld = None if low is None else call.inp(pairs(low))
        if inplace:
            o = call.out(raw.shape, fill=raw)
            raw_call(o.t, o.ptr(), md, mask_ny, ld, shape, **kw)
        else:
            o = call.out(raw.shape)
            raw_call(call.inp(raw), o.ptr(), md, mask_ny, ld, shape, **kw)
        return [o.t]
    return at_offsets(dev, offs, body, "cine_noise_add_raw")[0]


def planar(dev, raw, m, low, shape, seed=SEED, replica=REPLICA, point0=0, scale=SCALE):
    """cine_noise_add on the data permuted to (t, c, h = nx, w = ny), permuted back: what the raw kernel must give, bit for bit."""
    t, nx, ny, c = shape
    k = raw.permute(0, 3, 1, 2, 4).contiguous().to(dev)
    out = torch.full_like(k, float("nan"))
    md = None if m is None else torch.from_numpy(m).to(dev)
    ld = None if low is None else pairs(low).to(dev)
    mask_w = 1 if m is None or m.ndim == 2 else ny
    check(L().cine_noise_add(ptr(k), ptr(out), ptr(md), mask_w, ptr(ld), scale, seed, replica, None, point0, t, c, nx, ny, stream()), "cine_noise_add")
    torch.cuda.synchronize()
    return out.permute(0, 2, 3, 1, 4).contiguous().cpu()


def reference(raw, m, low, shape, **kw):
    """raw + eta at the sampled points in float64, and eta there: noise_reference.noise on (t, c, nx, ny), permuted to the raw layout."""
    t, nx, ny, c = shape
    eta = np.moveaxis(R.noise(t, c, nx, ny, chol=low, scale=SCALE, **kw), 1, -1) * sampled(m, shape)[..., None]
    return cplx(raw) + eta, eta


def crossing(shape):
    """A point0 that puts the carry into the high counter word inside the data (in the first run where there are several)."""
    t, nx, ny, _ = shape
    return 2 ** 32 - min(3, t * nx * ny - 1)


@pytest.mark.parametrize("chol", [0, 1], ids=["white", "coloured"])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_noise_add_raw_vs_reference_and_vs_noise_add(dev, shape, mask, chol):
    raw, m, low = operands(100 + 7 * SHAPES.index(shape) + 3 * MASKS.index(mask) + chol, shape, mask, chol)
    on = torch.from_numpy(np.broadcast_to(sampled(m, shape)[..., None], shape).copy())
    for kw in (dict(seed=SEED, point0=0), dict(seed=SEED, point0=crossing(shape)), dict(seed=-3, point0=0)):
        what = f"{shape} {mask} chol {chol} {kw}"
        kw = dict(kw, replica=REPLICA)
        got = run(dev, raw, m, low, shape, **kw)
        want, eta = reference(raw, m, low, shape, **kw)
        err, peak = float(np.abs(cplx(got) - want).max()), float(np.abs(eta).max())
        assert peak > 0.5 * SCALE
        WORST.record("cine_noise_add_raw", err, BAR * peak, what)
        assert same_bits(got[~on], raw[~on]), f"{what}: an unsampled sample changed"
        assert bool(((got != raw).any(dim=-1) == on).all()), f"{what}: a sampled sample kept its value"
        assert same_bits(got, planar(dev, raw, m, low, shape, **kw)), f"{what}: not the bits of cine_noise_add on the permuted data"
        assert same_bits(run(dev, raw, m, low, shape, inplace=True, **kw), got), f"{what}: in place differs from out of place"


@pytest.mark.parametrize("chol", [0, 1], ids=["white", "coloured"])
@pytest.mark.parametrize("mask", ["line", "sample"])
def test_unsampled_samples_are_not_touched_in_place(dev, mask, chol):
    """NaN at every unsampled sample, in place: they keep their bits and the sampled ones get the values of the clean input."""
    shape = (2, 5, 7, 3)
    raw, m, low = operands(31, shape, mask, chol)
    on = torch.from_numpy(np.broadcast_to(sampled(m, shape)[..., None], shape).copy())
    clean = run(dev, raw, m, low, shape, offs=(0,))
    holes = raw.clone()
    holes[~on] = float("nan")
    got = run(dev, holes, m, low, shape, offs=(0,), inplace=True)
    assert same_bits(got[~on], holes[~on]) and same_bits(got[on], clean[on]) and bool(torch.isnan(got[~on]).all())


@pytest.mark.parametrize("shape", [(2, 9, 1, 1), (2, 5, 7, 3)], ids=["one-run", "two-runs"])
def test_a_mask_that_samples_nothing(dev, shape):
    """Every run is fully unsampled: out of place a copy, in place nothing (NaN stays NaN)."""
    raw, _, low = operands(32, shape, "none", 1)
    t, nx, ny, _ = shape
    for m in (np.zeros((t, nx), dtype=np.uint8), np.zeros((t, nx, ny), dtype=np.uint8)):
        assert same_bits(run(dev, raw, m, low, shape), raw)
        nan = torch.full_like(raw, float("nan"))
        assert same_bits(run(dev, nan, m, low, shape, offs=(0,), inplace=True), nan)


def test_replica_dev_seed_and_replica(dev):
    """replica_dev gives the bits of the same replica by value; replicas r, r + 1 and seeds s, s + 1 differ at every sampled sample."""
    shape = (2, 5, 7, 3)
    raw, m, low = operands(33, shape, "sample", 1)
    on = torch.from_numpy(np.broadcast_to(sampled(m, shape)[..., None], shape).copy())
    base = run(dev, raw, m, low, shape, offs=(0,))
    counter = torch.tensor([REPLICA], dtype=torch.int64, device=dev)
    assert same_bits(run(dev, raw, m, low, shape, offs=(0,), replica=0, rdev=counter), base)
    counter += 1
    torch.cuda.synchronize()
    nxt = run(dev, raw, m, low, shape, offs=(0,), replica=0, rdev=counter)
    assert same_bits(nxt, run(dev, raw, m, low, shape, offs=(0,), replica=REPLICA + 1))
    other_seed = run(dev, raw, m, low, shape, offs=(0,), seed=SEED + 1)
    for other in (nxt, other_seed):
        assert bool((other != base).any(dim=-1)[on].all()) and same_bits(other[~on], base[~on])


@pytest.mark.parametrize("mask,chol", [("line", 1), ("sample", 0), ("none", 1)])
def test_a_stack_of_frames_equals_its_frames_one_by_one(dev, mask, chol):
    """A t = 3 call equals three t = 1 calls with point0 advanced by nx ny each, bit for bit -- the runs of the two cut the data differently."""
    shape = (3, 5, 7, 3)
    t, nx, ny, c = shape
    raw, m, low = operands(34, shape, mask, chol)
    p0 = 2 ** 32 - 50
    whole = run(dev, raw, m, low, shape, offs=(0,), point0=p0)
    for f in range(t):
        one = run(dev, raw[f:f + 1], None if m is None else m[f:f + 1], low, (1, nx, ny, c), offs=(0,), point0=p0 + f * nx * ny)
        assert same_bits(one, whole[f:f + 1]), f"frame {f}"


def test_noise_add_raw_refusals(dev):
    shape = t, nx, ny, c = 2, 4, 6, 3
    raw, m, low = operands(35, shape, "line", 1)
    call = Call(dev, 0)
    rd, md, ld = call.inp(raw), call.raw(torch.from_numpy(m)), call.inp(pairs(low))
    o = call.out(raw.shape)
    base = dict(raw=ptr(rd), out=o.ptr(), mask=ptr(md), mask_ny=1, chol=ptr(ld), replica=0, point0=0, t=t, nx=nx, ny=ny, c=c)

    def f(**kw):
        a = dict(base, **kw)
        return lambda: L().cine_noise_add_raw(a["raw"], a["out"], a["mask"], a["mask_ny"], a["chol"], 1.0, 1, a["replica"], None, a["point0"],
                                              a["t"], a["nx"], a["ny"], a["c"], stream())
    refused(f(c=65), EUNSUPPORTED, call, "cine_noise_add_raw c = 65")
    assert b"64" in L().cine_last_error()
    refused(f(t=2 ** 40, nx=1024, ny=1024, mask_ny=1024), EUNSUPPORTED, call, "cine_noise_add_raw a grid beyond the launch limits")
    refused(f(mask_ny=2), EINVAL, call, "cine_noise_add_raw mask_ny = 2")
    refused(f(mask_ny=nx), EINVAL, call, "cine_noise_add_raw mask_ny = nx")
    refused(f(replica=-1), EINVAL, call, "cine_noise_add_raw replica = -1")
    refused(f(replica=2 ** 32), EINVAL, call, "cine_noise_add_raw replica = 2^32")
    refused(f(point0=-1), EINVAL, call, "cine_noise_add_raw point0 = -1")
    refused(f(raw=None), EINVAL, call, "cine_noise_add_raw raw = NULL")
    refused(f(out=None), EINVAL, call, "cine_noise_add_raw out = NULL")
    refused(f(nx=0), EINVAL, call, "cine_noise_add_raw nx = 0")
    refused(f(out=o.ptr() + 4), EINVAL, call, "cine_noise_add_raw out off its alignment")
    refused(f(out=o.ptr() + 8, raw=o.ptr()), EINVAL, call, "cine_noise_add_raw out overlaps raw")
    check(f()(), "cine_noise_add_raw")
    call.finish("cine_noise_add_raw")
