"""cine_noise_add, cine_replica_accum and cine_replica_finish against tests/noise_reference.py (the definition of include/cine_hip.h
restated in numpy: uint64 Philox, float64 Box-Muller, colouring and Welford).

cine_noise_add: a seeded sweep in which every value of every axis appears -- c in {1, 2, 5, 64} (one coil, one pair, an odd last coil,
the limit), (h, w) in {(7, 13), (16, 12), (3, 1), (1, 40)}, bt in {1, 3}, no / row / plane mask, white / coloured, point0 in {0, 2^32 - 3}
(the carry into the high counter word) -- at storage offsets of 0 and 2 floats.  The bar: max |out - (kspace + eta_ref)| <= BAR x
max |eta_ref|; the k-space is of the noise's size, so the rounding of the final addition (2^-24 of the sum) is far below it.  Unsampled
points keep the input's bits, in place equals out of place, a second call gives the same bits, guards stay intact.
The statistics: 8 samples at 1, 63 and 4097 map elements, real and complex, with and without ref_std, at BAR of each map's peak."""
import numpy as np
import pytest
import torch

import noise_reference as R
from kernel_sweep import (BAR, EINVAL, EUNSUPPORTED, Call, Guarded, GuardedF64, L, Worst, at_offsets, case_id, check, hash_case, ptr,
                          refused, same_bits, stream, sweep)

pytestmark = pytest.mark.gpu
WORST = Worst()
OFFS = (0, 2)
SEED, REPLICA, SCALE = 0x5DEECE66D1234567, 5, 0.75

AXES = {"c": [1, 2, 5, 64], "hw": [(7, 13), (16, 12), (3, 1), (1, 40)], "bt": [1, 3], "mask": ["none", "row", "plane"],
        "chol": [0, 1], "point0": [0, 2 ** 32 - 3]}
CASES = sweep(20260, AXES, 12)
# the limit with a factor (L and the normals fill the 64 KB of LDS), and coil counts at which the four waves of a workgroup hold equal and
# unequal numbers of coil pairs, over a row wider than a workgroup's 64 points
CASES += [dict(c=64, hw=(7, 13), bt=3, mask="row", chol=1, point0=2 ** 32 - 3)]
CASES += [dict(c=c, hw=(3, 70), bt=1, mask="plane", chol=1, point0=0) for c in (16, 17, 32, 33)]


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


def operands(rs, bt, c, h, w, mask, chol):
    """kspace (bt, c, h, w, 2) float32 of unit size, the mask (uint8 (bt, h) / (bt, h, w) / None, some points on and -- where there is
    more than one -- some off) and L (c, c) complex64 or None."""
    k = torch.from_numpy(rs.standard_normal((bt, c, h, w, 2)).astype(np.float32))
    m = None
    if mask != "none":
        m = (rs.uniform(size=(bt, h) if mask == "row" else (bt, h, w)) < 0.5).astype(np.uint8)
        m.flat[0] = 1
        if m.size > 1:
            m.flat[-1] = 0
    low = R.random_chol(rs, c)[0] if chol else None
    return k, m, low


def noise_add(k, kd, out, md, mask_w, ld, shape, seed=SEED, replica=REPLICA, rdev=None, point0=0, scale=SCALE):
    bt, c, h, w = shape
    check(L().cine_noise_add(ptr(kd), out, ptr(md), mask_w, ptr(ld), scale, seed, replica, ptr(rdev), point0, bt, c, h, w, stream()), "cine_noise_add")


def run(dev, k, m, low, shape, offs=OFFS, inplace=False, **kw):
    """The call on fresh guarded operands at every offset of offs (twice each, the same bits): its output on the CPU."""
    mask_w = 1 if m is None or m.ndim == 2 else shape[3]

    def body(call):
        md = None if m is None else call.raw(torch.from_numpy(m))
        ld = None if low is None else call.inp(pairs(low))
        if inplace:
            o = call.out(k.shape, fill=k)
            noise_add(call, o.t, o.ptr(), md, mask_w, ld, shape, **kw)
        else:
            o = call.out(k.shape)
            noise_add(call, call.inp(k), o.ptr(), md, mask_w, ld, shape, **kw)
        return [o.t]
    return at_offsets(dev, offs, body, "cine_noise_add")[0]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_noise_add_vs_reference(dev, case):
    c, (h, w), bt = case["c"], case["hw"], case["bt"]
    rs = np.random.RandomState(hash_case({k: (v if not isinstance(v, tuple) else v[0] * 100 + v[1]) for k, v in case.items()}))
    k, m, low = operands(rs, bt, c, h, w, case["mask"], case["chol"])
    shape = (bt, c, h, w)
    kw = dict(seed=SEED, replica=REPLICA, point0=case["point0"])
    got = run(dev, k, m, low, shape, **kw)
    want, eta = R.noise_add(cplx(k), m, chol=low, scale=SCALE, **kw)
    err, peak = float(np.abs(cplx(got) - want).max()), float(np.abs(eta).max())
    assert peak > 0.5 * SCALE
    WORST.record("cine_noise_add", err, BAR * peak, case_id(case))
    on = torch.from_numpy(np.broadcast_to(R.sampled(m, bt, h, w), (bt, c, h, w)).copy())
    assert same_bits(got[~on], k[~on]), "an unsampled point changed"
    assert bool(((got != k).any(dim=-1) == on).all()), "a sampled point kept its value"
    assert same_bits(run(dev, k, m, low, shape, inplace=True, **kw), got), "in place differs from out of place"


def test_replica_dev_seed_and_replica(dev):
    """replica_dev gives the bits of the same replica by value; replicas r, r + 1 and seeds s, s + 1 differ at every sampled point."""
    bt, c, h, w = 2, 5, 7, 13
    k, m, low = operands(np.random.RandomState(11), bt, c, h, w, "plane", 1)
    shape = (bt, c, h, w)
    base = run(dev, k, m, low, shape, offs=(0,))
    counter = torch.tensor([REPLICA], dtype=torch.int64, device=dev)
    assert same_bits(run(dev, k, m, low, shape, offs=(0,), replica=0, rdev=counter), base)
    counter += 1
    torch.cuda.synchronize()
    nxt = run(dev, k, m, low, shape, offs=(0,), replica=0, rdev=counter)
    assert same_bits(nxt, run(dev, k, m, low, shape, offs=(0,), replica=REPLICA + 1))
    on = torch.from_numpy(np.broadcast_to(R.sampled(m, bt, h, w), (bt, c, h, w)).copy())
    other_seed = run(dev, k, m, low, shape, offs=(0,), seed=SEED + 1)
    for other in (nxt, other_seed):
        assert bool((other != base).any(dim=-1)[on].all()) and same_bits(other[~on], base[~on])
    neg = run(dev, k, m, low, shape, offs=(0,), seed=-3)                        # a negative long is its 64 bits
    want, eta = R.noise_add(cplx(k), m, chol=low, scale=SCALE, seed=-3, replica=REPLICA)
    WORST.record("cine_noise_add", float(np.abs(cplx(neg) - want).max()), BAR * float(np.abs(eta).max()), "seed -3")


@pytest.mark.parametrize("mask,chol", [("row", 1), ("plane", 0), ("none", 1)])
def test_layout_independence(dev, mask, chol):
    """A (bt = 3) call equals three bt = 1 calls with point0 advanced by h w each, bit for bit."""
    bt, c, h, w = 3, 5, 7, 13
    k, m, low = operands(np.random.RandomState(12), bt, c, h, w, mask, chol)
    p0 = 2 ** 32 - 100
    whole = run(dev, k, m, low, (bt, c, h, w), offs=(0,), point0=p0)
    for f in range(bt):
        one = run(dev, k[f:f + 1], None if m is None else m[f:f + 1], low, (1, c, h, w), offs=(0,), point0=p0 + f * h * w)
        assert same_bits(one, whole[f:f + 1]), f"frame {f}"


def test_noise_add_refusals(dev):
    bt, c, h, w = 2, 3, 4, 6
    k, m, low = operands(np.random.RandomState(13), bt, c, h, w, "row", 1)
    call = Call(dev, 0)
    kd, md, ld = call.inp(k), call.raw(torch.from_numpy(m)), call.inp(pairs(low))
    o = call.out(k.shape)
    base = dict(k=ptr(kd), out=o.ptr(), mask=ptr(md), mask_w=1, chol=ptr(ld), replica=0, point0=0, bt=bt, c=c, h=h, w=w)

    def f(**kw):
        a = dict(base, **kw)
        return lambda: L().cine_noise_add(a["k"], a["out"], a["mask"], a["mask_w"], a["chol"], 1.0, 1, a["replica"], None, a["point0"],
                                          a["bt"], a["c"], a["h"], a["w"], stream())
    refused(f(c=65), EUNSUPPORTED, call, "cine_noise_add c = 65")
    assert b"64" in L().cine_last_error()
    refused(f(mask_w=2), EINVAL, call, "cine_noise_add mask_w = 2")
    refused(f(replica=-1), EINVAL, call, "cine_noise_add replica = -1")
    refused(f(k=None), EINVAL, call, "cine_noise_add kspace = NULL")
    refused(f(out=None), EINVAL, call, "cine_noise_add out = NULL")
    refused(f(h=0), EINVAL, call, "cine_noise_add h = 0")
    refused(f(out=o.ptr() + 8, k=o.ptr()), EINVAL, call, "cine_noise_add out overlaps kspace")
    check(f()(), "cine_noise_add")
    call.finish("cine_noise_add")


# ------------------------------------------------------------------ the statistics
def samples(n, pair, seed):
    """8 samples of n map elements (x 2 floats for pairs): image-like values 50 +- 3; elements 1, 5 and 6, where they exist, are the
    same in every sample (zero variance); ref_std is 0 at every fourth element from 2 on."""
    rs = np.random.RandomState(seed)
    shape = (n, 2) if pair else (n,)
    x = (50.0 + 3.0 * rs.standard_normal((8,) + shape)).astype(np.float32)
    x[:, 1:2] = x[0, 1:2]
    x[:, 5:7] = x[0, 5:7]
    ref = np.abs(rs.standard_normal(n)).astype(np.float32) + 0.5
    ref[2::4] = 0.0
    return x, ref


@pytest.mark.parametrize("with_ref", [False, True], ids=["noref", "ref"])
@pytest.mark.parametrize("pair", [0, 1], ids=["real", "pairs"])
@pytest.mark.parametrize("n", [1, 63, 4097])
def test_replica_statistics_vs_float64(dev, n, pair, with_ref):
    x, ref = samples(n, pair, 100 + n + pair)
    nf = x[0].size
    acc = R.Welford()
    mean, m2 = GuardedF64(nf, dev), GuardedF64(nf, dev)                        # NaN: the first sample initialises them
    for i, s in enumerate(x):
        acc.add(s)
        check(L().cine_replica_accum(torch.from_numpy(s).to(dev).data_ptr(), mean.ptr(), m2.ptr(), nf, i + 1, stream()), "cine_replica_accum")
        torch.cuda.synchronize()
    assert mean.intact() and m2.intact()
    for got, want, what in ((mean.t, acc.mean, "mean"), (m2.t, acc.m2, "m2")):
        err = float(np.abs(got.cpu().numpy().reshape(want.shape) - want).max())
        WORST.record(f"cine_replica_accum {what}", err, BAR * float(np.abs(want).max()), (n, pair))
    outs = [Guarded((n,), 0, dev) for _ in range(4)]
    for o in outs:
        o.t.fill_(float("nan"))
    refd = torch.from_numpy(ref).to(dev) if with_ref else None
    accel = 4.0
    check(L().cine_replica_finish(mean.ptr(), m2.ptr(), nf, 8, pair, ptr(refd), accel, outs[0].ptr(), outs[1].ptr(), outs[2].ptr(),
                                  outs[3].ptr() if with_ref else None, stream()), "cine_replica_finish")
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs) and mean.intact() and m2.intact()
    wants = acc.finish(pairs=bool(pair), ref_std=ref if with_ref else None, accel=accel)
    for o, want, what in zip(outs, wants, ("mean", "std", "snr", "g")):
        got = o.t.cpu().numpy().astype(np.float64)
        if want is None:
            assert np.isnan(got).all(), "g_out = NULL, and yet something was written"
            continue
        assert np.isfinite(got).all(), f"{what}: not finite"
        WORST.record(f"cine_replica_finish {what}", float(np.abs(got - want).max()), BAR * float(np.abs(want).max()), (n, pair, with_ref))
    std, snr = outs[1].t.cpu().numpy(), outs[2].t.cpu().numpy()
    flat = [i for i in (1, 5, 6) if i < n]
    assert (std[flat] == 0).all() and (snr[flat] == 0).all(), "zero variance: std and snr are 0, not NaN"
    if with_ref:
        g = outs[3].t.cpu().numpy()
        assert (g[2::4] == 0).all() and (g[flat] == 0).all()
    # every output may be NULL
    check(L().cine_replica_finish(mean.ptr(), m2.ptr(), nf, 8, pair, None, 0.0, None, outs[1].ptr(), None, None, stream()), "cine_replica_finish")
    torch.cuda.synchronize()
    assert same_bits(outs[1].t.cpu(), torch.from_numpy(std))


def test_replica_statistics_refusals(dev):
    call = Call(dev, 0)
    x = call.inp(torch.ones(10))
    o = call.out((10,))
    mean, m2 = GuardedF64(10, dev), GuardedF64(10, dev)
    refused(lambda: L().cine_replica_accum(ptr(x), mean.ptr(), m2.ptr(), 10, 0, stream()), EINVAL, call, "cine_replica_accum k = 0")
    refused(lambda: L().cine_replica_accum(None, mean.ptr(), m2.ptr(), 10, 1, stream()), EINVAL, call, "cine_replica_accum x = NULL")
    refused(lambda: L().cine_replica_finish(mean.ptr(), m2.ptr(), 10, 1, 0, None, 0.0, o.ptr(), None, None, None, stream()), EINVAL, call,
            "cine_replica_finish k = 1")
    refused(lambda: L().cine_replica_finish(mean.ptr(), m2.ptr(), 10, 2, 0, None, 4.0, None, None, None, o.ptr(), stream()), EINVAL, call,
            "cine_replica_finish g_out without ref_std")
    assert torch.isnan(mean.t).all() and torch.isnan(m2.t).all() and mean.intact() and m2.intact()
