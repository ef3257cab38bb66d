"""cine_grappa_gaps and cine_grappa_apply_gaps through ctypes against the rule of include/cine_hip.h: the gap table against
cine_hip.grappa.plan_gaps, exactly; the application against float64 (tests/grappa_gaps_reference.py) within the bar of the lattice
apply test,

apply    each output component within (2 ns + 1) 2^-24 sum |w| |x| of float64: the bound of a 2 ns-term fp32 chain,

with NaN in every input row that is no source, every row that is no target bit for bit, in place against out of place, two calls
against each other, and on pure lattices bit for bit against cine_grappa_apply with the same weights.  The shapes are the smallest
that cross the boundaries of the kernel: kx itself and the 64-point workgroup seam in w, the 64-value weight chunk in ns (70 at c = 5,
kx = 7; 448 at c = 32), one 16-column tile and a four-tile group in (G - 1) c (105 at G = 8, c = 15), the 256-row chunk of the table's
prefix sum in h."""
import ctypes

import numpy as np
import pytest
import torch

import grappa_gaps_reference as gref
import grappa_reference as ref
from cine_hip import grappa as G
from kernel_sweep import (EINVAL, EUNSUPPORTED, Call, GuardedInt, L, at_offsets, case_id, hash_case, refused, same_bits, stream, sweep)

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 5, 8)
# frame 0 of every case, cut at h: a leading end of two rows (step 3, its lower source row outside the frame), the steps 2, 3, 5, 8 next
# to each other (neighbours share a source row), a block of four rows, a gap of nine (unfilled), a step 3 and a trailing end
ZOO = [2, 4, 7, 12, 20, 21, 22, 23, 32, 35]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def pairs(z):
    z = np.asarray(z)
    return torch.from_numpy(np.stack((z.real, z.imag), -1).astype(np.float32))


def cplx(t):
    a = t.detach().cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def zoo_mask(t, h, seed):
    """(t, h): frame 0 the ZOO; with three frames, frame 1 is empty and frame 2 walks from a random first row in random steps of
    1, 2, 3, 5, 8 and 9 (its ends may ask for a step without weights)."""
    m = np.zeros((t, h), np.uint8)
    m[0, [y for y in ZOO if y < h]] = 1
    if t == 3:
        rs = np.random.RandomState(seed)
        y = int(rs.randint(0, 4))
        while y < h:
            m[2, y] = 1
            y += int(rs.choice([1, 2, 3, 5, 8, 9]))
    return m


def woff_of(sizes, ns, c):
    off, row = [-1] * 9, 0
    for s in sizes:
        off[s] = row * ns * c
        row += s - 1
    return (ctypes.c_int * 9)(*off), row


def table_of(gaps, t, cap, garbage=True):
    """The (t, cap, 2) table and the counts of the host plan; entries from count on hold what must never be used."""
    tab = np.zeros((t, cap, 2), np.int32)
    if garbage:
        tab[..., 0], tab[..., 1] = -100000, 77
    count = np.zeros(t, np.int32)
    for f, g in enumerate(gaps):
        count[f] = len(g)
        for i, (lo, step) in enumerate(g):
            tab[f, i] = (lo, step)
    return tab, count


# ================================================================== the gap table
def run_gaps(dev, mask, max_gap, allowed):
    t, h = mask.shape
    cap = L().cine_grappa_gaps_cap(h)
    assert cap == h // 2 + 1
    m = torch.from_numpy(mask).to(dev)
    tab, count, unfilled = GuardedInt(t * cap * 2, dev, fill=-7), GuardedInt(t, dev, fill=-7), GuardedInt(t, dev, fill=-7)
    bits = sum(1 << s for s in allowed)
    assert L().cine_grappa_gaps(m.data_ptr(), tab.ptr(), count.ptr(), unfilled.ptr(), t, h, max_gap, bits, stream()) == 0, L().cine_last_error()
    torch.cuda.synchronize()
    assert tab.intact() and count.intact() and unfilled.intact() and torch.equal(m.cpu(), torch.from_numpy(mask))
    return tab.t.cpu().numpy().reshape(t, cap, 2), count.t.cpu().numpy(), unfilled.t.cpu().numpy()


def check_gaps(dev, mask, max_gap=8, allowed=tuple(range(2, 9))):
    t, h = mask.shape
    gaps, _, want_unfilled = G.plan_gaps(mask, max_gap, [s for s in allowed if s <= 8])
    tab, count, unfilled = run_gaps(dev, mask, max_gap, allowed)
    want_tab, want_count = table_of(gaps, t, h // 2 + 1, garbage=False)
    assert count.tolist() == want_count.tolist() and unfilled.tolist() == want_unfilled.tolist(), (mask, gaps)
    assert (tab == want_tab).all(), (mask, tab, want_tab)
    again = run_gaps(dev, mask, max_gap, allowed)
    assert (again[0] == tab).all() and (again[1] == count).all() and (again[2] == unfilled).all()


@pytest.mark.parametrize("h", [1, 2, 12, 13, 37, 40, 255, 256, 257, 600])
def test_gap_table_equals_the_plan(dev, h):
    rs = np.random.RandomState(h)
    frames = [zoo_mask(3, h, h), np.zeros((1, h), np.uint8), np.ones((1, h), np.uint8)]
    for p in (0.15, 0.35, 0.6):
        frames.append((rs.rand(2, h) < p).astype(np.uint8))
    one = np.zeros((2, h), np.uint8)
    one[0, h // 3] = 1                                                     # a single acquired row
    one[1, 0::2] = 1                                                       # every other row: the most gaps a frame can have
    frames.append(one)
    mask = np.concatenate(frames)
    check_gaps(dev, mask)
    check_gaps(dev, mask, max_gap=5)
    check_gaps(dev, mask, allowed=SIZES)
    tab, count, unfilled = run_gaps(dev, mask, 8, ())                      # nothing allowed: every missing row is unfilled
    assert not tab.any() and not count.any() and unfilled.tolist() == (mask == 0).sum(1).tolist()


@pytest.mark.parametrize("R", [2, 3, 4, 8])
def test_gap_table_of_a_lattice(dev, R):
    mask = ref.lattice_mask(R + 1, 37, R)
    tab, count, unfilled = run_gaps(dev, mask, 8, (R,))
    assert not unfilled.any()
    for f in range(R + 1):
        assert (tab[f, :count[f], 1] == R).all() and (np.diff(tab[f, :count[f], 0]) == R).all()
    check_gaps(dev, mask)


def test_gaps_refusals(dev):
    t, h = 3, 12
    m = torch.from_numpy(zoo_mask(t, h, 0)).to(dev)
    cap = L().cine_grappa_gaps_cap(h)
    k = Call(dev, 0)
    tab, count, unfilled = GuardedInt(t * cap * 2, dev), GuardedInt(t, dev), GuardedInt(t, dev)
    k.outs += [tab, count, unfilled]
    good = [m.data_ptr(), tab.ptr(), count.ptr(), unfilled.ptr(), t, h, 8, 0x1FC]
    for i in range(4):
        args = good[:i] + [None] + good[i + 1:]
        refused(lambda: L().cine_grappa_gaps(*args, stream()), EINVAL, k, "cine_grappa_gaps null pointer")
    for bad in ([good[0], good[1], good[2], good[2]] + good[4:], [good[0], good[1], good[1], good[3]] + good[4:], good[:4] + [0, h, 8, 0x1FC],
                good[:4] + [t, 0, 8, 0x1FC], good[:6] + [1, 0x1FC], good[:6] + [9, 0x1FC], good[:6] + [8, 0x1FE], good[:6] + [8, 0x3FC],
                [good[0], tab.ptr() + 2] + good[2:], [good[0], good[1], count.ptr() + 1] + good[3:]):
        refused(lambda: L().cine_grappa_gaps(*bad, stream()), EINVAL, k, f"cine_grappa_gaps {bad[4:]}")
    refused(lambda: L().cine_grappa_gaps(*(good[:5] + [(1 << 20) + 1, 8, 0x1FC]), stream()), EUNSUPPORTED, k, "cine_grappa_gaps too many rows")
    assert L().cine_grappa_gaps_cap(0) == 0 and L().cine_grappa_gaps_cap(-3) == 0
    assert L().cine_grappa_gaps(*good, stream()) == 0
    k.finish("cine_grappa_gaps after the refusals")


# ================================================================== apply
def apply_cases():
    axes = {"c": [1, 2, 5, 15, 32], "kx": [3, 5, 7], "t": [1, 3], "h": [12, 13, 24, 33, 40], "w": [7, 9, 64, 70, 130]}
    out = sweep(20261, axes, 20)
    out += [{"c": 5, "kx": 7, "t": 3, "h": 24, "w": 70},                   # ns = 70: one value past the 64-value weight chunk
            {"c": 32, "kx": 7, "t": 1, "h": 24, "w": 9},                   # ns = 448, (G - 1) c = 224: four groups of four tiles at step 8
            {"c": 15, "kx": 5, "t": 3, "h": 40, "w": 130},                 # (G - 1) c = 105 at step 8: seven tiles, two groups
            {"c": 2, "kx": 3, "t": 3, "h": 40, "w": 64}]                   # (G - 1) c = 14 at step 8: within one tile
    return out


def apply_inputs(case):
    """(k-space with NaN in every row that is no source of a listed gap, mask, gaps per frame, weights per step)."""
    c, kx, t, h, w = (case[x] for x in ("c", "kx", "t", "h", "w"))
    seed = hash_case(case)
    rs = np.random.RandomState(seed)
    mask = zoo_mask(t, h, seed)
    gaps, _, _ = G.plan_gaps(mask, 8, SIZES)
    source = np.zeros((t, h), bool)
    for f in range(t):
        for lo, s in gaps[f]:
            for r in (lo, lo + s):
                if 0 <= r < h:
                    source[f, r] = True
    assert (source <= mask.astype(bool)).all()
    k = (rs.standard_normal((t, c, h, w)) + 1j * rs.standard_normal((t, c, h, w))).astype(np.complex64)
    k = np.where(source[:, None, :, None], k, np.complex64(complex(np.nan, np.nan)))
    ns = 2 * kx * c
    W = {s: ((rs.standard_normal((s - 1, ns, c)) + 1j * rs.standard_normal((s - 1, ns, c))) / np.sqrt(ns)).astype(np.complex64) for s in SIZES}
    return k, mask, gaps, W


@pytest.mark.parametrize("case", apply_cases(), ids=case_id)
def test_apply_gaps_against_float64(dev, case):
    c, kx, t, h, w = (case[x] for x in ("c", "kx", "t", "h", "w"))
    ksp, mask, gaps, W = apply_inputs(case)
    if h >= 33:
        assert {s for _, s in gaps[0]} == set(SIZES) and gaps[0][0] == (-1, 3)             # every step, the leading end among them
    ns = 2 * kx * c
    cap = h // 2 + 1
    woff, rows = woff_of(SIZES, ns, c)
    tab, count = table_of(gaps, t, cap)
    want, mag = gref.apply(np.nan_to_num(ksp), W, mask, gaps, kx, bound=True)
    x_in, w_in = pairs(ksp), pairs(np.concatenate([W[s] for s in SIZES]))
    assert tuple(w_in.shape) == (rows, ns, c, 2)
    d_mask, d_tab, d_count = torch.from_numpy(mask), torch.from_numpy(tab), torch.from_numpy(count)

    def out_of_place(k):
        d_k, d_w = k.inp_among_nan(x_in), k.inp(w_in)
        out = k.out((t, c, h, w, 2))
        code = L().cine_grappa_apply_gaps(d_k.data_ptr(), d_w.data_ptr(), woff, k.raw(d_mask).data_ptr(), k.raw(d_tab).data_ptr(),
                                          k.raw(d_count).data_ptr(), out.ptr(), t, c, h, w, cap, kx, stream())
        assert code == 0, L().cine_last_error()
        return [out.t]

    def in_place(k):
        d_w = k.inp(w_in)
        buf = k.out((t, c, h, w, 2), fill=x_in)
        code = L().cine_grappa_apply_gaps(buf.ptr(), d_w.data_ptr(), woff, k.raw(d_mask).data_ptr(), k.raw(d_tab).data_ptr(),
                                          k.raw(d_count).data_ptr(), buf.ptr(), t, c, h, w, cap, kx, stream())
        assert code == 0, L().cine_last_error()
        return [buf.t]

    got = at_offsets(dev, (0, 2), out_of_place, "cine_grappa_apply_gaps")[0]        # twice at both placements, guards intact, the same bits
    same = at_offsets(dev, (0, 2), in_place, "cine_grappa_apply_gaps in place")[0]
    assert same_bits(got, same), "in place gives other bits than out of place"

    target = np.zeros((t, h), bool)
    for f in range(t):
        for lo, s in gaps[f]:
            target[f, max(lo + 1, 0):min(lo + s, h)] = True
    assert not (target & mask.astype(bool)).any()
    if t == 3:
        assert not target[1].any()                                                    # the empty frame
    if h >= 33:
        assert not target[0, 24:32].any()                                             # the gap of nine
    kept = torch.from_numpy(~target)
    sel = kept[:, None, :, None, None].expand(t, c, h, w, 2)
    assert torch.equal(got.view(torch.int32)[sel], x_in.view(torch.int32)[sel]), "a row that is not a target changed"
    Gk = cplx(got)
    tg = np.broadcast_to(target[:, None, :, None], Gk.shape)
    assert not np.isnan(Gk[tg].real).any() and not np.isnan(Gk[tg].imag).any(), "a target was not written, or a row that is no source was read"
    bar = (2 * ns + 1) * 2.0 ** -24
    e_re, e_im = np.abs(Gk.real - want.real)[tg], np.abs(Gk.imag - want.imag)[tg]
    b_re, b_im = bar * mag.real[tg], bar * mag.imag[tg]
    worst = max(float((e_re / np.maximum(b_re, 1e-300)).max()), float((e_im / np.maximum(b_im, 1e-300)).max()))
    print(f"{case_id(case)}: {int(target.sum())} target rows, worst error {worst:.3f} of its bound")
    assert (e_re <= b_re).all() and (e_im <= b_im).all()


@pytest.mark.parametrize("R,c,kx,w", [(2, 5, 3, 70), (3, 15, 5, 64), (4, 15, 5, 130), (8, 15, 7, 9), (8, 2, 3, 70), (4, 32, 5, 7)])
def test_apply_gaps_gives_the_bits_of_the_lattice_kernel(dev, R, c, kx, w):
    """A pure lattice: every gap, both ends included, has the step R, and the gap kernel runs the chain of cine_grappa_apply."""
    t, h = R + 1, 37
    rs = np.random.RandomState(100 * R + c)
    mask = ref.lattice_mask(t, h, R)
    off, _ = ref.offsets(mask, R)
    gaps, sizes, unfilled = G.plan_gaps(mask)
    assert sizes == (R,) and not unfilled.any()
    ns, cap = 2 * kx * c, h // 2 + 1
    ksp = (rs.standard_normal((t, c, h, w)) + 1j * rs.standard_normal((t, c, h, w))).astype(np.complex64) * mask[:, None, :, None]
    W = ((rs.standard_normal((R - 1, ns, c)) + 1j * rs.standard_normal((R - 1, ns, c))) / np.sqrt(ns)).astype(np.complex64)
    filler = (rs.standard_normal((3, ns, c)) + 1j * rs.standard_normal((3, ns, c))).astype(np.complex64)
    woff = [-1] * 9
    woff[R] = 3 * ns * c                                                               # the block of step R behind three rows of another
    woff = (ctypes.c_int * 9)(*woff)
    tab, count = table_of(gaps, t, cap)
    k = Call(dev, 0)
    d_k, d_w, d_wg = k.inp(pairs(ksp)), k.inp(pairs(W)), k.inp(pairs(np.concatenate([filler, W])))
    d_mask = k.raw(torch.from_numpy(mask))
    lattice, gapped = k.out((t, c, h, w, 2)), k.out((t, c, h, w, 2))
    code = L().cine_grappa_apply(d_k.data_ptr(), d_w.data_ptr(), d_mask.data_ptr(), k.raw(torch.from_numpy(off.astype(np.int32))).data_ptr(),
                                 lattice.ptr(), t, c, h, w, R, 2, kx, stream())
    assert code == 0, L().cine_last_error()
    code = L().cine_grappa_apply_gaps(d_k.data_ptr(), d_wg.data_ptr(), woff, d_mask.data_ptr(), k.raw(torch.from_numpy(tab)).data_ptr(),
                                      k.raw(torch.from_numpy(count)).data_ptr(), gapped.ptr(), t, c, h, w, cap, kx, stream())
    assert code == 0, L().cine_last_error()
    k.finish("cine_grappa_apply_gaps beside cine_grappa_apply")
    assert bool(torch.isfinite(lattice.t).all()) and float(lattice.t.abs().max()) > 0
    assert same_bits(gapped.t, lattice.t)


def test_apply_gaps_refusals(dev):
    c, kx, t, h, w = 3, 5, 2, 13, 9
    ns, cap = 2 * kx * c, h // 2 + 1
    lib = L()
    k = Call(dev, 0)
    mask = zoo_mask(t, h, 0)
    mask[1] = mask[0]
    gaps, _, _ = G.plan_gaps(mask, 8, SIZES)
    tab, count = table_of(gaps, t, cap)
    woff, rows = woff_of(SIZES, ns, c)
    d_k = k.inp(torch.ones(2 * t, c, h, w, 2))[:t]                                     # room behind the k-space for the overlap cases
    d_w = k.inp(torch.ones(rows, ns, c, 2))
    d_mask, d_tab, d_count = k.raw(torch.from_numpy(mask)), k.raw(torch.from_numpy(tab)), k.raw(torch.from_numpy(count))
    out = k.out((t, c, h, w, 2))
    names = ["in", "weights", "woff", "mask", "gaps", "count", "out", "t", "c", "h", "w", "cap", "kx"]
    good = [d_k.data_ptr(), d_w.data_ptr(), woff, d_mask.data_ptr(), d_tab.data_ptr(), d_count.data_ptr(), out.ptr(), t, c, h, w, cap, kx]

    def bad(want, what, **kw):
        args = [kw.get(nm, v) for nm, v in zip(names, good)]
        refused(lambda: lib.cine_grappa_apply_gaps(*args, stream()), want, k, f"cine_grappa_apply_gaps {what}")

    for nm in names[:7]:
        bad(EINVAL, f"null {nm}", **{nm: None})
    bad(EINVAL, "t = 0", t=0)
    bad(EINVAL, "w = 0", w=0)
    bad(EINVAL, "cap = 0", cap=0)
    bad(EUNSUPPORTED, "33 coils", c=33)
    bad(EINVAL, "kx = 4", kx=4)
    bad(EINVAL, "kx = 2 (what a caller with ky = 4 in mind might pass: there is no ky)", kx=2)
    bad(EINVAL, "no step with weights", woff=(ctypes.c_int * 9)(*([-1] * 9)))
    bad(EINVAL, "an offset below -1", woff=(ctypes.c_int * 9)(-1, -1, 0, -2, -1, -1, -1, -1, -1))
    bad(EINVAL, "in off its alignment", **{"in": d_k.data_ptr() + 4})
    bad(EINVAL, "out off its alignment", out=out.ptr() + 4)
    bad(EINVAL, "weights off their alignment", weights=d_w.data_ptr() + 4)
    bad(EINVAL, "gaps off their alignment", gaps=d_tab.data_ptr() + 2)
    bad(EINVAL, "count off its alignment", count=d_count.data_ptr() + 1)
    bad(EINVAL, "out overlaps in", out=d_k.data_ptr() + 8)
    bad(EINVAL, "out ends inside in", out=d_k.data_ptr() + 8 * c * h * w)
    bad(EUNSUPPORTED, "too many frames", t=65536)
    bad(EUNSUPPORTED, "too many table entries", cap=65536)
    # the limit ns + (G_max - 1) c <= 1152: 32 coils with a 2 x 7 kernel hold 896 + 7 x 32 = 1120; every shape the entry admits is within it,
    # as for cine_grappa_apply, so the refusal that is left is the coil count above
    assert lib.cine_grappa_apply_gaps(*good, stream()) == 0                            # and the call works after every refusal
    k.finish("cine_grappa_apply_gaps after the refusals")
    with pytest.raises(ValueError, match="ky = 2"):                                    # ky = 4 has no entry to reach: the binding refuses it
        G.grappa_apply_gaps(d_k, d_w, SIZES, d_mask, d_tab, d_count, kernel=(4, kx))
    with pytest.raises(ValueError, match="ky = 2"):
        G.grappa_weights_gaps(torch.ones(c, 12, w, 2, device=dev), SIZES, kernel=(4, kx))
