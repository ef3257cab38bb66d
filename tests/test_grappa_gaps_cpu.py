"""GRAPPA on unevenly spaced rows without a GPU: ``cine_hip.grappa.plan_gaps`` against hand-written cases of the rule of
include/cine_hip.h, the argument errors of the ``accel=None`` path that are raised before any device call, and the float64 reference
(tests/grappa_gaps_reference.py) -- on lattices against tests/grappa_reference.py, on the reference's equispaced masks, and on the
synthetic phantom.  The GPU tests compare against that reference."""
import numpy as np
import pytest
import torch

import grappa_gaps_reference as gref
import grappa_reference as ref
from cine_hip import grappa as G


def rows_mask(h, rows):
    m = np.zeros((1, h), np.uint8)
    m[0, list(rows)] = 1
    return m


def plan_one(h, rows, **kw):
    gaps, sizes, unfilled = G.plan_gaps(rows_mask(h, rows), **kw)
    assert unfilled.dtype == np.int32 and unfilled.shape == (1,)
    want = gref.plan(rows_mask(h, rows), kw.get("max_gap", 8), kw.get("allowed"))
    assert (gaps, sizes, unfilled.tolist()) == (want[0], want[1], want[2].tolist())          # the twin and the reference agree
    return gaps[0], sizes, int(unfilled[0])


# ------------------------------------------------------------------ the plan, case by case
@pytest.mark.parametrize("R", [2, 3, 4, 8])
def test_a_pure_lattice_has_every_gap_of_its_step(R):
    t, h = 2 * R + 1, 37
    mask = G.lattice_mask(t, h, R)
    off = G.plan_lattice(mask, R)[0]
    gaps, sizes, unfilled = G.plan_gaps(mask)
    assert sizes == (R,) and unfilled.shape == (1, t) and not unfilled.any()
    for f in range(t):
        o = int(off[f])
        want = [(o + g * R, R) for g in range(-1, (h - 1) // R + 1)]                          # the lattice gaps of cine_grappa_apply ...
        want = [(lo, R) for lo, _ in want if any(0 <= lo + m < h for m in range(1, R))]       # ... that hold a row of the frame
        assert gaps[0][f] == want, (R, f)
    assert G.plan_gaps(mask.numpy().reshape(t, h))[0] == gaps[0]                              # the (t, h) form


def test_an_acs_block_splits_the_gaps_around_it():
    #            0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16
    # acquired   x           x        x  x  x  x        x           x
    gaps, sizes, unfilled = plan_one(17, [0, 4, 7, 8, 9, 10, 12, 16])
    assert gaps == [(0, 4), (4, 3), (10, 2), (12, 4)] and sizes == (2, 3, 4) and unfilled == 0


def test_ends_longer_and_shorter_than_the_neighbouring_spacing():
    # leading end of 2 rows beside a spacing of 5: G = 5, the lower source row -3 lies outside; trailing end of 6 rows beside a spacing
    # of 3: G = 7
    gaps, sizes, unfilled = plan_one(16, [2, 7, 9])
    assert gaps == [(-3, 5), (2, 5), (7, 2), (9, 7)] and sizes == (2, 5, 7) and unfilled == 0
    # a neighbouring spacing of 1 does not count: G = e + 1
    gaps, _, _ = plan_one(10, [3, 4, 6, 7])
    assert gaps == [(-1, 4), (4, 2), (7, 3)]


def test_a_single_acquired_row():
    gaps, sizes, unfilled = plan_one(9, [3])
    assert gaps == [(-1, 4), (3, 6)] and sizes == (4, 6) and unfilled == 0
    assert plan_one(9, [0]) == ([], (), 8)                                                    # an end of 8 rows: G = 9, out of reach
    assert plan_one(1, [0]) == ([], (), 0)


def test_an_empty_frame_and_a_full_one():
    assert plan_one(11, []) == ([], (), 11)
    assert plan_one(11, range(11)) == ([], (), 0)
    gaps, sizes, unfilled = G.plan_gaps(np.array([[0, 0, 0, 0, 0], [1, 0, 1, 0, 1]], np.uint8))
    assert gaps == [[], [(0, 2), (2, 2)]] and sizes == (2,) and unfilled.tolist() == [5, 0]


def test_a_gap_of_nine_stays_unfilled():
    gaps, sizes, unfilled = plan_one(20, [1, 4, 13, 16])
    assert gaps == [(-2, 3), (1, 3), (13, 3), (16, 4)] and sizes == (3, 4) and unfilled == 8
    assert plan_one(20, [1, 4, 12, 16])[2] == 0                                               # eight is within reach
    gaps, _, unfilled = plan_one(20, [1, 4, 12, 16], max_gap=5)                               # ... unless max_gap says otherwise
    assert gaps == [(-2, 3), (1, 3), (12, 4), (16, 4)] and unfilled == 7


def test_a_size_that_is_not_allowed_stays_unfilled():
    gaps, sizes, unfilled = plan_one(17, [0, 4, 7, 8, 9, 10, 12, 16], allowed=[2, 4])
    assert gaps == [(0, 4), (10, 2), (12, 4)] and sizes == (2, 4) and unfilled == 2
    gaps, sizes, unfilled = plan_one(16, [2, 7, 9], allowed=[2, 7])                           # the leading end goes with its step
    assert gaps == [(7, 2), (9, 7)] and unfilled == 2 + 4


def test_plan_gaps_arguments():
    m = rows_mask(8, [0, 3])
    for bad in (1, 9, 2.5):
        with pytest.raises(ValueError, match="max_gap"):
            G.plan_gaps(m, max_gap=bad)
    for bad in ([1, 2], [2, 9], [2, 2.5], []):
        with pytest.raises(ValueError, match="gaps"):
            G.plan_gaps(m, allowed=bad)
    with pytest.raises(ValueError, match="mask"):
        G.plan_gaps(np.zeros((2, 3, 4), np.uint8))


def test_random_masks_against_the_reference_plan():
    rs = np.random.RandomState(7)
    for it in range(200):
        h = int(rs.randint(1, 45))
        m = (rs.rand(3, h) < rs.choice([0.15, 0.4, 0.7])).astype(np.uint8)
        max_gap = int(rs.choice([8, 5]))
        allowed = None if it % 2 else [2, 3, 5, 8]
        got, want = G.plan_gaps(m, max_gap, allowed), gref.plan(m, max_gap, allowed)
        assert got[0] == want[0] and got[1] == want[1] and got[2].tolist() == want[2].tolist(), m
        assert all(len(g) <= h // 2 + 1 for g in got[0])                                      # cine_grappa_gaps_cap


# ------------------------------------------------------------------ errors of the accel=None path that need no device
def test_settings_of_the_gap_path():
    k, m = torch.zeros(1, 2, 3, 16, 8, 2), torch.ones(1, 2, 1, 16, 1, 1)
    with pytest.raises(ValueError, match="ky = 2"):
        G.grappa(k, m, kernel=(4, 5))
    with pytest.raises(ValueError, match="ky = 2"):
        G.Grappa(accel=None, kernel=(4, 5))
    with pytest.raises(ValueError, match="max_gap"):
        G.grappa(k, m, max_gap=9)
    with pytest.raises(ValueError, match="gaps"):
        G.grappa(k, m, gaps=(2, 9))
    with pytest.raises(ValueError, match="max_unfilled"):
        G.grappa(k, m, max_unfilled=1.5)
    with pytest.raises(ValueError, match="explicit"):
        G.Grappa(accel=None, gaps="auto")
    mod = G.Grappa(accel=None, gaps=(5, 2, 3), kernel=(2, 3))
    assert mod.accel is None and mod.gaps == (2, 3, 5) and mod.kernel == (2, 3) and mod.max_gap == 8
    assert G.Grappa().gaps == (2, 3, 4, 5, 6)
    assert G.Grappa(accel=3).accel == 3                                                       # the lattice module is what it was


def test_host_checks_of_the_gap_path():
    """Raised from the host copy of the mask, before the first device call (the tensors are on the CPU: a call that got further would
    raise CineHipError)."""
    t, c, h, w = 2, 3, 24, 8
    k = torch.zeros(1, t, c, h, w, 2)
    rows = np.zeros((t, h), np.uint8)
    rows[:, [0, 3, 6, 8, 9, 10, 11, 12, 13, 14, 17, 20, 23]] = 1
    rows[1, 3] = 0                                                                            # frame 1: a gap of six
    m = torch.from_numpy(rows.reshape(1, t, 1, h, 1, 1))
    with pytest.raises(ValueError, match=r"row 1 of frame 1"):
        G.grappa(k, m, gaps=(2, 3), acs=(8, 15))
    with pytest.raises(ValueError, match="unfilled"):
        G.grappa(k, m, max_gap=5, acs=(8, 15))
    with pytest.raises(ValueError, match="calibration block of 6 rows"):                      # "auto" takes {2, 3, 6}: seven rows needed
        G.grappa(k, m, acs=(8, 14))
    from cine_hip._lib import CineHipError
    with pytest.raises(CineHipError, match="GPU tensors"):                                    # everything on the host is in order
        G.grappa(k, m, gaps=(2, 3), max_unfilled=0.5, acs=(8, 15))


# ------------------------------------------------------------------ the float64 reference
@pytest.mark.parametrize("R,kx", [(2, 3), (3, 5), (4, 5), (8, 3)])
def test_reference_equals_the_lattice_reference_on_lattices(R, kx):
    t, c, h, w = R + 1, 4, 37, 14
    k, mask, mk = ref.phantom_slice(t, c, h, w, R)
    want, info, _ = ref.grappa(mk, mask, R, (2, kx), 1e-4, calib="tgrappa", calib_rows=h)
    got, ginfo, sizes, unfilled = gref.grappa(mk, mask, kx, 1e-4, calib="tgrappa", calib_rows=h)
    assert sizes == (R,) and not unfilled.any() and (ginfo[R] == info).all()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("h", [200, 64, 40])
def test_equispaced_masks_are_within_reach(h):
    """EquispacedMaskFunc([0.08], [4]): every missing row lies in a gap of a step within {2 .. 6}."""
    seen = set()
    for seed in range(50):
        mask, (lo, hi) = gref.equispaced_mask(1, h, 0.08, 4, seed)
        gaps, sizes, unfilled = G.plan_gaps(mask)
        assert unfilled.tolist() == [0] and set(sizes) <= {2, 3, 4, 5, 6}, (seed, sizes)
        assert gref.plan(mask)[0] == gaps
        filled = np.zeros(h, bool)
        for glo, step in gaps[0]:
            filled[max(glo + 1, 0):min(glo + step, h)] = True
        assert (filled == (mask[0] == 0)).all()                                               # the gaps cover the missing rows, and only those
        seen |= set(sizes)
    assert {5, 6} <= seen


# t, c, h, w, center_fraction, acceleration, seed, kx, lam: a centre block of 16 rows, steps {2, 4, 5, 6}
PHANTOM = (2, 8, 200, 40, 0.08, 4, 1, 5, 0.3)
PHANTOM_NRMSE = 0.1177


def test_reference_beats_zero_filling_on_the_phantom():
    """The noisy phantom (noise 0.01) under EquispacedMaskFunc([0.08], [4]), calibrated on its centre block (rows 92 .. 107).
    Measured: NRMSE 0.1177 against 0.1318 zero-filled, at lam = 0.3.  The gain is small and needs that much regularisation: the
    phantom's eight smooth Gaussian coils carry a lattice step of 4 (0.199 against 0.727 in test_grappa_cpu.py) but hardly the steps 5
    and 6 these masks are made of, and at lam = 1e-4 the fit amplifies the noise (NRMSE 0.54).  The bar is the measured value with a
    1.25x margin for the seed-to-seed spread of the phantom; it is not tuned to the device path."""
    t, c, h, w, frac, acc, seed, kx, lam = PHANTOM
    k, mask, mk, acs = gref.phantom_slice(t, c, h, w, frac, acc, seed)
    assert acs == (92, 108) and acs[1] - acs[0] >= 7
    filled, info, sizes, unfilled = gref.grappa(mk, mask, kx, lam, calib="acs", acs=acs)
    assert sizes == (2, 4, 5, 6) and not unfilled.any()
    full = ref.rss(k)
    e_grappa, e_zero = ref.nrmse(ref.rss(filled), full), ref.nrmse(ref.rss(mk), full)
    print(f"NRMSE GRAPPA {e_grappa:.4f}, zero-filled {e_zero:.4f}, fit per step { {s: round(float(i[2]), 3) for s, i in info.items()} }")
    assert e_grappa < e_zero
    assert e_grappa <= 1.25 * PHANTOM_NRMSE
    acquired = mask.astype(bool)
    assert (filled[acquired.nonzero()[0], :, acquired.nonzero()[1]] == mk[acquired.nonzero()[0], :, acquired.nonzero()[1]]).all()
    assert (np.abs(filled).sum(axis=(1, 3))[~acquired] > 0).all()                             # every missing row is filled
