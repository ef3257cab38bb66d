"""cine_hip.gating.plan_gating without a GPU: both modes against a brute-force float64 restatement of the definition written here
(dense (rows, n_lines) matrices, no CSR, no sorting by numpy), the counts of what is dropped, the validator of GatingPlan, and the
readouts_from_raw round trip.

Schedules: 30 - 200 readouts, nx in {1, 7, 24}, n_frames in {1, 2, 5}; triggers on a coarse grid of 2.5 ms in beats of 1000 ms, so that
identical phases (duplicate nodes of the linear mode), cells with several readouts and a node exactly at a frame centre all occur; a few
lines are left without any readout and one line gets exactly one (the single-node rule of the linear mode)."""
import numpy as np
import pytest

from cine_hip import gating as G
from cine_hip._lib import CineHipError

RR = 1000.0
SCHEDULES = [(30, 1, 1), (30, 1, 5), (60, 7, 1), (60, 7, 2), (100, 7, 5), (120, 24, 2), (200, 24, 5), (45, 24, 5)]


def schedule(n, nx, n_frames, seed):
    """(pe_index, trigger_ms, rr_ms) of n readouts.  Line nx - 1 is never acquired (nx > 1), line nx - 2 exactly once (nx >= 7); phases
    sit on a grid of 400 values, so duplicates are common; readout 0 and 1 share line and phase when they are on the same line."""
    rs = np.random.RandomState(seed)
    hi = nx if nx == 1 else nx - 1 if nx < 7 else nx - 2
    pe = rs.randint(0, hi, size=n)
    trig = rs.randint(0, 400, size=n) * 2.5
    if nx >= 7:
        pe[n // 2] = nx - 2
    pe[1], trig[1] = pe[0], trig[0]                                           # a certain duplicate phase
    trig[2] = (0.5 / n_frames) * RR                                           # a node exactly at the first frame's centre
    return pe.astype(np.int64), trig.astype(np.float64), np.full(n, RR)


def dense_nearest(pe, phi, ok, n_frames, nx):
    a = np.zeros((n_frames * nx, pe.shape[0]))
    for f in range(n_frames):
        for x in range(nx):
            mem = [i for i in range(pe.shape[0]) if ok[i] and pe[i] == x and int(np.floor(phi[i] * n_frames)) == f]
            for i in mem:
                a[f * nx + x, i] = 1.0 / len(mem)
    return a


def dense_linear(pe, phi, ok, n_frames, nx):
    a = np.zeros((n_frames * nx, pe.shape[0]))
    for x in range(nx):
        mem = [i for i in range(pe.shape[0]) if ok[i] and pe[i] == x]
        nodes = sorted({phi[i] for i in mem})
        share = {p: [i for i in mem if phi[i] == p] for p in nodes}
        for f in range(n_frames):
            th = (f + 0.5) / n_frames
            if not nodes:
                continue
            if len(nodes) == 1:
                pairs = [(nodes[0], 1.0)]
            else:
                # the cyclic list: the last node one period earlier, the nodes, the first one period later
                cyc = [(nodes[-1] - 1.0, nodes[-1])] + [(p, p) for p in nodes] + [(nodes[0] + 1.0, nodes[0])]
                k = max(j for j in range(len(cyc)) if cyc[j][0] <= th)
                (pa, na), (pb, nb) = cyc[k], cyc[k + 1]
                assert pa <= th < pb
                wa = (pb - th) / (pb - pa)
                pairs = [(na, wa), (nb, 1.0 - wa)]
            for node, w in pairs:
                for i in share[node]:
                    a[f * nx + x, i] += w / len(share[node])
    return a


def dense_of(plan):
    a = np.zeros((plan.rows, plan.n_lines))
    for r in range(plan.rows):
        for j in range(plan.row_ptr[r], plan.row_ptr[r + 1]):
            a[r, plan.index[j]] += float(plan.weight[j])
    return a


@pytest.mark.parametrize("n,nx,n_frames", SCHEDULES)
def test_nearest_equals_the_brute_force_restatement(n, nx, n_frames):
    pe, trig, rr = schedule(n, nx, n_frames, seed=n + nx)
    plan = G.plan_gating(pe, trig, rr, n_frames, nx, mode="nearest")
    phi = trig / rr
    want = dense_nearest(pe, phi, np.ones(n, bool), n_frames, nx)
    got = dense_of(plan)
    assert plan.weight.dtype == np.float32 and plan.index.dtype == np.int32 and plan.row_ptr.dtype == np.int32
    assert np.array_equal(got != 0, want != 0)
    assert np.array_equal(got, want.astype(np.float32).astype(np.float64))    # 1 / k rounded once
    counts = np.diff(plan.row_ptr)
    assert np.array_equal(plan.acquired, (counts > 0).reshape(n_frames, nx).astype(np.uint8))
    assert plan.entries == n and plan.info["used"] == n and plan.info["empty_rows"] == int((counts == 0).sum())
    if (n, nx, n_frames) == (200, 24, 5):
        assert (counts == 0).any() and (counts == 1).any() and (counts > 1).any()          # cells with 0, 1 and several readouts
    for r in range(plan.rows):                                                # acquisition order inside a cell
        idx = plan.index[plan.row_ptr[r]:plan.row_ptr[r + 1]]
        assert np.all(np.diff(idx) > 0)
        assert np.all(plan.weight[plan.row_ptr[r]:plan.row_ptr[r + 1]] == np.float32(1.0 / max(len(idx), 1)))


@pytest.mark.parametrize("n,nx,n_frames", SCHEDULES)
def test_linear_equals_the_brute_force_restatement(n, nx, n_frames):
    pe, trig, rr = schedule(n, nx, n_frames, seed=n + nx)
    plan = G.plan_gating(pe, trig, rr, n_frames, nx, mode="linear")
    phi = trig / rr
    want = dense_linear(pe, phi, np.ones(n, bool), n_frames, nx)
    got = dense_of(plan)
    # one rounding to float32 per entry; a readout appears once per row, so the dense sum adds nothing
    assert np.abs(got - want).max() <= 2.0 ** -24 * max(np.abs(want).max(), 1e-300)
    assert np.array_equal(got != 0, want != 0)
    sums = got.sum(axis=1)
    filled = np.diff(plan.row_ptr) > 0
    assert np.all(np.abs(sums[filled] - 1.0) <= 2.0 ** -23)                   # every row interpolates: its weights sum to 1
    acquired_x = np.array([np.any(pe == x) for x in range(nx)])
    assert np.array_equal(plan.acquired, np.broadcast_to(acquired_x.astype(np.uint8), (n_frames, nx)))
    if nx > 1:
        assert not plan.acquired[:, nx - 1].any()                             # an x without a readout stays empty in every frame
    if nx >= 7:                                                               # an x with a single readout: weight 1 in every frame
        single = int(np.flatnonzero(pe == nx - 2)[0])
        for f in range(n_frames):
            r = f * nx + nx - 2
            assert plan.row_ptr[r + 1] - plan.row_ptr[r] == 1 and plan.index[plan.row_ptr[r]] == single and plan.weight[plan.row_ptr[r]] == 1.0


def test_linear_wraps_around_at_the_first_and_last_frame():
    # one line, three nodes at 0.3, 0.5 (twice, equal shares) and 0.75; 5 frames with centres 0.1, 0.3, 0.5, 0.7, 0.9
    pe = np.zeros(4, dtype=np.int64)
    trig = np.array([750.0, 500.0, 300.0, 500.0])
    plan = G.plan_gating(pe, trig, RR, 5, 1, mode="linear")
    rows = [(plan.index[plan.row_ptr[r]:plan.row_ptr[r + 1]].tolist(), plan.weight[plan.row_ptr[r]:plan.row_ptr[r + 1]].tolist()) for r in range(5)]
    f32 = lambda v: float(np.float32(v))
    # frame 0: between 0.75 - 1 and 0.3: w_a = (0.3 - 0.1) / 0.55
    wa = (0.3 - 0.1) / (0.3 - (0.75 - 1.0))
    assert rows[0] == ([0, 2], [f32(wa), f32(1.0 - wa)])
    assert rows[1] == ([2], [1.0])                                            # a node at the centre: the neighbour of weight 0 is left out
    assert rows[2] == ([1, 3], [0.5, 0.5])                                    # the merged node, equal shares, acquisition order
    wa = (0.75 - 0.7) / (0.75 - 0.5)
    assert rows[3] == ([1, 3, 0], [f32(wa / 2), f32(wa / 2), f32(1.0 - wa)])
    wa = ((0.3 + 1.0) - 0.9) / ((0.3 + 1.0) - 0.75)                           # frame 4: between 0.75 and 0.3 + 1
    assert rows[4] == ([0, 2], [f32(wa), f32(1.0 - wa)])


@pytest.mark.parametrize("mode", G.MODES)
def test_rejected_and_out_of_range_readouts_are_counted_and_absent(mode):
    n, nx, n_frames = 80, 7, 5
    pe, trig, rr = schedule(n, nx, n_frames, seed=9)
    rr = rr.copy()
    rr[10:14] = 1400.0                                                        # a long beat: rejected, whatever else is wrong with it
    rr[14:16] = 700.0                                                         # a short one
    pe[12] = -1
    pe[20], pe[21] = -1, nx                                                   # outside [0, nx)
    trig[30], trig[31], trig[32] = -5.0, 1000.0, np.nan                      # phase < 0, == 1, not a number
    plan = G.plan_gating(pe, trig, rr, n_frames, nx, mode=mode, reject=(0.8, 1.2))
    assert plan.info["dropped_reject"] == 6 and plan.info["dropped_index"] == 2 and plan.info["dropped_phase"] == 3
    assert plan.info["used"] == n - 11 and plan.n_lines == n
    gone = set(range(10, 16)) | {20, 21, 30, 31, 32}
    assert not gone & set(plan.index.tolist())
    ok = np.array([i not in gone for i in range(n)])
    phi = np.where(ok, trig / rr, 0.0)
    want = (dense_nearest if mode == "nearest" else dense_linear)(pe, phi, ok, n_frames, nx)
    assert np.abs(dense_of(plan) - want).max() <= 2.0 ** -24
    assert set(np.flatnonzero(want.any(axis=0))) == set(plan.index.tolist())
    free = G.plan_gating(pe, trig, rr, n_frames, nx, mode=mode)               # without reject the beats stay
    late = sum(1 for i in range(n) if i not in (12, 20, 21) and not 0.0 <= trig[i] / rr[i] < 1.0)      # 30, 31, 32 and triggers past a short beat
    assert late >= 3 and free.info["dropped_reject"] == 0 and free.info["dropped_index"] == 3 and free.info["dropped_phase"] == late
    assert free.info["used"] == n - 3 - late


def test_the_validator_refuses_bad_csr_arrays():
    good = dict(n_frames=2, nx=2, n_lines=3, row_ptr=[0, 1, 1, 3, 4], index=[0, 2, 1, 0], weight=[1.0, 0.5, 0.5, 1.0])
    plan = G.GatingPlan(**good)
    assert plan.acquired.tolist() == [[1, 0], [1, 1]] and plan.entries == 4
    for change, match in ((dict(row_ptr=[0, 2, 1, 3, 4]), "non-decreasing"), (dict(row_ptr=[1, 1, 1, 3, 4]), "non-decreasing"),
                          (dict(row_ptr=[0, 1, 1, 3, 5]), "non-decreasing"), (dict(row_ptr=[0, 1, 3, 4]), "row_ptr has 4 entries"),
                          (dict(index=[0, 3, 1, 0]), "outside"), (dict(index=[0, -1, 1, 0]), "outside"),
                          (dict(weight=[1.0, float("nan"), 0.5, 1.0]), "not finite"), (dict(weight=[1.0, float("inf"), 0.5, 1.0]), "not finite"),
                          (dict(weight=[1.0, 1e300, 0.5, 1.0]), "not finite"), (dict(weight=[1.0, 0.5, 0.5]), "weights"),
                          (dict(n_lines=-1), "n_lines"), (dict(nx=0), "nx")):
        with pytest.raises(CineHipError, match=match):
            G.GatingPlan(**dict(good, **change))
    with pytest.raises(CineHipError, match="mode"):
        G.plan_gating([0], [1.0], RR, 1, 1, mode="cubic")
    with pytest.raises(CineHipError, match="one value per readout"):
        G.plan_gating([0, 0], [1.0], RR, 1, 1)


@pytest.mark.parametrize("t,nx", [(1, 1), (2, 7), (5, 24)])
def test_readouts_from_raw_round_trip_gives_one_unit_entry_per_acquired_cell(t, nx):
    rs = np.random.RandomState(t + nx)
    raw = (rs.standard_normal((t, nx, 3, 2)) + 1j * rs.standard_normal((t, nx, 3, 2))).astype(np.complex64)
    acq = (rs.uniform(size=(t, nx)) < 0.5).astype(np.uint8)
    acq[0, 0] = 1
    lines, pe, trig, rr = G.readouts_from_raw(raw, acq, rr_ms=850.0)
    assert lines.shape == (int(acq.sum()), 3, 2) and lines.dtype == np.complex64
    plan = G.plan_gating(pe, trig, rr, t, nx, mode="nearest")
    assert np.array_equal(plan.acquired, acq)
    assert plan.entries == int(acq.sum()) and np.all(plan.weight == 1.0)
    assert np.array_equal(np.diff(plan.row_ptr), acq.reshape(-1))
    assert np.array_equal(plan.index, np.arange(plan.entries))                # frame by frame, x ascending: the CSR order
    f, x = np.nonzero(acq)
    assert np.array_equal(lines, raw[f, x])
    assert all(v == 0 for k, v in plan.info.items() if k.startswith("dropped"))
