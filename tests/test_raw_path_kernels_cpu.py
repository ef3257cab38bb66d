"""The parts of the raw-path sweep that need no GPU (the GPU half is test_raw_path_kernels.py, the yardsticks and case lists are in
raw_path_reference.py): that the case lists reach every class they are there for -- the four tile widths of cine_raw_ingest with every
parity of its two odd-first-element paths, the six launch_compress instances of cine_coil_compress with one and with several tiles per
workgroup, the staged-tile sizes of cine_coil_gram, cine_espirit_gram at c = 32 and n = 1152 --, the references against plain numpy, the
float64 condition (finite references from NaN-poisoned inputs; numpy's and torch's own float32 results within half the bar), the size
queries, and every refusal, all of which return before the first launch and so run here with made-up device addresses."""
import ctypes
import time

import numpy as np
import torch

import raw_path_reference as R
from kernel_sweep import BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, Worst, case_id

CODES = dict(EINVAL=EINVAL, EUNSUPPORTED=EUNSUPPORTED, EWORKSPACE=EWORKSPACE)
A, B, C = (ctypes.c_void_p(v) for v in (0x10000, 0x20000, 0x30000))          # never dereferenced


def L():
    from cine_hip._lib import lib
    return lib()


def _err():
    return L().cine_last_error().decode(errors="replace")


# ================================================================== the case lists reach what they are for
def test_ingest_tile_rule_and_limit():
    """The tile width changes at 17, 35 and 71 coils; 510 coils are the most the 64 KB of LDS take, and the library refuses 511."""
    assert [R.tile_width(c) for c in (1, 16, 17, 34, 35, 70, 71, 129, 510)] == [128, 128, 64, 64, 32, 32, 16, 16, 16]
    assert R.tile_width(R.INGEST_COILS_MAX) == 16 and R.tile_width(R.INGEST_COILS_MAX + 1) is None
    assert R.ingest_lds_bytes(510, 16) == 65416 and R.ingest_lds_bytes(511, 16) > R.INGEST_LDS_LIMIT
    for c in (16, 34, 70):                                               # the last count of a width fills the budget, the next leaves it
        assert R.ingest_lds_bytes(c, R.tile_width(c)) <= R.INGEST_LDS_BUDGET < R.ingest_lds_bytes(c + 1, R.tile_width(c))
    assert L().cine_raw_ingest(A, B, 1, 1, 16, R.INGEST_COILS_MAX + 1, 1, 1.0, None) == EUNSUPPORTED
    msg = _err()
    assert msg.startswith("cine_raw_ingest") and "511 coils" in msg and str(R.ingest_lds_bytes(511, 16)) in msg
    from cine_hip import _lib
    with open(_lib.HEADER_PATH) as f:
        assert f"the LDS limit ({R.INGEST_COILS_MAX}" in f.read()         # the header names the count this test pins


def test_ingest_cases_reach_every_class():
    cases = R.INGEST_CASES
    assert {c["c"] for c in cases} >= set(R.INGEST_COILS)
    assert {(c["t_in"], c["t_out"]) for c in cases} >= set(R.INGEST_FRAMES)
    assert {c["scale"] for c in cases} == set(R.INGEST_SCALES)
    assert any(c["nx"] == 1 and c["ny"] > 1 for c in cases) and any(c["ny"] == 1 and c["nx"] > 1 for c in cases)
    assert any(c["nx"] > 1 and c["ny"] > 1 for c in cases)
    seen = {}
    for c in cases:
        tp, odd_in, odd_full, even = R.ingest_parities(c)
        P = c["nx"] * c["ny"]
        forms = seen.setdefault(tp, dict(odd_in=0, odd_full=0, even=0, below=0, tile=0, plus1=0, odd2=0, ragged_even=0))
        forms["odd_in"] += odd_in and c["c"] % 2 == 1 and P % 2 == 1 and c["t_out"] >= 2
        forms["odd_full"] += odd_full and P % 2 == 1 and P > tp
        forms["even"] += even
        forms["below"] += P < tp
        forms["tile"] += P == tp
        forms["plus1"] += P == tp + 1
        forms["odd2"] += P % 2 == 1 and P > 2 * tp
        forms["ragged_even"] += P % 2 == 0 and P % 16 != 0
    assert set(seen) == {128, 64, 32, 16}
    for tp, forms in seen.items():
        print(f"tile {tp:3d}: {forms}")
        for k in ("odd_in", "odd_full", "even", "odd2"):
            assert forms[k] >= 1, (tp, k)
    for k in ("below", "tile", "plus1", "ragged_even"):                    # every form of P somewhere, the widest and the narrowest tile included
        assert sum(f[k] for f in seen.values()) >= 2, k
    assert any(c["c"] == R.INGEST_COILS_MAX and (c["nx"] * c["ny"]) % 2 == 1 for c in cases)
    assert any(c["c"] == 129 and c["nx"] * c["ny"] == 33 for c in cases) and any(c["c"] <= 16 and c["nx"] * c["ny"] == 257 for c in cases)
    assert len(cases) <= 60


def test_compress_cases_reach_every_class():
    cases = R.COMPRESS_CASES
    assert {c["c"] for c in cases} >= set(R.COMPRESS_COILS) and {c["v"] for c in cases} >= set(R.COMPRESS_VIRTUAL)
    assert {R.compress_m(c) for c in cases} >= set(R.COMPRESS_M)
    assert all(1 <= c["v"] <= c["c"] <= R.COMPRESS_MAX_COILS and c["v"] <= R.COMPRESS_MAX_VIRTUAL for c in cases)
    classes = {}
    for c in cases:
        classes.setdefault(R.compress_class(c["c"], c["v"]), set()).add(R.compress_tiles(R.compress_m(c))[1])
    assert set(classes) == {(n, q) for n in (1, 2) for q in (4, 8, 16)}, classes
    assert all(1 in per for per in classes.values())
    assert {q for (_, q), per in classes.items() if max(per) > 1} == {4, 8, 16}     # several tiles per workgroup in each coil class
    for c in cases:
        tiles, per = R.compress_tiles(R.compress_m(c))
        if per > 1:
            assert tiles % per != 0 and R.compress_m(c) % R.COMPRESS_TS != 0, c     # a short last workgroup, a ragged last tile
    eight = [c for c in cases if R.compress_tiles(R.compress_m(c))[1] == 8]
    assert [(c["c"], c["v"]) for c in eight] == [(5, 2)]
    assert any(R.compress_tiles(R.compress_m(c)) == (2049, 2) for c in cases)
    assert any(c["c"] % 2 and R.compress_m(c) % 2 and (R.compress_m(c) % R.COMPRESS_TS) % 2 for c in cases)      # `ne` odd in the last tile
    assert any(c["c"] % 2 and R.compress_m(c) == 1 for c in cases)
    # the branch that raises the kernel's dynamic LDS limit, in both instances of the widest class
    big = {R.compress_class(c["c"], c["v"]) for c in cases if R.compress_lds_bytes(c["c"], c["v"]) > 64 * 1024}
    assert big == {(1, 16), (2, 16), (2, 8)}                               # 64 coils onto 32 need 67072 bytes
    assert R.compress_lds_bytes(128, 32) == 116224 <= 160 * 1024
    assert any(c["v"] == c["c"] <= 32 for c in cases)


def test_gram_cases_reach_every_class():
    cases = R.GRAM_CASES
    assert {c["c"] for c in cases} >= set(R.GRAM_COILS)
    assert {c["region"] for c in cases} >= {0, 1, 7, 24} and any(c["region"] == c["nx"] + 1 for c in cases)
    assert {(c["nx"] % 2, c["ny"] % 2) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c["t_use"] < c["t_in"] for c in cases) and any(c["t_use"] == c["t_in"] for c in cases)
    plans = [R.gram_plan(c["t_use"], c["nx"], c["ny"], c["c"], c["region"]) for c in cases]
    assert {p["S"] for p in plans} >= {64, 62, 32, 31, 16}                 # S = min(2048 / c, 64) at 32, 33, 64, 65, 127 / 128 coils
    assert any(p["nwg"] == 1 and p["N"] < p["S"] for p in plans)           # fewer samples than one staged tile: a single partial
    assert any(c["t_use"] == 1 and c["region"] == 3 for c in cases)
    assert any(p["nwg"] > 1 and p["run"] == p["S"] for p in plans)         # one tile per workgroup
    assert sum(1 for p in plans if p["run"] > p["S"]) >= 2                 # several tiles per workgroup: a slot is read back and added to
    assert any(p["N"] % p["S"] for p in plans)                             # a ragged last tile
    assert any(c["c"] == 128 and c["region"] == 24 for c in cases)


def test_window_cases_reach_every_class():
    cases = R.WINDOW_CASES
    assert len(cases) <= 8 and {c["c"] for c in cases} >= {1, 3, 32}
    assert {1, 2} <= {n for c in cases for n in (c["nx"], c["ny"])}
    assert any(c["cx"] == c["nx"] and c["cy"] == c["ny"] for c in cases) and any(c["t_out"] < c["t_in"] for c in cases)
    assert all(max(c["nx"], c["ny"]) <= 1024 for c in cases)
    ragged = [c for c in cases if all(m % 64 and n % 64 and k % 16 for m, n, k in R.window_gemms(c)) and max(R.window_gemms(c)[0][:2]) > 64]
    assert {R.window_x_first(c) for c in ragged} == {True, False}, ragged
    assert {R.window_x_first(c) for c in cases} == {True, False}


def test_espirit_cases_reach_every_class():
    cases = R.ESPIRIT_CASES
    assert {(c["c"], c["kk"]) for c in cases} >= {(1, 1), (1, 6), (3, 5), (8, 6), (32, 6), (32, 5)}
    assert max(c["kk"] ** 2 * c["c"] for c in cases) == R.ESPIRIT_MAX_N == 32 * 36
    assert max(c["c"] for c in cases if c["kk"] == 5) == R.ESPIRIT_MAX_COILS          # 25 * 32 = 800 <= 1152: the coil limit decides
    assert any(c["ny"] % 2 and c["nx"] % 2 for c in cases)
    clipped = {(c["r"] > c["ny"], c["r"] > c["nx"]) for c in cases}
    assert (True, True) in clipped and ((True, False) in clipped or (False, True) in clipped) and (False, False) in clipped
    assert sum(1 for c in cases if c["r"] == c["kk"]) >= 2
    for c, _ in R.ESPIRIT_REFUSED:
        y0, x0, ry, rx = R.espirit_block(c)
        assert c["c"] > 32 or c["kk"] ** 2 * c["c"] > 1152 or min(ry, rx) < c["kk"]
    assert any(c["c"] <= 32 and 1152 < c["kk"] ** 2 * c["c"] <= 1152 + 49 for c, _ in R.ESPIRIT_REFUSED)


# ================================================================== the references against plain numpy
def test_ingest_reference_is_a_scaled_moveaxis():
    for shape, t_out, scale in (((2, 3, 5, 4), 1, 1e6), ((3, 1, 7, 3), 3, -0.5)):
        raw = R.crandn(sum(shape), *shape)
        want = (np.float32(scale) * np.moveaxis(raw[:t_out], 3, 1)).astype(np.complex64)      # numpy's own float32 products
        got = R.ingest_ref(raw, t_out, scale)
        assert got.dtype == np.float32 and got.shape == (t_out, shape[3], shape[1], shape[2], 2)
        assert np.array_equal(got[..., 0].view(np.int32), np.ascontiguousarray(want.real).view(np.int32))
        assert np.array_equal(got[..., 1].view(np.int32), np.ascontiguousarray(want.imag).view(np.int32))


def test_compress_reference_is_the_sum_it_names():
    for (t, nx, ny, c, v), t_out in (((2, 2, 3, 4, 2), 1), ((1, 1, 5, 3, 3), 1)):
        raw, m = R.crandn(1, t, nx, ny, c), R.crandn(2, v, c)
        got = R.compress_ref(raw, m, t_out)
        want = np.zeros((t_out, nx, ny, v), np.complex128)
        for j in range(v):
            for k in range(c):
                want[..., j] += m[j, k].astype(np.complex128) * raw[:t_out, ..., k]
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    m, pick = R.selection_matrix(3, 5, 0)
    assert (m.sum(axis=1) == 1).all() and (m != 0).sum() == 3 and np.array_equal(m[np.arange(3), pick], np.ones(3, np.complex64))


def test_gram_reference_is_the_sum_it_names():
    for c in (dict(c=3, region=2, nx=5, ny=4, t_in=2, t_use=1), dict(c=2, region=0, nx=3, ny=3, t_in=2, t_use=2)):
        raw = R.gram_input(c)
        x0, y0, rx, ry = R.gram_block(c)
        want = np.zeros((c["c"], c["c"]), np.complex128)
        for t in range(c["t_use"]):
            for x in range(x0, x0 + rx):
                for y in range(y0, y0 + ry):
                    s = raw[t, x, y].astype(np.complex128)
                    want += np.outer(s, s.conj())
        got = R.gram_ref(raw, c["t_use"], c["region"])
        assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_window_reference_is_the_centred_dft():
    for c in (dict(t_in=2, nx=5, ny=4, c=2, t_out=1, cx=3, cy=4, scale=2.0), dict(t_in=1, nx=2, ny=7, c=1, t_out=1, cx=1, cy=5, scale=1.0)):
        raw = R.window_input(c)
        nx, ny, cx, cy = c["nx"], c["ny"], c["cx"], c["cy"]

        def d(n, cw):
            m = (n - cw) // 2 + np.arange(cw)
            return np.exp(2j * np.pi * np.outer(m - n // 2, np.arange(n) - n // 2) / n) / np.sqrt(n)
        want = c["scale"] * np.einsum("ix,jy,txyc->tcij", d(nx, cx), d(ny, cy), raw[:c["t_out"]].astype(np.complex128))
        got = R.window_want(c)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_espirit_gram_reference_is_the_oracles():
    from oracle.frontend_ref import calibration_matrix
    for c in (dict(c=2, kk=2, ny=5, nx=6, r=4), dict(c=3, kk=3, ny=4, nx=9, r=7)):
        kavg = R.espirit_input(c)
        y0, x0, ry, rx = R.espirit_block(c)
        a = calibration_matrix(kavg[:, y0:y0 + ry, x0:x0 + rx].astype(np.complex128), c["kk"])
        got = R.espirit_gram_ref(kavg, c["r"], c["kk"])
        assert got.shape == (c["kk"] ** 2 * c["c"],) * 2 and np.array_equal(got, a.conj().T @ a)


# ================================================================== the float64 condition
YARD = Worst()


def test_ingest_references_are_finite_and_exact_products():
    for c in R.INGEST_CASES:
        raw = R.ingest_input(c)
        assert np.isnan(raw[c["t_out"]:]).all() and np.isfinite(raw[:c["t_out"]]).all()
        ref = R.ingest_ref(raw, c["t_out"], c["scale"])
        assert np.isfinite(ref).all() and ref.shape == (c["t_out"], c["c"], c["nx"], c["ny"], 2)
        assert float(np.float32(c["scale"])) == c["scale"]                 # the scale is a float32 value: the product is the kernel's


def test_compress_references_are_finite_and_float32_is_within_half_the_bar():
    worst_time = 0.0
    for c in R.COMPRESS_CASES:
        raw, m = R.compress_input(c)
        assert np.isnan(raw[c["t_out"]:]).all()
        t0 = time.perf_counter()
        want = R.compress_ref(raw, m, c["t_out"])
        worst_time = max(worst_time, time.perf_counter() - t0)
        assert np.isfinite(want).all() and want.shape == (c["t_out"], c["nx"], c["ny"], c["v"])
        got = raw[:c["t_out"]] @ m.T                                       # numpy's own complex64 product
        assert got.dtype == np.complex64
        YARD.record("compress, numpy float32", float(np.abs(got - want).max() / np.abs(want).max()), BAR / 2, case_id(c))
    print(f"the slowest float64 product of the compress cases: {worst_time:.2f} s")
    assert worst_time < 5.0


def test_gram_references_are_finite():
    for c in R.GRAM_CASES:
        raw = R.gram_input(c)
        x0, y0, rx, ry = R.gram_block(c)
        inside = np.zeros(raw.shape[:3], bool)
        inside[:c["t_use"], x0:x0 + rx, y0:y0 + ry] = True
        assert np.isfinite(raw[inside]).all() and np.isnan(raw[~inside]).all()
        g = R.gram_ref(raw, c["t_use"], c["region"])
        assert g.shape == (c["c"], c["c"]) and np.isfinite(g).all() and np.abs(g).max() > 0


def test_window_references_are_finite_and_float32_is_within_half_the_bar():
    for c in R.WINDOW_CASES:
        raw, want = R.window_input(c), R.window_want(c)
        assert np.isnan(raw[c["t_out"]:]).all() and np.isfinite(want).all()
        assert want.shape == (c["t_out"], c["c"], c["cx"], c["cy"])
        x = torch.from_numpy(raw[:c["t_out"]]).permute(0, 3, 1, 2) * np.float32(c["scale"])
        img = torch.fft.fftshift(torch.fft.ifftn(torch.fft.ifftshift(x, dim=(-2, -1)), dim=(-2, -1), norm="ortho"), dim=(-2, -1))
        assert img.dtype == torch.complex64                                # torch's own float32 transform
        x0, y0 = (c["nx"] - c["cx"]) // 2, (c["ny"] - c["cy"]) // 2
        got = img[:, :, x0:x0 + c["cx"], y0:y0 + c["cy"]].numpy()
        peak = max(np.abs(want.real).max(), np.abs(want.imag).max())
        err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()) / peak
        YARD.record("window, torch float32", float(err), R.BAR_WINDOW / 2, case_id(c))


def test_espirit_references_are_finite():
    for c in R.ESPIRIT_CASES:
        kavg = R.espirit_input(c)
        assert np.isnan(kavg).any() or (c["r"] >= c["ny"] and c["r"] >= c["nx"])
        g = R.espirit_gram_ref(kavg, c["r"], c["kk"])
        assert g.shape == (c["kk"] ** 2 * c["c"],) * 2 and np.isfinite(g).all() and np.abs(g).max() > 0


def test_float32_yardstick_report():
    """Prints the yardsticks of the tests above (run with -s)."""
    if YARD:
        YARD.report()


# ================================================================== the size queries
def test_gram_workspace_query():
    lib = L()
    for c in R.GRAM_CASES:
        plan = R.gram_plan(c["t_use"], c["nx"], c["ny"], c["c"], c["region"])
        got = lib.cine_coil_gram_ws_bytes(c["t_use"], c["nx"], c["ny"], c["c"], c["region"])
        assert got == plan["bytes"] > 0 and got <= R.GRAM_WS_BUDGET, (c, got, plan)
    assert lib.cine_coil_gram_ws_bytes(15, 832, 832, 128, 0) <= R.GRAM_WS_BUDGET        # a large scan stays within the budget too
    for args in ((0, 8, 8, 4, 0), (1, 0, 8, 4, 0), (1, 8, 0, 4, 0), (1, 8, 8, 0, 0), (1, 8, 8, 4, -1), (1, 8, 8, 129, 0)):
        assert lib.cine_coil_gram_ws_bytes(*args) == 0, args


def test_window_workspace_query():
    lib = L()

    def up(n):
        return (n + 255) // 256 * 256
    for c in R.WINDOW_CASES:
        z = c["t_out"] * (c["cx"] * c["ny"] if R.window_x_first(c) else c["nx"] * c["cy"]) * c["c"]
        want = up(c["cx"] * c["nx"] * 8) + up(c["cy"] * c["ny"] * 8) + up(z * 8)
        assert lib.cine_raw_window_ws_bytes(c["t_out"], c["nx"], c["ny"], c["c"], c["cx"], c["cy"]) == want > 0, c
    for args in ((0, 8, 8, 2, 4, 4), (1, 0, 8, 2, 4, 4), (1, 8, 8, 0, 4, 4), (1, 8, 8, 2, 9, 4), (1, 8, 8, 2, 4, 0)):
        assert lib.cine_raw_window_ws_bytes(*args) == 0, args


def test_espirit_workspace_query():
    lib = L()
    for c in R.ESPIRIT_CASES:
        _, _, ry, rx = R.espirit_block(c)
        assert lib.cine_espirit_gram_ws_bytes(c["c"], c["ny"], c["nx"], c["r"], c["kk"]) == ry * rx * c["c"] * 16 > 0, c
    for c, _ in R.ESPIRIT_REFUSED:                                         # the header: 0 for shapes it refuses
        assert lib.cine_espirit_gram_ws_bytes(c["c"], c["ny"], c["nx"], c["r"], c["kk"]) == 0, c
    for args in ((0, 8, 8, 6, 2), (2, 0, 8, 6, 2), (2, 8, 8, 0, 2), (2, 8, 8, 6, 0)):
        assert lib.cine_espirit_gram_ws_bytes(*args) == 0, args


# ================================================================== refusals, with made-up addresses
def _refusals():
    """(name, call, code): the refusals test_raw_path_kernels.py repeats with guarded outputs."""
    lib, big = L(), 1 << 30
    off8 = ctypes.c_void_p(A.value + 8)
    return [
        ("cine_raw_ingest 8-byte raw", lambda: lib.cine_raw_ingest(off8, B, 2, 4, 4, 3, 1, 1.0, None), EINVAL),
        ("cine_raw_ingest 8-byte out", lambda: lib.cine_raw_ingest(A, ctypes.c_void_p(B.value + 8), 2, 4, 4, 3, 1, 1.0, None), EINVAL),
        ("cine_raw_ingest t_out > t_in", lambda: lib.cine_raw_ingest(A, B, 2, 4, 4, 3, 3, 1.0, None), EINVAL),
        ("cine_raw_ingest aliased", lambda: lib.cine_raw_ingest(A, A, 2, 4, 4, 3, 1, 1.0, None), EINVAL),
        ("cine_raw_ingest 511 coils", lambda: lib.cine_raw_ingest(A, B, 2, 4, 4, 511, 1, 1.0, None), EUNSUPPORTED),
        ("cine_coil_compress 8-byte raw", lambda: lib.cine_coil_compress(off8, B, C, 2, 4, 4, 3, 1, 2, None), EINVAL),
        ("cine_coil_compress 8-byte out", lambda: lib.cine_coil_compress(A, B, ctypes.c_void_p(C.value + 8), 2, 4, 4, 3, 1, 2, None), EINVAL),
        ("cine_coil_compress 129 coils", lambda: lib.cine_coil_compress(A, B, C, 2, 4, 4, 129, 1, 2, None), EUNSUPPORTED),
        ("cine_coil_compress 33 virtual", lambda: lib.cine_coil_compress(A, B, C, 2, 4, 4, 64, 1, 33, None), EUNSUPPORTED),
        ("cine_coil_compress v > c", lambda: lib.cine_coil_compress(A, B, C, 2, 4, 4, 3, 1, 4, None), EINVAL),
        ("cine_coil_compress t_out > t_in", lambda: lib.cine_coil_compress(A, B, C, 2, 4, 4, 3, 3, 2, None), EINVAL),
        ("cine_coil_compress raw == out", lambda: lib.cine_coil_compress(A, B, A, 2, 4, 4, 3, 1, 2, None), EINVAL),
        ("cine_coil_compress matrix == out", lambda: lib.cine_coil_compress(A, B, B, 2, 4, 4, 3, 1, 2, None), EINVAL),
        ("cine_coil_gram 8-byte gram", lambda: lib.cine_coil_gram(A, ctypes.c_void_p(B.value + 8), C, big, 2, 4, 4, 3, 1, 0, None), EINVAL),
        ("cine_coil_gram 8-byte ws", lambda: lib.cine_coil_gram(A, B, ctypes.c_void_p(C.value + 8), big, 2, 4, 4, 3, 1, 0, None), EINVAL),
        ("cine_coil_gram 129 coils", lambda: lib.cine_coil_gram(A, B, C, big, 2, 4, 4, 129, 1, 0, None), EUNSUPPORTED),
        ("cine_coil_gram t_use > t_in", lambda: lib.cine_coil_gram(A, B, C, big, 2, 4, 4, 3, 3, 0, None), EINVAL),
        ("cine_coil_gram raw == gram", lambda: lib.cine_coil_gram(A, A, C, big, 2, 4, 4, 3, 1, 0, None), EINVAL),
        ("cine_coil_gram gram == ws", lambda: lib.cine_coil_gram(A, B, B, big, 2, 4, 4, 3, 1, 0, None), EINVAL),
        ("cine_coil_gram short ws",
         lambda: lib.cine_coil_gram(A, B, C, lib.cine_coil_gram_ws_bytes(1, 4, 4, 3, 0) - 1, 2, 4, 4, 3, 1, 0, None), EWORKSPACE),
        ("cine_raw_window_ifft2c t_out > t_in", lambda: lib.cine_raw_window_ifft2c(A, B, C, big, 2, 4, 4, 3, 3, 2, 2, 1.0, None), EINVAL),
        ("cine_raw_window_ifft2c aliased", lambda: lib.cine_raw_window_ifft2c(A, A, C, big, 2, 4, 4, 3, 1, 2, 2, 1.0, None), EINVAL),
        ("cine_raw_window_ifft2c short ws",
         lambda: lib.cine_raw_window_ifft2c(A, B, C, lib.cine_raw_window_ws_bytes(1, 4, 4, 3, 2, 2) - 1, 2, 4, 4, 3, 1, 2, 2, 1.0, None),
         EWORKSPACE),
        ("cine_espirit_gram 8-byte gram", lambda: lib.cine_espirit_gram(A, ctypes.c_void_p(B.value + 8), C, big, 2, 8, 8, 6, 2, None), EINVAL),
        ("cine_espirit_gram aliased", lambda: lib.cine_espirit_gram(A, B, B, big, 2, 8, 8, 6, 2, None), EINVAL),
        ("cine_espirit_gram short ws",
         lambda: lib.cine_espirit_gram(A, B, C, lib.cine_espirit_gram_ws_bytes(2, 8, 8, 6, 2) - 1, 2, 8, 8, 6, 2, None), EWORKSPACE),
    ] + [(f"cine_espirit_gram {case_id(c)}",
          lambda c=c: lib.cine_espirit_gram(A, B, C, big, c["c"], c["ny"], c["nx"], c["r"], c["kk"], None), CODES[code])
         for c, code in R.ESPIRIT_REFUSED]


def test_refusals_before_any_launch():
    for what, call, code in _refusals():
        assert L().cine_scale(None, 1, 1.0, None) == EINVAL                # another entry point's message in between
        assert call() == code, (what, _err())
        assert _err().startswith(what.split()[0]), (what, _err())
