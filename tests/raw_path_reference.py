"""The float64 yardsticks, the seeded inputs and the case lists of the raw-path sweep (test_raw_path_kernels_cpu.py, test_raw_path_kernels.py):
cine_raw_ingest, cine_coil_compress, cine_coil_gram, cine_raw_window_ifft2c and cine_espirit_gram, the first kernels a raw scan meets.  Every
reference is numpy in float64; those of the Gram matrix and of the windowed transform are the ones test_coil_compress.py and
test_frontend_any_size.py hold, imported from there.

The thresholds of the case lists are restated here from the launch code (tile_width from cine_raw_ingest, compress_class from
cine_coil_compress, gram_plan from gram_plan in csrc/coil_kernels.hip); the CPU file holds the restatements to the library where the library
can be asked without a launch, and asserts that the lists reach every class the restatements name.

Inputs the kernels must never read hold NaN: frames >= t_out / t_use of every raw array, and for the two Gram matrices every sample outside
the central block."""
import functools

import numpy as np

from kernel_sweep import hash_case, sweep
from test_coil_compress import designed_raw, gram_ref                     # noqa: F401 (gram_ref is the sweep's Gram reference)
from test_frontend_any_size import _window_want as window_ref

BAR_GRAM = 1e-9                                # test_coil_compress.py::test_gram_vs_float64
BAR_WINDOW = 1e-5                              # test_frontend_any_size.py, lengths <= 1024
BAR_ESPIRIT = 1e-12                            # test_espirit_sign.py::test_gram_vs_float64
GRAM_WS_BUDGET = 64 << 20                      # cc::kGramWsBudget, the header's "partial sums stay below"


def key(c):
    return tuple(sorted(c.items()))


def crandn(seed, *shape):
    rs = np.random.RandomState(seed % (2 ** 31))
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)


def poison_frames(raw, t_keep):
    """raw with NaN in every frame >= t_keep."""
    raw = raw.copy()
    raw[t_keep:] = np.nan + 1j * np.nan
    return raw


# ================================================================== cine_raw_ingest
INGEST_LDS_BUDGET, INGEST_LDS_LIMIT = 18 * 1024, 64 * 1024
INGEST_COILS_MAX = 510                         # ldc = (c + 1) | 1 = 511: (16 * 511 + 1) * 8 = 65416 <= 65536; 511 coils: ldc 513
INGEST_COILS = [1, 2, 3, 15, 16, 17, 34, 35, 70, 71, 129, INGEST_COILS_MAX]
INGEST_PFORMS = ["below", "tile", "tile+1", "odd", "even"]
INGEST_FRAMES = [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 3)]
INGEST_SCALES = [1.0, 1e6, -0.5]
INGEST_SPLITS = ["nx1", "ny1", "both"]


def ingest_ldc(c):
    return (c + 1) | 1


def ingest_lds_bytes(c, tp):
    return (tp * ingest_ldc(c) + 1) * 8


def tile_width(c):
    """Samples per workgroup: the widest of 128, 64, 32, 16 whose staged tile fits the budget; 16 at least.  None: refused (the LDS limit)."""
    tp = 128
    while tp > 16 and ingest_lds_bytes(c, tp) > INGEST_LDS_BUDGET:
        tp >>= 1
    return tp if ingest_lds_bytes(c, tp) <= INGEST_LDS_LIMIT else None


def _pform(form, tp):
    return {"below": tp - 3, "tile": tp, "tile+1": tp + 1, "odd": 2 * tp + 1, "even": 2 * tp + 6}[form]


def _split(p, how):
    if how == "nx1":
        return 1, p
    if how == "ny1":
        return p, 1
    a = next((d for d in range(int(p ** 0.5), 1, -1) if p % d == 0), 1)
    return p // a, a


def _ingest_case(c, form, frames, scale, split):
    nx, ny = _split(_pform(form, tile_width(c)), split)
    return dict(c=c, nx=nx, ny=ny, t_in=frames[0], t_out=frames[1], scale=scale)


def _ingest_cases():
    axes = dict(c=INGEST_COILS, form=INGEST_PFORMS, frames=INGEST_FRAMES, scale=INGEST_SCALES, split=INGEST_SPLITS)
    cases = [_ingest_case(**s) for s in sweep(20_261, axes, 36)]
    # per tile width: an odd coil count with an odd P above two tiles and three kept frames (odd first element of the run of raw in frame 1,
    # odd destinations with a full tile), the same with one frame kept, and an even coil count with P a multiple of the tile
    for c_odd, c_even in ((3, 16), (17, 34), (35, 70), (71, INGEST_COILS_MAX)):
        tp = tile_width(c_odd)
        assert tp == tile_width(c_even)
        cases.append(dict(c=c_odd, nx=1, ny=2 * tp + 1, t_in=4, t_out=3, scale=1e6))
        cases.append(dict(c=c_odd, nx=2 * tp + 1, ny=1, t_in=1, t_out=1, scale=-0.5))
        cases.append(dict(c=c_even, nx=2, ny=tp, t_in=2, t_out=2, scale=1.0))
    cases.append(dict(c=1, nx=129, ny=1, t_in=2, t_out=2, scale=1.0))                  # one coil: a plane's parity is the frame's
    cases.append(dict(c=129, nx=3, ny=11, t_in=4, t_out=3, scale=1e6))                 # 33 samples at the 16-sample tile
    cases.append(dict(c=INGEST_COILS_MAX, nx=33, ny=1, t_in=2, t_out=2, scale=-0.5))   # the largest admitted count, odd P
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


INGEST_CASES = _ingest_cases()


def ingest_parities(c):
    """What a case reaches: (tile width, odd first element of a run of raw, odd destination with a full tile, everything even)."""
    tp, P, nc = tile_width(c["c"]), c["nx"] * c["ny"], c["c"]
    tiles = range(0, P, tp)
    odd_in = any(((t * P + p0) * nc) & 1 for t in range(c["t_out"]) for p0 in tiles)
    odd_full = any((((t * nc + k) * P + p0) & 1) and P - p0 >= tp for t in range(c["t_out"]) for k in range(nc) for p0 in tiles)
    even = nc % 2 == 0 and P % 2 == 0
    return tp, odd_in, odd_full, even


def ingest_input(c):
    raw = crandn(hash_case(c), c["t_in"], c["nx"], c["ny"], c["c"])
    return poison_frames(raw, c["t_out"])


def ingest_ref(raw, t_out, scale):
    """out[t, k, x, y] = scale * raw[t, x, y, k]: the float64 product of two float32 values is exact, so one rounding to float32 gives the
    bits of ONE fp32 product per component.  (t_out, c, nx, ny, 2) float32."""
    s = np.float64(np.float32(scale))
    z = np.moveaxis(raw[:t_out], 3, 1)
    out = np.stack([s * z.real.astype(np.float64), s * z.imag.astype(np.float64)], axis=-1)
    return np.ascontiguousarray(out.astype(np.float32))


# ================================================================== cine_coil_compress
COMPRESS_COILS = [1, 2, 3, 5, 30, 32, 33, 64, 65, 96, 127, 128]
COMPRESS_VIRTUAL = [1, 15, 16, 17, 32]
COMPRESS_M = [1, 63, 64, 65, 3 * 64 + 7]
COMPRESS_TS, COMPRESS_TILES_PER_WG = 64, 8
COMPRESS_MAX_COILS, COMPRESS_MAX_VIRTUAL = 128, 32
# M -> (t_in, t_out, nx, ny)
_COMPRESS_SHAPES = {1: (2, 1, 1, 1), 63: (4, 3, 3, 7), 64: (2, 2, 4, 8), 65: (1, 1, 5, 13), 199: (2, 1, 199, 1)}


def compress_class(c, v):
    """(NCT, QMAX) of the launch_compress instance: 16-column MFMA tiles of virtual coils, 16-byte pieces of a tile per thread."""
    return (1 if v <= 16 else 2), (4 if c <= 32 else 8 if c <= 64 else 16)


def compress_tiles(m):
    """(tiles of 64 samples, tiles per workgroup)."""
    tiles = (m + COMPRESS_TS - 1) // COMPRESS_TS
    return tiles, min(max(tiles // 1024, 1), COMPRESS_TILES_PER_WG)


def compress_lds_bytes(c, v):
    ldc = (c + 3) // 4 * 4 + 2
    return ((16 * compress_class(c, v)[0] + COMPRESS_TS) * ldc + COMPRESS_TS * v) * 8


def _multi_tile_m(per_wg):
    """The smallest M with 1024 per_wg tiles, plus 64 + 5: one more tile than a multiple of per_wg, the last one ragged."""
    return (1024 * per_wg - 1) * COMPRESS_TS + 1 + COMPRESS_TS + 5


def _compress_cases():
    cases, i = [], 0
    for c in COMPRESS_COILS:
        for v in COMPRESS_VIRTUAL:
            if v > c:
                continue
            m = COMPRESS_M[i % len(COMPRESS_M)]
            i += 1
            t_in, t_out, nx, ny = _COMPRESS_SHAPES[m]
            cases.append(dict(c=c, v=v, t_in=t_in, t_out=t_out, nx=nx, ny=ny))
    cases.append(dict(c=127, v=32, t_in=4, t_out=3, nx=3, ny=7))                      # odd M with odd c at the widest class
    cases.append(dict(c=128, v=32, t_in=2, t_out=1, nx=199, ny=1))                    # the largest LDS image
    cases.append(dict(c=3, v=1, t_in=2, t_out=1, nx=1, ny=199))
    for c, v in ((32, 17), (33, 16), (65, 17)):                                        # two tiles per workgroup, each coil class
        cases.append(dict(c=c, v=v, t_in=2, t_out=1, nx=_multi_tile_m(2), ny=1))
    cases.append(dict(c=5, v=2, t_in=1, t_out=1, nx=1, ny=_multi_tile_m(8)))           # eight tiles per workgroup
    return cases


COMPRESS_CASES = _compress_cases()


def compress_m(c):
    return c["t_out"] * c["nx"] * c["ny"]


@functools.lru_cache(maxsize=None)
def _compress_input(k):
    c = dict(k)
    raw = poison_frames(crandn(hash_case(c), c["t_in"], c["nx"], c["ny"], c["c"]), c["t_out"])
    return raw, crandn(hash_case(c) + 1, c["v"], c["c"])


def compress_input(c):
    """(raw (t_in, nx, ny, c) with NaN beyond t_out, matrix (v, c)), both complex64."""
    return _compress_input(key(c))


def compress_ref(raw, matrix, t_out):
    return raw[:t_out].astype(np.complex128) @ matrix.astype(np.complex128).T


@functools.lru_cache(maxsize=None)
def _compress_want(k):
    c = dict(k)
    raw, matrix = compress_input(c)
    return compress_ref(raw, matrix, c["t_out"])


def compress_want(c):
    return _compress_want(key(c))


def selection_matrix(v, c, seed):
    """(v, c) complex64 with a single 1 per row, and the coil every row selects."""
    pick = np.random.RandomState(seed).permutation(c)[:v]
    m = np.zeros((v, c), np.complex64)
    m[np.arange(v), pick] = 1
    return m, pick


# ================================================================== cine_coil_gram
GRAM_COILS = [1, 2, 31, 32, 33, 64, 65, 127, 128]
GRAM_REGIONS = ["0", "1", "7", "24", "nx+1"]
GRAM_SHAPES = [(26, 25), (9, 12), (25, 31), (30, 8)]                                    # (nx, ny): every parity pair
GRAM_FRAMES = [(2, 1), (3, 2), (2, 2)]
GRAM_TILE, GRAM_MAX_PARTIALS = 2048, 1024


def gram_plan(t, nx, ny, c, region):
    """gram_plan of csrc/coil_kernels.hip: samples in the block, samples per staged tile, samples per workgroup, partials, bytes."""
    rx = nx if region == 0 or region > nx else region
    ry = ny if region == 0 or region > ny else region
    n, p = t * rx * ry, c * (c + 1) // 2
    s = min(GRAM_TILE // c, 64)
    maxp = min(max(GRAM_WS_BUDGET // (p * 16), 1), GRAM_MAX_PARTIALS)
    per = (n + maxp - 1) // maxp
    run = (per + s - 1) // s * s
    nwg = (n + run - 1) // run
    return dict(N=n, S=s, run=run, nwg=nwg, bytes=nwg * p * 16)


def _gram_cases():
    axes = dict(c=GRAM_COILS, region=GRAM_REGIONS, shape=GRAM_SHAPES, frames=GRAM_FRAMES)
    cases = []
    for s in sweep(20_262, axes, 18):
        nx, ny = s["shape"]
        region = nx + 1 if s["region"] == "nx+1" else int(s["region"])
        cases.append(dict(c=s["c"], region=region, nx=nx, ny=ny, t_in=s["frames"][0], t_use=s["frames"][1]))
    cases.append(dict(c=128, region=24, nx=26, ny=25, t_in=3, t_use=2))                # the largest coil count on the default block
    cases.append(dict(c=128, region=3, nx=9, ny=12, t_in=2, t_use=1))                  # 9 samples: less than one staged tile of 16
    cases.append(dict(c=5, region=3, nx=8, ny=7, t_in=2, t_use=1))                     # the same at 64 samples per tile: one partial
    cases.append(dict(c=128, region=0, nx=48, ny=48, t_in=5, t_use=4))                 # 9216 samples on 508 partials: two tiles each
    cases.append(dict(c=2, region=0, nx=150, ny=151, t_in=4, t_use=3))                 # 67950 samples on 1024 partials: two tiles each
    return cases


GRAM_CASES = _gram_cases()


def gram_block(c):
    nx, ny, region = c["nx"], c["ny"], c["region"]
    rx, ry = (nx, ny) if region == 0 else (min(region, nx), min(region, ny))
    return nx // 2 - rx // 2, ny // 2 - ry // 2, rx, ry


@functools.lru_cache(maxsize=None)
def _gram_input(k):
    c = dict(k)
    raw = designed_raw(c["t_in"], c["nx"], c["ny"], c["c"], seed=hash_case(c) % (2 ** 31))
    x0, y0, rx, ry = gram_block(c)
    poisoned = np.full_like(raw, np.nan + 1j * np.nan)
    poisoned[:c["t_use"], x0:x0 + rx, y0:y0 + ry] = raw[:c["t_use"], x0:x0 + rx, y0:y0 + ry]
    return poisoned


def gram_input(c):
    """designed_raw with NaN in every frame >= t_use and at every sample outside the calibration block."""
    return _gram_input(key(c))


# ================================================================== cine_raw_window_ifft2c
# (t_in, nx, ny, coils, t_out, cx, cy, scale): the small shapes of test_frontend_any_size.py (lengths 1 and 2, no crop, t_out < t_in, 1, 3
# and 32 coils), then both axis orders ragged against the 64 x 64 x 16 tile in M, N and K of both GEMMs at once
WINDOW_CASES = [dict(t_in=a, nx=b, ny=c, c=d, t_out=e, cx=f, cy=g, scale=s) for (a, b, c, d, e, f, g, s) in [
    (2, 1, 2, 1, 2, 1, 2, 1.0),
    (2, 2, 1, 3, 1, 1, 1, 1e6),
    (4, 13, 7, 3, 3, 13, 5, 1e6),
    (3, 13, 7, 2, 3, 13, 7, 1.0),
    (3, 40, 36, 2, 2, 20, 17, 1e6),
    (2, 45, 50, 32, 2, 33, 18, 1e6),
    (3, 23, 70, 3, 2, 19, 65, 1e6),            # x first: 19 x 210 x 23, then 57 x 65 x 70
    (2, 67, 70, 3, 1, 66, 5, 1.0),             # y first: 201 x 5 x 70, then 66 x 15 x 67
]]


def window_x_first(c):
    nx, ny, cx, cy = c["nx"], c["ny"], c["cx"], c["cy"]
    return nx * ny * cx + ny * cx * cy <= nx * ny * cy + nx * cy * cx


def window_gemms(c):
    """(M, N, K) of the two GEMMs (rw_plan and cine_raw_window_ifft2c)."""
    nx, ny, nc, cx, cy = c["nx"], c["ny"], c["c"], c["cx"], c["cy"]
    if window_x_first(c):
        return (cx, ny * nc, nx), (cx * nc, cy, ny)
    return (nx * nc, cy, ny), (cx, nc * cy, nx)


def window_input(c):
    return poison_frames(crandn(hash_case(c), c["t_in"], c["nx"], c["ny"], c["c"]), c["t_out"])


def window_want(c):
    return window_ref(window_input(c), c["t_out"], c["cx"], c["cy"], float(np.float32(c["scale"])))


# ================================================================== cine_espirit_gram
ESPIRIT_MAX_COILS, ESPIRIT_MAX_N = 32, 1152
# odd extents; r clipped on one axis (c 3) and on both (c 8); r = kk: the block holds exactly one kernel; n = 1152; the largest c at kk = 5
ESPIRIT_CASES = [dict(c=1, kk=1, ny=5, nx=7, r=1), dict(c=1, kk=6, ny=9, nx=11, r=6), dict(c=3, kk=5, ny=13, nx=31, r=24),
                 dict(c=8, kk=6, ny=11, nx=9, r=24), dict(c=32, kk=6, ny=25, nx=27, r=24), dict(c=32, kk=5, ny=24, nx=21, r=12),
                 dict(c=2, kk=3, ny=8, nx=8, r=200)]
# refused: (case, code name)
ESPIRIT_REFUSED = [(dict(c=33, kk=5, ny=24, nx=24, r=12), "EUNSUPPORTED"), (dict(c=24, kk=7, ny=24, nx=24, r=12), "EUNSUPPORTED"),
                   (dict(c=32, kk=7, ny=24, nx=24, r=12), "EUNSUPPORTED"), (dict(c=4, kk=6, ny=40, nx=40, r=5), "EINVAL"),
                   (dict(c=4, kk=6, ny=5, nx=40, r=24), "EINVAL")]


def espirit_block(c):
    ry, rx = min(c["r"], c["ny"]), min(c["r"], c["nx"])
    return c["ny"] // 2 - ry // 2, c["nx"] // 2 - rx // 2, ry, rx


def espirit_input(c):
    """kavg (c, ny, nx) complex64 with NaN outside the central block."""
    k = crandn(hash_case(c), c["c"], c["ny"], c["nx"])
    y0, x0, ry, rx = espirit_block(c)
    out = np.full_like(k, np.nan + 1j * np.nan)
    out[:, y0:y0 + ry, x0:x0 + rx] = k[:, y0:y0 + ry, x0:x0 + rx]
    return out


def espirit_gram_ref(kavg, r, kk):
    """A^H A of the patch matrix of the central min(r, ny) x min(r, nx) block: one row per kk x kk patch, columns ordered (py, px, coil)."""
    nc, ny, nx = kavg.shape
    ry, rx = min(r, ny), min(r, nx)
    y0, x0 = ny // 2 - ry // 2, nx // 2 - rx // 2
    block = kavg[:, y0:y0 + ry, x0:x0 + rx].astype(np.complex128)
    a = np.empty(((ry - kk + 1) * (rx - kk + 1), kk * kk * nc), np.complex128)
    for y in range(ry - kk + 1):
        for x in range(rx - kk + 1):
            a[y * (rx - kk + 1) + x] = block[:, y:y + kk, x:x + kk].transpose(1, 2, 0).reshape(-1)
    return a.conj().T @ a
