"""The centered transforms and the coil / data-consistency operators of include/cine_hip.h (csrc/fft_kernels.hip + fft_core.h and the
small kernels either side of them) called one by one through the C ABI, shape by shape, against float64 references on the CPU.

Entry points
  A  cine_fft1c, cine_fft2c, cine_fft_line_supported, cine_kspace_to_hybrid, cine_masked_kspace_to_hybrid
  B  cine_hybrid_reduce, cine_sens_reduce, cine_sens_expand_dc, cine_expand_dc_hybrid, cine_zero_filled_rss, cine_sens_prologue,
     cine_acs_window + cine_sens_prologue_win, cine_rss_normalise, cine_apply_mask, cine_scale
  C  cine_image_dc, cine_image_dc_t + cine_sens_tile_pack, cine_normal_op, cine_normal_op_t, cine_normal_op_pd,
     cine_image_dc_sens_grad + cine_coil_accum
Out of scope, by decision: the conjugate-gradient solver entry points (cine_cg_*, cine_conj_grad*, cine_normal_op_cg_fused*, cine_dot,
cine_axpby_*).  An iterative solver needs another kind of bar: they have a sweep of their own, test_cg_kernels.py.

References: complex128 on the CPU from the header's definitions and the reference's formulas -- fftshift(fft(ifftshift(x), "ortho")) with
torch.fft, the coil sums and products of varnet.py:181-194 / 281-282, softplus in float64.  The image-space operators (group C) are
compared with the COMPOSITION sens_reduce(DC(sens_expand(img))) with the k-space blend written out, not with the commuted single-axis
formula their kernels implement; cine_image_dc_sens_grad with float64 autograd of that composition.  Inputs are float32 values
(what the kernel sees), widened.  The CPU tests (no gpu mark) pin these references to oracle/ and to the reference's own recorded
outputs (tests/golden/ops.npz, fft_smooth.npz, varnet_block.npz) at 1e-6.

The route of a case is a pure function of its shape; the host-side rules are restated below (line_supported, engine, coil_tiling,
lds_opt_in, image_dc_ws_bytes, split_step) and the CPU tests assert that the case lists reach every value of every axis.  The 1-D list is
exhaustive: every supported length 1 .. 512, both directions, both shift variants.

Every GPU case checks: the error, conftest.rel_err (max |d| / peak of the reference) at kernel_sweep.BAR = 1e-5; a NaN prefill of every
output (the result must not depend on what the buffer held); guard floats on both sides of every output, and of tmp / hyb where the
call writes them; inputs the header does not declare destroyed are bit-unchanged; a second identical call gives the same bits.  Subsets
run again with every float pointer at a storage offset of 2 floats (8 bytes: complex-aligned, not 16-byte aligned) and must give the
bits of the aligned call.  Refusals are decided on the host before any launch: return code, message, outputs untouched.
No case needed the chained-operator yardstick of kernel_sweep._bar: every entry point meets BAR itself (DESIGN.md section 4c has the
measured worst error / bar per entry point and the mutations the sweep was tried against).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err, rnd
from kernel_sweep import (BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, NAN, Call, GuardedInt, L as _L, Worst, at_offsets as _at_offsets, cap_samples, case_id,
                          check as _check, hash_case, ptr as _p, refused as _refused, same_bits, stream as _stream, sweep, twice as _twice)

PIN = 1e-6                                      # float32 fixtures against a float64 restatement


# ================================================================== float64 references (CPU)
def cplx(x):
    """(..., 2) float32 pairs -> complex128."""
    return torch.view_as_complex(x.double().contiguous())


def pairs(z):
    """complex128 -> (..., 2) float64 pairs."""
    return torch.view_as_real(z.contiguous())


def ref_fftc(z, dims, inverse=False, variant=0):
    """Centered ortho transform over dims.  variant 0: fftshift(f(ifftshift(z))) (fftc.py); variant 1 forward:
    ifftshift(fft(fftshift(z))) (xpdnet.py:466); variant 1 inverse has the fftc.py order (xpdnet.py:500)."""
    f = torch.fft.ifftn if inverse else torch.fft.fftn
    if variant == 1 and not inverse:
        return torch.fft.ifftshift(f(torch.fft.fftshift(z, dim=dims), dim=dims, norm="ortho"), dim=dims)
    return torch.fft.fftshift(f(torch.fft.ifftshift(z, dim=dims), dim=dims, norm="ortho"), dim=dims)


def ref_softplus(lam):
    """log(1 + exp(x)) in float64 of the float32 value, without the shortcut above 20 that F.softplus and the kernels take."""
    x = torch.tensor(float(np.float32(lam)), dtype=torch.float64)
    return float(torch.log1p(torch.exp(x)))


def ref_to_hybrid(k):
    """Centered column IFFT (over h) of (..., h, w) k-space."""
    return ref_fftc(k, (-2,), inverse=True)


def ref_sens_expand(img, S):
    """varnet.py:181-185: img (b, t, h, w), S (b, c, h, w) -> (b, t, c, h, w)."""
    return ref_fftc(S[:, None] * img[:, :, None], (-2, -1))


def ref_sens_reduce(k, S):
    """varnet.py:187-194: k (b, t, c, h, w) -> (b, t, h, w)."""
    return (S.conj()[:, None] * ref_fftc(k, (-2, -1), inverse=True)).sum(2)


def _rows(mask):
    """mask (b, t, h) uint8 -> bool (b, t, 1, h, 1)."""
    return mask.bool()[:, :, None, :, None]


def ref_blend(kth, kref, mask, lam, hard):
    """The data-consistency step of cine_sens_expand_dc on kth (b, t, c, h, w): soft (varnet.py:281-282), hard_mask 1 (cinenet.py:121-133),
    hard_mask 2 (xpdnet.py:128-131).  torch.where selects: what kref holds on dropped rows never enters the result."""
    if hard == 1:
        return torch.where(_rows(mask), kth, torch.zeros_like(kth))
    if hard == 2:
        return torch.where(_rows(mask), kth - kref, torch.zeros_like(kth))
    if kref is None:
        return kth
    v = ref_softplus(lam)
    return torch.where(_rows(mask), (kth + v * kref) / (1 + v), kth)


def ref_image_dc(img, S, mask, lam=None, kref=None, weights=None, zf=None):
    """sens_reduce(DC(sens_expand(img))) as a composition.  lam given: the soft DC against kref (zero when None).  Else weights
    (w_sampled, w_unsampled, beta): k-space rows scaled by the mask's weight, plus beta * zf."""
    kth = ref_sens_expand(img, S)
    if lam is not None:
        return ref_sens_reduce(ref_blend(kth, torch.zeros_like(kth) if kref is None else kref, mask, lam, 0), S)
    w1, w0, beta = (float(np.float32(x)) for x in weights)
    out = ref_sens_reduce(torch.where(_rows(mask), w1 * kth, w0 * kth), S)
    return out if zf is None else out + beta * zf


def ref_normal_op(img, S, mask, lam):
    """cinenet.py:121-133: A^H M A img + softplus(lambda) img."""
    kth = ref_sens_expand(img, S)
    return ref_sens_reduce(torch.where(_rows(mask), kth, torch.zeros_like(kth)), S) + ref_softplus(lam) * img


def ref_image_dc_sens_grad(img, g, S, mask, lam=None, weights=None):
    """Float64 autograd of ref_image_dc's composition with respect to the maps, per frame: (b, t, c, h, w), for the output gradient g
    in the real-pair convention d loss = Re(conj(g) d out) (torch's complex gradient of a real loss is d/d re + i d/d im)."""
    b, t = img.shape[:2]
    Sbt = S[:, None].expand(b, t, *S.shape[1:]).clone().requires_grad_(True)
    w1, w0 = (1 / (1 + ref_softplus(lam)), 1.0) if lam is not None else (float(np.float32(weights[0])), float(np.float32(weights[1])))
    with torch.enable_grad():
        kth = ref_fftc(Sbt * img[:, :, None], (-2, -1))
        k = torch.where(_rows(mask), w1 * kth, w0 * kth)
        out = (Sbt.conj() * ref_fftc(k, (-2, -1), inverse=True)).sum(2)
        (g.conj() * out).real.sum().backward()
    return Sbt.grad


def ref_acs_window(rows, h):
    """cine_acs_window: rows[:h] of the 1-D pattern; left = the last unsampled row below h // 2, right = the first one at or above it;
    {pad, pad + n_low} with n_low = right - left, pad = (h - n_low + 1) // 2; every row when either side has no unsampled row."""
    rows = list(rows[:h])
    cent = h // 2
    left = max([i for i in range(cent) if rows[i] == 0], default=-1)
    right = min([i for i in range(cent, h) if rows[i] == 0], default=h)
    if left < 0 or right >= h:
        return [0, h]
    n_low = right - left
    pad = (h - n_low + 1) // 2
    return [max(pad, 0), min(pad + n_low, h)]


def ref_tile_pack(S):
    """cine_sens_tile_pack's layout [b][c][ceil(w / 5)][200][5] of S (b, c, 200, w, 2), zero past the last column."""
    b, c, h, w, _ = S.shape
    ntx = -(-w // 5)
    out = np.zeros((b, c, ntx, h, 5, 2), np.float32)
    for tile in range(ntx):
        n = min(5, w - 5 * tile)
        out[:, :, tile, :, :n] = S[:, :, :, 5 * tile:5 * tile + n].numpy()
    return torch.from_numpy(out)


# ================================================================== the host-side rules of csrc/fft_kernels.hip, restated
SPLIT = 32768                  # images per column-pass launch (grid.y <= 65535)
MAX_BT = 65535


def smooth(n):
    """2^a 3^b 5^c, n >= 2 (MixedRadix::smooth)."""
    if n < 2:
        return False
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def line_supported(n):
    return n >= 1 and (n <= 400 or (n <= 512 and smooth(n)))


def engine(n):
    return "200" if n == 200 else "smooth" if smooth(n) else "direct"


def lds_opt_in(n):
    """The generic line kernels hold two n x 9 tiles and n twiddles: more than the default 64 KB of dynamic LDS from n = 432."""
    return n != 200 and (2 * n * 9 + n) * 8 > 64 * 1024


def coil_tiling(C, W):
    """(rows per workgroup, coils per chunk, shrunk) of the coil-mode row passes."""
    lines, threads = (16, 160) if W == 200 else (8, 256)
    cc = min(C, lines)
    rpw = lines // cc
    first = rpw
    while rpw > 1 and rpw * W > 4 * threads:
        rpw -= 1
    return rpw, cc, rpw < first


def image_dc_ws_bytes(b, t, c, h, w):
    return 0 if h != 200 or c <= 5 else -(-c // 5) * b * t * h * w * 8


def split_step(c):
    return SPLIT // c * c


SUPPORTED = [n for n in range(1, 513) if line_supported(n)]


def fft1c_nlines(n):
    """nlines = 1 and a count that leaves the last workgroup ragged (8 lines per workgroup, 32 at n = 200)."""
    return (1, 37 if n == 200 else 9 + n % 7)


# ================================================================== case lists
def _rand(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed % (2 ** 31)).standard_normal(shape).astype(np.float32))


def make_mask(seed, bt, h, kind):
    """uint8 (bt, h): "none" keeps no row, "all" every row, "one" one row (the same in every frame), "frame" a pattern per frame
    (every frame keeps at least one row and drops at least one where h > 1)."""
    rs = np.random.RandomState(seed % (2 ** 31))
    m = np.zeros((bt, h), np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "one":
        m[:, rs.randint(h)] = 1
    elif kind == "frame":
        m[:] = rs.rand(bt, h) < 0.5
        kept = rs.randint(h, size=bt)
        m[np.arange(bt), kept] = 1
        if h > 1:
            m[np.arange(bt), (kept + 1) % h] = 0
    else:
        assert kind == "none", kind
    return torch.from_numpy(m)


LAMBDAS = [-30.0, -1.3, 0.5413, 19.9, 20.1, 25.0]          # both sides of softplus1's switch at 20
MASKS = ["none", "all", "one", "frame"]

# ---- group A, 2-D
T2_AXES = dict(h=[200, 24, 96, 400, 405, 432, 450, 480, 486, 500, 512, 397, 399, 203, 1, 2, 7],
               w=[200, 20, 120, 384, 405, 432, 450, 480, 486, 500, 512, 397, 399, 203, 1, 2, 13, 9],
               n=[1, 2, 3], inverse=[0, 1], alias=[False, True], premask=MASKS, coils=[1, 2, 3])
_T2 = sweep(11, T2_AXES, 36)
_T2 += [dict(h=h, w=w, n=n, inverse=i, alias=a, premask=p, coils=c) for h, w, n, i, a, p, c in [
    (200, 200, 2, 0, False, "frame", 2), (200, 1, 3, 1, True, "one", 3), (200, 13, 2, 0, True, "frame", 1),
    (200, 405, 1, 1, False, "all", 2), (1, 1, 3, 0, False, "all", 1), (2, 3, 3, 1, True, "frame", 3),
    (512, 512, 1, 0, False, "frame", 1), (1, 200, 2, 1, False, "none", 2), (432, 200, 1, 0, True, "one", 2),
    (397, 8, 2, 1, False, "frame", 3), (500, 33, 1, 0, False, "none", 1)]]
for _c in _T2:
    _c["n"] = cap_samples(_c["n"], _c["h"] * _c["w"] * _c["coils"], 400_000)
T2_CASES = _T2
SPLIT_NIMG = SPLIT + 5                                     # cine_fft2c / cine_kspace_to_hybrid: 2 x 3 images
SPLIT_BT = 10_925                                          # c = 3: 32 775 images, the second chunk starts at frame 10 922

# ---- group B
B_AXES = dict(C=[1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 30, 32, 33], w=[1, 7, 20, 33, 130, 200, 300, 432], h=[1, 2, 3, 5, 7, 24, 200],
              b=[1, 2, 3], t=[1, 2, 3], magnitude=[0, 1], mode=["plain", "soft", "hard1", "hard1_kref", "hard2"],
              lam=LAMBDAS, mask=MASKS)
_B = sweep(23, B_AXES, 39)
_B += [dict(C=C, w=w, h=h, b=b, t=t, magnitude=m, mode=mode, lam=lam, mask=mk) for C, w, h, b, t, m, mode, lam, mk in [
    (1, 200, 7, 2, 2, 0, "soft", 0.5413, "frame"),      # w = 200: rpw 16 -> 3, h % 3 != 0
    (2, 200, 2, 1, 3, 1, "hard2", 19.9, "frame"),        # rpw 8 -> 3, h < rpw
    (3, 200, 200, 1, 1, 0, "soft", 20.1, "frame"),      # rpw 5 -> 3
    (4, 200, 5, 3, 1, 0, "hard1", -1.3, "one"),          # rpw 4 -> 3
    (5, 200, 4, 2, 1, 1, "soft", 25.0, "frame"),        # rpw 3, no shrink, 16 % 5 != 0
    (16, 200, 3, 1, 2, 0, "soft", -30.0, "all"),        # C equal to the lines
    (17, 200, 24, 2, 1, 0, "hard2", 0.5413, "frame"),    # one coil in the ragged last chunk
    (33, 200, 200, 1, 1, 1, "soft", -1.3, "frame"),     # three chunks, the last one ragged
    (1, 130, 9, 2, 2, 0, "soft", 0.5413, "frame"),      # generic: rpw 8 -> 7, h % 7 != 0
    (2, 300, 5, 1, 2, 1, "hard1_kref", 19.9, "frame"),   # rpw 4 -> 3
    (3, 20, 1, 3, 2, 0, "soft", 20.1, "one"),           # rpw 2, 8 % 3 != 0, h = 1 < rpw
    (8, 33, 5, 2, 1, 0, "hard2", 25.0, "frame"),        # C equal to the lines, direct engine along w
    (9, 20, 200, 1, 2, 1, "soft", -30.0, "none"),        # ragged last chunk of one coil; h = 200 columns
    (33, 7, 3, 2, 2, 0, "plain", 0.5413, "all"),        # five chunks, the last one ragged
    (32, 432, 2, 1, 1, 0, "soft", 0.5413, "frame"),     # LDS opt-in along w
    (2, 24, 24, 1, 2, 0, "hard1", 0.5413, "none")]]     # every row dropped: exactly zero
# the crossings an axis-by-axis walk does not promise: every lambda in a call that reads lambda_dev, and every mode on every column /
# row kernel (h = 200 or not: col200_kernel or col_pass_kernel; w = 200 or not: the 200-point row kernels or row_pass_kernel)
_B += [dict(C=3, w=20, h=h, b=2, t=2, magnitude=0, mode="soft", lam=lam, mask=mk)
       for h in (200, 7) for lam, mk in zip(LAMBDAS, ("frame", "one", "all", "frame", "one", "frame"))]
_B += [dict(C=C, w=w, h=h, b=1, t=2, magnitude=i % 2, mode=mode, lam=LAMBDAS[i % 6], mask=("frame", "one")[i % 2])
       for i, (mode, h, w, C) in enumerate((m, h, w, C) for m in B_AXES["mode"] for h, w, C in ((200, 200, 2), (200, 20, 9), (7, 200, 5), (7, 20, 3)))]
for _c in _B:
    _c["t"] = cap_samples(_c["t"], _c["b"] * _c["C"] * _c["h"] * _c["w"], 1_500_000)
B_CASES = _B
MASKED_SPLIT_CASE = dict(h=3, w=2, n=SPLIT_BT, inverse=0, alias=False, premask="frame", coils=3)
B_SPLIT_CASES = [dict(entry=e, h=h, w=w) for e, h, w in [("cine_sens_expand_dc", 200, 1), ("cine_sens_expand_dc", 2, 3),
                                                            ("cine_expand_dc_hybrid", 200, 2), ("cine_expand_dc_hybrid", 3, 2)]]


def expand_split_case(s):
    """The group B case of a split case: c = 3, b * t = 10 925, soft DC with a mask per frame and a kref."""
    return dict(C=3, w=s["w"], h=s["h"], b=5, t=SPLIT_BT // 5, magnitude=0, mode="soft", lam=0.5413, mask="frame")


# (b, t, c, h, w, row_lo, row_hi)
PROLOGUE_CASES = [(1, 3, 2, 24, 20, 0, 24), (2, 2, 3, 24, 20, 0, 1), (1, 1, 1, 7, 5, 6, 7), (3, 2, 2, 9, 200, 3, 6), (1, 4, 5, 200, 13, 90, 110),
                  (2, 1, 1, 1, 1, 0, 1), (1, 2, 3, 33, 432, 10, 23)]
# (h, n, unsampled rows)
ACS_CASES = [(24, 24, [2, 5, 8, 15, 20]), (25, 25, [0, 11, 13, 24]), (24, 24, []), (24, 24, [3, 7]), (24, 24, [12, 20]), (24, 30, [3, 7, 26]),
             (25, 40, [11, 12]), (1, 1, []), (2, 2, [0, 1]), (200, 200, list(range(0, 90, 3)) + list(range(111, 200, 4))), (300, 512, [7, 290])]
EW_LENGTHS = [1, 3, 4, 5, 1023, 70_001]
# (bt, c, h, w, mask kind)
APPLY_MASK_CASES = [(1, 1, 1, 1, "all"), (2, 1, 3, 1, "frame"), (3, 2, 2, 2, "frame"), (2, 3, 5, 1, "one"), (2, 2, 24, 20, "none"), (5, 3, 7, 23, "frame"),
                    (2, 3, 200, 67, "frame")]
RSS_CASES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 8, 24, 20), (1, 33, 9, 200)]

# ---- group C
C200_AXES = dict(c=[1, 5, 6, 10, 11, 16, 21, 26, 31, 35], w=[1, 3, 5, 7, 12, 41], b=[1, 2], t=[1, 2, 3], form=["lam", "cine", "xpd", "rand"],
                 zf=[False, True], magnitude=[0, 1], lam=LAMBDAS, mask=MASKS)
CGEN_AXES = dict(C200_AXES, h=[2, 24, 77, 397, 432, 512], c=[1, 3, 8, 9], w=[1, 8, 9, 20])
C_CASES = [dict(c, h=200) for c in sweep(31, C200_AXES, 20)] + sweep(37, CGEN_AXES, 12)
# the crossings: {form} x {zf} on both kernels, and every lambda in the lambda_dev form on both kernels
C_CASES += [dict(c=c, w=w, b=2, t=2, form=f, zf=zf, magnitude=i % 2, lam=LAMBDAS[i % 6], mask="frame", h=h)
            for i, (h, c, w, f, zf) in enumerate((h, c, w, f, zf) for h, c, w in ((200, 7, 7), (77, 3, 9)) for f in C200_AXES["form"] for zf in (False, True))]
C_CASES += [dict(c=c, w=w, b=1, t=2, form="lam", zf=bool(i % 2), magnitude=0, lam=lam, mask=("frame", "one")[i % 2], h=h)
            for h, c, w in ((200, 11, 3), (24, 2, 20)) for i, lam in enumerate(LAMBDAS)]
for _c in C_CASES:
    _c["t"] = cap_samples(_c["t"], _c["b"] * _c["c"] * _c["h"] * _c["w"], 400_000)
SGRAD_CASES = [dict(b=b, t=t, c=c, h=h, w=w, form=f, lam=lam, mask=mk) for b, t, c, h, w, f, lam, mk in [
    (1, 2, 3, 200, 5, "lam", 0.5413, "frame"), (2, 1, 6, 200, 9, "rand", 0.0, "frame"), (1, 1, 2, 200, 1, "cine", 0.0, "one"),
    (2, 2, 3, 24, 20, "lam", 20.1, "frame"), (1, 2, 2, 77, 13, "rand", 0.0, "frame"), (1, 1, 1, 432, 3, "lam", -1.3, "all"),
    (1, 3, 4, 7, 8, "xpd", 0.0, "one")]]
ACCUM_CASES = [(1, 1, 1, 1, 1), (2, 3, 2, 5, 7), (1, 4, 9, 24, 20), (3, 2, 33, 3, 200)]


def weights_of(c):
    """(lam or None, (w_sampled, w_unsampled, beta)) of a group C case."""
    if c["form"] == "lam":
        return c["lam"], (0.0, 0.0, 0.0)
    if c["form"] == "cine":
        return None, (1.0, 0.0, 0.0)
    if c["form"] == "xpd":
        return None, (1.0, 0.0, -1.0)
    rs = np.random.RandomState(hash_case(c) % (2 ** 31))
    return None, tuple(float(np.float32(x)) for x in rs.uniform(-1.5, 1.5, 3))


def c_expects_zero(c):
    return c["mask"] == "none" and (c["form"] == "cine" or (c["form"] == "xpd" and not c["zf"]))


# ================================================================== inputs and references per case (CPU; shared by the GPU tests)
def t2_data(c, seed):
    bt, co, h, w = c["n"], c["coils"], c["h"], c["w"]
    k = _rand(seed, bt, co, h, w, 2)
    mask = make_mask(seed + 1, bt, h, c["premask"])
    return k, mask


def b_data(c, seed):
    """Group B inputs: k-space, maps, image, kref (NaN on the rows the mask drops; all NaN where the call ignores it), mask."""
    b, t, C, h, w = c["b"], c["t"], c["C"], c["h"], c["w"]
    k = _rand(seed, b, t, C, h, w, 2)
    S = _rand(seed + 1, b, C, h, w, 2)
    img = _rand(seed + 2, b, t, h, w, 2)
    mask = make_mask(seed + 3, b * t, h, c["mask"]).view(b, t, h)
    kref = _rand(seed + 4, b, t, C, h, w, 2)
    kref[(mask == 0)[:, :, None, :, None, None].expand_as(kref)] = NAN
    if c["mode"] == "hard1_kref":
        kref[:] = NAN
    return k, S, img, kref, mask


def b_expand_ref(c, S, img, kref, mask):
    mode = c["mode"]
    hard = {"plain": 0, "soft": 0, "hard1": 1, "hard1_kref": 1, "hard2": 2}[mode]
    use_kref = mode in ("soft", "hard2")
    return ref_blend(ref_sens_expand(cplx(img), cplx(S)), cplx(kref) if use_kref else None, mask, c["lam"], hard), hard


def c_data(c, seed):
    b, t, C, h, w = c["b"], c["t"], c["c"], c["h"], c["w"]
    img = _rand(seed, b, t, h, w, 2)
    S = _rand(seed + 1, b, C, h, w, 2)
    mask = make_mask(seed + 2, b * t, h, c["mask"]).view(b, t, h)
    lam, wts = weights_of(c)
    kref = zf = None
    if c["zf"]:
        if lam is not None:                 # zf = sens_reduce(mask * kref), the float32 tensor the caller would hold
            kref = cplx(_rand(seed + 3, b, t, C, h, w, 2))
            zf = pairs(ref_sens_reduce(torch.where(_rows(mask), kref, torch.zeros_like(kref)), cplx(S))).float()
        else:
            zf = _rand(seed + 3, b, t, h, w, 2)
    ref = ref_image_dc(cplx(img), cplx(S), mask, lam=lam, kref=kref, weights=wts, zf=None if zf is None else cplx(zf))
    return img, S, mask, zf, lam, wts, ref


# ================================================================== CPU tests: the references and the case lists
def test_reference_transforms_match_the_oracle():
    from oracle import centered_fft as cf
    for seed, shape in ((1, (2, 5, 7)), (2, (3, 4, 15)), (3, (2, 24, 20)), (4, (1, 397, 33)), (5, (2, 200, 9))):
        x = rnd(seed, *shape, 2)
        z = cplx(x)
        assert rel_err(pairs(ref_fftc(z, (-1,))), cf.fft1c(x)) < PIN
        assert rel_err(pairs(ref_fftc(z, (-1,), inverse=True)), cf.ifft1c(x)) < PIN
        assert rel_err(pairs(ref_fftc(z, (-2, -1))), cf.fft2c(x)) < PIN
        assert rel_err(pairs(ref_fftc(z, (-2, -1), inverse=True)), cf.ifft2c(x)) < PIN
        assert rel_err(pairs(ref_fftc(z, (-1,), variant=1)), torch.view_as_real(cf.xpd_temporal_fft(torch.view_as_complex(x), -1))) < PIN
        assert rel_err(pairs(ref_fftc(z, (-1,), inverse=True, variant=1)),
                       torch.view_as_real(cf.xpd_temporal_ifft(torch.view_as_complex(x), -1))) < PIN
        assert rel_err(pairs(ref_to_hybrid(z)), cf.ifft1c(x.transpose(-2, -3)).transpose(-2, -3)) < PIN
    odd = cplx(rnd(6, 4, 15, 2))            # the two shift orders differ for odd n, forward only
    assert rel_err(pairs(ref_fftc(odd, (-1,), variant=1)), pairs(ref_fftc(odd, (-1,)))) > 0.1
    even = cplx(rnd(7, 4, 16, 2))
    assert rel_err(pairs(ref_fftc(even, (-1,), variant=1)), pairs(ref_fftc(even, (-1,)))) < 1e-12


def test_reference_transforms_match_the_recorded_outputs():
    g = load_golden("ops")
    for tag in ("odd", "t15", "even", "mixed"):
        z = cplx(torch.from_numpy(g[tag + "_x"]))
        assert rel_err(pairs(ref_fftc(z, (-1,))), g[tag + "_fft1c"]) < PIN, tag
        assert rel_err(pairs(ref_fftc(z, (-1,), inverse=True)), g[tag + "_ifft1c"]) < PIN, tag
        assert rel_err(pairs(ref_fftc(z, (-2, -1))), g[tag + "_fft2c"]) < PIN, tag
        assert rel_err(pairs(ref_fftc(z, (-2, -1), inverse=True)), g[tag + "_ifft2c"]) < PIN, tag
    z = cplx(rnd(int(g["full200_seed"]), 2, 200, 200, 2))
    assert rel_err(pairs(ref_fftc(z, (-2, -1))), g["full200_fft2c"]) < PIN
    assert rel_err(pairs(ref_fftc(z, (-2, -1), inverse=True)), g["full200_ifft2c"]) < PIN
    g = load_golden("fft_smooth")
    for tag in ("a96x120", "a192x160", "a256x320", "a384x512", "a45x250", "a400x405"):
        n, h, w = (int(v) for v in g[tag + "_shape"])
        sh, sw = (int(v) for v in g[tag + "_stride"])
        z = cplx(rnd(int(g[tag + "_seed"]), n, h, w, 2))
        assert rel_err(pairs(ref_fftc(z, (-2, -1)))[:, ::sh, ::sw], g[tag + "_fft2c"]) < PIN, tag
        assert rel_err(pairs(ref_fftc(z, (-2, -1), inverse=True))[:, ::sh, ::sw], g[tag + "_ifft2c"]) < PIN, tag
    for n in (30, 128, 360, 512):
        z = cplx(rnd(int(g[f"l{n}_seed"]), 3, n, 2))
        assert rel_err(pairs(ref_fftc(z, (-1,))), g[f"l{n}_fft1c"]) < PIN, n
        assert rel_err(pairs(ref_fftc(z, (-1,), inverse=True)), g[f"l{n}_ifft1c"]) < PIN, n


def test_reference_coil_operators_match_the_oracle_and_the_recorded_block():
    from oracle import varnet_ref as V
    g = load_golden("varnet_block")
    k, kref, sens = (torch.from_numpy(g[n]) for n in ("k", "kref", "sens"))
    mask = torch.from_numpy(g["mask"])
    S, m3 = cplx(sens[:, 0]), mask.view(1, 5, 24)
    red = ref_sens_reduce(cplx(k), S)
    assert rel_err(pairs(red), g["XF_reduce"][:, :, 0]) < PIN
    img32 = torch.from_numpy(g["XF_reduce"])
    assert rel_err(pairs(ref_sens_expand(cplx(img32[:, :, 0]), S)), g["XF_expand"]) < PIN
    assert rel_err(pairs(red), V.VarNetBlock.sens_reduce(k, sens)[:, :, 0]) < PIN
    assert rel_err(pairs(ref_sens_expand(cplx(img32[:, :, 0]), S)), V.VarNetBlock.sens_expand(img32, sens)) < PIN
    # the soft data consistency of VarNetBlock.forward (:108) on the same operands, and the composition group C is compared with
    for lam in (0.5413, -1.3, 20.1):
        v = F.softplus(torch.tensor([lam]))
        kth = V.VarNetBlock.sens_expand(img32, sens)
        want = (1 - mask) * kth + mask * (kth + v * kref) / (1 + v)
        got = ref_blend(ref_sens_expand(cplx(img32[:, :, 0]), S), cplx(kref), m3, lam, 0)
        assert rel_err(pairs(got), want) < PIN, lam
        assert rel_err(pairs(ref_image_dc(cplx(img32[:, :, 0]), S, m3, lam=lam, kref=cplx(kref))), V.VarNetBlock.sens_reduce(want, sens)[:, :, 0]) < PIN
    kth = ref_sens_expand(cplx(img32[:, :, 0]), S)
    m5 = mask.view(1, 5, 1, 24, 1).bool()
    assert torch.equal(ref_blend(kth, None, m3, 0.0, 1), kth * m5)
    assert torch.equal(ref_blend(kth, cplx(kref), m3, 0.0, 2), (kth - cplx(kref)) * m5)
    poisoned = kref.clone()
    poisoned[(mask == 0).expand_as(kref)] = NAN
    assert torch.equal(ref_blend(kth, cplx(poisoned), m3, 0.5, 0), ref_blend(kth, cplx(kref), m3, 0.5, 0))


def test_reference_sens_grad_is_the_headers_closed_form():
    """Autograd of the composition against conj(g) T(S m) + T(S g) conj(m), T = IFFT_h W FFT_h (include/cine_hip.h)."""
    b, t, c, h, w = 2, 2, 3, 7, 5
    img, g, S = cplx(rnd(1, b, t, h, w, 2)), cplx(rnd(2, b, t, h, w, 2)), cplx(rnd(3, b, c, h, w, 2))
    mask = make_mask(4, b * t, h, "frame").view(b, t, h)
    for lam, wts in ((0.5413, None), (None, (0.75, -0.5, 0.0))):
        w1, w0 = (1 / (1 + ref_softplus(lam)), 1.0) if lam is not None else wts[:2]
        W = torch.where(_rows(mask), torch.tensor(w1, dtype=torch.float64), torch.tensor(w0, dtype=torch.float64))
        T = lambda x: ref_fftc(W * ref_fftc(x, (-2,)), (-2,), inverse=True)           # noqa: E731
        want = g.conj()[:, :, None] * T(S[:, None] * img[:, :, None]) + T(S[:, None] * g[:, :, None]) * img.conj()[:, :, None]
        assert rel_err(pairs(ref_image_dc_sens_grad(img, g, S, mask, lam=lam, weights=wts)), pairs(want)) < 1e-12


def test_reference_acs_window_matches_the_oracle():
    from oracle.varnet_ref import SensitivityModel
    for h, n, zeros in ACS_CASES:
        rows = np.ones(n, np.float32)
        rows[zeros] = 0
        below, above = [z for z in zeros if z < h // 2], [z for z in zeros if h // 2 <= z < h]
        got = ref_acs_window(rows, h)
        if below and above:                 # the oracle on the first h entries (all the entry point reads)
            pad, n_low = SensitivityModel.acs_window(torch.from_numpy(rows[:h].copy()).view(1, 1, 1, h, 1, 1))
            assert got == [pad, pad + n_low], (h, zeros)
        else:
            assert got == [0, h]
    kinds = {(bool([z for z in zs if z < h // 2]), bool([z for z in zs if h // 2 <= z < h]), h % 2, n > h) for h, n, zs in ACS_CASES}
    assert {k[:2] for k in kinds} == {(True, True), (False, False), (True, False), (False, True)}
    assert {k[2] for k in kinds} == {0, 1} and {k[3] for k in kinds} == {False, True}


def test_restated_length_rules():
    assert len(SUPPORTED) == 407 and sum(smooth(n) for n in SUPPORTED) == 67 and sum(engine(n) == "direct" for n in SUPPORTED) == 340
    assert [n for n in SUPPORTED if n > 400] == [405, 432, 450, 480, 486, 500, 512]
    assert not line_supported(0) and not line_supported(-1) and not line_supported(401) and not line_supported(540) and line_supported(1)
    assert [n for n in SUPPORTED if lds_opt_in(n)] == [432, 450, 480, 486, 500, 512]
    for n in SUPPORTED:
        per = 32 if n == 200 else 8
        assert fft1c_nlines(n)[0] == 1 and fft1c_nlines(n)[1] % per != 0 and fft1c_nlines(n)[1] > per
    assert coil_tiling(1, 200) == (3, 1, True) and coil_tiling(4, 200) == (3, 4, True) and coil_tiling(5, 200) == (3, 5, False)
    assert coil_tiling(1, 130) == (7, 1, True) and coil_tiling(1, 128) == (8, 1, False) and coil_tiling(33, 20) == (1, 8, False)
    assert image_dc_ws_bytes(2, 3, 5, 200, 7) == 0 and image_dc_ws_bytes(2, 3, 6, 200, 7) == 2 * 2 * 3 * 200 * 7 * 8
    assert split_step(3) == 32766 and SPLIT_BT * 3 > 32766 and SPLIT_NIMG > SPLIT


def test_transform_cases_reach_every_engine_and_edge():
    for name, vals in T2_AXES.items():
        if name != "n":                                                                        # (the batch count is capped by the plane size)
            assert {c[name] for c in T2_CASES} >= set(vals), name
    for axis in ("h", "w"):
        got = {c[axis] for c in T2_CASES}
        assert {200, 1, 2} <= got and {405, 432, 450, 480, 486, 500, 512} <= got               # every smooth length above 400 (LDS opt-in from 432)
        assert {397, 399, 203} <= got                                                          # direct: a prime and two composites
        assert {n for n in got if smooth(n) and n <= 400 and n != 200}
    assert any(c["h"] == 200 and c["w"] % 16 for c in T2_CASES) and any(c["h"] == 200 and c["w"] == 1 for c in T2_CASES)
    assert any(c["h"] != 200 and c["w"] % 8 for c in T2_CASES) and any(c["h"] != 200 and c["w"] == 1 for c in T2_CASES)
    assert {(engine(c["h"]), engine(c["w"])) for c in T2_CASES} >= {(a, b) for a in ("200", "smooth", "direct") for b in ("200", "smooth", "direct")}
    assert {(c["premask"], c["h"] == 200) for c in T2_CASES} >= {(m, f) for m in MASKS for f in (False, True)} - {("none", True)}
    for c in T2_CASES:
        k, mask = t2_data(c, hash_case(c))
        if c["premask"] == "frame" and c["n"] > 1 and c["h"] > 2:
            assert not torch.equal(mask[0], mask[1]), c


def test_coil_cases_reach_every_tiling():
    for name, vals in B_AXES.items():
        if name != "t":
            assert {c[name] for c in B_CASES} >= set(vals), name
    assert {c["t"] for c in B_CASES} >= {1, 2}
    for f200 in (False, True):
        lines = 16 if f200 else 8
        cs = [c for c in B_CASES if (c["w"] == 200) == f200]
        tl = [(c, *coil_tiling(c["C"], c["w"])) for c in cs]
        assert any(c["C"] < lines and lines % c["C"] == 0 for c in cs) and any(c["C"] < lines and lines % c["C"] for c in cs)
        assert any(c["C"] == lines for c in cs)
        assert any(c["C"] > lines and c["C"] % lines for c in cs), "ragged last coil chunk"
        assert any(c["C"] > lines and c["C"] % lines == 1 for c in cs) and any(c["C"] > 2 * lines for c in cs)
        assert any(sh for _, _, _, sh in tl) and any(not sh and rpw > 1 for _, rpw, _, sh in tl)
        assert any(rpw > 1 and c["h"] % rpw and c["h"] > rpw for c, rpw, _, _ in tl), "h % rpw != 0"
        assert any(c["h"] < rpw for c, rpw, _, _ in tl), "h < rpw"
        assert any(c["b"] > 1 for c in cs) and any(c["h"] == 1 for c in B_CASES)
    assert {c["C"] for c in B_CASES if c["w"] == 200 and coil_tiling(c["C"], 200)[2]} == {1, 2, 3, 4}
    for c in B_CASES:
        assert c["b"] * c["t"] <= MAX_BT and line_supported(c["h"]) and line_supported(c["w"])
    assert any(lds_opt_in(c["w"]) for c in B_CASES) and any(c["h"] == 200 and c["mode"] == "soft" for c in B_CASES)
    assert any(c["mode"] == "hard1" and c["mask"] == "none" for c in B_CASES)
    # crossings: a value only counts where the call uses it
    for h200 in (False, True):
        soft = [c for c in B_CASES if c["mode"] == "soft" and (c["h"] == 200) == h200 and c["mask"] != "none"]
        assert {c["lam"] for c in soft} == set(LAMBDAS), "every lambda in a soft DC that blends at least one row"
        for w200 in (False, True):
            assert {c["mode"] for c in B_CASES if (c["h"] == 200) == h200 and (c["w"] == 200) == w200} == set(B_AXES["mode"]), (h200, w200)
    assert {(c["mode"], c["mask"]) for c in B_CASES if c["mode"] != "plain"} >= {(m, k) for m in ("soft", "hard1", "hard2") for k in MASKS}
    for h, n, zeros in ACS_CASES:
        assert n >= h and all(z < n for z in zeros)
    for b, t, c, h, w, lo, hi in PROLOGUE_CASES:
        assert 0 <= lo < hi <= h
    assert any(lo == 0 for *_, lo, hi in PROLOGUE_CASES) and any(hi == h for *_, h, w, lo, hi in PROLOGUE_CASES)
    assert any(hi - lo == 1 for *_, lo, hi in PROLOGUE_CASES)


def test_image_space_cases_reach_every_route():
    for name, vals in C200_AXES.items():
        if name != "t":
            assert {c[name] for c in C_CASES if c["h"] == 200} >= set(vals), name
    for name in ("h", "c", "w"):
        assert {c[name] for c in C_CASES if c["h"] != 200} >= set(CGEN_AXES[name]), name
    c200 = [c for c in C_CASES if c["h"] == 200]
    assert {-(-c["c"] // 5) for c in c200} == set(range(1, 8))
    assert any(image_dc_ws_bytes(c["b"], c["t"], c["c"], 200, c["w"]) == 0 for c in c200)
    assert any(c["w"] % 5 for c in c200) and any(c["w"] == 1 for c in c200) and any(c["b"] > 1 for c in c200)
    assert any((-(-c["w"] // 5) * -(-c["c"] // 5)) % 8 for c in c200), "grid rounded up to 8s"
    gen = {engine(c["h"]) for c in C_CASES if c["h"] != 200}
    assert gen == {"smooth", "direct"} and any(lds_opt_in(c["h"]) for c in C_CASES)
    for h200 in (False, True):
        cs = [c for c in C_CASES if (c["h"] == 200) == h200]
        assert {(c["form"], c["zf"]) for c in cs} == {(f, z) for f in C200_AXES["form"] for z in (False, True)}, h200
        assert {c["lam"] for c in cs if c["form"] == "lam" and c["mask"] != "none"} == set(LAMBDAS), h200
        assert {c["magnitude"] for c in cs} == {0, 1} and {c["mask"] for c in cs} == set(MASKS)
    assert {c["h"] == 200 for c in SGRAD_CASES} == {False, True} and any(c["w"] % 8 for c in SGRAD_CASES)
    assert {c["form"] == "lam" for c in SGRAD_CASES} == {False, True}


def test_references_are_well_conditioned():
    """peak > 0 for the reference of every case (so max |d| / peak is a relative error), except the hard mask that drops every row,
    whose expected output is exactly zero."""
    for c in T2_CASES:
        k, mask = t2_data(c, hash_case(c))
        assert float(ref_fftc(cplx(k), (-2, -1)).abs().max()) > 0
        kept = torch.where(mask.bool()[:, None, :, None], cplx(k), torch.zeros_like(cplx(k)))
        assert float(ref_to_hybrid(kept).abs().max()) > 0 or c["premask"] == "none"
    for c in B_CASES:
        k, S, img, kref, mask = b_data(c, hash_case(c))
        assert float(ref_sens_reduce(cplx(k), cplx(S)).abs().max()) > 0
        ref, hard = b_expand_ref(c, S, img, kref, mask)
        assert not torch.isnan(pairs(ref)).any(), c
        if hard and c["mask"] == "none":
            assert float(ref.abs().max()) == 0
        else:
            assert float(ref.abs().max()) > 0
    for c in C_CASES:
        ref = c_data(c, hash_case(c))[-1]
        assert not torch.isnan(pairs(ref)).any(), c
        if c_expects_zero(c):               # weights (1, 0, .) are a hard mask: with every row dropped and no zf term the output is 0
            assert float(ref.abs().max()) == 0, c
        else:
            assert float(ref.abs().max()) > 0, c


def test_split_cases_cross_the_batch_split_with_another_mask():
    """The frames behind the split must not carry the masks of the first frames, or a lost mask offset would go unseen: checked on the
    masks the split cases themselves use."""
    first = split_step(3) // 3
    assert SPLIT_BT * 3 > split_step(3) and first < SPLIT_BT
    masks = [t2_data(MASKED_SPLIT_CASE, hash_case(MASKED_SPLIT_CASE))[1]]
    masks += [b_data(c, hash_case(c))[4].view(SPLIT_BT, c["h"]) for c in map(expand_split_case, B_SPLIT_CASES)]
    assert len(masks) == 5
    for m in masks:
        assert m.shape[0] == SPLIT_BT and not torch.equal(m[first:], m[:SPLIT_BT - first])


# ================================================================== GPU harness
gpu = pytest.mark.gpu
WORST = Worst()     # entry point -> (worst error / bar, case)
_record = WORST.record


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


ALIGNED, BOTH = (0,), (0, 2)


# ================================================================== A: plain transforms
@gpu
@pytest.mark.parametrize("n", SUPPORTED)
def test_fft1c_every_length(dev, n):
    """cine_fft1c at every supported length: forward / inverse, both shift variants, one line and a ragged last workgroup, in place;
    every fifth length also 8 bytes past a 16-byte boundary."""
    L = _L()
    for nl in fft1c_nlines(n):
        x = _rand(1000 + n, nl, n, 2)
        for inverse in (0, 1):
            for variant in (0, 1):
                ref = pairs(ref_fftc(cplx(x), (-1,), bool(inverse), variant))
                assert float(ref.abs().max()) > 0

                def body(k):
                    xi, o = k.inp(x), k.out(x.shape)
                    _check(L.cine_fft1c(xi.data_ptr(), o.ptr(), nl, n, inverse, variant, _stream()), "cine_fft1c")
                    return [o.t]

                def in_place(k):
                    o = k.out(x.shape, x)
                    _check(L.cine_fft1c(o.ptr(), o.ptr(), nl, n, inverse, variant, _stream()), "cine_fft1c")
                    return [o.t]
                got, = _at_offsets(dev, BOTH if n % 5 == 0 or n == 397 else ALIGNED, body, "cine_fft1c")
                _record(f"cine_fft1c ({engine(n)})", rel_err(got, ref), BAR, dict(n=n, nlines=nl, inverse=inverse, variant=variant))
                same, = _twice(dev, 0, in_place, "cine_fft1c in place")
                assert same_bits(same, got), (n, nl, inverse, variant)


@gpu
def test_fft_line_supported_is_the_restated_predicate(dev):
    L = _L()
    for n in range(-1, 601):
        assert L.cine_fft_line_supported(n) == int(line_supported(n)), n


def _run_fft2c(dev, c, offs):
    L, h, w = _L(), c["h"], c["w"]
    x = t2_data(c, hash_case(c))[0].view(-1, h, w, 2)
    nimg = x.shape[0]
    ref = pairs(ref_fftc(cplx(x), (-2, -1), bool(c["inverse"])))

    def body(k):
        if c["alias"]:
            o = k.out(x.shape, x)
            src = o.t
        else:
            src, o = k.inp(x), k.out(x.shape)
        _check(L.cine_fft2c(src.data_ptr(), o.ptr(), nimg, h, w, c["inverse"], _stream()), "cine_fft2c")
        return [o.t]
    got, = _at_offsets(dev, offs, body, "cine_fft2c")
    _record("cine_fft2c", rel_err(got, ref), BAR, c)


def _run_to_hybrid(dev, c, offs):
    L, h, w = _L(), c["h"], c["w"]
    x = t2_data(c, hash_case(c))[0].view(-1, h, w, 2)
    ref = pairs(ref_to_hybrid(cplx(x)))

    def body(k):
        if c["alias"]:
            o = k.out(x.shape, x)
            src = o.t
        else:
            src, o = k.inp(x), k.out(x.shape)
        _check(L.cine_kspace_to_hybrid(src.data_ptr(), o.ptr(), x.shape[0], h, w, _stream()), "cine_kspace_to_hybrid")
        return [o.t]
    got, = _at_offsets(dev, offs, body, "cine_kspace_to_hybrid")
    _record("cine_kspace_to_hybrid", rel_err(got, ref), BAR, c)


def _run_masked_to_hybrid(dev, c, offs):
    """The rows the mask drops hold NaN: the kernel must not read them."""
    L, h, w, bt, co = _L(), c["h"], c["w"], c["n"], c["coils"]
    x, mask = t2_data(c, hash_case(c))
    keep = mask.bool()[:, None, :, None]
    ref = pairs(ref_to_hybrid(torch.where(keep, cplx(x), torch.zeros_like(cplx(x)))))
    xn = x.clone()
    xn[~keep[..., None].expand_as(xn)] = NAN

    def body(k):
        src, md, o = k.inp(xn), k.raw(mask), k.out(x.shape)
        _check(L.cine_masked_kspace_to_hybrid(src.data_ptr(), md.data_ptr(), o.ptr(), bt, co, h, w, _stream()), "cine_masked_kspace_to_hybrid")
        return [o.t]
    got, = _at_offsets(dev, offs, body, "cine_masked_kspace_to_hybrid")
    assert float(ref.abs().max()) > 0 or c["premask"] == "none"
    _record("cine_masked_kspace_to_hybrid", rel_err(got, ref), BAR, c)


@gpu
@pytest.mark.parametrize("c", T2_CASES, ids=case_id)
def test_fft2c_sweep(dev, c):
    _run_fft2c(dev, c, ALIGNED)


@gpu
@pytest.mark.parametrize("c", T2_CASES, ids=case_id)
def test_kspace_to_hybrid_sweep(dev, c):
    _run_to_hybrid(dev, c, ALIGNED)


@gpu
@pytest.mark.parametrize("c", T2_CASES, ids=case_id)
def test_masked_kspace_to_hybrid_sweep(dev, c):
    _run_masked_to_hybrid(dev, c, ALIGNED)


@gpu
@pytest.mark.parametrize("c", T2_CASES[::4], ids=case_id)
def test_plain_transforms_8_bytes_past_a_16_byte_boundary(dev, c):
    _run_fft2c(dev, c, BOTH)
    _run_to_hybrid(dev, c, BOTH)
    _run_masked_to_hybrid(dev, c, BOTH)


@gpu
@pytest.mark.parametrize("entry", ["cine_fft2c", "cine_kspace_to_hybrid", "cine_masked_kspace_to_hybrid"])
def test_plain_transforms_across_the_batch_split(dev, entry):
    """Tiny images, a batch just over the 32 768 images of one column-pass launch; the masked form with c = 3 and a mask per frame,
    so that the mask offset of the second chunk matters."""
    if entry == "cine_masked_kspace_to_hybrid":
        _run_masked_to_hybrid(dev, MASKED_SPLIT_CASE, ALIGNED)
    else:
        c = dict(h=2, w=3, n=SPLIT_NIMG, inverse=0, alias=entry == "cine_fft2c", premask="all", coils=1)
        (_run_fft2c if entry == "cine_fft2c" else _run_to_hybrid)(dev, c, ALIGNED)


# ================================================================== B: coil operators
def _run_reduce(dev, c, offs):
    """cine_sens_reduce (tmp == k and tmp != k: the same image), cine_hybrid_reduce on the float32 hybrid-space tensor, cine_zero_filled_rss."""
    L = _L()
    b, t, C, h, w, mag = c["b"], c["t"], c["C"], c["h"], c["w"], c["magnitude"]
    k, S = b_data(c, hash_case(c))[:2]
    kz, Sz = cplx(k), cplx(S)
    oshape = (b, t, h, w) if mag else (b, t, h, w, 2)
    shaped = (lambda z: z.abs()) if mag else pairs
    route = dict(c, tiling=coil_tiling(C, w))

    def reduce_body(alias):
        def body(kk):
            Sd, o = kk.inp(S), kk.out(oshape)
            tmp = kk.out(k.shape, k if alias else None)
            kd = tmp.t if alias else kk.inp(k)
            _check(L.cine_sens_reduce(kd.data_ptr(), Sd.data_ptr(), o.ptr(), tmp.ptr(), b, t, C, h, w, mag, _stream()), "cine_sens_reduce")
            return [o.t]
        return body
    got, = _at_offsets(dev, offs, reduce_body(False), "cine_sens_reduce")
    ref = shaped(ref_sens_reduce(kz, Sz))
    assert float(ref.abs().max()) > 0
    _record("cine_sens_reduce", rel_err(got, ref), BAR, route)
    got2, = _twice(dev, offs[-1], reduce_body(True), "cine_sens_reduce (tmp == k)")
    assert same_bits(got, got2), c

    hyb = pairs(ref_to_hybrid(kz)).float()

    def hyb_body(kk):
        hd, Sd, o = kk.inp(hyb), kk.inp(S), kk.out(oshape)
        _check(L.cine_hybrid_reduce(hd.data_ptr(), Sd.data_ptr(), o.ptr(), b, t, C, h, w, mag, _stream()), "cine_hybrid_reduce")
        return [o.t]
    got, = _at_offsets(dev, offs, hyb_body, "cine_hybrid_reduce")
    ref = shaped((Sz.conj()[:, None] * ref_fftc(cplx(hyb), (-1,), inverse=True)).sum(2))
    _record("cine_hybrid_reduce", rel_err(got, ref), BAR, route)

    def rss_body(alias):
        def body(kk):
            o = kk.out((b, t, h, w))
            tmp = kk.out(k.shape, k if alias else None)
            kd = tmp.t if alias else kk.inp(k)
            _check(L.cine_zero_filled_rss(kd.data_ptr(), o.ptr(), tmp.ptr(), b, t, C, h, w, _stream()), "cine_zero_filled_rss")
            return [o.t]
        return body
    got, = _at_offsets(dev, offs, rss_body(False), "cine_zero_filled_rss")
    ref = ref_fftc(kz, (-2, -1), inverse=True).abs().pow(2).sum(2).sqrt()
    _record("cine_zero_filled_rss", rel_err(got, ref), BAR, route)
    got2, = _twice(dev, offs[-1], rss_body(True), "cine_zero_filled_rss (tmp == k)")
    assert same_bits(got, got2), c


def _run_expand(dev, c, offs, entries=("cine_sens_expand_dc", "cine_expand_dc_hybrid")):
    """cine_sens_expand_dc and cine_expand_dc_hybrid in the case's mode.  kref holds NaN on the rows the mask drops (everywhere in
    mode hard1_kref, where the header says it is ignored)."""
    L = _L()
    b, t, C, h, w, mode = c["b"], c["t"], c["C"], c["h"], c["w"], c["mode"]
    k, S, img, kref, mask = b_data(c, hash_case(c))
    ref, hard = b_expand_ref(c, S, img, kref, mask)
    route = dict(c, tiling=coil_tiling(C, w))
    for entry in entries:
        fn = getattr(L, entry)

        def body(kk):
            imgd, Sd = kk.inp(img), kk.inp(S)
            krefd = kk.inp(kref) if mode in ("soft", "hard2", "hard1_kref") else None
            md = None if mode == "plain" else kk.raw(mask.view(b * t, h))
            lamd = kk.lam(c["lam"]) if mode == "soft" else None
            o = kk.out(k.shape)
            _check(fn(imgd.data_ptr(), Sd.data_ptr(), _p(krefd), _p(md), _p(lamd), o.ptr(), b, t, C, h, w, hard, _stream()), entry)
            return [o.t]
        got, = _at_offsets(dev, offs, body, entry)
        want = pairs(ref if entry == "cine_sens_expand_dc" else ref_to_hybrid(ref))
        zero = bool(hard) and c["mask"] == "none"
        assert (float(want.abs().max()) == 0) if zero else (float(want.abs().max()) > 0)
        _record(f"{entry} ({mode})", rel_err(got, want), BAR, route)
        if hard and entry == "cine_sens_expand_dc":
            dropped = (mask == 0)[:, :, None, :, None, None].expand_as(got)
            assert bool((got[dropped] == 0).all()), f"{entry}: a row the hard mask drops is not exactly zero {c}"


@gpu
@pytest.mark.parametrize("c", B_CASES, ids=case_id)
def test_coil_reduce_sweep(dev, c):
    _run_reduce(dev, c, ALIGNED)


@gpu
@pytest.mark.parametrize("c", B_CASES, ids=case_id)
def test_expand_dc_sweep(dev, c):
    _run_expand(dev, c, ALIGNED)


@gpu
@pytest.mark.parametrize("c", B_CASES[::5], ids=case_id)
def test_coil_operators_8_bytes_past_a_16_byte_boundary(dev, c):
    _run_reduce(dev, c, BOTH)
    _run_expand(dev, c, BOTH)


@gpu
@pytest.mark.parametrize("s", B_SPLIT_CASES, ids=case_id)
def test_expand_dc_across_the_batch_split(dev, s):
    """c = 3 and b * t = 10 925: the second column-pass chunk starts at frame 10 922 and must take that frame's mask and kref."""
    c = expand_split_case(s)
    assert c["b"] * c["t"] == SPLIT_BT
    _run_expand(dev, c, ALIGNED, entries=(s["entry"],))


@gpu
@pytest.mark.parametrize("case", PROLOGUE_CASES, ids=str)
def test_sens_prologue(dev, case):
    """cine_sens_prologue with windows at the edges; the device-window form gives the same bits."""
    L = _L()
    b, t, c, h, w, lo, hi = case
    k = _rand(hash(case) % 1000 + 5, b, t, c, h, w, 2)
    mean = cplx(k).mean(1)
    rows = torch.zeros(h, dtype=torch.bool)
    rows[lo:hi] = True
    ref = pairs(ref_fftc(torch.where(rows[:, None], mean, torch.zeros_like(mean)), (-2, -1), inverse=True))
    assert float(ref.abs().max()) > 0

    def host(kk):
        kd, o = kk.inp(k), kk.out((b, c, h, w, 2))
        _check(L.cine_sens_prologue(kd.data_ptr(), o.ptr(), b, t, c, h, w, lo, hi, _stream()), "cine_sens_prologue")
        return [o.t]

    def device(kk):
        kd, o, win = kk.inp(k), kk.out((b, c, h, w, 2)), kk.raw(torch.tensor([lo, hi], dtype=torch.int32))
        _check(L.cine_sens_prologue_win(kd.data_ptr(), o.ptr(), b, t, c, h, w, win.data_ptr(), _stream()), "cine_sens_prologue_win")
        return [o.t]
    got, = _at_offsets(dev, BOTH, host, "cine_sens_prologue")
    _record("cine_sens_prologue", rel_err(got, ref), BAR, case)
    got2, = _at_offsets(dev, BOTH, device, "cine_sens_prologue_win")
    assert same_bits(got, got2), case


@gpu
@pytest.mark.parametrize("case", ACS_CASES, ids=lambda c: f"h{c[0]}-n{c[1]}-{len(c[2])}")
def test_acs_window(dev, case):
    L = _L()
    h, n, zeros = case
    rows = np.ones(n, np.float32)
    rows[zeros] = 0
    for _ in range(2):
        k = Call(dev, 0)
        rd, win = k.raw(torch.from_numpy(rows)), GuardedInt(2, dev)
        _check(L.cine_acs_window(rd.data_ptr(), n, h, win.ptr(), _stream()), "cine_acs_window")
        k.finish("cine_acs_window")
        assert win.intact() and win.t.cpu().tolist() == ref_acs_window(rows, h), case


@gpu
@pytest.mark.parametrize("case", RSS_CASES, ids=str)
def test_rss_normalise(dev, case):
    L = _L()
    b, c, h, w = case
    x = _rand(sum(case), b, c, h, w, 2)
    z = cplx(x)
    ref = pairs(z / z.abs().pow(2).sum(1, keepdim=True).sqrt())

    def body(kk):
        o = kk.out(x.shape, x)
        _check(L.cine_rss_normalise(o.ptr(), b, c, h, w, _stream()), "cine_rss_normalise")
        return [o.t]
    got, = _at_offsets(dev, BOTH, body, "cine_rss_normalise")
    _record("cine_rss_normalise", rel_err(got, ref), BAR, case)


@gpu
@pytest.mark.parametrize("case", APPLY_MASK_CASES, ids=str)
def test_apply_mask(dev, case):
    """kspace * mask + 0.0, out of place and in place: one exact product per component, kept rows bit-unchanged, dropped rows +0."""
    L = _L()
    bt, c, h, w, kind = case
    k = _rand(bt * 7 + h, bt, c, h, w, 2)
    mask = make_mask(bt + h, bt, h, kind)
    want = k * mask[:, None, :, None, None].float() + 0.0

    def body(alias):
        def run(kk):
            md = kk.raw(mask)
            o = kk.out(k.shape, k if alias else None)
            src = o.t if alias else kk.inp(k)
            _check(L.cine_apply_mask(src.data_ptr(), md.data_ptr(), o.ptr(), bt, c, h, w, _stream()), "cine_apply_mask")
            return [o.t]
        return run
    for alias in (False, True):
        got, = _at_offsets(dev, BOTH, body(alias), "cine_apply_mask")
        assert same_bits(got, want), (case, alias)
    WORST.record("cine_apply_mask", 0.0, BAR, case)


@gpu
@pytest.mark.parametrize("n", EW_LENGTHS)
def test_scale(dev, n):
    L = _L()
    x = _rand(n, n)
    s = 0.7071067690849304          # a float32 value

    def body(kk):
        o = kk.out((n,), x)
        _check(L.cine_scale(o.ptr(), n, s, _stream()), "cine_scale")
        return [o.t]
    for offs in ((0, 2), (1, 3)):       # plain floats: any 4-byte alignment
        got, = _at_offsets(dev, offs, body, "cine_scale")
        _record("cine_scale", rel_err(got, x.double() * s), BAR, n)


# ================================================================== C: image-space operators
def _run_image_dc(dev, c, offs):
    """cine_image_dc against the composition; at h = 200 cine_sens_tile_pack against its layout and cine_image_dc_t for the same bits."""
    L = _L()
    b, t, C, h, w, mag = c["b"], c["t"], c["c"], c["h"], c["w"], c["magnitude"]
    img, S, mask, zf, lam, wts, ref = c_data(c, hash_case(c))
    nb = L.cine_image_dc_ws_bytes(b, t, C, h, w)
    assert nb == image_dc_ws_bytes(b, t, C, h, w), c
    ntile = L.cine_sens_tile_floats(b, C, h, w)
    assert ntile == (b * C * -(-w // 5) * 200 * 5 * 2 if h == 200 else 0)
    oshape = (b, t, h, w) if mag else (b, t, h, w, 2)
    route = dict(c, nz=-(-C // 5) if h == 200 else 0, ws=nb)

    def body(tiled):
        def run(kk):
            imgd, Sd, zfd, md, lamd = kk.inp(img), kk.inp(S), kk.inp(zf), kk.raw(mask), kk.lam(lam)
            o, ws = kk.out(oshape), kk.ws(nb)
            if tiled:
                St = kk.out((ntile,))
                _check(L.cine_sens_tile_pack(Sd.data_ptr(), St.ptr(), b, C, h, w, _stream()), "cine_sens_tile_pack")
                _check(L.cine_image_dc_t(imgd.data_ptr(), Sd.data_ptr(), St.ptr(), _p(zfd), md.data_ptr(), _p(lamd), *wts, o.ptr(), b, t, C, h, w,
                                         mag, ws.ptr() if ws else None, nb, _stream()), "cine_image_dc_t")
                return [o.t, St.t]
            _check(L.cine_image_dc(imgd.data_ptr(), Sd.data_ptr(), _p(zfd), md.data_ptr(), _p(lamd), *wts, o.ptr(), b, t, C, h, w, mag,
                                   ws.ptr() if ws else None, nb, _stream()), "cine_image_dc")
            return [o.t]
        return run
    got, = _at_offsets(dev, offs, body(False), "cine_image_dc")
    want = ref.abs() if mag else pairs(ref)
    assert (float(want.abs().max()) == 0) if c_expects_zero(c) else (float(want.abs().max()) > 0)
    _record(f"cine_image_dc ({'200' if h == 200 else 'generic'})", rel_err(got, want), BAR, route)
    if h == 200:
        got_t, St = _at_offsets(dev, offs, body(True), "cine_image_dc_t")
        assert same_bits(got_t, got), c
        assert same_bits(St, ref_tile_pack(S).reshape(-1)), c


def _run_normal_op(dev, c, offs):
    """cine_normal_op, its tiled form (the same bits) and, where the shape has a partial-sum kernel, cine_normal_op_pd: the sum of its 256
    partials against the float64 <img, out> of its own out."""
    L = _L()
    b, t, C, h, w, lam = c["b"], c["t"], c["c"], c["h"], c["w"], c["lam"]
    img, S, mask = c_data(c, hash_case(c))[:3]
    nb = L.cine_image_dc_ws_bytes(b, t, C, h, w)
    ref = pairs(ref_normal_op(cplx(img), cplx(S), mask, lam))
    assert float(ref.abs().max()) > 0

    def body(kind):
        def run(kk):
            imgd, Sd, md, lamd = kk.inp(img), kk.inp(S), kk.raw(mask), kk.lam(lam)
            o, ws = kk.out(img.shape), kk.ws(nb)
            wsp = ws.ptr() if ws else None
            if kind == "tiled":
                St = kk.out((L.cine_sens_tile_floats(b, C, h, w),))
                _check(L.cine_sens_tile_pack(Sd.data_ptr(), St.ptr(), b, C, h, w, _stream()), "cine_sens_tile_pack")
                _check(L.cine_normal_op_t(imgd.data_ptr(), Sd.data_ptr(), St.ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), b, t, C, h, w,
                                          wsp, nb, _stream()), "cine_normal_op_t")
            elif kind == "pd":
                pd = kk.out((256,))
                _check(L.cine_normal_op_pd(imgd.data_ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), pd.ptr(), b, t, C, h, w,
                                           wsp, nb, _stream()), "cine_normal_op_pd")
                return [o.t, pd.t]
            else:
                _check(L.cine_normal_op(imgd.data_ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), b, t, C, h, w, wsp, nb,
                                        _stream()), "cine_normal_op")
            return [o.t]
        return run
    got, = _at_offsets(dev, offs, body("plain"), "cine_normal_op")
    _record(f"cine_normal_op ({'200' if h == 200 else 'generic'})", rel_err(got, ref), BAR, c)
    if h == 200:
        got_t, = _at_offsets(dev, offs, body("tiled"), "cine_normal_op_t")
        assert same_bits(got_t, got), c
    if nb:
        got_pd, pd = _at_offsets(dev, offs, body("pd"), "cine_normal_op_pd")
        _record("cine_normal_op_pd (out)", rel_err(got_pd, ref), BAR, c)
        dot = float((img.double() * got_pd.double()).sum())
        _record("cine_normal_op_pd (p.d)", rel_err(pd.double().sum(), dot), BAR, c)


@gpu
@pytest.mark.parametrize("c", C_CASES, ids=case_id)
def test_image_dc_sweep(dev, c):
    _run_image_dc(dev, c, ALIGNED)


@gpu
@pytest.mark.parametrize("c", C_CASES, ids=case_id)
def test_normal_op_sweep(dev, c):
    _run_normal_op(dev, c, ALIGNED)


@gpu
@pytest.mark.parametrize("c", C_CASES[::4], ids=case_id)
def test_image_space_operators_8_bytes_past_a_16_byte_boundary(dev, c):
    _run_image_dc(dev, c, BOTH)
    _run_normal_op(dev, c, BOTH)


@gpu
def test_normal_op_pd_is_refused_without_a_partial_sum_kernel(dev):
    L = _L()
    for b, t, C, h, w in ((1, 2, 5, 200, 7), (1, 2, 8, 24, 20)):
        k = Call(dev, 0)
        img, S, mask = _rand(1, b, t, h, w, 2), _rand(2, b, C, h, w, 2), make_mask(3, b * t, h, "frame")
        imgd, Sd, md, lamd, o, pd = k.inp(img), k.inp(S), k.raw(mask), k.lam(0.5), k.out(img.shape), k.out((256,))
        _refused(lambda: L.cine_normal_op_pd(imgd.data_ptr(), Sd.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), pd.ptr(), b, t, C, h, w, None, 0,
                                     _stream()), EUNSUPPORTED, k, "cine_normal_op_pd")


@gpu
@pytest.mark.parametrize("c", SGRAD_CASES, ids=case_id)
def test_image_dc_sens_grad(dev, c):
    """cine_image_dc_sens_grad against float64 autograd of the composition, per frame, then cine_coil_accum(NULL, part) over the frames."""
    L = _L()
    b, t, C, h, w = c["b"], c["t"], c["c"], c["h"], c["w"]
    seed = hash_case(c)
    img, g, S = _rand(seed, b, t, h, w, 2), _rand(seed + 1, b, t, h, w, 2), _rand(seed + 2, b, C, h, w, 2)
    mask = make_mask(seed + 3, b * t, h, c["mask"]).view(b, t, h)
    lam, wts = weights_of(c)
    ref = ref_image_dc_sens_grad(cplx(img), cplx(g), cplx(S), mask, lam=lam, weights=wts)
    assert float(ref.abs().max()) > 0

    def body(kk):
        imgd, gd, Sd, md, lamd = kk.inp(img), kk.inp(g), kk.inp(S), kk.raw(mask), kk.lam(lam)
        part, gs = kk.out((b, t, C, h, w, 2)), kk.out((b, C, h, w, 2))
        _check(L.cine_image_dc_sens_grad(imgd.data_ptr(), gd.data_ptr(), Sd.data_ptr(), md.data_ptr(), _p(lamd), wts[0], wts[1], part.ptr(),
                                         b, t, C, h, w, _stream()), "cine_image_dc_sens_grad")
        _check(L.cine_coil_accum(None, part.ptr(), gs.ptr(), b, t, C, h, w, 0, _stream()), "cine_coil_accum")
        return [part.t, gs.t]
    part, gs = _at_offsets(dev, BOTH, body, "cine_image_dc_sens_grad")
    _record(f"cine_image_dc_sens_grad ({'200' if h == 200 else 'generic'})", rel_err(part, pairs(ref)), BAR, c)
    _record("cine_coil_accum (frames of the map gradient)", rel_err(gs, pairs(ref.sum(1))), BAR, c)


@gpu
@pytest.mark.parametrize("with_g", [False, True])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", ACCUM_CASES, ids=str)
def test_coil_accum(dev, case, accumulate, with_g):
    """gs (+)= sum_t conj(g) z against a complex128 einsum: overwrite over a NaN prefill, accumulate onto a prefill at the output's scale."""
    L = _L()
    b, t, c, h, w = case
    z, g = _rand(sum(case), b, t, c, h, w, 2), _rand(sum(case) + 1, b, t, h, w, 2)
    ref = pairs(torch.einsum("bthw,btchw->bchw", cplx(g).conj(), cplx(z)) if with_g else cplx(z).sum(1))
    pre = _rand(sum(case) + 2, b, c, h, w, 2) * float(ref.abs().max())

    def body(kk):
        zd, gd = kk.inp(z), kk.inp(g) if with_g else None
        gs = kk.out(pre.shape, pre if accumulate else None)
        _check(L.cine_coil_accum(_p(gd), zd.data_ptr(), gs.ptr(), b, t, c, h, w, accumulate, _stream()), "cine_coil_accum")
        return [gs.t]
    got, = _at_offsets(dev, BOTH, body, "cine_coil_accum")
    _record("cine_coil_accum", rel_err(got.double() - (pre.double() if accumulate else 0), ref), BAR, (case, accumulate, with_g))


# ================================================================== refusals: decided on the host, before any launch
@gpu
def test_transform_refusals(dev):
    L, st = _L(), _stream()
    for n, want in ((401, EUNSUPPORTED), (540, EUNSUPPORTED), (0, EINVAL)):
        m = max(n, 1)
        k = Call(dev, 0)
        x, o = k.inp(_rand(1, 2, m, 2)), k.out((2, m, 2))
        _refused(lambda: L.cine_fft1c(x.data_ptr(), o.ptr(), 2, n, 0, 0, st), want, k, f"cine_fft1c n={n}")
        k = Call(dev, 0)
        x, o = k.inp(_rand(1, 1, m, 3, 2)), k.out((1, m, 3, 2))
        _refused(lambda: L.cine_fft2c(x.data_ptr(), o.ptr(), 1, n, 3, 0, st), want, k, f"cine_fft2c h={n}")
        _refused(lambda: L.cine_kspace_to_hybrid(x.data_ptr(), o.ptr(), 1, n, 3, st), want, k, f"cine_kspace_to_hybrid h={n}")
        md = k.raw(torch.ones(1, m, dtype=torch.uint8))
        _refused(lambda: L.cine_masked_kspace_to_hybrid(x.data_ptr(), md.data_ptr(), o.ptr(), 1, 1, n, 3, st), want, k, f"cine_masked_kspace_to_hybrid h={n}")
        k = Call(dev, 0)
        x, o = k.inp(_rand(1, 1, 3, m, 2)), k.out((1, 3, m, 2))
        _refused(lambda: L.cine_fft2c(x.data_ptr(), o.ptr(), 1, 3, n, 1, st), want, k, f"cine_fft2c w={n}")
    k = Call(dev, 0)
    x, o, md = k.inp(_rand(1, 2, 8, 2)), k.out((2, 8, 2)), k.raw(torch.ones(2, 8, dtype=torch.uint8))
    _refused(lambda: L.cine_fft1c(x.data_ptr(), o.ptr(), 2, 8, 0, 2, st), EINVAL, k, "cine_fft1c variant=2")
    _refused(lambda: L.cine_fft1c(None, o.ptr(), 2, 8, 0, 0, st), EINVAL, k, "cine_fft1c in=NULL")
    _refused(lambda: L.cine_fft1c(x.data_ptr(), None, 2, 8, 0, 0, st), EINVAL, k, "cine_fft1c out=NULL")
    _refused(lambda: L.cine_fft2c(None, o.ptr(), 2, 8, 1, 0, st), EINVAL, k, "cine_fft2c in=NULL")
    _refused(lambda: L.cine_kspace_to_hybrid(x.data_ptr(), None, 2, 8, 1, st), EINVAL, k, "cine_kspace_to_hybrid hyb=NULL")
    _refused(lambda: L.cine_masked_kspace_to_hybrid(x.data_ptr(), None, o.ptr(), 2, 1, 8, 1, st), EINVAL, k, "cine_masked_kspace_to_hybrid mask=NULL")
    _refused(lambda: L.cine_acs_window(x.data_ptr(), 8, 9, md.data_ptr(), st), EINVAL, k, "cine_acs_window n < h")


@gpu
def test_coil_operator_refusals(dev):
    L, st = _L(), _stream()
    for n in (401, 540):                        # an unsupported width, everything else valid: nothing may be written, tmp included
        b, t, C, h = 1, 2, 2, 3
        k = Call(dev, 0)
        kd, S, img, o, tmp = k.inp(_rand(1, b, t, C, h, n, 2)), k.inp(_rand(2, b, C, h, n, 2)), k.inp(_rand(3, b, t, h, n, 2)), k.out((b, t, h, n, 2)), k.out((b, t, C, h, n, 2))
        _refused(lambda: L.cine_sens_reduce(kd.data_ptr(), S.data_ptr(), o.ptr(), tmp.ptr(), b, t, C, h, n, 0, st), EUNSUPPORTED, k, f"cine_sens_reduce w={n}")
        _refused(lambda: L.cine_hybrid_reduce(kd.data_ptr(), S.data_ptr(), o.ptr(), b, t, C, h, n, 0, st), EUNSUPPORTED, k, f"cine_hybrid_reduce w={n}")
        _refused(lambda: L.cine_zero_filled_rss(kd.data_ptr(), o.ptr(), tmp.ptr(), b, t, C, h, n, st), EUNSUPPORTED, k, f"cine_zero_filled_rss w={n}")
        _refused(lambda: L.cine_sens_expand_dc(img.data_ptr(), S.data_ptr(), None, None, None, tmp.ptr(), b, t, C, h, n, 0, st), EUNSUPPORTED, k, f"cine_sens_expand_dc w={n}")
        _refused(lambda: L.cine_expand_dc_hybrid(img.data_ptr(), S.data_ptr(), None, None, None, tmp.ptr(), b, t, C, h, n, 0, st), EUNSUPPORTED, k, f"cine_expand_dc_hybrid w={n}")
        o2 = k.out((b, C, h, n, 2))
        _refused(lambda: L.cine_sens_prologue(kd.data_ptr(), o2.ptr(), b, t, C, h, n, 0, h, st), EUNSUPPORTED, k, f"cine_sens_prologue w={n}")
        k = Call(dev, 0)                        # the same along h
        kd, S, o, tmp = k.inp(_rand(1, b, t, C, n, 3, 2)), k.inp(_rand(2, b, C, n, 3, 2)), k.out((b, t, n, 3, 2)), k.out((b, t, C, n, 3, 2))
        _refused(lambda: L.cine_sens_reduce(kd.data_ptr(), S.data_ptr(), o.ptr(), tmp.ptr(), b, t, C, n, 3, 0, st), EUNSUPPORTED, k, f"cine_sens_reduce h={n}")
        _refused(lambda: L.cine_zero_filled_rss(kd.data_ptr(), o.ptr(), tmp.ptr(), b, t, C, n, 3, st), EUNSUPPORTED, k, f"cine_zero_filled_rss h={n}")
        o2 = k.out((b, C, n, 3, 2))
        _refused(lambda: L.cine_sens_prologue(kd.data_ptr(), o2.ptr(), b, t, C, n, 3, 0, n, st), EUNSUPPORTED, k, f"cine_sens_prologue h={n}")
    # b * t = 65 536 frames of one pixel and one coil: every buffer has its full size
    b, t = 2, 32768
    k = Call(dev, 0)
    kd, S, o, tmp = k.inp(_rand(1, b, t, 1, 1, 1, 2)), k.inp(_rand(2, b, 1, 1, 1, 2)), k.out((b, t, 1, 1, 2)), k.out((b, t, 1, 1, 1, 2))
    md, lamd = k.raw(torch.ones(b * t, 1, dtype=torch.uint8)), k.lam(0.5)
    img = kd.view(b, t, 1, 1, 2)
    _refused(lambda: L.cine_sens_reduce(kd.data_ptr(), S.data_ptr(), o.ptr(), tmp.ptr(), b, t, 1, 1, 1, 0, st), EUNSUPPORTED, k, "cine_sens_reduce b*t=65536")
    _refused(lambda: L.cine_hybrid_reduce(kd.data_ptr(), S.data_ptr(), o.ptr(), b, t, 1, 1, 1, 0, st), EUNSUPPORTED, k, "cine_hybrid_reduce b*t=65536")
    _refused(lambda: L.cine_zero_filled_rss(kd.data_ptr(), o.ptr(), tmp.ptr(), b, t, 1, 1, 1, st), EUNSUPPORTED, k, "cine_zero_filled_rss b*t=65536")
    _refused(lambda: L.cine_sens_expand_dc(img.data_ptr(), S.data_ptr(), kd.data_ptr(), md.data_ptr(), lamd.data_ptr(), tmp.ptr(), b, t, 1, 1, 1, 0, st),
             EUNSUPPORTED, k, "cine_sens_expand_dc b*t=65536")
    _refused(lambda: L.cine_expand_dc_hybrid(img.data_ptr(), S.data_ptr(), kd.data_ptr(), md.data_ptr(), lamd.data_ptr(), tmp.ptr(), b, t, 1, 1, 1, 0, st),
             EUNSUPPORTED, k, "cine_expand_dc_hybrid b*t=65536")
    _refused(lambda: L.cine_image_dc(img.data_ptr(), S.data_ptr(), None, md.data_ptr(), lamd.data_ptr(), 0.0, 0.0, 0.0, o.ptr(), b, t, 1, 1, 1, 0, None, 0, st),
             EUNSUPPORTED, k, "cine_image_dc b*t=65536")
    _refused(lambda: L.cine_image_dc_sens_grad(img.data_ptr(), img.data_ptr(), S.data_ptr(), md.data_ptr(), lamd.data_ptr(), 0.0, 0.0, tmp.ptr(), b, t, 1, 1, 1, st),
             EINVAL, k, "cine_image_dc_sens_grad b*t=65536")
    _refused(lambda: L.cine_apply_mask(kd.data_ptr(), md.data_ptr(), tmp.ptr(), b * t, 1, 1, 1, st), EINVAL, k, "cine_apply_mask bt*c=65536")
    # the modes of the data-consistency step
    b, t, C, h, w = 1, 2, 2, 4, 3
    k = Call(dev, 0)
    img, S, kref, o = k.inp(_rand(1, b, t, h, w, 2)), k.inp(_rand(2, b, C, h, w, 2)), k.inp(_rand(3, b, t, C, h, w, 2)), k.out((b, t, C, h, w, 2))
    md, lamd = k.raw(make_mask(1, b * t, h, "frame")), k.lam(0.5)
    args = (b, t, C, h, w)
    for name in ("cine_sens_expand_dc", "cine_expand_dc_hybrid"):
        entry = getattr(L, name)
        _refused(lambda: entry(img.data_ptr(), S.data_ptr(), None, md.data_ptr(), lamd.data_ptr(), o.ptr(), *args, 2, st), EINVAL, k, f"{name} hard_mask=2 without kref")
        _refused(lambda: entry(img.data_ptr(), S.data_ptr(), kref.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), *args, 3, st), EINVAL, k, f"{name} hard_mask=3")
        _refused(lambda: entry(img.data_ptr(), S.data_ptr(), None, None, None, o.ptr(), *args, 1, st), EINVAL, k, f"{name} hard_mask=1 without mask")
        _refused(lambda: entry(img.data_ptr(), S.data_ptr(), kref.data_ptr(), md.data_ptr(), None, o.ptr(), *args, 0, st), EINVAL, k, f"{name} soft DC without lambda")
        _refused(lambda: entry(None, S.data_ptr(), None, None, None, o.ptr(), *args, 0, st), EINVAL, k, f"{name} img=NULL")
        _refused(lambda: entry(img.data_ptr(), S.data_ptr(), None, None, None, None, *args, 0, st), EINVAL, k, f"{name} out=NULL")
        _refused(lambda: entry(img.data_ptr(), S.data_ptr(), None, None, None, o.ptr(), b, 0, C, h, w, 0, st), EINVAL, k, f"{name} t=0")
    _refused(lambda: L.cine_sens_reduce(kref.data_ptr(), None, o.ptr(), o.ptr(), *args, 0, st), EINVAL, k, "cine_sens_reduce sens=NULL")
    _refused(lambda: L.cine_coil_accum(None, None, o.ptr(), *args, 0, st), EINVAL, k, "cine_coil_accum z=NULL")


@gpu
def test_image_space_refusals(dev):
    L, st = _L(), _stream()
    b, t, C, h, w = 1, 2, 7, 200, 3
    nb = L.cine_image_dc_ws_bytes(b, t, C, h, w)
    assert nb > 0
    k = Call(dev, 0)
    img, S, o = k.inp(_rand(1, b, t, h, w, 2)), k.inp(_rand(2, b, C, h, w, 2)), k.out((b, t, h, w, 2))
    md, lamd, ws = k.raw(make_mask(1, b * t, h, "frame")), k.lam(0.5), k.ws(nb)

    def dc(imgp, outp, wsp, nbytes, lam=lamd.data_ptr(), hh=h):
        return L.cine_image_dc(imgp, S.data_ptr(), None, md.data_ptr(), lam, 0.0, 0.0, 0.0, outp, b, t, C, hh, w, 0, wsp, nbytes, st)
    _refused(lambda: dc(img.data_ptr(), o.ptr(), ws.ptr(), nb - 1), EWORKSPACE, k, "cine_image_dc workspace one byte short")
    _refused(lambda: dc(img.data_ptr(), o.ptr(), None, nb), EWORKSPACE, k, "cine_image_dc ws=NULL")
    _refused(lambda: dc(o.ptr(), o.ptr(), ws.ptr(), nb), EINVAL, k, "cine_image_dc img == out")
    _refused(lambda: dc(None, o.ptr(), ws.ptr(), nb), EINVAL, k, "cine_image_dc img=NULL")
    _refused(lambda: L.cine_normal_op(img.data_ptr(), S.data_ptr(), md.data_ptr(), None, o.ptr(), b, t, C, h, w, ws.ptr(), nb, st), EINVAL, k, "cine_normal_op lambda=NULL")
    _refused(lambda: L.cine_normal_op_pd(img.data_ptr(), S.data_ptr(), md.data_ptr(), lamd.data_ptr(), o.ptr(), None, b, t, C, h, w, ws.ptr(), nb, st), EINVAL, k,
             "cine_normal_op_pd pd_part=NULL")
    _refused(lambda: L.cine_image_dc_sens_grad(img.data_ptr(), None, S.data_ptr(), md.data_ptr(), lamd.data_ptr(), 0.0, 0.0, o.ptr(), b, t, C, h, w, st), EINVAL, k,
             "cine_image_dc_sens_grad gout=NULL")
    for n in (401, 540):
        k = Call(dev, 0)
        img, S, o, part = k.inp(_rand(1, 1, 1, n, 2, 2)), k.inp(_rand(2, 1, 2, n, 2, 2)), k.out((1, 1, n, 2, 2)), k.out((1, 1, 2, n, 2, 2))
        md, lamd = k.raw(torch.ones(1, n, dtype=torch.uint8)), k.lam(0.5)
        _refused(lambda: L.cine_image_dc(img.data_ptr(), S.data_ptr(), None, md.data_ptr(), lamd.data_ptr(), 0.0, 0.0, 0.0, o.ptr(), 1, 1, 2, n, 2, 0, None, 0, st),
                 EUNSUPPORTED, k, f"cine_image_dc h={n}")
        _refused(lambda: L.cine_image_dc_sens_grad(img.data_ptr(), img.data_ptr(), S.data_ptr(), md.data_ptr(), lamd.data_ptr(), 0.0, 0.0, part.ptr(), 1, 1, 2, n, 2, st),
                 EUNSUPPORTED, k, f"cine_image_dc_sens_grad h={n}")
    k = Call(dev, 0)
    S, o = k.inp(_rand(2, 1, 2, 24, 5, 2)), k.out((1, 2, 24, 5, 2))
    _refused(lambda: L.cine_sens_tile_pack(S.data_ptr(), o.ptr(), 1, 2, 24, 5, st), EUNSUPPORTED, k, "cine_sens_tile_pack h != 200")
    assert L.cine_sens_tile_floats(1, 2, 24, 5) == 0 and L.cine_image_dc_ws_bytes(1, 1, 8, 24, 5) == 0
