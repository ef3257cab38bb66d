"""The calibration and front-end entry points of include/cine_hip.h (csrc/frontend_kernels.hip) called one by one through the C ABI,
shape by shape, against float64 references on the CPU, and the calibration composed on the shapes no other test runs.

Entry points
  E  cine_espirit_eig: the three instances espirit_eig_kernel<8>, <16>, <32> (1..8, 9..16, 17..32 coils) on matrices with a known spectrum
  K  cine_espirit_lag_kernels: alone, and through cine_fft2c(kpad, inverse) as the per-pixel operator the header promises
  G  cine_gauss_axis
  C  cine_crop_select
  T  cine_combine_target
  composed: frontend.espirit_maps ("eigh" and "sign") against oracle.frontend_ref.espirit_maps on non-square, odd and 32-coil shapes

References: every operation restated in float64 numpy below; inputs are the float32 values the kernel sees, widened.  Unmarked CPU tests
hold the restatements to 1e-10 against oracle/frontend_ref.py: the image-space operator on a small odd, non-square phantom (the matrix
the oracle diagonalises, caught at its call of numpy.linalg.eigh; its float32 results through the eigenpairs) and the Gaussian pass; the
crop bit for bit; the target to the one float32 rounding of the oracle's result.

E.  m = s_p Q_p diag(lam) Q_p^H per pixel, Q_p the QR factor of a seeded complex Gaussian, lam = (1, 0.5 u_2, ..., 0.5 u_c), u uniform in
(0, 1), s_p uniform in (0.3, 1.2), 60 iterations.  The reference is numpy.linalg.eigh of the float32-rounded matrix in complex128: top
eigenpair, coil 0 real and non-negative, zero where lam < crop; lam is compared at every pixel.  Where row and column 0 of M vanish the
eigenvector has no coil-0 component and the kernel hands out the iterate unrotated: the reference there is u (u^H 1) / |u^H 1| (u from
the eigh of the remaining block), which for M = 0 is the zero vector with lam = 0.  Cases of at least 63 pixels carry one pixel of each
kind (ZERO_PIXEL, NOCOIL0_PIXEL).  A CPU test asserts the conditions on the draw: start overlap |u^H 1| / sqrt(c) >= 1e-3 and
|lam - crop| >= 1e-4 at every pixel with M != 0 (at M = 0 both sides of any crop give the same zeros), and with crop = 0.8 at least a
quarter of the pixels on each side wherever there are 63 pixels or more.  The bar is kernel_sweep.BAR on max |lam - lam_ref| / peak lam
and on max |v - v_ref| (unit vectors); what licenses it is the textbook power iteration in numpy float32 on the same inputs, held to
BAR / 2 on the CPU for every (c, npix).

K.  proj -> kpad is linear: proj is any seeded complex64 matrix.  BAR against the peak of the reference (at most 36 float32 terms);
everything outside the (2 kk - 1)^2 window is +0.0 bit for bit.  The identity: with proj = V V^H (V seeded, orthonormal),
cine_fft2c(kpad, inverse) is M(r) = g^H g / kk^2 of oracle/frontend_ref.py:118-123, evaluated here from the projector's float32 values.

G.  scipy.ndimage.gaussian_filter1d (reflect, truncate 4) on the widened parts; bar 2^-22 of the reference's peak: at most 33 float64
terms rounded once to float32.  C.  bits of the slice.  T.  BAR against the peak; torch's float32 result is held to BAR / 2 on the CPU.

Every GPU case checks: the error; every float pointer at storage offsets of 0 and 2 floats (complex operands ask for 8-byte alignment)
with the same bits at both; a second call gives the same bits; a NaN prefill of every output between intact guard floats; inputs
bit-unchanged.  Refusals are decided on the host before any launch and write nothing.  DESIGN.md section 4f has the measured worst
error / bar per entry point, the float32 yardsticks, the seeds and the mutations the sweep was tried against.
"""
import functools

import numpy as np
import pytest
import torch

from kernel_sweep import BAR, EINVAL, EUNSUPPORTED, Call, L, Worst, at_offsets, case_id, check, hash_case, refused, same_bits, stream

PIN = 1e-10                                    # float64 restatement against the float64 oracle
OFFS = (0, 2)                                  # storage offsets in floats: complex operands must be 8-byte aligned (cine_hip.h)
BAR_GAUSS = 2.0 ** -22                         # one float32 rounding of a float64 sum, against the peak


def _pairs(z):
    """complex array -> float32 (..., 2) tensor: the values the kernel sees."""
    z = np.asarray(z)
    return torch.from_numpy(np.stack([z.real, z.imag], axis=-1).astype(np.float32)).contiguous()


def _cplx(t):
    """float32 (..., 2) tensor -> complex128 array: the same values, widened."""
    a = t.detach().cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _crandn(rs, *shape):
    return rs.standard_normal(shape) + 1j * rs.standard_normal(shape)


def _key(c):
    return tuple(sorted(c.items()))


# ================================================================== E: the float64 reference, the draw, the float32 yardstick
E_SEED = 20_253                                # the first of 20251, 20252, ... whose draws meet test_eig_draw_meets_its_conditions
E_COILS = [1, 2, 7, 8, 9, 16, 17, 31, 32]      # both sides of the instance boundaries 8 | 9 and 16 | 17
E_NPIX = [1, 63, 64, 65, 333]                  # the 64-thread tail
E_CROPS = [0.0, 0.8, 2.0]
E_ITERS = 60
ZERO_PIXEL, NOCOIL0_PIXEL, SPECIAL_MIN = 3, 5, 63
E_SHAPES = [dict(c=c, npix=n) for c in E_COILS for n in E_NPIX]
E_CASES = [dict(c=s["c"], npix=s["npix"], crop=crop) for s in E_SHAPES for crop in E_CROPS]


def _spectral(rs, n, s):
    """s Q diag(1, 0.5 u_2, ..., 0.5 u_n) Q^H with Q the QR factor of a complex Gaussian: the second eigenvalue is at most half the first."""
    q = np.linalg.qr(_crandn(rs, n, n))[0]
    lam = np.concatenate([[1.0], 0.5 * rs.uniform(size=n - 1)])
    return s * (q * lam) @ q.conj().T


@functools.lru_cache(maxsize=None)
def _eig_draw(c, npix):
    """(npix, c, c) complex64, exactly Hermitian, and the tensor (c*c, npix, 2) cine_espirit_eig reads (plane (i, j) = row i, column j)."""
    rs = np.random.RandomState(E_SEED + hash_case(dict(c=c, npix=npix)))
    m = np.zeros((npix, c, c), np.complex128)
    scale = rs.uniform(0.3, 1.2, size=npix)
    for p in range(npix):
        if npix >= SPECIAL_MIN and p == ZERO_PIXEL:
            continue
        if npix >= SPECIAL_MIN and p == NOCOIL0_PIXEL and c > 1:
            m[p, 1:, 1:] = _spectral(rs, c - 1, scale[p])
        else:
            m[p] = _spectral(rs, c, scale[p])
    m32 = (0.5 * (m + m.conj().transpose(0, 2, 1))).astype(np.complex64)
    return m32, _pairs(m32.transpose(1, 2, 0).reshape(c * c, npix))


def _top(m):
    """Top eigenpair of the Hermitian (npix, n, n): eigenvalue, unit eigenvector."""
    w, v = np.linalg.eigh(m)
    return w[:, -1], v[:, :, -1]


def ref_eig(m32, crop):
    """cine_espirit_eig at convergence: (maps (c, npix) complex128, lam (npix), overlap (npix)) from eigh of the widened float32 matrix.
    overlap = |u^H 1| / sqrt(c), the start vector's share of the eigenvector (nan where M = 0)."""
    m = m32.astype(np.complex128)
    npix, c, _ = m.shape
    lam, vec = _top(m)
    nocoil0 = ~m[:, 0, :].any(axis=1) & ~m[:, :, 0].any(axis=1)
    zero = ~m.reshape(npix, -1).any(axis=1)
    overlap = np.abs(vec.conj().sum(axis=1)) / np.sqrt(c)
    vec = vec * np.exp(-1j * np.angle(vec[:, :1]))
    for p in np.nonzero(nocoil0 & ~zero)[0]:                       # the iterate unrotated: its phase is the start vector's
        lam[p], u = (a[0] for a in _top(m[p:p + 1, 1:, 1:]))
        dot = u.conj().sum()
        vec[p, 0], vec[p, 1:], overlap[p] = 0.0, u * dot / abs(dot), abs(dot) / np.sqrt(c)
    vec[zero], lam[zero], overlap[zero] = 0.0, 0.0, np.nan
    vec = vec * (lam >= crop)[:, None]
    return vec.T.copy(), lam, overlap


def ref_eig_steps(m32, iters):
    """The power iteration itself in float64, `iters` steps from the uniform vector: (maps, lam) with lam = v^H M v of the vector BEFORE
    the last step (for iters = 1: sum_ij M_ij / c), nothing cropped."""
    return _power(m32.astype(np.complex128), iters, -np.inf)


def _power(m, iters, crop):
    """The textbook power iteration in m's own precision (complex128: a reference, complex64: the float32 yardstick)."""
    npix, c, _ = m.shape
    real = m.real.dtype.type
    v = np.full((npix, c), real(1.0) / np.sqrt(real(c)), m.dtype)
    ev = np.zeros(npix, m.real.dtype)
    for _ in range(iters):
        u = np.einsum("pij,pj->pi", m, v)
        nn = (u.real * u.real + u.imag * u.imag).sum(axis=1)
        ev = (u.real * v.real + u.imag * v.imag).sum(axis=1)
        inv = np.where(nn > 0, real(1.0) / np.sqrt(np.where(nn > 0, nn, real(1.0))), real(0.0))
        v = u * inv[:, None]
    a0 = np.abs(v[:, 0])
    ph = np.where(a0 > 0, v[:, 0].conj() / np.where(a0 > 0, a0, real(1.0)), real(1.0)).astype(m.dtype)
    v = v * ph[:, None] * (ev >= crop)[:, None]
    assert v.dtype == m.dtype and ev.dtype == m.real.dtype
    return v.T.copy(), ev


def eig_errs(maps, lam, ref_maps, ref_lam):
    """(max |lam - lam_ref| / peak lam, max |v - v_ref|); a NaN anywhere gives NaN, which no bar admits."""
    return (float(np.abs(lam - ref_lam).max() / max(float(ref_lam.max()), 1e-30)), float(np.abs(maps - ref_maps).max()))


# ================================================================== K: lag kernels and the operator behind them
K_KK = [1, 2, 3, 6]
K_COILS = [1, 3, 17]
K_BUDGET = 250_000                             # c c ny nx complex values at the most


def _k_shapes(kk):
    n = 2 * kk - 1
    return [(n, n), (n, n + 1), (n + 1, n), (11, 16), (17, 12), (21, 33)]


K_CASES = [dict(kk=kk, c=c, ny=ny, nx=nx) for kk in K_KK for c in K_COILS for ny, nx in _k_shapes(kk)
           if ny >= 2 * kk - 1 and nx >= 2 * kk - 1 and c * c * ny * nx <= K_BUDGET]
# (c, kk, ny, nx): mixed-radix lines (12, 20, 15, 9, 25, 10), direct-DFT lines (11, 7), the 10 x 20 engine (200), both parities
I_CASES = [dict(c=2, kk=3, ny=12, nx=20), dict(c=3, kk=2, ny=15, nx=9), dict(c=2, kk=6, ny=11, nx=25), dict(c=1, kk=1, ny=7, nx=10),
           dict(c=1, kk=2, ny=200, nx=12)]


def ref_lag_kernels(w, c, kk, ny, nx):
    """K[c][d](ly, lx) = scale sum_{p - q = l} conj(W[(p, c), (q, d)]) at (ny // 2 + ly, nx // 2 + lx) of the zero array (c, c, ny, nx),
    scale = sqrt(ny nx) / kk^2; W (kk kk c square) with row / column index (py, px, coil)."""
    w6 = np.asarray(w, np.complex128).reshape(kk, kk, c, kk, kk, c)
    out = np.zeros((c, c, ny, nx), np.complex128)
    scale = np.sqrt(ny * nx) / kk ** 2
    for ly in range(-(kk - 1), kk):
        for lx in range(-(kk - 1), kk):
            acc = np.zeros((c, c), np.complex128)
            for qy in range(max(0, -ly), min(kk, kk - ly)):
                for qx in range(max(0, -lx), min(kk, kk - lx)):
                    acc += w6[qy + ly, qx + lx, :, qy, qx, :].conj()
            out[:, :, ny // 2 + ly, nx // 2 + lx] = scale * acc
    return out


def _modulations(k, n):
    """frontend_ref.py:118-121: a k-space offset p is the modulation exp(-2 pi i p r / n) of the centred image grid."""
    return np.exp(-2j * np.pi * np.outer(np.arange(k), (np.arange(n) - n // 2) / n))


def ref_operator(v, c, kk, ny, nx):
    """frontend_ref.py:115-123 as a function of the kept vectors V (kk kk c, n): g = einsum(kern, ey, ex), M = g^H g / kk^2, (ny, nx, c, c)."""
    kern = np.asarray(v, np.complex128).reshape(kk, kk, c, -1)
    g = np.einsum("pqcn,py,qx->yxcn", kern, _modulations(kk, ny), _modulations(kk, nx))
    return np.einsum("yxcn,yxdn->yxcd", g.conj(), g) / (kk * kk)


def ref_operator_of_projector(w, c, kk, ny, nx):
    """The same M from W = V V^H alone (M is linear in W): M_cd(r) = sum_{p, q} conj(e_p(r)) e_q(r) conj(W[(p, c), (q, d)]) / kk^2.  This
    is what the device can be held to: it sees the projector's float32 values, not V."""
    w6 = np.asarray(w, np.complex128).reshape(kk, kk, c, kk, kk, c).conj()
    ey, ex = _modulations(kk, ny), _modulations(kk, nx)
    return np.einsum("abcdef,ay,bx,dy,ex->yxcf", w6, ey.conj(), ex.conj(), ey, ex) / (kk * kk)


def _orthonormal(seed, n, cols):
    return np.linalg.qr(_crandn(np.random.RandomState(seed), n, cols))[0]


@functools.lru_cache(maxsize=None)
def _identity_ref(key):
    c = dict(key)
    n = c["kk"] * c["kk"] * c["c"]
    v = _orthonormal(hash_case(c), n, max(1, n // 3))
    proj = _pairs(v @ v.conj().T)
    return dict(v=v, proj=proj, m=ref_operator_of_projector(_cplx(proj), c["c"], c["kk"], c["ny"], c["nx"]))


# ================================================================== G, C, T
G_SHAPES = [(1, 1, 1), (3, 2, 5), (2, 5, 1), (1, 40, 7), (4, 33, 3), (2, 200, 2)]          # (outer, n, inner)
G_SIGMAS = [0.3, 0.374, 0.375, 0.7, 1.1, 3.9, 4.1]                                        # radii 1, 1, 2, 3, 4, 16, 16
G_CASES = [dict(outer=o, n=n, inner=i, sigma=s) for (o, n, i) in G_SHAPES for s in G_SIGMAS]
C_CASES = [dict(t_in=t, c=c, hin=hi, win=wi, t_out=to, hout=ho, wout=wo)
           for (t, c, hi, wi, to, ho, wo) in [(3, 2, 9, 8, 2, 4, 5), (1, 1, 5, 5, 1, 5, 5), (4, 3, 30, 28, 3, 21, 17), (2, 1, 7, 6, 2, 1, 1),
                                               (2, 2, 8, 9, 1, 3, 5)]]
T_CASES = [dict(t=t, c=c, h=h, w=w, ch=ch, cw=cw) for (t, c, h, w, ch, cw) in [(2, 1, 6, 7, 6, 7), (3, 5, 9, 8, 4, 5), (1, 34, 12, 10, 7, 3), (2, 15, 21, 17, 20, 16)]]


def gauss_radius(sigma):
    return int(4.0 * sigma + 0.5)


def ref_gauss_axis(z, sigma):
    """One pass along axis 1 of the complex128 (outer, n, inner): scipy's filter on the real and the imaginary part."""
    from scipy.ndimage import gaussian_filter1d
    f = functools.partial(gaussian_filter1d, sigma=sigma, axis=1, mode="reflect", truncate=4.0)
    return f(np.ascontiguousarray(z.real)) + 1j * f(np.ascontiguousarray(z.imag))


def ref_crop_select(x, t_out, hout, wout):
    y0, x0 = (x.shape[2] - hout) // 2, (x.shape[3] - wout) // 2
    return x[:t_out, :, y0:y0 + hout, x0:x0 + wout]


def ref_combine_target(img, sens, ch, cw):
    """| sum_c img conj(sens) | of (t, c, h, w) and (c, h, w), cropped to the centred (ch, cw)."""
    t = np.abs((img * sens.conj()[None]).sum(axis=1))
    y0, x0 = (t.shape[-2] - ch) // 2, (t.shape[-1] - cw) // 2
    return t[:, y0:y0 + ch, x0:x0 + cw]


def _pairs_rand(seed, *shape):
    rs = np.random.RandomState(seed % (2 ** 31))
    return torch.from_numpy(rs.standard_normal(shape + (2,)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _target_ref(key):
    c = dict(key)
    img, sens = _pairs_rand(hash_case(c), c["t"], c["c"], c["h"], c["w"]), _pairs_rand(hash_case(c) + 1, c["c"], c["h"], c["w"])
    return dict(img=img, sens=sens, ref=ref_combine_target(_cplx(img), _cplx(sens), c["ch"], c["cw"]))


# ================================================================== the composed calibration
# (coils, ny, nx, calibration region, kernel): non-square even; an odd extent; 32 coils at the k k c = 1152 limit of the sign projector
COMPOSED = [dict(c=4, ny=40, nx=52, r=16, k=6), dict(c=3, ny=45, nx=36, r=15, k=6), dict(c=32, ny=36, nx=32, r=16, k=6)]
COMPOSED_SEED = 1
INSIDE_MIN, INSIDE_SHARE = 200, 1.0 / 3.0


def _phantom(t, c, ny, nx, seed, center_lines=10):
    """test_frontend.py's phantom on a rectangle: time-averaged k-space (c, ny, nx) complex64 and the object's support."""
    from cine_hip import synth
    ex = synth.make_cine_slice(t, c, ny, nx, accel=4, center_lines=center_lines, seed=seed)
    k = torch.view_as_complex(ex["kspace"][0].contiguous()).numpy()
    tgt = ex["target"][0].numpy().mean(0)
    return k.mean(0), tgt > 0.1 * tgt.max()


@functools.lru_cache(maxsize=None)
def _composed_ref(key):
    from oracle import frontend_ref as F
    c = dict(key)
    kavg, sup = _phantom(5, c["c"], c["ny"], c["nx"], COMPOSED_SEED, center_lines=4)
    maps, lam, lam2 = F.espirit_maps(kavg, r=c["r"], k=c["k"], with_second=True)
    inside = sup & (lam >= 0.9) & (lam2 < 0.9 * lam)               # test_frontend.py::test_espirit_vs_oracle's region, from the oracle alone
    return dict(kavg=kavg, sup=sup, maps=maps, lam=lam, inside=inside)


# ================================================================== CPU tests: the restatements against the oracle
def test_reference_operator_is_the_oracles(monkeypatch):
    """ref_operator (M as a function of V) and ref_operator_of_projector (M as a function of V V^H) against frontend_ref.espirit_maps on a
    small phantom, odd and non-square.  The oracle hands its results out in float32, so the matrix it diagonalises is caught on its way
    into numpy.linalg.eigh (the oracle itself is not touched) and the restatements are held to it at 1e-10, with V recomputed the
    oracle's way; the eigenpairs of the restated M are then the oracle's own to float32."""
    from oracle import frontend_ref as F
    c, ny, nx, r, k = 3, 15, 12, 9, 3
    kavg, _ = _phantom(3, c, ny, nx, 2, center_lines=2)
    seen, eigh = [], np.linalg.eigh
    monkeypatch.setattr(np.linalg, "eigh", lambda a: (seen.append(a), eigh(a))[1])
    maps, lam, lam2 = F.espirit_maps(kavg, r=r, k=k, crop=0.0, with_second=True)
    monkeypatch.undo()
    (m_oracle,) = seen
    y0, x0 = ny // 2 - r // 2, nx // 2 - r // 2
    a = F.calibration_matrix(np.asarray(kavg[:, y0:y0 + r, x0:x0 + r], np.complex128), k)
    _, s, vh = np.linalg.svd(a, full_matrices=False)
    v = vh[s >= 1e-3 * s[0]].conj().T
    assert 0 < v.shape[1] < k * k * c
    m = ref_operator(v, c, k, ny, nx)
    assert m.shape == m_oracle.shape == (ny, nx, c, c) and np.abs(m - m_oracle).max() < PIN
    assert np.abs(ref_operator_of_projector(v @ v.conj().T, c, k, ny, nx) - m_oracle).max() < PIN
    w, vec = np.linalg.eigh(m)
    assert np.abs(w[..., -1] - lam).max() < 1e-6 and np.abs(w[..., -2] - lam2).max() < 1e-6          # float32 results
    vec = vec[..., -1] * np.exp(-1j * np.angle(vec[..., :1, -1]))
    sep = (w[..., -1] - w[..., -2]) > 1e-2
    assert sep.sum() > ny * nx // 2
    assert np.abs(vec.transpose(2, 0, 1) - maps)[:, sep].max() < 1e-6


@pytest.mark.parametrize("c", [c for c in K_CASES if c["c"] <= 3 and c["ny"] * c["nx"] <= 300], ids=case_id)
def test_reference_lag_kernels_transform_to_the_operator(c):
    """The header's identity in float64: ifft2c of ref_lag_kernels(V V^H) is ref_operator(V), on every small K shape (transposed extents
    or (n - 1) // 2 for n // 2 break it on the odd and the non-square ones)."""
    from oracle import frontend_ref as F
    n = c["kk"] * c["kk"] * c["c"]
    v = _orthonormal(hash_case(c), n, max(1, n // 2))
    m = F._ifft2c_np(ref_lag_kernels(v @ v.conj().T, c["c"], c["kk"], c["ny"], c["nx"]))
    assert np.abs(m.transpose(2, 3, 0, 1) - ref_operator(v, c["c"], c["kk"], c["ny"], c["nx"])).max() < PIN


def test_reference_eig_agrees_with_the_float64_iteration():
    """ref_eig (eigh) against the float64 power iteration run to convergence, special pixels included, and the meaning of lam after one
    step: the Rayleigh quotient of the uniform vector."""
    for c in (1, 2, 9):
        m32, _ = _eig_draw(c, 65)
        for crop in E_CROPS:
            maps, lam, _ = ref_eig(m32, crop)
            got, ev = _power(m32.astype(np.complex128), 200, crop)
            assert np.abs(ev - lam).max() < PIN and np.abs(got - maps).max() < 1e-9
        _, ev = ref_eig_steps(m32, 1)
        assert np.abs(ev - m32.astype(np.complex128).sum(axis=(1, 2)).real / c).max() < PIN


@pytest.mark.parametrize("sigma", G_SIGMAS)
def test_reference_gauss_axis_is_the_oracles(sigma):
    from oracle import frontend_ref as F
    assert 2 * gauss_radius(sigma) + 1 == len(F._gauss_weights(sigma)) <= 33
    for outer, n, inner in G_SHAPES:
        z = _cplx(_pairs_rand(n, outer, n, inner))
        want = F.gaussian_filter_axis(np.ascontiguousarray(z.real), sigma, 1) + 1j * F.gaussian_filter_axis(np.ascontiguousarray(z.imag), sigma, 1)
        assert np.abs(ref_gauss_axis(z, sigma) - want).max() < PIN


def test_reference_crop_and_target_are_the_oracles():
    """The crop bit for bit; the target to the one float32 rounding the oracle's result carries (2^-24 of the element)."""
    from oracle import frontend_ref as F
    for c in C_CASES:
        x = _cplx(_pairs_rand(hash_case(c), c["t_in"], c["c"], c["hin"], c["win"]))
        want, _ = F.filtered_crop_center_and_slices(x, (c["hout"], c["wout"]), c["t_out"], (0, 0, 0, 0))
        assert np.array_equal(ref_crop_select(x, c["t_out"], c["hout"], c["wout"]), want)
    for c in T_CASES:
        d = _target_ref(_key(c))
        want = F.combine_target(_cplx(d["img"]), _cplx(d["sens"]), (c["ch"], c["cw"]))
        assert want.shape == d["ref"].shape and np.abs(d["ref"] - want).max() <= 2.0 ** -24 * d["ref"].max()


# ------------------------------------------------------------------ the case lists reach what they are for
def test_case_lists_reach_every_instance_and_edge():
    inst = {c: 8 if c <= 8 else 16 if c <= 16 else 32 for c in E_COILS}
    assert set(inst.values()) == {8, 16, 32} and {8, 9, 16, 17, 32} <= set(E_COILS) and sum(1 for c in E_COILS if c > 16) == 3
    assert {(c["c"], c["npix"], c["crop"]) for c in E_CASES} == {(c, n, cr) for c in E_COILS for n in E_NPIX for cr in E_CROPS}
    assert {n % 64 for n in E_NPIX} >= {0, 1, 63} and max(E_NPIX) > 5 * 64
    # K: every kernel size and coil count; the window touching every edge; odd and even extents mixed on non-square arrays
    assert {c["kk"] for c in K_CASES} == set(K_KK) and {c["c"] for c in K_CASES} == set(K_COILS)
    for kk in K_KK:
        shapes = {(c["ny"], c["nx"]) for c in K_CASES if c["kk"] == kk}
        assert shapes >= set(_k_shapes(kk)), kk
    assert all(c["c"] ** 2 * c["ny"] * c["nx"] <= K_BUDGET for c in K_CASES) and any(c["c"] == 17 and c["kk"] == 6 for c in K_CASES)
    assert {(c["ny"] % 2, c["nx"] % 2) for c in K_CASES if c["ny"] != c["nx"]} >= {(0, 1), (1, 0), (1, 1)}
    assert [c for c in I_CASES if c["ny"] == 200] and {c["ny"] % 2 for c in I_CASES} == {0, 1} == {c["nx"] % 2 for c in I_CASES}
    assert all(L().cine_fft_line_supported(n) == 1 for c in I_CASES for n in (c["ny"], c["nx"]))
    # G: radii either side of the 0.374 | 0.375 step, the 33-tap limit, reflections longer than the axis
    assert [gauss_radius(s) for s in G_SIGMAS] == [1, 1, 2, 3, 4, 16, 16] and gauss_radius(4.2) == 17
    assert any(c["n"] < gauss_radius(c["sigma"]) for c in G_CASES) and any(c["n"] == 1 for c in G_CASES)
    # C, T: an odd difference on one axis only, the identity, one pixel, fewer frames; more coils than a wave has lanes / 2
    odd = {((c["hin"] - c["hout"]) % 2, (c["win"] - c["wout"]) % 2) for c in C_CASES}
    assert odd >= {(1, 0), (0, 1), (0, 0), (1, 1)} and any(c["t_out"] < c["t_in"] for c in C_CASES)
    assert any((c["hin"], c["win"]) == (c["hout"], c["wout"]) for c in C_CASES) and any(c["hout"] * c["wout"] == 1 for c in C_CASES)
    assert {((c["h"] - c["ch"]) % 2, (c["w"] - c["cw"]) % 2) for c in T_CASES} >= {(0, 0), (1, 1)}
    # composed: non-square, odd, and the <32> instance within the sign projector's k k c <= 1152
    assert any(c["ny"] != c["nx"] and c["ny"] % 2 == 0 == c["nx"] % 2 for c in COMPOSED) and any(c["ny"] % 2 or c["nx"] % 2 for c in COMPOSED)
    assert any(17 <= c["c"] <= 32 for c in COMPOSED) and all(c["k"] ** 2 * c["c"] <= 1152 for c in COMPOSED)


# ------------------------------------------------------------------ the conditions on the draws
@pytest.mark.parametrize("s", E_SHAPES, ids=case_id)
def test_eig_draw_meets_its_conditions(s):
    c, npix = s["c"], s["npix"]
    m32, t = _eig_draw(c, npix)
    assert tuple(t.shape) == (c * c, npix, 2) and np.array_equal(m32, m32.conj().transpose(0, 2, 1))
    special = npix >= SPECIAL_MIN
    for crop in E_CROPS:
        maps, lam, overlap = ref_eig(m32, crop)
        live = lam != 0
        assert live.sum() == npix - special and np.nanmin(overlap) >= 1e-3, float(np.nanmin(overlap))
        assert np.abs(lam[live] - crop).min() >= 1e-4
        assert not special or (lam[ZERO_PIXEL] == 0 and not maps[:, ZERO_PIXEL].any())
        if special and c > 1:
            assert not m32[NOCOIL0_PIXEL, 0].any() and not m32[NOCOIL0_PIXEL, :, 0].any() and lam[NOCOIL0_PIXEL] > 0.3
        if crop == 0.8 and special:
            assert (lam >= crop).sum() >= npix / 4 and (lam < crop).sum() >= npix / 4
        norms = np.sqrt((np.abs(maps) ** 2).sum(axis=0))
        assert np.abs(norms[(lam >= crop) & live] - 1).max(initial=0) < PIN and not norms[lam < crop].any()
    w = np.linalg.eigvalsh(m32.astype(np.complex128))
    if c > 1:
        assert (w[:, -2] <= 0.5 * w[:, -1] + 1e-6).all()                 # the gap the 60 iterations rely on


@pytest.mark.parametrize("c", COMPOSED, ids=case_id)
def test_composed_shapes_have_a_region_to_compare(c):
    """`inside` depends on the oracle alone: at least 200 pixels and a third of the support, so that the GPU test cannot pass on nothing."""
    d = _composed_ref(_key(c))
    print(f"\n  {case_id(c)}: inside {int(d['inside'].sum())} of support {int(d['sup'].sum())}")
    assert d["inside"].sum() >= INSIDE_MIN and d["inside"].sum() >= INSIDE_SHARE * d["sup"].sum()


# ------------------------------------------------------------------ the float32 yardsticks
YARD = Worst()


@pytest.mark.parametrize("s", E_SHAPES, ids=case_id)
def test_float32_yardstick_of_the_power_iteration(s):
    """The textbook iteration in numpy float32 on the inputs of the GPU test against the float64 reference, at every crop: at most
    BAR / 2, the condition for holding the device to the plain BAR."""
    m32, _ = _eig_draw(s["c"], s["npix"])
    for crop in E_CROPS:
        maps, lam, _ = ref_eig(m32, crop)
        got, ev = _power(m32, E_ITERS, np.float32(crop))
        e_lam, e_v = eig_errs(got, ev, maps, lam)
        YARD.record("power iteration lam", e_lam, BAR / 2, case_id(s))
        YARD.record("power iteration maps", e_v, BAR / 2, case_id(s))


@pytest.mark.parametrize("c", T_CASES, ids=case_id)
def test_float32_yardstick_of_the_target(c):
    d = _target_ref(_key(c))
    img, sens = torch.view_as_complex(d["img"]), torch.view_as_complex(d["sens"])
    got = (img * sens.conj()[None]).sum(dim=1).abs()                    # torch's own float32 result
    y0, x0 = (c["h"] - c["ch"]) // 2, (c["w"] - c["cw"]) // 2
    got = got[:, y0:y0 + c["ch"], x0:x0 + c["cw"]].numpy()
    assert got.dtype == np.float32
    YARD.record("combine target", float(np.abs(got - d["ref"]).max() / d["ref"].max()), BAR / 2, case_id(c))


def test_float32_yardstick_report():
    """Prints the yardsticks of the two tests above (run with -s); they are recorded in DESIGN.md 4f."""
    if YARD:
        YARD.report()


# ================================================================== GPU tests
gpu = pytest.mark.gpu
WORST = Worst()
_record = WORST.record


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def _eig_call(dev, t, c, npix, iters, crop, what):
    def body(k):
        m, maps, lam = k.inp(t), k.out((c, npix, 2)), k.out((npix,))
        check(L().cine_espirit_eig(m.data_ptr(), maps.ptr(), lam.ptr(), c, npix, iters, crop, stream()), what)
        return [maps.t, lam.t]
    maps, lam = at_offsets(dev, OFFS, body, what)
    return _cplx(maps), lam.numpy().astype(np.float64)


@gpu
@pytest.mark.parametrize("c", E_CASES, ids=case_id)
def test_espirit_eig(dev, c):
    name, nc, npix, crop = "cine_espirit_eig", c["c"], c["npix"], c["crop"]
    m32, t = _eig_draw(nc, npix)
    ref_maps, ref_lam, _ = ref_eig(m32, crop)
    maps, lam = _eig_call(dev, t, nc, npix, E_ITERS, crop, name)
    e_lam, e_v = eig_errs(maps, lam, ref_maps, ref_lam)
    print(f"\n  {case_id(c)}: lam {e_lam:.3e} maps {e_v:.3e}")
    _record(name + " lam", e_lam, BAR, case_id(c))
    _record(name + " maps", e_v, BAR, case_id(c))
    cropped = ref_lam < crop
    assert not maps[:, cropped].any(), f"{name}: a cropped map is not exactly 0"
    if crop == 2.0:
        assert cropped.all()
    if crop == 0.0:
        assert not cropped.any()
    if npix >= SPECIAL_MIN:
        assert lam[ZERO_PIXEL] == 0 and not maps[:, ZERO_PIXEL].any(), f"{name}: M = 0 does not give exact zeros"
        if nc > 1 and crop < 2.0 and ref_lam[NOCOIL0_PIXEL] >= crop:
            assert not maps[0, NOCOIL0_PIXEL].any(), f"{name}: coil 0 of a pixel without a coil-0 component is not exactly 0"


@gpu
@pytest.mark.parametrize("nc", E_COILS)
def test_espirit_eig_one_iteration(dev, nc):
    """iters = 1 pins what lam means: v^H M v of the vector BEFORE the last step, here sum_ij M_ij / c of the uniform vector; the maps are
    one normalised step from it."""
    name, npix = "cine_espirit_eig iters=1", 65
    m32, t = _eig_draw(nc, npix)
    ref_maps, ref_lam = ref_eig_steps(m32, 1)
    assert np.abs(ref_lam - m32.astype(np.complex128).sum(axis=(1, 2)).real / nc).max() < PIN
    maps, lam = _eig_call(dev, t, nc, npix, 1, 0.0, name)
    peak = float(np.abs(ref_lam).max())
    _record(name + " lam", float(np.abs(lam - ref_lam).max()) / peak, BAR, f"c{nc}")
    _record(name + " maps", float(np.abs(maps - ref_maps).max()), BAR, f"c{nc}")


def _window(kk, ny, nx):
    win = np.zeros((ny, nx), bool)
    win[ny // 2 - (kk - 1):ny // 2 + kk, nx // 2 - (kk - 1):nx // 2 + kk] = True
    return win


@gpu
@pytest.mark.parametrize("c", K_CASES, ids=case_id)
def test_espirit_lag_kernels(dev, c):
    name, nc, kk, ny, nx = "cine_espirit_lag_kernels", c["c"], c["kk"], c["ny"], c["nx"]
    n = kk * kk * nc
    proj = _pairs_rand(hash_case(c), n, n)
    ref = ref_lag_kernels(_cplx(proj), nc, kk, ny, nx)

    def body(k):
        p, kpad = k.inp(proj), k.out((nc * nc, ny, nx, 2))
        check(L().cine_espirit_lag_kernels(p.data_ptr(), kpad.ptr(), nc, kk, ny, nx, stream()), name)
        return [kpad.t]
    kpad, = at_offsets(dev, OFFS, body, name)
    _record(name, float(np.abs(_cplx(kpad).reshape(ref.shape) - ref).max() / np.abs(ref).max()), BAR, case_id(c))
    outside = kpad.view(nc * nc, ny, nx, 2)[:, torch.from_numpy(~_window(kk, ny, nx))]
    assert not bool(outside.view(torch.int32).any()), f"{name}: the zero padding is not +0.0 bit for bit"


@gpu
@pytest.mark.parametrize("c", I_CASES, ids=case_id)
def test_lag_kernels_transform_to_the_operator(dev, c):
    """cine_fft2c(kpad, inverse) is the c x c operator of every pixel (cine_hip.h), for proj = V V^H."""
    name, nc, kk, ny, nx = "cine_espirit_lag_kernels + cine_fft2c", c["c"], c["kk"], c["ny"], c["nx"]
    d = _identity_ref(_key(c))

    def body(k):
        p, kpad, m = k.inp(d["proj"]), k.out((nc * nc, ny, nx, 2)), k.out((nc * nc, ny, nx, 2))
        check(L().cine_espirit_lag_kernels(p.data_ptr(), kpad.ptr(), nc, kk, ny, nx, stream()), name)
        check(L().cine_fft2c(kpad.ptr(), m.ptr(), nc * nc, ny, nx, 1, stream()), name)
        return [m.t]
    m, = at_offsets(dev, OFFS, body, name)
    got = _cplx(m).reshape(nc, nc, ny, nx).transpose(2, 3, 0, 1)
    _record(name, float(np.abs(got - d["m"]).max() / np.abs(d["m"]).max()), BAR, case_id(c))


@gpu
@pytest.mark.parametrize("c", G_CASES, ids=case_id)
def test_gauss_axis(dev, c):
    pytest.importorskip("scipy.ndimage")
    name, outer, n, inner, sigma = "cine_gauss_axis", c["outer"], c["n"], c["inner"], c["sigma"]
    x = _pairs_rand(hash_case(dict(outer=outer, n=n, inner=inner)), outer, n, inner)
    ref = ref_gauss_axis(_cplx(x), sigma)

    def body(k):
        xi, o = k.inp(x), k.out(x.shape)
        check(L().cine_gauss_axis(xi.data_ptr(), o.ptr(), outer, n, inner, sigma, stream()), name)
        return [o.t]
    o, = at_offsets(dev, OFFS, body, name)
    _record(name, float(np.abs(_cplx(o) - ref).max() / np.abs(ref).max()), BAR_GAUSS, case_id(c))


@gpu
@pytest.mark.parametrize("c", C_CASES, ids=case_id)
def test_crop_select(dev, c):
    name = "cine_crop_select"
    x = _pairs_rand(hash_case(c), c["t_in"], c["c"], c["hin"], c["win"])
    ref = ref_crop_select(x, c["t_out"], c["hout"], c["wout"]).contiguous()

    def body(k):
        xi, o = k.inp(x), k.out(ref.shape)
        check(L().cine_crop_select(xi.data_ptr(), o.ptr(), c["t_in"], c["c"], c["hin"], c["win"], c["t_out"], c["hout"], c["wout"], stream()), name)
        return [o.t]
    o, = at_offsets(dev, OFFS, body, name)
    assert same_bits(o, ref), f"{name} {case_id(c)}: not the bits of the slice"


@gpu
@pytest.mark.parametrize("c", T_CASES, ids=case_id)
def test_combine_target(dev, c):
    name = "cine_combine_target"
    d = _target_ref(_key(c))

    def body(k):
        img, sens, o = k.inp(d["img"]), k.inp(d["sens"]), k.out(d["ref"].shape)
        check(L().cine_combine_target(img.data_ptr(), sens.data_ptr(), o.ptr(), c["t"], c["c"], c["h"], c["w"], c["ch"], c["cw"], stream()), name)
        return [o.t]
    o, = at_offsets(dev, OFFS, body, name)
    _record(name, float(np.abs(o.numpy().astype(np.float64) - d["ref"]).max() / d["ref"].max()), BAR, case_id(c))


# ------------------------------------------------------------------ the composed calibration
@gpu
@pytest.mark.parametrize("method", ["eigh", "sign"])
@pytest.mark.parametrize("c", COMPOSED, ids=case_id)
def test_espirit_maps_on_new_shapes(dev, c, method):
    """test_frontend.py::test_espirit_vs_oracle's region and bars on a non-square, an odd and a 32-coil shape, both methods."""
    from cine_hip import frontend as FE
    d = _composed_ref(_key(c))
    inside, want, lam_w = d["inside"], d["maps"], d["lam"]
    assert inside.sum() >= INSIDE_MIN and inside.sum() >= INSIDE_SHARE * d["sup"].sum()
    k = _pairs(d["kavg"]).to(dev)
    if method == "sign":
        got, lam_g, resid = FE.espirit_maps(k, r=c["r"], k=c["k"], method="sign", return_residual=True)
        assert float(resid) <= 1e-6, float(resid)
    else:
        got, lam_g = FE.espirit_maps(k, r=c["r"], k=c["k"])
    got, lam_g = _cplx(got), lam_g.cpu().numpy()
    assert np.abs(lam_g - lam_w)[inside].max() < 1e-3
    assert np.abs(got - want)[:, inside].max() < 5e-3
    assert np.sqrt((np.abs(got - want)[:, inside] ** 2).mean()) < 5e-4
    flip = (lam_g >= 0.8) != (lam_w >= 0.8)
    assert np.all(np.abs(lam_w[flip] - 0.8) < 5e-3)


# ================================================================== refusals: decided on the host, before any launch
def _swap(args, i, v):
    return args[:i] + (v,) + args[i + 1:]


def _refuse(k, name, args, nulls=(), bad=()):
    """Every pointer of `nulls` NULL in turn -> EINVAL; every ({index: value}, code, what) of `bad`."""
    entry = getattr(L(), name)
    for i in nulls:
        refused(lambda: entry(*_swap(args, i, None)), EINVAL, k, f"{name} argument {i} NULL")
    for repl, code, what in bad:
        a = args
        for i, v in repl.items():
            a = _swap(a, i, v)
        refused(lambda: entry(*a), code, k, f"{name} {what}")


@gpu
def test_calibration_refusals(dev):
    """Buffers sized for 33 coils on 4 pixels and for kk = 2, c = 2 on 4 x 4, so every refused call would have stayed inside them."""
    st = stream()
    k = Call(dev, 0)
    m, proj = k.inp(_pairs_rand(1, 33 * 33, 4)), k.inp(_pairs_rand(2, 8, 8))
    maps, lam, kpad = k.out((33, 4, 2)), k.out((4,)), k.out((4, 4, 4, 2))
    _refuse(k, "cine_espirit_eig", (m.data_ptr(), maps.ptr(), lam.ptr(), 2, 4, 3, 0.8, st), (0, 1, 2),
            [({3: 0}, EINVAL, "c=0"), ({3: 33}, EINVAL, "c=33"), ({3: -1}, EINVAL, "c=-1"), ({4: 0}, EINVAL, "npix=0"), ({5: 0}, EINVAL, "iters=0")])
    _refuse(k, "cine_espirit_lag_kernels", (proj.data_ptr(), kpad.ptr(), 2, 2, 4, 4, st), (0, 1),
            [({4: 2}, EINVAL, "ny=2 < 2 kk - 1"), ({5: 2}, EINVAL, "nx=2 < 2 kk - 1"), ({2: 0}, EINVAL, "c=0"), ({2: -1}, EINVAL, "c=-1"),
             ({3: 0}, EINVAL, "kk=0"), ({3: -1}, EINVAL, "kk=-1")])


@gpu
def test_front_end_refusals(dev):
    st = stream()
    k = Call(dev, 0)
    x, s = k.inp(_pairs_rand(3, 2, 3, 6, 5)), k.inp(_pairs_rand(4, 3, 6, 5))
    o, tg = k.out((2, 3, 6, 5, 2)), k.out((2, 6, 5))
    X, S, O, T = x.data_ptr(), s.data_ptr(), o.ptr(), tg.ptr()
    _refuse(k, "cine_gauss_axis", (X, O, 6, 6, 5, 0.7, st), (0, 1),
            [({5: 4.2}, EUNSUPPORTED, "sigma=4.2 (35 taps)"), ({5: 0.0}, EINVAL, "sigma=0"), ({0: O}, EINVAL, "in == out"),
             ({2: 0}, EINVAL, "outer=0"), ({3: 0}, EINVAL, "n=0"), ({4: 0}, EINVAL, "inner=0")])
    _refuse(k, "cine_crop_select", (X, O, 2, 3, 6, 5, 2, 4, 3, st), (0, 1),
            [({7: 7}, EINVAL, "hout > hin"), ({8: 6}, EINVAL, "wout > win"), ({6: 3}, EINVAL, "t_out > t_in"), ({0: O}, EINVAL, "in == out"),
             ({6: 0}, EINVAL, "t_out=0"), ({3: 0}, EINVAL, "c=0")])
    _refuse(k, "cine_combine_target", (X, S, T, 2, 3, 6, 5, 4, 3, st), (0, 1, 2),
            [({7: 7}, EINVAL, "ch > h"), ({8: 6}, EINVAL, "cw > w"), ({3: 0}, EINVAL, "t=0"), ({4: 0}, EINVAL, "c=0"), ({7: 0}, EINVAL, "ch=0")])
