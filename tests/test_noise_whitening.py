"""cine_coil_matrix_whitened (frontend.coil_matrix_from_gram(..., method="jacobi", whitener=W)): noise pre-whitening folded into the
coil-compression matrix on the device, frontend.noise_covariance / noise_whitener in front of it, and the ``whitener=`` argument of
prepare_slice / prepare_masked_slice.

Against the float64 restatement of tests/whitening_ref.py on its designed inputs (raw data built from the noise covariance so that
the WHITENED Gram matrix has the gaps tests/test_coil_compress.py designs; asserted in float64 before anything runs on the device),
with the bars tests/test_coil_matrix_kernel.py holds the plain kernel to, scaled by the size m = max(1, max |A_ref|) of the entries:
the rows of A = U^H W are not unit vectors any more.  The complex64 rounding of the float64 answer alone is at most 1.5e-7 m^2 on these
inputs."""
import ctypes

import numpy as np
import pytest
import torch

from test_coil_compress import designed_raw, gram_ref
from whitening_ref import CASES, IDS, SHAPE, check_against_ref, designed_case

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
TOL, SWEEP_CAP = 1e-14, 40                                   # kLsJacobiTol, kLsMaxSweeps (csrc/ls_jacobi.h)
FS = (0.7, 0.0, 0.3, 0.3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(x):
    return torch.view_as_real(x) if x.is_complex() else x


def _same(got, want):
    return all(torch.equal(_bits(g), _bits(w)) for g, w in zip(got, want))


# ------------------------------------------------------------------ 1. parity with float64 on the designed inputs
@pytest.mark.parametrize("c,v,seed", CASES, ids=IDS)
def test_whitened_jacobi_matrix_vs_float64(dev, c, v, seed):
    from cine_hip import frontend as FE
    case = designed_case(c, v, seed)                                  # asserts the gaps of the whitened Gram matrix, in float64
    x = torch.from_numpy(case["raw"].copy()).to(dev)
    w = FE.noise_whitener(cov=torch.from_numpy(case["psi"].copy()).to(dev))
    assert w.dtype == torch.complex128 and w.device.type == "cuda" and tuple(w.shape) == (c, c)
    assert np.abs(w.cpu().numpy() - case["w"]).max() <= 1e-12 * np.abs(case["w"]).max()
    a, lam, info = FE.coil_compression_matrix(x, v, SHAPE[0], 24, cc_method="jacobi", whitener=w)
    assert a.dtype == torch.complex64 and tuple(a.shape) == (v, c) and a.device.type == "cuda"
    assert lam.dtype == torch.float64 and tuple(lam.shape) == (c,)
    assert info.dtype == torch.float64 and tuple(info.shape) == (4,) and info.device.type == "cuda"
    a, lam, info = a.cpu().numpy().astype(np.complex128), lam.cpu().numpy(), info.cpu().numpy()
    print(f"whitened jacobi {c} -> {v}: residual {info[0]:.3e}, sweeps {info[1]:.0f}, kept {info[2]:.9f}")
    check_against_ref(a, lam, case, v, f"whitened jacobi {c} -> {v}")
    lam_w = case["lam"]
    assert info[0] <= TOL and 0 <= info[1] < SWEEP_CAP
    assert abs(info[2] - lam_w[:v].sum() / lam_w.sum()) <= 1e-9 and info[3] == lam[0]
    # the same decomposition as method="eigh" on the device, to the same bars
    a_e, lam_e = FE.coil_compression_matrix(x, v, SHAPE[0], 24, whitener=w)
    a_e, lam_e = a_e.cpu().numpy().astype(np.complex128), lam_e.cpu().numpy()
    check_against_ref(a_e, lam_e, case, v, f"whitened eigh on the device {c} -> {v}")
    m = max(1.0, float(np.abs(case["a"]).max()))
    assert np.abs(a.conj().T @ a - a_e.conj().T @ a_e).max() <= 1e-6 * m ** 2 and np.abs(lam - lam_e).max() <= 1e-9 * lam_w[0]


# ------------------------------------------------------------------ 2. the identity as whitener: the bits of cine_coil_matrix
def _grams(n, c, seed):
    return np.stack([gram_ref(designed_raw(2, 10, 10, c, seed=seed + j), 2, 0) for j in range(n)])


def test_identity_whitener_gives_the_bits_of_the_plain_kernel(dev):
    from cine_hip import frontend as FE
    g = torch.from_numpy(_grams(3, 13, 20)).to(dev)
    eye = torch.eye(13, dtype=torch.complex128, device=dev)
    want = FE.coil_matrix_from_gram(g, 6, method="jacobi")
    got = FE.coil_matrix_from_gram(g, 6, method="jacobi", whitener=eye)
    assert tuple(got[0].shape) == (3, 6, 13) and _same(got, want)
    assert _same(FE.coil_matrix_from_gram(g[1], 6, method="jacobi", whitener=eye), FE.coil_matrix_from_gram(g[1], 6, method="jacobi"))
    assert float(want[2][:, 1].min()) > 0                             # sweeps were run: the rotations saw the same numbers


# ------------------------------------------------------------------ 3. the whitener alone; the covariance
def _mask(t, X, seed, dev):
    rs = np.random.RandomState(1000 + seed)
    m = (rs.uniform(size=(1, t, 1, X, 1, 1)) < 0.3).astype(np.uint8)
    m[:, :, :, X // 2 - 2:X // 2 + 2] = 1
    return torch.from_numpy(m).to(dev)


def test_whitener_alone_is_the_coil_matrix_w(dev):
    from cine_hip import frontend as FE
    case = designed_case(5, 5, 10)
    raw = torch.from_numpy(case["raw"] * np.float32(1e-6)).to(dev)
    w = torch.from_numpy(case["w"].copy()).to(dev)
    mask = _mask(2, 21, 1, dev)
    want = FE.prepare_masked_slice(raw, mask, (21, 17), 2, FS, 1e6, coil_matrix=w.to(torch.complex64))
    got = FE.prepare_masked_slice(raw, mask, (21, 17), 2, FS, 1e6, whitener=w)
    assert tuple(got.shape) == (1, 2, 5, 21, 17, 2) and torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert not torch.equal(got, FE.prepare_masked_slice(raw, mask, (21, 17), 2, FS, 1e6))
    k, f = FE.prepare_slice(raw, (21, 17), 2, FS, whitener=w)
    k2, f2 = FE.prepare_slice(raw, (21, 17), 2, FS, coil_matrix=w.to(torch.complex64))
    assert torch.equal(k, k2) and torch.equal(f, f2)
    with pytest.raises(FE.CineHipError, match="virtual_coils="):
        FE.prepare_masked_slice(torch.zeros(2, 24, 24, 40, dtype=torch.complex64, device=dev), mask, (21, 17), 2, FS, 1e6,
                                whitener=torch.eye(40, dtype=torch.complex128, device=dev))
    with pytest.raises(ValueError, match=r"coil_matrix_from_gram\(\.\.\., whitener=W\)"):
        FE.prepare_masked_slice(raw, mask, (21, 17), 2, FS, 1e6, coil_matrix=w.to(torch.complex64), whitener=w)
    for bad in (w.cpu(), w.to(torch.complex64)):
        with pytest.raises(FE.CineHipError, match="complex128 GPU"):
            FE.prepare_masked_slice(raw, mask, (21, 17), 2, FS, 1e6, whitener=bad)
    with pytest.raises(ValueError, match="whitener"):
        FE.prepare_masked_slice(raw, mask, (21, 17), 2, FS, 1e6, whitener=w[:4, :4])


def test_noise_covariance_vs_float64(dev):
    from cine_hip import frontend as FE
    rs = np.random.RandomState(12)
    mix = rs.standard_normal((12, 12)) + 1j * rs.standard_normal((12, 12))
    eta = ((rs.standard_normal((4096, 12)) + 1j * rs.standard_normal((4096, 12))) @ mix.T * 1e-3).astype(np.complex64)
    e = eta.astype(np.complex128)
    want = e.T @ e.conj() / 4096
    x = torch.from_numpy(eta).to(dev)
    psi = FE.noise_covariance(x)
    assert psi.dtype == torch.complex128 and tuple(psi.shape) == (12, 12)
    err = np.abs(psi.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"noise covariance (4096, 12): max|Psi - Psi_ref| / max|Psi_ref| = {err:.3e}")
    assert err <= 1e-12                                               # exact products, float64 sums
    assert torch.equal(psi, psi.conj().transpose(0, 1).resolve_conj()) and bool((psi.diagonal().imag == 0).all())
    assert torch.equal(FE.noise_covariance(x), psi)                   # bit-identical on a second call
    assert torch.equal(FE.noise_covariance(x.view(64, 64, 12)), psi)  # any leading axes: the same factorisation
    # and the whitener of the samples is the whitener of that covariance
    w = FE.noise_whitener(x)
    assert torch.equal(_bits(w), _bits(FE.noise_whitener(cov=psi)))
    wn = w.cpu().numpy()
    s2 = want.diagonal().real.sum() / 12
    assert np.abs(wn @ want @ wn.conj().T / s2 - np.eye(12)).max() <= 1e-10
    with pytest.raises(ValueError, match="too few noise samples"):
        FE.noise_whitener(x[:7])
    with pytest.raises(FE.CineHipError, match="at most 128"):
        FE.noise_covariance(torch.zeros(4, 129, dtype=torch.complex64, device=dev))


# ------------------------------------------------------------------ 4. memory discipline
def test_unread_triangles_batches_and_repeats(dev):
    from cine_hip import frontend as FE
    case = designed_case(33, 12, 45)
    w = torch.from_numpy(case["w"].copy()).to(dev)
    gs = np.stack([case["gram"], 2.0 * case["gram"], gram_ref(designed_raw(2, 10, 10, 33, seed=40), 2, 0)])
    g = torch.from_numpy(gs).to(dev)
    want = FE.coil_matrix_from_gram(g, 12, method="jacobi", whitener=w)
    assert tuple(want[0].shape) == (3, 12, 33) and tuple(want[1].shape) == (3, 33) and tuple(want[2].shape) == (3, 4)
    assert not torch.equal(want[0][0], want[0][2])
    # NaN junk in the upper triangle of W, in the lower triangle of G and in both diagonals' imaginary parts changes no bit
    junk_w = case["w"].copy()
    up = np.triu_indices(33, 1)
    junk_w[up] = np.random.RandomState(1).standard_normal(len(up[0])) * 1e3 + 1j * np.nan
    junk_w[np.diag_indices(33)] += 1j * 7.0
    junk_g = gs.copy()
    low = np.tril_indices(33, -1)
    junk_g[:, low[0], low[1]] = np.nan + 1j * 1e3
    junk_g[:, np.arange(33), np.arange(33)] += 1j * 5.0
    got = FE.coil_matrix_from_gram(torch.from_numpy(junk_g).to(dev), 12, method="jacobi", whitener=torch.from_numpy(junk_w).to(dev))
    assert _same(got, want)
    # a batch is its single calls; repeats give equal bits
    for j in range(3):
        assert _same(FE.coil_matrix_from_gram(g[j], 12, method="jacobi", whitener=w), [x[j] for x in want]), j
    for _ in range(3):
        assert _same(FE.coil_matrix_from_gram(g, 12, method="jacobi", whitener=w), want)


@pytest.mark.parametrize("where", [(2, 2), (1, 4)], ids=["diagonal", "off-diagonal"])
def test_nan_in_gram_returns_and_the_next_call_is_right(dev, where):
    from cine_hip import frontend as FE
    case = designed_case(17, 8, 21)
    w = torch.from_numpy(case["w"].copy()).to(dev)
    g = case["gram"].copy()
    g[where] = np.nan
    a, lam, info = FE.coil_matrix_from_gram(torch.from_numpy(g).to(dev), 8, method="jacobi", whitener=w)
    torch.cuda.synchronize()                                          # the call returns: bounded sweeps
    info = info.cpu().numpy()
    print(f"NaN at {where}: residual {info[0]}, sweeps {info[1]}")
    assert np.isnan(info[0]) or info[1] == SWEEP_CAP
    assert tuple(a.shape) == (8, 17) and tuple(lam.shape) == (17,)
    a, lam, info = FE.coil_matrix_from_gram(torch.from_numpy(case["gram"].copy()).to(dev), 8, method="jacobi", whitener=w)
    check_against_ref(a.cpu().numpy().astype(np.complex128), lam.cpu().numpy(), case, 8, "after the NaN")
    assert float(info[0]) <= TOL


def test_refusals_before_any_launch(dev):
    from cine_hip import _lib, frontend as FE
    from cine_hip._lib import CineHipError
    L = _lib.lib()
    g, w, m, lam, info = (ctypes.c_void_p(p) for p in (0x1000, 0x5000, 0x2000, 0x3000, 0x4000))          # never dereferenced

    def call(g=g, w=w, m=m, lam=lam, info=info, nb=1, c=30, v=15):
        return L.cine_coil_matrix_whitened(g, w, m, lam, info, nb, c, v, None)

    assert call(c=65) == EUNSUPPORTED and b"64" in L.cine_last_error()
    assert call(c=64, v=33) == EUNSUPPORTED and b"32" in L.cine_last_error()
    assert call(v=0) == EINVAL and b"Invalid shapes" in L.cine_last_error()
    assert call(v=31) == EINVAL and call(nb=0) == EINVAL and call(c=0, v=0) == EINVAL
    for kw in (dict(g=None), dict(w=None), dict(m=None), dict(lam=None), dict(info=None)):
        assert call(**kw) == EINVAL and b"null" in L.cine_last_error(), kw
    assert call(m=g) == EINVAL and b"aliased" in L.cine_last_error()
    assert call(w=g) == EINVAL and b"aliased" in L.cine_last_error()
    assert call(g=ctypes.c_void_p(0x1008)) == EINVAL and b"aligned" in L.cine_last_error()
    assert call(w=ctypes.c_void_p(0x5008)) == EINVAL and b"aligned" in L.cine_last_error()
    g65 = torch.eye(65, dtype=torch.complex128, device=dev)
    with pytest.raises(CineHipError, match="at most 64"):
        FE.coil_matrix_from_gram(g65, 15, method="jacobi", whitener=g65.clone())
    g64 = g65[:64, :64].contiguous()
    with pytest.raises(CineHipError, match="at most 32"):
        FE.coil_matrix_from_gram(g64, 33, method="jacobi", whitener=g64.clone())
    with pytest.raises(ValueError, match="whitener"):
        FE.coil_matrix_from_gram(g64, 15, method="jacobi", whitener=g65)
    a, _ = FE.coil_matrix_from_gram(g65, 15, whitener=g65)            # the default method still takes 65 coils
    assert tuple(a.shape) == (15, 65)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ prepare_masked_slice(virtual_coils=V, whitener=W): composition, capture
def test_prepare_masked_slice_whitened_is_the_composition_and_capturable(dev):
    from cine_hip import frontend as FE
    from cine_hip.pipeline import pipeline_streams
    shape, crop, n = (3, 40, 36, 12), (21, 17), 3
    case = designed_case(17, 8, 21)
    w = FE.noise_whitener(cov=torch.from_numpy(case["psi"][:12, :12].copy()).to(dev))
    raws = [torch.from_numpy(designed_raw(*shape, seed=60 + j) * np.float32(1e-6)).to(dev) for j in range(2)]
    mask = _mask(n, crop[0], 2, dev)
    want = []
    for v in (6, 12):                                                 # V == c is not passed through: the data are whitened
        for r in raws:
            a = FE.coil_matrix_from_gram(FE.coil_gram(r, n, 24), v, method="jacobi", whitener=w)[0]
            ref = FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, coil_matrix=a).clone()
            eager = FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, virtual_coils=v, whitener=w)
            assert tuple(eager.shape) == (1, n, v) + crop + (2,) and torch.equal(eager, ref)
            assert not torch.equal(eager, FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, virtual_coils=v))
            k, f = FE.prepare_slice(r, crop, n, FS, virtual_coils=v, cc_method="jacobi", whitener=w)
            k2, f2 = FE.prepare_slice(r, crop, n, FS, coil_matrix=a)
            assert torch.equal(k, k2) and torch.equal(f, f2)
            if v == 6:
                want.append(ref)
    assert not torch.equal(want[0], want[1])
    static = torch.zeros_like(raws[0])
    s = pipeline_streams(dev, 1)[0][0]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        FE.prepare_masked_slice(static, mask, crop, n, FS, 1e6, virtual_coils=6, whitener=w)      # warm outside capture (a zero slice: finite)
    s.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        out = FE.prepare_masked_slice(static, mask, crop, n, FS, 1e6, virtual_coils=6, whitener=w)
    for j, r in enumerate(raws):
        static.copy_(r)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[j]), j
