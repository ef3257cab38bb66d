"""The float64 restatement of noise pre-whitening folded into the coil-compression matrix (frontend.noise_whitener,
coil_matrix_from_gram(..., whitener=W), cine_coil_matrix_whitened), in numpy (cholesky, inv, eigh), and the designed inputs its tests share.

Definitions: Psi[i, j] = 1/n sum_s eta_s[i] conj(eta_s[j]) = L L^H (L lower-triangular, real positive diagonal), W = s L^-1 with
s = sqrt(trace(Psi) / c) (or 1), G' = W G W^H = U diag(lam) U^H (lam descending), A[r] = p_r sum_k conj(U[k, r]) W[k, :] with p_r the
unit phase that makes the row's largest-magnitude entry real and positive.

Designed input.  Whitening an arbitrary spectrum scrambles its gaps, so the raw data are built from the covariance: Psi = Q diag(1e-5
100^(-k / (c - 1))) Q^H (condition number 100, Q from the QR of a seeded complex Gaussian) and raw = complex64(z (L / s)^T) with z the
designed input of tests/test_coil_compress.py: the whitened samples W raw are z again (up to the complex64 rounding), whose spectrum
has the gaps that file designs.  Every test asserts the gaps of its own whitened Gram matrix in float64 before anything runs."""
import numpy as np

from test_coil_compress import assert_gaps, designed_raw, gram_ref

# (c, V, seed), (t, nx, ny) = (2, 24, 24), region 24
CASES = [(2, 1, 3), (3, 2, 4), (5, 5, 10), (17, 8, 21), (30, 15, 45), (33, 12, 45), (64, 32, 9)]
IDS = [f"{c}to{v}" for c, v, _ in CASES]
SHAPE = (2, 24, 24)


def designed_cov(c, seed):
    rs = np.random.RandomState(1000 + seed)
    q, _ = np.linalg.qr(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c)))
    d = 1e-5 * 100.0 ** (-np.arange(c) / max(c - 1, 1))
    psi = (q * d) @ q.conj().T
    psi = (psi + psi.conj().T) / 2
    psi[np.diag_indices(c)] = psi.diagonal().real
    return psi


def whitener_ref(psi, preserve_scale=True):
    """(W, s): W = s L^-1, lower-triangular with a real positive diagonal."""
    c = psi.shape[0]
    low = np.linalg.cholesky(psi)                                     # lower, real positive diagonal
    s = np.sqrt(psi.diagonal().real.sum() / c) if preserve_scale else 1.0
    w = np.tril(s * np.linalg.inv(low))
    w[np.diag_indices(c)] = w.diagonal().real
    return w, s


def whitened_matrix_ref(gram, w, v):
    """(A (V, c), lam (c,)) of the definitions above."""
    gp = w @ gram @ w.conj().T
    gp = (gp + gp.conj().T) / 2
    lam, u = np.linalg.eigh(gp)
    lam, u = lam[::-1], u[:, ::-1]
    a = u[:, :v].conj().T @ w
    for r in range(v):
        k = int(np.argmax(np.abs(a[r])))                              # the first of equal maxima
        a[r] *= np.conj(a[r, k]) / abs(a[r, k])
    return a, lam


_CACHE = {}


def designed_case(c, v, seed):
    """dict(raw complex64 (2, 24, 24, c), psi, w, s, gram (float64, region 24), a, lam) of a case, computed once; the gaps of the
    whitened Gram matrix are asserted here, in float64."""
    key = (c, v, seed)
    if key not in _CACHE:
        psi = designed_cov(c, seed)
        w, s = whitener_ref(psi)
        low = np.linalg.cholesky(psi)
        z = designed_raw(*SHAPE, c, seed).astype(np.complex128)
        raw = (z @ (low / s).T).astype(np.complex64)
        gram = gram_ref(raw, SHAPE[0], 24)
        a, lam = whitened_matrix_ref(gram, w, v)
        assert_gaps(lam, v)
        for x in (raw, psi, w, gram, a, lam):
            x.setflags(write=False)
        _CACHE[key] = dict(raw=raw, psi=psi, w=w, s=s, gram=gram, a=a, lam=lam)
    return _CACHE[key]


def check_against_ref(a, lam, case, v, what=""):
    """The bars of the parity tests, for a (V, c) complex128 and lam (c,) float64 computed by the code under test.  m = max(1, max
    |A_ref|): the entries of A are no longer bounded by 1, and every bar that tests/test_coil_matrix_kernel.py derives for entries of
    size one (eigenvectors off by about 1e-9 under these gaps, below the complex64 rounding) scales with their size."""
    a_w, lam_w, psi, gram, s = case["a"], case["lam"], case["psi"], case["gram"], case["s"]
    m = max(1.0, float(np.abs(a_w).max()))
    e_lam = np.abs(lam - lam_w).max() / lam_w[0]
    e_proj = np.abs(a.conj().T @ a - a_w.conj().T @ a_w).max() / m ** 2
    align = min(abs(np.vdot(a_w[r], a[r])) / (np.linalg.norm(a_w[r]) * np.linalg.norm(a[r])) for r in range(v))
    e_white = np.abs(a @ psi @ a.conj().T / s ** 2 - np.eye(v)).max() / m ** 2
    e_diag = np.abs(a @ gram @ a.conj().T - np.diag(lam[:v])).max() / (m ** 2 * lam[0])
    print(f"{what}: m {m:.3f}, lam {e_lam:.3e}, projector {e_proj:.3e}, worst row alignment 1 - {1 - align:.3e}, "
          f"A Psi A^H {e_white:.3e}, A G A^H {e_diag:.3e}")
    assert (np.diff(lam) <= 0).all() and e_lam <= 1e-9
    assert e_proj <= 1e-6
    assert align >= 1 - 1e-6
    assert e_white <= 1e-6 and e_diag <= 1e-6
    for row in a:                                                     # the phase rule, the peak stored exactly real
        pk = row[int(np.argmax(np.abs(row)))]
        assert pk.real > 0 and pk.imag == 0.0
