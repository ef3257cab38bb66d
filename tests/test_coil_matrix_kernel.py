"""cine_coil_matrix (frontend.coil_matrix_from_gram(..., method="jacobi")): the eigen step of the coil compression on the device, and
frontend.prepare_masked_slice(..., virtual_coils=V) that runs it per slice.

Against the float64 restatement of tests/test_coil_compress.py (gram_ref, matrix_ref) on its designed inputs and under its input
conditions (assert_gaps, checked in float64 before anything runs on the device), with the bars that file derives and holds
method="eigh" to: with every consecutive gap >= 1e-5 lam[0] and a Jacobi stop at max |off-diagonal| <= 1e-14 max |diagonal| the
eigenvectors are off by about 1e-9, below the complex64 rounding of A (2.3e-8), so no new number is needed.  Where the basis is free
(equal eigenvalues) only what does not depend on the choice is checked: A A^H = I, A G A^H = diag(lam[:V]), the kept share."""
import ctypes

import numpy as np
import pytest
import torch

from test_coil_compress import assert_gaps, designed_raw, gram_ref, matrix_ref, phase_rule_holds

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
TOL, SWEEP_CAP = 1e-14, 40                                   # kLsJacobiTol, kLsMaxSweeps (csrc/ls_jacobi.h)
FS = (0.7, 0.0, 0.3, 0.3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _jacobi(g, v, dev):
    from cine_hip import frontend as FE
    a, lam, info = FE.coil_matrix_from_gram(torch.as_tensor(g, dtype=torch.complex128).to(dev), v, method="jacobi")
    return a, lam, info


def _np(a, lam, info):
    return a.cpu().numpy().astype(np.complex128), lam.cpu().numpy(), info.cpu().numpy()


# ------------------------------------------------------------------ parity with float64 on the designed inputs
# (c, V, seed): (t, nx, ny) = (2, 24, 24), region 24 -- the (64, 32) case and its seed are those of test_coil_compress.py
PARITY = [(2, 1, 3), (5, 5, 10), (30, 15, 45), (33, 12, 45), (64, 32, 9)]


@pytest.mark.parametrize("c,v,seed", PARITY, ids=[f"{c}to{v}" for c, v, _ in PARITY])
def test_jacobi_matrix_vs_float64(dev, c, v, seed):
    from cine_hip import frontend as FE
    raw = designed_raw(2, 24, 24, c, seed=seed)
    a_w, lam_w = matrix_ref(gram_ref(raw, 2, 24), v)
    assert_gaps(lam_w, v)
    x = torch.from_numpy(raw).to(dev)
    a, lam, info = FE.coil_compression_matrix(x, v, 2, 24, cc_method="jacobi")
    assert a.dtype == torch.complex64 and tuple(a.shape) == (v, c) and a.device.type == "cuda"
    assert lam.dtype == torch.float64 and tuple(lam.shape) == (c,)
    assert info.dtype == torch.float64 and tuple(info.shape) == (4,) and info.device.type == "cuda"
    a, lam, info = _np(a, lam, info)
    e_lam = np.abs(lam - lam_w).max() / lam_w[0]
    e_proj = np.abs(a.conj().T @ a - a_w.conj().T @ a_w).max()
    align = min(abs(np.vdot(a_w[r], a[r])) for r in range(v))
    print(f"jacobi {c} -> {v}: lam {e_lam:.3e}, projector {e_proj:.3e}, worst row alignment 1 - {1 - align:.3e}, "
          f"residual {info[0]:.3e}, sweeps {info[1]:.0f}")
    assert (np.diff(lam) <= 0).all() and e_lam <= 1e-9
    assert e_proj <= 1e-6
    assert align >= 1 - 1e-6
    assert phase_rule_holds(a)
    for row in a:                                                     # the peak is stored exactly real
        assert row[int(np.argmax(np.abs(row)))].imag == 0.0
    assert info[0] <= TOL and 0 <= info[1] < SWEEP_CAP
    assert abs(info[2] - lam_w[:v].sum() / lam_w.sum()) <= 1e-9 and info[3] == lam[0]
    # the same decomposition as method="eigh" on the device, to the same bars
    a_e, lam_e = FE.coil_compression_matrix(x, v, 2, 24)
    a_e = a_e.cpu().numpy().astype(np.complex128)
    assert np.abs(a.conj().T @ a - a_e.conj().T @ a_e).max() <= 1e-6 and np.abs(lam - lam_e.cpu().numpy()).max() <= 1e-9 * lam_w[0]


# ------------------------------------------------------------------ structure where the basis is free
def _structure(g, v, dev):
    a, lam, info = _np(*_jacobi(g, v, dev))
    c = g.shape[0]
    assert (np.diff(lam) <= 0).all()
    assert np.abs(a @ a.conj().T - np.eye(v)).max() <= 1e-6
    assert np.abs(a @ g @ a.conj().T - np.diag(lam[:v])).max() <= 1e-6 * lam[0]
    assert abs(info[2] - lam[:v].sum() / lam.sum()) <= 1e-12
    assert info[0] <= TOL and info[3] == lam[0] and tuple(a.shape) == (v, c)
    return a, lam, info


def test_all_eigenvalues_equal(dev):
    a, lam, info = _structure(3.0 * np.eye(7, dtype=np.complex128), 4, dev)
    assert (lam == 3.0).all() and info[1] == 0 and abs(info[2] - 4 / 7) <= 1e-12


def test_one_repeated_pair(dev):
    rs = np.random.RandomState(5)
    q, _ = np.linalg.qr(rs.standard_normal((9, 9)) + 1j * rs.standard_normal((9, 9)))
    ev = np.array([5.0, 4.0, 2.5, 2.5, 1.0, 0.5, 0.25, 0.1, 0.05])
    g = (q * ev) @ q.conj().T
    for v in (3, 4, 9):                                               # a split inside the pair, behind it, and V = c
        a, lam, _ = _structure(g, v, dev)
        assert np.abs(lam - ev).max() <= 1e-12 * ev[0]


# ------------------------------------------------------------------ edge inputs
def test_diagonal_input_orders_without_a_sweep(dev):
    d = np.array([2.0, 7.0, 0.5, 7.0, 3.0, 0.5, 9.0, 1.0, 7.0, 4.0, 6.0])          # ties at 7 (columns 1, 3, 8) and 0.5 (2, 5)
    a, lam, info = _np(*_jacobi(np.diag(d).astype(np.complex128), 6, dev))
    assert info[0] == 0.0 and info[1] == 0
    assert (lam == np.sort(d)[::-1]).all()
    want_cols = [6, 1, 3, 8, 10, 9]                                   # descending, equal values by column index
    want = np.zeros((6, 11), np.complex128)
    want[np.arange(6), want_cols] = 1.0
    assert (a == want).all()
    assert info[2] == (9.0 + 7.0 + 7.0 + 7.0 + 6.0 + 4.0) / d.sum() and info[3] == 9.0


def test_zero_matrix(dev):
    a, lam, info = _np(*_jacobi(np.zeros((6, 6), np.complex128), 3, dev))
    assert np.isfinite(a).all() and (np.abs((np.abs(a) ** 2).sum(axis=1) - 1.0) <= 1e-6).all()
    assert (lam == 0).all() and info[0] == 0.0 and info[2] == 1.0 and info[3] == 0.0


@pytest.mark.parametrize("where", [(2, 2), (1, 4)], ids=["diagonal", "off-diagonal"])
def test_nan_input_returns(dev, where):
    raw = designed_raw(2, 12, 12, 8, seed=3)
    g = gram_ref(raw, 2, 0)
    g[where] = np.nan
    a, lam, info = _jacobi(g, 4, dev)
    torch.cuda.synchronize()                                          # the call returns: bounded sweeps
    info = info.cpu().numpy()
    print(f"NaN at {where}: residual {info[0]}, sweeps {info[1]}")
    assert np.isnan(info[0]) or info[1] == SWEEP_CAP
    assert tuple(a.shape) == (4, 8) and tuple(lam.shape) == (8,)
    ok = _np(*_jacobi(gram_ref(raw, 2, 0), 4, dev))                   # and the device goes on working
    assert ok[2][0] <= TOL and np.isfinite(ok[0]).all()


def _grams(n, c, seed):
    return np.stack([gram_ref(designed_raw(2, 10, 10, c, seed=seed + j), 2, 0) for j in range(n)])


def test_batch_equals_single_calls_and_repeats_bit_for_bit(dev):
    from cine_hip import frontend as FE
    g = torch.from_numpy(_grams(3, 13, 20)).to(dev)
    a, lam, info = FE.coil_matrix_from_gram(g, 6, method="jacobi")
    assert tuple(a.shape) == (3, 6, 13) and tuple(lam.shape) == (3, 13) and tuple(info.shape) == (3, 4)
    assert not torch.equal(a[0], a[1])
    for j in range(3):
        aj, lj, ij = FE.coil_matrix_from_gram(g[j], 6, method="jacobi")
        assert torch.equal(torch.view_as_real(aj), torch.view_as_real(a[j])) and torch.equal(lj, lam[j]) and torch.equal(ij, info[j]), j
    for _ in range(3):
        a2, lam2, info2 = FE.coil_matrix_from_gram(g, 6, method="jacobi")
        assert torch.equal(torch.view_as_real(a2), torch.view_as_real(a)) and torch.equal(lam2, lam) and torch.equal(info2, info)
    # the default method on a stack: the stacked single results
    a_e, lam_e = FE.coil_matrix_from_gram(g, 6)
    for j in range(3):
        aj, lj = FE.coil_matrix_from_gram(g[j], 6)
        assert torch.equal(torch.view_as_real(aj), torch.view_as_real(a_e[j])) and torch.equal(lj, lam_e[j])


def test_lower_triangle_is_never_read(dev):
    g = _grams(1, 33, 40)[0]
    want = _jacobi(g, 12, dev)
    junk = g.copy()
    low = np.tril_indices(33, -1)
    junk[low] = np.random.RandomState(1).standard_normal(len(low[0])) * 1e3 + 1j * np.nan
    junk[np.diag_indices(33)] += 1j * 5.0                             # the diagonal's imaginary part is dropped too
    got = _jacobi(junk, 12, dev)
    for w, x in zip(want, got):
        assert torch.equal(torch.view_as_real(w) if w.is_complex() else w, torch.view_as_real(x) if x.is_complex() else x)


# ------------------------------------------------------------------ refusals, before any launch
def test_refusals(dev):
    from cine_hip import _lib, frontend as FE
    from cine_hip._lib import CineHipError
    L = _lib.lib()
    g, m, lam, info = (ctypes.c_void_p(p) for p in (0x1000, 0x2000, 0x3000, 0x4000))          # never dereferenced

    def call(g=g, m=m, lam=lam, info=info, nb=1, c=30, v=15):
        return L.cine_coil_matrix(g, m, lam, info, nb, c, v, None)

    assert call(c=65) == EUNSUPPORTED and b"64" in L.cine_last_error()
    assert call(c=64, v=33) == EUNSUPPORTED and b"32" in L.cine_last_error()
    assert call(v=0) == EINVAL and b"Invalid shapes" in L.cine_last_error()
    assert call(v=31) == EINVAL
    assert call(nb=0) == EINVAL and call(c=0, v=0) == EINVAL
    for kw in (dict(g=None), dict(m=None), dict(lam=None), dict(info=None)):
        assert call(**kw) == EINVAL and b"null" in L.cine_last_error(), kw
    assert call(m=g) == EINVAL and b"aliased" in L.cine_last_error()
    assert call(g=ctypes.c_void_p(0x1008)) == EINVAL and b"aligned" in L.cine_last_error()
    g65 = torch.eye(65, dtype=torch.complex128, device=dev)
    with pytest.raises(CineHipError, match="at most 64"):
        FE.coil_matrix_from_gram(g65, 15, method="jacobi")
    with pytest.raises(CineHipError, match="at most 32"):
        FE.coil_matrix_from_gram(g65[:64, :64].contiguous(), 33, method="jacobi")
    for v in (0, 65):
        with pytest.raises(ValueError, match="virtual_coils"):
            FE.coil_matrix_from_gram(g65[:64, :64].contiguous(), v, method="jacobi")
    with pytest.raises(ValueError, match="method"):
        FE.coil_matrix_from_gram(g65, 15, method="svd")
    a, _ = FE.coil_matrix_from_gram(g65, 15)                          # the default method still takes 65 coils
    assert tuple(a.shape) == (15, 65)


# ------------------------------------------------------------------ prepare_masked_slice(virtual_coils=V): composition, capture
def _mask(t, X, seed, dev):
    rs = np.random.RandomState(1000 + seed)
    m = (rs.uniform(size=(1, t, 1, X, 1, 1)) < 0.3).astype(np.uint8)
    m[:, :, :, X // 2 - 2:X // 2 + 2] = 1
    return torch.from_numpy(m).to(dev)


# the headline 30 -> 15 on sizes the line engines take, and one they refuse
CAPTURE = {"line": ((3, 40, 36, 30), (21, 17), 3, 15), "window": ((2, 416, 24, 6), (21, 17), 2, 4)}


@pytest.mark.parametrize("name", list(CAPTURE))
def test_prepare_masked_slice_virtual_coils_is_the_composition_and_capturable(dev, name):
    from cine_hip import frontend as FE, ops
    from cine_hip.pipeline import pipeline_streams
    shape, crop, n, v = CAPTURE[name]
    assert (ops.fft_line_supported(shape[1]) and ops.fft_line_supported(shape[2])) == (name == "line")
    raws = [torch.from_numpy(designed_raw(*shape, seed=60 + j) * np.float32(1e-6)).to(dev) for j in range(2)]
    mask = _mask(n, crop[0], 2, dev)
    want = []
    for r in raws:
        a = FE.coil_matrix_from_gram(FE.coil_gram(r, n, 24), v, method="jacobi")[0]
        want.append(FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, coil_matrix=a).clone())
        eager = FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, virtual_coils=v)
        assert tuple(eager.shape) == (1, n, v) + crop + (2,) and torch.equal(eager, want[-1])
        assert torch.equal(FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, coil_matrix=a, virtual_coils=v), want[-1])
        with pytest.raises(ValueError, match="rows"):
            FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, coil_matrix=a, virtual_coils=v - 1)
    assert not torch.equal(want[0], want[1])
    for bad in (0, shape[3] + 1):
        with pytest.raises(ValueError, match="virtual_coils"):
            FE.prepare_masked_slice(raws[0], mask, crop, n, FS, 1e6, virtual_coils=bad)
    static = torch.zeros_like(raws[0])
    s = pipeline_streams(dev, 1)[0][0]
    assert s != torch.cuda.default_stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        FE.prepare_masked_slice(static, mask, crop, n, FS, 1e6, virtual_coils=v)      # warm outside capture (a zero slice: finite)
    s.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        out = FE.prepare_masked_slice(static, mask, crop, n, FS, 1e6, virtual_coils=v)
    for j, r in enumerate(raws):
        static.copy_(r)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[j]), (name, j)


# ------------------------------------------------------------------ the default path keeps its bits
def test_default_method_changes_nothing(dev):
    """Without cc_method / method the eigen step is what it was: torch.linalg.eigh and the phase rule, written out here from public
    torch calls; prepare_slice(virtual_coils=V) is the composition of the public pieces with that matrix."""
    from cine_hip import frontend as FE
    raw = torch.from_numpy(designed_raw(3, 40, 36, 30, seed=109)).to(dev)
    v, crop = 15, (21, 17)
    g = FE.coil_gram(raw, 3, 24)
    ev, vec = torch.linalg.eigh(g)
    a = vec.flip(1)[:, :v].conj().transpose(0, 1).contiguous()
    mag = a.abs()
    idx = mag.argmax(dim=1, keepdim=True)
    peak = a.gather(1, idx)
    a = a * (peak.conj() / peak.abs())
    a.scatter_(1, idx, mag.gather(1, idx).to(a.dtype))
    a = a.to(torch.complex64)
    for got in (FE.coil_matrix_from_gram(g, v), FE.coil_matrix_from_gram(g, v, "eigh"), FE.coil_compression_matrix(raw, v, 3, 24)):
        assert len(got) == 2
        assert torch.equal(torch.view_as_real(got[0]), torch.view_as_real(a)) and torch.equal(got[1], ev.flip(0))
    want_k, want_f = FE.prepare_slice(FE.compress_coils(raw, a), crop, 3, FS)
    for kw in ({}, {"cc_method": "eigh"}):
        k, f = FE.prepare_slice(raw, crop, 3, FS, virtual_coils=v, **kw)
        assert torch.equal(k, want_k) and torch.equal(f, want_f), kw
    # cc_method="jacobi" goes through the kernel: the composition with ITS matrix
    a_j = FE.coil_matrix_from_gram(g, v, method="jacobi")[0]
    want_k, want_f = FE.prepare_slice(FE.compress_coils(raw, a_j), crop, 3, FS)
    k, f = FE.prepare_slice(raw, crop, 3, FS, virtual_coils=v, cc_method="jacobi")
    assert torch.equal(k, want_k) and torch.equal(f, want_f)
    with pytest.raises(ValueError, match="method"):
        FE.prepare_slice(raw, crop, 3, FS, virtual_coils=v, cc_method="qr")
