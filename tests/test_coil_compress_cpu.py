"""Coil compression of the front-end (cine_coil_gram / cine_coil_compress, frontend.coil_matrix_from_gram) on the host: the binding
table, argument validation before any launch, the workspace size, and the eigen step on CPU tensors against numpy.linalg.eigh.  Runs
without a GPU, through the loaded library."""
import ctypes

import numpy as np
import pytest
import torch

from cine_hip import _lib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAMES = ("cine_coil_gram_ws_bytes", "cine_coil_gram", "cine_coil_compress")


def test_symbols_are_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    L = _lib.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib._SIGS, name
    assert L.cine_version() == 3


def test_coil_gram_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    raw, gram, ws = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)   # never dereferenced
    big = 1 << 40
    args = dict(t_in=4, nx=40, ny=36, c=30, t_use=3, region=24)

    def call(r=raw, g=gram, w=ws, nbytes=big, **kw):
        a = dict(args, **kw)
        return L.cine_coil_gram(r, g, w, nbytes, a["t_in"], a["nx"], a["ny"], a["c"], a["t_use"], a["region"], None)

    assert call(r=None) == EINVAL and b"null" in L.cine_last_error()
    assert call(g=None) == EINVAL
    assert call(w=None) == EINVAL
    assert call(g=raw) == EINVAL and b"aliased" in L.cine_last_error()
    assert call(w=raw) == EINVAL
    assert call(w=gram) == EINVAL
    assert call(t_use=0) == EINVAL and b"Invalid shapes" in L.cine_last_error()
    assert call(t_use=5) == EINVAL
    assert call(t_in=0, t_use=0) == EINVAL
    assert call(region=-1) == EINVAL
    assert call(nx=0) == EINVAL
    assert call(ny=-2) == EINVAL
    assert call(c=0) == EINVAL
    assert call(r=ctypes.c_void_p(0x1008)) == EINVAL and b"16-byte" in L.cine_last_error()
    assert call(c=129) == EUNSUPPORTED and b"128" in L.cine_last_error()
    need = L.cine_coil_gram_ws_bytes(3, 40, 36, 30, 24)
    assert call(nbytes=need - 1) == EWORKSPACE and b"workspace" in L.cine_last_error()


def test_coil_compress_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    raw, mat, out = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    args = dict(t_in=4, nx=40, ny=36, c=30, t_out=3, v=15)

    def call(r=raw, m=mat, o=out, **kw):
        a = dict(args, **kw)
        return L.cine_coil_compress(r, m, o, a["t_in"], a["nx"], a["ny"], a["c"], a["t_out"], a["v"], None)

    assert call(r=None) == EINVAL and b"null" in L.cine_last_error()
    assert call(m=None) == EINVAL
    assert call(o=None) == EINVAL
    assert call(o=raw) == EINVAL and b"aliased" in L.cine_last_error()
    assert call(m=raw) == EINVAL
    assert call(o=mat) == EINVAL
    assert call(t_out=0) == EINVAL and b"Invalid shapes" in L.cine_last_error()
    assert call(t_out=5) == EINVAL
    assert call(nx=0) == EINVAL
    assert call(ny=0) == EINVAL
    assert call(c=0, v=0) == EINVAL
    assert call(v=0) == EINVAL
    assert call(v=31) == EINVAL                                        # more virtual coils than coils
    assert call(o=ctypes.c_void_p(0x3008)) == EINVAL and b"16-byte" in L.cine_last_error()
    assert call(c=129, v=15) == EUNSUPPORTED and b"128" in L.cine_last_error()
    assert call(c=64, v=33) == EUNSUPPORTED and b"32" in L.cine_last_error()


def test_coil_gram_workspace_depends_on_its_arguments_only():
    L = _lib.lib()
    f = L.cine_coil_gram_ws_bytes
    shapes = [(15, 416, 208, 30, 24), (3, 40, 36, 30, 24), (3, 33, 21, 34, 0), (1, 1, 1, 1, 0), (2, 24, 24, 128, 24), (25, 832, 416, 128, 0)]
    first = [f(*s) for s in shapes]
    assert all(b > 0 for b in first), first
    f(7, 100, 90, 12, 5)
    assert [f(*s) for s in shapes] == first
    for t, nx, ny, c, region in shapes:                               # at least one upper triangle of complex128 partial sums
        assert f(t, nx, ny, c, region) >= 16 * c * (c + 1) // 2
    assert f(15, 416, 208, 30, 0) >= f(15, 416, 208, 30, 24)
    for bad in ((0, 40, 36, 30, 24), (3, 0, 36, 30, 24), (3, 40, 0, 30, 24), (3, 40, 36, 0, 24), (3, 40, 36, 30, -1), (3, 40, 36, 129, 24)):
        assert f(*bad) == 0, bad


def _designed_gram(c, seed):
    """A Hermitian positive matrix with eigenvalues 1e-4^(i / (c - 1)) in a seeded random unitary basis."""
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c)))
    lam = 1e-4 ** (np.arange(c) / max(c - 1, 1))
    g = (q * lam) @ q.conj().T
    return (g + g.conj().T) / 2


@pytest.mark.parametrize("c,v", [(30, 15), (34, 12), (5, 5), (38, 1), (64, 32)])
def test_coil_matrix_from_gram_on_cpu_tensors_vs_numpy(c, v):
    from cine_hip import frontend as FE
    g = _designed_gram(c, seed=c + v)
    a, lam = FE.coil_matrix_from_gram(torch.from_numpy(g), v)
    assert a.dtype == torch.complex64 and tuple(a.shape) == (v, c) and lam.dtype == torch.float64 and tuple(lam.shape) == (c,)
    a, lam = a.numpy().astype(np.complex128), lam.numpy()
    ev, u = np.linalg.eigh(g)
    ev, u = ev[::-1], u[:, ::-1]
    assert (np.diff(lam) <= 0).all()
    assert np.abs(lam - ev).max() <= 1e-12 * ev[0]
    assert np.abs(a @ a.conj().T - np.eye(v)).max() <= 1e-6
    for r in range(v):
        k = int(np.argmax(np.abs(a[r])))
        assert a[r, k].real > 0 and a[r, k].imag == 0.0                # the phase rule
        assert abs(np.vdot(u[:, r].conj(), a[r])) >= 1 - 1e-6


def test_coil_matrix_from_gram_error_cases():
    from cine_hip import frontend as FE
    g = torch.from_numpy(_designed_gram(6, seed=1))
    with pytest.raises(ValueError, match="square"):
        FE.coil_matrix_from_gram(g[:, :5], 3)
    bad = g.clone()
    bad[0, 1] += 1e-6
    with pytest.raises(ValueError, match="Hermitian"):
        FE.coil_matrix_from_gram(bad, 3)
    for v in (0, 7, -1):
        with pytest.raises(ValueError, match="virtual_coils"):
            FE.coil_matrix_from_gram(g, v)
