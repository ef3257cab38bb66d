"""Noise pre-whitening folded into the coil-compression matrix, on the host: the binding of cine_coil_matrix_whitened and its argument
validation before any launch, the set key and the argument rules of ``submit_raw(..., whitener=W)``, and ``noise_whitener(cov=)`` /
``coil_matrix_from_gram(..., method="eigh", whitener=W)`` on CPU tensors against the float64 restatement of tests/whitening_ref.py on
its designed inputs, to the bars of the GPU parity test.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from cine_hip import _lib
from whitening_ref import CASES, IDS, check_against_ref, designed_case, whitener_ref

EINVAL, EUNSUPPORTED = -1, -2


def test_symbol_is_declared_exported_and_bound():
    assert "cine_coil_matrix_whitened" in _lib.declared_symbols()
    assert hasattr(_lib.lib(), "cine_coil_matrix_whitened")
    res, args = _lib._SIGS["cine_coil_matrix_whitened"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p]


def test_whitened_matrix_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    g, w, m, lam, info = (ctypes.c_void_p(p) for p in (0x1000, 0x5000, 0x2000, 0x3000, 0x4000))          # never dereferenced

    def call(g=g, w=w, m=m, lam=lam, info=info, nb=1, c=30, v=15):
        return L.cine_coil_matrix_whitened(g, w, m, lam, info, nb, c, v, None)

    for kw in (dict(g=None), dict(w=None), dict(m=None), dict(lam=None), dict(info=None)):
        assert call(**kw) == EINVAL and b"null" in L.cine_last_error(), kw
    for kw in (dict(m=g), dict(lam=g), dict(info=g), dict(lam=m), dict(info=m), dict(info=lam), dict(w=g), dict(m=w), dict(lam=w),
               dict(info=w)):
        assert call(**kw) == EINVAL and b"aliased" in L.cine_last_error(), kw
    assert call(nb=0) == EINVAL and b"Invalid shapes" in L.cine_last_error()
    assert call(c=0, v=0) == EINVAL
    assert call(v=0) == EINVAL and b"virtual coils 0" in L.cine_last_error()
    assert call(v=31) == EINVAL                                        # more virtual coils than coils
    assert call(c=65) == EUNSUPPORTED and b"at most 64" in L.cine_last_error() and b"cine_coil_matrix_whitened" in L.cine_last_error()
    assert call(c=128, v=15) == EUNSUPPORTED
    assert call(c=64, v=33) == EUNSUPPORTED and b"at most 32" in L.cine_last_error()
    assert call(g=ctypes.c_void_p(0x1008)) == EINVAL and b"16-byte" in L.cine_last_error()
    assert call(w=ctypes.c_void_p(0x5008)) == EINVAL and b"16-byte" in L.cine_last_error()
    assert call(m=ctypes.c_void_p(0x2004)) == EINVAL and call(lam=ctypes.c_void_p(0x3004)) == EINVAL and call(info=ctypes.c_void_p(0x4004)) == EINVAL


# ------------------------------------------------------------------ the set key and the argument rules of submit_raw
KW = dict(n_frames=15, crop_shape=(200, 200), filter_size=(0.7, 0.0, 0.3, 0.3), scaling=1e6, apply_mask=True,
          mask_shape=(1, 15, 1, 200, 1, 1), sens_shape=None)


def test_raw_set_key_with_a_whitener():
    from cine_hip.pipeline import raw_set_key
    plain = raw_set_key((25, 384, 144, 30), virtual_coils=(15, 24), **KW)
    k20 = raw_set_key((25, 384, 144, 20), virtual_coils=(15, 24), whitened=True, **KW)
    k30 = raw_set_key((25, 384, 144, 30), virtual_coils=(15, 24), whitened=True, **KW)
    assert k20 == k30 and hash(k30) is not None and 20 not in k20[1] and 30 not in k30[1]           # the coil count stays out
    assert k30 != plain and k30[:9] == plain[:9] and k30[9:] == (("virtual", 15, 24, "whitened"),)
    # every key without the new argument is what it was
    assert plain[9:] == (("virtual", 15, 24),)
    assert raw_set_key((25, 384, 144, 30), virtual_coils=(15, 24), whitened=False, **KW) == plain
    want = ("raw", (15, 384, 144, 15), None, (200, 200), (0.7, 0.0, 0.3, 0.3), 1e6, True, (1, 15, 1, 200, 1, 1), None)
    assert raw_set_key((25, 384, 144, 15), **KW) == want
    want_cm = ("raw", (15, 384, 144), 12, (200, 200), (0.7, 0.0, 0.3, 0.3), 1e6, True, (1, 15, 1, 200, 1, 1), None)
    assert raw_set_key((25, 384, 144, 20), coil_matrix_shape=(12, 20), **KW) == want_cm
    with pytest.raises(ValueError, match="whitened"):
        raw_set_key((25, 384, 144, 30), whitened=True, **KW)
    with pytest.raises(ValueError, match="whitened"):
        raw_set_key((25, 384, 144, 30), coil_matrix_shape=(15, 30), whitened=True, **KW)


class _Pipe:
    """What _RawSource asks of its pipeline."""
    _takes_sens, _needs_sens, model, device = False, False, None, torch.device("cpu")


def _source(c=12, **kw):
    from cine_hip.pipeline import _RawSource
    raw = np.zeros((6, 30, 28, c), np.complex64)
    mask = np.ones((1, 5, 1, 24, 1, 1), np.uint8)
    args = dict(crop_shape=(24, 20), n_frames=5, filter_size=(0.7, 0.0, 0.3, 0.3), scaling=1e6, coil_matrix=None, apply_mask=True)
    args.update(kw)
    return _RawSource(_Pipe(), raw, mask, None, **args)


def test_raw_source_with_a_whitener():
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import raw_set_key
    w = np.tril(np.arange(144).reshape(12, 12) + 1.0).astype(np.complex128)
    base = ((5, 30, 28, 12), 5, (24, 20), (0.7, 0.0, 0.3, 0.3), 1e6, True)
    s = _source(virtual_coils=6, whitener=w)
    assert (s.vc, s.v, s.cmat, s.cmat_shape) == (6, 6, None, (6, 12, 2)) and s.mk_shape == (1, 5, 6, 24, 20, 2)
    assert s.wh.dtype == torch.float64 and tuple(s.wh.shape) == (12, 12, 2) and s.wh_kind == "pageable"
    assert np.array_equal(torch.view_as_complex(s.wh).numpy(), w)
    assert s.key == raw_set_key(*base, s.mask_shape, None, virtual_coils=(6, 24), whitened=True)
    assert s.key != _source(virtual_coils=6).key and _source(virtual_coils=6).wh is None
    assert _source(c=20, virtual_coils=6, whitener=np.eye(20, dtype=np.complex128)).key == s.key              # the coil count stays out
    assert _source(virtual_coils=6, whitener=torch.from_numpy(w).pin_memory() if torch.cuda.is_available() else torch.from_numpy(w)).key == s.key
    assert _source(virtual_coils=12, whitener=w).v == 12                                                      # V == c is served
    # the whitener alone is the coil matrix W.to(complex64)
    alone = _source(whitener=w)
    assert alone.vc is None and alone.wh is None and alone.v == 12
    assert alone.key == _source(coil_matrix=w.astype(np.complex64)).key
    assert torch.equal(alone.cmat, torch.view_as_real(torch.from_numpy(w).to(torch.complex64)))
    with pytest.raises(CineHipError, match="virtual_coils="):
        _source(c=40, whitener=np.eye(40, dtype=np.complex128))
    with pytest.raises(CineHipError, match=r"coil_matrix_from_gram\(\.\.\., whitener=W\)"):
        _source(whitener=w, coil_matrix=np.zeros((6, 12), np.complex64))
    with pytest.raises(CineHipError, match=r"coil_matrix_from_gram\(\.\.\., whitener=W\)"):
        _source(virtual_coils=6, whitener=w, coil_matrix=np.zeros((6, 12), np.complex64))
    with pytest.raises(CineHipError, match="shape"):
        _source(virtual_coils=6, whitener=w[:11, :11])
    with pytest.raises(CineHipError, match="complex128"):
        _source(virtual_coils=6, whitener=w.astype(np.complex64))
    with pytest.raises(CineHipError, match="complex128"):
        _source(virtual_coils=6, whitener=torch.from_numpy(w).to(torch.complex64))
    with pytest.raises(CineHipError, match="whitener"):
        _source(virtual_coils=6, whitener=[[1.0]])


# ------------------------------------------------------------------ noise_whitener and the "eigh" method against numpy, on CPU tensors
@pytest.mark.parametrize("c,v,seed", CASES, ids=IDS)
def test_whitener_and_eigh_matrix_on_cpu_tensors_vs_float64(c, v, seed):
    from cine_hip import frontend as FE
    case = designed_case(c, v, seed)                                  # asserts the gaps of the whitened Gram matrix
    psi = torch.from_numpy(case["psi"].copy())
    w = FE.noise_whitener(cov=psi)
    assert w.dtype == torch.complex128 and tuple(w.shape) == (c, c) and w.device.type == "cpu"
    wn = w.numpy()
    assert (np.triu(wn, 1) == 0).all() and (wn.diagonal().imag == 0).all() and (wn.diagonal().real > 0).all()
    # W is the inverse of a factor of condition 10: float64 rounding times a small multiple of that
    assert np.abs(wn - case["w"]).max() <= 1e-12 * np.abs(case["w"]).max()
    assert np.abs(wn @ case["psi"] @ wn.conj().T / case["s"] ** 2 - np.eye(c)).max() <= 1e-12
    w1 = FE.noise_whitener(cov=psi, preserve_scale=False).numpy()
    assert np.abs(w1 - whitener_ref(case["psi"], False)[0]).max() <= 1e-12 * np.abs(w1).max()
    assert np.abs(w1 @ case["psi"] @ w1.conj().T - np.eye(c)).max() <= 1e-12
    g = torch.from_numpy(case["gram"].copy())
    a, lam = FE.coil_matrix_from_gram(g, v, method="eigh", whitener=w)
    assert a.dtype == torch.complex64 and tuple(a.shape) == (v, c) and lam.dtype == torch.float64 and tuple(lam.shape) == (c,)
    check_against_ref(a.numpy().astype(np.complex128), lam.numpy(), case, v, f"eigh on the CPU {c} -> {v}")
    # only the lower triangle of W is used, its diagonal taken as real
    junk_w = w + torch.triu(torch.full((c, c), complex(3.0, float("nan")), dtype=torch.complex128), 1) + 2j * torch.eye(c, dtype=torch.complex128)
    a2, lam2 = FE.coil_matrix_from_gram(g, v, method="eigh", whitener=junk_w)
    assert torch.equal(torch.view_as_real(a2), torch.view_as_real(a)) and torch.equal(lam2, lam)


def test_eigh_without_a_whitener_is_unchanged_and_stacks_pass_it_on():
    """whitener=None is today's path: torch.linalg.eigh and the phase rule, written out from public torch calls."""
    from cine_hip import frontend as FE
    case = designed_case(5, 5, 10)
    g = torch.from_numpy(case["gram"].copy())
    ev, vec = torch.linalg.eigh(g)
    a = vec.flip(1)[:, :3].conj().transpose(0, 1).contiguous()
    mag = a.abs()
    idx = mag.argmax(dim=1, keepdim=True)
    peak = a.gather(1, idx)
    a = a * (peak.conj() / peak.abs())
    a.scatter_(1, idx, mag.gather(1, idx).to(a.dtype))
    for got in (FE.coil_matrix_from_gram(g, 3), FE.coil_matrix_from_gram(g, 3, "eigh", None)):
        assert torch.equal(torch.view_as_real(got[0]), torch.view_as_real(a.to(torch.complex64))) and torch.equal(got[1], ev.flip(0))
    w = torch.from_numpy(case["w"].copy())
    one = FE.coil_matrix_from_gram(g, 3, whitener=w)
    stack = FE.coil_matrix_from_gram(torch.stack([g, 2 * g]), 3, whitener=w)
    assert tuple(stack[0].shape) == (2, 3, 5) and torch.equal(torch.view_as_real(stack[0][0]), torch.view_as_real(one[0]))
    assert not torch.equal(torch.view_as_real(one[0]), torch.view_as_real(a.to(torch.complex64)))
    with pytest.raises(ValueError, match="whitener"):
        FE.coil_matrix_from_gram(g, 3, whitener=w[:4, :4])
    with pytest.raises(FE.CineHipError, match="GPU"):
        FE.coil_matrix_from_gram(g, 3, method="jacobi", whitener=w)  # no CPU fallback


# ------------------------------------------------------------------ refusals
def test_rank_deficient_covariance_raises():
    from cine_hip import frontend as FE
    rs = np.random.RandomState(7)
    for n, c in ((5, 8), (11, 12), (1, 2)):                           # fewer noise samples than coils
        eta = rs.standard_normal((n, c)) + 1j * rs.standard_normal((n, c))
        psi = torch.from_numpy(eta.T @ eta.conj() / n)
        with pytest.raises(ValueError, match="too few noise samples"):
            FE.noise_whitener(cov=psi)
    eta = rs.standard_normal((64, 8)) + 1j * rs.standard_normal((64, 8))
    psi = torch.from_numpy(eta.T @ eta.conj() / 64)
    assert tuple(FE.noise_whitener(cov=psi).shape) == (8, 8)          # enough samples: served
    bad = psi.clone()
    bad[2, 2] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        FE.noise_whitener(cov=bad)
    with pytest.raises(ValueError, match="positive definite"):
        FE.noise_whitener(cov=-psi)
    with pytest.raises(ValueError, match="one of the two"):
        FE.noise_whitener()
    with pytest.raises(ValueError, match="one of the two"):
        FE.noise_whitener(torch.zeros(4, 2, dtype=torch.complex64), cov=psi)
    with pytest.raises(ValueError, match="square"):
        FE.noise_whitener(cov=psi[:, :5])
    with pytest.raises(FE.CineHipError, match="GPU"):
        FE.noise_whitener(torch.zeros(40, 4, dtype=torch.complex64))  # the covariance of samples is cine_coil_gram: no CPU fallback


def test_whitener_with_a_coil_matrix_raises():
    from cine_hip import frontend as FE
    raw = torch.zeros(2, 4, 4, 4, dtype=torch.complex64)
    w = torch.eye(4, dtype=torch.complex128)
    a = torch.zeros(2, 4, dtype=torch.complex64)
    with pytest.raises(ValueError, match=r"coil_matrix_from_gram\(\.\.\., whitener=W\)"):
        FE._compressed(raw, 2, None, a, 24, "eigh", w)
    with pytest.raises(ValueError, match=r"coil_matrix_from_gram\(\.\.\., whitener=W\)"):
        FE._compressed(raw, 2, 2, a, 24, "eigh", w)
    with pytest.raises(FE.CineHipError, match="virtual_coils="):
        FE._compressed(torch.zeros(2, 4, 4, 40, dtype=torch.complex64), 2, None, None, 24, "eigh", torch.eye(40, dtype=torch.complex128))
    import inspect
    for f in (FE.prepare_slice, FE.prepare_example, FE.prepare_masked_slice):
        assert list(inspect.signature(f).parameters)[-1] == "whitener" and inspect.signature(f).parameters["whitener"].default is None
