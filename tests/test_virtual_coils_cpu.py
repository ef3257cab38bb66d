"""Per-slice coil compression in flight, on the host: the binding of cine_coil_matrix and its argument validation before any launch,
the key of the graph set that serves ``submit_raw(..., virtual_coils=V)``, the validation of a raw slice's arguments, and the
``method`` / ``cc_method`` switch.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from cine_hip import _lib

EINVAL, EUNSUPPORTED = -1, -2


def test_symbol_is_declared_exported_and_bound():
    assert "cine_coil_matrix" in _lib.declared_symbols()
    assert hasattr(_lib.lib(), "cine_coil_matrix")
    res, args = _lib._SIGS["cine_coil_matrix"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p]


def test_coil_matrix_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    g, m, lam, info = (ctypes.c_void_p(p) for p in (0x1000, 0x2000, 0x3000, 0x4000))          # never dereferenced

    def call(g=g, m=m, lam=lam, info=info, nb=1, c=30, v=15):
        return L.cine_coil_matrix(g, m, lam, info, nb, c, v, None)

    for kw in (dict(g=None), dict(m=None), dict(lam=None), dict(info=None)):
        assert call(**kw) == EINVAL and b"null" in L.cine_last_error(), kw
    for kw in (dict(m=g), dict(lam=g), dict(info=g), dict(lam=m), dict(info=m), dict(info=lam)):
        assert call(**kw) == EINVAL and b"aliased" in L.cine_last_error(), kw
    assert call(nb=0) == EINVAL and b"Invalid shapes" in L.cine_last_error()
    assert call(c=0, v=0) == EINVAL
    assert call(v=0) == EINVAL and b"virtual coils 0" in L.cine_last_error()
    assert call(v=31) == EINVAL                                        # more virtual coils than coils
    assert call(c=65) == EUNSUPPORTED and b"at most 64" in L.cine_last_error()
    assert call(c=128, v=15) == EUNSUPPORTED
    assert call(c=64, v=33) == EUNSUPPORTED and b"at most 32" in L.cine_last_error()
    assert call(g=ctypes.c_void_p(0x1008)) == EINVAL and b"16-byte" in L.cine_last_error()
    assert call(m=ctypes.c_void_p(0x2004)) == EINVAL and call(lam=ctypes.c_void_p(0x3004)) == EINVAL and call(info=ctypes.c_void_p(0x4004)) == EINVAL


KW = dict(n_frames=15, crop_shape=(200, 200), filter_size=(0.7, 0.0, 0.3, 0.3), scaling=1e6, apply_mask=True,
          mask_shape=(1, 15, 1, 200, 1, 1), sens_shape=None)


def test_raw_set_key_with_virtual_coils():
    from cine_hip.pipeline import espirit_key, raw_set_key
    k20 = raw_set_key((25, 384, 144, 20), virtual_coils=(15, 24), **KW)
    k30 = raw_set_key((25, 384, 144, 30), virtual_coils=(15, 24), **KW)
    assert k20 == k30 and hash(k20) is not None and 20 not in k20[1] and 30 not in k30[1]           # the coil count stays out
    assert raw_set_key((25, 384, 144, 30), virtual_coils=(12, 24), **KW) != k30                     # V is in
    assert raw_set_key((25, 384, 144, 30), virtual_coils=(15, 0), **KW) != k30                      # the region is in
    assert raw_set_key((25, 384, 144, 30), virtual_coils=[15, 24], **KW) == k30
    assert raw_set_key((25, 384, 160, 30), virtual_coils=(15, 24), **KW) != k30
    # a set that computes its matrix is not the set that is handed one, nor the uncompressed set of V coils
    assert raw_set_key((25, 384, 144, 30), coil_matrix_shape=(15, 30), **KW) != k30
    assert raw_set_key((25, 384, 144, 15), **KW) != k30
    assert raw_set_key((25, 384, 144, 30), virtual_coils=(15, 24), espirit=espirit_key(15, 60), **KW) != k30
    with pytest.raises(ValueError, match="not both"):
        raw_set_key((25, 384, 144, 30), coil_matrix_shape=(15, 30), virtual_coils=(15, 24), **KW)
    # without the keyword the keys are what they were: the 9-tuple written out
    want = ("raw", (15, 384, 144, 15), None, (200, 200), (0.7, 0.0, 0.3, 0.3), 1e6, True, (1, 15, 1, 200, 1, 1), None)
    assert raw_set_key((25, 384, 144, 15), **KW) == raw_set_key((25, 384, 144, 15), virtual_coils=None, **KW) == want
    want_cm = ("raw", (15, 384, 144), 12, (200, 200), (0.7, 0.0, 0.3, 0.3), 1e6, True, (1, 15, 1, 200, 1, 1), None)
    assert raw_set_key((25, 384, 144, 20), coil_matrix_shape=(12, 20), **KW) == want_cm
    assert k30[:9] == ("raw", (15, 384, 144), 15) + want[3:] and k30[9:] == (("virtual", 15, 24),)


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


def test_raw_source_validation():
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import raw_set_key
    s = _source(virtual_coils=6)
    assert (s.vc, s.cc_region, s.v, s.cmat, s.cmat_shape) == (6, 24, 6, None, (6, 12, 2)) and s.mk_shape == (1, 5, 6, 24, 20, 2)
    assert s.key == raw_set_key((5, 30, 28, 12), 5, (24, 20), (0.7, 0.0, 0.3, 0.3), 1e6, True, s.mask_shape, None, virtual_coils=(6, 24))
    assert _source(c=20, virtual_coils=6).key == s.key and _source(virtual_coils=6, cc_region=0).key != s.key
    assert _source(c=64, virtual_coils=32).v == 32 and _source(c=1, virtual_coils=1).v == 1 and _source(virtual_coils=12).v == 12
    plain = _source()
    assert (plain.vc, plain.v) == (None, None) and len(plain.key) == 9
    a = np.zeros((6, 12), np.complex64)
    assert _source(coil_matrix=a).vc is None
    with pytest.raises(CineHipError, match="one of the two"):
        _source(virtual_coils=6, coil_matrix=a)
    for v in (0, -3, 13, 2.0, "6", True):
        with pytest.raises(CineHipError, match="virtual_coils"):
            _source(virtual_coils=v)
    with pytest.raises(CineHipError, match="at most 32"):
        _source(c=40, virtual_coils=33)
    for region in (-1, 2.5, None):
        with pytest.raises(CineHipError, match="cc_region"):
            _source(virtual_coils=6, cc_region=region)
    with pytest.raises(CineHipError, match="65 coils.*at most 64.*coil_matrix="):
        _source(c=65, virtual_coils=6)
    assert _source(c=65, coil_matrix=np.zeros((6, 65), np.complex64)).v == 6           # coil_matrix= still serves such scans


def test_unknown_method_raises():
    from cine_hip import frontend as FE
    g = torch.eye(4, dtype=torch.complex128)
    with pytest.raises(ValueError, match="method"):
        FE.coil_matrix_from_gram(g, 2, method="svd")
    with pytest.raises(ValueError, match="method"):
        FE.coil_matrix_from_gram(g, 2, "Jacobi")
    with pytest.raises(ValueError, match="method"):
        FE._compressed(torch.zeros(2, 4, 4, 4, dtype=torch.complex64), 2, 2, None, 24, "qr")
    a, lam = FE.coil_matrix_from_gram(g, 2)                            # the default is "eigh", and runs where the tensor lives
    a2, lam2 = FE.coil_matrix_from_gram(g, 2, "eigh")
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(a2)) and torch.equal(lam, lam2)
    stack_a, stack_lam = FE.coil_matrix_from_gram(torch.stack([g, 2 * g]), 2)
    assert tuple(stack_a.shape) == (2, 2, 4) and torch.equal(stack_lam[1], 2 * lam)
    with pytest.raises(FE.CineHipError, match="GPU"):
        FE.coil_matrix_from_gram(g, 2, method="jacobi")                # no CPU fallback
