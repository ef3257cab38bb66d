"""cine_noise_add_raw and its binding without a GPU: the ABI table carries the entry point, every refusal of the header returns its code,
names the entry point in cine_last_error() and comes before any launch (the pointers are never dereferenced), the flat pass's float
division is the integer one over its whole range, and the Python layer refuses CPU tensors, grad-requiring inputs and bad masks."""
import ctypes

import numpy as np
import pytest

from cine_hip import _lib

EINVAL, EUNSUPPORTED = -1, -2
NAME = "cine_noise_add_raw"
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]                      # never dereferenced


def test_symbol_is_declared_exported_and_bound():
    i, lg, f, p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    assert NAME in _lib.declared_symbols() and hasattr(_lib.lib(), NAME)
    assert _lib._SIGS[NAME] == (i, [p, p, p, i, p, f, lg, lg, p, lg, lg, i, i, i, p])
    assert _lib._SIGS[NAME] == _lib._SIGS["cine_noise_add"]                   # the same argument list, the sizes in another order


def test_noise_add_raw_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()

    def call(raw=P[0], out=P[1], mask=P[2], mask_ny=1, chol=P[3], scale=1.0, seed=5, replica=0, rdev=None, point0=0, t=2, nx=8, ny=6, c=4):
        return L.cine_noise_add_raw(raw, out, mask, mask_ny, chol, scale, seed, replica, rdev, point0, t, nx, ny, c, None)

    def refused(code, word=None, **kw):
        assert L.cine_scale(None, 1, 1.0, None) == EINVAL and L.cine_last_error().startswith(b"cine_scale")      # another call's message
        assert call(**kw) == code, kw
        msg = L.cine_last_error()
        assert msg.startswith(NAME.encode() + b":"), (kw, msg)
        assert word is None or word in msg, (kw, msg)

    refused(EUNSUPPORTED, b"64", c=65)
    refused(EUNSUPPORTED, b"64", c=128, chol=None)
    refused(EUNSUPPORTED, b"points", t=2 ** 40, nx=1024, ny=1024)              # beyond one workgroup per 64 points on the grid's x axis
    refused(EUNSUPPORTED, b"points", t=2 ** 62, nx=2 ** 30, ny=2 ** 30)        # and where t * nx * ny leaves the long
    refused(EINVAL, b"mask_ny", mask_ny=2)
    refused(EINVAL, b"mask_ny", mask_ny=2, mask=None)
    refused(EINVAL, b"mask_ny", mask_ny=0)
    refused(EINVAL, b"mask_ny", mask_ny=8)                                     # nx is not ny
    refused(EINVAL, b"replica", replica=-1)
    refused(EINVAL, b"replica", replica=2 ** 32)
    refused(EINVAL, b"point0", point0=-1)
    for kw in (dict(raw=None), dict(out=None)):
        refused(EINVAL, b"null", **kw)
    for kw in (dict(t=0), dict(c=0), dict(nx=0), dict(ny=-1), dict(t=-3)):
        refused(EINVAL, b"shapes", **kw)
    nbytes = 2 * 8 * 6 * 4 * 8
    refused(EINVAL, b"overlaps", out=ctypes.c_void_p(0x1000 + 8))
    refused(EINVAL, b"overlaps", out=ctypes.c_void_p(0x1000 + nbytes - 8))
    refused(EINVAL, b"overlaps", raw=ctypes.c_void_p(0x2000), out=ctypes.c_void_p(0x2000 - 8))
    refused(EINVAL, b"aligned", raw=ctypes.c_void_p(0x1004))
    refused(EINVAL, b"aligned", out=ctypes.c_void_p(0x2004))
    refused(EINVAL, b"aligned", chol=ctypes.c_void_p(0x4004))
    refused(EINVAL, b"aligned", rdev=ctypes.c_void_p(0x5004))


def test_the_flat_pass_divides_exactly():
    """The kernel finds the point of span element e as int((float(e) + 0.5f) * (1.0f / c)): equal to e // c for every e < 64 c, c <= 64."""
    for c in range(1, 65):
        e = np.arange(64 * c, dtype=np.int64)
        inv = np.float32(1.0) / np.float32(c)
        got = ((e.astype(np.float32) + np.float32(0.5)) * inv).astype(np.float32).astype(np.int64)
        assert np.array_equal(got, e // c), c


def test_python_layer_refuses_without_a_gpu_or_with_bad_arguments():
    import torch
    import cine_hip
    from cine_hip import noise as N
    from cine_hip._lib import CineHipError
    assert cine_hip.noise is N and "add_noise_raw" in N.__all__ and "pseudo_replica_raw" in N.__all__ and N.NOISE_MAX_COILS == 64
    with pytest.raises(CineHipError, match="no CPU fallback"):
        N.add_noise_raw(torch.zeros(2, 3, 4, 5, 2))
    with pytest.raises(CineHipError, match="no CPU fallback"):
        N.add_noise_raw(torch.zeros(2, 3, 4, 5, dtype=torch.complex64))
    with pytest.raises(CineHipError, match="requires grad"):
        N.add_noise_raw(torch.zeros(2, 3, 4, 5, 2, requires_grad=True))
    with pytest.raises(ValueError, match="expected"):
        N.add_noise_raw(torch.zeros(3, 4, 5, 2))
    with pytest.raises(CineHipError, match="complex64"):
        N.add_noise_raw(torch.zeros(2, 3, 4, 5, dtype=torch.complex128))
    with pytest.raises(ValueError, match="at least 2"):
        N.pseudo_replica_raw(None, torch.zeros(2, 3, 4, 5, 2), None, replicas=1)
    with pytest.raises(TypeError, match="unknown front-end keywords"):
        N.pseudo_replica_raw(None, torch.zeros(2, 3, 4, 5, 2), None, replicas=2, crop=(2, 2))
    with pytest.raises(ValueError, match="one"):
        N.pseudo_replica_raw(None, torch.zeros(2, 3, 4, 5, 2), None, replicas=2, n_frames=2, n_slices=2)


def test_pipeline_noise_mask_is_checked_against_the_kept_frames():
    import torch
    from cine_hip import noise as N
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import _check_noise_mask
    spec = N.NoiseSpec()
    assert _check_noise_mask(None, None, 4, 20, 14) == (None, None)
    with pytest.raises(CineHipError, match="without noise="):
        _check_noise_mask(torch.ones(4, 20, dtype=torch.uint8), None, 4, 20, 14)
    for shape in ((4, 20), (1, 20), (4, 20, 14), (1, 20, 14)):
        m, kind = _check_noise_mask(np.ones(shape, dtype=np.uint8), spec, 4, 20, 14)
        assert tuple(m.shape) == (4,) + shape[1:] and kind == "pageable" and m.dtype == torch.uint8 and m.is_contiguous()
    m, kind = _check_noise_mask(torch.ones(4, 20, dtype=torch.bool), spec, 4, 20, 14)
    assert m.dtype == torch.uint8
    for shape in ((6, 20), (4, 14), (4, 20, 13), (20,), (1, 1, 20, 14), (4, 16)):
        with pytest.raises(CineHipError, match="noise_mask: shape"):
            _check_noise_mask(torch.ones(shape, dtype=torch.uint8), spec, 4, 20, 14)
    with pytest.raises(CineHipError, match="uint8 or bool"):
        _check_noise_mask(torch.ones(4, 20), spec, 4, 20, 14)
