"""The raw-input path of the pipeline on the host: the binding of cine_raw_ingest and its argument validation before any launch, through
the loaded library, and the pure-Python key of the graph set that serves a ``submit_raw`` call.  Runs without a GPU."""
import ctypes

import pytest

from cine_hip import _lib

EINVAL, EUNSUPPORTED = -1, -2


def test_symbol_is_declared_exported_and_bound():
    assert "cine_raw_ingest" in _lib.declared_symbols()
    assert hasattr(_lib.lib(), "cine_raw_ingest")
    assert "cine_raw_ingest" in _lib._SIGS


def test_raw_ingest_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    raw, out = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)       # never dereferenced
    args = dict(t_in=4, nx=40, ny=36, c=30, t_out=3)

    def call(r=raw, o=out, **kw):
        a = dict(args, **kw)
        return L.cine_raw_ingest(r, o, a["t_in"], a["nx"], a["ny"], a["c"], a["t_out"], 1.0, None)

    assert call(r=None) == EINVAL and b"null" in L.cine_last_error()
    assert call(o=None) == EINVAL and b"cine_raw_ingest" in L.cine_last_error()
    assert call(o=raw) == EINVAL and b"aliased" in L.cine_last_error()
    assert call(t_out=0) == EINVAL and b"Invalid shapes" in L.cine_last_error() and b"t_out 0" in L.cine_last_error()
    assert call(t_out=5) == EINVAL and b"t_out 5" in L.cine_last_error()           # more frames than the scan holds
    assert call(t_in=0, t_out=0) == EINVAL
    assert call(nx=0) == EINVAL and b"nx 0" in L.cine_last_error()
    assert call(ny=-2) == EINVAL and b"ny -2" in L.cine_last_error()
    assert call(c=0) == EINVAL and b"coils 0" in L.cine_last_error()
    assert call(r=ctypes.c_void_p(0x1008)) == EINVAL and b"16-byte" in L.cine_last_error()
    assert call(o=ctypes.c_void_p(0x2004)) == EINVAL and b"16-byte" in L.cine_last_error()
    assert call(t_in=40000, t_out=40000, nx=4096, ny=4096, c=1) == EUNSUPPORTED and b"grid limit" in L.cine_last_error()
    assert call(c=4000) == EUNSUPPORTED and b"LDS" in L.cine_last_error()


KW = dict(n_frames=15, crop_shape=(200, 200), filter_size=(0.7, 0.0, 0.3, 0.3), scaling=1e6, apply_mask=True,
          mask_shape=(1, 15, 1, 200, 1, 1), sens_shape=None)


def test_raw_set_key():
    from cine_hip.pipeline import raw_set_key
    base = raw_set_key((25, 384, 144, 15), **KW)
    assert base == raw_set_key((25, 384, 144, 15), **KW)
    assert base == raw_set_key((15, 384, 144, 15), **dict(KW, filter_size=[0.7, 0, 0.3, 0.3], crop_shape=[200, 200], scaling=1000000))
    assert base == raw_set_key((40, 384, 144, 15), **KW)                               # frames past the kept ones are never copied
    assert hash(base) is not None and base[0] == "raw"
    for change in (dict(n_frames=12), dict(crop_shape=(200, 144)), dict(filter_size=(0.7, 0.0, 0.3, 0.0)), dict(scaling=1.0),
                   dict(apply_mask=False), dict(mask_shape=(1, 15, 1, 200, 200, 1)), dict(sens_shape=(1, 1, 15, 200, 200, 2))):
        assert raw_set_key((25, 384, 144, 15), **dict(KW, **change)) != base, change
    for shape in ((25, 384, 144, 16), (25, 384, 160, 15), (25, 416, 144, 15), (9, 384, 144, 15)):
        assert raw_set_key(shape, **KW) != base, shape
    # with a coil matrix the coil count of the scan is not in the key, the number of virtual coils is
    k20 = raw_set_key((25, 384, 144, 20), coil_matrix_shape=(12, 20), **KW)
    k30 = raw_set_key((25, 384, 144, 30), coil_matrix_shape=(12, 30), **KW)
    assert k20 == k30 and 20 not in k20[1] and 30 not in k30[1]
    assert raw_set_key((25, 384, 144, 30), coil_matrix_shape=(15, 30), **KW) != k30
    assert raw_set_key((25, 384, 144, 12), **KW) != raw_set_key((25, 384, 144, 20), coil_matrix_shape=(12, 20), **KW)
    with pytest.raises(ValueError, match="Invalid shapes."):
        raw_set_key((25, 384, 144, 15), **dict(KW, n_frames=0))


def test_a_change_of_kind_changes_the_key():
    """``submit`` keys its sets by (k-space shape, mask shape, sens shape); the key of a raw set never equals one of those."""
    from cine_hip.pipeline import raw_set_key
    kspace_key = ((1, 15, 15, 200, 200, 2), (1, 15, 1, 200, 1, 1), None)
    raw_key = raw_set_key((15, 200, 200, 15), **KW)
    assert raw_key != kspace_key and raw_key[0] == "raw" and kspace_key[0] != "raw"
