"""Masks that vary along w, on the host: the binding of cine_image_dc_general / cine_normal_op_general / cine_apply_mask2d, their argument
validation before any launch through the loaded library, the workspace formula, the switch ops.GENERAL_MASK_FUSED, and what
SlicePipeline's input validation (_Source, _RawSource) accepts and refuses for such masks.  Runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from cine_hip import _lib
from cine_hip._lib import CineHipError

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAMES = ("cine_image_dc_general_ws_bytes", "cine_image_dc_general", "cine_normal_op_general", "cine_apply_mask2d")


def test_symbols_are_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    L = _lib.lib()
    for name in NAMES:
        assert name in declared and hasattr(L, name) and name in _lib._SIGS, name


def test_the_workspace_is_the_hybrid_space_coil_images():
    L = _lib.lib()
    for b, t, c, h, w in ((1, 15, 15, 200, 200), (2, 3, 17, 7, 13), (1, 1, 1, 1, 1), (1, 3, 12000, 4, 2), (1, 1, 2, 512, 480)):
        assert L.cine_image_dc_general_ws_bytes(b, t, c, h, w) == b * t * c * h * w * 8
    for bad in ((0, 1, 1, 8, 8), (1, 0, 1, 8, 8), (1, 1, 0, 8, 8), (1, 1, 1, -1, 8), (1, 1, 1, 8, 0)):
        assert L.cine_image_dc_general_ws_bytes(*bad) == 0
    assert L.cine_image_dc_general_ws_bytes(4, 25, 32, 512, 512) == 4 * 25 * 32 * 512 * 512 * 8          # above 2^32: size_t


def test_image_dc_general_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = {k: ctypes.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(("img", "sens", "zf", "mask", "lam", "out", "ws"))}   # never dereferenced
    args = dict(b=1, t=3, c=4, h=24, w=20, magnitude=0)

    def call(nbytes=1 << 40, **kw):
        a = dict(args, **p)
        a.update(kw)
        return L.cine_image_dc_general(a["img"], a["sens"], a["zf"], a["mask"], a["lam"], 1.0, 0.0, 0.0, a["out"], a["b"], a["t"], a["c"], a["h"], a["w"],
                                       a["magnitude"], a["ws"], nbytes, None)

    for name in ("img", "sens", "mask", "out", "ws"):
        assert call(**{name: None}) == EINVAL and L.cine_last_error().startswith(b"cine_image_dc_general") and b"null" in L.cine_last_error(), name
    assert call(out=p["img"]) == EINVAL and b"alias" in L.cine_last_error()
    for name in ("b", "t", "c", "h", "w"):
        assert call(**{name: 0}) == EINVAL, name
    assert call(c=32769) == EINVAL
    assert call(b=256, t=256) == EUNSUPPORTED and b"65535" in L.cine_last_error()
    assert call(h=401) == EUNSUPPORTED and b"401" in L.cine_last_error()
    assert call(w=401) == EUNSUPPORTED
    assert call(h=514) == EUNSUPPORTED
    need = L.cine_image_dc_general_ws_bytes(1, 3, 4, 24, 20)
    assert call(nbytes=need - 1) == EWORKSPACE and b"workspace" in L.cine_last_error()
    assert call(nbytes=0) == EWORKSPACE


def test_normal_op_general_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = {k: ctypes.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(("img", "sens", "mask", "lam", "out", "ws"))}
    args = dict(b=1, t=3, c=4, h=200, w=20)

    def call(nbytes=1 << 40, **kw):
        a = dict(args, **p)
        a.update(kw)
        return L.cine_normal_op_general(a["img"], a["sens"], a["mask"], a["lam"], a["out"], a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"], nbytes, None)

    for name in ("img", "sens", "mask", "lam", "out", "ws"):
        assert call(**{name: None}) == EINVAL and L.cine_last_error().startswith(b"cine_normal_op_general"), name
    assert call(out=p["img"]) == EINVAL
    assert call(t=0) == EINVAL
    assert call(b=65536, t=1) == EUNSUPPORTED
    assert call(w=401) == EUNSUPPORTED
    assert call(nbytes=L.cine_image_dc_general_ws_bytes(1, 3, 4, 200, 20) - 1) == EWORKSPACE


def test_apply_mask2d_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    k, m, o = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    assert L.cine_apply_mask2d(None, m, o, 2, 3, 8, 6, None) == EINVAL and L.cine_last_error().startswith(b"cine_apply_mask2d")
    assert L.cine_apply_mask2d(k, None, o, 2, 3, 8, 6, None) == EINVAL
    assert L.cine_apply_mask2d(k, m, None, 2, 3, 8, 6, None) == EINVAL
    for bt, c, h, w in ((0, 3, 8, 6), (2, 0, 8, 6), (2, 3, 0, 6), (2, 3, 8, 0), (256, 256, 8, 6)):
        assert L.cine_apply_mask2d(k, m, o, bt, c, h, w, None) == EINVAL, (bt, c, h, w)


def test_the_counter_of_mask_plane_column_passes_exists():
    L = _lib.lib()
    assert L.cine_diag_counter(15, 0) >= 0 and L.cine_diag_counter(16, 0) == -1


def test_the_switch_and_the_layout_predicates():
    from cine_hip import ops
    assert ops.GENERAL_MASK_FUSED is True
    ks = torch.zeros(1, 3, 2, 8, 6, 2)
    row, general = torch.zeros(1, 3, 1, 8, 1, 1, dtype=torch.uint8), torch.zeros(1, 3, 1, 8, 6, 1, dtype=torch.uint8)
    assert ops.general_mask_fused(general, ks) and not ops.general_mask_fused(row, ks)
    old = ops.GENERAL_MASK_FUSED
    try:
        ops.GENERAL_MASK_FUSED = False
        assert not ops.general_mask_fused(general, ks)
    finally:
        ops.GENERAL_MASK_FUSED = old
    assert ops.as_mask_u8(general, ks) is general


def test_as_mask_u8_returns_the_row_layout_or_the_general_layout_and_nothing_else(monkeypatch):
    """What lets the models' data consistency (cine_hip/dc.py) dispatch on two layouts only: for every mask that broadcasts as
    (b|1, t|1, 1, h, w|1, 1), of every accepted dtype, the result is exactly (b, t, 1, h, 1, 1) or -- only with w > 1 -- (b, t, 1, h, w, 1);
    any other shape raises."""
    import itertools
    from cine_hip import ops
    from cine_hip.dc import Acquisition
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)      # (as_mask_u8 asks before it converts; the question needs a device)
    for (b, t, h, w), dtype in itertools.product(((1, 3, 8, 6), (2, 3, 8, 6), (2, 1, 5, 1), (1, 1, 1, 1), (3, 2, 4, 2)),
                                                 (torch.uint8, torch.bool, torch.int32, torch.int64, torch.float16, torch.float32, torch.float64)):
        ks = torch.zeros(b, t, 2, h, w, 2)
        for mb, mt, mw in itertools.product({1, b}, {1, t}, {1, w}):
            g = torch.Generator().manual_seed(mb * 100 + mt * 10 + mw)
            src = torch.rand(mb, mt, 1, h, mw, 1, generator=g) < 0.5
            out = ops.as_mask_u8(src.to(dtype) * (3 if dtype not in (torch.bool, torch.uint8) else 1), ks)      # any non-zero value samples
            assert out.dtype == torch.uint8 and out.is_contiguous() and torch.equal(out, src.expand(b, t, 1, h, mw, 1).to(torch.uint8))
            row, general = ops.is_row_mask(out, ks), ops.is_general_mask(out, ks)
            assert row != general, (tuple(src.shape), tuple(out.shape))
            assert row == (mw == 1) and ops.mask_layout(out, ks) == ("row" if row else "general")
            assert tuple(out.shape) == ((b, t, 1, h, 1, 1) if row else (b, t, 1, h, w, 1)) and (row or w > 1)
            assert ops.mask_layout(out, ks[:, :1], t) == ops.mask_layout(out, ks)                     # the shape from the maps and t
            acq = Acquisition(ks, out, ks[:, :1])
            assert acq.row == row and acq.fused and not Acquisition(ks, out, ks[:, :1], train=True).fused
    b, t, h, w = 2, 3, 8, 6
    ks = torch.zeros(b, t, 2, h, w, 2)
    for shape in ((b, t, 1, h, w), (b, t, 1, h, w, 2), (b, t, 2, h, w, 1), (b, t, 1, h - 1, w, 1), (b, t, 1, 1, w, 1), (b, t, 1, h, w - 1, 1),
                  (b, t, 1, h, 2, 1), (3, t, 1, h, w, 1), (b, 2, 1, h, 1, 1), (b, t, h, 1, 1, 1), (h,), (b, t, 1, h, 1, 1, 1)):
        with pytest.raises(ValueError, match="does not broadcast"):
            ops.as_mask_u8(torch.zeros(shape, dtype=torch.uint8), ks)
        assert ops.mask_layout(torch.zeros(shape, dtype=torch.uint8), ks) is None
    with pytest.raises(ValueError, match="neither layout"):
        Acquisition(ks, torch.zeros(1, t, 1, h, 1, 1, dtype=torch.uint8), ks[:, :1])               # not passed through as_mask_u8
    old = ops.GENERAL_MASK_FUSED
    try:        # read when the object is built, not when the module is imported
        ops.GENERAL_MASK_FUSED = False
        general = torch.zeros(b, t, 1, h, w, 1, dtype=torch.uint8)
        assert not Acquisition(ks, general, ks[:, :1]).fused and Acquisition(ks, torch.zeros(b, t, 1, h, 1, 1, dtype=torch.uint8), ks[:, :1]).fused
    finally:
        ops.GENERAL_MASK_FUSED = old


class _Stand:
    """The attributes of a SlicePipeline that input validation reads."""

    def __init__(self, model, takes, needs):
        self.model, self._takes_sens, self._needs_sens, self.device = model, takes, needs, torch.device("cuda", 0)


def test_sources_accept_and_refuse_masks_that_vary_along_w():
    from cine_hip.pipeline import _RawSource, _Source
    varnet, cinenet, xpd = _Stand("VarNet", True, False), _Stand("CineNet", True, True), _Stand("XPDNet", False, False)
    raw = np.zeros((7, 30, 28, 3), np.complex64)
    kw = dict(crop_shape=(24, 20), n_frames=5, filter_size=(0.7, 0.0, 0.3, 0.3), scaling=1e6, coil_matrix=None, apply_mask=True)
    row = torch.zeros(1, 5, 1, 24, 1, 1, dtype=torch.uint8)
    general = torch.zeros(1, 5, 1, 24, 20, 1, dtype=torch.uint8)
    shared = torch.zeros(1, 1, 1, 24, 20, 1)                                 # one float pattern for all frames, from the host
    sens = torch.zeros(1, 1, 3, 24, 20, 2)
    for pipe in (varnet, cinenet):
        src = _RawSource(pipe, raw, general, sens, **kw)
        assert src.mask_shape == (1, 5, 1, 24, 20, 1) and src.key[7] == (1, 5, 1, 24, 20, 1) and src.key[8] == (1, 1, 3, 24, 20, 2)
        assert _RawSource(pipe, raw, shared, sens, **kw).key == src.key and tuple(_RawSource(pipe, raw, shared, sens, **kw).mask.shape) == src.mask_shape
        assert _RawSource(pipe, raw, row, sens, **kw).key != src.key
    for pipe in (varnet, xpd):                                               # their sensitivity network reads its ACS window off a row mask
        with pytest.raises(CineHipError, match="varies along w"):
            _RawSource(pipe, raw, general, None, **kw)
        assert _RawSource(pipe, raw, row, None, **kw).mask_shape == (1, 5, 1, 24, 1, 1)
    with pytest.raises(CineHipError, match="needs sens_maps"):
        _RawSource(cinenet, raw, general, None, **kw)
    with pytest.raises(CineHipError, match="takes no sens_maps"):
        _RawSource(xpd, raw, general, sens, **kw)
    with pytest.raises(CineHipError, match="does not broadcast"):
        _RawSource(varnet, raw, torch.zeros(1, 5, 1, 24, 19, 1, dtype=torch.uint8), sens, **kw)
    with pytest.raises(CineHipError, match="sens_maps: shape"):
        _RawSource(varnet, raw, general, torch.zeros(1, 1, 3, 24, 19, 2), **kw)
    # ``submit`` keeps its rules
    mk = torch.zeros(1, 5, 3, 24, 20, 2)
    assert _Source(cinenet, mk, general, sens).mask_shape == (1, 5, 1, 24, 20, 1)
    with pytest.raises(CineHipError, match="varies along w"):
        _Source(varnet, mk, general, None)
