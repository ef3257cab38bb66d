"""The host side of the in-flight ESPIRiT calibration: what the three entry points refuse before any launch (through the loaded
library, no GPU), what ``SlicePipeline`` accepts for ``sens_maps="espirit"``, and the set keys."""
import ctypes

import pytest
import torch

from cine_hip import _lib
from cine_hip._lib import CineHipError

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
PTR = 1 << 20                                # never dereferenced: every refusal below comes before the first launch


def _err():
    return _lib.lib().cine_last_error().decode()


def test_entry_points_are_declared_and_bound():
    declared = _lib.declared_symbols()
    for name in ("cine_espirit_gram_ws_bytes", "cine_espirit_gram", "cine_zgemm_f64", "cine_espirit_projector_ws_bytes",
                 "cine_espirit_projector"):
        assert name in declared and name in _lib._SIGS and hasattr(_lib.lib(), name), name


def test_gram_refusals():
    L = _lib.lib()
    a, b, c = PTR, 2 * PTR, 3 * PTR
    need = L.cine_espirit_gram_ws_bytes(15, 200, 200, 24, 6)
    assert need == 24 * 24 * 15 * 16
    assert L.cine_espirit_gram_ws_bytes(3, 14, 17, 200, 6) == 14 * 17 * 3 * 16      # r larger than the image: clipped
    for args in ((None, b, c), (a, None, c), (a, b, None)):
        assert L.cine_espirit_gram(*args, need, 15, 200, 200, 24, 6, None) == EINVAL and "null" in _err()
    assert L.cine_espirit_gram(a, b, c, 1 << 30, 33, 200, 200, 24, 6, None) == EUNSUPPORTED and "at most 32" in _err()
    assert L.cine_espirit_gram_ws_bytes(33, 200, 200, 24, 6) == 0
    assert L.cine_espirit_gram(a, b, c, 1 << 30, 9, 200, 200, 24, 12, None) == EUNSUPPORTED and "at most 1152" in _err()   # n = 1296
    assert L.cine_espirit_gram(a, b, c, 1 << 30, 4, 40, 40, 5, 6, None) == EINVAL and "smaller than" in _err()
    assert L.cine_espirit_gram(a, b, c, 1 << 30, 4, 40, 40, 0, 6, None) == EINVAL
    assert L.cine_espirit_gram(a, b, c, need - 1, 15, 200, 200, 24, 6, None) == EWORKSPACE and str(need) in _err()


def test_zgemm_refusals():
    L = _lib.lib()
    a, b, d, c = PTR, 2 * PTR, 3 * PTR, 4 * PTR
    assert L.cine_zgemm_f64(None, b, d, c, 36, 1.0, 0.0, 0.0, 0.0, None) == EINVAL and "null" in _err()
    assert L.cine_zgemm_f64(a, b, None, c, 36, 1.0, 0.0, 1.0, 0.0, None) == EINVAL          # beta != 0 reads d
    assert L.cine_zgemm_f64(a, b, d, a, 36, 1.0, 0.0, 0.0, 0.0, None) == EINVAL and "alias" in _err()
    assert L.cine_zgemm_f64(a, b, d, c, 0, 1.0, 0.0, 0.0, 0.0, None) == EINVAL
    assert L.cine_zgemm_f64(a, b, d, c, 1153, 1.0, 0.0, 0.0, 0.0, None) == EUNSUPPORTED and "at most 1152" in _err()
    assert L.cine_zgemm_f64(a + 8, b, d, c, 36, 1.0, 0.0, 0.0, 0.0, None) == EINVAL and "aligned" in _err()


def test_projector_refusals():
    L = _lib.lib()
    g, p, lam, res, ws = PTR, 2 * PTR, 3 * PTR, 3 * PTR + 64, 4 * PTR
    n = 540
    need = L.cine_espirit_projector_ws_bytes(n)
    assert need >= 3 * n * n * 16
    assert L.cine_espirit_projector_ws_bytes(1153) == 0 and L.cine_espirit_projector_ws_bytes(0) == 0
    ok = (g, n, 1e-3, 60, p, lam, res, ws, need, None)
    for i in (0, 4, 5, 6, 7):
        args = list(ok)
        args[i] = None
        assert L.cine_espirit_projector(*args) == EINVAL and "null" in _err(), i
    assert L.cine_espirit_projector(g, n, 1e-3, 0, p, lam, res, ws, need, None) == EINVAL and "at least 1" in _err()
    assert L.cine_espirit_projector(g, n, 0.0, 60, p, lam, res, ws, need, None) == EINVAL and "> 0" in _err()
    assert L.cine_espirit_projector(g, n, -1e-3, 60, p, lam, res, ws, need, None) == EINVAL
    assert L.cine_espirit_projector(g, 1153, 1e-3, 60, p, lam, res, ws, 1 << 40, None) == EUNSUPPORTED and "at most 1152" in _err()
    assert L.cine_espirit_projector(g, n, 1e-3, 60, p, lam, res, ws, need - 1, None) == EWORKSPACE and str(need) in _err()


# ------------------------------------------------------------------ the pipeline's sources and keys
class _Takes(torch.nn.Module):
    def forward(self, masked_kspace, mask, sens_maps=None):
        return masked_kspace


class _Needs(torch.nn.Module):
    def forward(self, masked_kspace, mask, sens_maps):
        return masked_kspace


class _TakesNone(torch.nn.Module):
    def forward(self, masked_kspace, mask):
        return masked_kspace


class _Pipe:
    """What _Source / _RawSource read of a pipeline."""
    def __init__(self, model):
        from cine_hip.pipeline import _forward_params
        self.model, self.device = model, torch.device("cuda:0")
        self._takes_sens, self._needs_sens = _forward_params(model)


MK = torch.zeros((1, 5, 6, 32, 32, 2))
MASK = torch.ones((1, 5, 1, 32, 1, 1), dtype=torch.uint8)
RAW = torch.zeros((5, 40, 36, 6, 2))
RAW_ARGS = ((32, 32), 5, (0.7, 0.0, 0.3, 0.3), 1e6, None, True)


def test_sources_accept_and_refuse_espirit():
    from cine_hip.pipeline import _RawSource, _Source, espirit_key
    for model in (_Takes(), _Needs()):
        src = _Source(_Pipe(model), MK, MASK, "espirit")
        assert src.sens is None and src.espirit == espirit_key(15, 60) == ("espirit", 15, 6, 1e-3, 0.8, 60)
        assert [name for name, *_ in src.items({"mk": None, "mask": None, "sens": None})] == ["mk", "mask"]     # nothing to copy in
        raw = _RawSource(_Pipe(model), RAW, MASK, "espirit", *RAW_ARGS, 12, 40)
        assert raw.sens is None and raw.espirit == ("espirit", 12, 6, 1e-3, 0.8, 40)
    with pytest.raises(CineHipError, match="takes no sens_maps"):
        _Source(_Pipe(_TakesNone()), MK, MASK, "espirit")
    with pytest.raises(CineHipError, match="takes no sens_maps"):
        _RawSource(_Pipe(_TakesNone()), RAW, MASK, "espirit", *RAW_ARGS)
    for bad in ("ESPIRiT", "eigh", ""):
        with pytest.raises(CineHipError, match="not a tensor, None or 'espirit'"):
            _Source(_Pipe(_Takes()), MK, MASK, bad)
        with pytest.raises(CineHipError, match="not a tensor, None or 'espirit'"):
            _RawSource(_Pipe(_Takes()), RAW, MASK, bad, *RAW_ARGS)
    with pytest.raises(CineHipError, match="ecalib_r"):
        _Source(_Pipe(_Takes()), MK, MASK, "espirit", 5, 60)                 # smaller than the kernel
    with pytest.raises(CineHipError, match="sign_iters"):
        _Source(_Pipe(_Takes()), MK, MASK, "espirit", 15, 0)
    with pytest.raises(CineHipError, match="at most 32 coils"):
        _Source(_Pipe(_Takes()), torch.zeros((1, 2, 33, 16, 16, 2)), torch.ones((1, 2, 1, 16, 1, 1), dtype=torch.uint8), "espirit")
    # a mask that varies along w: refused without maps, served with "espirit" (the sensitivity network is not run)
    gmask = torch.ones((1, 5, 1, 32, 32, 1), dtype=torch.uint8)
    with pytest.raises(CineHipError, match="varies along w"):
        _Source(_Pipe(_Takes()), MK, gmask, None)
    assert _Source(_Pipe(_Takes()), MK, gmask, "espirit").espirit is not None


def test_set_keys():
    from cine_hip.pipeline import _RawSource, _Source, espirit_key, raw_set_key
    pipe = _Pipe(_Takes())
    sens = torch.zeros((1, 1, 6, 32, 32, 2))
    k_tensor = _Source(pipe, MK, MASK, sens).key
    k15, k24 = _Source(pipe, MK, MASK, "espirit").key, _Source(pipe, MK, MASK, "espirit", 24).key
    assert len({k_tensor, k15, k24, _Source(pipe, MK, MASK, None).key, _Source(pipe, MK, MASK, "espirit", 15, 80).key}) == 5
    assert k15 == _Source(pipe, MK, MASK, "espirit", ecalib_r=15, sign_iters=60).key
    r_tensor = _RawSource(pipe, RAW, MASK, sens, *RAW_ARGS).key
    r15, r24 = _RawSource(pipe, RAW, MASK, "espirit", *RAW_ARGS).key, _RawSource(pipe, RAW, MASK, "espirit", *RAW_ARGS, 24, 60).key
    assert len({r_tensor, r15, r24, k15}) == 4
    args = (RAW.shape, 5, (32, 32), (0.7, 0.0, 0.3, 0.3), 1e6, True, MASK.shape)
    assert r15 == raw_set_key(*args, None, espirit=espirit_key(15, 60))
    assert r_tensor == raw_set_key(*args, sens.shape)
    assert raw_set_key(*args, sens.shape) == raw_set_key(*args, sens.shape, None, None)       # the old call is unchanged
