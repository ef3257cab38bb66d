"""Training on the image-space data consistency for masks that vary along w, on the host: the binding of cine_image_dc_general_sens_grad and
its size query, the argument validation before any launch through the loaded library, the switch ops.GENERAL_MASK_FUSED_TRAIN and what
cine_hip.dc.Acquisition(train=True) decides from the two switches.  Runs without a GPU."""
import ctypes

import torch

from cine_hip import _lib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAMES = ("cine_image_dc_general_sens_grad_ws_bytes", "cine_image_dc_general_sens_grad")
ME = b"cine_image_dc_general_sens_grad"


def test_symbols_are_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    L = _lib.lib()
    for name in NAMES:
        assert name in declared and hasattr(L, name) and name in _lib._SIGS, name


def test_the_workspace_is_one_set_of_hybrid_space_coil_images():
    """The header: the two operands go one after the other through ONE buffer of b*t*c*h*w complex values, the size cine_image_dc_general needs."""
    L = _lib.lib()
    for b, t, c, h, w in ((1, 15, 15, 200, 200), (2, 3, 17, 7, 13), (1, 1, 1, 1, 1), (1, 3, 12000, 4, 2), (1, 1, 2, 512, 480)):
        assert L.cine_image_dc_general_sens_grad_ws_bytes(b, t, c, h, w) == b * t * c * h * w * 8 == L.cine_image_dc_general_ws_bytes(b, t, c, h, w)
    for bad in ((0, 1, 1, 8, 8), (1, 0, 1, 8, 8), (1, 1, 0, 8, 8), (1, 1, 1, -1, 8), (1, 1, 1, 8, 0)):
        assert L.cine_image_dc_general_sens_grad_ws_bytes(*bad) == 0
    assert L.cine_image_dc_general_sens_grad_ws_bytes(4, 25, 32, 512, 512) == 4 * 25 * 32 * 512 * 512 * 8          # above 2^32: size_t


def test_sens_grad_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = {k: ctypes.c_void_p(0x1000 * (i + 1)) for i, k in enumerate(("img", "gout", "sens", "mask", "lam", "part", "ws"))}   # never dereferenced
    args = dict(b=1, t=3, c=4, h=24, w=20)

    def call(nbytes=1 << 40, **kw):
        a = dict(args, **p)
        a.update(kw)
        return L.cine_image_dc_general_sens_grad(a["img"], a["gout"], a["sens"], a["mask"], a["lam"], 1.0, 0.0, a["part"],
                                                 a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"], nbytes, None)

    def mine():
        return L.cine_last_error().startswith(ME + b":")

    for name in ("img", "gout", "sens", "mask", "part", "ws"):
        assert call(**{name: None}) == EINVAL and mine() and b"null" in L.cine_last_error(), name
    for name in ("img", "gout"):
        assert call(part=p[name]) == EINVAL and mine() and b"alias" in L.cine_last_error(), name
    for name in ("b", "t", "c", "h", "w"):
        assert call(**{name: 0}) == EINVAL and mine(), name
    assert call(c=32769) == EINVAL and mine()
    assert call(c=32768, nbytes=0) == EWORKSPACE                                       # the largest coil count gets as far as the workspace
    assert call(b=256, t=256) == EUNSUPPORTED and mine() and b"65535" in L.cine_last_error()
    assert call(b=65536, t=1) == EUNSUPPORTED
    assert call(h=401) == EUNSUPPORTED and mine() and b"401" in L.cine_last_error()
    assert call(w=401) == EUNSUPPORTED and mine()
    assert call(h=514) == EUNSUPPORTED and mine() and b"514" in L.cine_last_error()
    need = L.cine_image_dc_general_sens_grad_ws_bytes(1, 3, 4, 24, 20)
    assert call(nbytes=need - 1) == EWORKSPACE and mine() and b"workspace" in L.cine_last_error()
    assert call(nbytes=0) == EWORKSPACE
    assert call(lam=None, nbytes=need - 1) == EWORKSPACE                               # lambda_dev may be NULL: the fixed weights


def test_the_training_switch_is_off_by_default():
    from cine_hip import ops
    assert ops.GENERAL_MASK_FUSED_TRAIN is False and ops.GENERAL_MASK_FUSED is True
    L = _lib.lib()
    assert L.cine_diag_counter(15, 0) >= 0 and L.cine_diag_counter(16, 0) == -1        # the new passes count in 15: no new counter


def test_a_training_acquisition_follows_the_two_switches(monkeypatch):
    from cine_hip import ops
    from cine_hip.dc import Acquisition
    b, t, h, w = 2, 3, 8, 6
    ks = torch.zeros(b, t, 2, h, w, 2)
    general = torch.zeros(b, t, 1, h, w, 1, dtype=torch.uint8)
    row = torch.zeros(b, t, 1, h, 1, 1, dtype=torch.uint8)
    for fused in (False, True):
        for train_switch in (False, True):
            monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", fused)
            monkeypatch.setattr(ops, "GENERAL_MASK_FUSED_TRAIN", train_switch)
            acq = Acquisition(ks, general, ks[:, :1], train=True)
            assert acq.fused == (fused and train_switch) and not acq.row and acq.train and acq.tiled is None, (fused, train_switch)
            assert ops.general_mask_fused_train(general, ks) == (fused and train_switch)
            assert Acquisition(ks, general, ks[:, :1]).fused == fused                  # inference reads its own switch only
            # a row mask is unaffected: the image-space kernel in inference, its autograd functions in training
            assert Acquisition(ks, row, ks[:, :1]).fused and not Acquisition(ks, row, ks[:, :1], train=True).fused
            assert not ops.general_mask_fused_train(row, ks)
    # read when the object is built: a later flip does not change an object
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", True)
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED_TRAIN", True)
    acq = Acquisition(ks, general, ks[:, :1], train=True)
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED_TRAIN", False)
    assert acq.fused and not Acquisition(ks, general, ks[:, :1], train=True).fused
