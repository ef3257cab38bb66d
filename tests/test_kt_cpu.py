"""The k-t SPARSE-SENSE baseline without a GPU: the ABI table carries the new entry points, the momentum is the double recurrence, the public
functions refuse what they cannot do, and the float64 yardstick (tests/kt_reference.py) is itself checked -- ISTA with a step inside the
bound never increases the objective -- before the kernels are compared with it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kt_reference as R
from conftest import ROOT

NEW = ("cine_kt_prox_pixels", "cine_kt_prox_ws_bytes", "cine_kt_prox", "cine_kt_fista_ws_bytes", "cine_kt_fista")


def test_the_header_declares_the_five_prototypes_and_the_table_carries_them():
    from cine_hip import _lib
    with open(os.path.join(ROOT, "include", "cine_hip.h")) as f:
        text = f.read()
    for name in NEW:
        assert f" {name}(" in text and name in _lib._SIGS and name in _lib.declared_symbols(), name
    i, p, f32, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t
    assert _lib._SIGS["cine_kt_prox_pixels"] == (i, [])
    assert _lib._SIGS["cine_kt_prox_ws_bytes"] == (sz, [i, i, i, i])
    assert _lib._SIGS["cine_kt_prox"] == (i, [p, p, p, p, p, f32, i, p, p, p, i, i, i, i, p, sz, p])
    assert _lib._SIGS["cine_kt_fista_ws_bytes"] == (sz, [i] * 7)
    assert _lib._SIGS["cine_kt_fista"] == (i, [p, p, p, p, p, i, p, p, i, i, p, i, i, i, i, i, p, sz, p])


def test_fista_momentum_is_the_double_recurrence():
    import cine_hip
    from cine_hip import classical
    got = classical.fista_momentum(40)
    want, s = [], 1.0
    for _ in range(40):
        s1 = (1.0 + (1.0 + 4.0 * s * s) ** 0.5) / 2.0
        want.append((s - 1.0) / s1)
        s = s1
    assert got.dtype == np.float32 and got.shape == (40,) and got[0] == 0.0
    assert np.array_equal(got, np.array(want, dtype=np.float64).astype(np.float32))
    assert np.array_equal(got, R.momentum(40))
    assert 0.28 < got[1] < 0.29 and np.all(np.diff(got) > 0) and got[-1] < 1.0           # (1 - 1) / s_1, then rising towards 1
    assert cine_hip.fista_momentum is classical.fista_momentum and cine_hip.KtSparseSense is classical.KtSparseSense
    assert cine_hip.kt_sparse_sense is classical.kt_sparse_sense


def test_cpu_tensors_and_inputs_that_require_grad_are_refused():
    from cine_hip import classical, ops
    from cine_hip._lib import CineHipError
    p = R.problem((1, 5, 3, 24, 20), "row")
    mk, mask, sens = p["masked_kspace"], p["mask"], p["sens_maps"]
    model = classical.KtSparseSense(iters=3).eval()
    assert not list(model.parameters())
    with pytest.raises(CineHipError, match="GPU"):
        classical.kt_sparse_sense(mk, mask, sens)
    with pytest.raises(CineHipError, match="GPU"):
        model(mk, mask, sens)
    one = torch.ones(1)
    with pytest.raises(CineHipError, match="GPU"):
        ops.kt_prox(torch.zeros(1, 2, 3, 4, 2), torch.zeros(1, 2, 3, 4, 2), torch.zeros(1, 2, 3, 4, 2), one, one)
    with pytest.raises(CineHipError, match="GPU"):
        ops.kt_fista(torch.zeros(1, 5, 1, 24, 20, 2), sens, mask, one, one, 3)
    with torch.enable_grad():
        for kw in ({"masked_kspace": mk.clone().requires_grad_(True)}, {"sens_maps": sens.clone().requires_grad_(True)}):
            args = {"masked_kspace": mk, "mask": mask, "sens_maps": sens, **kw}
            with pytest.raises(CineHipError, match="not differentiable"):
                classical.kt_sparse_sense(**args)
            with pytest.raises(CineHipError, match="requires grad"):
                model(args["masked_kspace"], args["mask"], args["sens_maps"])
    with pytest.raises(ValueError):
        classical.kt_sparse_sense(mk, mask, sens, output="phase")
    with pytest.raises(ValueError):
        classical.KtSparseSense(iters=0)


def test_the_module_has_the_signature_the_pipeline_dispatches_on():
    from cine_hip import classical, pipeline
    assert pipeline._forward_params(classical.KtSparseSense()) == (True, True)


@pytest.mark.parametrize("penalise_dc", [True, False])
def test_ista_on_the_yardstick_never_increases_the_objective(penalise_dc):
    """beta = 0 and step = 1 / max sum |S|^2 (inside 1 / ||A^H M A||): a proximal-gradient step is a descent step."""
    p = R.problem((1, 5, 3, 24, 20), "row")
    y, m, s, zf = p["y"], p["m"], p["s"], p["zf"]
    step = R.default_step(s)
    lam = 0.02 * np.abs(R.fft1c(zf, 1)).max()
    x = z = zf
    obj = [R.objective(x, y, s, m, lam, penalise_dc)]
    for _ in range(20):
        x, z, _ = R.prox(z, R.gradient(z, s, m, zf), x, step, lam, 0.0, penalise_dc)
        obj.append(R.objective(x, y, s, m, lam, penalise_dc))
    obj = np.array(obj)
    assert np.all(np.diff(obj) <= 1e-12 * obj[0]), obj
    assert obj[-1] < 0.9 * obj[0]
    # the same loop through fista() with zero momentum, and the record's sums against their definitions
    x2, rec = R.fista(zf, s, m, step, lam, 20, penalise_dc, betas=np.zeros(20))
    assert np.array_equal(x2, x)
    w = R.bin_weights(5, penalise_dc).reshape(1, -1, 1, 1)
    assert np.isclose(rec[-1, 1], (np.abs(x) ** 2).sum()) and np.isclose(rec[-1, 2], (w * np.abs(R.fft1c(x, 1))).sum())


def test_the_yardsticks_transforms_are_unitary_and_centered():
    rs = np.random.RandomState(0)
    for t in (2, 5, 16):
        x = rs.standard_normal((1, t, 3, 4)) + 1j * rs.standard_normal((1, t, 3, 4))
        f = R.fft1c(x, 1)
        assert np.allclose(R.fft1c(f, 1, inverse=True), x) and np.isclose((np.abs(f) ** 2).sum(), (np.abs(x) ** 2).sum())
        const = np.ones((1, t, 1, 1), dtype=complex)
        fc = R.fft1c(const, 1)[0, :, 0, 0]
        assert np.isclose(abs(fc[t // 2]), np.sqrt(t)) and np.allclose(np.delete(fc, t // 2), 0)      # the DC bin sits at t // 2
    s = R.problem((1, 5, 3, 24, 20), "row")["s"]
    x = rs.standard_normal((1, 5, 24, 20)) + 1j * rs.standard_normal((1, 5, 24, 20))
    k = rs.standard_normal((1, 5, 3, 24, 20)) + 1j * rs.standard_normal((1, 5, 3, 24, 20))
    assert np.isclose(np.vdot(k, R.forward_op(x, s)), np.vdot(R.adjoint_op(k, s), x))                 # <k, A x> = <A^H k, x>
