"""The total-variation baseline without a GPU: the ABI table carries the new entry points, the public names are exported and refuse what
they cannot do, and the float64 yardstick (tests/tv_reference.py) is itself checked -- D^H is the adjoint of D, the projection is one, the
norm bound behind the default sigma holds, and the iteration with the defaults reconstructs -- before the kernels are compared with it.

The objective is not monotone under the Condat-Vu iteration (single-iteration increases of about 1 % of the start value were seen at
(1, 15, 4, 48, 40)), so nothing here asserts descent per iteration.  With the defaults (0.02, 0.01) and sigma = 1 / (24 tau) the yardstick
ends 30 iterations at 0.63 / 0.72 of the starting objective and 0.51 / 0.56 of the zero-filled NRMSE on the two shapes below."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kt_reference as K
import tv_reference as R
from cine_hip.classical import TotalVariation, total_variation, tv_peaks  # noqa: F401  (the names this file is about: without them it does not load)
from conftest import ROOT

NEW = ("cine_tv_pd_tile", "cine_tv_pd_ws_bytes", "cine_tv_pd_step", "cine_tv_solve_ws_bytes", "cine_tv_solve")


def test_the_header_declares_the_five_prototypes_and_the_table_carries_them():
    from cine_hip import _lib
    with open(os.path.join(ROOT, "include", "cine_hip.h")) as f:
        text = f.read()
    for name in NEW:
        assert f" {name}(" in text and name in _lib._SIGS and name in _lib.declared_symbols(), name
    i, p, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib._SIGS["cine_tv_pd_tile"] == (i, [p, p])
    assert _lib._SIGS["cine_tv_pd_ws_bytes"] == (sz, [i, i, i, i])
    assert _lib._SIGS["cine_tv_pd_step"] == (i, [p] * 7 + [i, i, p, p, p, i, i, i, i, p, sz, p])
    assert _lib._SIGS["cine_tv_solve_ws_bytes"] == (sz, [i] * 7)
    assert _lib._SIGS["cine_tv_solve"] == (i, [p, p, p, p, p, i, p, p, p, p, i, i, i, p, p, i, i, i, i, i, p, sz, p])


def test_the_names_are_exported_and_lazily_resolved():
    import cine_hip
    from cine_hip import classical
    assert "total_variation" in cine_hip.__all__ and "TotalVariation" in cine_hip.__all__
    assert "total_variation" in cine_hip._CLASSICAL and "TotalVariation" in cine_hip._CLASSICAL
    for name in ("total_variation", "TotalVariation", "tv_peaks"):
        assert name in classical.__all__, name
    assert cine_hip.total_variation is classical.total_variation and cine_hip.TotalVariation is classical.TotalVariation
    assert callable(classical.tv_peaks)
    for doc in (classical.total_variation.__doc__, classical.TotalVariation.__doc__):
        assert "untuned" in doc or "nobody has tuned" in doc


def test_the_module_has_the_signature_the_pipeline_dispatches_on_and_no_parameters():
    from cine_hip import classical, pipeline
    model = classical.TotalVariation()
    assert pipeline._forward_params(model) == (True, True)
    assert not list(model.parameters()) and not list(model.buffers())
    assert (model.iters, model.lam_t, model.lam_s, model.step, model.sigma, model.periodic) == (50, 0.02, 0.01, None, None, True)


def test_cpu_tensors_inputs_that_require_grad_and_bad_settings_are_refused():
    from cine_hip import classical, ops
    from cine_hip._lib import CineHipError
    p = K.problem((1, 5, 3, 24, 20), "row")
    mk, mask, sens = p["masked_kspace"], p["mask"], p["sens_maps"]
    model = classical.TotalVariation(iters=3).eval()
    with pytest.raises(CineHipError, match="GPU"):
        classical.total_variation(mk, mask, sens)
    with pytest.raises(CineHipError, match="GPU"):
        model(mk, mask, sens)
    one = torch.ones(1)
    img = torch.zeros(1, 2, 3, 4, 2)
    with pytest.raises(CineHipError, match="GPU"):
        ops.tv_pd_step(img, img.clone(), torch.zeros(3, 1, 2, 3, 4, 2), one, one, one, one)
    with pytest.raises(CineHipError, match="GPU"):
        ops.tv_solve(torch.zeros(1, 5, 1, 24, 20, 2), sens, mask, one, one, one, one, 3)
    with torch.enable_grad():
        for kw in ({"masked_kspace": mk.clone().requires_grad_(True)}, {"sens_maps": sens.clone().requires_grad_(True)}):
            args = {"masked_kspace": mk, "mask": mask, "sens_maps": sens, **kw}
            with pytest.raises(CineHipError, match="not differentiable"):
                classical.total_variation(**args)
            with pytest.raises(CineHipError, match="requires grad"):
                model(args["masked_kspace"], args["mask"], args["sens_maps"])
        with pytest.raises(CineHipError, match="requires grad"):
            classical.total_variation(mk, mask, sens, lam_s=torch.ones(1, requires_grad=True))
    with pytest.raises(ValueError):
        classical.total_variation(mk, mask, sens, iters=0)
    with pytest.raises(ValueError):
        classical.TotalVariation(iters=0)
    with pytest.raises(ValueError):
        classical.total_variation(mk, mask, sens, output="phase")
    with pytest.raises(ValueError, match="both 0"):
        classical.total_variation(mk, mask, sens, lam_t=0.0, lam_s=0.0)
    with pytest.raises(ValueError, match="both 0"):
        classical.TotalVariation(lam_t=0.0, lam_s=0.0)(mk, mask, sens)


def _crandn(rs, shape):
    return rs.standard_normal(shape) + 1j * rs.standard_normal(shape)


@pytest.mark.parametrize("shape", [(2, 5, 6, 7), (1, 2, 1, 9), (1, 2, 9, 1), (1, 3, 1, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("periodic", [True, False])
def test_dh_is_the_adjoint_of_d(shape, periodic):
    rs = np.random.RandomState(7)
    x, p = _crandn(rs, shape), _crandn(rs, (3,) + shape)
    for terms in (1, 2, 3):
        lhs, rhs = np.vdot(p, R.D(x, periodic, terms)), np.vdot(R.DH(p, periodic, terms), x)      # <D x, p> = <x, D^H p>
        scale = np.linalg.norm(x) * np.linalg.norm(p)
        assert abs(lhs - rhs) <= 1e-12 * scale, (terms, lhs, rhs)
    d = R.D(x, periodic, 3)
    b, t, h, w = shape
    assert not d[1][:, :, h - 1].any() and not d[2][:, :, :, w - 1].any()                         # 0 at the last row / column
    assert np.array_equal(d[0][:, t - 1], x[:, 0] - x[:, t - 1] if periodic else np.zeros_like(x[:, 0]))
    if h == 1:
        assert not d[1].any()                                                                     # a length-1 axis: all-zero differences
    if w == 1:
        assert not d[2].any()
    assert not R.D(x, periodic, 1)[1:].any() and not R.D(x, periodic, 2)[0].any()                 # a term that is off has zero planes


def test_project_is_idempotent_and_leaves_the_inside_alone():
    rs = np.random.RandomState(3)
    p = _crandn(rs, (3, 1, 4, 5, 6))
    lam_t, lam_s = 0.8, 1.1
    q = R.project(p, lam_t, lam_s)
    assert np.abs(q[0]).max() <= lam_t * (1 + 1e-15) and np.sqrt(np.abs(q[1]) ** 2 + np.abs(q[2]) ** 2).max() <= lam_s * (1 + 1e-15)
    assert np.allclose(R.project(q, lam_t, lam_s), q, rtol=0, atol=1e-15)
    in_t, in_s = np.abs(p[0]) <= lam_t, np.sqrt(np.abs(p[1]) ** 2 + np.abs(p[2]) ** 2) <= lam_s
    assert in_t.any() and not in_t.all() and in_s.any() and not in_s.all()                        # the fixture has points on both sides
    assert np.array_equal(q[0][in_t], p[0][in_t]) and np.array_equal(q[1][in_s], p[1][in_s]) and np.array_equal(q[2][in_s], p[2][in_s])
    out = ~in_s
    assert np.allclose(np.sqrt(np.abs(q[1]) ** 2 + np.abs(q[2]) ** 2)[out], lam_s)                # outside: onto the sphere, jointly
    assert np.allclose(q[1][out] * p[2][out], q[2][out] * p[1][out])                              # ... along the same direction
    one = R.project(p, lam_t, lam_s, terms=1)
    assert np.array_equal(one[1:], p[1:]) and np.array_equal(one[0], q[0])                        # a plane that is off passes through


@pytest.mark.parametrize("periodic", [True, False])
def test_the_norm_bound_behind_the_default_sigma_holds(periodic):
    for terms, bound in ((1, 4.0), (2, 8.0), (3, 12.0)):
        assert R.norm_bound(terms) == bound
        for shape in ((1, 5, 6, 7), (1, 8, 1, 9), (2, 16, 12, 10)):
            lam = R.power_iteration(shape, periodic, terms)
            assert 0.0 < lam <= bound, (terms, shape, lam)
    assert R.power_iteration((1, 16, 16, 16), periodic, 3) > 11.0                                 # and the bound is not slack by much
    tau = 0.7
    assert np.isclose(1.0 / tau - R.default_sigma(tau, 3) * 12.0, 0.5 / tau)                      # Condat: 1 / tau - sigma ||D||^2 >= L / 2


@pytest.mark.parametrize("shape,layout", [((1, 5, 3, 24, 20), "row"), ((1, 7, 4, 21, 17), "plane")], ids=["5x3x24x20-row", "7x4x21x17-plane"])
def test_the_yardstick_reconstructs_with_the_defaults(shape, layout):
    p = K.problem(shape, layout)
    y, m, s, zf = p["y"], p["m"], p["s"], p["zf"]
    tau = K.default_step(s)
    sigma = R.default_sigma(tau, 3)
    assert np.isclose(sigma, 1.0 / (24.0 * tau))
    peak_t, peak_s = R.peaks(zf, True)
    lam_t, lam_s = 0.02 * peak_t, 0.01 * peak_s
    x, dual, rec = R.solve(zf, s, m, tau, sigma, lam_t, lam_s, 30)
    start, end = R.objective(zf, y, s, m, lam_t, lam_s), R.objective(x, y, s, m, lam_t, lam_s)
    truth = p["target"].numpy()
    got, zero_filled = K.nrmse(np.abs(x), truth), K.nrmse(np.abs(zf), truth)
    print(f"{shape} {layout}: objective {end / start:.3f} of the start, NRMSE {got / zero_filled:.3f} of the zero-filled one")
    assert end < 0.9 * start
    assert got <= 0.6 * zero_filled
    # the dual stays in its balls, the record is what it says, and one iteration by hand is the first row
    assert np.abs(dual[0]).max() <= lam_t * (1 + 1e-12) and np.sqrt(np.abs(dual[1]) ** 2 + np.abs(dual[2]) ** 2).max() <= lam_s * (1 + 1e-12)
    d = R.D(x, True, 3)
    assert np.isclose(rec[-1, 1], (np.abs(x) ** 2).sum()) and np.isclose(rec[-1, 2], np.abs(d[0]).sum())
    assert np.isclose(rec[-1, 3], np.sqrt(np.abs(d[1]) ** 2 + np.abs(d[2]) ** 2).sum())
    x1 = zf - tau * K.gradient(zf, s, m, zf)
    p1 = R.project(sigma * R.D(2 * x1 - zf), lam_t, lam_s)
    got1 = R.solve(zf, s, m, tau, sigma, lam_t, lam_s, 1)
    assert np.array_equal(got1[0], x1) and np.allclose(got1[1], p1, rtol=0, atol=1e-15)
