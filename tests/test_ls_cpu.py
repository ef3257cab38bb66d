"""The low-rank plus sparse baseline without a GPU: the ABI table carries the new entry points, the public functions are exported and
refuse what they cannot do, and the float64 yardstick (tests/ls_reference.py) is itself checked -- with the default step an iteration never
increases the objective, and the Gram route to singular-value thresholding agrees with the SVD route -- before the kernels are compared
with it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import kt_reference as R
import ls_reference as LS
from conftest import ROOT

NEW = ("cine_casorati_gram_pixels", "cine_casorati_gram_ws_bytes", "cine_casorati_gram", "cine_svt_weight", "cine_ls_prox_pixels",
       "cine_ls_prox_ws_bytes", "cine_ls_prox", "cine_ls_solve_ws_bytes", "cine_ls_solve")


def test_the_header_declares_the_prototypes_and_the_table_carries_them():
    from cine_hip import _lib
    with open(os.path.join(ROOT, "include", "cine_hip.h")) as f:
        text = f.read()
    for name in NEW:
        assert f" {name}(" in text and name in _lib._SIGS and name in _lib.declared_symbols(), name
    i, p, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib._SIGS["cine_casorati_gram_pixels"] == (i, [i])
    assert _lib._SIGS["cine_casorati_gram_ws_bytes"] == (sz, [i, i, i, i])
    assert _lib._SIGS["cine_casorati_gram"] == (i, [p, p, p, p, i, i, i, i, p, sz, p])
    assert _lib._SIGS["cine_svt_weight"] == (i, [p, p, p, p, p, i, i, p])
    assert _lib._SIGS["cine_ls_prox_pixels"] == (i, [])
    assert _lib._SIGS["cine_ls_prox_ws_bytes"] == (sz, [i, i, i, i])
    assert _lib._SIGS["cine_ls_prox"] == (i, [p] * 10 + [i, i, i, i, p, sz, p])
    assert _lib._SIGS["cine_ls_solve_ws_bytes"] == (sz, [i] * 7)
    assert _lib._SIGS["cine_ls_solve"] == (i, [p] * 7 + [i, p, p, p, i, p, p, i, i, i, i, i, p, sz, p])


def test_exports_and_the_signature_the_pipeline_dispatches_on():
    import cine_hip
    from cine_hip import classical, ops, pipeline
    assert cine_hip.low_rank_plus_sparse is classical.low_rank_plus_sparse and cine_hip.LowRankPlusSparse is classical.LowRankPlusSparse
    assert "low_rank_plus_sparse" in cine_hip.__all__ and "LowRankPlusSparse" in classical.__all__
    assert pipeline._forward_params(classical.LowRankPlusSparse()) == (True, True)
    assert not list(classical.LowRankPlusSparse().parameters())
    for name in ("casorati_gram", "svt_weight", "ls_prox", "ls_solve", "ls_prox_pixels"):
        assert callable(getattr(ops, name)), name


def test_cpu_tensors_inputs_that_require_grad_and_bad_settings_are_refused():
    from cine_hip import classical, ops
    from cine_hip._lib import CineHipError
    p = R.problem((1, 5, 3, 24, 20), "row")
    mk, mask, sens = p["masked_kspace"], p["mask"], p["sens_maps"]
    model = classical.LowRankPlusSparse(iters=3).eval()
    with pytest.raises(CineHipError, match="GPU"):
        classical.low_rank_plus_sparse(mk, mask, sens)
    with pytest.raises(CineHipError, match="GPU"):
        model(mk, mask, sens)
    one, img = torch.ones(1), torch.zeros(1, 2, 3, 4, 2)
    with pytest.raises(CineHipError, match="GPU"):
        ops.casorati_gram(img)
    with pytest.raises(CineHipError, match="GPU"):
        ops.svt_weight(torch.zeros(1, 2, 2, 2, dtype=torch.float64), one)
    with pytest.raises(CineHipError, match="GPU"):
        ops.ls_prox(img, img.clone(), img.clone(), torch.zeros(1, 2, 2, 2), one, one)
    with pytest.raises(CineHipError, match="GPU"):
        ops.ls_solve(torch.zeros(1, 5, 1, 24, 20, 2), sens, mask, one, one, one, 3)
    with torch.enable_grad():
        for kw in ({"masked_kspace": mk.clone().requires_grad_(True)}, {"sens_maps": sens.clone().requires_grad_(True)}):
            args = {"masked_kspace": mk, "mask": mask, "sens_maps": sens, **kw}
            with pytest.raises(CineHipError, match="low_rank_plus_sparse: .* requires grad, but the solver is not differentiable"):
                classical.low_rank_plus_sparse(**args)
            with pytest.raises(CineHipError, match="requires grad"):
                model(args["masked_kspace"], args["mask"], args["sens_maps"])
    with pytest.raises(ValueError, match="iters = 0"):
        classical.low_rank_plus_sparse(mk, mask, sens, iters=0)
    with pytest.raises(ValueError, match="iters = 0"):
        classical.LowRankPlusSparse(iters=0)
    with pytest.raises(ValueError):
        classical.low_rank_plus_sparse(mk, mask, sens, output="phase")


@pytest.mark.parametrize("shape,layout", LS.FIXTURES, ids=["row", "plane"])
def test_the_yardstick_never_increases_the_objective(shape, layout):
    """step = 0.5 / max sum |S|^2, inside 1 / (2 ||A^H M A||), the Lipschitz constant of the data term in (L, S): a descent step."""
    _, _, _, obj = LS.solved(shape, layout, rounded=False)
    print(f"{shape} {layout}: objective {obj[0]:.6g} -> {obj[-1]:.6g} ({obj[-1] / obj[0]:.3f}), largest increase {np.diff(obj).max() / obj[0]:.2e}")
    assert obj.shape == (LS.ITERS + 1,)
    assert np.all(np.diff(obj) <= 1e-12 * obj[0]), obj
    assert obj[-1] < 0.9 * obj[0]


@pytest.mark.parametrize("shape,layout", LS.FIXTURES, ids=["row", "plane"])
def test_the_gram_route_matches_the_svd_route(shape, layout):
    """X W with W from the float64 Gram matrix against thresholding numpy.linalg.svd's singular values, on the operand of every iteration."""
    p, _, step, thl, ths = LS.settings(shape, layout)
    zf = p["zf"]
    l, s = zf, np.zeros_like(zf)
    worst = 0.0
    for _ in range(LS.ITERS):
        g = R.gradient(l + s, p["s"], p["m"], zf)
        v = l - step * g
        want, want_nuc = LS.svt(v, step * thl)
        for i in range(v.shape[0]):
            x = LS.casorati(v[i])
            w, smax, nuc = LS.gram_weight(LS.gram(v[i:i + 1])[0], step * thl)
            worst = max(worst, float(np.abs(x @ w - LS.casorati(want[i])).max() / np.abs(x).max()))
            assert abs(nuc - want_nuc[i]) <= 1e-10 * want_nuc[i]
            assert abs(smax - np.linalg.svd(x, compute_uv=False).max()) <= 1e-10 * smax
        l, s, _ = LS.prox(l, s, g, step, thl, ths)
    print(f"{shape} {layout}: Gram route against the SVD route, {worst:.2e} of the peak (bar 1e-10)")
    assert worst <= 1e-10


def test_the_yardsticks_pieces():
    rs = np.random.RandomState(0)
    x = rs.standard_normal((2, 5, 3, 4)) + 1j * rs.standard_normal((2, 5, 3, 4))
    assert LS.casorati(x[0]).shape == (12, 5) and np.array_equal(LS.uncasorati(LS.casorati(x[0]), x[0].shape), x[0])
    same, nuc = LS.svt(x, 0.0)
    assert np.allclose(same, x) and np.allclose(nuc, [np.linalg.svd(LS.casorati(v), compute_uv=False).sum() for v in x])
    none, nuc = LS.svt(x, 1.5 * LS.sigma_max(x))
    assert not none.any() and not nuc.any()
    g = LS.gram(x)
    assert g.shape == (2, 5, 5) and np.allclose(g, np.conj(np.swapaxes(g, 1, 2)))
    assert np.allclose(LS.gram_sqrt(g[0]) @ LS.gram_sqrt(g[0]), g[0])
