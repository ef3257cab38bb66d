"""The locally low-rank baseline without a GPU: the ABI table carries the new entry points, the public functions are exported and refuse
what they cannot do, the C entry points refuse bad arguments before their first launch (so no GPU is needed to see it), and the float64
yardstick (tests/llr_reference.py) is itself checked -- with a fixed partition and the default step an iteration never increases the
objective, one block over the whole image is the global SVT of tests/ls_reference.py, and the seeded shifts remove enough of the
aliasing -- before the kernels are compared with it."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import kt_reference as R
import llr_reference as LLR
import ls_reference as LS
from conftest import ROOT

NEW = ("cine_llr_prox_ws_bytes", "cine_llr_prox", "cine_llr_solve_ws_bytes", "cine_llr_solve")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


def test_the_header_declares_the_prototypes_and_the_table_carries_them():
    from cine_hip import _lib
    with open(os.path.join(ROOT, "include", "cine_hip.h")) as f:
        text = f.read()
    for name in NEW:
        assert f" {name}(" in text and name in _lib._SIGS and name in _lib.declared_symbols(), name
        assert hasattr(_lib.lib(), name), name
    i, p, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib._SIGS["cine_llr_prox_ws_bytes"] == (sz, [i] * 7)
    assert _lib._SIGS["cine_llr_prox"] == (i, [p, p, p, p, i, i, i, p, p, p, i, i, i, i, p, sz, p])
    assert _lib._SIGS["cine_llr_solve_ws_bytes"] == (sz, [i] * 8)
    assert _lib._SIGS["cine_llr_solve"] == (i, [p] * 5 + [i, p, p, i, p, i, p, p, i, i, i, i, i, p, sz, p])


def test_exports_and_the_signature_the_pipeline_dispatches_on():
    import cine_hip
    from cine_hip import classical, ops, pipeline
    assert cine_hip.locally_low_rank is classical.locally_low_rank and cine_hip.LocallyLowRank is classical.LocallyLowRank
    assert "locally_low_rank" in cine_hip.__all__ and "LocallyLowRank" in cine_hip.__all__
    for name in ("llr_shifts", "block_sigma_max", "locally_low_rank", "LocallyLowRank"):
        assert name in classical.__all__, name
    assert pipeline._forward_params(classical.LocallyLowRank()) == (True, True)
    assert list(inspect.signature(classical.LocallyLowRank.forward).parameters) == ["self", "masked_kspace", "mask", "sens_maps", "output"]
    assert not list(classical.LocallyLowRank().parameters())
    assert callable(ops.llr_prox) and callable(ops.llr_solve) and ops.LLR_REC == 4 and ops.LLR_INFO == 4
    d = inspect.signature(classical.locally_low_rank).parameters
    assert (d["iters"].default, d["lam"].default, d["block"].default, d["shifts"].default) == (LLR.ITERS, LLR.LAM, LLR.BLOCK, "random")


def test_cpu_tensors_inputs_that_require_grad_and_bad_settings_are_refused():
    from cine_hip import classical, ops
    from cine_hip._lib import CineHipError
    p = R.problem((1, 5, 3, 24, 20), "row")
    mk, mask, sens = p["masked_kspace"], p["mask"], p["sens_maps"]
    model = classical.LocallyLowRank(iters=3).eval()
    with pytest.raises(CineHipError, match="GPU"):
        classical.locally_low_rank(mk, mask, sens)
    with pytest.raises(CineHipError, match="GPU"):
        model(mk, mask, sens)
    one, img = torch.ones(1), torch.zeros(1, 2, 3, 4, 2)
    with pytest.raises(CineHipError, match="GPU"):
        ops.llr_prox(img, img.clone(), one, one, 8)
    with pytest.raises(CineHipError, match="GPU"):
        ops.llr_solve(torch.zeros(1, 5, 1, 24, 20, 2), sens, mask, one, one, 8, 3)
    with pytest.raises(CineHipError, match="GPU"):
        classical.block_sigma_max(img, 8)
    with torch.enable_grad():
        for kw in ({"masked_kspace": mk.clone().requires_grad_(True)}, {"sens_maps": sens.clone().requires_grad_(True)}):
            args = {"masked_kspace": mk, "mask": mask, "sens_maps": sens, **kw}
            with pytest.raises(CineHipError, match="locally_low_rank: .* requires grad, but the solver is not differentiable"):
                classical.locally_low_rank(**args)
            with pytest.raises(CineHipError, match="requires grad"):
                model(args["masked_kspace"], args["mask"], args["sens_maps"])
    with pytest.raises(ValueError, match="iters = 0"):
        classical.locally_low_rank(mk, mask, sens, iters=0)
    with pytest.raises(ValueError, match="iters = 0"):
        classical.LocallyLowRank(iters=0)
    for block in (1, 17):
        with pytest.raises(ValueError, match=f"block = {block}"):
            classical.locally_low_rank(mk, mask, sens, block=block)
        with pytest.raises(ValueError, match=f"block = {block}"):
            classical.LocallyLowRank(block=block)
    good = np.zeros((4, 2), dtype=np.int64)
    bad = {"the wrong shape": np.zeros((3, 2), dtype=np.int64), "one column": np.zeros((4,), dtype=np.int64), "floats": np.zeros((4, 2)),
           "a negative entry": np.array([[0, 0], [0, 0], [0, 0], [0, -1]]), "an entry = block": np.array([[0, 0], [8, 0], [0, 0], [0, 0]])}
    for name, s in bad.items():
        with pytest.raises(ValueError, match="shifts"):
            classical.locally_low_rank(mk, mask, sens, iters=4, shifts=s)
        with pytest.raises(ValueError, match="shifts"):
            classical.LocallyLowRank(iters=4, shifts=s)
    with pytest.raises(ValueError, match="shifts"):
        classical.locally_low_rank(mk, mask, sens, shifts="spin")
    with pytest.raises(CineHipError, match="GPU"):                 # a good array passes the host checks and reaches the device check
        classical.locally_low_rank(mk, mask, sens, iters=4, shifts=good)
    for s in (None, "fixed"):
        assert classical.LocallyLowRank(shifts=s).shifts is None
    with pytest.raises(ValueError):
        classical.locally_low_rank(mk, mask, sens, output="phase")


def test_the_seeded_shifts_are_the_contract():
    from cine_hip import classical
    for iters, block, seed in ((30, 8, 0), (7, 3, 5), (1, 16, 2), (50, 2, 0)):
        got = classical.llr_shifts(iters, block, seed)
        assert got.dtype == np.int32 and got.shape == (iters, 2) and got.min() >= 0 and got.max() < block
        assert np.array_equal(got, LLR.shifts(iters, block, seed))
        assert np.array_equal(got, np.random.RandomState(seed).randint(0, block, size=(iters, 2)))
    assert np.array_equal(classical.LocallyLowRank().shifts, LLR.shifts(LLR.ITERS, LLR.BLOCK, 0))
    assert len({tuple(r) for r in classical.llr_shifts(30, 8).tolist()}) > 10              # it does move


# ------------------------------------------------------------------ refusals through the C ABI: every argument is checked before the first launch
def fake(n):
    return ctypes.c_void_p(0x10000 * (n + 1))                       # never dereferenced; 16-byte aligned


def refused(L, code, want, name, what):
    assert L.cine_scale(None, 1, 1.0, None) == EINVAL and L.cine_last_error().startswith(b"cine_scale")
    got = code()
    msg = L.cine_last_error().decode(errors="replace")
    assert got == want, f"{what}: returned {got}, expected {want} ({msg})"
    assert msg.startswith(name), f"{what}: the message is not this call's: {msg!r}"


def test_llr_prox_rejects_bad_arguments_before_any_launch():
    from cine_hip import _lib
    L = _lib.lib()
    base = dict(x=fake(0), g=fake(1), step=fake(2), thresh=fake(3), block=8, sh=0, sw=0, xnew=fake(4), rec=fake(5), info=fake(6),
                b=1, t=5, h=9, w=17, ws=fake(7), nbytes=1 << 40)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L.cine_llr_prox(a["x"], a["g"], a["step"], a["thresh"], a["block"], a["sh"], a["sw"], a["xnew"], a["rec"], a["info"],
                                       a["b"], a["t"], a["h"], a["w"], a["ws"], a["nbytes"], None)
    need = L.cine_llr_prox_ws_bytes(1, 5, 9, 17, 8, 0, 0)
    assert need == (1 + 2 * 3) * 64 and L.cine_llr_prox_ws_bytes(1, 5, 9, 17, 8, 7, 1) == (1 + 2 * 3) * 64
    assert L.cine_llr_prox_ws_bytes(2, 5, 8, 8, 8, 0, 0) == (1 + 2) * 64 and L.cine_llr_prox_ws_bytes(1, 5, 8, 8, 8, 3, 5) == (1 + 4) * 64
    assert L.cine_llr_prox_ws_bytes(1, 5, 200, 200, 8, 0, 0) == (1 + 625) * 64 and L.cine_llr_prox_ws_bytes(1, 5, 200, 200, 8, 1, 1) == (1 + 676) * 64
    for bad in (dict(t=1), dict(t=65), dict(block=1), dict(block=17), dict(sh=-1), dict(sw=8), dict(b=0)):
        a = {**dict(b=1, t=5, h=9, w=17, block=8, sh=0, sw=0), **bad}
        assert L.cine_llr_prox_ws_bytes(a["b"], a["t"], a["h"], a["w"], a["block"], a["sh"], a["sw"]) == 0, bad
    for kw, want in ((dict(t=1), EUNSUPPORTED), (dict(t=65), EUNSUPPORTED), (dict(block=1), EUNSUPPORTED), (dict(block=17), EUNSUPPORTED),
                     (dict(b=65536), EUNSUPPORTED), (dict(sh=-1), EINVAL), (dict(sh=8), EINVAL), (dict(sw=-1), EINVAL), (dict(sw=8), EINVAL),
                     (dict(block=3, sh=3), EINVAL), (dict(x=None), EINVAL), (dict(thresh=None), EINVAL), (dict(step=None), EINVAL),
                     (dict(b=0), EINVAL), (dict(t=0), EINVAL), (dict(h=0), EINVAL), (dict(w=-1), EINVAL), (dict(block=0), EINVAL),
                     (dict(ws=None), EINVAL), (dict(ws=None, rec=None), EINVAL), (dict(ws=ctypes.c_void_p(0x80008)), EINVAL),
                     (dict(info=ctypes.c_void_p(0x70004)), EINVAL), (dict(xnew=base["g"]), EINVAL), (dict(rec=base["x"]), EINVAL),
                     (dict(info=base["xnew"]), EINVAL), (dict(ws=base["rec"]), EINVAL), (dict(xnew=base["thresh"]), EINVAL),
                     (dict(nbytes=need - 1), EWORKSPACE), (dict(nbytes=0), EWORKSPACE)):
        refused(L, call(**kw), want, "cine_llr_prox", f"cine_llr_prox {kw}")


def test_llr_solve_rejects_bad_arguments_before_any_launch():
    from cine_hip import _lib
    L = _lib.lib()
    iters = 4
    good = (ctypes.c_int * (2 * iters))(*[3, 5, 0, 7, 7, 0, 1, 1])
    base = dict(x=fake(0), zf=fake(1), sens=fake(2), mask=fake(3), mask_w=1, step=fake(4), thresh=fake(5), block=8, shifts=good, iters=iters,
                rec=fake(6), info=fake(7), b=1, t=5, c=3, h=24, w=20, ws=fake(8), nbytes=1 << 40)

    def call(**kw):
        a = {**base, **kw}
        return lambda: L.cine_llr_solve(a["x"], a["zf"], a["sens"], None, a["mask"], a["mask_w"], a["step"], a["thresh"], a["block"], a["shifts"],
                                        a["iters"], a["rec"], a["info"], a["b"], a["t"], a["c"], a["h"], a["w"], a["ws"], a["nbytes"], None)
    need = L.cine_llr_solve_ws_bytes(1, 5, 3, 24, 20, 1, 8, iters)
    assert need > L.cine_llr_solve_ws_bytes(1, 5, 3, 24, 20, 1, 8, iters - 1) > 5 * 24 * 20 * 8
    # the rows of records are sized for the worst case over all shifts: (ceil(31 / 8) x ceil(27 / 8) = 4 x 4 blocks and a header) x 64 bytes
    assert need - L.cine_llr_solve_ws_bytes(1, 5, 3, 24, 20, 1, 8, iters - 1) == (1 + 16) * 64
    for bad in (dict(t=1), dict(t=65), dict(block=1), dict(block=17), dict(iters=0), dict(c=0)):
        a = {**dict(b=1, t=5, c=3, h=24, w=20, block=8, iters=iters), **bad}
        assert L.cine_llr_solve_ws_bytes(a["b"], a["t"], a["c"], a["h"], a["w"], 1, a["block"], a["iters"]) == 0, bad

    def shifts_with(last):
        v = list(good)
        v[-2:] = last
        return (ctypes.c_int * (2 * iters))(*v)
    for kw, want in ((dict(t=1), EUNSUPPORTED), (dict(t=65), EUNSUPPORTED), (dict(block=1), EUNSUPPORTED), (dict(block=17), EUNSUPPORTED),
                     (dict(iters=0), EINVAL), (dict(c=0), EINVAL), (dict(mask_w=2), EINVAL), (dict(x=None), EINVAL), (dict(zf=None), EINVAL),
                     (dict(thresh=None), EINVAL), (dict(ws=None), EINVAL), (dict(shifts=shifts_with((0, 8))), EINVAL),
                     (dict(shifts=shifts_with((-1, 0))), EINVAL), (dict(ws=ctypes.c_void_p(0x90008)), EINVAL), (dict(x=base["zf"]), EINVAL),
                     (dict(rec=base["x"]), EINVAL), (dict(info=base["rec"]), EINVAL), (dict(nbytes=need - 1), EWORKSPACE)):
        refused(L, call(**kw), want, "cine_llr_solve", f"cine_llr_solve {kw}")
    refused(L, call(h=401), EUNSUPPORTED, "cine_llr_solve", "cine_llr_solve h = 401 (the operator's refusal)")
    assert b"cine_image_dc" in L.cine_last_error()


# ------------------------------------------------------------------ the yardstick
def test_the_partition_covers_every_pixel_once():
    for h, w, block, sh, sw in ((1, 1, 8, 0, 0), (7, 9, 8, 0, 0), (8, 8, 8, 3, 5), (9, 17, 8, 7, 1), (19, 13, 8, 0, 7), (35, 19, 16, 15, 1),
                                (9, 4, 3, 2, 1), (200, 200, 8, 1, 1)):
        seen = np.zeros((h, w), dtype=int)
        bl = LLR.blocks(h, w, block, sh, sw)
        for r0, r1, c0, c1 in bl:
            assert 0 <= r0 < r1 <= h and 0 <= c0 < c1 <= w and r1 - r0 <= block and c1 - c0 <= block
            seen[r0:r1, c0:c1] += 1
        assert (seen == 1).all() and len(bl) == -(-(h + sh) // block) * -(-(w + sw) // block)
    assert LLR.blocks(8, 8, 8, 3, 5) == [(0, 5, 0, 3), (0, 5, 3, 8), (5, 8, 0, 3), (5, 8, 3, 8)]


def test_one_block_over_the_whole_image_is_the_global_svt():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((2, 5, 7, 6)) + 1j * rs.standard_normal((2, 5, 7, 6))
    theta = 0.4 * LS.sigma_max(x)
    got, nuc, smax = LLR.block_svt(x, theta, 8)
    want, want_nuc = LS.svt(x, theta)
    assert np.allclose(got, want, rtol=0, atol=1e-12) and abs(nuc - want_nuc.sum()) <= 1e-12 * nuc and abs(smax - LS.sigma_max(x)) <= 1e-12 * smax
    same, _, _ = LLR.block_svt(x, 0.0, 3, 2, 1)
    assert np.allclose(same, x, rtol=0, atol=1e-12)
    none, nuc, smax = LLR.block_svt(x, 1.01 * LLR.block_sigma_max(x, 3), 3)
    assert not none.any() and nuc == 0.0 and smax == LLR.block_sigma_max(x, 3)


@pytest.mark.parametrize("shape,layout", LLR.FIXTURES, ids=["row", "plane"])
def test_with_a_fixed_partition_the_yardstick_never_increases_the_objective(shape, layout):
    """step = 1 / max sum |S|^2 <= 1 / ||A^H M A||: ISTA, a descent step.  Measured: the objective ends at 0.79 (row) and 0.73 (plane) of its start."""
    _, _, obj = LLR.solved(shape, layout, shifted=False, rounded=False)
    print(f"{shape} {layout}: objective {obj[0]:.6g} -> {obj[-1]:.6g} ({obj[-1] / obj[0]:.3f}), largest increase {np.diff(obj).max() / obj[0]:.2e}")
    assert obj.shape == (LLR.ITERS + 1,)
    assert np.all(np.diff(obj) <= 1e-12 * obj[0]), obj
    assert obj[-1] < 0.9 * obj[0]


@pytest.mark.parametrize("shape,layout,bound", [(*LLR.FIXTURES[0], 0.75), (*LLR.FIXTURES[1], 0.6)], ids=["row", "plane"])
def test_the_yardstick_with_seeded_shifts_beats_the_zero_filled_image(shape, layout, bound):
    """30 iterations, seed-0 shifts.  Measured: 0.64 of the zero-filled NRMSE on the 5-frame row fixture, 0.50 on the plane fixture."""
    p = R.problem(shape, layout)
    truth = p["target"].numpy()
    x, rec, _ = LLR.solved(shape, layout, shifted=True, rounded=False)
    got, zero_filled = R.nrmse(np.abs(x), truth), R.nrmse(np.abs(p["zf"]), truth)
    fixed = R.nrmse(np.abs(LLR.solved(shape, layout, shifted=False, rounded=False)[0]), truth)
    print(f"{shape} {layout}: NRMSE zero-filled {zero_filled:.3f}, fixed partition {fixed:.3f}, seeded shifts {got:.3f} ({got / zero_filled:.2f} of zero-filled)")
    assert got <= bound * zero_filled
    assert rec.shape == (LLR.ITERS, 4) and (rec[:, :3] > 0).all() and not rec[:, 3].any()
