"""cine_hip.grappa without a GPU: the lattice masks and the host plan, the argument errors of ``grappa``, and the float64 reference
(tests/grappa_reference.py) on the synthetic phantom -- the GPU tests compare against that reference, so it must reconstruct."""
import numpy as np
import pytest
import torch

import grappa_reference as ref
from cine_hip import grappa as G
from cine_hip._lib import CineHipError

# t, c, h, w, R, (ky, kx): the shapes of the issue's table; GRAPPA NRMSE 0.096 / 0.199 / 0.045 against 0.667 / 0.727 / 0.631 zero-filled
PHANTOM_SHAPES = [(6, 8, 48, 40, 3, (2, 5)), (8, 8, 48, 40, 4, (2, 5)), (5, 6, 30, 22, 2, (2, 3))]


# ------------------------------------------------------------------ masks and the plan
@pytest.mark.parametrize("interleave", [True, False])
@pytest.mark.parametrize("t,h,accel,acs", [(5, 13, 3, 0), (8, 48, 4, 0), (6, 48, 3, 12), (3, 9, 8, 0), (4, 30, 2, 7)])
def test_lattice_mask_and_plan(t, h, accel, acs, interleave):
    m = G.lattice_mask(t, h, accel, acs=acs, interleave=interleave)
    assert m.dtype == torch.uint8 and tuple(m.shape) == (1, t, 1, h, 1, 1)
    rows = m.numpy().reshape(t, h)
    lo = h // 2 - acs // 2
    for f in range(t):
        want = np.zeros(h, np.uint8)
        want[(f % accel if interleave else 0)::accel] = 1
        want[lo:lo + acs] = 1
        assert (rows[f] == want).all()
    assert (rows == ref.lattice_mask(t, h, accel, acs=acs, interleave=interleave)).all()
    off = G.plan_lattice(m, accel)
    assert off.dtype == np.int32 and off.shape == (1, t)
    want = [(f % accel if interleave else 0) for f in range(t)]
    if acs >= h:                                                       # everything acquired
        want = [0] * t
    assert off[0].tolist() == want                                     # an ACS block does not disturb the rule
    assert G.plan_lattice(rows, accel).tolist() == want                # the (t, h) form
    assert ref.offsets(rows, accel)[0].tolist() == want


def test_plan_every_residue_and_extras():
    h, R = 17, 5
    for r in range(R):
        rows = np.zeros((1, h), np.uint8)
        rows[0, r::R] = 1
        rows[0, (r + 2) % h] = 1                                       # a stray extra row
        assert G.plan_lattice(rows, R).tolist() == [r]
    full = np.ones((2, h), np.uint8)
    assert G.plan_lattice(full, R).tolist() == [0, 0]                  # fully sampled: offset 0
    both = np.zeros((1, 12), np.uint8)
    both[0, 1::4] = 1
    both[0, 3::4] = 1
    assert G.plan_lattice(both, 4).tolist() == [1]                     # two lattices: the lowest residue


def test_plan_raises_for_a_frame_without_a_lattice():
    rows = ref.lattice_mask(4, 20, 4)
    rows[2, 6] = 0                                                     # frame 2 (offset 2) loses a lattice row
    with pytest.raises(ValueError, match="frame 2"):
        G.plan_lattice(rows, 4)
    with pytest.raises(ValueError, match="frame 2 of batch element 0"):
        G.plan_lattice(torch.from_numpy(rows.reshape(1, 4, 1, 20, 1, 1)), 4)
    off, status = ref.offsets(rows, 4)
    assert off.tolist() == [0, 1, -1, 3] and status.tolist() == [0, 0, 1, 0]
    with pytest.raises(ValueError):
        G.plan_lattice(np.zeros((2, 3, 4)), 2)


def test_argument_errors_raise_without_a_device():
    k = torch.zeros(1, 4, 3, 24, 16, 2)
    m = G.lattice_mask(4, 24, 3)
    for kw in ({"accel": 1}, {"accel": 9}, {"accel": 2.5}, {"accel": 3, "kernel": (3, 5)}, {"accel": 3, "kernel": (2, 4)}, {"accel": 3, "kernel": 5},
               {"accel": 3, "lam": 0.0}, {"accel": 3, "lam": -1.0}, {"accel": 3, "lam": float("nan")}, {"accel": 3, "calib": "kt"},
               {"accel": 3, "calib": "acs"}, {"accel": 3, "acs": (10, 9)}, {"accel": 3, "acs": (0, 25)}, {"accel": 3, "output": "image"},
               {"accel": 3, "output": "complex"}, {"accel": 3, "calib_rows": 3}, {"accel": 3, "acs": (10, 13)},
               {"accel": 8, "kernel": (4, 7), "calib_rows": 24}):
        with pytest.raises(ValueError):
            G.grappa(k, m, **kw)
    with pytest.raises(ValueError):                                    # 33 coils
        G.grappa(torch.zeros(1, 2, 33, 24, 16, 2), G.lattice_mask(2, 24, 2), accel=2)
    with pytest.raises(ValueError):                                    # w < kx
        G.grappa(torch.zeros(1, 2, 3, 24, 4, 2), G.lattice_mask(2, 24, 2), accel=2)
    with pytest.raises(ValueError):
        G.grappa(k[0], m, accel=3)                                     # no batch axis
    with pytest.raises(CineHipError, match="GPU tensors"):             # valid settings, CPU tensors: there is no fallback
        G.grappa(k, m, accel=3)
    with pytest.raises(CineHipError, match="requires grad"):
        G.grappa(k.clone().requires_grad_(), m, accel=3)
    with pytest.raises(ValueError):
        G.Grappa(accel=1)
    with pytest.raises(ValueError):
        G.Grappa(accel=3, calib="acs")
    mod = G.Grappa(accel=3, kernel=(4, 5), lam=1e-3, acs=(6, 18))
    assert (mod.accel, mod.kernel, mod.lam, mod.acs) == (3, (4, 5), 1e-3, (6, 18)) and not list(mod.parameters())


def test_exports():
    import cine_hip
    assert cine_hip.grappa is G and cine_hip.Grappa is G.Grappa and cine_hip.lattice_mask is G.lattice_mask
    from cine_hip import pipeline
    assert pipeline._forward_params(G.Grappa(accel=2)) == (True, False)          # takes maps, does not need them


# ------------------------------------------------------------------ the reference reconstructs
@pytest.fixture(scope="module")
def phantoms():
    return {s: ref.phantom_slice(*s[:5]) for s in PHANTOM_SHAPES}


@pytest.mark.parametrize("shape", PHANTOM_SHAPES, ids=lambda s: "t%d-c%d-%dx%d-R%d-k%dx%d" % (s[:5] + s[5]))
def test_reference_beats_zero_filling_by_half(phantoms, shape):
    t, c, h, w, R, kernel = shape
    k, mask, mk = phantoms[shape]
    filled, info, off = ref.grappa(mk, mask, R, kernel, 1e-4, calib="tgrappa", calib_rows=h)
    assert off.tolist() == [f % R for f in range(t)]
    full = ref.rss(k)
    e_grappa, e_zero = ref.nrmse(ref.rss(filled), full), ref.nrmse(ref.rss(mk), full)
    print(f"NRMSE GRAPPA {e_grappa:.3f}, zero-filled {e_zero:.3f}, info {info}")
    assert e_grappa <= 0.5 * e_zero
    acquired = mask.astype(bool)
    assert (filled[acquired.nonzero()[0], :, acquired.nonzero()[1]] == mk[acquired.nonzero()[0], :, acquired.nonzero()[1]]).all()
    missing = ~acquired
    assert (np.abs(filled).sum(axis=(1, 3))[missing] > 0).all()       # every missing row is filled
    assert info[0] < 1e-12 and 0 < info[2] < 1
    cal = ref.calibration_data(mk, mask, "tgrappa", None, h)
    g = ref.geom(c, R, *kernel)
    Gm = ref.gram(cal, R, *kernel)
    assert Gm.shape == (g["n_aug"], g["n_aug"]) and np.abs(Gm - Gm.conj().T).max() <= 1e-12 * np.abs(Gm).max()
    cond = np.linalg.cond(Gm[:g["ns"], :g["ns"]] + info[1] * np.eye(g["ns"]))
    assert 1e3 < cond < g["ns"] / 1e-4 + 1                            # 4e3 .. 8e3 measured; ns / lam + 1 bounds it by construction


def test_reference_weights_reproduce_the_calibration_targets():
    """On noise-free data that the kernel can represent exactly (one coil, a k-space that is a geometric sequence along h), the
    targets are predicted exactly: a check of the source / target bookkeeping that does not go through the phantom."""
    R, ky, kx = 3, 2, 3
    h, w = 24, 9
    y = np.arange(h)[:, None]
    cal = (np.exp(0.05j * y) * 0.98 ** y * (1.0 + 0.1 * np.arange(w)[None, :]))[None].astype(np.complex64)
    W, info = ref.weights(ref.gram(cal, R, ky, kx), 1, R, ky, kx, 1e-9)
    assert info[2] < 1e-3
    k = cal[None]                                                      # one frame (1, 1, h, w)
    mask = ref.lattice_mask(1, h, R, offsets=[1])
    out = ref.apply(k * mask[:, None, :, None], W, mask, [1], R, ky, kx)
    inner = slice(1 + R, h - R)                                        # targets with both source rows inside, away from the column edges
    assert np.abs(out[0, 0, inner, 1:-1] - k[0, 0, inner, 1:-1]).max() < 1e-3


def test_reference_acs_variant(phantoms):
    t, c, h, w, R, kernel = PHANTOM_SHAPES[0]
    k, mask, mk = ref.phantom_slice(t, c, h, w, R, acs=12)
    lo = h // 2 - 6
    assert ref.offsets(mask, R)[0].tolist() == [f % R for f in range(t)]
    filled, info, _ = ref.grappa(mk, mask, R, kernel, 1e-4, acs=(lo, lo + 12))
    same, _, _ = ref.grappa(mk, mask, R, kernel, 1e-4, calib="acs", acs=(lo, lo + 12))
    assert (filled == same).all()
    full = ref.rss(k)
    e_grappa, e_zero = ref.nrmse(ref.rss(filled), full), ref.nrmse(ref.rss(mk), full)
    print(f"ACS: NRMSE GRAPPA {e_grappa:.3f}, zero-filled {e_zero:.3f}")
    assert e_grappa < e_zero                                           # 0.092 against 0.124
    with pytest.raises(ValueError):                                    # TGRAPPA over rows nobody acquired
        ref.calibration_data(mk * 0, np.zeros_like(mask), "tgrappa", None, 8)
