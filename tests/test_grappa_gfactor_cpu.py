"""The closed form behind cine_grappa_image_weights / cine_grappa_gfactor, checked in float64 numpy without a GPU
(tests/grappa_gfactor_reference.py), and the host side of the new functions of cine_hip.grappa.

(a) signs and centring: ifft2c(K applied circularly to z) == Wimg ifft2c(z) to 1e-12 on a lattice of every offset;
(b) the variance formula, exactly: the dense linear operator (lattice samples -> circular application -> ifft2c -> combination) A gives
    diag(A (I x Psi) A^H) == amp^2 / R to 1e-12;
(c) away from the frame's edges the circular application is tests/grappa_reference.py's ``apply``;
(d) the header declares the two entry points and the derived ctypes table carries them;
(e) exports and what is refused before a device is asked for."""
from ctypes import c_int, c_void_p

import numpy as np
import pytest
import torch

import grappa_gfactor_reference as gref
import grappa_reference as ref
from cine_hip import _lib, grappa as G
from cine_hip._lib import CineHipError

# c, h, w, R, ky, kx
SHAPES = [(3, 12, 10, 3, 2, 5), (2, 21, 9, 4, 4, 3), (2, 16, 7, 2, 2, 7), (1, 9, 8, 8, 2, 3)]


def crandn(rs, *shape):
    return rs.standard_normal(shape) + 1j * rs.standard_normal(shape)


def weights_of(rs, c, R, ky, kx):
    return crandn(rs, R - 1, ky * kx * c, c) / np.sqrt(ky * kx * c)


def lattice(rs, c, h, w, R, off):
    z = np.zeros((c, h, w), np.complex128)
    z[:, off::R] = crandn(rs, c, len(range(off, h, R)), w)
    return z


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d-%dx%d-R%d-k%dx%d" % s)
def test_image_weights_are_the_transform_of_the_circular_application(shape):
    c, h, w, R, ky, kx = shape
    rs = np.random.RandomState(sum(shape))
    W = weights_of(rs, c, R, ky, kx)
    Wimg = gref.image_weights(W, c, R, ky, kx, h, w)
    assert Wimg.shape == (c, c, h, w)
    for off in range(R):
        z = lattice(rs, c, h, w, R, off)
        want = gref.ifft2c(gref.circular_apply(z, W, R, ky, kx))
        got = np.einsum("qkyx,kyx->qyx", Wimg, gref.ifft2c(z))
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (shape, off)


def test_combined_kernel_layout():
    c, R, ky, kx = 2, 3, 4, 5
    rs = np.random.RandomState(3)
    W = weights_of(rs, c, R, ky, kx)
    K, dys = gref.combined_kernel(W, c, R, ky, kx)
    base, hx = (ky // 2 - 1) * R, kx // 2
    assert len(dys) == 1 + (R - 1) * ky and dys == sorted(dys) and K.shape == (c, c, len(dys), kx)
    assert all(dy % R != 0 for dy in dys if dy != 0)                                   # only the identity tap hits a lattice row
    zero = dys.index(0)
    assert (K[:, :, zero, hx] == np.eye(c)).all() and np.abs(K[:, :, zero]).sum() == c
    for m in range(1, R):
        for j in range(ky):
            for dx in range(kx):
                for k in range(c):
                    for q in range(c):
                        assert K[q, k, dys.index(-m - base + j * R), dx] == W[m - 1][(j * kx + dx) * c + k][q]


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("with_coef", [True, False])
def test_variance_formula_against_the_dense_operator(R, with_coef):
    c, h, w, ky, kx = 2, 6, 4, 2, 3
    rs = np.random.RandomState(10 + R)
    W = weights_of(rs, c, R, ky, kx)
    M = crandn(rs, c, c)
    psi = M @ M.conj().T + 0.5 * np.eye(c)
    L = np.linalg.cholesky(psi)
    p = crandn(rs, 1, c, h, w) if with_coef else None
    g, amp = gref.gfactor(W, c, R, ky, kx, h, w, chol=L, coef=p)
    for off in range(R):
        rows = list(range(off, h, R))
        A = np.zeros((c if p is None else 1, h * w, len(rows) * w, c), np.complex128)  # [combination][pixel][sample][coil]
        for s, (y, x) in enumerate((y, x) for y in rows for x in range(w)):
            for k in range(c):
                z = np.zeros((c, h, w), np.complex128)
                z[k, y, x] = 1.0
                img = gref.ifft2c(gref.circular_apply(z, W, R, ky, kx))
                comb = img if p is None else np.einsum("nqyx,qyx->nyx", p, img)
                A[:, :, s, k] = comb.reshape(comb.shape[0], -1)
        var = np.einsum("npsk,kl,npsl->np", A, psi, A.conj()).real.reshape(-1, h, w)
        assert np.abs(var - amp ** 2 / R).max() <= 1e-12 * var.max(), (R, off)
        # the fully sampled acquisition: every sample carries noise and nothing is predicted, var_full = p Psi p^H
        if p is None:
            full = np.broadcast_to(np.diagonal(psi).real[:, None, None], (c, h, w))
        else:
            full = np.einsum("nqyx,ql,nlyx->nyx", p, psi, p.conj()).real
        assert np.abs(np.sqrt(var / full / R) - g).max() <= 1e-12 * g.max()


def test_gfactor_is_zero_where_the_combination_is():
    c, h, w, R, ky, kx = 2, 5, 4, 2, 2, 3
    rs = np.random.RandomState(5)
    p = crandn(rs, 1, c, h, w)
    p[0, :, 2, 1] = 0
    g, amp = gref.gfactor(weights_of(rs, c, R, ky, kx), c, R, ky, kx, h, w, coef=p)
    assert g[0, 2, 1] == 0 and amp[0, 2, 1] == 0 and (np.delete(g.ravel(), 2 * w + 1) > 0).all()
    g, amp = gref.gfactor(np.zeros((R - 1, ky * kx * c, c)), c, R, ky, kx, h, w)      # zero weights: zero filling, amp = 1, g = 1 / R
    assert np.abs(amp - 1).max() <= 1e-15 and np.abs(g - 1 / R).max() <= 1e-15


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "c%d-%dx%d-R%d-k%dx%d" % s)
def test_circular_application_is_the_reference_apply_away_from_the_edges(shape):
    c, h, w, R, ky, kx = shape
    rs = np.random.RandomState(7 + sum(shape))
    W = weights_of(rs, c, R, ky, kx)
    dys = gref.row_offsets(R, ky)
    ys, xs = slice(-min(dys), h - max(dys)), slice(kx // 2, w - kx // 2)
    assert ys.stop - ys.start >= 1 and xs.stop - xs.start >= 1
    z = np.stack([lattice(rs, c, h, w, R, off) for off in range(R)])
    mask = ref.lattice_mask(R, h, R, offsets=list(range(R)))
    want = ref.apply(z, W, mask, np.arange(R), R, ky, kx)
    for off in range(R):
        got = gref.circular_apply(z[off], W, R, ky, kx)
        assert np.abs(got[:, ys, xs] - want[off][:, ys, xs]).max() <= 1e-12 * np.abs(want).max(), (shape, off)
        kept = [y for y in range(ys.start, ys.stop) if (y - off) % R == 0]             # acquired rows are kept, exactly (at the edges
        assert kept and (got[:, kept] == z[off][:, kept]).all()                        # the wrap can land on a lattice row: h mod R != 0)


def test_the_header_declares_the_entry_points():
    P = c_void_p
    assert _lib._SIGS_ERROR is None
    assert _lib._SIGS["cine_grappa_image_weights"] == (c_int, [P, P, c_int, c_int, c_int, c_int, c_int, c_int, P])
    assert _lib._SIGS["cine_grappa_gfactor"] == (c_int, [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P])
    assert {"cine_grappa_image_weights", "cine_grappa_gfactor"} <= set(_lib.declared_symbols())


def test_exports():
    import cine_hip
    for name in ("grappa_image_weights", "grappa_gfactor_from_weights", "grappa_noise_maps"):
        assert name in G.__all__ and name in cine_hip.__all__ and getattr(cine_hip, name) is getattr(G, name)
    assert "GfactorMaps" in G.__all__ and G.GfactorMaps._fields == ("g", "std") and callable(G.Grappa.noise_maps)


def test_refusals_without_a_device():
    c, h, w, R, kernel = 3, 24, 16, 3, (2, 5)
    k = torch.zeros(1, 4, c, h, w, 2)
    m = G.lattice_mask(4, h, R)
    wts = torch.zeros(R - 1, 2 * 5 * c, c, 2)
    with pytest.raises(ValueError, match="shift-invariant"):                           # unevenly spaced rows have no closed form
        G.grappa_noise_maps(k, m, None)
    with pytest.raises(ValueError, match="shift-invariant"):
        G.Grappa(accel=None).noise_maps(k, m)
    for bad in (torch.zeros(c + 1, c + 1, 2), torch.zeros(c, c), torch.zeros(c, c, 2, dtype=torch.float64),
                torch.zeros(c, c - 1, dtype=torch.complex64)):
        with pytest.raises(ValueError, match="chol must be"):
            G.grappa_gfactor_from_weights(wts, R, kernel, h, w, chol=bad)
    with pytest.raises(TypeError):
        G.grappa_gfactor_from_weights(wts, R, kernel, h, w, chol=np.eye(c))
    for kw in ({"accel": 1}, {"accel": 9}, {"kernel": (3, 5)}, {"kernel": (2, 4)}, {"h": 0}, {"w": 0}, {"accel": 4},
               {"weights": torch.zeros(R - 1, 2 * 5 * c + 1, c, 2)}, {"weights": torch.zeros(R - 1, 2 * 5 * c, c)}):
        args = {"weights": wts, "accel": R, "kernel": kernel, "h": h, "w": w, **kw}
        with pytest.raises(ValueError):
            G.grappa_gfactor_from_weights(**args)
        with pytest.raises(ValueError):
            G.grappa_image_weights(**args)
    with pytest.raises(ValueError, match="at most 32 coils"):
        G.grappa_image_weights(torch.zeros(1, 2 * 3 * 33, 33, 2), 2, (2, 3), h, w)
    for call in (lambda: G.grappa_image_weights(wts, R, kernel, h, w), lambda: G.grappa_gfactor_from_weights(wts, R, kernel, h, w),
                 lambda: G.grappa_gfactor_from_weights(wts, R, kernel, h, w, chol=torch.zeros(c, c, dtype=torch.complex64))):
        with pytest.raises(CineHipError):                                              # valid arguments, CPU tensors: there is no fallback
            call()
    with pytest.raises(CineHipError, match="GPU tensors"):
        G.grappa_noise_maps(k, m, R)
    with pytest.raises(CineHipError, match="GPU tensors"):
        G.Grappa(accel=R).noise_maps(k, m)
    with pytest.raises(CineHipError, match="requires grad"):
        G.grappa_noise_maps(k.clone().requires_grad_(), m, R)
    with pytest.raises(CineHipError, match="requires grad"):
        G.grappa_gfactor_from_weights(wts.clone().requires_grad_(), R, kernel, h, w)
    with pytest.raises(ValueError):
        G.grappa_noise_maps(k, m, R, kernel=(3, 5))
