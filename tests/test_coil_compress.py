"""SVD coil compression of the data front-end (frontend.coil_gram / coil_matrix_from_gram / compress_coils, and the virtual_coils /
coil_matrix arguments of prepare_slice / prepare_example) against a float64 restatement in numpy, written out below.

Inputs have a designed spectrum so that the comparison is well-posed: complex white samples scaled per coil by
sigma_i^2 = 1e-4^(i / (c - 1)) and mixed by a seeded random unitary matrix.  Every test first asserts, in float64 on its own input,
that the eigenvalue gap at V is >= 1e-3 of lam[0] and every consecutive gap >= 1e-5 of lam[0] (a condition on the input, not on the
code under test).  Under it a 1e-12 perturbation of the Gram matrix moves the projector A^H A by <= 2e-10, rounding A to complex64
by <= 2.3e-8, and applying a complex64 matrix in fp32 differs from float64 by <= 1.8e-7 of the peak."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ the float64 restatement
def gram_ref(raw, n_frames, region):
    t, nx, ny, c = raw.shape
    T = min(n_frames, t)
    rx, ry = (nx, ny) if region == 0 else (min(region, nx), min(region, ny))
    x0, y0 = nx // 2 - rx // 2, ny // 2 - ry // 2
    s = raw[:T, x0:x0 + rx, y0:y0 + ry].reshape(-1, c).astype(np.complex128)
    return s.T @ s.conj()                                             # G[i, j] = sum raw_i conj(raw_j)


def matrix_ref(gram, v):
    lam, u = np.linalg.eigh(gram)
    lam, u = lam[::-1], u[:, ::-1]
    a = u[:, :v].conj().T.copy()
    for r in range(v):
        k = int(np.argmax(np.abs(a[r])))                              # the first of equal maxima
        a[r] *= np.conj(a[r, k]) / abs(a[r, k])
    return a, lam


def compress_ref(raw, a, n_frames):
    return raw[:min(n_frames, raw.shape[0])].astype(np.complex128) @ np.asarray(a, np.complex128).T


def designed_raw(t, nx, ny, c, seed):
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c)))
    sigma = np.sqrt(1e-4 ** (np.arange(c) / max(c - 1, 1)))
    w = (rs.standard_normal((t, nx, ny, c)) + 1j * rs.standard_normal((t, nx, ny, c))) * sigma
    return (w @ q.T).astype(np.complex64)


def assert_gaps(lam, v):
    """The condition on the input: the subspace split at V, and every eigenvector, is well separated."""
    c = len(lam)
    if v < c:
        assert (lam[v - 1] - lam[v]) / lam[0] >= 1e-3
    assert (-np.diff(lam)).min() / lam[0] >= 1e-5


def phase_rule_holds(a):
    a = np.asarray(a, np.complex128)
    for row in a:
        k = int(np.argmax(np.abs(row)))
        if not (row[k].real > 0 and abs(row[k].imag) <= 1e-7 * row[k].real):
            return False
    return True


# (t_in, nx, ny, c, V, region, n_frames)
CASES = [
    (3, 40, 36, 30, 15, 24, 3),        # the headline 30 -> 15
    (4, 33, 21, 34, 12, 0, 3),         # more than 32 coils, odd sizes, whole-matrix region, n_frames < t_in
    (2, 26, 50, 20, 8, 24, 2),         # region clipped on one axis
    (2, 24, 24, 64, 32, 24, 2),        # the largest V
    (3, 13, 7, 5, 5, 24, 3),           # V = c: a unitary change of basis
    (2, 48, 40, 38, 1, 16, 1),         # V = 1
    (2, 416, 208, 30, 15, 24, 2),      # a raw size the line engines refuse
]
IDS = ["x".join(map(str, c)) for c in CASES]


# The seed is part of the designed input: with 64 coils on 2 x 24 x 24 samples the nominal smallest gap (1.4e-5 of lam[0]) is close
# to the condition, and this draw meets it (assert_gaps checks every draw in float64 before anything runs on the device).
SEEDS = {(2, 24, 24, 64, 32, 24, 2): 9}


def _case(case):
    t_in, nx, ny, c, v, region, n_frames = case
    raw = designed_raw(t_in, nx, ny, c, seed=SEEDS.get(case, sum(case)))
    return raw, c, v, region, n_frames


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gram_vs_float64(dev, case):
    from cine_hip import frontend as FE
    raw, c, v, region, n_frames = _case(case)
    want = gram_ref(raw, n_frames, region)
    assert_gaps(matrix_ref(want, v)[1], v)
    x = torch.from_numpy(raw).to(dev)
    got = FE.coil_gram(x, n_frames, region)
    assert got.dtype == torch.complex128 and tuple(got.shape) == (c, c)
    g = got.cpu().numpy()
    err = np.abs(g - want).max() / np.abs(want).max()
    print(f"gram {case}: max|G - G_ref| / max|G_ref| = {err:.3e}")
    assert err <= 1e-9
    assert torch.equal(got, got.conj().transpose(0, 1).resolve_conj())          # Hermitian exactly
    assert (g.diagonal().imag == 0).all()
    assert torch.equal(FE.coil_gram(x, n_frames, region), got)                  # fixed order, no atomics: bit-identical


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matrix_vs_float64(dev, case):
    from cine_hip import frontend as FE
    raw, c, v, region, n_frames = _case(case)
    a_w, lam_w = matrix_ref(gram_ref(raw, n_frames, region), v)
    assert_gaps(lam_w, v)
    a, lam = FE.coil_compression_matrix(torch.from_numpy(raw).to(dev), v, n_frames, region)
    assert a.dtype == torch.complex64 and tuple(a.shape) == (v, c) and a.device.type == "cuda"
    assert lam.dtype == torch.float64 and tuple(lam.shape) == (c,)
    a, lam = a.cpu().numpy().astype(np.complex128), lam.cpu().numpy()
    e_lam = np.abs(lam - lam_w).max() / lam_w[0]
    e_proj = np.abs(a.conj().T @ a - a_w.conj().T @ a_w).max()
    align = min(abs(np.vdot(a_w[r], a[r])) for r in range(v))
    print(f"matrix {case}: lam {e_lam:.3e}, projector {e_proj:.3e}, worst row alignment 1 - {1 - align:.3e}")
    assert (np.diff(lam) <= 0).all() and e_lam <= 1e-9
    assert e_proj <= 1e-6
    assert align >= 1 - 1e-6
    assert phase_rule_holds(a)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_apply_vs_float64(dev, case):
    from cine_hip import frontend as FE
    raw, c, v, region, n_frames = _case(case)
    assert_gaps(matrix_ref(gram_ref(raw, n_frames, region), v)[1], v)
    x = torch.from_numpy(raw).to(dev)
    a, _ = FE.coil_compression_matrix(x, v, n_frames, region)
    got = FE.compress_coils(x, a, n_frames)
    T = min(n_frames, raw.shape[0])
    assert got.dtype == torch.complex64 and tuple(got.shape) == (T,) + raw.shape[1:3] + (v,)   # n_frames honoured
    want = compress_ref(raw, a.cpu().numpy(), n_frames)                          # the DEVICE's matrix, applied in float64
    err = rel_err(torch.view_as_real(got.cpu()), torch.view_as_real(torch.from_numpy(want)))
    print(f"apply {case}: rel_err = {err:.3e}")
    assert err < 1e-5
    assert torch.equal(FE.compress_coils(x, a, n_frames), got)                   # bit-identical
    every = FE.compress_coils(x, a)                                              # all frames; the first T are the same bits
    assert every.shape[0] == raw.shape[0] and torch.equal(every[:T], got)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kept_energy_is_the_leading_eigenvalue_share(dev, case):
    """With the whole matrix as the calibration region the compressed data hold exactly the share sum(lam[:V]) / sum(lam) of the energy
    of the kept frames; for V = c the change of basis is unitary and keeps all of it (to 1e-6)."""
    from cine_hip import frontend as FE
    raw, c, v, _, n_frames = _case(case)
    lam_w = matrix_ref(gram_ref(raw, n_frames, 0), v)[1]
    assert_gaps(lam_w, v)
    x = torch.from_numpy(raw).to(dev)
    a, _ = FE.coil_compression_matrix(x, v, n_frames, 0)
    out = FE.compress_coils(x, a, n_frames).cpu().numpy().astype(np.complex128)
    T = min(n_frames, raw.shape[0])
    got = (np.abs(out) ** 2).sum() / (np.abs(raw[:T].astype(np.complex128)) ** 2).sum()
    want = lam_w[:v].sum() / lam_w.sum()
    print(f"energy {case}: kept {got:.8f}, eigenvalue share {want:.8f}")
    assert abs(got - want) <= (1e-6 if v == c else 1e-5)


def _phantom_raw(t, nx, ny, c, seed, noise=1e-3):
    from cine_hip import synth
    img = synth.cine_phantom(t, nx, ny, seed=seed)[:, None] * synth.coil_maps(c, nx, ny)[None]
    k = synth._fft2c_np(img).transpose(0, 2, 3, 1)                               # (t, x, y, c)
    rs = np.random.RandomState(seed)
    k = k + noise * np.abs(k).max() * (rs.standard_normal(k.shape) + 1j * rs.standard_normal(k.shape))
    return np.ascontiguousarray(k.astype(np.complex64))


def test_phantom_kept_energy(dev):
    """Phantom x analytic coil maps, 30 -> 15, whole-matrix region.  The tail eigenvalues of such data are nearly degenerate (gap at V
    of 2e-7 of lam[0]), so this case checks the energy, which does not depend on the basis chosen inside the tail, not the projector.
    In float64 the kept fraction is 0.9989."""
    from cine_hip import frontend as FE
    raw = _phantom_raw(6, 64, 48, 30, seed=1)
    lam_w = matrix_ref(gram_ref(raw, 6, 0), 15)[1]
    x = torch.from_numpy(raw).to(dev)
    a, _ = FE.coil_compression_matrix(x, 15, None, 0)
    out = FE.compress_coils(x, a).cpu().numpy().astype(np.complex128)
    got = (np.abs(out) ** 2).sum() / (np.abs(raw.astype(np.complex128)) ** 2).sum()
    want = lam_w[:15].sum() / lam_w.sum()
    print(f"phantom: kept {got:.8f}, eigenvalue share {want:.8f}")
    assert abs(got - want) <= 1e-5
    assert 0.99 < want < 1.0


def _cplx(a):
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.complex64)))).contiguous()


@pytest.mark.parametrize("shape,crop,n_slices", [((3, 40, 36, 30), (21, 17), 3), ((2, 416, 208, 30), (200, 200), 2)],
                         ids=["line-engines", "416x208"])
def test_prepare_slice_with_virtual_coils(dev, shape, crop, n_slices):
    """prepare_slice(raw, virtual_coils=V) is prepare_slice of the compressed raw data, bit for bit, and matches the float64 front-end
    applied to the float64-compressed raw data (the device's matrix)."""
    from cine_hip import frontend as FE
    from oracle import frontend_ref as F
    v, fs = 15, (0.7, 0.0, 0.3, 0.3)
    raw = designed_raw(*shape, seed=sum(shape))
    assert_gaps(matrix_ref(gram_ref(raw, n_slices, 24), v)[1], v)
    x = torch.from_numpy(raw).to(dev)
    a, _ = FE.coil_compression_matrix(x, v, n_slices, 24)
    k, filt = FE.prepare_slice(x, crop, n_slices, fs, virtual_coils=v)
    assert tuple(k.shape) == (n_slices, v) + tuple(crop) + (2,)
    k2, filt2 = FE.prepare_slice(FE.compress_coils(x, a), crop, n_slices, fs)
    assert torch.equal(k, k2) and torch.equal(filt, filt2)
    k3, filt3 = FE.prepare_slice(x, crop, n_slices, fs, coil_matrix=a)
    assert torch.equal(k, k3) and torch.equal(filt, filt3)
    k4, _ = FE.prepare_slice(x, crop, n_slices, fs, virtual_coils=v, coil_matrix=a)
    assert torch.equal(k, k4)
    k_w, filt_w = F.prepare_slice(compress_ref(raw, a.cpu().numpy(), n_slices), crop, n_slices, fs)
    e_f, e_k = rel_err(filt.cpu(), _cplx(filt_w)), rel_err(k.cpu(), _cplx(k_w))
    print(f"prepare_slice {shape}: filtered crop {e_f:.3e}, k-space {e_k:.3e}")
    assert e_f < 1e-5 and e_k < 1e-5
    with pytest.raises(ValueError):
        FE.prepare_slice(x, crop, n_slices, fs, virtual_coils=v + 1, coil_matrix=a)
    with pytest.raises(ValueError):
        FE.prepare_slice(x, crop, n_slices, fs, virtual_coils=shape[3] + 1)
    with pytest.raises(ValueError):
        FE.prepare_slice(x, crop, n_slices, fs, virtual_coils=0)


def test_defaults_change_nothing(dev):
    """With the new arguments left out, and with virtual_coils equal to the coil count, prepare_slice is the composition of the public
    pieces it was before, bit for bit, on both of its branches."""
    from cine_hip import frontend as FE, ops
    rs = np.random.RandomState(11)
    fs, scaling = (0.7, 0.0, 0.3, 0.3), 1e6
    raw = torch.from_numpy((rs.standard_normal((5, 40, 36, 3)) + 1j * rs.standard_normal((5, 40, 36, 3))).astype(np.complex64)).to(dev)
    crop = (21, 17)
    images = ops.fft2c(torch.view_as_real((raw * scaling).permute(0, 3, 1, 2).contiguous()), inverse=True)
    want_filt = FE.gaussian_filter(FE.crop_select(images, 3, crop), fs)
    xr = torch.roll(want_filt, shifts=[-1, -1], dims=[-3, -2]).contiguous()              # both crop sides odd
    want_k = torch.roll(ops.fft2c(xr), shifts=[1, 1], dims=[-3, -2]).contiguous()
    for kw in ({}, {"virtual_coils": 3}, {"virtual_coils": None, "coil_matrix": None, "cc_region": 24}):
        k, filt = FE.prepare_slice(raw, crop, 3, fs, scaling, **kw)
        assert torch.equal(filt, want_filt) and torch.equal(k, want_k), kw
    raw = torch.from_numpy((rs.standard_normal((3, 416, 208, 4)) + 1j * rs.standard_normal((3, 416, 208, 4))).astype(np.complex64)).to(dev)
    crop = (200, 200)
    want_filt = FE.gaussian_filter(ops.raw_window_ifft2c(raw, 2, crop, scaling), fs)
    want_k = FE._to_kspace(want_filt)
    for kw in ({}, {"virtual_coils": 4}):
        k, filt = FE.prepare_slice(raw, crop, 2, fs, scaling, **kw)
        assert torch.equal(filt, want_filt) and torch.equal(k, want_k), kw


def test_prepare_example_beyond_32_coils(dev):
    from cine_hip import frontend as FE
    from cine_hip._lib import CineHipError
    raw = _phantom_raw(5, 48, 40, 34, seed=3)
    kw = dict(crop_shape=(40, 32), crop_target=(36, 28), n_slices=15, ecalib_r=24)
    with pytest.raises(CineHipError, match="at most 32 coils"):
        FE.prepare_example(raw, **kw)                                            # today's behaviour, kept
    k, mask, target, attrs, fname, _ = FE.prepare_example(raw, virtual_coils=12, fname="c34.h5", **kw)
    assert k.dtype == np.complex64 and k.shape == (5, 12, 40, 32) and np.isfinite(k).all()
    assert target.dtype == np.float32 and target.shape == (5, 36, 28) and np.isfinite(target).all() and target.max() > 0
    assert fname == "c34.h5"
    a, _ = FE.coil_compression_matrix(torch.from_numpy(raw).to(dev), 12, 15, 24)
    k2, *_ = FE.prepare_example(raw, coil_matrix=a, **kw)
    assert np.array_equal(k, k2)
    rs = np.random.RandomState(4)
    sens34 = (rs.standard_normal((34, 40, 32)) + 1j * rs.standard_normal((34, 40, 32))).astype(np.complex64)
    with pytest.raises(ValueError):
        FE.prepare_example(raw, sens=sens34, virtual_coils=12, **kw)
    k3, _, target3, *_ = FE.prepare_example(raw, sens=sens34[:12], virtual_coils=12, **kw)
    assert np.array_equal(k, k3) and np.isfinite(target3).all()


def test_one_pipeline_graph_set_for_mixed_coil_counts(dev):
    """Slices from 20-coil and 30-coil scans, compressed to 12 virtual coils, go alternately through ONE SlicePipeline without a
    rebuild between them (the same buffer-set object throughout) and give the bits of the sequential forward.  Uncompressed, the same
    two scans have different input shapes and do rebuild."""
    import reconstruction.models as M
    from cine_hip import frontend as FE, synth
    from cine_hip.pipeline import SlicePipeline
    net = M.VarNet(6, 8, 3, 16, 3, "XF")
    synth.fill_parameters_(net, 1, keep=("lambda",))
    net = net.to(dev).eval()
    crop, frames, fs = (32, 24), 5, (0.7, 0.0, 0.3, 0.3)

    def example(c, seed, **kw):
        raw = torch.from_numpy(_phantom_raw(6, 48, 40, c, seed=seed)).to(dev)
        k, _ = FE.prepare_slice(raw, crop, frames, fs, 1.0, **kw)                # (t, coils, X, Y, 2)
        np.random.seed(seed)
        mf = synth.create_mask_for_mask_type("random", [4], [4])
        masked, mask = synth.apply_mask(k.cpu(), mf, None)
        return masked.unsqueeze(0).contiguous(), mask.unsqueeze(0).byte().contiguous()

    exs = [example(c, seed, virtual_coils=12) for c, seed in ((20, 1), (30, 2), (20, 3), (30, 4), (20, 5))]
    assert all(tuple(mk.shape) == (1, frames, 12) + crop + (2,) for mk, _ in exs)
    with torch.no_grad():
        want = [net(mk.to(dev), mask.to(dev)).clone() for mk, mask in exs]
    with SlicePipeline(net, slots=2) as pipe:
        pipe.submit(exs[0][0].pin_memory(), exs[0][1], tag=0)
        first = pipe._set
        assert first is not None
        for j in range(1, len(exs)):
            pipe.submit(exs[j][0].pin_memory(), exs[j][1], tag=j)
            assert pipe._set is first, j                                         # no rebuild
        got = list(pipe.drain())
        assert pipe._set is first
    assert [t for t, _ in got] == list(range(len(exs)))
    for j, o in got:
        assert o.shape == want[j].shape and torch.equal(o.cpu(), want[j].cpu()), j

    plain = [example(20, 1), example(30, 2)]
    assert plain[0][0].shape[2] == 20 and plain[1][0].shape[2] == 30
    with SlicePipeline(net, slots=2) as pipe:
        pipe.submit(plain[0][0].pin_memory(), plain[0][1], tag=0)
        first = pipe._set
        pipe.submit(plain[1][0].pin_memory(), plain[1][1], tag=1)
        assert pipe._set is not first                                            # a new coil count is a new buffer set
        list(pipe.drain())
