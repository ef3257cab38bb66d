"""ESPIRiT calibration without an eigensolver: the projector of the calibration as a matrix sign function on the float64 matrix
cores (cine_espirit_gram, cine_zgemm_f64, cine_espirit_projector), ``frontend.espirit_maps(method="sign")`` and
``SlicePipeline.submit(..., sens_maps="espirit")``.

The fixtures are time-averaged phantom k-spaces ``(t, c, n, r, seed, noise)``; each test asserts on the host that every eigenvalue of
the float64 Gram matrix keeps a relative distance >= 1e-3 from the threshold thresh^2 lam_max (fixture 2 sits 0.5 % from it).

The oracle (oracle/frontend_ref.espirit_maps) builds a (ny, nx, c, kept) complex128 array: gigabytes and minutes at 15 coils x 200 x
200.  For those three fixtures its formula is evaluated in float64 on the device (``_oracle_dev``, the oracle's lines in torch, from
the oracle's own kept singular vectors); ``test_device_oracle_restates_the_oracle`` pins that restatement to the oracle itself on a
small fixture.  The bars are the same for every fixture.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURES = [(5, 6, 64, 24, 1, 0.0), (5, 3, 48, 16, 1, 0.0), (5, 6, 64, 24, 1, 1e-3), (5, 8, 64, 24, 3, 1e-2), (5, 4, 40, 15, 7, 1e-3),
            (15, 15, 200, 24, 2, 0.0), (15, 15, 200, 24, 2, 1e-3), (15, 15, 200, 15, 2, 1e-3)]
NEAR = 2                                   # the fixture whose eigenvalue sits 0.5 % from the threshold
K, THRESH = 6, 1e-3
U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _phantom(t, c, n, seed):
    from cine_hip import synth
    ex = synth.make_cine_slice(t, c, n, n, accel=4, center_lines=10, seed=seed)
    k = torch.view_as_complex(ex["kspace"][0].contiguous()).numpy()                  # (t, c, n, n)
    tgt = ex["target"][0].numpy().mean(0)
    return k, tgt > 0.1 * tgt.max()


@functools.lru_cache(maxsize=None)
def _fixture(i):
    """(kavg complex64 (c, n, n), object support, r)."""
    t, c, n, r, seed, noise = FIXTURES[i]
    k, sup = _phantom(t, c, n, seed)
    if noise:
        rs = np.random.RandomState(seed + 100)
        re = rs.standard_normal(k.shape)
        im = rs.standard_normal(k.shape)
        k = k + noise * np.abs(k).max() * (re + 1j * im)
    return k.mean(0).astype(np.complex64), sup, r


def _acs(kavg, r):
    c, ny, nx = kavg.shape
    ry, rx = min(r, ny), min(r, nx)
    y0, x0 = ny // 2 - ry // 2, nx // 2 - rx // 2
    return np.asarray(kavg[:, y0:y0 + ry, x0:x0 + rx], np.complex128)


def _host_gram(kavg, r):
    from oracle.frontend_ref import calibration_matrix
    a = calibration_matrix(_acs(kavg, r), K)
    return a.conj().T @ a


@functools.lru_cache(maxsize=None)
def _host_eig(i):
    """(G float64 Gram, eigenvalues ascending, P_eigh) of fixture i; asserts the fixture's condition."""
    kavg, _, r = _fixture(i)
    g = _host_gram(kavg, r)
    ev, vec = np.linalg.eigh(g)
    mu = THRESH * THRESH * ev[-1]
    dist = float(np.abs(ev - mu).min() / mu)
    assert dist >= 1e-3, (i, dist)
    v = vec[:, ev >= mu]
    return g, ev, v @ v.conj().T, dist


def _cplx(a):
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.complex64)))).contiguous()


def _z(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).to(dev)


# ------------------------------------------------------------------ 1. the complex128 GEMM
def _zgemm(a, b, d, alpha, beta, dev):
    """cine_zgemm_f64 into an output between guards, prefilled with NaN; returns (C, guards intact)."""
    from cine_hip import ops
    from cine_hip._lib import check, lib
    n = a.shape[0]
    guard, gv = 16, 1234.5
    buf = torch.full((2 * guard + 2 * n * n,), gv, device=dev, dtype=torch.float64)
    out = buf[guard:guard + 2 * n * n]
    out.fill_(float("nan"))
    A, B, D = _z(a, dev), _z(b, dev), _z(d, dev)
    check(lib().cine_zgemm_f64(A.data_ptr(), B.data_ptr(), D.data_ptr(), out.data_ptr(), n, alpha.real, alpha.imag, beta.real, beta.imag,
                               ops._stream()), "cine_zgemm_f64")
    torch.cuda.synchronize()
    ok = bool((buf[:guard] == gv).all()) and bool((buf[guard + 2 * n * n:] == gv).all())
    c = out.cpu().numpy().reshape(n, n, 2)
    return c[..., 0] + 1j * c[..., 1], ok


@pytest.mark.parametrize("n", [36, 108, 144, 180, 252, 540, 1152])
def test_zgemm_vs_numpy(dev, n):
    rs = np.random.RandomState(n)
    gen = lambda: rs.standard_normal((n, n)) + 1j * rs.standard_normal((n, n))
    h = gen()
    herm = h + h.conj().T
    d = gen()
    for name, (a, b) in {"hermitian": (herm, herm), "general": (gen(), gen())}.items():
        for alpha, beta in ((1 + 0j, 1 + 0j), (-0.5 + 1.5j, 1 + 0j), (1 + 0j, -0.5 + 1.5j), (-0.5 + 1.5j, -0.5 + 1.5j)):
            got, guards = _zgemm(a, b, d, alpha, beta, dev)
            want = alpha * (a @ b) + beta * d
            bar = 4 * n * U * (np.abs(a) @ np.abs(b) + abs(beta) * np.abs(d))
            err = np.abs(got - want)
            assert guards, (name, alpha, beta)
            assert not np.isnan(got).any(), (name, alpha, beta, "an output tile was skipped")
            worst = float((err / bar).max())
            print(f"zgemm n={n} {name} alpha={alpha} beta={beta}: worst err / bar = {worst:.3f}")
            assert worst <= 1.0, (name, alpha, beta, worst)


def test_zgemm_beta_zero_does_not_read_d(dev):
    n = 52
    rs = np.random.RandomState(5)
    a = rs.standard_normal((n, n)) + 1j * rs.standard_normal((n, n))
    b = rs.standard_normal((n, n)) + 1j * rs.standard_normal((n, n))
    got, guards = _zgemm(a, b, np.full((n, n), np.nan + 0j), 1 + 0j, 0j, dev)
    assert guards and np.abs(got - a @ b).max() <= 4 * n * U * (np.abs(a) @ np.abs(b)).max()


# ------------------------------------------------------------------ 2. the Gram matrix
def _dev_gram(kavg, r, dev):
    from cine_hip import frontend as FE
    g = FE.espirit_gram(_cplx(kavg).to(dev), r, K)
    return g


@pytest.mark.parametrize("i", range(len(FIXTURES)))
def test_gram_vs_float64(dev, i):
    kavg, _, r = _fixture(i)
    want = _host_eig(i)[0]
    g1 = _dev_gram(kavg, r, dev)
    g2 = _dev_gram(kavg, r, dev)
    got = g1.cpu().numpy()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"gram fixture {i}: max|d| / max|G| = {err:.3e}")
    assert err <= 1e-12
    assert np.array_equal(got, got.conj().T)                                # exactly Hermitian
    assert torch.equal(torch.view_as_real(g1), torch.view_as_real(g2))      # the same bits


@pytest.mark.parametrize("c,ny,nx,r", [(3, 41, 50, 15), (2, 14, 17, 200), (5, 33, 20, 24)])
def test_gram_odd_and_clipped(dev, c, ny, nx, r):
    """ny != nx, odd sizes, r larger than the image (the block is clipped to the image)."""
    rs = np.random.RandomState(ny)
    kavg = (rs.standard_normal((c, ny, nx)) + 1j * rs.standard_normal((c, ny, nx))).astype(np.complex64)
    want = _host_gram(kavg, r)
    g1, g2 = _dev_gram(kavg, r, dev), _dev_gram(kavg, r, dev)
    got = g1.cpu().numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(got, got.conj().T) and torch.equal(torch.view_as_real(g1), torch.view_as_real(g2))


# ------------------------------------------------------------------ 3. the projector
def _projector(g, dev, iters=60):
    from cine_hip import frontend as FE
    p, lam, resid = FE.espirit_projector(_z(g, dev), THRESH, iters)
    torch.cuda.synchronize()
    p = p.cpu().numpy()
    return p[..., 0] + 1j * p[..., 1], float(lam.cpu()[0]), float(resid.cpu()[0])


@pytest.mark.parametrize("i", range(len(FIXTURES)))
def test_projector_vs_eigh(dev, i):
    g, ev, p_eigh, dist = _host_eig(i)
    p, lam, resid = _projector(g, dev)
    # the entry point hands P out rounded once to complex64: here the float64 projector goes through the same rounding (the 1e-8 bar on
    # the float64 iterate itself: test_sign_matrix_vs_eigh_float64)
    err32 = float(np.abs(p - p_eigh.astype(np.complex64)).max())
    lam_err = abs(lam / ev[-1] - 1.0)
    print(f"projector fixture {i}: distance {dist:.2e}, |P - P_eigh| after float32 rounding = {err32:.3e}, lam err = {lam_err:.2e}, resid = {resid:.2e}")
    assert lam_err <= 1e-12
    assert resid <= 1e-12
    assert err32 <= 1e-8 + 2.0 ** -24                                        # 1e-8 plus half a float32 spacing below 1 (both sides rounded once)


@pytest.mark.parametrize("i", range(len(FIXTURES)))
def test_sign_matrix_vs_eigh_float64(dev, i):
    """The bar max|P - P_eigh| <= 1e-8 on the float64 iterate itself: the same launch sequence as cine_espirit_projector, driven
    through cine_zgemm_f64 from here, so that X is seen before its rounding to complex64."""
    from cine_hip import ops
    from cine_hip._lib import check, lib
    g, ev, p_eigh, _ = _host_eig(i)
    n = g.shape[0]
    _, lam, _ = _projector(g, dev)                                           # lam^ of the entry point
    inv = 1.0 / (1.0001 * lam)                                               # sign_start_kernel's arithmetic
    x0 = g * inv
    x0[np.arange(n), np.arange(n)] = (g.real.diagonal() - THRESH * THRESH * lam) * inv + 1j * (g.imag.diagonal() * inv)
    x, y, xn = _z(x0, dev), torch.empty((n, n), dtype=torch.complex128, device=dev), torch.empty((n, n), dtype=torch.complex128, device=dev)
    L, st = lib(), ops._stream()
    for _ in range(60):
        check(L.cine_zgemm_f64(x.data_ptr(), x.data_ptr(), None, y.data_ptr(), n, 1.0, 0.0, 0.0, 0.0, st))
        check(L.cine_zgemm_f64(x.data_ptr(), y.data_ptr(), x.data_ptr(), xn.data_ptr(), n, -0.5, 0.0, 1.5, 0.0, st))
        x, xn = xn, x
    p64 = 0.5 * (np.eye(n) + x.cpu().numpy())
    err = float(np.abs(p64 - p_eigh).max())
    p32, _, _ = _projector(g, dev)
    print(f"sign matrix fixture {i}: max|P - P_eigh| = {err:.3e}")
    assert err <= 1e-8
    assert np.array_equal(p32, p64.astype(np.complex64))                     # the entry point hands out exactly this iterate, rounded once


def test_residual_flag_is_live(dev):
    g = _host_eig(NEAR)[0]
    _, _, resid = _projector(g, dev, iters=30)
    print(f"residual after 30 steps on the 0.5 % fixture: {resid:.3e}")
    assert resid > 1e-6


def test_projector_repeats_bit_identically(dev):
    from cine_hip import frontend as FE
    g = _z(_host_eig(4)[0], dev)
    a, b = FE.espirit_projector(g), FE.espirit_projector(g)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 4. method="sign" against method="eigh" and the oracle
def _oracle_dev(kavg, r, dev):
    """oracle/frontend_ref.espirit_maps(with_second=True) line by line in float64 on the device, from the oracle's own kept vectors."""
    from oracle.frontend_ref import calibration_matrix
    c, ny, nx = kavg.shape
    a = calibration_matrix(_acs(kavg, r), K)
    _, s, vh = np.linalg.svd(a, full_matrices=False)
    vpar = vh[s >= THRESH * s[0]].conj().T
    n = vpar.shape[1]
    kern = torch.from_numpy(vpar.reshape(K, K, c, n)).to(dev)
    ry = (np.arange(ny) - ny // 2) / ny
    rx = (np.arange(nx) - nx // 2) / nx
    ey = torch.from_numpy(np.exp(-2j * np.pi * np.outer(np.arange(K), ry))).to(dev)
    ex = torch.from_numpy(np.exp(-2j * np.pi * np.outer(np.arange(K), rx))).to(dev)
    lam, lam2, vecs = [], [], []
    for y0 in range(0, ny, 25):                                             # rows in chunks: (25, nx, c, n) complex128 at a time
        g = torch.einsum("pqcn,py,qx->yxcn", kern, ey[:, y0:y0 + 25], ex)
        m = torch.einsum("yxcn,yxdn->yxcd", g.conj(), g) / (K * K)
        w, v = np.linalg.eigh(m.cpu().numpy())                               # the small per-pixel problems: numpy, as in the oracle
        vec = v[..., -1]
        vec = vec * np.exp(-1j * np.angle(vec[..., :1]))
        vec = vec * (w[..., -1:] >= 0.8)
        lam.append(w[..., -1]); lam2.append(w[..., -2]); vecs.append(vec)
    vec = np.concatenate(vecs).transpose(2, 0, 1).astype(np.complex64)
    return vec, np.concatenate(lam).astype(np.float32), np.concatenate(lam2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(i):
    from oracle import frontend_ref as F
    kavg, _, r = _fixture(i)
    if kavg.shape[0] * kavg.shape[1] * kavg.shape[2] > 100000:
        return _oracle_dev(kavg, r, torch.device("cuda:0"))
    return F.espirit_maps(kavg, r=r, with_second=True)


def test_device_oracle_restates_the_oracle(dev):
    from oracle import frontend_ref as F
    kavg, sup, r = _fixture(4)
    want, lam_w, lam2_w = F.espirit_maps(kavg, r=r, with_second=True)
    got, lam_g, lam2_g = _oracle_dev(kavg, r, dev)
    inside = sup & (lam_w >= 0.9) & (lam2_w < 0.9 * lam_w)                   # elsewhere the eigenvector of a near-degenerate pair is not pinned
    assert np.abs(lam_g - lam_w).max() < 1e-6 and np.abs(lam2_g - lam2_w).max() < 1e-6
    assert np.abs(got - want)[:, inside].max() < 1e-5


@pytest.mark.parametrize("i", range(len(FIXTURES)))
def test_sign_vs_eigh_and_oracle(dev, i):
    from cine_hip import frontend as FE
    kavg, sup, r = _fixture(i)
    _host_eig(i)                                                            # the fixture's condition
    want, lam_w, lam2 = _oracle(i)
    kd = _cplx(kavg).to(dev)
    maps_s, lam_s, resid = FE.espirit_maps(kd, r=r, method="sign", return_residual=True)
    maps_e, lam_e = FE.espirit_maps(kd, r=r, method="eigh")
    assert float(resid.cpu()[0]) <= 1e-12
    inside = sup & (lam_w >= 0.9) & (lam2 < 0.9 * lam_w)
    if i != 3:                                                              # fixture 3 keeps every vector: P = I, M(r) = I, no separated eigenvalue
        assert inside.sum() >= 200
    mx = lambda v: float(v.max()) if v.size else 0.0
    ms, me = torch.view_as_complex(maps_s.cpu()).numpy(), torch.view_as_complex(maps_e.cpu()).numpy()
    ls, le = lam_s.cpu().numpy(), lam_e.cpu().numpy()
    d_lam, d_maps = float(np.abs(ls - le).max()), mx(np.abs(ms - me)[:, inside])
    o_lam, o_max = mx(np.abs(ls - lam_w)[inside]), mx(np.abs(ms - want)[:, inside])
    o_rms = float(np.sqrt((np.abs(ms - want)[:, inside] ** 2).mean())) if inside.any() else 0.0
    print(f"fixture {i}: {int(inside.sum())} pixels; sign vs eigh: lam {d_lam:.2e}, maps {d_maps:.2e}; vs oracle: lam {o_lam:.2e}, "
          f"maps max {o_max:.2e} rms {o_rms:.2e}")
    assert d_lam <= 1e-5
    assert d_maps <= 1e-4
    assert o_lam < 1e-3 and o_max < 5e-3 and o_rms < 5e-4


# ------------------------------------------------------------------ 5. graph capture
def test_sign_method_is_capturable(dev):
    from cine_hip import frontend as FE
    (k0, _, r), (k1, _, r1) = _fixture(0), _fixture(2)
    assert k0.shape == k1.shape and r == r1
    a, b = _cplx(k0).to(dev), _cplx(k1).to(dev)
    static = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        FE.espirit_maps(static, r=r, method="sign", return_residual=True)   # per-stream caches are filled outside capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = FE.espirit_maps(static, r=r, method="sign", return_residual=True)
    static.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    want = FE.espirit_maps(b, r=r, method="sign", return_residual=True)
    assert all(torch.equal(x, y) for x, y in zip(out, want))
    assert not torch.equal(out[0], FE.espirit_maps(a, r=r, method="sign")[0])


# ------------------------------------------------------------------ 6. the pipeline
T, C, N, ECALIB_R = 5, 6, 64, 12
RAW_SHAPE, CROP, FS = (T, 72, 68, C), (N, N), (0.7, 0.0, 0.3, 0.3)


def _raw(seed):
    rs = np.random.RandomState(seed)
    t, nx, ny, c = RAW_SHAPE
    x, y = np.arange(nx)[:, None] - nx // 2, np.arange(ny)[None, :] - ny // 2
    w = np.exp(-(x * x / (2.0 * (nx / 8.0) ** 2) + y * y / (2.0 * (ny / 8.0) ** 2))) + 0.02
    z = rs.standard_normal((t, nx, ny, c)) + 1j * rs.standard_normal((t, nx, ny, c))
    return torch.from_numpy((1e-6 * z * w[None, :, :, None]).astype(np.complex64))


def _row_mask(seed):
    rs = np.random.RandomState(1000 + seed)
    m = (rs.uniform(size=(1, T, 1, N, 1, 1)) < 0.3).astype(np.uint8)
    m[:, :, :, N // 2 - 5:N // 2 + 5] = 1
    return torch.from_numpy(m)


def _general_mask(seed):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(1, T, 1, N, N, 1, generator=g) < 0.4).to(torch.uint8)
    m[:, :, :, N // 2 - 8:N // 2 + 8, N // 2 - 8:N // 2 + 8] = 1
    return m


def _matrix(v, c, seed):
    rs = np.random.RandomState(2000 + seed)
    q, _ = np.linalg.qr(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c)))
    return torch.from_numpy(q[:v].astype(np.complex64))


def _net(kind, dev):
    import reconstruction.models as M
    from cine_hip import synth
    # VarNet "2D": its NormUnet normalises whole frames.  The x-f planes of "XF" that lie outside the object are all zero under ESPIRiT's
    # cropped maps (eigenvalue < 0.8 -> 0), and a zero plane has no standard deviation to normalise by, here as in the reference.
    net = M.CineNet(2, 3, 4, 2, "XF") if kind == "cinenet" else M.VarNet(2, 4, 2, 4, 2, "2D")
    synth.fill_parameters_(net, 7, keep=("lambda",))
    return net.to(dev).eval()


def _eager(net, mk, mask, r=ECALIB_R):
    """The identity the pipeline states: model(mk, mask, espirit_maps(time_average(mk[i]), r, method="sign")[0][None, None])."""
    from cine_hip import frontend as FE, ops
    with torch.no_grad(), ops.branches(1):
        maps = torch.stack([FE.espirit_maps(FE.time_average(mk[i]), r=r, method="sign")[0] for i in range(mk.shape[0])])[:, None]
        return net(mk, mask, maps).clone()


def _slices(dev, n=5):
    from cine_hip import synth
    exs = [synth.make_cine_slice(T, C, N, N, accel=4, center_lines=10, seed=10 + j) for j in range(n)]
    return [(ex["masked_kspace"].to(dev), ex["mask"].to(torch.uint8).to(dev)) for ex in exs]


@pytest.mark.parametrize("graphs", [True, False])
def test_pipeline_cinenet_submit(dev, graphs):
    from cine_hip.pipeline import SlicePipeline
    net = _net("cinenet", dev)
    ins = _slices(dev)
    want = [_eager(net, mk, mask) for mk, mask in ins]
    assert not torch.equal(want[0], want[1]) and all(torch.isfinite(w).all() for w in want)
    with SlicePipeline(net, slots=2, graphs=graphs) as pipe:
        for j, (mk, mask) in enumerate(ins):
            pipe.submit(mk, mask, "espirit", tag=j, ecalib_r=ECALIB_R)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    assert sorted(got) == list(range(len(ins)))
    for j in range(len(ins)):
        assert torch.equal(got[j], want[j]), j


@pytest.mark.parametrize("with_matrix", [False, True])
def test_pipeline_cinenet_submit_raw(dev, with_matrix):
    from cine_hip import frontend as FE
    from cine_hip.pipeline import SlicePipeline
    net = _net("cinenet", dev)
    a = _matrix(4, C, 3).to(dev) if with_matrix else None
    raws = [_raw(50 + j).to(dev) for j in range(5)]
    masks = [_row_mask(j).to(dev) for j in range(5)]
    want = []
    for raw, mask in zip(raws, masks):
        with torch.no_grad():
            mk = FE.prepare_masked_slice(raw, mask, CROP, T, FS, 1e6, coil_matrix=a)
        want.append(_eager(net, mk, mask))
    assert not torch.equal(want[0], want[1]) and all(torch.isfinite(w).all() for w in want)
    with SlicePipeline(net, slots=2) as pipe:
        for j in range(5):
            pipe.submit_raw(raws[j], masks[j], "espirit", tag=j, crop_shape=CROP, n_frames=T, coil_matrix=a, ecalib_r=ECALIB_R)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    for j in range(5):
        assert torch.equal(got[j], want[j]), j


def test_pipeline_varnet_w_varying_mask(dev):
    from cine_hip import frontend as FE
    from cine_hip.pipeline import SlicePipeline
    net = _net("varnet", dev)
    from cine_hip import synth
    masks = [_general_mask(20 + j).to(dev) for j in range(3)]
    full = [synth.make_cine_slice(T, C, N, N, accel=4, center_lines=10, seed=30 + j)["kspace"].to(dev) for j in range(3)]
    mks = [(k * m).contiguous() for k, m in zip(full, masks)]                # fully sampled k-space under the w-varying mask
    raws = [_raw(70 + j).to(dev) for j in range(3)]
    want = [_eager(net, mk, m) for mk, m in zip(mks, masks)]
    want_raw = []
    for raw, m in zip(raws, masks):
        with torch.no_grad():
            want_raw.append(_eager(net, FE.prepare_masked_slice(raw, m, CROP, T, FS, 1e6), m))
    with SlicePipeline(net, slots=2) as pipe:
        for j in range(3):
            pipe.submit(mks[j], masks[j], "espirit", tag=("k", j), ecalib_r=ECALIB_R)
        for j in range(3):
            pipe.submit_raw(raws[j], masks[j], "espirit", tag=("raw", j), crop_shape=CROP, n_frames=T, ecalib_r=ECALIB_R)
        got = dict(pipe.drain())
    for j in range(3):
        assert torch.isfinite(want[j]).all() and torch.isfinite(want_raw[j]).all(), j
        assert torch.equal(got[("k", j)], want[j]), j
        assert torch.equal(got[("raw", j)], want_raw[j]), j
    assert not torch.equal(want[0], want[1])


def test_pipeline_reports_an_unconverged_calibration(dev):
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    net = _net("cinenet", dev)
    (mk, mask), = _slices(dev, 1)
    with SlicePipeline(net, slots=1) as pipe:
        pipe.submit(mk, mask, "espirit", tag="slice-7", ecalib_r=ECALIB_R, sign_iters=3)
        with pytest.raises(CineHipError, match="slice-7.*sign_iters"):
            list(pipe.drain())
        pipe.submit(mk, mask, "espirit", tag="ok", ecalib_r=ECALIB_R)          # a new key: a new set; the pipeline is usable afterwards
        (tag, out), = list(pipe.drain())
    assert tag == "ok" and torch.equal(out, _eager(net, mk, mask))
