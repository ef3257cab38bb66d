"""The analytic GRAPPA noise maps on the GPU: ``grappa_noise_maps`` and ``Grappa.noise_maps`` bit for bit against the composition of
``grappa_weights`` and ``grappa_gfactor_from_weights`` (with and without maps, two batch elements, captured and replayed), agreement
with the package's own noise model (``noise.pseudo_replica`` of the FIXED kernels, 200 replicas, both masks), and the exact case."""
import numpy as np
import pytest
import torch

import grappa_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def pairs(z):
    z = np.asarray(z)
    return torch.from_numpy(np.stack((z.real, z.imag), -1).astype(np.float32))


def random_chol(c, seed, dev):
    """L of a random positive-definite Psi with correlated coils of unequal noise levels (noise.noise_cholesky)."""
    from cine_hip import noise as N
    rs = np.random.RandomState(seed)
    M = rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c))
    psi = M @ M.conj().T / c + np.diag(0.5 + rs.uniform(size=c))
    return N.noise_cholesky(torch.from_numpy(psi)).to(dev)


def unit_maps(c, h, w, dev):
    from cine_hip import synth
    s = synth.coil_maps(c, h, w).astype(np.complex128)
    s = s / np.sqrt((np.abs(s) ** 2).sum(0, keepdims=True))
    return pairs(s)[None, None].to(dev)                                                  # (1, 1, c, h, w, 2)


# ================================================================== (1) the public entries are the composition, bit for bit
def batch_problem(dev):
    t, c, h, w, R = 6, 5, 30, 22, 3
    _, mask, mk = ref.phantom_slice(t, c, h, w, R)
    d_mk = torch.stack((pairs(mk), 1.5 * pairs(mk).flip(3))).to(dev)                     # two batch elements with kernels of their own
    d_mask = torch.from_numpy(mask.reshape(1, t, 1, h, 1, 1)).repeat(2, 1, 1, 1, 1, 1).to(dev)
    sens = unit_maps(c, h, w, dev)
    sens = torch.cat((sens, sens.flip(3))).contiguous()
    return (t, c, h, w, R), d_mk, d_mask, sens


@pytest.mark.parametrize("with_maps", [True, False], ids=["maps", "per-coil"])
def test_noise_maps_are_the_composition_bit_for_bit(dev, with_maps):
    from cine_hip import grappa as G
    from cine_hip.pipeline import pipeline_streams
    (t, c, h, w, R), d_mk, d_mask, sens = batch_problem(dev)
    kernel, lam, scale = (2, 5), 1e-3, 0.7
    chol = random_chol(c, 4, dev)
    sens = sens if with_maps else None
    want_g, want_std = [], []
    cal = G.calibration_data(d_mk, d_mask, "tgrappa", None, 16)
    for i in range(2):
        weights, info = G.grappa_weights(cal[i], R, kernel, lam)
        coef = None if sens is None else (sens[i] * sens.new_tensor([1.0, -1.0]))
        maps = G.grappa_gfactor_from_weights(weights, R, kernel, h, w, chol=chol, coef=coef, scale=scale)
        assert tuple(maps.g.shape) == ((1, h, w) if with_maps else (c, h, w)) and maps.g.dtype == torch.float32
        want_g.append(maps.g[0] if with_maps else maps.g)
        want_std.append(maps.std[0] if with_maps else maps.std)
    want_g, want_std = torch.stack(want_g), torch.stack(want_std)
    assert bool(torch.isfinite(want_g).all()) and float(want_g.min()) > 0 and not torch.equal(want_g[0], want_g[1])

    kw = dict(kernel=kernel, lam=lam, calib="tgrappa", calib_rows=16)
    maps, info = G.grappa_noise_maps(d_mk, d_mask, R, sens_maps=sens, chol=chol, scale=scale, **kw)
    assert tuple(maps.g.shape) == ((2, h, w) if with_maps else (2, c, h, w)) and tuple(info.shape) == (2, 4)
    assert torch.equal(maps.g, want_g) and torch.equal(maps.std, want_std) and float(info[:, 0].max()) <= G.RESIDUAL_MAX
    white = G.grappa_noise_maps(d_mk, d_mask, R, sens_maps=sens, **kw)[0]                # chol=None, scale=1: other maps
    assert not torch.equal(white.std, want_std) and bool(torch.isfinite(white.g).all())

    model = G.Grappa(accel=R, **kw).eval()
    eager = model.noise_maps(d_mk, d_mask, sens, chol=chol, scale=scale)
    assert torch.equal(eager.g, want_g) and torch.equal(eager.std, want_std) and tuple(model.last_info["info"].shape) == (2, 4)
    s = pipeline_streams(dev, 1)[0][0]                                                   # a stream of the pipelines' pool
    with torch.cuda.stream(s):
        model.noise_maps(d_mk, d_mask, sens, chol=chol, scale=scale)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        out = model.noise_maps(d_mk, d_mask, sens, chol=chol, scale=scale)
    for _ in range(2):
        out.g.fill_(float("nan"))
        out.std.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.g, want_g) and torch.equal(out.std, want_std)


# ================================================================== (2) agreement with the package's own noise model
@pytest.mark.parametrize("R,kernel", [(3, (2, 3)), (2, (4, 3))], ids=["R3-k2x3", "R2-k4x3"])
def test_analytic_maps_against_pseudo_replicas_of_the_fixed_kernels(dev, R, kernel):
    """The medians over the pixels with analytic g >= 0.5 of measured / analytic, for g and for std, must lie in [0.90, 1.10] in every
    frame: a wrong convention (sqrt(R), sqrt(2), R, a missing scale) misses by a factor of 1.41 at least, while 200 replicas scatter a
    pixel's ratio by 1 / sqrt(2 * 200) = 5 % and its median over a hundred pixels far less.  The float64 reference alone sits at
    0.956 .. 0.983: the zero boundary of the k-space application removes a little noise at matrices this small."""
    from cine_hip import grappa as G, noise as N, ops
    t, c, h, w = 4, 4, 24, 16
    scale, replicas = 0.6, 200
    full, mask, mk = ref.phantom_slice(t, c, h, w, R)
    d_full, d_mk = pairs(full)[None].to(dev), pairs(mk)[None].to(dev)
    d_mask = torch.from_numpy(mask.reshape(1, t, 1, h, 1, 1)).to(dev)
    d_ones = torch.ones_like(d_mask)
    sens = unit_maps(c, h, w, dev)
    chol = random_chol(c, 11 + R, dev)
    weights, info = G.grappa_weights(G.calibration_data(d_mk, d_mask, "tgrappa", None, h)[0], R, kernel, 1e-2)
    assert float(info[0]) <= G.RESIDUAL_MAX

    def model(k, m, s, output="complex"):
        """The FIXED kernels: a replica must not refit them, the closed form knows nothing of calibration noise."""
        offsets, _ = G.lattice_offsets(m, R)
        filled = G.grappa_apply(k[0], weights, m.view(t, h), offsets[0], R, kernel)[None]
        return ops.sens_reduce(filled, s).squeeze(2)

    accel = N.pseudo_replica(model, d_mk, d_mask, sens, chol=chol, scale=scale, replicas=replicas, seed=5, output="complex")
    whole = N.pseudo_replica(model, d_full, d_ones, sens, chol=chol, scale=scale, replicas=replicas, seed=6, output="complex")
    assert tuple(accel.std.shape) == (1, t, h, w)
    g_meas = N.g_factor(accel.std, whole.std, d_mask)
    coef = sens[0] * sens.new_tensor([1.0, -1.0])                                        # p = conj(S), (1, c, h, w, 2)
    maps = G.grappa_gfactor_from_weights(weights, R, kernel, h, w, chol=chol, coef=coef, scale=scale)
    sel = maps.g[0] >= 0.5
    share = float(sel.float().mean())
    assert share >= 0.25, f"only {share:.0%} of the pixels have an analytic g >= 0.5"
    for f in range(t):
        m_g = float((g_meas[0, f][sel] / maps.g[0][sel]).median())
        m_s = float((accel.std[0, f][sel] / maps.std[0][sel]).median())
        print(f"R {R} kernel {kernel} frame {f}: median measured / analytic g {m_g:.4f}, std {m_s:.4f} over {share:.0%} of the pixels; analytic g "
              f"in [{float(maps.g.min()):.3f}, {float(maps.g.max()):.3f}]")
        assert 0.90 <= m_g <= 1.10 and 0.90 <= m_s <= 1.10, (f, m_g, m_s)


# ================================================================== (3) the exact case
@pytest.mark.parametrize("R", [2, 3, 4, 8])
def test_zero_weights_give_one_over_r_exactly(dev, R):
    """Psi = I, one coil, all-zero weights (zero filling): amp = 1 and g = 1 / R, to the bit, per coil and for the coefficient 1."""
    from cine_hip import grappa as G
    from kernel_sweep import L, stream
    h, w, ky, kx = 9, 70, 2, 3
    weights = torch.zeros(R - 1, ky * kx, 1, 2, device=dev)
    one = torch.zeros(1, 1, h, w, 2, device=dev)
    one[..., 0] = 1
    for coef in (None, one):
        maps = G.grappa_gfactor_from_weights(weights, R, (ky, kx), h, w, coef=coef)
        assert torch.equal(maps.g, torch.full((1, h, w), 1.0 / R, device=dev, dtype=torch.float32))
        assert torch.equal(maps.std, torch.full((1, h, w), 1.0 / float(np.sqrt(R)), device=dev, dtype=torch.float32))
        amp = torch.full((1, h, w), float("nan"), device=dev)
        assert L().cine_grappa_gfactor(weights.data_ptr(), None, None if coef is None else coef.data_ptr(), None, amp.data_ptr(), 1, 1, h, w, R,
                                       ky, kx, stream()) == 0, L().cine_last_error()
        assert torch.equal(amp, torch.ones(1, h, w, device=dev))
    wimg = G.grappa_image_weights(weights, R, (ky, kx), h, w)
    assert tuple(wimg.shape) == (1, 1, h, w, 2) and torch.equal(wimg, one[0, 0][None, None])
