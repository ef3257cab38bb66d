"""cine_hip.noise end to end: pseudo_replica as a loop and through a SlicePipeline (``submit(..., noise=)``) give the same bits, graphs on
and off, and a pipeline that serves plain submissions in between returns for those what it always returned; the std map of a linear
reconstruction (ops.sens_reduce as a module) against the float64 restatement fed the reference's own noise, at kernel_sweep.BAR_CAP;
``add_noise(..., replica_dev=counter)`` captured in a graph with the counter bumped inside draws replicas 0, 1, 2 on three replays."""
import numpy as np
import pytest
import torch

import noise_reference as R
from kernel_sweep import BAR_CAP, same_bits

pytestmark = pytest.mark.gpu
SEED, SCALE = 7, 0.05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


_CACHE = {}


def slice_inputs(dev):
    """(1, 4, 4, 16, 12): the synthetic slice, a random L, and the sequential results every pipeline case is compared with."""
    if "in" not in _CACHE:
        from cine_hip import noise as N, synth
        from cine_hip.classical import KtSparseSense
        ex = synth.make_cine_slice(4, 4, 16, 12, accel=2, center_lines=4, seed=1)
        mk, mask, sens = (ex[k].to(dev) for k in ("masked_kspace", "mask", "sens_maps"))
        low = torch.from_numpy(R.random_chol(np.random.RandomState(5), 4)[0]).to(dev)
        model = KtSparseSense(iters=3).eval()
        scale = SCALE * float(mk.abs().max())
        plain = model(mk, mask, sens)
        noisy = [model(N.add_noise(mk, mask, low, scale=scale, seed=SEED, replica=r), mask, sens) for r in range(16)]
        maps = N.pseudo_replica(model, mk, mask, sens, chol=low, scale=scale, replicas=16, seed=SEED)
        torch.cuda.synchronize()
        _CACHE["in"] = (model, mk, mask, sens, low, scale, plain, noisy, maps)
    return _CACHE["in"]


def same_maps(a, b):
    return a.replicas == b.replicas and a.g is None and b.g is None and all(same_bits(x, y) for x, y in zip(a[:3], b[:3]))


def test_sequential_maps_are_the_statistics_of_the_sequential_replicas(dev):
    model, mk, mask, sens, low, scale, plain, noisy, maps = slice_inputs(dev)
    acc = R.Welford()
    for o in noisy:
        acc.add(o.cpu().numpy())
    mean, std, snr, _ = acc.finish()
    assert maps.replicas == 16 and maps.g is None and tuple(maps.std.shape) == tuple(plain.shape)
    for got, want in ((maps.mean, mean), (maps.std, std), (maps.snr, snr)):
        assert float(np.abs(got.cpu().numpy() - want).max()) <= 1e-5 * float(np.abs(want).max())
    assert float(maps.std.min()) > 0 and not same_bits(noisy[0], noisy[1]) and not same_bits(noisy[0], plain)


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
def test_in_flight_equals_sequential(dev, graphs):
    from cine_hip import noise as N
    from cine_hip.pipeline import SlicePipeline
    model, mk, mask, sens, low, scale, plain, noisy, maps = slice_inputs(dev)
    with SlicePipeline(model, slots=2, graphs=graphs) as pipe:
        # replicas and plain submissions interleaved: each gets the bits of the same call run alone
        for r in range(5):
            pipe.submit(mk, mask, sens, tag=("noise", r), noise=N.NoiseSpec(low, scale, SEED, r))
            pipe.submit(mk, mask, sens, tag=("plain", r))
        got = dict(pipe.drain())
        assert pipe.set_builds == 1                                           # the spec is not part of the set key
        for r in range(5):
            assert same_bits(got[("plain", r)], plain), f"plain submission {r}"
            assert same_bits(got[("noise", r)], noisy[r]), f"replica {r}"
        assert same_maps(N.pseudo_replica(model, mk, mask, sens, chol=low, scale=scale, replicas=16, seed=SEED, pipeline=pipe), maps)
        assert pipe.pending() == 0 and pipe.set_builds == 1
        pipe.submit(mk, mask, sens)
        assert same_bits(list(pipe.drain())[0][1], plain)                      # and the caller's k-space was never written


def test_pipeline_refuses_a_bad_spec(dev):
    from cine_hip import noise as N
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    model, mk, mask, sens, low, scale, plain, noisy, maps = slice_inputs(dev)
    with SlicePipeline(model, slots=1, graphs=False) as pipe:
        for bad in ((low, scale, SEED, 0), N.NoiseSpec(low, scale, SEED, -1), N.NoiseSpec(low[:3, :3], scale, SEED, 0), N.NoiseSpec(low.cpu())):
            with pytest.raises((CineHipError, ValueError)):
                pipe.submit(mk, mask, sens, noise=bad)
        with pytest.raises(CineHipError, match="forward"):
            N.pseudo_replica(model, mk, mask, sens, replicas=4, pipeline=pipe, output="complex")


class SensReduce(torch.nn.Module):
    """x = sum_c conj(S_c) IFFT2c(k_c): a linear reconstruction with the models' forward signature."""

    def forward(self, masked_kspace, mask, sens_maps, output="complex"):
        from cine_hip import ops
        assert output == "complex"
        return ops.sens_reduce(masked_kspace, sens_maps)


def ifft2c(k):
    ax = (-2, -1)
    return np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(k, axes=ax), norm="ortho"), axes=ax)


@pytest.mark.parametrize("t,c,h,w", [(4, 4, 16, 12), (3, 5, 7, 13)])
def test_linear_reconstruction_vs_reference(dev, t, c, h, w):
    """32 replicas: the std (and mean) map against the float64 restatement fed the reference's own noise, at BAR_CAP of the map's peak."""
    from cine_hip import noise as N
    n_rep = 32
    rs = np.random.RandomState(40 + c)
    sens = (rs.standard_normal((c, h, w)) + 1j * rs.standard_normal((c, h, w))) / np.sqrt(2 * c)
    low = R.random_chol(rs, c)[0]
    m = (rs.uniform(size=(t, h)) < 0.5).astype(np.uint8)
    m[:, h // 2] = 1
    k0 = ((rs.standard_normal((t, c, h, w)) + 1j * rs.standard_normal((t, c, h, w))) * m[:, None, :, None]).astype(np.complex64)
    sens32 = sens.astype(np.complex64)
    acc = R.Welford()
    for r in range(n_rep):
        kr, _ = R.noise_add(k0, m, chol=low, scale=0.5, seed=SEED, replica=r)
        x = (sens32.astype(np.complex128).conj()[None] * ifft2c(kr)).sum(axis=1)
        acc.add(np.stack([x.real, x.imag], axis=-1))
    mean, std, snr, _ = acc.finish(pairs=True)

    def pairs(z):
        return torch.from_numpy(np.stack([z.real, z.imag], axis=-1).astype(np.float32)).to(dev)
    got = N.pseudo_replica(SensReduce().eval(), pairs(k0)[None], torch.from_numpy(m).to(dev).view(1, t, 1, h, 1, 1),
                           pairs(sens32)[None, None], chol=torch.from_numpy(low).to(dev), scale=0.5, replicas=n_rep, seed=SEED,
                           output="complex")
    assert got.replicas == n_rep and tuple(got.std.shape) == (1, t, 1, h, w)
    for name, a, want in (("std", got.std, std), ("mean", got.mean, mean), ("snr", got.snr, snr)):
        err = float(np.abs(a.cpu().numpy().reshape(want.shape) - want).max()) / float(np.abs(want).max())
        print(f"({t},{c},{h},{w}) {name}: {err:.3e} of the peak (bar {BAR_CAP:.0e})")
        assert err <= BAR_CAP, name


def test_g_factor_and_finish_with_reference(dev):
    from cine_hip import noise as N
    rs = np.random.RandomState(9)
    a = torch.from_numpy(np.abs(rs.standard_normal((2, 5, 7))).astype(np.float32)).to(dev)
    f = torch.from_numpy(np.abs(rs.standard_normal((2, 5, 7))).astype(np.float32) + 0.1).to(dev)
    f[0, 0, 0] = 0.0
    mask = torch.zeros(1, 4, 1, 8, 1, 1, dtype=torch.uint8, device=dev)
    mask[:, :, :, ::4] = 1                                                    # R = 4
    g = N.g_factor(a, f, mask)
    want = a.double() / (f.double() * 2.0)
    want[0, 0, 0] = 0.0
    assert float((g.double() - want).abs().max()) <= 1e-6 * float(want.abs().max()) and float(g[0, 0, 0]) == 0.0


def test_capture_with_a_device_counter(dev):
    """The call and the counter's bump in one graph: three replays give the bits of replicas 0, 1, 2 passed by value."""
    from cine_hip import noise as N
    model, mk, mask, sens, low, scale, plain, noisy, maps = slice_inputs(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty_like(mk)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        N.add_noise(mk, mask, low, scale=scale, seed=SEED, replica_dev=counter, out=out)      # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        N.add_noise(mk, mask, low, scale=scale, seed=SEED, replica_dev=counter, out=out)
        counter.add_(1)
    counter.zero_()
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, N.add_noise(mk, mask, low, scale=scale, seed=SEED, replica=r)), f"replay {r}"
    assert int(counter) == 3
