"""Noise in front of the front-end, end to end: ``SlicePipeline.submit_raw(..., noise=, noise_mask=)`` and ``noise.pseudo_replica_raw``.

In flight against sequential: every replica's result equals ``model(prepare_masked_slice(add_noise_raw(raw[:n], ...), mask, <the same
front-end arguments>), mask, sens)`` bit for bit, graphs on and off -- plain, with a coil matrix, with ``virtual_coils`` (the matrix of
the NOISY slice), with a whitener folded in, prospectively undersampled raw with a ``noise_mask`` of both layouts from all three places,
and a raw size the line engines refuse (the window transform).  Replicas are interleaved with plain submissions, which return what
they always returned; one graph set serves all; the caller's raw data keep their bits.
``pseudo_replica_raw`` with and without ``pipeline=`` gives the same maps.  A linear reconstruction (ops.sens_reduce as a module)
against the float64 restatement of the whole chain -- oracle.frontend_ref.prepare_slice, the mask, the coil sum -- fed
tests/noise_reference.py's own noise on the raw layout, at kernel_sweep.BAR_CAP of each map's peak.  ``add_noise_raw(...,
replica_dev=counter)`` captured in a graph with the counter bumped inside draws replicas 0, 1, 2 on three replays."""
import numpy as np
import pytest
import torch

import noise_reference as R
from kernel_sweep import BAR_CAP, same_bits
from whitening_ref import designed_cov, whitener_ref

pytestmark = pytest.mark.gpu
FS = (0.7, 0.0, 0.3, 0.3)
SEED, AMP = 11, 1e-6
SCALE = 0.05 * AMP                                                            # noise of 5 % of the raw data's peak


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def raw_data(t, nx, ny, c, seed, floor=0.02):
    """Complex64 (t, x, y, coil) with the energy of a k-space: a peak at the centre over a floor."""
    rs = np.random.RandomState(seed)
    x, y = np.arange(nx)[:, None] - nx // 2, np.arange(ny)[None, :] - ny // 2
    w = np.exp(-(x * x / (2.0 * (nx / 8.0) ** 2) + y * y / (2.0 * (ny / 8.0) ** 2))) + floor
    z = rs.standard_normal((t, nx, ny, c)) + 1j * rs.standard_normal((t, nx, ny, c))
    return (AMP * z * w[None, :, :, None]).astype(np.complex64)


def row_mask(t, X, seed):
    """uint8 (1, t, 1, X, 1, 1): a fully sampled centre, every third row or so elsewhere."""
    rs = np.random.RandomState(1000 + seed)
    m = (rs.uniform(size=(1, t, 1, X, 1, 1)) < 0.3).astype(np.uint8)
    m[:, :, :, X // 2 - 2:X // 2 + 2] = 1
    return torch.from_numpy(m)


def sens_maps(c, X, Y, seed):
    """(1, 1, c, X, Y, 2) float32: smooth random maps of unit root-sum-of-squares."""
    rs = np.random.RandomState(2000 + seed)
    x, y = np.meshgrid(np.linspace(-1, 1, X), np.linspace(-1, 1, Y), indexing="ij")
    a = rs.standard_normal((c, 3)) + 1j * rs.standard_normal((c, 3))
    s = a[:, 0, None, None] + a[:, 1, None, None] * x[None] + a[:, 2, None, None] * y[None]
    s = s / np.sqrt((np.abs(s) ** 2).sum(axis=0, keepdims=True))
    return torch.from_numpy(np.stack([s.real, s.imag], axis=-1).astype(np.float32))[None, None]


def acquired_lines(n, nx, seed):
    """uint8 (n, nx): the acquired lines of prospectively undersampled raw data."""
    rs = np.random.RandomState(3000 + seed)
    m = (rs.uniform(size=(n, nx)) < 0.4).astype(np.uint8)
    m[:, nx // 2 - 2:nx // 2 + 2] = 1
    return m


# name -> (raw shape (t, x, y, c), crop, n_frames, coils behind the front-end, front-end keywords(dev))
def _matrix(dev):
    rs = np.random.RandomState(7)
    q, _ = np.linalg.qr(rs.standard_normal((4, 4)) + 1j * rs.standard_normal((4, 4)))
    return torch.from_numpy(q[:3].astype(np.complex64)).to(dev)


def _whitener(dev):
    return torch.from_numpy(whitener_ref(designed_cov(4, 5))[0]).to(dev)


CASES = {
    "plain": ((6, 20, 14, 4), (16, 12), 4, 4, lambda dev: {}),
    "coil_matrix": ((6, 20, 14, 4), (16, 12), 4, 3, lambda dev: {"coil_matrix": _matrix(dev)}),
    "virtual": ((6, 20, 14, 4), (16, 12), 4, 3, lambda dev: {"virtual_coils": 3}),
    "whitened": ((6, 20, 14, 4), (16, 12), 4, 3, lambda dev: {"virtual_coils": 3, "whitener": _whitener(dev)}),
    "prospective": ((6, 20, 14, 4), (16, 12), 4, 4, lambda dev: {"apply_mask": False}),
    "window": ((3, 401, 6, 3), (16, 6), 4, 3, lambda dev: {}),
}
_CACHE = {}


def case(name, dev):
    """The inputs of a case and its sequential results, computed once: (model, raw (host complex64), mask, sens, L, n, crop, keywords,
    noise masks per replica, plain result, noisy results of replicas 0 .. 3)."""
    if name in _CACHE:
        return _CACHE[name]
    from cine_hip import frontend as FE, noise as N, ops
    from cine_hip.classical import KtSparseSense
    shape, crop, frames, v, make = CASES[name]
    t, nx, ny, c = shape
    n = min(frames, t)
    assert (ops.fft_line_supported(nx) and ops.fft_line_supported(ny)) == (name != "window")
    raw = raw_data(*shape, seed=len(name))
    nmasks = [None] * 4
    if name == "prospective":                                                  # unacquired lines hold zeros and get no noise
        lines = acquired_lines(n, nx, 1)                                       # (n, nx): a pattern per frame
        raw[:n] *= lines[:, :, None, None]
        samples = np.repeat(lines[:1, :, None], ny, axis=2)                    # (1, nx, ny): one pattern for all frames, with holes in a line
        samples[0, nx // 2, ::2] = 0
        nmasks = [torch.from_numpy(lines), torch.from_numpy(samples), torch.from_numpy(lines).bool(), torch.from_numpy(samples)]
    raw = torch.from_numpy(raw)
    mask, sens = row_mask(n, crop[0], 3).to(dev), sens_maps(v, crop[0], crop[1], 4).to(dev)
    low = torch.from_numpy(R.random_chol(np.random.RandomState(5), c)[0]).to(dev)
    fe = make(dev)
    model = KtSparseSense(iters=3).eval()
    rd = raw.to(dev)

    def sequential(r):
        x = rd[:n]
        if r is not None:
            nm = None if nmasks[r] is None else nmasks[r].to(dev)
            x = N.add_noise_raw(x, low, noise_mask=nm, scale=SCALE, seed=SEED, replica=r)
        with torch.no_grad():
            return model(FE.prepare_masked_slice(x, mask, crop, n, FS, 1e6, **fe), mask, sens).clone()
    plain = sequential(None)
    noisy = [sequential(r) for r in range(4)]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(plain).all()) and not same_bits(noisy[0], plain) and not same_bits(noisy[0], noisy[1])
    _CACHE[name] = (model, raw, mask, sens, low, n, crop, fe, nmasks, plain, noisy)
    return _CACHE[name]


def places(x, r, dev):
    """A host tensor from the three places an input may lie in, by replica."""
    return (x.to(dev), x.pin_memory(), x.numpy())[r % 3]


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("name", list(CASES))
def test_in_flight_equals_sequential(dev, name, graphs):
    from cine_hip import noise as N
    from cine_hip.pipeline import SlicePipeline
    model, raw, mask, sens, low, n, crop, fe, nmasks, plain, noisy = case(name, dev)
    keep = raw.clone()
    on_dev = raw.to(dev)
    kw = dict(crop_shape=crop, n_frames=CASES[name][2], **fe)
    with SlicePipeline(model, slots=2, graphs=graphs) as pipe:
        for r in range(4):                                                     # replicas and plain submissions interleaved
            src = on_dev if r % 3 == 0 else places(raw, r, dev)
            nm = None if nmasks[r] is None else places(nmasks[r], r, dev)      # device lines, pinned samples, numpy bool lines, device samples
            pipe.submit_raw(src, mask, sens, tag=("noise", r), noise=N.NoiseSpec(low, SCALE, SEED, r), noise_mask=nm, **kw)
            pipe.submit_raw(src, mask, sens, tag=("plain", r), **kw)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1                                            # neither the spec nor the mask is part of the set key
    for r in range(4):
        assert same_bits(got[("plain", r)], plain), f"{name}: plain submission {r}"
        assert same_bits(got[("noise", r)], noisy[r]), f"{name}: replica {r}"
    assert torch.equal(raw, keep) and torch.equal(on_dev.cpu(), keep), "the caller's raw data were written"


@pytest.mark.parametrize("name", ["plain", "virtual", "prospective"])
def test_pseudo_replica_raw_loop_and_pipeline_give_the_same_maps(dev, name):
    from cine_hip import noise as N
    from cine_hip.pipeline import SlicePipeline
    model, raw, mask, sens, low, n, crop, fe, nmasks, plain, noisy = case(name, dev)
    nm = None if nmasks[0] is None else nmasks[0].to(dev)
    kw = dict(chol=low, scale=SCALE, replicas=16, seed=SEED, noise_mask=nm, crop_shape=crop, n_frames=CASES[name][2], **fe)
    loop = N.pseudo_replica_raw(model, raw, mask, sens, **kw)
    if nm is None:                                                             # (the prospective case's replicas differ in their masks)
        acc = R.Welford()
        for o in noisy:                                                        # the loop's first replicas are the sequential ones
            acc.add(o.cpu().numpy())
        first = N.pseudo_replica_raw(model, raw.numpy(), mask, sens, **dict(kw, replicas=4))
        mean, std, _, _ = acc.finish()
        for a, want in ((first.mean, mean), (first.std, std)):
            assert float(np.abs(a.cpu().numpy() - want).max()) <= 1e-5 * float(np.abs(want).max())
    with SlicePipeline(model, slots=3) as pipe:
        piped = N.pseudo_replica_raw(model, raw, mask, sens, pipeline=pipe, **kw)
        assert pipe.pending() == 0 and pipe.set_builds == 1
    assert loop.replicas == piped.replicas == 16 and loop.g is None and piped.g is None and float(loop.std.min()) > 0
    for a, b, what in zip(loop[:3], piped[:3], ("mean", "std", "snr")):
        assert same_bits(a, b), f"{name}: {what} differs between the loop and the pipeline"


class SensReduce(torch.nn.Module):
    """x = sum_c conj(S_c) IFFT2c(k_c): a linear reconstruction with the models' forward signature."""

    def forward(self, masked_kspace, mask, sens_maps, output="complex"):
        from cine_hip import ops
        assert output == "complex"
        return ops.sens_reduce(masked_kspace, sens_maps)


def ifft2c(k):
    ax = (-2, -1)
    return np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(k, axes=ax), norm="ortho"), axes=ax)


def test_linear_end_to_end_vs_float64(dev):
    """32 replicas of raw (4, 18, 14, 4) through front-end, mask and coil sum: std, mean and SNR maps against the float64 restatement fed
    the reference's own noise on the raw layout, at BAR_CAP of each map's peak; first the noise-free output at BAR_CAP / 4."""
    from cine_hip import frontend as FE, noise as N
    from oracle import frontend_ref as F
    (t, nx, ny, c), crop, n_rep, scale = (4, 18, 14, 4), (16, 12), 32, 0.25 * AMP
    rs = np.random.RandomState(44)
    raw = raw_data(t, nx, ny, c, seed=9)
    sens = sens_maps(c, crop[0], crop[1], 6)
    s = sens[0, 0].numpy().astype(np.float64)
    s = s[..., 0] + 1j * s[..., 1]
    low = R.random_chol(rs, c)[0]
    mask = row_mask(t, crop[0], 8)
    m = mask.numpy().reshape(t, 1, crop[0], 1).astype(np.float64)

    def restated(raw_c):
        k, _ = F.prepare_slice(raw_c, crop, t, FS, 1e6)
        return (s.conj()[None] * ifft2c(np.asarray(k, dtype=np.complex128) * m)).sum(axis=1)          # (t, X, Y)

    model = SensReduce().eval()
    rd, md, sd = torch.from_numpy(raw).to(dev), mask.to(dev), sens.to(dev)
    clean = model(FE.prepare_masked_slice(rd, md, crop, t, FS, 1e6), md, sd).cpu().numpy().reshape(t, crop[0], crop[1], 2)
    want0 = restated(raw)
    err0 = float(np.abs((clean[..., 0] + 1j * clean[..., 1]) - want0).max()) / float(np.abs(want0).max())
    print(f"noise-free output vs the oracle: {err0:.3e} of the peak (bar {BAR_CAP / 4:.1e})")
    assert err0 <= BAR_CAP / 4
    acc = R.Welford()
    for r in range(n_rep):
        eta = np.moveaxis(R.noise(t, c, nx, ny, seed=SEED, replica=r, chol=low, scale=scale), 1, -1)     # (t, nx, ny, c)
        x = restated(raw.astype(np.complex128) + eta)
        acc.add(np.stack([x.real, x.imag], axis=-1))
    mean, std, snr, _ = acc.finish(pairs=True)
    got = N.pseudo_replica_raw(model, rd, md, sd, chol=torch.from_numpy(low).to(dev), scale=scale, replicas=n_rep, seed=SEED,
                               output="complex", crop_shape=crop, n_frames=t)
    assert got.replicas == n_rep and got.std.numel() == std.size
    for name, a, want in (("std", got.std, std), ("mean", got.mean, mean), ("snr", got.snr, snr)):
        err = float(np.abs(a.cpu().numpy().reshape(want.shape) - want).max()) / float(np.abs(want).max())
        print(f"{name}: {err:.3e} of the peak (bar {BAR_CAP:.0e})")
        assert err <= BAR_CAP, name


def test_binding_forms(dev):
    """Complex in, complex out; pairs in, pairs out; a leading 1 of the mask is expanded; a bool mask is a uint8 one; out= is filled."""
    from cine_hip import noise as N
    raw = torch.from_numpy(raw_data(3, 5, 7, 3, seed=2)).to(dev)
    low = torch.from_numpy(R.random_chol(np.random.RandomState(6), 3)[0]).to(dev)
    kw = dict(scale=SCALE, seed=SEED, replica=2)
    a = N.add_noise_raw(raw, low, **kw)
    b = N.add_noise_raw(torch.view_as_real(raw), low, **kw)
    assert a.dtype == torch.complex64 and b.dtype == torch.float32 and same_bits(torch.view_as_real(a), b) and not torch.equal(a, raw)
    one = torch.from_numpy(acquired_lines(1, 5, 2)).to(dev)
    full = one.expand(3, 5).contiguous()
    for mk in (one, one.bool(), full.bool()):
        assert same_bits(N.add_noise_raw(torch.view_as_real(raw), low, noise_mask=mk, **kw), N.add_noise_raw(torch.view_as_real(raw), low, noise_mask=full, **kw))
    plane = full[:, :, None].expand(3, 5, 7).contiguous()
    assert same_bits(N.add_noise_raw(torch.view_as_real(raw), low, noise_mask=plane[:1], **kw), N.add_noise_raw(torch.view_as_real(raw), low, noise_mask=full, **kw))
    out = torch.empty_like(raw)
    assert N.add_noise_raw(raw, low, out=out, **kw) is out and torch.equal(out, a)
    work = raw.clone()
    assert N.add_noise_raw(work, low, out=work, **kw) is work and torch.equal(work, a)


def test_capture_with_a_device_counter(dev):
    """The call and the counter's bump in one graph: three replays give the bits of replicas 0, 1, 2 passed by value."""
    from cine_hip import noise as N
    raw = torch.view_as_real(torch.from_numpy(raw_data(3, 5, 7, 3, seed=3)).to(dev))
    low = torch.from_numpy(R.random_chol(np.random.RandomState(6), 3)[0]).to(dev)
    nm = torch.from_numpy(acquired_lines(3, 5, 4)).to(dev)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty_like(raw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        N.add_noise_raw(raw, low, noise_mask=nm, scale=SCALE, seed=SEED, replica_dev=counter, out=out)      # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        N.add_noise_raw(raw, low, noise_mask=nm, scale=SCALE, seed=SEED, replica_dev=counter, out=out)
        counter.add_(1)
    counter.zero_()
    for r in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, N.add_noise_raw(raw, low, noise_mask=nm, scale=SCALE, seed=SEED, replica=r)), f"replay {r}"
    assert int(counter) == 3


def test_refusals_leave_nothing_pending(dev):
    from cine_hip import noise as N
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    model, raw, mask, sens, low, n, crop, fe, nmasks, plain, noisy = case("plain", dev)
    kw = dict(crop_shape=crop, n_frames=CASES["plain"][2])
    spec = N.NoiseSpec(low, SCALE, SEED, 0)
    with SlicePipeline(model, slots=1, graphs=False) as pipe:
        pipe.submit_raw(raw, mask, sens, tag="first", **kw)
        before = (pipe.pending(), pipe.set_builds)
        for bad in ((low, SCALE, SEED, 0), N.NoiseSpec(low, SCALE, SEED, -1), N.NoiseSpec(low[:3, :3], SCALE, SEED, 0), N.NoiseSpec(low.cpu())):
            with pytest.raises((CineHipError, ValueError)):
                pipe.submit_raw(raw, mask, sens, noise=bad, **kw)
        for shape in ((n + 1, 20), (n, 16), (n, 20, 12), (20,)):               # not the kept frames, the crop grid, a wrong ny, no frame axis
            with pytest.raises(CineHipError, match="noise_mask: shape"):
                pipe.submit_raw(raw, mask, sens, noise=spec, noise_mask=torch.ones(shape, dtype=torch.uint8), **kw)
        with pytest.raises(CineHipError, match="uint8 or bool"):
            pipe.submit_raw(raw, mask, sens, noise=spec, noise_mask=torch.ones(n, 20), **kw)
        with pytest.raises(CineHipError, match="without noise="):
            pipe.submit_raw(raw, mask, sens, noise_mask=torch.ones(n, 20, dtype=torch.uint8), **kw)
        assert (pipe.pending(), pipe.set_builds) == before
        with pytest.raises(CineHipError, match="forward"):
            N.pseudo_replica_raw(model, raw, mask, sens, replicas=4, pipeline=pipe, output="complex", **kw)
        with pytest.raises(CineHipError, match="pending"):
            N.pseudo_replica_raw(model, raw, mask, sens, replicas=4, pipeline=pipe, **kw)
        pipe.submit_raw(raw, mask, sens, tag="noisy", noise=spec, **kw)        # usable after every refusal
        got = dict(pipe.drain())
    assert same_bits(got["first"], plain) and same_bits(got["noisy"], noisy[0])
    with pytest.raises(CineHipError, match="espirit"):
        N.pseudo_replica_raw(model, raw, mask, "espirit", replicas=4, **kw)
    with pytest.raises(CineHipError, match="noise_mask"):
        N.add_noise_raw(raw.to(dev), low, noise_mask=torch.ones(n, 20, dtype=torch.uint8))
    with pytest.raises(ValueError, match="noise_mask"):
        N.add_noise_raw(raw.to(dev), low, noise_mask=torch.ones(n, 20, dtype=torch.uint8, device=dev))       # raw has all 6 frames
