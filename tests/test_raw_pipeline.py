"""Raw k-space in flight: ops.raw_ingest, frontend.prepare_masked_slice and SlicePipeline.submit_raw on the GPU.

The ingest kernel against the torch expression prepare_slice uses, shape by shape; prepare_masked_slice against today's composition
(prepare_slice, then ops.apply_mask) bit for bit, against the reference's stored result and against the float64 oracle; its capture on a
pipeline stream; submit_raw against the sequential forward ``model(prepare_masked_slice(raw, mask, ...), mask)`` bit for bit."""
import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

FS = (0.7, 0.0, 0.3, 0.3)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _raw(t, nx, ny, c, seed, amp=1.0):
    """Complex64 (t, x, y, coil) with the energy of a k-space: a peak at the centre over a noise floor."""
    rs = np.random.RandomState(seed)
    x, y = np.arange(nx)[:, None] - nx // 2, np.arange(ny)[None, :] - ny // 2
    w = np.exp(-(x * x / (2.0 * (nx / 8.0) ** 2) + y * y / (2.0 * (ny / 8.0) ** 2))) + 0.02
    z = rs.standard_normal((t, nx, ny, c)) + 1j * rs.standard_normal((t, nx, ny, c))
    return (amp * z * w[None, :, :, None]).astype(np.complex64)


def _row_mask(t, X, seed, shared=False):
    """uint8 (1, t | 1, 1, X, 1, 1): a fully sampled centre whose width depends on the seed, every third row or so elsewhere."""
    rs = np.random.RandomState(1000 + seed)
    tt = 1 if shared else t
    m = (rs.uniform(size=(1, tt, 1, X, 1, 1)) < 0.3).astype(np.uint8)
    half = 1 + seed % 3
    m[:, :, :, X // 2 - half:X // 2 + half] = 1
    return torch.from_numpy(m)


def _matrix(v, c, seed):
    rs = np.random.RandomState(2000 + seed)
    q, _ = np.linalg.qr(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c)))
    return torch.from_numpy(q[:v].astype(np.complex64))


def _cplx(a):
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(a).astype(np.complex64)))


# ------------------------------------------------------------------ 1. the ingest kernel, shape by shape
@pytest.mark.parametrize("nx,ny", [(7, 5), (200, 200), (384, 144), (243, 125)])
@pytest.mark.parametrize("c", [1, 3, 15, 30, 33, 128])
def test_raw_ingest_equals_the_torch_expression(dev, c, nx, ny):
    from cine_hip import ops
    rs = np.random.RandomState(c * 1000 + nx)
    for t_in, t_out in ((3, 2), (2, 2)):
        n_in = t_in * nx * ny * c
        for shift in (0, 2):                                   # complex elements: 0, or 16 bytes past a 128-byte boundary
            flat = torch.empty(n_in + 4, dtype=torch.complex64, device=dev)
            assert flat.data_ptr() % 128 == 0
            raw = flat[shift:shift + n_in].view(t_in, nx, ny, c)
            raw.copy_(torch.from_numpy((rs.standard_normal((t_in, nx, ny, c)) + 1j * rs.standard_normal((t_in, nx, ny, c))).astype(np.complex64)))
            assert raw.data_ptr() % 16 == 0 and (shift == 0 or raw.data_ptr() % 128 == 16)
            for scale in (1.0, 1e6):
                want = torch.view_as_real((raw[:t_out] * scale).permute(0, 3, 1, 2).contiguous())
                n_out, pad = want.numel(), 64
                big = torch.full((n_out + 2 * pad,), float("nan"), dtype=torch.float32, device=dev)
                out = big[pad:pad + n_out].view(want.shape)
                got = ops.raw_ingest(raw, t_out, scale, out=out)
                assert got.data_ptr() == out.data_ptr()
                assert torch.equal(got, want), (c, nx, ny, t_in, t_out, shift, scale, float((got - want).abs().max()))
                assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + n_out:]).all()), "wrote outside its output"
                fresh = ops.raw_ingest(torch.view_as_real(raw), t_out, scale)       # float32 pairs in, an output of its own
                assert torch.equal(fresh, want)


# ------------------------------------------------------------------ 2. prepare_masked_slice == today's composition
FRONT_CASES = {"line": ((4, 30, 28, 3), (24, 20), 3), "window": ((3, 416, 208, 4), (200, 200), 2), "odd_crop": ((4, 30, 28, 2), (21, 17), 3),
               "window_odd": ((3, 416, 24, 2), (21, 17), 3)}


@pytest.mark.parametrize("apply_mask", [True, False])
@pytest.mark.parametrize("with_matrix", [False, True])
@pytest.mark.parametrize("name", list(FRONT_CASES))
def test_prepare_masked_slice_equals_todays_composition(dev, name, with_matrix, apply_mask):
    from cine_hip import frontend as FE, ops
    shape, crop, n = FRONT_CASES[name]
    assert (ops.fft_line_supported(shape[1]) and ops.fft_line_supported(shape[2])) == (not name.startswith("window"))
    raw = torch.from_numpy(_raw(*shape, seed=3, amp=1e-6)).to(dev)
    a = _matrix(max(1, shape[3] - 1), shape[3], 5).to(dev) if with_matrix else None
    k, _ = FE.prepare_slice(raw, crop, n, FS, 1e6, coil_matrix=a)
    T = min(n, shape[0])
    for shared in (False, True):
        mask = _row_mask(T, crop[0], seed=7, shared=shared).to(dev)
        got = FE.prepare_masked_slice(raw, mask, crop, n, FS, 1e6, coil_matrix=a, apply_mask=apply_mask)
        want = ops.apply_mask(k, mask.expand(1, T, 1, crop[0], 1, 1).contiguous())[None] if apply_mask else k[None]
        assert got.shape == want.shape == (1, T, k.shape[1]) + crop + (2,)
        assert torch.equal(got, want), (name, with_matrix, apply_mask, shared, float((got - want).abs().max()))
        out = torch.full_like(want, float("nan"))
        assert FE.prepare_masked_slice(torch.view_as_real(raw), mask.bool(), crop, n, FS, 1e6, coil_matrix=a, apply_mask=apply_mask, out=out) is out
        assert torch.equal(out, want)


# ------------------------------------------------------------------ 3. against something that is not the code under test
def test_prepare_masked_slice_vs_reference_golden_and_oracle(golden, dev):
    from cine_hip import frontend as FE
    from oracle import frontend_ref
    g = golden("frontend")
    crop, n, fs = tuple(int(v) for v in g["crop_shape"]), int(g["n_slices"]), tuple(float(v) for v in g["filter_size"])
    raw = torch.from_numpy(g["raw"]).to(dev)
    got = FE.prepare_masked_slice(raw, None, crop, n, fs, apply_mask=False)
    e = rel_err(got[0].cpu(), _cplx(g["kspace"]))
    print(f"unmasked vs the reference's stored kspace: rel_err {e:.3e}")
    assert e < 1e-5
    T = got.shape[1]
    mask = _row_mask(T, crop[0], seed=4)
    kref, _ = frontend_ref.prepare_slice(g["raw"], crop, n, fs)
    want = np.asarray(kref) * mask[0].numpy().reshape(T, 1, crop[0], 1)
    gotm = FE.prepare_masked_slice(raw, mask.to(dev), crop, n, fs)[0].cpu()
    e = rel_err(gotm, _cplx(want))
    print(f"masked vs the oracle times the mask: rel_err {e:.3e}")
    assert e < 1e-5
    dropped = (mask[0].reshape(T, 1, crop[0], 1, 1) == 0).expand_as(gotm)
    assert bool(dropped.any()) and bool((gotm[dropped] == 0).all())


# ------------------------------------------------------------------ 4. capturable
@pytest.mark.parametrize("name,with_matrix", [("line", False), ("window_odd", False), ("line", True), ("window_odd", True)])
def test_prepare_masked_slice_is_capturable_on_a_pipeline_stream(dev, name, with_matrix):
    from cine_hip import frontend as FE
    from cine_hip.pipeline import pipeline_streams
    shape, crop, n = FRONT_CASES[name]
    T = min(n, shape[0])
    raws = [torch.from_numpy(_raw(*shape, seed=20 + j, amp=1e-6)).to(dev) for j in range(3)]
    a = _matrix(2, shape[3], 9).to(dev) if with_matrix else None
    mask = _row_mask(T, crop[0], seed=2).to(dev)
    want = [FE.prepare_masked_slice(r, mask, crop, n, FS, 1e6, coil_matrix=a).clone() for r in raws]
    static = torch.zeros_like(raws[0])
    s = pipeline_streams(dev, 1)[0][0]
    assert s != torch.cuda.default_stream(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        FE.prepare_masked_slice(static, mask, crop, n, FS, 1e6, coil_matrix=a)       # warm outside capture
    s.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        out = FE.prepare_masked_slice(static, mask, crop, n, FS, 1e6, coil_matrix=a)
    for j, r in enumerate(raws):
        static.copy_(r)
        torch.cuda.synchronize()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[j]), (name, with_matrix, j)


# ------------------------------------------------------------------ 5. submit_raw == the sequential forward
def _model(name):
    import reconstruction.models as M
    if name == "cfg2":
        return M.VarNet(6, 8, 3, 16, 3, "XF"), 1, ("lambda",)
    if name == "xpdnet_xt":
        return M.XPDNet(num_cascades=2, sens_chans=4, sens_pools=2, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[1, 1],
                        first_conv_n_filters=8, n_primal=2, dynamic_type="XT"), 6, ()
    if name == "cinenet_3d":
        return M.CineNet(2, 3, 4, 2, "3D"), 7, ("lambda",)
    return M.VarNet_RNN(2, 4, 2, 6), 9, ("lambda",)


RAW_SHAPE, CROP, FRAMES, COILS = (7, 30, 28, 3), (24, 20), 5, 3           # 7 frames in the file, 5 kept
N_SLICES = 13                                                             # 4 S + 1 for S = 3 (S = 1 uses the first 5)


class Case:
    def __init__(self, name, dev):
        from cine_hip import frontend as FE, ops, synth
        net, wseed, keep = _model(name)
        synth.fill_parameters_(net, wseed, keep=keep)
        self.name, self.net, self.dev = name, net.to(dev).eval(), dev
        self.raws = [_raw(*RAW_SHAPE, seed=50 + j, amp=1e-6) for j in range(N_SLICES)]
        self.masks = [_row_mask(FRAMES, CROP[0], seed=j) for j in range(N_SLICES)]
        self.sens = None
        if name == "cinenet_3d":
            self.sens = [synth.make_cine_slice(FRAMES, COILS, CROP[0], CROP[1], accel=4, center_lines=4, seed=70 + j)["sens_maps"].contiguous()
                         for j in range(N_SLICES)]
        self.want, self.zf = [], []
        with torch.no_grad():
            for j in range(N_SLICES):
                mk = FE.prepare_masked_slice(torch.from_numpy(self.raws[j]).to(dev), self.masks[j].to(dev), CROP, FRAMES, FS, 1e6)
                args = (mk, self.masks[j].to(dev)) + ((self.sens[j].to(dev),) if self.sens else ())
                self.want.append(self.net(*args).clone())
                self.zf.append(ops.zero_filled_rss(mk))
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(w).all()) for w in self.want)
        assert not torch.equal(self.want[0], self.want[1])

    def inputs(self, j, form):
        raw, mask, sens = torch.from_numpy(self.raws[j]), self.masks[j], self.sens[j] if self.sens else None
        if form == "device":
            return raw.to(self.dev), mask.to(self.dev), None if sens is None else sens.to(self.dev)
        if form == "pinned":
            return raw.pin_memory(), mask.pin_memory(), None if sens is None else sens.pin_memory()
        return self.raws[j], mask.numpy().astype(np.float32), None if sens is None else np.ascontiguousarray(torch.view_as_complex(sens).numpy())


_CASES = {}


@pytest.fixture
def case(request, dev):
    name = request.param
    if name not in _CASES:
        _CASES.clear()
        _CASES[name] = Case(name, dev)
    return _CASES[name]


def _run(case, S, form="device", **kw):
    from cine_hip.pipeline import SlicePipeline
    n = 4 * S + 1
    got, order = {}, []
    with SlicePipeline(case.net, slots=S, **kw) as pipe:
        for j in range(n):
            raw, mask, sens = case.inputs(j, form)
            h = pipe.submit_raw(raw, mask, sens, tag=f"s{j}", crop_shape=CROP, n_frames=FRAMES)
            assert (h.index, h.slot) == (j, j % S) and h.parity == (j // S) & 1
            for tag, out in pipe.results():
                order.append(tag); got[tag] = out
        for tag, out in pipe.drain():
            order.append(tag); got[tag] = out
        assert pipe.pending() == 0 and pipe.set_builds == 1
    assert order == [f"s{j}" for j in range(n)]
    return [got[f"s{j}"] for j in range(n)]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("form", ["device", "pinned", "numpy"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("case", ["cfg2", "xpdnet_xt", "cinenet_3d", "varnet_rnn"], indirect=True)
def test_submit_raw_matches_the_sequential_forward_bit_for_bit(case, S, form):
    outs = _run(case, S, form)
    for j, o in enumerate(outs):
        assert o.is_cuda and _same(o, case.want[j]), (case.name, S, form, j, float((o - case.want[j]).abs().max()))


@pytest.mark.parametrize("case", ["cfg2", "cinenet_3d"], indirect=True)
def test_submit_raw_host_outputs_and_zero_filled(case):
    outs = _run(case, 3, "pinned", out="host", zero_filled=True)
    for j, (o, z) in enumerate(outs):
        assert not o.is_cuda and o.is_pinned() and not z.is_cuda
        assert _same(o, case.want[j]) and _same(z, case.zf[j]), j


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("case", ["cfg2", "varnet_rnn"], indirect=True)
def test_submit_raw_eager_mode_gives_the_same_bits(case, S):
    outs = _run(case, S, "device", graphs=False, zero_filled=True)
    for j, (o, z) in enumerate(outs):
        assert _same(o, case.want[j]) and _same(z, case.zf[j]), j


# ------------------------------------------------------------------ 6. mixed coil counts, one graph set
@pytest.mark.parametrize("nx,ny,crop", [(48, 40, (32, 24)), (416, 24, (32, 20))], ids=["line", "window"])
def test_mixed_coil_counts_share_one_graph_set(dev, nx, ny, crop):
    import reconstruction.models as M
    from cine_hip import frontend as FE, synth
    from cine_hip.pipeline import SlicePipeline
    net = M.VarNet(6, 8, 3, 16, 3, "XF")
    synth.fill_parameters_(net, 1, keep=("lambda",))
    net = net.to(dev).eval()
    frames, V = 5, 12
    plan = [(20, 1), (30, 2), (20, 3), (30, 4), (20, 5), (30, 6), (20, 7)]           # the larger scan arrives second: the raw buffers grow
    raws = [torch.from_numpy(_raw(6, nx, ny, c, seed=seed, amp=1e-6)) for c, seed in plan]
    mats = [FE.coil_compression_matrix(r.to(dev), V, frames)[0] for r in raws]     # one matrix per scan
    masks = [_row_mask(frames, crop[0], seed=seed) for _, seed in plan]
    with torch.no_grad():
        want = [net(FE.prepare_masked_slice(r.to(dev), m.to(dev), crop, frames, FS, 1e6, coil_matrix=a), m.to(dev)).clone()
                for r, m, a in zip(raws, masks, mats)]
        plain = [net(FE.prepare_masked_slice(r.to(dev), m.to(dev), crop, frames, FS, 1e6), m.to(dev)).clone() for r, m in zip(raws[:3], masks[:3])]
    with SlicePipeline(net, slots=2) as pipe:
        for j, (r, m, a) in enumerate(zip(raws, masks, mats)):
            matrix = (a, a.cpu().pin_memory(), a.cpu().numpy())[j % 3]                # the matrix from all three places
            pipe.submit_raw(r.pin_memory(), m, tag=j, crop_shape=crop, n_frames=frames, coil_matrix=matrix)
        got = list(pipe.drain())
        assert pipe.set_builds == 1
    assert [t for t, _ in got] == list(range(len(plan)))
    for j, o in got:
        assert _same(o, want[j]), j
    with SlicePipeline(net, slots=2) as pipe:
        for j in range(3):
            pipe.submit_raw(raws[j].pin_memory(), masks[j], tag=j, crop_shape=crop, n_frames=frames)
        got = list(pipe.drain())
        assert pipe.set_builds >= 2                                                  # a new coil count is a new key without a matrix
    assert [t for t, _ in got] == [0, 1, 2]
    for j, o in got:
        assert _same(o, plain[j]), j


# ------------------------------------------------------------------ 7. submit and submit_raw on one pipeline
@pytest.mark.parametrize("case", ["xpdnet_xt"], indirect=True)
def test_submit_and_submit_raw_alternate(case):
    from cine_hip import frontend as FE
    from cine_hip.pipeline import SlicePipeline
    dev = case.dev
    plan = [("raw", 0), ("raw", 1), ("k", 2), ("k", 3), ("raw", 4), ("k", 5), ("raw", 6), ("raw", 7), ("raw", 8)]
    with SlicePipeline(case.net, slots=2) as pipe:
        for kind, j in plan:
            raw, mask, _ = case.inputs(j, "pinned")
            if kind == "raw":
                pipe.submit_raw(raw, mask, tag=(kind, j), crop_shape=CROP, n_frames=FRAMES)
            else:
                mk = FE.prepare_masked_slice(raw.to(dev), mask.to(dev), CROP, FRAMES, FS, 1e6)
                pipe.submit(mk, mask.to(dev), tag=(kind, j))
        got = list(pipe.drain())
        assert pipe.set_builds == 5                                                  # raw, k-space, raw, k-space, raw: each change of kind
    assert [t for t, _ in got] == plan
    for (kind, j), o in got:
        assert _same(o, case.want[j]), (kind, j)


# ------------------------------------------------------------------ 8. refusals
def test_submit_raw_refusals(dev, monkeypatch):
    import reconstruction.models as M
    from cine_hip import synth
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    raw = torch.from_numpy(_raw(*RAW_SHAPE, seed=1, amp=1e-6)).to(dev)
    mask = _row_mask(FRAMES, CROP[0], seed=1).to(dev)
    kw = dict(crop_shape=CROP, n_frames=FRAMES)
    cine, _, keep = _model("cinenet_3d")
    synth.fill_parameters_(cine, 7, keep=keep)
    with SlicePipeline(cine.to(dev).eval(), slots=1) as pipe:
        with pytest.raises(CineHipError, match="needs sens_maps"):
            pipe.submit_raw(raw, mask, **kw)
    net = M.VarNet_RNN(2, 4, 2, 6)
    synth.fill_parameters_(net, 9, keep=("lambda",))
    pipe = SlicePipeline(net.to(dev).eval(), slots=2)
    with pytest.raises(CineHipError, match="coil_matrix"):
        pipe.submit_raw(raw, mask, coil_matrix=_matrix(2, COILS + 1, 1), **kw)
    with pytest.raises(ValueError, match="Invalid shapes."):
        pipe.submit_raw(raw, mask, crop_shape=(RAW_SHAPE[1] + 2, CROP[1]), n_frames=FRAMES)
    with pytest.raises(CineHipError, match="uint8 or bool"):
        pipe.submit_raw(raw, mask.float(), **kw)
    assert pipe.set_builds == 0 and pipe.pending() == 0
    real = torch.cuda.mem_get_info
    need = 2 * 2 * FRAMES * RAW_SHAPE[1] * RAW_SHAPE[2] * RAW_SHAPE[3] * 8
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (need - 1, real()[1]))
    with pytest.raises(CineHipError, match=f"{need} bytes.*slots=1 would fit"):
        pipe.submit_raw(raw, mask, **kw)
    monkeypatch.setattr(torch.cuda, "mem_get_info", real)
    pipe.submit_raw(raw, mask, **kw)                                                 # the pipeline is usable after every refusal
    assert len(list(pipe.drain())) == 1 and pipe.set_builds >= 1
    pipe.close()
    with pytest.raises(CineHipError, match="after close"):
        pipe.submit_raw(raw, mask, **kw)


# ------------------------------------------------------------------ 9. no side streams, no host synchronisation
@pytest.mark.parametrize("case", ["varnet_rnn"], indirect=True)
def test_submit_raw_creates_no_side_streams_and_does_not_wait_for_the_device(case):
    from cine_hip import ops
    from cine_hip.pipeline import SlicePipeline
    with SlicePipeline(case.net, slots=3) as pipe:
        ins = [case.inputs(j, "pinned")[:2] for j in range(8)]
        for j in range(4):
            pipe.submit_raw(*ins[j], tag=j, crop_shape=CROP, n_frames=FRAMES)
        ids = {s.cuda_stream for s in pipe.streams + [pipe.copy_stream]}
        assert not [k for k in ops._SIDE_STREAMS if k[1] in ids]
        got = dict(pipe.drain())
        torch.cuda.set_sync_debug_mode("error")                                      # warm from here on: a blocking torch call would raise
        try:
            for j in range(4, 8):
                pipe.submit_raw(*ins[j], tag=j, crop_shape=CROP, n_frames=FRAMES)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        got.update(pipe.drain())
    assert sorted(got) == list(range(8))
    assert all(_same(got[j], case.want[j]) for j in range(8))
