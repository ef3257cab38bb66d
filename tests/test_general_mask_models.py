"""Sampling masks that vary along w in inference: every model family on the image-space operator with both line passes
(ops.GENERAL_MASK_FUSED, cine_image_dc_general / cine_normal_op_general), the front-end and SlicePipeline.submit_raw with such masks.

Per family, on the tiny models and shapes of test_masks_that_vary_along_w_* (test_hip_grad.py), under no_grad:
  * counter 15 of cine_diag_counter (column passes that weight by a mask plane) moves with the flag on and stays still with it off;
  * the output is within the existing bars (2e-5 VarNet / CineNet, 5e-5 XPDNet and the CRNN models) of the oracle's float64 forward, either way;
  * a general mask whose columns are all equal reproduces the row-mask output within 2e-5;
  * one captured graph, replayed with a second mask of different content, gives the eager result for that content bit for bit."""
import numpy as np
import pytest
import torch

from conftest import rel_err, rnd

pytestmark = pytest.mark.gpu
D_MASK2D = 15
ACS = (9, 6)                                     # rows [9, 15): what the sens-nets keep; pinned on both sides
XKW = dict(num_cascades=2, sens_chans=4, sens_pools=2, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[1, 1], first_conv_n_filters=8,
           n_primal=2, dynamic_type="XF", weight_sharing=False)
A, B = (5, 3, 20, 18), (4, 3, 24, 20)            # (t, c, h, w)
# family -> (constructor, oracle module, takes sens_maps, shape, bar against float64)
FAMILIES = {
    "varnet_XF": (lambda m: m.VarNet(2, 4, 2, 4, 2, "XF"), "varnet_ref", True, A, 2e-5),
    "varnet_2D": (lambda m: m.VarNet(2, 4, 2, 4, 2, "2D"), "varnet_ref", True, A, 2e-5),
    "varnet_3D": (lambda m: m.VarNet(2, 4, 2, 4, 2, "3D"), "varnet_ref", True, A, 2e-5),
    "cinenet_XF": (lambda m: m.CineNet(2, 3, 4, 2, "XF"), "cinenet_ref", True, A, 2e-5),
    "cinenet_3D": (lambda m: m.CineNet(2, 2, 4, 2, "3D"), "cinenet_ref", True, A, 2e-5),
    "xpdnet": (lambda m: m.XPDNet(primal_only=True, **XKW), "xpdnet_ref", False, B, 5e-5),
    "varnet_rnn": (lambda m: m.VarNet_RNN(2, 4, 2, 6), "recurrent_ref", False, B, 5e-5),
    "cinenet_rnn": (lambda m: m.CineNet_RNN(2, 3, 6), "recurrent_ref", True, B, 5e-5),
    "xpdnet_rnn": (lambda m: m.XPDNet_RNN(2, 4, 2, 6, True, 2, 1), "recurrent_ref", False, B, 5e-5),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def general_mask(t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(1, t, 1, h, w, 1, generator=g) < 0.4).to(torch.uint8)
    m[:, :, :, 9:15, w // 2 - 4:w // 2 + 4] = 1
    return m


def counter(reset=1):
    from cine_hip._lib import lib
    return lib().cine_diag_counter(D_MASK2D, reset)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_family_on_the_fused_operator(dev, family, monkeypatch):
    import importlib
    import reconstruction.models as M
    from cine_hip import ops, synth
    from cine_hip.pipeline import pipeline_streams
    from oracle import recurrent_ref as R, varnet_ref as V, xpdnet_ref as X
    make, refname, takes_sens, (t, c, h, w), bar = FAMILIES[family]
    net = make(M)
    synth.fill_parameters_(net, 17, keep=("lambda",))
    ref = make(importlib.import_module("oracle." + refname)).double().eval()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()}, strict=True)
    net = net.to(dev).eval()
    for mod in (V, X, R):                          # the sens-nets read their window off a 1-D mask: pinned to the rows the HIP side is given
        for name in dir(mod):
            cls = getattr(mod, name)
            if isinstance(cls, type) and hasattr(cls, "acs_window"):
                monkeypatch.setattr(cls, "acs_window", staticmethod(lambda mask: ACS))
    sens = rnd(32, 1, 1, c, h, w, 2)
    sens = sens / sens.pow(2).sum(dim=(2, 5), keepdim=True).sqrt()
    masks = [general_mask(t, h, w, 6), general_mask(t, h, w, 7)]
    assert not torch.equal(masks[0], masks[1])
    mks = [rnd(34 + i, 1, t, c, h, w, 2) * m for i, m in enumerate(masks)]

    sens_d = sens.to(dev)

    def hip(mk, mask):
        with torch.no_grad(), ops.branches(1):
            return net(mk, mask, sens_d) if takes_sens else net(mk, mask, acs=ACS)

    with torch.no_grad():
        a64 = (mks[0].double(), masks[0])
        want = (ref(*a64, sens.double()) if takes_sens else ref(*a64)).float()
    # flag on / off: which path ran, and both against float64
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", True)
    counter()
    on = hip(mks[0].to(dev), masks[0].to(dev)).cpu()
    assert counter() > 0, "the flag is on and no column pass weighted by a mask plane"
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", False)
    off = hip(mks[0].to(dev), masks[0].to(dev)).cpu()
    assert counter() == 0, "the flag is off and the mask-plane column pass ran"
    e_on, e_off = rel_err(on, want), rel_err(off, want)
    print(f"{family}: fused {e_on:.3e}, literal {e_off:.3e} of the float64 peak (bar {bar:.0e})")
    assert e_on < bar and e_off < bar, (e_on, e_off)
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", True)
    # columns all equal: the row-mask kernels' result
    row = masks[0][:, :, :, :, w // 2:w // 2 + 1, :].contiguous()              # (1, t, 1, h, 1, 1)
    assert 0 < int(row.sum()) < row.numel()
    mk_r = (rnd(40, 1, t, c, h, w, 2) * row).to(dev)
    o_row = hip(mk_r, row.to(dev))
    assert counter() == 0
    o_gen = hip(mk_r, row.expand(1, t, 1, h, w, 1).contiguous().to(dev))
    assert counter() > 0
    e = rel_err(o_gen.cpu(), o_row.cpu())
    print(f"{family}: equal columns against the row mask {e:.3e}")
    assert e < 2e-5, e
    # one graph, two masks
    eager = [hip(mk.to(dev), m.to(dev)).clone() for mk, m in zip(mks, masks)]
    assert not torch.equal(eager[0], eager[1])
    smk, smask = mks[0].to(dev).clone(), masks[0].to(dev).clone()
    st = pipeline_streams(dev, 1)[0][0]                  # a pipeline stream, as SlicePipeline captures (and no stream of this test's own)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        hip(smk, smask)                            # this stream's caches, outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        gout = hip(smk, smask)
    for i in (1, 0, 1):
        smk.copy_(mks[i]); smask.copy_(masks[i])
        gout.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, eager[i]), (family, i, float((gout - eager[i]).abs().max()))


# ------------------------------------------------------------------ front-end and pipeline
FS = (0.7, 0.0, 0.3, 0.3)
RAW_SHAPE, CROP, FRAMES, COILS = (7, 30, 28, 3), (24, 20), 5, 3


def _raw(t, nx, ny, c, seed, amp=1e-6):
    rs = np.random.RandomState(seed)
    x, y = np.arange(nx)[:, None] - nx // 2, np.arange(ny)[None, :] - ny // 2
    wgt = np.exp(-(x * x / (2.0 * (nx / 8.0) ** 2) + y * y / (2.0 * (ny / 8.0) ** 2))) + 0.02
    z = rs.standard_normal((t, nx, ny, c)) + 1j * rs.standard_normal((t, nx, ny, c))
    return torch.from_numpy((amp * z * wgt[None, :, :, None]).astype(np.complex64))


def _mask2d(t, X, Y, seed):
    m = (torch.rand(1, t, 1, X, Y, 1, generator=torch.Generator().manual_seed(seed)) < 0.35).to(torch.uint8)
    m[:, :, :, X // 2 - 2:X // 2 + 2, :Y * 3 // 4] = 1
    m[..., Y * 3 // 4:, :] = 0                   # a readout cut-off
    return m


@pytest.mark.parametrize("shape,crop,n", [((4, 30, 28, 3), (24, 20), 3), ((3, 416, 24, 2), (21, 17), 3)])
def test_prepare_masked_slice_takes_masks_that_vary_along_w(dev, shape, crop, n):
    from cine_hip import frontend as FE, ops
    raw = _raw(*shape, seed=3).to(dev)
    k, _ = FE.prepare_slice(raw, crop, n, FS, 1e6)
    T = min(n, shape[0])
    for tt in (T, 1):
        m2d = _mask2d(tt, crop[0], crop[1], 11).to(dev)
        full = m2d.expand(1, T, 1, crop[0], crop[1], 1).contiguous()
        want = ops.apply_mask(k, full[0])[None]
        assert torch.equal(want, (k * full[0] + 0.0)[None])
        got = FE.prepare_masked_slice(raw, m2d, crop, n, FS, 1e6)
        assert got.shape == want.shape and torch.equal(got, want), (shape, tt)
        out = torch.full_like(want, float("nan"))
        assert FE.prepare_masked_slice(raw, m2d.bool(), crop, n, FS, 1e6, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError, match="is not a row mask"):
        FE.prepare_masked_slice(raw, torch.ones(1, T, 1, crop[0], crop[1] - 1, 1, dtype=torch.uint8, device=dev), crop, n, FS, 1e6)


def test_submit_raw_with_masks_that_vary_along_w(dev):
    import reconstruction.models as M
    from cine_hip import frontend as FE, synth
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    net = M.CineNet(2, 3, 4, 2, "3D")
    synth.fill_parameters_(net, 7, keep=("lambda",))
    net = net.to(dev).eval()
    raws = [_raw(*RAW_SHAPE, seed=50 + j).to(dev) for j in range(3)]
    masks = [_mask2d(FRAMES, CROP[0], CROP[1], 20 + j).to(dev) for j in range(3)]
    sens = [synth.make_cine_slice(FRAMES, COILS, CROP[0], CROP[1], accel=4, center_lines=4, seed=70 + j)["sens_maps"].contiguous().to(dev)
            for j in range(3)]
    counter()
    from cine_hip import ops
    with torch.no_grad(), ops.branches(1):
        want = [net(FE.prepare_masked_slice(raws[j], masks[j], CROP, FRAMES, FS, 1e6), masks[j], sens[j]).clone() for j in range(3)]
    assert counter() > 0 and not torch.equal(want[0], want[1])
    got = {}
    with SlicePipeline(net, slots=2) as pipe:
        for j in range(3):
            pipe.submit_raw(raws[j], masks[j], sens[j], tag=j, crop_shape=CROP, n_frames=FRAMES)
            got.update(pipe.results())
        got.update(pipe.drain())
        assert pipe.set_builds == 1
    for j in range(3):
        assert torch.equal(got[j], want[j]), (j, float((got[j] - want[j]).abs().max()))
    vn = M.VarNet(2, 4, 2, 4, 2, "XF")
    synth.fill_parameters_(vn, 1)
    with SlicePipeline(vn.to(dev).eval(), slots=1) as pipe:
        with pytest.raises(CineHipError, match="varies along w"):
            pipe.submit_raw(raws[0], masks[0], crop_shape=CROP, n_frames=FRAMES)          # the sens-net's ACS window needs a row mask
