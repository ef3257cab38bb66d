"""The packed-weight cache on the device (cine_hip.ops.PackCache behind UnetWeights, MwcnnWeights and the CRNN body): a graph captured
before an in-place weight update keeps its packs, XPDNet's I-step refuses stale activations, a training loop fills every cache once per step."""
import copy

import pytest
import torch

from conftest import rnd, state_dict_from
from cine_hip import ops, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def _small_mwcnn(dev, seed):
    from reconstruction.models.denoisers.mwcnn import MWCNN
    mw = MWCNN(6, 4, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[2, 1], n_first_convs=1, first_conv_n_filters=8, res=False)
    return synth.fill_parameters_(mw, seed, keep=()).to(dev)


def _unet_case(dev):
    from reconstruction.models.denoisers.unet import Unet
    net = synth.fill_parameters_(Unet(5, 2, in_chans=3, out_chans=2), 3, keep=()).to(dev)
    x = rnd(1, 2, 3, 16, 16).to(dev)
    holder = ops.UnetWeights([net])
    return net, holder, (lambda w: [ops.unet2d_forward(x, w)]), (lambda: ops.UnetWeights([net]))


def _mwcnn_case(dev):
    net = _small_mwcnn(dev, 4)
    x = rnd(2, 2, 6, 16, 16).to(dev)
    holder = ops.MwcnnWeights(net)
    return net, holder, (lambda w: [ops.mwcnn_forward(x, w)]), (lambda: ops.MwcnnWeights(net))


def _crnn_case(dev):
    import reconstruction.models as M
    net = synth.fill_parameters_(M.VarNet_RNN(1, 4, 2, 8), 5).to(dev).eval()
    t, h, w = 3, 16, 16
    x = rnd(3, t, 2, h, w).to(dev)

    def run(body_of):
        out, feats = body_of.body(x.view(t, 1, 2, h, w), body_of.zero_state(t, 1, h, w, x), x)
        return [out] + feats
    return net, net, run, (lambda: copy.deepcopy(net))          # a copy of the module starts with empty caches


@pytest.mark.parametrize("case", [_unet_case, _mwcnn_case, _crnn_case], ids=["unet2d", "mwcnn", "crnn_body"])
def test_a_captured_graph_outlives_an_inplace_weight_update(dev, case):
    """A hipGraph captured from a forward pass holds the ADDRESSES of the packed weights.  After an in-place update of the convolution weights
    (the final 1x1 / 3x3 bias of the U-Net and of the MWCNN is read at its own address by design, so the biases stay) an eager call re-packs and
    equals a fresh object's result bit for bit, while the replay of the old graph still computes with the old packs: they are parked until
    ``release_old()``, not handed back to the allocator."""
    net, holder, run, fresh = case(dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        first = [y.clone() for y in run(holder)]                 # eager: fills the caches (and whatever else must exist before a capture)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = run(holder)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() > 1:
                p.mul_(1.25).add_(0.01)
    with torch.cuda.stream(s):
        second = [y.clone() for y in run(holder)]
        scratch = [torch.full_like(y, 7.0) for y in first for _ in range(4)]       # allocations that would reuse freed packs
        want = run(fresh())
    s.synchronize()
    for a, b in zip(second, want):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(first, second))            # the update is visible
    g.replay()
    torch.cuda.synchronize(dev)
    for a, b in zip(captured, first):
        assert torch.equal(a, b)
    del g, scratch
    holder.release_old()
    ops.release_side_streams([s.cuda_stream])       # the stream's handle may be given to a later stream: leave no side stream under it


@pytest.mark.parametrize("h,w,joint", [(16, 16, True), (8, 16, False)])
def test_xpdnet_istep_refuses_a_backward_pass_on_stale_activations(dev, h, w, joint):
    """autograd.xpd_regularise (the path XPDNet training takes), plane sets of one shape (both MWCNNs in the same launches) and of two: an
    in-place update of an MWCNN weight between the forward and the backward pass raises what MwcnnFn raises for the same sequence -- the saved
    activations belong to the old weights.  Host-side, before any launch of the backward pass."""
    from cine_hip import autograd as ag
    n, n_scales, t = 2, 2, 16
    wx, wy = ops.MwcnnWeights(_small_mwcnn(dev, 6)), ops.MwcnnWeights(_small_mwcnn(dev, 7))
    buf, extra = rnd(4, 1, t, 1, h, w, 2 * n).to(dev), rnd(5, 1, t, 1, h, w, 2).to(dev)
    pxf, pyf, _ = ops.xpd_pack(buf, extra, n, n_scales, True)
    assert (pxf.shape[1:] == pyf.shape[1:]) == joint and tuple(pxf.shape[2:]) == (16, 16)

    def stale(loss_of):
        with torch.enable_grad():
            loss = loss_of()
            with torch.no_grad():
                wy.net.first_convs[0].layers[0].weight.add_(1)
            with pytest.raises(RuntimeError, match="modified between the forward and the backward pass.*the saved activations belong to the old weights"):
                loss.backward()
            with torch.no_grad():
                wy.net.first_convs[0].layers[0].weight.sub_(1)
    stale(lambda: ag.xpd_regularise(buf.clone().requires_grad_(True), extra, n, n_scales, True, wx, wy).sum())
    planes = rnd(6, 4, 6, 16, 16).to(dev)
    stale(lambda: ag.mwcnn(planes.clone().requires_grad_(True), wx, wy, 2).sum())          # MwcnnFn: the same error
    with torch.enable_grad():                                                              # and without the update the pass goes through
        x = buf.clone().requires_grad_(True)
        ag.xpd_regularise(x, extra, n, n_scales, True, wx, wy).sum().backward()
    assert torch.isfinite(x.grad).all() and all(p.grad is not None for p in wy.net.parameters())


def _pack_caches(module):
    """Every PackCache reachable from the attributes of the module tree (weight holders and tuples of them included)."""
    found = {}

    def visit(v):
        if isinstance(v, ops.PackCache):
            found[id(v)] = v
        elif isinstance(v, ops._NetWeights):
            visit(v._fwd); visit(v._dgrad)
        elif isinstance(v, (tuple, list)):
            for e in v:
                visit(e)
    for m in module.modules():
        for v in vars(m).values():
            visit(v)
    return list(found.values())


def test_a_training_loop_fills_each_cache_once_per_step(dev, golden):
    """Three optimiser steps of the tiny CRNN-VarNet (3 cascades): the body's training packs are built once per step -- the cascades of a step
    share them -- and no other per-tensor cache is filled more than once per step."""
    import reconstruction.models as M
    from reconstruction.data import transforms
    from reconstruction.utils import SSIMLoss
    g = golden("rnn_grad")
    net = M.VarNet_RNN(3, 4, 2, 6)
    net.load_state_dict(state_dict_from(g, "varnet_rnn::sd::"), strict=True)
    net = net.to(dev).train()
    mk, mask, target = (torch.from_numpy(g[k]).to(dev) for k in ("masked_kspace", "mask", "target"))
    lossf = SSIMLoss().to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=0.0003)
    with torch.enable_grad():
        for step in range(1, 4):
            opt.zero_grad()
            tgt, out = transforms.center_crop_to_smallest(target, net(mk, mask))
            lossf(out.unsqueeze(1), tgt.unsqueeze(1), data_range=tgt.max()).backward()
            opt.step()
            assert net._train_cache.fills == step
            fills = [(c.what, c.fills) for c in _pack_caches(net)]
            assert all(f in (0, step) for _, f in fills), fills
    assert net._body_packs.fills == 0 and net.bcrnn._packs.fills == 0           # the inference caches are not touched by training
