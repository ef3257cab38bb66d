"""cine_hip.dc.Acquisition: every data-consistency operator of the model forwards, in each mask layout (row, varies along w) and mode
(image-space operator, literal k-space chain with ops.GENERAL_MASK_FUSED off, training), against the float64 formulas of the reference
written with the oracle's sens_expand / sens_reduce and the literal DC lines (as test_image_dc_vs_oracle does for the row mask).

Bars, of the float64 peak: 2e-5 for the soft-DC forms and the single coil operators they are made of, 5e-5 for the residual forms --
the bars tests/test_general_mask_models.py states for the families built on them.  Shapes: the two tiny ones of those tests, and
(2, 2, 200, 16), the smallest at which the h == 200 one-kernel column pass and the tile-packed maps are in play."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, rnd

pytestmark = pytest.mark.gpu
D_MASK2D = 15
SOFT, RESID = 2e-5, 5e-5
LAM = 0.5413
SHAPES = [(5, 3, 20, 18), (4, 3, 24, 20), (2, 2, 200, 16)]          # (t, c, h, w)
CASES = [(b,) + s for s in SHAPES for b in (1, 2)]
MODES = ("fused", "literal", "train")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def counter(reset=1):
    from cine_hip._lib import lib
    return lib().cine_diag_counter(D_MASK2D, reset)


def make_mask(layout, b, t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(b, t, 1, h, 1 if layout == "row" else w, 1, generator=g) < 0.4).to(torch.uint8)
    m[:, :, :, h // 2 - 2:h // 2 + 2] = 1
    return m


_REF = {}


def reference(layout, b, t, c, h, w):
    """Inputs (float32) and the float64 formulas on them, computed once per case and shared by the modes."""
    key = (layout, b, t, c, h, w)
    if key not in _REF:
        from oracle import varnet_ref as V
        expand, reduce = V.VarNetBlock.sens_expand, V.VarNetBlock.sens_reduce
        x = dict(img=rnd(1, b, t, 1, h, w, 2), sens=rnd(2, b, 1, c, h, w, 2), kref=rnd(3, b, t, c, h, w, 2), k0=rnd(4, b, t, c, h, w, 2),
                 mask=make_mask(layout, b, t, h, w, 5), wgt=rnd(6, b, t, 1, h, w, 2))
        img, sens, kref, k0, mask = (x[k].double() if k != "mask" else x[k] for k in ("img", "sens", "kref", "k0", "mask"))
        img.requires_grad_(True)
        v = F.softplus(torch.tensor([LAM], dtype=torch.float64))
        with torch.enable_grad():
            kth = expand(img, sens)
            soft = reduce((1 - mask) * kth + mask * (kth + v * kref) / (1 + v), sens)            # reference varnet.py:281-282, then :187-194
            resid = reduce((kth * mask - kref) * mask + 0.0, sens)                               # A^H M (M A x0 - k_ref), xpdnet.py:128-131, 161-167
            g_soft, = torch.autograd.grad((soft * x["wgt"].double()).sum(), img, retain_graph=True)
            g_resid, = torch.autograd.grad((resid * x["wgt"].double()).sum(), img)
        want = dict(image=reduce(kref, sens), zf=reduce(kref * mask, sens), soft=soft.detach(), resid=resid.detach(),
                    mag=soft.detach().squeeze(2).pow(2).sum(-1).sqrt(), fwd=(kth * mask + 0.0).detach(), bwd=reduce(k0 * mask + 0.0, sens),
                    g_soft=g_soft, g_resid=g_resid)
        _REF[key] = (x, want)
    return _REF[key]


def run_all(acq, img, k0, lam, magnitude=True):
    """Every method of the object once: name -> output."""
    out = dict(image=acq.image(), soft=acq.soft_dc(img, lam), resid=acq.residual_backward(img), fwd=acq.forward_masked(img),
               bwd=acq.backward_masked(k0.clone()))
    if magnitude:
        out["mag"] = acq.soft_dc(img, lam, magnitude=True)
    if acq.fused or (acq.train and acq.row):
        out["zf"] = acq.zero_filled()
    return out


BARS = dict(image=SOFT, zf=SOFT, soft=SOFT, mag=SOFT, fwd=SOFT, bwd=SOFT, resid=RESID, g_soft=SOFT, g_resid=RESID)


@pytest.mark.parametrize("layout", ["row", "general"])
@pytest.mark.parametrize("b,t,c,h,w", CASES)
def test_every_method_in_every_mode_vs_float64(dev, monkeypatch, b, t, c, h, w, layout):
    from cine_hip import ops
    from cine_hip._lib import lib
    from cine_hip.dc import Acquisition
    x, want = reference(layout, b, t, c, h, w)
    d = {k: v.to(dev) for k, v in x.items()}
    lam = torch.tensor([LAM], device=dev)
    mask = ops.as_mask_u8(d["mask"], d["kref"])
    assert mask is d["mask"]
    for mode in MODES:
        monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", mode != "literal")
        counter()
        if mode == "train":
            img = d["img"].clone().requires_grad_(True)
            with torch.enable_grad():
                acq = Acquisition(d["kref"], mask, d["sens"], train=True)
                got = run_all(acq, img, d["k0"], lam, magnitude=False)
                got["g_soft"], = torch.autograd.grad((got["soft"] * d["wgt"]).sum(), img)
                got["g_resid"], = torch.autograd.grad((got["resid"] * d["wgt"]).sum(), img)
            assert not acq.fused and acq.tiled is None
        else:
            acq = Acquisition(d["kref"], mask, d["sens"])
            assert acq.fused == (layout == "row" or mode == "fused") and acq.row == (layout == "row")
            got = run_all(acq, d["img"], d["k0"], lam)
            # what is constant over the cascades is made once
            if acq.fused:
                assert acq.zero_filled() is got["zf"] and acq.zero_filled() is acq.zero_filled()
            packs = layout == "row" and lib().cine_sens_tile_floats(b, c, h, w) > 0
            assert (acq.tiled is not None) == packs and acq.tiled is acq.tiled
            assert (h == 200) <= (layout != "row" or packs)                 # the third shape is there for the tile-packed maps
        moved = counter()
        if layout == "general":
            assert (moved > 0) == (mode == "fused"), (mode, moved)          # flag off, and the training forms: no mask-plane column pass
        else:
            assert moved == 0
        for name, g in got.items():
            e = rel_err(g.detach().cpu(), want[name])
            print(f"b={b} {(t, c, h, w)} {layout} {mode} {name}: {e:.3e} of the float64 peak (bar {BARS[name]:.0e})")
            assert g.shape == want[name].shape and e < BARS[name], (mode, name, e)
        for k in ("img", "kref", "k0", "sens"):
            assert torch.equal(d[k].cpu(), x[k]), (mode, k)                # the caller's tensors are untouched


@pytest.mark.parametrize("layout,fused", [("row", True), ("general", True), ("general", False)])
def test_inference_methods_capture_and_replay_with_another_mask(dev, monkeypatch, layout, fused):
    from cine_hip import ops
    from cine_hip.dc import Acquisition
    from cine_hip.pipeline import pipeline_streams
    b, (t, c, h, w) = 1, SHAPES[2]
    x, _ = reference(layout, b, t, c, h, w)
    masks = [x["mask"].to(dev), make_mask(layout, b, t, h, w, 9).to(dev)]
    assert not torch.equal(masks[0], masks[1])
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", fused)
    s = {k: x[k].to(dev).clone() for k in ("img", "sens", "kref", "k0", "mask")}
    lam = torch.tensor([LAM], device=dev)

    def forward():
        return run_all(Acquisition(s["kref"], s["mask"], s["sens"]), s["img"], s["k0"], lam)
    eager = []
    for m in masks:
        s["mask"].copy_(m)
        eager.append({k: v.clone() for k, v in forward().items()})
    assert not torch.equal(eager[0]["soft"], eager[1]["soft"])
    st = pipeline_streams(dev, 1)[0][0]                  # a pipeline stream, as SlicePipeline captures
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        forward()                                        # this stream's caches, outside capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st):
        gout = forward()
    for i in (1, 0, 1):
        s["mask"].copy_(masks[i])
        for v in gout.values():
            v.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for k, v in gout.items():
            assert torch.equal(v, eager[i][k]), (layout, fused, i, k, float((v - eager[i][k]).abs().max()))
