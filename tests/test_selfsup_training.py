"""Self-supervised training through the HIP path: ``output="complex"`` on the six model families, and one training step on held-out samples
(forward on Theta, cine_hip.selfsup.KspaceLoss on Lambda, backward) against float64 autograd of the oracle's blocks, chained here up to the
image in front of the oracle's final magnitude, followed by the loss formula.

Shapes, seeds, masks and pinned ACS rows are those of the model cases of tests/test_general_mask_training.py.  Bars of the end-to-end cases:
what test_hip_grad.py::test_masks_that_vary_along_w_inference_and_training_vs_oracle_float64 holds VarNet and CineNet to -- the output (here
the loss value) within 2e-5, every parameter gradient within 1e-3 of its peak for the best of the three k-spaces and 5e-2 for the worst.
The maps' gradient is checked directly in the CineNet case (its maps are the caller's: a leaf of their own on both sides), at the kernel bar
of tests/test_kspace_loss_kernels.py, 5e-5 of the float64 peak; in the VarNet case the maps are the sensitivity network's output, so their
gradient is checked through that network's parameter gradients."""
import numpy as np
import pytest
import torch

from conftest import rel_err, rnd
from kernel_sweep import same_bits

pytestmark = pytest.mark.gpu
FAMILIES = ["varnet", "cinenet", "xpdnet", "varnet_rnn", "cinenet_rnn", "xpdnet_rnn"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def tiny(family):
    """Constructor, needs maps, (t, c, h, w), acs rows: the tiny models of test_general_mask_training.py."""
    kw = dict(num_cascades=2, sens_chans=4, sens_pools=2, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[1, 1], first_conv_n_filters=8,
              n_primal=2, dynamic_type="XF", weight_sharing=False)
    return {"varnet": (lambda m: m.VarNet(2, 4, 2, 4, 2, "XF"), True, (5, 3, 20, 18), None),
            "cinenet": (lambda m: m.CineNet(2, 3, 4, 2, "XF"), True, (5, 3, 20, 18), None),
            "xpdnet": (lambda m: m.XPDNet(primal_only=True, **kw), False, (4, 3, 24, 20), (9, 6)),
            "varnet_rnn": (lambda m: m.VarNet_RNN(2, 4, 2, 6), False, (4, 3, 24, 20), (9, 6)),
            "cinenet_rnn": (lambda m: m.CineNet_RNN(2, 3, 6), True, (4, 3, 24, 20), None),
            "xpdnet_rnn": (lambda m: m.XPDNet_RNN(2, 4, 2, 6, True, 2, 1), False, (4, 3, 24, 20), (9, 6))}[family]


@pytest.mark.parametrize("family", FAMILIES)
def test_the_complex_output_is_the_image_in_front_of_the_magnitude(dev, family):
    import reconstruction.models as M
    from cine_hip import autograd as ag, ops, synth
    make, needs_sens, (t, c, h, w), acs = tiny(family)
    net = make(M)
    synth.fill_parameters_(net, 17, keep=("lambda",))
    net = net.to(dev)
    g = torch.Generator().manual_seed(6)
    mask = (torch.rand(1, t, 1, h, w, 1, generator=g) < 0.4).to(torch.uint8)
    mask[:, :, :, 9:15, w // 2 - 4:w // 2 + 4] = 1
    sens = rnd(32, 1, 1, c, h, w, 2)
    sens = (sens / sens.pow(2).sum(dim=(2, 5), keepdim=True).sqrt()).to(dev)
    k = (rnd(34, 1, t, c, h, w, 2) * mask).to(dev)
    args, kw = ((k, mask.to(dev), sens), {}) if needs_sens else ((k, mask.to(dev)), {"acs": acs})
    net.train()
    with torch.enable_grad():
        default = net(*args, **kw)
        named = net(*args, **kw, output="magnitude")
        cplx = net(*args, **kw, output="complex")
        assert default.requires_grad and cplx.requires_grad
        assert cplx.shape == (1, t, h, w, 2) and default.shape == (1, t, h, w)
        assert same_bits(default.detach(), named.detach())
        assert same_bits(ag.AbsFn.apply(cplx).detach(), default.detach())
    net.eval()
    default, named, cplx = net(*args, **kw), net(*args, **kw, output="magnitude"), net(*args, **kw, output="complex")
    assert same_bits(default, named) and cplx.shape == (1, t, h, w, 2) and not cplx.requires_grad
    e = float((ops.complex_abs(cplx.contiguous()) - default).abs().max() / default.abs().max())
    print(f"{family}: inference, |complex output| against the default output {e:.3e} of the peak (bar 1e-6)")
    assert e < 1e-6
    with pytest.raises(ValueError):
        net(*args, **kw, output="phase")


def loss_formula(u, y, lam):
    r, v = lam * (u - y), lam * y
    return 0.5 * (r * r).sum().sqrt() / (v * v).sum().sqrt() + 0.5 * r.abs().sum() / v.abs().sum()


def oracle_image(family, ref, k, theta, sens, acs):
    """The oracle's blocks chained up to the image in front of its final magnitude (varnet.py:143-150, cinenet.py:64-72) -> (image, maps)."""
    from oracle import complex_ops as co, centered_fft as cf
    if family == "varnet":
        maps = ref.sens_net(k, theta)
        kk = k.clone()
        for cascade in ref.cascades:
            kk = cascade(kk, k, theta, maps)
        return co.complex_mul(cf.ifft2c(kk), co.complex_conj(maps)).sum(dim=2), maps
    image = type(ref.cascades[0]).sens_reduce(k, sens)
    first = image.clone()
    for cascade in ref.cascades:
        image = cascade(image, first, theta, sens)
    return image.squeeze(2), sens


@pytest.mark.parametrize("family", ["varnet", "cinenet"])
def test_a_training_step_on_held_out_samples_vs_oracle_float64(dev, family, monkeypatch):
    import reconstruction.models as M
    from cine_hip import synth
    from cine_hip.selfsup import KspaceLoss, split_mask
    from oracle import varnet_ref as V, cinenet_ref as C
    t, c, h, w = 5, 3, 20, 18
    make, mod = {"varnet": (lambda m: m.VarNet(2, 4, 2, 4, 2, "XF"), V), "cinenet": (lambda m: m.CineNet(2, 3, 4, 2, "XF"), C)}[family]
    net = make(M)
    synth.fill_parameters_(net, 13, keep=("lambda",))
    ref = make(mod).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()}, strict=True)
    net, ref = net.to(dev).train(), ref.train()
    acs = (h // 2 - 2, 4)                                                            # the rows of the mask's centre box, pinned on both sides
    monkeypatch.setattr(V.SensitivityModel, "acs_window", staticmethod(lambda mask: acs))
    g = torch.Generator().manual_seed(5)
    omega = (torch.rand(1, t, 1, h, w, 1, generator=g) < 0.4).to(torch.uint8)
    omega[:, :, :, h // 2 - 2:h // 2 + 2, w // 2 - 3:w // 2 + 3] = 1
    theta, lam = split_mask(omega, rho=0.4, acs=4, rng=np.random.default_rng(5))
    assert int(lam.sum()) > 0 and int((theta & lam).sum()) == 0
    sens = rnd(32, 1, 1, c, h, w, 2)
    sens = sens / sens.pow(2).sum(dim=(2, 5), keepdim=True).sqrt()
    crit = KspaceLoss()
    best, worst, loss_errs, maps_errs = {}, {}, [], []
    for seed in (31, 41, 51):
        k_theta = rnd(seed, 1, t, c, h, w, 2) * theta
        # float64: the oracle on Theta, then the measurement on Lambda without a kink: y = u + d, |d| in [0.51, 1.5] per real component
        ref.zero_grad()
        with torch.enable_grad():
            maps_leaf = sens.double().requires_grad_(True)                           # CineNet: the maps of the loss, a leaf of their own
            image64, maps64 = oracle_image(family, ref, k_theta.double(), theta, sens.double(), acs)
            u64 = V.VarNetBlock.sens_expand(image64.unsqueeze(2), maps64 if family == "varnet" else maps_leaf)
            gd = torch.Generator().manual_seed(seed + 1)
            d = (0.51 + 0.99 * torch.rand(u64.shape, generator=gd, dtype=torch.float64)) * \
                torch.where(torch.rand(u64.shape, generator=gd) < 0.5, -1.0, 1.0).double()
            y = (k_theta.double() + lam * (u64.detach() + d)).float()                # measured on Omega = Theta + Lambda
            r64 = (u64.detach() - y.double())[lam.bool().expand_as(u64)]
            assert float(r64.abs().min()) >= 0.5, "the Lambda residual has a component within 0.5 of zero"
            l64 = loss_formula(u64, y.double(), lam.double())
            l64.backward()
        # the HIP path
        net.zero_grad()
        maps32 = sens.to(dev).requires_grad_(True)
        with torch.enable_grad():
            if family == "varnet":
                image = net(k_theta.to(dev), theta.to(dev), acs=acs, output="complex")
                # the maps of the loss are the sensitivity network's (the oracle's chain above): run it again, as a training loop would keep them
                maps = net.sens_net(k_theta.to(dev), theta.to(dev), acs)
            else:
                image = net(k_theta.to(dev), theta.to(dev), sens.to(dev), output="complex")
                maps = maps32
            l32 = crit(image, maps, y.to(dev), lam.to(dev))
            l32.backward()
        assert l32.shape == () and l32.dtype == torch.float32
        loss_errs.append(abs(float(l32) - float(l64)) / abs(float(l64)))
        if family == "cinenet":
            maps_errs.append(rel_err(maps32.grad.cpu(), maps_leaf.grad))
        want = {k: p for k, p in ref.named_parameters() if p.grad is not None}
        assert len(want) >= 10
        for k, p in net.named_parameters():
            if k not in want:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
                continue
            e = rel_err(p.grad.cpu(), want[k].grad.float())
            best[k] = min(best.get(k, 1e9), e); worst[k] = max(worst.get(k, 0.0), e)
    print(f"{family}: loss {max(loss_errs):.3e} relative (bar 2e-5); parameter gradients: worst best-of-three {max(best.values()):.3e} (bar 1e-3), "
          f"worst {max(worst.values()):.3e} (bar 5e-2)" + (f"; maps' gradient {max(maps_errs):.3e} of the peak (bar 5e-5)" if maps_errs else ""))
    assert max(loss_errs) < 2e-5, loss_errs
    bad = {k: (best[k], worst[k]) for k in best if best[k] > 1e-3 or worst[k] > 5e-2}
    assert not bad, bad
    assert all(e < 5e-5 for e in maps_errs), maps_errs              # the kernel bar (RESID): the maps are a leaf of the loss alone here


def test_the_loss_saves_its_inputs_and_a_small_record(dev):
    from cine_hip import ops
    from cine_hip.selfsup import kspace_loss
    b, t, c, h, w = 1, 3, 4, 24, 20
    image = rnd(1, b, t, h, w, 2).to(dev).requires_grad_(True)
    sens = rnd(2, b, 1, c, h, w, 2).to(dev).requires_grad_(True)
    y = rnd(3, b, t, c, h, w, 2).to(dev)
    lam = ops.as_mask_u8((torch.rand(b, t, 1, h, w, 1, generator=torch.Generator().manual_seed(4)) < 0.4).to(dev), y)
    inputs = {v.data_ptr() for v in (image, sens, y, lam)}
    saved = []
    with torch.enable_grad(), torch.autograd.graph.saved_tensors_hooks(lambda x: saved.append(x) or x, lambda x: x):
        loss = kspace_loss(image, sens, y, lam)
    extra = sum(v.numel() * v.element_size() for v in saved if v.data_ptr() not in inputs)
    print(f"KspaceLossFn saves {len(saved)} tensors, {extra} bytes beside its inputs (bar 4096)")
    assert len(saved) >= 4 and extra <= 4096
    with torch.enable_grad():
        loss.backward()
    assert image.grad.shape == image.shape and sens.grad.shape == sens.shape
    assert bool(torch.isfinite(image.grad).all()) and bool(torch.isfinite(sens.grad).all())
