"""Training on the image-space data consistency for sampling masks that vary along w: ops.GENERAL_MASK_FUSED_TRAIN (with ops.GENERAL_MASK_FUSED)
sends a training step through ImageDcFn / ImageDcFixedFn / CoilReduceFn with the mask plane / ConjGradFn on cine_normal_op_general instead of
the literal chain on the coil-wise k-space.

a. the autograd functions and cine_hip.dc.Acquisition(train=True) against float64 autograd of the literal composition.  Bars, of the float64
   peak: SOFT = 2e-5 for the soft-DC forms, RESID = 5e-5 for the (1, 0, -1) weights (the bars test_dc_operator.py holds the same methods to);
   lambda: LAM_REL = 1e-4 relative, the bar test_hip_grad.py::test_image_dc_backward_vs_oracle holds lambda_reg's gradient to (its TOL).
b. the nine model families of test_hip_grad.py's two test_masks_that_vary_along_w_* tests -- their shapes, seeds, masks and pinned ACS rows --
   in train() with both switches on against the oracle's float64 autograd, at the bars those tests hold the literal path to, with counter 15 of
   cine_diag_counter as the proof of the route in the forward and in the backward pass.
c. the peak memory of one training step, switch off against switch on."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, rnd

pytestmark = pytest.mark.gpu
D_MASK2D = 15
SOFT, RESID = 2e-5, 5e-5
LAM_REL = 1e-4
LAM = 0.5413
FN_SHAPES = [(1, 3, 3, 24, 20), (2, 2, 9, 200, 12)]          # (b, t, c, h, w): mixed radix; the h == 200 one-kernel column pass with 9 coils


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def counter(reset=1):
    from cine_hip._lib import lib
    return lib().cine_diag_counter(D_MASK2D, reset)


def switches(monkeypatch, train_on):
    from cine_hip import ops
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED", True)
    monkeypatch.setattr(ops, "GENERAL_MASK_FUSED_TRAIN", train_on)


def make_mask(b, t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(b, t, 1, h, w, 1, generator=g) < 0.4).to(torch.uint8)
    m[:, :, :, h // 2 - 2:h // 2 + 2] = 1
    return m


# ------------------------------------------------------------------ a. the functions and the object
_REF = {}


def reference(b, t, c, h, w):
    """Inputs (float32) and float64 autograd of the literal composition on them, once per shape: the operators as functions of the image, the
    maps, the zero-filled term (a leaf of its own) and lambda, and Acquisition's methods as test_dc_operator.py states them."""
    key = (b, t, c, h, w)
    if key in _REF:
        return _REF[key]
    from oracle import varnet_ref as V
    expand, reduce = V.VarNetBlock.sens_expand, V.VarNetBlock.sens_reduce
    x = dict(img=rnd(1, b, t, 1, h, w, 2), sens=rnd(2, b, 1, c, h, w, 2), kref=rnd(3, b, t, c, h, w, 2), k0=rnd(4, b, t, c, h, w, 2),
             mask=make_mask(b, t, h, w, 5), wgt=rnd(6, b, t, 1, h, w, 2), zf=rnd(7, b, t, 1, h, w, 2))
    mask, wgt, kref, k0 = x["mask"], x["wgt"].double(), x["kref"].double(), x["k0"].double()
    want = {}
    with torch.enable_grad():
        img, sens, zf = (x[k].double().requires_grad_(True) for k in ("img", "sens", "zf"))
        lam = torch.tensor([LAM], dtype=torch.float64, requires_grad=True)
        v = F.softplus(lam)
        kth = expand(img, sens)
        # ImageDcFn with zf as its own input: reduce of the DC line's model term (varnet.py:281-282 without the measurement) + v / (1 + v) zf
        soft = reduce((1 - mask) * kth + mask * kth / (1 + v), sens) + v / (1 + v) * zf
        fixed = reduce(kth * mask + 0.0, sens) - zf                                                # ImageDcFixedFn (1, 0, -1)
        want["fn_soft"], want["fn_fixed"] = soft.detach(), fixed.detach()
        for name, out, wrt in (("fn_soft", soft, (img, sens, zf, lam)), ("fn_fixed", fixed, (img, sens, zf))):
            for k, g in zip(("img", "sens", "zf", "lam"), torch.autograd.grad((out * wgt).sum(), wrt, retain_graph=True)):
                want[f"{name}:{k}"] = g
        # the object's methods (test_dc_operator.py's formulas)
        v0 = v.detach()
        a_soft = reduce((1 - mask) * kth + mask * (kth + v0 * kref) / (1 + v0), sens)
        a_resid = reduce((kth * mask - kref) * mask + 0.0, sens)
        want["g_soft"], = torch.autograd.grad((a_soft * wgt).sum(), img, retain_graph=True)
        want["g_resid"], = torch.autograd.grad((a_resid * wgt).sum(), img, retain_graph=True)
        sd = sens.detach()
        want.update(image=reduce(kref, sd), zf=reduce(kref * mask, sd), soft=a_soft.detach(), resid=a_resid.detach(),
                    fwd=(kth * mask + 0.0).detach(), bwd=reduce(k0 * mask + 0.0, sd))
    _REF[key] = (x, want)
    return _REF[key]


@pytest.mark.parametrize("b,t,c,h,w", FN_SHAPES)
def test_image_dc_functions_with_a_general_mask_vs_float64_autograd(dev, b, t, c, h, w):
    """The functions themselves: they dispatch on the mask's layout, whatever the switches say."""
    from cine_hip import autograd as ag
    x, want = reference(b, t, c, h, w)
    d = {k: v.to(dev) for k, v in x.items()}
    for name, bar in (("fn_soft", SOFT), ("fn_fixed", RESID)):
        img, sens, zf = (d[k].clone().requires_grad_(True) for k in ("img", "sens", "zf"))
        lam = torch.tensor([LAM], device=dev, requires_grad=True)
        counter()
        with torch.enable_grad():
            out = ag.ImageDcFn.apply(img, sens, zf, d["mask"], lam) if name == "fn_soft" else \
                ag.ImageDcFixedFn.apply(img, sens, zf, d["mask"], 1.0, 0.0, -1.0)
            assert counter() > 0
            (out * d["wgt"]).sum().backward()
        # image gradient: one operator; maps: the new entry point, one pass per operand; lambda (soft only): one more operator
        assert counter() >= 3
        errs = {"out": rel_err(out.detach().cpu(), want[name])}
        for k, leaf in (("img", img), ("sens", sens), ("zf", zf)):
            assert leaf.grad.shape == want[f"{name}:{k}"].shape
            errs[k] = rel_err(leaf.grad.cpu(), want[f"{name}:{k}"])
        print(f"{name} {(b, t, c, h, w)}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f" of the float64 peak (bar {bar:.0e})")
        if name == "fn_soft":
            e = rel_err(lam.grad.cpu(), want["fn_soft:lam"])
            print(f"{name} {(b, t, c, h, w)}: lambda {e:.3e} relative (bar {LAM_REL:.0e})")
            assert e < LAM_REL, e
        assert all(e < bar for e in errs.values()), (name, errs)


BARS = dict(image=SOFT, zf=SOFT, soft=SOFT, fwd=SOFT, bwd=SOFT, resid=RESID, g_soft=SOFT, g_resid=RESID)


def run_all(acq, img, k0, lam):
    """Every method of the object once (test_dc_operator.py's run_all, training form): name -> output."""
    out = dict(image=acq.image(), soft=acq.soft_dc(img, lam), resid=acq.residual_backward(img), fwd=acq.forward_masked(img),
               bwd=acq.backward_masked(k0.clone()))
    if acq.fused or (acq.train and acq.row):
        out["zf"] = acq.zero_filled()
    return out


@pytest.mark.parametrize("b,t,c,h,w", FN_SHAPES)
def test_a_training_acquisition_with_both_switches_on_vs_float64(dev, monkeypatch, b, t, c, h, w):
    from cine_hip import ops
    from cine_hip.dc import Acquisition
    x, want = reference(b, t, c, h, w)
    d = {k: v.to(dev) for k, v in x.items()}
    lam = torch.tensor([LAM], device=dev)
    mask = ops.as_mask_u8(d["mask"], d["kref"])
    assert mask is d["mask"]
    switches(monkeypatch, True)
    counter()
    img = d["img"].clone().requires_grad_(True)
    with torch.enable_grad():
        acq = Acquisition(d["kref"], mask, d["sens"], train=True)
        got = run_all(acq, img, d["k0"], lam)
        forward_moved = counter()
        got["g_soft"], = torch.autograd.grad((got["soft"] * d["wgt"]).sum(), img)
        got["g_resid"], = torch.autograd.grad((got["resid"] * d["wgt"]).sum(), img)
    assert acq.fused and acq.train and not acq.row and acq.tiled is None and "zf" in got
    assert forward_moved >= 2 and counter() >= 2, "the image-space operators did not run"
    for name, g in got.items():
        e = rel_err(g.detach().cpu(), want[name])
        print(f"{(b, t, c, h, w)} train fused {name}: {e:.3e} of the float64 peak (bar {BARS[name]:.0e})")
        assert g.shape == want[name].shape and e < BARS[name], (name, e)
    for k in ("img", "kref", "k0", "sens"):
        assert torch.equal(d[k].cpu(), x[k]), k                                   # the caller's tensors are untouched


# ------------------------------------------------------------------ b. the model families
FAMILIES_A = ["varnet_XF", "cinenet_XF", "cinenet_3D"]                            # the caller's maps; three k-spaces, best / worst bars
FAMILIES_B = ["xpdnet", "xpdnet_dual", "varnet_rnn", "cinenet_rnn", "xpdnet_rnn", "xpdnet_rnn_dual"]
DUAL = ("xpdnet_dual", "xpdnet_rnn_dual")


def _step(net, run, monkeypatch, train_on):
    """One forward + backward of the HIP model under the given switch: output, loss, gradients, counter 15 over the forward and the backward."""
    switches(monkeypatch, train_on)
    net.zero_grad()
    counter()
    with torch.enable_grad():
        out, loss = run()
        fwd = counter()
        loss.backward()
    bwd = counter()
    return out.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}, fwd, bwd


@pytest.mark.parametrize("family", FAMILIES_A)
def test_varnet_and_cinenet_train_on_the_image_space_operators_vs_oracle_float64(dev, family, monkeypatch):
    """test_hip_grad.py::test_masks_that_vary_along_w_inference_and_training_vs_oracle_float64 with both switches on."""
    import reconstruction.models as M
    from cine_hip import synth
    from oracle import varnet_ref as V, cinenet_ref as C
    t, c, h, w = 5, 3, 20, 18
    make = {"varnet_XF": (lambda m: m.VarNet(2, 4, 2, 4, 2, "XF"), V), "cinenet_XF": (lambda m: m.CineNet(2, 3, 4, 2, "XF"), C),
            "cinenet_3D": (lambda m: m.CineNet(2, 2, 4, 2, "3D"), C)}[family]
    net = make[0](M)
    synth.fill_parameters_(net, 13, keep=("lambda",))
    ref = make[0](make[1]).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()}, strict=True)
    net = net.to(dev).train()
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand(1, t, 1, h, w, 1, generator=g) < 0.4).to(torch.uint8)
    mask[:, :, :, h // 2 - 2:h // 2 + 2, w // 2 - 3:w // 2 + 3] = 1
    sens = rnd(32, 1, 1, c, h, w, 2)
    sens = sens / sens.pow(2).sum(dim=(2, 5), keepdim=True).sqrt()
    target = rnd(33, 1, t, h, w).abs() + 0.1

    def run(model, mk, device, dtype):
        out = model(mk.to(device, dtype), mask.to(device), sens.to(device, dtype))
        return out, ((out - target.to(device, dtype)) ** 2).mean()
    best, worst = {}, {}
    for seed in (31, 41, 51):
        mk = rnd(seed, 1, t, c, h, w, 2) * mask
        ref.zero_grad()
        with torch.enable_grad():
            o64, l64 = run(ref, mk, torch.device("cpu"), torch.float64); l64.backward()
        o32, _, grads, fwd, bwd = _step(net, lambda: run(net, mk, dev, torch.float32), monkeypatch, True)
        assert fwd > 0 and bwd > 0, (fwd, bwd)                                   # the route: mask-plane column passes in both directions
        if seed == 31:
            _, _, _, fwd_off, bwd_off = _step(net, lambda: run(net, mk, dev, torch.float32), monkeypatch, False)
            assert fwd_off == 0 and bwd_off == 0, (fwd_off, bwd_off)
        assert rel_err(o32.cpu(), o64.detach().float()) < 2e-5, seed
        want = {k: p for k, p in ref.named_parameters() if p.grad is not None}
        assert len(want) >= 10
        for k, p in net.named_parameters():
            if k not in want:
                assert k not in grads or float(grads[k].abs().max()) == 0.0, k
                continue
            e = rel_err(grads[k].cpu(), want[k].grad.float())
            best[k] = min(best.get(k, 1e9), e); worst[k] = max(worst.get(k, 0.0), e)
    print(f"{family}: worst best-of-three {max(best.values()):.3e} (bar 1e-3), worst {max(worst.values()):.3e} (bar 5e-2)")
    bad = {k: (best[k], worst[k]) for k in best if best[k] > 1e-3 or worst[k] > 5e-2}
    assert not bad, bad


def _family_b(family, monkeypatch):
    """Model, oracle and inputs of test_hip_grad.py::test_masks_that_vary_along_w_xpdnet_and_crnn_models_vs_oracle_float64."""
    import reconstruction.models as M
    from cine_hip import synth
    from oracle import recurrent_ref as R, xpdnet_ref as X, varnet_ref as V
    t, c, h, w = 4, 3, 24, 20
    kw = dict(num_cascades=2, sens_chans=4, sens_pools=2, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[1, 1], first_conv_n_filters=8,
              n_primal=2, dynamic_type="XF", weight_sharing=False)
    make, needs_sens = {
        "xpdnet": (lambda m: m.XPDNet(primal_only=True, **kw), False), "xpdnet_dual": (lambda m: m.XPDNet(primal_only=False, **kw), False),
        "varnet_rnn": (lambda m: m.VarNet_RNN(2, 4, 2, 6), False), "cinenet_rnn": (lambda m: m.CineNet_RNN(2, 3, 6), True),
        "xpdnet_rnn": (lambda m: m.XPDNet_RNN(2, 4, 2, 6, True, 2, 1), False), "xpdnet_rnn_dual": (lambda m: m.XPDNet_RNN(2, 4, 2, 6, False, 2, 1), False)}[family]
    net = make(M)
    synth.fill_parameters_(net, 17, keep=("lambda",))
    ref = make(X if family.startswith("xpdnet") and "rnn" not in family else R).double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()}, strict=True)
    acs = (9, 6)                                     # rows [9, 15): what the sens-nets keep; pinned on both sides
    for mod in (V, X, R):
        for name in dir(mod):
            cls = getattr(mod, name)
            if isinstance(cls, type) and hasattr(cls, "acs_window"):
                monkeypatch.setattr(cls, "acs_window", staticmethod(lambda mask: acs))
    g = torch.Generator().manual_seed(6)
    mask = (torch.rand(1, t, 1, h, w, 1, generator=g) < 0.4).to(torch.uint8)
    mask[:, :, :, 9:15, w // 2 - 4:w // 2 + 4] = 1
    sens = rnd(32, 1, 1, c, h, w, 2)
    sens = sens / sens.pow(2).sum(dim=(2, 5), keepdim=True).sqrt()
    target = rnd(33, 1, t, h, w).abs() + 0.1

    def run(model, mask, device, dtype, hip):
        a = ((rnd(34, 1, t, c, h, w, 2) * mask).to(device, dtype), mask.to(device))
        if needs_sens:
            out = model(*a, sens.to(device, dtype))
        else:
            out = model(*a, acs=acs) if hip else model(*a)
        return out, ((out - target.to(device, dtype)) ** 2).mean()
    return net, ref.train(), mask, run


def _l2(got, want):
    return float((got.cpu().double() - want.cpu().double()).norm() / want.cpu().double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("family", FAMILIES_B)
def test_xpdnet_and_crnn_models_train_on_the_image_space_operators_vs_oracle_float64(dev, family, monkeypatch):
    net, ref, mask, run = _family_b(family, monkeypatch)
    net = net.to(dev).train()
    with torch.enable_grad():
        o64, l64 = run(ref, mask, torch.device("cpu"), torch.float64, False); l64.backward()
    o32, _, grads, fwd, bwd = _step(net, lambda: run(net, mask, dev, torch.float32, True), monkeypatch, True)
    o_off, _, grads_off, fwd_off, bwd_off = _step(net, lambda: run(net, mask, dev, torch.float32, True), monkeypatch, False)
    assert fwd_off == 0 and bwd_off == 0, (fwd_off, bwd_off)
    if family in DUAL:
        # the K step of the dual nets goes through forward_masked / backward_masked, which stay literal (the k-space CNN needs the k-space), and
        # nothing else in these models calls soft_dc / residual_backward: no mask-plane column pass, and the switch changes no bit
        assert fwd == 0 and bwd == 0, (fwd, bwd)
        assert torch.equal(o32, o_off) and grads.keys() == grads_off.keys() and all(torch.equal(grads[k], grads_off[k]) for k in grads)
    else:
        assert fwd > 0 and bwd > 0, (fwd, bwd)
    assert rel_err(o32.cpu(), o64.detach().float()) < 5e-5
    want = {k: p for k, p in ref.named_parameters() if p.grad is not None}
    assert len(want) >= 8
    bad, errs = {}, {}
    for k, p in net.named_parameters():
        if k not in want:
            assert k not in grads or float(grads[k].abs().max()) == 0.0, k
            continue
        errs[k] = _l2(grads[k], want[k].grad)
        if errs[k] > 2e-3:                           # (L2: a ReLU / LeakyReLU kink that flips between float32 and float64 moves isolated entries)
            bad[k] = errs[k]
    print(f"{family}: worst L2 error of a parameter gradient {max(errs.values()):.3e} (bar 2e-3)")
    assert not bad, bad


def test_varnet_rnn_with_equal_columns_agrees_with_the_row_mask_run(dev, monkeypatch):
    """A general-layout mask whose columns are all equal is a row mask: trained through the image-space operators with both line passes it gives
    the row-mask run's output and gradients within the bars of the family (5e-5 of the peak, 2e-3 in L2)."""
    net, _, mask, run = _family_b("varnet_rnn", monkeypatch)
    net = net.to(dev).train()
    row = mask[:, :, :, :, :1].contiguous()                                       # (1, t, 1, h, 1, 1): column 0's pattern
    general = row.expand(mask.shape).contiguous()
    o_row, _, g_row, fwd_row, bwd_row = _step(net, lambda: run(net, row, dev, torch.float32, True), monkeypatch, True)
    o_gen, _, g_gen, fwd, bwd = _step(net, lambda: run(net, general, dev, torch.float32, True), monkeypatch, True)
    assert fwd_row == 0 and bwd_row == 0 and fwd > 0 and bwd > 0
    assert rel_err(o_gen.cpu(), o_row.cpu()) < 5e-5
    assert g_row.keys() == g_gen.keys() and len(g_row) >= 8
    errs = {k: _l2(g_gen[k], g_row[k]) for k in g_row}
    print(f"varnet_rnn, equal columns vs row mask: worst L2 difference of a parameter gradient {max(errs.values()):.3e} (bar 2e-3)")
    assert max(errs.values()) <= 2e-3, {k: e for k, e in errs.items() if e > 2e-3}


# ------------------------------------------------------------------ c. memory
def test_a_training_step_keeps_images_not_kspaces(dev, monkeypatch):
    """Peak memory of one forward + backward of a four-cascade VarNet at (t, c, h, w) = (4, 8, 40, 36), where a coil-wise k-space is 368 640
    bytes.  Counted, not measured: the literal chain keeps at least two k-space-sized tensors per cascade until backward (the blend's input and
    SensReduceFn's saved k-space), >= 8 over four cascades; the image-space path adds one cached k-space-sized workspace: a difference of >= 7
    k-spaces, of which the test asks for 4."""
    import reconstruction.models as M
    from cine_hip import ops, synth
    t, c, h, w = 4, 8, 40, 36
    kbytes = t * c * h * w * 2 * 4
    assert kbytes == 368_640
    net = M.VarNet(4, 4, 2, 4, 2, "XF")
    synth.fill_parameters_(net, 13, keep=("lambda",))
    net = net.to(dev).train()
    mask = make_mask(1, t, h, w, 5).to(dev)
    sens = rnd(32, 1, 1, c, h, w, 2)
    sens = (sens / sens.pow(2).sum(dim=(2, 5), keepdim=True).sqrt()).to(dev)
    mk = rnd(31, 1, t, c, h, w, 2).to(dev) * mask
    target = (rnd(33, 1, t, h, w).abs() + 0.1).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        with torch.enable_grad():
            out = net(mk, mask, sens)
            ((out - target) ** 2).mean().backward()
    peak = {}
    for train_on in (False, True):
        switches(monkeypatch, train_on)
        ops.release_general_workspaces()
        step()                                                                    # warm-up: workspaces and caches of this setting exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        counter()
        step()
        torch.cuda.synchronize()
        peak[train_on] = torch.cuda.max_memory_allocated(dev)
        assert (counter() > 0) == train_on
    ops.release_general_workspaces()
    print(f"peak memory of a step: literal {peak[False]} B, image-space {peak[True]} B, difference {(peak[False] - peak[True]) / kbytes:.2f} k-spaces")
    assert peak[False] - peak[True] >= 4 * kbytes, peak
