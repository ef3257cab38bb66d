"""Drop-in boundary against the reference's own callers.

The cases that run the reference's own modules (pl_modules, data) need its checkout (CINE_REFERENCE_ROOT or /root/reference)
and skip without it; the SSIM parity and the layout of a reference-made checkpoint come from tests/golden/dropin_glue.npz
(made by tests/golden/make_golden.py from the reference) and run anywhere.  Each reference case runs in a fresh interpreter
with exactly the path order INTEGRATION.md section 1 prescribes (this build's package first, the reference checkout second) and stubs for the third-party packages the image
lacks (pytorch_lightning, torchmetrics, bart, h5py, skimage): import-time stand-ins only, none of them is on the path
under test.  The reference-made checkpoint is produced by a second interpreter that sees ONLY the reference.
"""
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import PKG, ROOT

REF = os.environ.get("CINE_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "reconstruction")),
                                     reason="reference checkout not present (build container only)")

STUBS = textwrap.dedent("""
    import sys, types, torch
    for name in ("bart", "h5py", "torchmetrics", "skimage", "skimage.metrics"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.metrics"].peak_signal_noise_ratio = None
    sys.modules["skimage.metrics"].structural_similarity = None
    pl = types.ModuleType("pytorch_lightning")
    class LightningModule(torch.nn.Module):
        def save_hyperparameters(self, *a, **k): pass
    class LightningDataModule: pass
    class Metric(torch.nn.Module):
        def __init__(self, dist_sync_on_step=True): super().__init__()
        def add_state(self, name, default, dist_reduce_fx=None): self.register_buffer(name, default)
    pl.LightningModule, pl.LightningDataModule = LightningModule, LightningDataModule
    pl.metrics = types.ModuleType("pytorch_lightning.metrics"); pl.metrics.Metric = Metric
    sys.modules["pytorch_lightning"] = pl; sys.modules["pytorch_lightning.metrics"] = pl.metrics
""")


def _run(code, pythonpath, extra_env=None):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join(pythonpath)
    env.pop("CINE_REFERENCE_ROOT", None)
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, "-c", STUBS + textwrap.dedent(code)], env=env, capture_output=True, text=True,
                       timeout=600, cwd="/tmp")
    assert r.returncode == 0, r.stdout + "\n" + r.stderr
    return r.stdout


@needs_reference
def test_reference_import_lines_resolve_with_integration_path_order():
    """The import lines of pl_modules/varnet_module.py:4-6, data_module.py:15, mri_module.py:18-19 and run_inference.py."""
    out = _run("""
        import os
        import reconstruction
        from reconstruction.data import transforms
        from reconstruction.utils import SSIMLoss
        from reconstruction.models import VarNet, VarNet_RNN, CineNet, CineNet_RNN, XPDNet, XPDNet_RNN
        from reconstruction.data import CombinedSliceDataset, SliceDataset, VolumeSampler
        from reconstruction.data.mri_data import fetch_dir
        from reconstruction.utils import evaluate
        from reconstruction.data.transforms import VarNetDataTransform, center_crop_to_smallest, to_tensor, mask_center
        from reconstruction.data.subsample import create_mask_for_mask_type
        import reconstruction.pl_modules as P
        build = os.environ["BUILD_PKG"]; ref = os.environ["CINE_REFERENCE_ROOT"]
        here = lambda o: os.path.abspath(sys.modules[o.__module__].__file__)
        assert here(VarNet).startswith(build) and here(SSIMLoss).startswith(build) and here(XPDNet_RNN).startswith(build)
        assert os.path.abspath(evaluate.__file__).startswith(build)
        assert here(SliceDataset).startswith(ref) and here(VolumeSampler).startswith(ref) and here(fetch_dir).startswith(ref)
        assert here(VarNetDataTransform).startswith(ref) and here(P.VarNetModule).startswith(ref)
        assert mask_center.__module__ == "reconstruction.data.transforms" and here(mask_center).startswith(build)
        print("ok")
    """, [PKG, REF], {"CINE_REFERENCE_ROOT": REF, "BUILD_PKG": PKG})
    assert out.strip().endswith("ok")


@needs_reference
def test_varnet_module_constructs_on_the_build_and_loads_a_reference_checkpoint(tmp_path):
    ckpt = str(tmp_path / "ref_varnet_module_state.pt")
    # (1) reference only: a Lightning-style state dict of the DEFAULT VarNetModule (varnet_module.py:74-90), 'varnet.' prefix
    _run(f"""
        torch.Tensor.cuda = lambda self, *a, **k: self
        import reconstruction.utils
        from reconstruction.models import VarNet
        import reconstruction.models.varnet as V
        assert V.__file__.startswith({REF!r})
        torch.manual_seed(3)
        net = VarNet(num_cascades=12, sens_chans=8, sens_pools=4, chans=18, pools=4, dynamic_type="XF", weight_sharing=False)
        torch.save({{"varnet." + k: v for k, v in net.state_dict().items()}}, {ckpt!r})
    """, [REF])
    # (2) build first, reference second: the reference's VarNetModule, unmodified, wraps the build's VarNet
    out = _run(f"""
        import os, pathlib
        import reconstruction.pl_modules as P
        import reconstruction.pl_modules.mri_module as MM
        MM.fetch_dir = lambda key, cfg=None: pathlib.Path("/tmp")      # MriModule.__init__ writes a yaml next to the scripts otherwise
        m = P.VarNetModule()
        import reconstruction.models.varnet as V
        assert V.__file__.startswith(os.environ["BUILD_PKG"]) and type(m.varnet) is V.VarNet
        assert type(m.loss).__module__ == "reconstruction.utils.losses"
        sd = torch.load({ckpt!r})
        own = {{k: v for k, v in m.state_dict().items() if k.startswith("varnet.")}}
        assert set(own) == set(sd), (sorted(set(own) ^ set(sd))[:5])
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(not k.startswith("varnet.") for k in missing), (missing[:5], unexpected[:5])
        m.varnet.load_state_dict({{k[len("varnet."):]: v for k, v in sd.items()}}, strict=True)
        k0 = "varnet.cascades.3.model.0.unet.conv.layers.0.weight"
        assert torch.equal(m.state_dict()[k0], sd[k0]) and m.state_dict()[k0].data_ptr() == m.state_dict()["varnet.model.0.unet.conv.layers.0.weight"].data_ptr()
        # the module's forward is the reference's code calling the build's model: GPU tensors only, loud on CPU
        from cine_hip._lib import CineHipError
        try:
            m(torch.zeros(1, 2, 2, 16, 16, 2), torch.ones(1, 2, 1, 16, 1, 1, dtype=torch.uint8))
        except (CineHipError, IndexError):
            print("ok")
    """, [PKG, REF], {"CINE_REFERENCE_ROOT": REF, "BUILD_PKG": PKG})
    assert out.strip().endswith("ok")


@needs_reference
def test_cinenet_and_xpdnet_modules_construct_on_the_build():
    out = _run("""
        import os, pathlib
        import reconstruction.pl_modules as P
        import reconstruction.pl_modules.mri_module as MM
        MM.fetch_dir = lambda key, cfg=None: pathlib.Path("/tmp")
        build = os.environ["BUILD_PKG"]
        c = P.CineNetModule(); x = P.XPDNetModule()
        for mod in (c.cinenet, x.xpdnet):
            assert os.path.abspath(sys.modules[type(mod).__module__].__file__).startswith(build), type(mod)
        r = P.VarNetModule(dynamic_type="CRNN")
        assert type(r.varnet).__name__ == "VarNet_RNN" and sys.modules[type(r.varnet).__module__].__file__.startswith(build)
        print("ok")
    """, [PKG, REF], {"CINE_REFERENCE_ROOT": REF, "BUILD_PKG": PKG})
    assert out.strip().endswith("ok")


def test_varnet_default_checkpoint_layout_loads_on_the_build(golden):
    """The build's DEFAULT VarNetModule model (varnet_module.py:74-90) against the reference's: the same 'varnet.' keys, shapes and
    aliases (tensors registered under several names share storage), and a checkpoint of that layout loads strict=True."""
    import json
    import torch
    from reconstruction.models import VarNet
    g = golden("dropin_glue")
    layout = json.loads(bytes(g["ckpt_layout"]).decode())
    gen = torch.Generator().manual_seed(3)
    sd = {}
    for k, (shape, canon) in layout.items():
        sd[k] = sd[canon] if canon != k else torch.randn(shape, generator=gen)
    net = VarNet(num_cascades=12, sens_chans=8, sens_pools=4, chans=18, pools=4, dynamic_type="XF", weight_sharing=False)
    own = {"varnet." + k: v for k, v in net.state_dict().items()}
    assert set(own) == set(sd), (sorted(set(own) ^ set(sd))[:5])
    assert all(tuple(own[k].shape) == tuple(v.shape) for k, v in sd.items())
    net.load_state_dict({k[len("varnet."):]: v for k, v in sd.items()}, strict=True)
    mine = net.state_dict()
    for k, (_, canon) in layout.items():
        assert torch.equal(mine[k[len("varnet."):]], sd[k])
        if canon != k:                                   # an alias in the reference: one storage in the build as well
            assert mine[k[len("varnet."):]].data_ptr() == mine[canon[len("varnet."):]].data_ptr(), k
    k0 = "cascades.3.model.0.unet.conv.layers.0.weight"
    assert mine[k0].data_ptr() == mine["model.0.unet.conv.layers.0.weight"].data_ptr()


def test_ssim_loss_matches_reference_on_cpu(golden):
    """The build's SSIMLoss (device-agnostic) against the reference's (utils/losses.py:25-58, hard-wired .to('cuda')) on the pair
    of tests/golden/dropin_glue.npz and the loss the reference computed for it."""
    import torch
    from reconstruction.utils import SSIMLoss
    g = golden("dropin_glue")
    got = SSIMLoss()(torch.from_numpy(g["ssim_x"]), torch.from_numpy(g["ssim_y"]), torch.tensor([1.0]))
    assert abs(float(got) - float(g["ssim_loss"])) < 1e-6, (float(got), float(g["ssim_loss"]))
