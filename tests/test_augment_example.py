"""cine_hip.augment on the device, one level above the kernel: warp, warp_maps, augment_example and augment.prepare_example(augment=)
on a tiny slice -- 4 frames, 3 coils, 24 x 20 raw, crop 16 x 12, target 12 x 8, given maps of unit root-sum-of-squares."""
import numpy as np
import pytest
import torch

import augment_reference as R
from kernel_sweep import same_bits

pytestmark = pytest.mark.gpu

T, C, NX, NY = 4, 3, 24, 20
CROP, TARGET = (16, 12), (12, 8)
KW = dict(crop_shape=CROP, crop_target=TARGET, n_slices=T)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def slice_(dev):
    """raw (t, x, y, coil) complex64 on the host, maps (coil, X, Y) complex64 of unit RSS, the row mask, and the filtered crop images."""
    from cine_hip import frontend as FE
    rs = np.random.RandomState(21)
    raw = ((rs.standard_normal((T, NX, NY, C)) + 1j * rs.standard_normal((T, NX, NY, C))) * 1e-6).astype(np.complex64)
    # smooth coil profiles, as real maps are: Gaussian magnitudes around three centres with linear phases, unit RSS everywhere.
    # (Maps that are random from pixel to pixel interpolate to a small RSS, and warp_maps would rightly zero them.)
    yy, xx = np.meshgrid(np.linspace(-1, 1, CROP[0]), np.linspace(-1, 1, CROP[1]), indexing="ij")
    s = np.stack([np.exp(-((yy - np.sin(a)) ** 2 + (xx - np.cos(a)) ** 2) / 2.0) * np.exp(1j * (0.9 * np.cos(a) * yy + 0.7 * a * xx))
                  for a in 2 * np.pi * np.arange(C) / C])
    sens = (s / np.sqrt((np.abs(s) ** 2).sum(axis=0, keepdims=True))).astype(np.complex64)
    mask = (rs.rand(T, 1, CROP[0], 1, 1) < 0.4).astype(np.uint8)
    mask[:, :, CROP[0] // 2 - 2:CROP[0] // 2 + 2] = 1
    _, filt = FE.prepare_slice(torch.from_numpy(raw).to(dev), CROP, T)
    return raw, sens, torch.from_numpy(mask).to(dev), filt


def test_prepare_example_without_augmentation_is_unchanged(dev, slice_):
    from cine_hip import augment as A, frontend as FE
    raw, sens, _, _ = slice_
    k0, m0, t0, *rest0 = FE.prepare_example(raw, sens=sens, fname="a.h5", **KW)                     # the front-end's own, as it was
    k1, m1, t1, *rest1 = A.prepare_example(raw, sens=sens, fname="a.h5", augment=None, **KW)
    kd, _, td, *restd = A.prepare_example(raw, sens=sens, fname="a.h5", **KW)                       # without the keyword
    assert kd.tobytes() == k0.tobytes() and td.tobytes() == t0.tobytes() and restd == rest0
    assert k0.tobytes() == k1.tobytes() and t0.tobytes() == t1.tobytes() and m0 is m1 is None and rest0 == rest1
    k2, _, t2, *rest2 = A.prepare_example(raw, sens=sens, fname="a.h5", augment=A.identity(), **KW)
    assert k2.shape == k0.shape and k2.dtype == k0.dtype and t2.shape == (T,) + TARGET and t2.dtype == np.float32
    assert k2.tobytes() == k0.tobytes() and t2.tobytes() == t0.tobytes() and rest2 == rest0
    k3, _, t3, *_ = A.prepare_example(raw, sens=sens, augment=A.identity(mode="bilinear", border="zeros"), **KW)
    assert k3.tobytes() == k0.tobytes() and t3.tobytes() == t0.tobytes()
    with pytest.raises(Exception, match="Augmentation"):
        A.prepare_example(raw, sens=sens, augment="flip", **KW)
    # the arguments are the front-end's, in its order, with augment behind them
    import inspect
    fe, au = list(inspect.signature(FE.prepare_example).parameters), list(inspect.signature(A.prepare_example).parameters)
    assert au == fe + ["augment"] and inspect.signature(A.prepare_example).parameters["augment"].default is None
    assert all(inspect.signature(A.prepare_example).parameters[k].default == inspect.signature(FE.prepare_example).parameters[k].default for k in fe)


def test_prepare_example_flip_gives_the_flipped_target(dev, slice_):
    """A horizontal flip moves pixels only: the maps are flipped with the images, so the target is the plain example's, flipped (the
    center crop is symmetric: 2 pixels on either side), bit for bit.  The same for a vertical flip with the cardiac cycle reversed."""
    from cine_hip import augment as A, frontend as FE
    raw, sens, _, filt = slice_
    _, _, t0, *_ = FE.prepare_example(raw, sens=sens, **KW)
    for mode in ("bilinear", "bicubic"):
        k1, _, t1, *_ = A.prepare_example(raw, sens=sens, augment=A.Augmentation.from_params(*CROP, flip_h=True, mode=mode), **KW)
        assert t1.tobytes() == np.ascontiguousarray(t0[:, :, ::-1]).tobytes()
        # its k-space is the transform of the flipped images
        want = FE._to_kspace_hip(torch.flip(filt, (3,)).contiguous())
        assert same_bits(torch.view_as_real(torch.from_numpy(k1)), want.cpu())
        # the plain example with the flipped maps, on the flipped images, is the same thing
        t_direct = FE.combine_target(torch.flip(filt, (3,)).contiguous(), torch.view_as_real(torch.from_numpy(sens[:, :, ::-1].copy())).to(dev), TARGET)
        assert t_direct.cpu().numpy().tobytes() == t1.tobytes()
        _, _, t2, *_ = A.prepare_example(raw, sens=sens, augment=A.Augmentation.from_params(*CROP, flip_v=True, t_shift=T - 1, t_reverse=True, mode=mode), **KW)
        assert t2.tobytes() == np.ascontiguousarray(t0[::-1, ::-1]).tobytes()


def test_augment_example_is_its_composition(dev, slice_):
    from cine_hip import augment as A, frontend as FE, ops
    _, sens, mask, filt = slice_
    maps = torch.view_as_real(torch.from_numpy(sens)).contiguous().to(dev)
    keep = filt.clone()
    for aug in (A.Augmentation.from_params(*CROP, rotation_deg=10.0, scale=(1.1, 1.1), t_shift=1, t_reverse=True),
                A.Augmentation.from_params(*CROP, shear_deg=(5.0, -8.0), translate=(1.5, -2.25), flip_h=True, t_shift=3, mode="bilinear", border="zeros"),
                A.sample((1, 2, 3), *CROP, p=1.0, frames=T)):
        k, s, t = A.augment_example(filt, aug, mask, maps, TARGET)
        assert k.shape == filt.shape and s.shape == maps.shape and t.shape == (T,) + TARGET and k.is_cuda and s.is_cuda and t.is_cuda
        images = A.warp(filt, aug)
        want_s = A.warp_maps(maps, aug)
        assert same_bits(k, ops.apply_mask(FE._to_kspace_hip(images), mask))
        assert same_bits(s, want_s)
        assert same_bits(t, FE.combine_target(images, want_s, TARGET))
        k_open, _, _ = A.augment_example(filt, aug, None, maps, TARGET)
        assert same_bits(k_open, FE._to_kspace_hip(images))
        # the warp itself against float64, at the kernel's bar
        ref, foot = R.warp_reference(filt.cpu().numpy(), aug.matrix, A.MODES.index(aug.mode), A.BORDERS.index(aug.border), aug.t_shift % T, aug.t_reverse)
        err = np.abs(images.cpu().numpy().astype(np.float64) - ref)
        assert (err <= R.C_BAR[A.MODES.index(aug.mode)] * R.U * foot).all()
        # complex tensors pass through view_as_real; out= is honoured
        zc = A.warp(torch.view_as_complex(filt), aug)
        assert zc.dtype == torch.complex64 and same_bits(torch.view_as_real(zc), images)
        out = torch.full_like(filt, float("nan"))
        assert A.warp(filt, aug, out=out) is out and same_bits(out, images)
    assert same_bits(filt, keep), "the input images were written"
    assert same_bits(A.warp(filt[0], A.identity()), filt[0])                          # (c, h, w, 2): no frame axis
    from cine_hip._lib import CineHipError
    with pytest.raises(CineHipError, match="t_shift"):
        A.warp(filt[0].contiguous(), A.Augmentation(t_shift=1))
    with pytest.raises(CineHipError, match="overlaps"):
        A.warp(filt, A.identity(), out=filt)


def test_augment_example_calibrates_when_no_maps_are_given(dev, slice_):
    """sens=None: ESPIRiT on the time average of the augmented k-space -- the call frontend.prepare_example makes on the plain one."""
    from cine_hip import augment as A, frontend as FE
    _, _, _, filt = slice_
    aug = A.Augmentation.from_params(*CROP, rotation_deg=-20.0, t_shift=2)
    k, s, t = A.augment_example(filt, aug, None, None, TARGET, ecalib_r=12)
    assert same_bits(k, FE._to_kspace_hip(A.warp(filt, aug)))
    assert s.shape == (C,) + CROP + (2,) and s.is_cuda and bool(torch.isfinite(s).all())
    rss = s.double().square().sum(dim=(0, 3)).sqrt()
    assert bool(((rss - 1.0).abs() < 1e-3)[rss > 0].all()) and bool((rss > 0).any())  # ecalib's maps: unit RSS where they are kept
    assert same_bits(t, FE.combine_target(A.warp(filt, aug), s, TARGET)) and bool(torch.isfinite(t).all())


def test_warp_maps_has_unit_or_zero_rss(dev, slice_):
    from cine_hip import augment as A
    _, sens, _, _ = slice_
    h, w = CROP
    yy, xx = np.meshgrid(np.arange(h) - (h - 1) / 2, np.arange(w) - (w - 1) / 2, indexing="ij")
    support = ((yy / 6.5) ** 2 + (xx / 4.5) ** 2 <= 1.0)                               # ESPIRiT-like: RSS 1 inside an ellipse, 0 outside
    for given in (sens, sens * support[None]):
        maps = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(given).astype(np.complex64))).contiguous().to(dev)
        for aug in (A.Augmentation.from_params(h, w, rotation_deg=33.0, scale=(0.8, 1.3), translate=(2.5, -1.5), border="zeros"),
                    A.Augmentation.from_params(h, w, rotation_deg=-12.0, shear_deg=(10.0, 4.0), border="reflect", t_shift=2, t_reverse=True),
                    A.Augmentation.from_params(h, w, translate=(0.5, 0.5), border="zeros")):
            got = A.warp_maps(maps, aug)
            rss = got.double().square().sum(dim=(0, 3)).sqrt().cpu().numpy()
            assert (np.abs(rss - 1.0) < 1e-6)[rss != 0].all(), rss
            # zero exactly where the bilinear warp of the maps has RSS below one half
            ref, _ = R.warp_planes(maps.cpu().numpy(), aug.matrix, 0, A.BORDERS.index(aug.border))
            ref_rss = np.sqrt((ref ** 2).sum(axis=(0, 3)))
            clear = np.abs(ref_rss - 0.5) > 1e-5
            assert ((rss != 0) == (ref_rss >= 0.5))[clear].all()
            want = np.where(ref_rss[None, :, :, None] >= 0.5, ref / np.maximum(ref_rss, 1e-30)[None, :, :, None], 0.0)
            assert np.abs(got.cpu().numpy() - want)[:, clear].max() < 1e-5
        zc = A.warp_maps(torch.view_as_complex(maps), aug)
        assert zc.dtype == torch.complex64 and same_bits(torch.view_as_real(zc), got)
    # a map that only moves pixels returns the maps' own bits
    maps = torch.view_as_real(torch.from_numpy(sens)).contiguous().to(dev)
    assert same_bits(A.warp_maps(maps, A.identity()), maps)
    assert same_bits(A.warp_maps(maps, A.Augmentation.from_params(h, w, flip_h=True, t_shift=3)), torch.flip(maps, (2,)))


def test_a_training_step_on_an_augmented_example(dev, slice_):
    import reconstruction.models as M
    from cine_hip import augment as A, synth
    _, sens, mask, filt = slice_
    maps = torch.view_as_real(torch.from_numpy(sens)).contiguous().to(dev)
    aug = A.sample((7, 3, 0), *CROP, p=A.schedule(40, 40, p_max=1.0), frames=T)
    assert not aug.is_identity()
    k, s, target = A.augment_example(filt, aug, mask, maps, TARGET)
    assert bool((s.square().sum(dim=(0, 3)) > 0).all())      # smooth maps, reflecting border: no pixel without a map (there the magnitude is 0 and has no gradient)
    net = M.VarNet(2, 4, 2, 4, 2, "XF")
    synth.fill_parameters_(net, 3)
    net = net.to(dev).train()
    y0, x0 = (CROP[0] - TARGET[0]) // 2, (CROP[1] - TARGET[1]) // 2
    with torch.enable_grad():
        out = net(k[None], mask[None], s[None, None])
        assert out.shape == (1, T) + CROP
        loss = (out[0, :, y0:y0 + TARGET[0], x0:x0 + TARGET[1]] - target).pow(2).mean()
        loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
