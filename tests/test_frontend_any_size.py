"""The data front-end on raw k-space of any matrix size (reference data/mri_data.py:283-303): the windowed centered IDFT
(ops.raw_window_ifft2c / cine_raw_window_ifft2c) against numpy in float64, and prepare_slice / prepare_example at raw sizes the
FFT line engines refuse against the CPU oracle (oracle/frontend_ref.py, computed at test time)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _raw(shape, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)


def _cplx(a):
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.complex64)))).contiguous()


def _window_want(raw, t_out, cx, cy, scale):
    from oracle.frontend_ref import _ifft2c_np
    img = _ifft2c_np(scale * raw.astype(np.complex128).transpose(0, 3, 1, 2))
    nx, ny = raw.shape[1], raw.shape[2]
    x0, y0 = (nx - cx) // 2, (ny - cy) // 2
    return img[:t_out, :, x0:x0 + cx, y0:y0 + cy]


# (t_in, nx, ny, coils, t_out, cx, cy): supported and refused lengths, odd and even, lengths 1 and 2, k tails off multiples of 4 / 16,
# no crop, t_out < t_in, 1 and 32 coils, primes 523 and 2053; both axis orders (x first for the wide windows, y first e.g. for 13 x 7)
CASES = [
    (3, 40, 36, 2, 2, 20, 17),
    (2, 1, 2, 1, 2, 1, 2),
    (2, 2, 1, 3, 1, 1, 1),
    (4, 13, 7, 3, 3, 13, 5),
    (3, 13, 7, 2, 3, 13, 7),
    (2, 416, 208, 4, 1, 200, 200),
    (3, 401, 203, 1, 2, 37, 203),
    (2, 45, 50, 32, 2, 33, 18),
    (2, 523, 30, 2, 1, 200, 30),
    (1, 2053, 6, 1, 1, 31, 6),
    (2, 97, 1030, 2, 2, 41, 512),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_raw_window_ifft2c_vs_numpy(dev, case):
    from cine_hip import ops
    t_in, nx, ny, c, t_out, cx, cy = case
    raw = _raw((t_in, nx, ny, c), seed=sum(case))
    scale = 1e6
    x = torch.from_numpy(raw).to(dev)
    got = ops.raw_window_ifft2c(x, t_out, (cx, cy), scale)
    assert tuple(got.shape) == (t_out, c, cx, cy, 2)
    want = _window_want(raw, t_out, cx, cy, scale)
    bar = 1e-5 if max(nx, ny) <= 1024 else 3e-5
    assert rel_err(got.cpu(), torch.view_as_real(torch.from_numpy(np.ascontiguousarray(want)))) < bar
    again = ops.raw_window_ifft2c(x, t_out, (cx, cy), scale)
    assert torch.equal(got, again)                                   # fixed k order, no atomics: bit-identical


@pytest.mark.gpu
@pytest.mark.parametrize("shape,crop,n_slices", [((17, 416, 208, 4), (200, 200), 15),
                                                 ((12, 768, 246, 3), (192, 200), 15),
                                                 ((6, 523, 97, 2), (201, 41), 4)])
def test_prepare_slice_at_refused_raw_sizes_vs_oracle(dev, shape, crop, n_slices):
    """Raw sizes cine_fft2c refuses (416, 768, 523 along x) go through the windowed transform; the filtered crop and its k-space
    match the reference's numpy lines.  (6, 523, 97) has odd raw and odd crop sizes."""
    from cine_hip import frontend as FE, ops
    from oracle import frontend_ref as F
    assert not ops.fft_line_supported(shape[1])
    raw = _raw(shape, seed=shape[1])
    fs = (0.7, 0.0, 0.3, 0.3)
    k, filt = FE.prepare_slice(torch.from_numpy(raw).to(dev), crop, n_slices, fs)
    k_w, filt_w = F.prepare_slice(raw, crop, n_slices, fs)
    assert tuple(filt.shape) == filt_w.shape + (2,) and tuple(k.shape) == k_w.shape + (2,)
    assert rel_err(filt.cpu(), _cplx(filt_w)) < 1e-5
    assert rel_err(k.cpu(), _cplx(k_w)) < 1e-5


@pytest.mark.gpu
def test_prepare_example_at_a_refused_raw_size(dev):
    from cine_hip import frontend as FE
    from oracle import frontend_ref as F
    raw = _raw((17, 416, 208, 4), seed=7)
    rs = np.random.RandomState(8)
    sens = (rs.standard_normal((4, 200, 200)) + 1j * rs.standard_normal((4, 200, 200))).astype(np.complex64)
    k, mask, target, attrs, fname, _ = FE.prepare_example({"y": raw, "mask": np.arange(3)}, sens=sens, fname="raw_416.h5")
    k_w, filt_w = F.prepare_slice(raw)
    tgt_w = F.combine_target(filt_w, sens, (180, 180))
    assert k.dtype == np.complex64 and k.shape == k_w.shape and rel_err(_cplx(k), _cplx(k_w)) < 1e-5
    assert target.dtype == np.float32 and target.shape == tgt_w.shape and rel_err(target, tgt_w) < 1e-5
    assert (mask == np.arange(3)).all() and attrs == {} and fname == "raw_416.h5"
    k2, _, target2, *_ = FE.prepare_example(raw, ecalib_r=24)                            # the ESPIRiT leg (parity unpinned)
    assert rel_err(_cplx(k2), _cplx(k_w)) < 1e-5 and target2.shape == (15, 180, 180) and np.isfinite(target2).all()


@pytest.mark.gpu
def test_supported_raw_sizes_keep_the_line_engines(dev):
    """Raw sizes cine_fft2c takes follow the full-image path, bit for bit."""
    from cine_hip import frontend as FE, ops
    raw = torch.from_numpy(_raw((5, 40, 36, 3), seed=11)).to(dev)
    fs, crop, scaling = (0.7, 0.0, 0.3, 0.3), (21, 17), 1e6
    k, filt = FE.prepare_slice(raw, crop, 3, fs, scaling)
    images = ops.fft2c(torch.view_as_real((raw * scaling).permute(0, 3, 1, 2).contiguous()), inverse=True)
    want_filt = FE.gaussian_filter(FE.crop_select(images, 3, crop), fs)
    x = torch.roll(want_filt, shifts=[-1, -1], dims=[-3, -2]).contiguous()              # both crop sides odd
    want_k = torch.roll(ops.fft2c(x), shifts=[1, 1], dims=[-3, -2]).contiguous()
    assert torch.equal(filt, want_filt) and torch.equal(k, want_k)


@pytest.mark.gpu
def test_invalid_window_raises_before_any_launch(dev):
    from cine_hip import frontend as FE, ops
    from cine_hip._lib import lib
    raw = torch.from_numpy(_raw((3, 416, 30, 2), seed=5)).to(dev)
    L = lib()
    nfam = L.cine_profile_families()
    ms, launches = (ctypes.c_double * nfam)(), (ctypes.c_long * nfam)()
    torch.cuda.synchronize()
    L.cine_profile_begin()
    try:
        for window, frames in (((417, 10), 2), ((200, 31), 2), ((0, 10), 2), ((200, 10), 4), ((200, 10), 0)):
            with pytest.raises(ValueError, match="Invalid shapes."):
                ops.raw_window_ifft2c(raw, frames, window, 1.0)
        with pytest.raises(ValueError, match="Invalid shapes."):
            FE.prepare_slice(raw, (200, 31), 2)
    finally:
        L.cine_profile_end(ms, launches, nfam)
    assert sum(launches) == 0
