"""The SSIM loss and the image metrics without a GPU: the float64 yardstick (tests/ssim_reference.py, centred window moments) is itself checked
against the CPU path of SSIMLoss in float64 and against the host metrics of utils/evaluate.py, its own uncertainty is measured, and the
workspace sizes and the refusals of cine_ssim_loss / cine_ssim_loss_bwd / cine_image_metrics that come before any launch are checked through
the loaded library."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_reference as R
from cine_hip import _lib

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAMES = ("cine_ssim_loss_ws_bytes", "cine_ssim_loss", "cine_ssim_loss_bwd", "cine_image_metrics_ws_bytes", "cine_image_metrics")
# the bars of test_loss_metric_kernels.py; the yardstick has to be ten times better than each
LOSS_ABS, GRAD_REL, SSIM_ABS, PSNR_ABS, NMSE_REL = 2e-6, 1e-5, 1e-8, 1e-8, 1e-12
SHAPE = (2, 40, 36)
PAIRS = {"noise": lambda: R.noise_pair(*SHAPE, seed=1), "phantom-1e-2": lambda: R.phantom_pair(*SHAPE, 1e-2, seed=2),
         "phantom-1e-4": lambda: R.phantom_pair(*SHAPE, 1e-4, seed=3), "phantom-dark": lambda: R.phantom_pair(*SHAPE, 1e-3, dark_frame=1, seed=4)}


def raw_moment_loss_and_grad(tgt, rec, win):
    """SSIMLoss's CPU path (raw moments through conv2d) in float64, with its autograd gradient.  The module builds its window weights in
    float32, so .double() alone would leave 1 / win^2 rounded to float32 (1e-8 off unless win^2 is a power of two): they are set again."""
    from reconstruction.utils import SSIMLoss
    module = SSIMLoss(win_size=win).double()
    module.w.copy_(torch.full((1, 1, win, win), 1.0 / win ** 2, dtype=torch.float64))
    with torch.enable_grad():
        r64 = rec.double().requires_grad_(True)
        loss = module(r64[None, None], tgt.double()[None, None], tgt.max())
        g, = torch.autograd.grad(loss, r64)
    return float(loss.detach()), g


def grad_errors(got, want):
    """(relative L2 error, max |error| / max |reference|)"""
    d = got.double() - want.double()
    return float(d.norm() / want.norm()), float(d.abs().max() / want.abs().max())


def test_symbols_are_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    L = _lib.lib()
    for name in NAMES:
        assert name in declared and hasattr(L, name) and name in _lib._SIGS, name


@pytest.mark.parametrize("win", [3, 4, 7, 11])
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_the_yardstick_agrees_with_ssimloss_in_float64(pair, win):
    tgt, rec = PAIRS[pair]()
    want, want_g = raw_moment_loss_and_grad(tgt, rec, win)
    got, got_g = R.ssim_loss_grad(rec, tgt, win)
    l2, mx = grad_errors(got_g, want_g)
    print(f"{pair} win {win}: loss {got:.9f}, |d loss| {abs(got - want):.2e}, gradient relative L2 {l2:.2e}, max {mx:.2e}")
    assert got == pytest.approx(R.ssim_loss(rec.numpy(), tgt.numpy(), win), abs=1e-14)          # the numpy and the torch form of the yardstick
    assert abs(got - want) <= LOSS_ABS / 10 and l2 <= GRAD_REL / 10 and mx <= GRAD_REL / 10


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_the_yardstick_agrees_with_the_host_metrics(pair):
    from reconstruction.utils import evaluate
    tgt, rec = (v.double().numpy() for v in PAIRS[pair]())
    for mode, maxval in ((0, None), (2, 2.5)):
        m = R.image_metrics(tgt, rec, 7, 0.01, 0.03, mode, maxval)
        assert abs(m["ssim"] - evaluate.ssim(tgt, rec, maxval)) <= SSIM_ABS / 10
        assert abs(m["psnr"] - float(evaluate.psnr(tgt, rec, maxval))) <= PSNR_ABS / 10
        assert abs(m["nmse"] - float(evaluate.nmse(tgt, rec))) <= NMSE_REL / 10 * m["nmse"]
        assert abs(m["mse"] - float(evaluate.mse(tgt, rec))) <= NMSE_REL / 10 * m["mse"]
        assert m["ssim_frames"].shape == (SHAPE[0],) and m["ssim"] == pytest.approx(m["ssim_frames"].mean(), abs=1e-15)
    per_frame = R.image_metrics(tgt, rec, 7, 0.01, 0.03, 1)
    assert 1.0 - per_frame["ssim"] == pytest.approx(R.ssim_loss(rec, tgt, 7), abs=1e-14)        # the loss is the per-frame-range SSIM


def test_the_yardstick_crops_each_side_on_its_own():
    """gt 21 x 30 against pred 26 x 23: rows 2..22 of pred ((26 - 21) // 2 = 2), columns 3..25 of gt ((30 - 23) // 2 = 3)."""
    from reconstruction.utils import evaluate
    rs = np.random.RandomState(6)
    gt, pred = rs.uniform(0, 1, size=(2, 21, 30)), rs.uniform(0, 1, size=(2, 26, 23))
    g, p = gt[:, :, 3:26], pred[:, 2:23, :]
    m = R.image_metrics(gt, pred)
    assert abs(m["ssim"] - evaluate.ssim(g, p)) <= SSIM_ABS / 10 and abs(m["mse"] - float(evaluate.mse(g, p))) <= 1e-15
    assert np.array_equal(R.center_crop(gt, 21, 23), g) and np.array_equal(R.center_crop(pred, 21, 23), p)


def test_the_yardsticks_own_uncertainty():
    """The centred form against the raw-moment float64 form on the phantom at sigma 1e-4, where raw moments cancel most.  Measured (2 x 40 x 36,
    windows 3 / 7 / 11): loss 3.2e-15, gradient 6.6e-13 relative L2 and 8.3e-13 of the maximum, SSIM 4.8e-15, PSNR 0.  Each is far below a
    tenth of the bar that the kernels are held to (2e-6, 1e-5, 1e-5, 1e-8, 1e-8); NMSE and MSE hold no window moments."""
    from reconstruction.utils import evaluate
    tgt, rec = R.phantom_pair(*SHAPE, 1e-4, seed=3)
    worst = dict(loss=0.0, l2=0.0, mx=0.0)
    for win in (3, 7, 11):
        want, want_g = raw_moment_loss_and_grad(tgt, rec, win)
        got, got_g = R.ssim_loss_grad(rec, tgt, win)
        l2, mx = grad_errors(got_g, want_g)
        worst = dict(loss=max(worst["loss"], abs(got - want)), l2=max(worst["l2"], l2), mx=max(worst["mx"], mx))
    t64, r64 = tgt.double().numpy(), rec.double().numpy()
    m = R.image_metrics(t64, r64)
    d_ssim, d_psnr = abs(m["ssim"] - evaluate.ssim(t64, r64)), abs(m["psnr"] - float(evaluate.psnr(t64, r64)))
    print(f"yardstick uncertainty: loss {worst['loss']:.2e}, gradient L2 {worst['l2']:.2e}, gradient max {worst['mx']:.2e}, "
          f"SSIM {d_ssim:.2e}, PSNR {d_psnr:.2e}")
    assert worst["loss"] <= LOSS_ABS / 10 and worst["l2"] <= GRAD_REL / 10 and worst["mx"] <= GRAD_REL / 10
    assert d_ssim <= SSIM_ABS / 10 and d_psnr <= PSNR_ABS / 10


def test_the_input_makers_are_seeded_and_image_like():
    a, b = R.phantom_pair(3, 24, 20, 1e-3, dark_frame=2, seed=5), R.phantom_pair(3, 24, 20, 1e-3, dark_frame=2, seed=5)
    assert all(torch.equal(u, v) and u.dtype == torch.float32 for u, v in zip(a, b))
    assert not torch.equal(a[0], R.phantom_pair(3, 24, 20, 1e-3, dark_frame=2, seed=6)[0])
    tgt, rec = a
    assert 0.99 < float(tgt[0].max()) < 1.01 and 0.04 < float(tgt[0].min()) < 0.06 and float(tgt[2].max()) < 1.1e-3
    assert 0.5e-3 < float((tgt - rec)[:2].std()) / 2 ** 0.5 < 2e-3 and not torch.equal(tgt, rec)
    clean = R.phantom(1, 3, 3)[0]
    assert clean.min() == 0.05 and clean.max() > 0.05                      # even the smallest frame holds an edge
    n = R.noise_pair(2, 8, 8, seed=1)
    assert torch.equal(n[0], R.noise_pair(2, 8, 8, seed=1)[0]) and float(n[1].min()) >= 0.0


# ------------------------------------------------------------------ workspace sizes
def ceil_div(a, b):
    return -(-a // b)


def loss_ws(t, h, w, win):
    """Doubles first -- t * tiles (16 x 16 windows each) partial sums and 2 spare, then three derivatives per window -- then t + 16 floats (the frame maxima)."""
    ho, wo = h - win + 1, w - win + 1
    return 8 * (t * ceil_div(ho, 16) * ceil_div(wo, 16) + 2 + 3 * t * ho * wo) + 4 * (t + 16)


def metric_ws(t, hg, wg, hp, wp, win):
    """Per frame four doubles and one partial sum for every 32 x 32 tile of window positions of the common crop."""
    ch, cw = min(hg, hp), min(wg, wp)
    return 8 * (4 * t + t * ceil_div(ch - win + 1, 32) * ceil_div(cw - win + 1, 32))


def test_the_workspace_sizes():
    L = _lib.lib()
    for t, h, w, win in ((15, 180, 180, 7), (1, 3, 3, 3), (2, 17, 33, 2), (5, 26, 11, 11), (1, 270, 60, 7), (3, 19, 18, 4), (65535, 7, 7, 7)):
        assert L.cine_ssim_loss_ws_bytes(t, h, w, win) == loss_ws(t, h, w, win), (t, h, w, win)
        assert loss_ws(t, h, w, win) % 4 == 0 and (loss_ws(t, h, w, win) - 4 * (t + 16)) % 8 == 0         # the doubles come first: 8-byte aligned
    for bad in ((0, 20, 20, 7), (-1, 20, 20, 7), (2, 6, 20, 7), (2, 20, 6, 7), (2, 20, 20, 12), (2, 20, 20, 1), (2, 20, 20, 0), (2, 20, 20, -3)):
        assert L.cine_ssim_loss_ws_bytes(*bad) == 0, bad
    for t, hg, wg, hp, wp, win in ((15, 180, 180, 180, 180, 7), (3, 180, 150, 200, 200, 7), (1, 3, 3, 3, 3, 3), (4, 43, 35, 38, 44, 11),
                                   (2, 38, 70, 41, 39, 7), (1, 33, 7, 33, 7, 7)):
        assert L.cine_image_metrics_ws_bytes(t, hg, wg, hp, wp, win) == metric_ws(t, hg, wg, hp, wp, win), (t, hg, wg, hp, wp, win)
    for bad in ((0, 20, 20, 20, 20, 7), (-2, 20, 20, 20, 20, 7), (2, 6, 20, 20, 20, 7), (2, 20, 20, 20, 6, 7), (2, 20, 0, 20, 20, 7),
                (2, 20, 20, 20, 20, 13), (2, 20, 20, 20, 20, 1), (2, 20, 20, 20, 20, 0)):
        assert L.cine_image_metrics_ws_bytes(*bad) == 0, bad


# ------------------------------------------------------------------ refusals before any launch
def _fake(names):
    return {k: ctypes.c_void_p(0x10000 * (i + 1)) for i, k in enumerate(names)}       # never dereferenced


def _mine(L, name):
    return L.cine_last_error().startswith(name + b":")


def test_ssim_loss_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = _fake(("x", "y", "loss", "ws"))
    ME = b"cine_ssim_loss"

    def call(nbytes=1 << 40, **kw):
        a = dict(p, t=2, h=20, w=18, win=7)
        a.update(kw)
        return L.cine_ssim_loss(a["x"], a["y"], a["t"], a["h"], a["w"], a["win"], 0.01, 0.03, a["loss"], a["ws"], nbytes, None)

    for name in p:
        assert call(**{name: None}) == EINVAL and _mine(L, ME) and b"null" in L.cine_last_error(), name
    for bad in (dict(t=0), dict(t=-1), dict(t=65536), dict(h=6), dict(w=6), dict(h=0), dict(w=-4)):
        assert call(**bad) == EINVAL and _mine(L, ME), bad
    for win in (1, 0, -7, 12):
        assert call(win=win) == EINVAL and _mine(L, ME) and b"window" in L.cine_last_error(), win
    assert call(win=1, h=1, w=1) == EINVAL and _mine(L, ME) and b"window 1" in L.cine_last_error()
    need = L.cine_ssim_loss_ws_bytes(2, 20, 18, 7)
    assert call(nbytes=need - 1) == EWORKSPACE and _mine(L, ME) and b"workspace" in L.cine_last_error()
    assert call(nbytes=0) == EWORKSPACE


def test_ssim_loss_bwd_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = _fake(("x", "y", "gloss", "ws", "gx"))
    ME = b"cine_ssim_loss_bwd"

    def call(nbytes=1 << 40, **kw):
        a = dict(p, t=2, h=20, w=18, win=7)
        a.update(kw)
        return L.cine_ssim_loss_bwd(a["x"], a["y"], a["t"], a["h"], a["w"], a["win"], a["gloss"], a["ws"], nbytes, a["gx"], None)

    for name in p:
        assert call(**{name: None}) == EINVAL and _mine(L, ME) and b"null" in L.cine_last_error(), name
    for bad in (dict(t=0), dict(t=-1), dict(h=6), dict(w=6), dict(h=0), dict(w=-4)):
        assert call(**bad) == EINVAL and _mine(L, ME), bad
    for win in (1, 0, -7, 12):
        assert call(win=win) == EINVAL and _mine(L, ME) and b"window" in L.cine_last_error(), win
    assert call(win=1, h=1, w=1) == EINVAL and _mine(L, ME) and b"window 1" in L.cine_last_error()
    need = L.cine_ssim_loss_ws_bytes(2, 20, 18, 7)
    assert call(nbytes=need - 1) == EWORKSPACE and _mine(L, ME) and b"workspace" in L.cine_last_error()
    assert call(nbytes=0) == EWORKSPACE


def test_image_metrics_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()
    p = _fake(("gt", "pred", "out", "ws"))
    ME = b"cine_image_metrics"

    def call(nbytes=1 << 40, **kw):
        a = dict(p, t=2, hg=20, wg=18, hp=22, wp=17, win=7, mode=0, maxval=0.0)
        a.update(kw)
        return L.cine_image_metrics(a["gt"], a["pred"], a["t"], a["hg"], a["wg"], a["hp"], a["wp"], a["win"], 0.01, 0.03, a["mode"], a["maxval"],
                                    a["out"], a["ws"], nbytes, None)

    for name in p:
        assert call(**{name: None}) == EINVAL and _mine(L, ME) and b"null" in L.cine_last_error(), name
    for bad in (dict(t=0), dict(t=-1), dict(t=65536), dict(hg=0), dict(wg=-1), dict(hp=0), dict(wp=0)):
        assert call(**bad) == EINVAL and _mine(L, ME), bad
    for bad in (dict(hg=6), dict(wp=6), dict(hp=6, wg=6)):
        assert call(**bad) == EINVAL and _mine(L, ME) and b"smaller than" in L.cine_last_error(), bad
    for win in (1, 0, -7, 13, 2, 4, 6, 10):                                   # one, none, above 11, even
        assert call(win=win) == EINVAL and _mine(L, ME) and b"window" in L.cine_last_error(), win
    assert call(win=1, hg=1, wg=1, hp=1, wp=1) == EINVAL and _mine(L, ME) and b"window 1" in L.cine_last_error()
    for mode in (-1, 3, 7):
        assert call(mode=mode) == EINVAL and _mine(L, ME) and b"range_mode" in L.cine_last_error(), mode
    need = L.cine_image_metrics_ws_bytes(2, 20, 18, 22, 17, 7)
    assert call(nbytes=need - 1) == EWORKSPACE and _mine(L, ME) and b"workspace" in L.cine_last_error()
    assert call(nbytes=0) == EWORKSPACE
    for mode in (0, 1, 2):                                                    # every valid mode gets as far as the workspace
        assert call(mode=mode, nbytes=need - 1) == EWORKSPACE
