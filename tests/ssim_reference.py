"""SSIMLoss (utils/losses.py), its gradient and the image metrics (utils/evaluate.py after center_crop_to_smallest) restated in float64 on
the CPU: the yardstick of test_loss_metric_cpu.py and test_loss_metric_kernels.py.  A plain module, imported like kernel_sweep.py.

The kernels, SSIMLoss and evaluate.ssim all form the window variances from raw moments, uxx - ux * ux.  The yardstick does not: every window
is cut out (numpy sliding_window_view, torch unfold), its mean is subtracted, and the variances are sums of squared deviations over np - 1.
Nothing cancels, so the yardstick stays exact on smooth windows, where the raw-moment form is at its weakest.

    S = (2 ux uy + C1) (2 vxy + C2) / ((ux^2 + uy^2 + C1) (vx + vy + C2)),   C1 = (k1 L)^2,  C2 = (k2 L)^2,  L the data range

x is the reconstruction, y the target; both (t, h, w)."""
import numpy as np
import torch
from numpy.lib.stride_tricks import sliding_window_view


def ssim_map(x, y, win, k1, k2, data_range):
    """The SSIM of every win x win window of two (h, w) images -> (h - win + 1, w - win + 1), float64, centred moments."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    wx, wy = sliding_window_view(x, (win, win)), sliding_window_view(y, (win, win))
    ux, uy = wx.mean(axis=(-2, -1)), wy.mean(axis=(-2, -1))
    dx, dy = wx - ux[..., None, None], wy - uy[..., None, None]
    n1 = win * win - 1
    vx, vy, vxy = (dx * dx).sum(axis=(-2, -1)) / n1, (dy * dy).sum(axis=(-2, -1)) / n1, (dx * dy).sum(axis=(-2, -1)) / n1
    c1, c2 = (k1 * float(data_range)) ** 2, (k2 * float(data_range)) ** 2
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim_loss(x, y, win=7, k1=0.01, k2=0.03):
    """mean over frames of 1 - mean over windows of S, the data range of a frame being the maximum of its TARGET frame y."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.mean([1.0 - ssim_map(x[f], y[f], win, k1, k2, y[f].max()).mean() for f in range(x.shape[0])]))


def _ssim_loss_torch(x, y, win, k1, k2):
    """ssim_loss on float64 torch tensors (t, h, w), the same centred formula: what autograd differentiates."""
    wx, wy = x.unfold(1, win, 1).unfold(2, win, 1), y.unfold(1, win, 1).unfold(2, win, 1)          # (t, Ho, Wo, win, win)
    ux, uy = wx.mean(dim=(-2, -1)), wy.mean(dim=(-2, -1))
    dx, dy = wx - ux[..., None, None], wy - uy[..., None, None]
    n1 = win * win - 1
    vx, vy, vxy = (dx * dx).sum(dim=(-2, -1)) / n1, (dy * dy).sum(dim=(-2, -1)) / n1, (dx * dy).sum(dim=(-2, -1)) / n1
    rng = y.amax(dim=(1, 2)).reshape(-1, 1, 1)
    c1, c2 = (k1 * rng) ** 2, (k2 * rng) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return (1.0 - s.mean(dim=(1, 2))).mean()


def ssim_loss_grad(x, y, win=7, k1=0.01, k2=0.03, gloss=1.0):
    """(loss, gloss * d loss / d x) by float64 autograd through the centred formula; x, y torch tensors (t, h, w)."""
    with torch.enable_grad():
        x64 = x.detach().double().requires_grad_(True)
        loss = _ssim_loss_torch(x64, y.detach().double(), win, k1, k2)
        g, = torch.autograd.grad(gloss * loss, x64)
    return float(loss.detach()), g


def center_crop(a, ch, cw):
    """The centre (ch, cw) of the last two dimensions: from = (size - crop) // 2, each side on its own."""
    fy, fx = (a.shape[-2] - ch) // 2, (a.shape[-1] - cw) // 2
    return a[..., fy:fy + ch, fx:fx + cw]


def image_metrics(gt, pred, win=7, k1=0.01, k2=0.03, range_mode=0, maxval=None):
    """gt (t, hg, wg) and pred (t, hp, wp) cropped to (min h, min w) -> dict(ssim, ssim_frames, nmse, psnr, mse) in float64.
    range_mode 0: the data range is the maximum of the cropped gt volume; 1: of each cropped gt frame; 2: maxval.  The peak of the PSNR is
    maxval in mode 2 and the maximum of the cropped gt volume otherwise."""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred, np.float64)
    ch, cw = min(gt.shape[1], pred.shape[1]), min(gt.shape[2], pred.shape[2])
    g, p = center_crop(gt, ch, cw), center_crop(pred, ch, cw)
    rng = [{0: g.max(), 1: g[f].max(), 2: maxval}[range_mode] for f in range(g.shape[0])]
    frames = np.array([ssim_map(g[f], p[f], win, k1, k2, rng[f]).mean() for f in range(g.shape[0])])
    d = g - p
    se, mse = float((d * d).sum()), float((d * d).mean())
    peak = float(maxval) if range_mode == 2 else float(g.max())
    return dict(ssim=float(frames.mean()), ssim_frames=frames, nmse=se / float((g * g).sum()), psnr=10.0 * np.log10(peak * peak / mse), mse=mse)


# ------------------------------------------------------------------ seeded inputs: (target, reconstruction), float32 torch tensors (t, h, w)
def noise_pair(t, h, w, seed=0):
    """Uniform noise in [0, 1.5] and a copy with noise of standard deviation 0.1, clamped at 0: every window has a variance far above C2."""
    rs = np.random.RandomState(seed)
    tgt = torch.from_numpy(rs.uniform(0, 1.5, size=(t, h, w)).astype(np.float32))
    rec = (tgt + torch.from_numpy((0.1 * rs.standard_normal((t, h, w))).astype(np.float32))).clamp_min(0)
    return tgt, rec


def phantom(t, h, w):
    """Piecewise-constant discs on a background of 0.05, peak 1 (float64, no noise): a bright ring around a dark pool whose radius changes
    from frame to frame, two smaller discs beside it.  Sizes follow the frame, so a 3 x 3 frame still holds an edge."""
    yy, xx = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    out = np.empty((t, h, w))
    for f in range(t):
        beat = 0.5 + 0.5 * np.cos(2 * np.pi * f / max(t, 1))
        r = np.hypot(yy + 0.1, xx - 0.05)
        img = np.full((h, w), 0.05)
        img[r < 0.62 + 0.08 * beat] = 0.6
        img[r < 0.38 + 0.10 * beat] = 0.25
        img[np.hypot(yy - 0.55, xx + 0.6) < 0.28] = 1.0
        img[np.hypot(yy + 0.7, xx - 0.7) < 0.2] = 0.8
        out[f] = img
    return out


def phantom_pair(t, h, w, sigma, dark_frame=None, seed=0):
    """The phantom with independent Gaussian noise of standard deviation sigma on the target and on the reconstruction: smooth plateaus,
    a dark background, a reconstruction within sigma of its target.  dark_frame: that frame of both is scaled by 1e-3 (per-frame range)."""
    rs = np.random.RandomState(seed)
    clean = phantom(t, h, w)
    tgt, rec = clean + sigma * rs.standard_normal(clean.shape), clean + sigma * rs.standard_normal(clean.shape)
    if dark_frame is not None:
        tgt[dark_frame] *= 1e-3
        rec[dark_frame] *= 1e-3
    return torch.from_numpy(tgt.astype(np.float32)), torch.from_numpy(rec.astype(np.float32))
