"""Self-supervised training on prospectively undersampled scans: SSDU (Yaman et al., MRM 2020).

A scan that was undersampled at the scanner has no fully sampled target, so ``SSIMLoss`` cannot train on it.  Self-supervision by data
undersampling splits the acquired set Omega into Theta and Lambda: the model sees Theta only (its data-consistency steps included), and
the k-space of its output is penalised on the held-out Lambda with a normalised l1-l2 loss,

    u = fft2c(S_c * x),  r = Lambda (u - y),  v = Lambda y,   L = 1/2 ||r||_2 / ||v||_2 + 1/2 ||r||_1 / ||v||_1

(both norms over every real component of the batch; ||.||_1 is the sum of |re| + |im|).  The loss is ONE fused operator
(cine_kspace_loss / cine_kspace_loss_grad, ``autograd.KspaceLossFn``): the coil-wise k-space exists only inside its kernels.

    theta, lam = split_mask(mask)                                        # host, once per sample
    image = model(kspace * theta, theta, output="complex")              # every family takes output="complex"
    loss = KspaceLoss()(image, sens_maps, kspace, lam)
    loss.backward(); optimiser.step()
"""
from typing import Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import autograd as ag
from . import ops


def kspace_loss(image: torch.Tensor, sens_maps: torch.Tensor, kspace: torch.Tensor, loss_mask: torch.Tensor) -> torch.Tensor:
    """The loss above as a float32 scalar on the device.  image (b, t, h, w, 2) or (b, t, 1, h, w, 2), sens_maps (b, 1, c, h, w, 2), measured
    kspace (b, t, c, h, w, 2), loss_mask Lambda: any 0 / 1 mask that broadcasts as (b|1, t|1, 1, h, w|1, 1).  Gradients go to the image, and to
    the maps when they require them.  An empty Lambda gives what the expression gives (nan): no host check is made."""
    mask = ops.as_mask_u8(loss_mask, kspace)
    return ag.KspaceLossFn.apply(image, sens_maps, kspace.detach(), mask)


class KspaceLoss(nn.Module):
    """``kspace_loss`` as a module, beside ``reconstruction.utils.losses.SSIMLoss``."""

    def forward(self, image: torch.Tensor, sens_maps: torch.Tensor, kspace: torch.Tensor, loss_mask: torch.Tensor) -> torch.Tensor:
        return kspace_loss(image, sens_maps, kspace, loss_mask)


def split_mask(mask, rho: float = 0.4, acs: int = 4, std_scale: float = 4, rng: Optional[np.random.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Split the sampled set Omega of ``mask`` into (Theta, Lambda), both uint8 in the input's layout and on its device.

    ``mask`` is a row mask (b, t, 1, h, 1, 1) or a plane mask (b, t, 1, h, w, 1).  Per frame, ``round(rho * n)`` of the ``n`` sampled
    positions outside the centre -- the central ``acs`` rows, for planes the central ``acs`` x ``acs`` box -- move from Omega into Lambda,
    drawn without replacement with probability proportional to a Gaussian of std ``size / std_scale`` around the centre (per axis).  The
    centre stays in Theta.  Runs on the host with a numpy ``Generator`` (``rng``; a fresh default one if None), as the reference's mask
    functions do (data/transforms.py); the input is not modified."""
    if not 0.0 <= rho <= 1.0:
        raise ValueError(f"rho={rho}: expected a fraction in [0, 1]")
    rng = np.random.default_rng() if rng is None else rng
    m = torch.as_tensor(mask)
    if m.dim() != 6 or m.shape[2] != 1 or m.shape[5] != 1:
        raise ValueError(f"mask {tuple(m.shape)}: expected (b, t, 1, h, 1, 1) or (b, t, 1, h, w, 1)")
    omega = (m.detach().cpu().numpy() != 0)
    b, t, _, h, w, _ = omega.shape
    cy, cx = h // 2, w // 2
    centre = np.zeros((h, w), dtype=bool)
    y0 = max(cy - acs // 2, 0)
    if w == 1:
        centre[y0:y0 + acs, :] = True
    else:
        x0 = max(cx - acs // 2, 0)
        centre[y0:y0 + acs, x0:x0 + acs] = True
    gy = np.exp(-0.5 * ((np.arange(h) - cy) / (h / std_scale)) ** 2)
    gx = np.exp(-0.5 * ((np.arange(w) - cx) / (w / std_scale)) ** 2) if w > 1 else np.ones(1)
    weight = np.outer(gy, gx)
    lam = np.zeros_like(omega)
    for ib in range(b):
        for it in range(t):
            frame = omega[ib, it, 0, :, :, 0]
            cand = np.flatnonzero(frame & ~centre)
            k = int(round(rho * cand.size))
            if k == 0:
                continue
            p = weight.reshape(-1)[cand]
            pick = rng.choice(cand, size=k, replace=False, p=p / p.sum())
            lam[ib, it, 0].reshape(-1)[pick] = True
    theta = omega & ~lam
    dev = m.device
    return (torch.from_numpy(theta.astype(np.uint8)).to(dev), torch.from_numpy(lam.astype(np.uint8)).to(dev))
