"""The k-t SPARSE-SENSE iteration of cine_hip.classical / cine_kt_prox / cine_kt_fista restated in float64 numpy: the yardstick of
test_kt_cpu.py, test_kt_prox_kernels.py, test_kt_fista.py and test_kt_classical_models.py.  A plain module, imported like kernel_sweep.py.

Complex arrays throughout: image (b, t, h, w), maps (b, c, h, w), k-space (b, t, c, h, w), mask (b, t, 1, h, w | 1) of 0 / 1.
The centered transforms are those of reconstruction/utils/fftc.py (ifftshift, ortho transform, fftshift) restated with np.fft.

    x_0 = z_0 = zf,  s_0 = 1
    g = A^H M A z_k - zf;  v = z_k - step g;  x_{k+1} = F_t^H soft(F_t v, step thresh w_f);  z_{k+1} = x_{k+1} + beta_k (x_{k+1} - x_k)
    s_{k+1} = (1 + sqrt(1 + 4 s_k^2)) / 2,  beta_k = float32((s_k - 1) / s_{k+1})
"""
import numpy as np


def to_complex(pairs):
    """(..., 2) float pairs (numpy or torch) -> complex128."""
    a = np.asarray(pairs.detach().cpu().numpy() if hasattr(pairs, "detach") else pairs, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1]


def to_pairs(z):
    return np.stack((z.real, z.imag), axis=-1)


def mask_array(mask):
    """A model-layout mask (b, t, 1, h, w | 1, 1) (numpy or torch) -> float64 (b, t, 1, h, w | 1), broadcasting against k-space."""
    m = np.asarray(mask.detach().cpu().numpy() if hasattr(mask, "detach") else mask)
    assert m.ndim == 6 and m.shape[2] == 1 and m.shape[5] == 1, m.shape
    return (m[..., 0] != 0).astype(np.float64)


def fft2c(x, inverse=False):
    ax = (-2, -1)
    f = np.fft.ifft2 if inverse else np.fft.fft2
    return np.fft.fftshift(f(np.fft.ifftshift(x, axes=ax), axes=ax, norm="ortho"), axes=ax)


def fft1c(x, axis, inverse=False):
    f = np.fft.ifft if inverse else np.fft.fft
    return np.fft.fftshift(f(np.fft.ifftshift(x, axes=axis), axis=axis, norm="ortho"), axes=axis)


def forward_op(x, sens):
    """A x = fft2c(S_c x): (b, t, h, w) -> (b, t, c, h, w)."""
    return fft2c(x[:, :, None] * sens[:, None])


def adjoint_op(k, sens):
    """A^H k = sum_c conj(S_c) ifft2c(k_c)."""
    return (np.conj(sens[:, None]) * fft2c(k, inverse=True)).sum(axis=2)


def zero_filled(y, sens, mask):
    return adjoint_op(mask * y, sens)


def gradient(z, sens, mask, zf):
    """A^H M A z - zf."""
    return adjoint_op(mask * forward_op(z, sens), sens) - zf


def bin_weights(t, penalise_dc):
    """w_f along the centered temporal axis: 1, or 0 at the DC bin t // 2."""
    w = np.ones(t)
    if not penalise_dc:
        w[t // 2] = 0.0
    return w


def soft(c, theta):
    """c max(|c| - theta, 0) / |c|, 0 at c = 0; theta broadcasts."""
    mag = np.abs(c)
    return c * (np.maximum(mag - theta, 0.0) / np.where(mag > 0, mag, 1.0))


def prox(z, g, xprev, step, thresh, beta, penalise_dc=True):
    """One iteration's second half -> (xnew, znew, [sum |xnew - xprev|^2, sum |xnew|^2, sum_f w_f |F_t xnew|]).  Frames on axis 1."""
    w = bin_weights(z.shape[1], penalise_dc).reshape(1, -1, 1, 1)
    v = z - step * g
    xnew = fft1c(soft(fft1c(v, 1), step * thresh * w), 1, inverse=True)
    znew = xnew + beta * (xnew - xprev)
    rec = np.array([(np.abs(xnew - xprev) ** 2).sum(), (np.abs(xnew) ** 2).sum(), (w * np.abs(fft1c(xnew, 1))).sum()])
    return xnew, znew, rec


def momentum(iters):
    """beta_k as the float32 values the solver uses, from the double recurrence."""
    out, s = [], 1.0
    for _ in range(iters):
        s1 = (1.0 + np.sqrt(1.0 + 4.0 * s * s)) / 2.0
        out.append(np.float32((s - 1.0) / s1))
        s = s1
    return np.array(out, dtype=np.float32)


def fista(zf, sens, mask, step, thresh, iters, penalise_dc=True, betas=None):
    """-> (x after `iters` iterations, rec (iters, 3)).  betas: the momentum per iteration (default `momentum(iters)`; zeros give ISTA)."""
    betas = momentum(iters) if betas is None else betas
    x = z = zf
    rec = np.zeros((iters, 3))
    for k in range(iters):
        x, z, rec[k] = prox(z, gradient(z, sens, mask, zf), x, step, thresh, float(betas[k]), penalise_dc)
    return x, rec


def objective(x, y, sens, mask, lam, penalise_dc=True):
    """1/2 || M A x - y ||^2 + lam || w F_t x ||_1 with y the masked k-space."""
    r = mask * forward_op(x, sens) - y
    w = bin_weights(x.shape[1], penalise_dc).reshape(1, -1, 1, 1)
    return 0.5 * (np.abs(r) ** 2).sum() + lam * (w * np.abs(fft1c(x, 1))).sum()


def default_step(sens):
    """1 / max_pixel sum_c |S_c|^2."""
    return 1.0 / (np.abs(sens) ** 2).sum(axis=1).max()


def nrmse(x, truth):
    return float(np.sqrt((np.abs(x - truth) ** 2).sum() / (np.abs(truth) ** 2).sum()))


# ------------------------------------------------------------------ the shared fixture
_PROBLEMS = {}


def problem(shape, layout, seed=0):
    """One seeded k-t problem, made once per (shape, layout) and shared: cine_hip.synth's moving-disc phantom on RSS-normalised smooth maps,
    1 % k-space noise, about one row in three per frame plus four centre rows; layout "plane" also drops the first fifth of every readout
    outside the centre rows (a partial echo), so the mask varies along w.  Returns a dict of float32 / uint8 torch tensors in the models'
    layouts -- masked_kspace (b, t, c, h, w, 2), mask (b, t, 1, h, w | 1, 1), sens_maps (b, 1, c, h, w, 2), target (b, t, h, w) -- and their
    float64 numpy forms y, m, s, zf for the functions above."""
    import torch
    from cine_hip import synth
    key = (tuple(shape), layout, seed)
    if key not in _PROBLEMS:
        b, t, c, h, w = shape
        ex = [synth.make_cine_slice(t, c, h, w, accel=3, center_lines=4, seed=seed + i, noise_std=0.01) for i in range(b)]
        kspace = torch.cat([e["kspace"] for e in ex])
        mask = torch.cat([e["mask"] for e in ex])
        if layout == "plane":
            mask = mask.expand(b, t, 1, h, w, 1).clone()
            mask[:, :, :, :h // 2 - 2, :w // 5] = 0
            mask[:, :, :, h // 2 + 2:, :w // 5] = 0
        else:
            assert layout == "row", layout
        mask = mask.contiguous()
        p = {"masked_kspace": (kspace * mask + 0.0).contiguous(), "mask": mask, "sens_maps": torch.cat([e["sens_maps"] for e in ex]),
             "target": torch.cat([e["target"] for e in ex])}
        p["y"], p["m"], p["s"] = to_complex(p["masked_kspace"]), mask_array(mask), to_complex(p["sens_maps"])[:, 0]
        p["zf"] = zero_filled(p["y"], p["s"], p["m"])
        _PROBLEMS[key] = p
    return _PROBLEMS[key]
