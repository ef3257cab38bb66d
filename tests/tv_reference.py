"""The spatio-temporal total-variation iteration of cine_hip.classical / cine_tv_pd_step / cine_tv_solve restated in float64 numpy: the
yardstick of test_tv_cpu.py, test_tv_step_kernels.py, test_tv_solve.py and test_tv_models.py.  A plain module, imported like kernel_sweep.py;
the transforms, the operator and the shared problems are kt_reference's.

Complex arrays throughout: image (b, t, h, w), dual p (3, b, t, h, w) = (p_t, p_h, p_w).  terms: 1 = temporal, 2 = spatial, 3 = both; the
planes of a term that is off pass through `step` unchanged and count as zero in D^H.

    minimise  1/2 || M A x - y ||^2  +  lam_t || D_t x ||_1  +  lam_s sum sqrt(|D_h x|^2 + |D_w x|^2)
    x_0 = zf, p_0 = 0
    g = A^H M A x_k - zf;   x_{k+1} = x_k - tau (g + D^H p_k);   p_{k+1} = P(p_k + sigma D (2 x_{k+1} - x_k))
"""
import numpy as np

import kt_reference as K


def _fwd(x, axis, periodic=False):
    """x[i + 1] - x[i] along axis; at the last index 0, or with periodic x[0] - x[last]."""
    d = np.zeros_like(x)
    n = x.shape[axis]
    lo = [slice(None)] * x.ndim
    hi = [slice(None)] * x.ndim
    lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
    d[tuple(lo)] = x[tuple(hi)] - x[tuple(lo)]
    if periodic:
        first, last = [slice(None)] * x.ndim, [slice(None)] * x.ndim
        first[axis], last[axis] = 0, n - 1
        d[tuple(last)] = x[tuple(first)] - x[tuple(last)]
    return d


def _adj(p, axis, periodic=False):
    """The adjoint of _fwd: p[i - 1] - p[i], where an index that _fwd never wrote (the last one, unless periodic) counts as zero."""
    n = p.shape[axis]
    if periodic:
        return np.roll(p, 1, axis=axis) - p
    q = p.copy()
    last = [slice(None)] * p.ndim
    last[axis] = n - 1
    q[tuple(last)] = 0
    out = -q
    lo = [slice(None)] * p.ndim
    hi = [slice(None)] * p.ndim
    lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
    out[tuple(hi)] += q[tuple(lo)]
    return out


def D(x, periodic=True, terms=3):
    """(b, t, h, w) -> (3, b, t, h, w); the planes of a term that is off are zero."""
    out = np.zeros((3,) + x.shape, dtype=x.dtype)
    if terms & 1:
        out[0] = _fwd(x, 1, periodic)
    if terms & 2:
        out[1], out[2] = _fwd(x, 2), _fwd(x, 3)
    return out


def DH(p, periodic=True, terms=3):
    """(3, b, t, h, w) -> (b, t, h, w): the exact adjoint of D, boundary rules included."""
    out = np.zeros(p.shape[1:], dtype=p.dtype)
    if terms & 1:
        out = out + _adj(p[0], 1, periodic)
    if terms & 2:
        out = out + _adj(p[1], 2) + _adj(p[2], 3)
    return out


def project(p, lam_t, lam_s, terms=3):
    """p_t onto the complex ball of radius lam_t, (p_h, p_w) jointly onto the ball of radius lam_s; a plane that is off passes through."""
    out = p.copy()
    if terms & 1:
        out[0] = p[0] / np.maximum(1.0, np.abs(p[0]) / lam_t)
    if terms & 2:
        s = np.maximum(1.0, np.sqrt(np.abs(p[1]) ** 2 + np.abs(p[2]) ** 2) / lam_s)
        out[1], out[2] = p[1] / s, p[2] / s
    return out


def record(xnew, x, periodic=True, terms=3):
    """[sum |xnew - x|^2, sum |xnew|^2, sum |D_t xnew|, sum sqrt(|D_h xnew|^2 + |D_w xnew|^2)]; the sum of a term that is off is 0."""
    d = D(xnew, periodic, terms)
    return np.array([(np.abs(xnew - x) ** 2).sum(), (np.abs(xnew) ** 2).sum(), np.abs(d[0]).sum(),
                     np.sqrt(np.abs(d[1]) ** 2 + np.abs(d[2]) ** 2).sum()])


def step(x, g, p, tau, sigma, lam_t, lam_s, periodic=True, terms=3):
    """Everything after g of one iteration -> (xnew, pnew, record)."""
    xnew = x - tau * (g + DH(p, periodic, terms))
    pnew = project(p + sigma * D(2.0 * xnew - x, periodic, terms), lam_t, lam_s, terms)
    return xnew, pnew, record(xnew, x, periodic, terms)


def norm_bound(terms):
    """B >= ||D||^2: 4 per difference axis."""
    return 4.0 * bool(terms & 1) + 8.0 * bool(terms & 2)


def default_sigma(tau, terms):
    """1 / (2 tau B): with tau <= 1 / L this gives 1 / tau - sigma ||D||^2 >= L / 2, Condat's condition."""
    return 1.0 / (2.0 * tau * norm_bound(terms))


def solve(zf, sens, mask, tau, sigma, lam_t, lam_s, iters, periodic=True, terms=3):
    """-> (x, p (3, b, t, h, w), rec (iters, 4)) after `iters` iterations from x = zf, p = 0."""
    x, p = zf, np.zeros((3,) + zf.shape, dtype=complex)
    rec = np.zeros((iters, 4))
    for k in range(iters):
        x, p, rec[k] = step(x, K.gradient(x, sens, mask, zf), p, tau, sigma, lam_t, lam_s, periodic, terms)
    return x, p, rec


def objective(x, y, sens, mask, lam_t, lam_s, periodic=True):
    """1/2 || M A x - y ||^2 + lam_t || D_t x ||_1 + lam_s sum sqrt(|D_h x|^2 + |D_w x|^2) with y the masked k-space."""
    r = mask * K.forward_op(x, sens) - y
    d = D(x, periodic, 3)
    return 0.5 * (np.abs(r) ** 2).sum() + lam_t * np.abs(d[0]).sum() + lam_s * np.sqrt(np.abs(d[1]) ** 2 + np.abs(d[2]) ** 2).sum()


def peaks(zf, periodic=True):
    """(max |D_t zf|, max sqrt(|D_h zf|^2 + |D_w zf|^2)): the scales lam_t and lam_s are fractions of."""
    d = D(zf, periodic, 3)
    return float(np.abs(d[0]).max()), float(np.sqrt(np.abs(d[1]) ** 2 + np.abs(d[2]) ** 2).max())


def power_iteration(shape, periodic=True, terms=3, iters=200, seed=0):
    """The largest eigenvalue of D^H D on `shape` (b, t, h, w), by power iteration from a seeded start."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(shape) + 1j * rs.standard_normal(shape)
    lam = 0.0
    for _ in range(iters):
        x = x / np.linalg.norm(x)
        y = DH(D(x, periodic, terms), periodic, terms)
        lam = float(np.vdot(x, y).real)
        x = y
    return lam
