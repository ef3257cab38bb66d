"""The low-rank plus sparse iteration of cine_hip.classical / cine_casorati_gram / cine_svt_weight / cine_ls_prox / cine_ls_solve restated in
float64 numpy on the operators of tests/kt_reference.py: the yardstick of test_ls_cpu.py, test_ls_kernels.py, test_ls_solve.py and
test_ls_models.py.  A plain module, imported like kernel_sweep.py.

Complex arrays as in kt_reference: images (b, t, h, w).  Per batch element

    minimise  1/2 || M A (L + S) - y ||^2 + lam_l || C(L) ||_* + lam_s || F_t S ||_1
    L_0 = zf, S_0 = 0;  g = A^H M A (L_k + S_k) - zf;  L_{k+1} = SVT(L_k - step g, step lam_l);  S_{k+1} = F_t^H soft(F_t (S_k - step g), step lam_s)

The singular values are thresholded through numpy.linalg.svd, NOT through the Gram matrix: the yardstick stays independent of the kernels'
method.  gram_weight() is the kernels' route in float64 (numpy.linalg.eigh), kept apart for the tests that compare the two."""
import numpy as np

import kt_reference as R


def casorati(x):
    """(t, h, w) -> (h w, t): pixels x frames."""
    return x.reshape(x.shape[0], -1).T


def uncasorati(m, shape):
    return m.T.reshape(shape)


def svt(x, theta):
    """Singular-value thresholding of the Casorati matrix of each batch element of x (b, t, h, w) -> (result, nuclear norms (b,))."""
    out, nuc = np.empty_like(x), np.zeros(x.shape[0])
    for i in range(x.shape[0]):
        u, s, vh = np.linalg.svd(casorati(x[i]), full_matrices=False)
        s = np.maximum(s - theta, 0.0)
        out[i] = uncasorati((u * s) @ vh, x[i].shape)
        nuc[i] = s.sum()
    return out, nuc


def gram(x):
    """(b, t, h, w) -> (b, t, t): G = X^H X of the Casorati matrix X."""
    return np.stack([casorati(v).conj().T @ casorati(v) for v in x])


def gram_weight(g, theta):
    """One (t, t) Gram matrix -> (W, sigma_max, nuclear norm after thresholding): W = V diag(h) V^H, h = 1 - theta / sqrt(lam) above theta^2."""
    lam, v = np.linalg.eigh(g)
    sq = np.sqrt(np.maximum(lam, 0.0))
    keep = lam > theta * theta
    h = np.where(keep, 1.0 - theta / np.where(keep, sq, 1.0), 0.0)
    return (v * h) @ v.conj().T, float(sq.max()), float((sq * h).sum())


def gram_sqrt(g):
    lam, v = np.linalg.eigh(g)
    return (v * np.sqrt(np.maximum(lam, 0.0))) @ v.conj().T


def prox(l, s, g, step, thresh_l, thresh_s):
    """The proximal half of an iteration -> (lnew, snew, [sum |xnew - (l + s)|^2, sum |xnew|^2, sum |F_t snew|, nuclear norm of lnew])."""
    lnew, nuc = svt(l - step * g, step * thresh_l)
    snew = R.fft1c(R.soft(R.fft1c(s - step * g, 1), step * thresh_s), 1, inverse=True)
    x = lnew + snew
    rec = np.array([(np.abs(x - (l + s)) ** 2).sum(), (np.abs(x) ** 2).sum(), np.abs(R.fft1c(snew, 1)).sum(), nuc.sum()])
    return lnew, snew, rec


def ls_iteration(l, s, zf, sens, mask, step, thresh_l, thresh_s):
    return prox(l, s, R.gradient(l + s, sens, mask, zf), step, thresh_l, thresh_s)


def ls_solve(zf, sens, mask, step, thresh_l, thresh_s, iters, history=None):
    """-> (L, S, rec (iters, 4)); history: a list that receives (L, S) after every iteration."""
    l, s = zf, np.zeros_like(zf)
    rec = np.zeros((iters, 4))
    for k in range(iters):
        l, s, rec[k] = ls_iteration(l, s, zf, sens, mask, step, thresh_l, thresh_s)
        if history is not None:
            history.append((l, s))
    return l, s, rec


def objective(l, s, y, sens, mask, lam_l, lam_s):
    r = mask * R.forward_op(l + s, sens) - y
    nuc = sum(np.linalg.svd(casorati(v), compute_uv=False).sum() for v in l)
    return 0.5 * (np.abs(r) ** 2).sum() + lam_l * nuc + lam_s * np.abs(R.fft1c(s, 1)).sum()


def default_step(sens):
    """Half of kt_reference's: the gradient in (L, S) jointly has Lipschitz constant 2 ||A^H M A||."""
    return 0.5 * R.default_step(sens)


def sigma_max(zf):
    """The largest singular value of the Casorati matrices of zf, over the batch."""
    return max(float(np.linalg.svd(casorati(v), compute_uv=False).max()) for v in zf)


# ------------------------------------------------------------------ the shared solves
FIXTURES = [((1, 5, 3, 24, 20), "row"), ((2, 15, 4, 32, 28), "plane")]
ITERS, LAM_L, LAM_S = 30, 0.01, 0.01
_SOLVES = {}


def settings(shape, layout):
    """(problem, zf as float32 pairs, step, thresh_l, thresh_s) with the three scalars as float32 values: what the GPU solve is handed."""
    p = R.problem(shape, layout)
    step = float(np.float32(default_step(p["s"])))
    thresh_l = float(np.float32(LAM_L * sigma_max(p["zf"])))
    thresh_s = float(np.float32(LAM_S * np.abs(R.fft1c(p["zf"], 1)).max()))
    return p, R.to_pairs(p["zf"]).astype(np.float32), step, thresh_l, thresh_s


def solved(shape, layout, rounded=True):
    """The float64 solve of ITERS iterations, made once: (L, S, rec, objective per iteration incl. the start).  rounded: from the
    float32-rounded zf the GPU solve is handed; else from the float64 zf = A^H M y, the gradient of exactly the objective() reported."""
    key = (tuple(shape), layout, rounded)
    if key not in _SOLVES:
        p, zf32, step, thl, ths = settings(shape, layout)
        zf = R.to_complex(zf32) if rounded else p["zf"]
        hist = []
        l, s, rec = ls_solve(zf, p["s"], p["m"], step, thl, ths, ITERS, hist)
        obj = [objective(zf, np.zeros_like(zf), p["y"], p["s"], p["m"], thl, ths)]
        obj += [objective(a, b, p["y"], p["s"], p["m"], thl, ths) for a, b in hist]
        _SOLVES[key] = (l, s, rec, np.array(obj))
    return _SOLVES[key]
