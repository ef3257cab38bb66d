"""The locally low-rank iteration of cine_hip.classical / cine_llr_prox / cine_llr_solve restated in float64 numpy on the operators of
tests/kt_reference.py: the yardstick of test_llr_cpu.py, test_llr_kernels.py, test_llr_solve.py and test_llr_models.py.  A plain module,
imported like kernel_sweep.py.

Complex arrays as in kt_reference: images (b, t, h, w).  Per batch element

    minimise  1/2 || M A x - y ||^2 + lam sum over the blocks beta of P of || C_beta(x) ||_*
    x_0 = zf;  g = A^H M A x_k - zf;  x_{k+1} = BlockSVT_{P_k}(x_k - step g, step lam)

P: block x block squares on a grid with its origin at (-sh, -sw), 0 <= shift < block, clipped to the image (no wrap-around); P_k has the
shift of iteration k.  The seeded sequence of ``shifts`` is the contract cine_hip.classical.llr_shifts states too:
numpy.random.RandomState(seed).randint(0, block, size=(iters, 2)).

The singular values of a block are thresholded through numpy.linalg.svd, NOT through the Gram matrix: the yardstick stays independent of
the kernels' route."""
import numpy as np

import kt_reference as R


def blocks(h, w, block, sh=0, sw=0):
    """The partition as a list of (r0, r1, c0, c1), rows first: every pixel lies in exactly one block."""
    assert 0 <= sh < block and 0 <= sw < block, (block, sh, sw)
    rows = [(max(r, 0), min(r + block, h)) for r in range(-sh, h, block)]
    cols = [(max(c, 0), min(c + block, w)) for c in range(-sw, w, block)]
    return [(r0, r1, c0, c1) for r0, r1 in rows for c0, c1 in cols]


def block_svt(x, theta, block, sh=0, sw=0):
    """x (b, t, h, w) -> (result, the nuclear norms of the thresholded blocks added up, the largest block singular value of x)."""
    b, t, h, w = x.shape
    out, nuc, smax = np.empty_like(x), 0.0, 0.0
    for i in range(b):
        for r0, r1, c0, c1 in blocks(h, w, block, sh, sw):
            m = x[i, :, r0:r1, c0:c1].reshape(t, -1).T                   # pixels x frames
            u, s, vh = np.linalg.svd(m, full_matrices=False)
            smax = max(smax, float(s.max()))
            s = np.maximum(s - theta, 0.0)
            out[i, :, r0:r1, c0:c1] = ((u * s) @ vh).T.reshape(t, r1 - r0, c1 - c0)
            nuc += float(s.sum())
    return out, nuc, smax


def prox(x, g, step, thresh, block, sh=0, sw=0):
    """The proximal half of an iteration -> (xnew, [sum |xnew - x|^2, sum |xnew|^2, sum of the blocks' nuclear norms, 0], sigma_max of v).
    g None: v = x and theta = thresh (step None) or step * thresh."""
    v = x if g is None else x - step * g
    theta = thresh if step is None else step * thresh
    xnew, nuc, smax = block_svt(v, theta, block, sh, sw)
    return xnew, np.array([(np.abs(xnew - x) ** 2).sum(), (np.abs(xnew) ** 2).sum(), nuc, 0.0]), smax


def shifts(iters, block, seed=0):
    return np.random.RandomState(seed).randint(0, block, size=(iters, 2)).astype(np.int32)


def solve(zf, sens, mask, step, thresh, block, iters, shift_seq=None, history=None):
    """-> (x, rec (iters, 4)); shift_seq: (iters, 2) or None for the fixed partition; history: a list that receives x after every iteration."""
    x = zf
    rec = np.zeros((iters, 4))
    for k in range(iters):
        sh, sw = (0, 0) if shift_seq is None else (int(shift_seq[k][0]), int(shift_seq[k][1]))
        x, rec[k], _ = prox(x, R.gradient(x, sens, mask, zf), step, thresh, block, sh, sw)
        if history is not None:
            history.append(x)
    return x, rec


def objective(x, y, sens, mask, lam, block):
    """1/2 || M A x - y ||^2 + lam sum of the blocks' nuclear norms, on the fixed (unshifted) partition."""
    r = mask * R.forward_op(x, sens) - y
    return 0.5 * (np.abs(r) ** 2).sum() + lam * block_svt(x, 0.0, block)[1]


def block_sigma_max(zf, block):
    """The largest singular value over the blocks of the unshifted partition and over the batch."""
    return block_svt(zf, 0.0, block)[2]


# ------------------------------------------------------------------ the shared solves
FIXTURES = [((1, 5, 3, 24, 20), "row"), ((2, 15, 4, 32, 28), "plane")]
ITERS, LAM, BLOCK = 30, 0.005, 8
_SOLVES = {}


def settings(shape, layout):
    """(problem, zf as float32 pairs, step, thresh) with the two scalars as float32 values: what the GPU solve is handed."""
    p = R.problem(shape, layout)
    step = float(np.float32(R.default_step(p["s"])))
    thresh = float(np.float32(LAM * block_sigma_max(p["zf"], BLOCK)))
    return p, R.to_pairs(p["zf"]).astype(np.float32), step, thresh


def solved(shape, layout, shifted=True, rounded=True):
    """The float64 solve of ITERS iterations, made once: (x, rec, objective per iteration incl. the start -- of the fixed partition, so
    meaningful for shifted=False only).  shifted: the seed-0 shifts, else the fixed partition.  rounded: from the float32-rounded zf the GPU
    solve is handed; else from the float64 zf = A^H M y, the gradient of exactly the objective() reported."""
    key = (tuple(shape), layout, shifted, rounded)
    if key not in _SOLVES:
        p, zf32, step, thresh = settings(shape, layout)
        zf = R.to_complex(zf32) if rounded else p["zf"]
        hist = []
        x, rec = solve(zf, p["s"], p["m"], step, thresh, BLOCK, ITERS, shifts(ITERS, BLOCK, 0) if shifted else None, hist)
        obj = None
        if not shifted:
            obj = np.array([objective(v, p["y"], p["s"], p["m"], thresh, BLOCK) for v in [zf] + hist])
        _SOLVES[key] = (x, rec, obj)
    return _SOLVES[key]
