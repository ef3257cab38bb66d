"""GRAPPA on unevenly spaced rows in float64 numpy, written from the rule of include/cine_hip.h (not from the kernels and not from
cine_hip.grappa.plan_gaps): the gaps of a frame, the kernels per step from numpy.linalg.solve on the definition's normal equations
(grappa_reference.gram / weights with R = G, ky = 2), their application, and the whole reconstruction.

k-space of a slice is (t, c, h, w) complex, the mask (t, h).  A gap is (lo, G): the targets are the rows lo + m, m = 1 .. G - 1, the
sources the rows lo and lo + G; a row outside the frame reads as zero."""
import numpy as np

import grappa_reference as ref


def plan(mask, max_gap=8, allowed=None):
    """(gaps per frame [(lo, G), ...], the sorted steps among them, unfilled rows per frame (t,) int32) of a (t, h) mask."""
    mask = np.asarray(mask) != 0
    t, h = mask.shape
    allowed = set(range(2, max_gap + 1)) if allowed is None else set(allowed)
    gaps, unfilled = [], np.zeros(t, np.int32)
    for f in range(t):
        acq = [y for y in range(h) if mask[f, y]]
        mine, left = [], h - len(acq)
        if acq:
            entries = []                                                 # (lo, G, rows it fills)
            e = acq[0]
            if e > 0:
                nb = acq[1] - acq[0] if len(acq) >= 2 else 0
                G = max(nb if nb >= 2 else 0, e + 1)
                entries.append((acq[0] - G, G, e))
            for lo, hi in zip(acq[:-1], acq[1:]):
                if hi - lo >= 2:
                    entries.append((lo, hi - lo, hi - lo - 1))
            e = h - 1 - acq[-1]
            if e > 0:
                nb = acq[-1] - acq[-2] if len(acq) >= 2 else 0
                G = max(nb if nb >= 2 else 0, e + 1)
                entries.append((acq[-1], G, e))
            for lo, G, rows in entries:
                if G <= max_gap and G in allowed:
                    mine.append((lo, G))
                    left -= rows
        gaps.append(mine)
        unfilled[f] = left
    return gaps, tuple(sorted({G for g in gaps for _, G in g})), unfilled


def weights(cal, sizes, kx, lam):
    """{G: W_G (G - 1, ns, c) complex128} and {G: info} of the calibration array (c, hc, w): the lattice fit of step G with two source rows."""
    c = np.asarray(cal).shape[0]
    W, info = {}, {}
    for G in sizes:
        W[G], info[G] = ref.weights(ref.gram(cal, G, 2, kx), c, G, 2, kx, lam)
    return W, info


def apply(kspace, W, mask, gaps, kx, bound=False):
    """The filled k-space (t, c, h, w) complex128 from the weights {G: (G - 1, ns, c)} and the gaps per frame; rows of no gap are kept.
    bound=True: also sum |w| |x| of the real products behind each output component (as grappa_reference.apply)."""
    k = np.asarray(kspace)
    t, c, h, w = k.shape
    out = k.astype(np.complex128).copy()
    mag = np.zeros(out.shape, np.complex128) if bound else None
    for f in range(t):
        for lo, G in gaps[f]:
            for r in (lo, lo + G):
                assert not (0 <= r < h) or mask[f, r], "a source row that is not acquired"
            S = ref.source_matrix(k[f], [lo, lo + G], kx).astype(np.complex128)
            for m in range(1, G):
                y = lo + m
                if not 0 <= y < h:
                    continue
                assert not mask[f, y], "a target row that is acquired"
                Wm = np.asarray(W[G][m - 1]).astype(np.complex128)
                out[f, :, y, :] = (S @ Wm).T
                if bound:
                    Sr, Si, Wr, Wi = np.abs(S.real), np.abs(S.imag), np.abs(Wm.real), np.abs(Wm.imag)
                    mag[f, :, y, :] = ((Sr @ Wr + Si @ Wi) + 1j * (Sr @ Wi + Si @ Wr)).T
    return (out, mag) if bound else out


def grappa(kspace, mask, kx=5, lam=1e-4, calib="auto", acs=None, calib_rows=32, max_gap=8, sizes=None):
    """(filled k-space (t, c, h, w) complex128, {G: info}, steps, unfilled (t,)) of one masked slice; `sizes`: the steps with weights,
    by default those that occur.  The weights are rounded to complex64 once, as the device hands them out."""
    k = np.asarray(kspace)
    if sizes is None:
        sizes = plan(mask, max_gap)[1]
    gaps, _, unfilled = plan(mask, max_gap, sizes)
    cal = ref.calibration_data(k, mask, calib, acs, calib_rows)
    W, info = weights(cal, sizes, kx, lam)
    W = {G: v.astype(np.complex64) for G, v in W.items()}
    return apply(k, W, mask, gaps, kx), info, tuple(sizes), unfilled


def equispaced_mask(t, h, center_fraction, acceleration, seed):
    """The (t, h) uint8 mask of cine_hip.synth.EquispacedMaskFunc (one mask for every frame) and the rows [lo, hi) of its centre block."""
    from cine_hip import synth
    m = synth.EquispacedMaskFunc([center_fraction], [acceleration])((t, 1, h, 1, 2), seed=seed).numpy().reshape(h)
    n_low = int(round(h * center_fraction))
    lo = (h - n_low + 1) // 2
    assert m[lo:lo + n_low].all()
    return np.repeat((m != 0).astype(np.uint8)[None], t, 0), (lo, lo + n_low)


def phantom_slice(t, c, h, w, center_fraction, acceleration, seed, noise=0.01):
    """(fully sampled k-space (t, c, h, w) complex64, mask (t, h) uint8, masked k-space, ACS rows (lo, hi)): the noisy synthetic phantom
    of grappa_reference.phantom_slice under an equispaced mask."""
    k, _, _ = ref.phantom_slice(t, c, h, w, 2, noise=noise)
    mask, acs = equispaced_mask(t, h, center_fraction, acceleration, seed)
    return k, mask, (k * mask[:, None, :, None]).astype(np.complex64), acs
