"""GRAPPA / TGRAPPA in float64 numpy, written from the definitions of include/cine_hip.h (not from the kernels): lattice offsets,
calibration data, the augmented patch matrix P, G = P^H P, the weights, their application and the whole reconstruction.

k-space of a slice is (t, c, h, w) complex, the mask (t, h); R the acceleration, the kernel ky x kx, hx = kx // 2, ns = ky kx c sources
in the order (j, dx, coil), span = (ky - 1) R + 1, base = (ky // 2 - 1) R."""
import numpy as np


def geom(c, R, ky, kx):
    return {"ns": ky * kx * c, "nr": (R - 1) * c, "n_aug": ky * kx * c + (R - 1) * c, "span": (ky - 1) * R + 1, "base": (ky // 2 - 1) * R,
            "hx": kx // 2}


def lattice_mask(t, h, R, acs=0, interleave=True, offsets=None):
    m = np.zeros((t, h), np.uint8)
    for f in range(t):
        off = offsets[f] if offsets is not None else (f % R if interleave else 0)
        m[f, off::R] = 1
    if acs:
        lo = h // 2 - acs // 2
        m[:, lo:lo + acs] = 1
    return m


def offsets(mask, R):
    """(offsets, status) per frame: the lowest residue whose rows are all acquired, -1 / 1 without one."""
    mask = np.asarray(mask) != 0
    off = np.full(mask.shape[0], -1, np.int32)
    for f in range(mask.shape[0]):
        for r in range(R):
            if mask[f, r::R].all():
                off[f] = r
                break
    return off, (off < 0).astype(np.int32)


def tgrappa_average(kspace, mask):
    """Per-row average over the frames that acquired the row, (c, h, w) complex128; rows nobody acquired stay zero.  Also the counts (h,)."""
    m = (np.asarray(mask) != 0).astype(np.float64)                       # (t, h)
    k = np.asarray(kspace).astype(np.complex128)
    total = (k * m[:, None, :, None]).sum(0)
    count = m.sum(0)
    return total / np.maximum(count, 1.0)[None, :, None], count


def calibration_data(kspace, mask, calib="auto", acs=None, calib_rows=32):
    """(c, hc, w) complex64 calibration array of a masked slice (t, c, h, w)."""
    if calib == "auto":
        calib = "acs" if acs is not None else "tgrappa"
    avg, count = tgrappa_average(kspace, mask)
    h = avg.shape[1]
    if calib == "acs":
        lo, hi = acs
    else:
        n = min(calib_rows, h)
        lo = h // 2 - n // 2
        hi = lo + n
    if not (count[lo:hi] > 0).all():
        raise ValueError("a row of the calibration block was acquired by no frame")
    return avg[:, lo:hi].astype(np.complex64)


def patch_matrix(cal, R, ky, kx):
    """P (n_pos, n_aug) complex128: one row per window position y in [0, hc - span], x in [hx, w - hx), y-major."""
    cal = np.asarray(cal).astype(np.complex128)
    c, hc, w = cal.shape
    g = geom(c, R, ky, kx)
    my, mx = hc - g["span"] + 1, w - kx + 1
    cols = []
    for j in range(ky):
        for dx in range(kx):
            cols.append(cal[:, j * R:j * R + my, dx:dx + mx])                              # (c, my, mx): x + dx - hx, x = hx + x'
    for m in range(1, R):
        cols.append(cal[:, g["base"] + m:g["base"] + m + my, g["hx"]:g["hx"] + mx])
    P = np.stack(cols, 0)                                                                   # (taps, c, my, mx)
    return P.reshape(-1, my * mx).T.copy()


def gram(cal, R, ky, kx):
    P = patch_matrix(cal, R, ky, kx)
    return P.conj().T @ P


def gram_bounds(cal, R, ky, kx):
    """(bound of the real parts, bound of the imaginary parts): n_pos 2^-52 sum |terms| per entry, the bound of a float64 sum of the
    n_pos exact complex products conj(u) v = (ur vr + ui vi) + i (ur vi - ui vr)."""
    P = patch_matrix(cal, R, ky, kx)
    Pr, Pi = np.abs(P.real), np.abs(P.imag)
    scale = P.shape[0] * 2.0 ** -52
    return scale * (Pr.T @ Pr + Pi.T @ Pi), scale * (Pr.T @ Pi + Pi.T @ Pr)


def weights(G, c, R, ky, kx, lam):
    """(W (R - 1, ns, c) complex128, info [residual, tau, fit, trace]) from the complex128 Gram matrix."""
    g = geom(c, R, ky, kx)
    ns = g["ns"]
    G = np.asarray(G).astype(np.complex128)
    Gss, Gst, Gtt = G[:ns, :ns], G[:ns, ns:], G[ns:, ns:]
    tr = float(np.trace(Gss).real)
    tau = lam * tr / ns
    if tr == 0.0:
        return np.zeros((R - 1, ns, c), np.complex128), np.array([0.0, tau, 0.0, tr])
    A = Gss + tau * np.eye(ns)
    W = np.linalg.solve(A, Gst)
    nb = np.linalg.norm(Gst)
    resid = np.linalg.norm(A @ W - Gst) / nb if nb > 0 else 0.0
    ttr = float(np.trace(Gtt).real)
    fit = np.sqrt(max(0.0, float(np.trace(Gtt - W.conj().T @ Gst).real)) / ttr) if ttr > 0 else 0.0
    return W.reshape(ns, R - 1, c).transpose(1, 0, 2).copy(), np.array([resid, tau, fit, tr])


def source_matrix(frame, rows, kx):
    """S (w, len(rows) kx c) of one frame (c, h, w): S[x][(j, dx, k)] = frame[k, rows[j], x + dx - hx], zero outside the frame."""
    c, h, w = frame.shape
    hx = kx // 2
    pad = np.zeros((c, len(rows), w + 2 * hx), frame.dtype)
    for j, r in enumerate(rows):
        if 0 <= r < h:
            pad[:, j, hx:hx + w] = frame[:, r]
    S = np.empty((w, len(rows), kx, c), frame.dtype)
    for dx in range(kx):
        S[:, :, dx, :] = pad[:, :, dx:dx + w].transpose(2, 1, 0)
    return S.reshape(w, -1)


def apply(kspace, W, mask, offs, R, ky, kx, bound=False):
    """The filled k-space (t, c, h, w) complex128; acquired rows and frames with offset -1 are kept.  bound=True: also sum |w| |x| of the
    real products that make up each output component, as a complex array (real part: of the real component, imaginary part: of the
    imaginary one); 0 where nothing is computed."""
    k = np.asarray(kspace)
    t, c, h, w = k.shape
    g = geom(c, R, ky, kx)
    out = k.astype(np.complex128).copy()
    mag = np.zeros(out.shape, np.complex128) if bound else None
    W = np.asarray(W).astype(np.complex128)
    for f in range(t):
        off = int(offs[f])
        if off < 0:
            continue
        for y in range(h):
            if mask[f, y]:
                continue
            m = (y - off) % R
            assert 1 <= m < R
            rows = [y - m - g["base"] + j * R for j in range(ky)]
            for r in rows:
                assert not (0 <= r < h) or mask[f, r], "a source row that is not acquired"
            S = source_matrix(k[f], rows, kx).astype(np.complex128)
            out[f, :, y, :] = (S @ W[m - 1]).T
            if bound:
                Sr, Si, Wr, Wi = np.abs(S.real), np.abs(S.imag), np.abs(W[m - 1].real), np.abs(W[m - 1].imag)
                mag[f, :, y, :] = ((Sr @ Wr + Si @ Wi) + 1j * (Sr @ Wi + Si @ Wr)).T
    return (out, mag) if bound else out


def ifft2c(x):
    ax = (-2, -1)
    return np.fft.fftshift(np.fft.ifft2(np.fft.ifftshift(x, axes=ax), norm="ortho"), axes=ax)


def rss(kspace):
    return np.sqrt((np.abs(ifft2c(kspace)) ** 2).sum(-3))


def grappa(kspace, mask, R, kernel=(2, 5), lam=1e-4, calib="auto", acs=None, calib_rows=32):
    """(filled k-space (t, c, h, w) complex128, info, offsets) of one masked slice; the weights are rounded to complex64 once."""
    ky, kx = kernel
    k = np.asarray(kspace)
    off, status = offsets(mask, R)
    if status.any():
        raise ValueError(f"frame {int(np.argmax(status))} has no lattice of step {R}")
    cal = calibration_data(k, mask, calib, acs, calib_rows)
    W, info = weights(gram(cal, R, ky, kx), k.shape[1], R, ky, kx, lam)
    return apply(k, W.astype(np.complex64), mask, off, R, ky, kx), info, off


def nrmse(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


def phantom_slice(t, c, h, w, R, acs=0, noise=0.01):
    """(fully sampled k-space (t, c, h, w) complex64, mask (t, h) uint8, masked k-space): the synthetic phantom with complex white noise of
    standard deviation `noise` per component from RandomState(1), under an interleaved lattice."""
    from cine_hip import synth
    img = synth.cine_phantom(t, h, w)
    sens = synth.coil_maps(c, h, w)
    k = synth._fft2c_np(img[:, None] * sens[None])
    rs = np.random.RandomState(1)
    k = (k + noise * (rs.standard_normal(k.shape) + 1j * rs.standard_normal(k.shape))).astype(np.complex64)
    mask = lattice_mask(t, h, R, acs=acs)
    return k, mask, (k * mask[:, None, :, None]).astype(np.complex64)
