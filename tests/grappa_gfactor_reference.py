"""The analytic GRAPPA noise map (Breuer et al., MRM 62:739, 2009) in float64 numpy, written from the formulas of include/cine_hip.h (not
from the kernels): the combined convolution kernel of the R - 1 lattice kernels, its image-domain weights, the g-factor and noise
amplitude of a linear coil combination, the circular application the closed form describes, and the error bounds of the fp32 kernels.

Notation of tests/grappa_reference.py: W (R - 1, ns, c) with W[m - 1][(j, dx, k)][q], hx = kx // 2, base = (ky // 2 - 1) R.
    K[q, k, dy, dx]:  K[., ., 0, 0] = I,  K[q, k, -m - base + j R, dx - hx] = W[m - 1][(j, dx, k)][q]
    Wimg[q, k](y, x) = sum K[q, k, dy, dx] exp(-2 pi i (dy (y - h // 2) / h + dx (x - w // 2) / w))
    amp^2 = p Wimg Psi Wimg^H p^H,  Psi = L L^H;   g = sqrt(amp^2 / (p Psi p^H)) / R, 0 where p Psi p^H is 0."""
import numpy as np

import grappa_reference as ref

U = 2.0 ** -24                 # one fp32 rounding
PHASE = 8                      # a phase factor of the kernels is within PHASE * U of exp(-2 pi i r / n): the argument 2 r / n is one
                               # rounded division (pi U of phase at most), sincospif is good to 2 ulp per component (2 sqrt(2) U)


def row_offsets(R, ky):
    """The distinct row offsets dy of the combined kernel in ascending order: 0 and -m - base + j R."""
    base = (ky // 2 - 1) * R
    return sorted({0} | {-m - base + j * R for m in range(1, R) for j in range(ky)})


def combined_kernel(W, c, R, ky, kx):
    """(K (c, c, ndy, kx) complex128 indexed [q, k, i, dx] with row offset dys[i] and column offset dx - hx, dys)."""
    W = np.asarray(W).astype(np.complex128).reshape(R - 1, ky, kx, c, c)          # [m - 1][j][dx][k][q]
    dys = row_offsets(R, ky)
    assert len(dys) == 1 + (R - 1) * ky
    base, hx = (ky // 2 - 1) * R, kx // 2
    K = np.zeros((c, c, len(dys), kx), np.complex128)
    K[:, :, dys.index(0), hx] = np.eye(c)
    for m in range(1, R):
        for j in range(ky):
            K[:, :, dys.index(-m - base + j * R), :] = W[m - 1, j].transpose(2, 1, 0)   # [dx][k][q] -> [q][k][dx]
    return K, dys


def phases(offsets, n):
    """E[i, p] = exp(-2 pi i offsets[i] (p - n // 2) / n) from the exactly reduced integer (offsets[i] (p - n // 2)) mod n."""
    rho = np.arange(n) - n // 2
    r = np.mod(np.asarray(offsets, np.int64)[:, None] * rho[None, :], n)
    return np.exp(-2j * np.pi * r / n)


def image_weights(W, c, R, ky, kx, h, w):
    """Wimg (c, c, h, w) complex128."""
    K, dys = combined_kernel(W, c, R, ky, kx)
    return np.einsum("qkab,ay,bx->qkyx", K, phases(dys, h), phases(np.arange(kx) - kx // 2, w), optimize=True)


def image_weights_bound(W, c, R, ky, kx):
    """(c, c): the bound of each component of the fp32 image weights, the same at every pixel.  A weight is sum_dx ex[dx] (sum_dy ey[dy]
    K[dy, dx]): two fmaf per complex term and component, a chain of ndy terms inside one of kx terms, one rounding per fmaf, two phase
    factors per term; every real product is at most |K| in modulus, so the bound is (2 ndy + 2 kx + 2 + 2 PHASE) U sum |K|."""
    K, dys = combined_kernel(W, c, R, ky, kx)
    return (2 * len(dys) + 2 * kx + 2 + 2 * PHASE) * U * np.abs(K).sum(axis=(2, 3))


def lower(chol, c):
    """L (c, c) complex128: the lower triangle of chol, the identity for None."""
    return np.eye(c, dtype=np.complex128) if chol is None else np.tril(np.asarray(chol).astype(np.complex128))


def gfactor(W, c, R, ky, kx, h, w, chol=None, coef=None, bound=False):
    """(g, amp), float64 of shape (n, h, w) with coef (n, c, h, w) or (c, h, w) without (p = e_q).  bound=True: also the bounds of the fp32
    kernel's g and amp.  With t_j = sum_{q, k} p_q Wimg[q, k] L[k, j] the kernel forms amp = sqrt(sum_j |t_j|^2): t_j is a chain of
    complex fmaf over dy (ndy terms), k (c), dx (kx) and q (c), two roundings per term and component, over terms whose moduli sum to
    M_j = sum |p_q| |K[q, k]| |L[k, j]|; the sum of 2 c squares and the root add (c + 3) U of amp.  The denominator sqrt(p Psi p^H) is
    the same with K = I.  g = sqrt(amp^2 / den^2) / R adds four roundings.  First order in U."""
    Wimg = image_weights(W, c, R, ky, kx, h, w)
    L = lower(chol, c)
    p = None if coef is None else np.asarray(coef).astype(np.complex128)
    if p is None:
        t = np.einsum("qkyx,kj->qjyx", Wimg, L, optimize=True)
        d = np.broadcast_to(L[:, :, None, None], (c, c, h, w))
    else:
        t = np.einsum("nqyx,qkyx,kj->njyx", p, Wimg, L, optimize=True)
        d = np.einsum("nqyx,qj->njyx", p, L, optimize=True)
    amp = np.sqrt((np.abs(t) ** 2).sum(1))
    den = np.sqrt((np.abs(d) ** 2).sum(1))
    safe = np.where(den > 0, den, 1.0)
    g = np.where(den > 0, amp / safe / R, 0.0)
    if not bound:
        return g, amp
    K, dys = combined_kernel(W, c, R, ky, kx)
    A, aL = np.abs(K).sum(axis=(2, 3)), np.abs(L)
    eps_t = (2 * len(dys) + 2 * c + 2 * kx + 2 * c + 2 + 2 * PHASE) * U
    eps_d = (2 * c + 2) * U
    if p is None:
        Mj = np.broadcast_to((A @ aL)[:, :, None, None], (c, c, h, w))
        Dj = np.broadcast_to(aL[:, :, None, None], (c, c, h, w))
    else:
        Mj = np.einsum("nqyx,qk,kj->njyx", np.abs(p), A, aL, optimize=True)
        Dj = np.einsum("nqyx,qj->njyx", np.abs(p), aL, optimize=True)
    amp_b = eps_t * np.sqrt((Mj ** 2).sum(1)) + (c + 3) * U * amp
    den_b = eps_d * np.sqrt((Dj ** 2).sum(1)) + (c + 3) * U * den
    g_b = np.where(den > 0, (amp_b / safe + amp * den_b / safe ** 2) / R + 4 * U * g, 0.0)
    return g, amp, g_b, amp_b


def circular_apply(z, W, R, ky, kx):
    """out[q, y, x] = sum K[q, k, dy, dx] z[k, (y + dy) mod h, (x + dx - hx) mod w] of z (c, h, w): what the closed form describes.  On a
    zero-filled lattice of any offset this is cine_grappa_apply (acquired rows kept, the others predicted) except that rows and columns
    outside the frame wrap around instead of reading as zero."""
    z = np.asarray(z).astype(np.complex128)
    c = z.shape[0]
    K, dys = combined_kernel(W, c, R, ky, kx)
    out = np.zeros_like(z)
    for i, dy in enumerate(dys):
        for dx in range(kx):
            out += np.einsum("qk,kyx->qyx", K[:, :, i, dx], np.roll(z, (-dy, -(dx - kx // 2)), axis=(1, 2)))
    return out


def ifft2c(x):
    return ref.ifft2c(x)
