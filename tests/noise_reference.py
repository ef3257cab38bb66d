"""The noise source of cine_noise_add and the replica statistics restated in numpy, from the definition in include/cine_hip.h (not from
csrc/philox.h): Philox4x32-10 in uint64 arithmetic, the uniforms, Box-Muller and the Cholesky colouring in float64, Welford's update
and the maps of cine_replica_finish in float64.  The yardstick of tests/test_noise_cpu.py, test_noise_kernels.py and
test_noise_replicas.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) of 32-bit words (any integer dtype, broadcast against each other) -> (..., 4) uint64 words."""
    counter = np.asarray(counter, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (counter[..., i] & LO for i in range(4))
    k0, k1 = key[..., 0] & LO, key[..., 1] & LO
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                                     # 32 x 32 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO, (p0 >> S32) ^ c3 ^ k1, p0 & LO
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def words(seed, replica, p, c):
    """The words (a, b) of every coil of the points p (uint64 array): two uint64 arrays p.shape + (c,)."""
    p = np.asarray(p, dtype=np.uint64)
    s = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    key = np.array([s & LO, s >> S32], dtype=np.uint64)
    npair = (c + 1) // 2
    ctr = np.empty(p.shape + (npair, 4), dtype=np.uint64)
    ctr[..., 0] = (p & LO)[..., None]
    ctr[..., 1] = (p >> S32)[..., None]
    ctr[..., 2] = np.uint64(int(replica))
    ctr[..., 3] = np.arange(npair, dtype=np.uint64)
    x = philox4x32_10(ctr, key)                                       # (..., npair, 4)
    a = x[..., 0::2].reshape(p.shape + (2 * npair,))[..., :c]         # coil 2j: x0, coil 2j+1: x2
    b = x[..., 1::2].reshape(p.shape + (2 * npair,))[..., :c]
    return a, b


def uniforms(a, b):
    """u1 in [2^-24, 1 - 2^-24], u2 in [0, 1) as float64 (both are exact float32 values)."""
    u1 = ((a >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normals(seed, replica, p, c):
    """z (p.shape + (c,)) complex128, E|z|^2 = 1."""
    u1, u2 = uniforms(*words(seed, replica, p, c))
    return np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)


def points(bt, h, w, point0=0):
    """p of every (frame, y, x): uint64 (bt, h, w)."""
    return np.uint64(point0) + np.arange(bt * h * w, dtype=np.uint64).reshape(bt, h, w)


def noise(bt, c, h, w, seed=0, replica=0, chol=None, scale=1.0, point0=0):
    """eta (bt, c, h, w) complex128 at EVERY point: scale * L z with the lower triangle of chol (c, c), or scale * z."""
    z = normals(seed, replica, points(bt, h, w, point0), c)          # (bt, h, w, c)
    if chol is not None:
        z = z @ np.tril(np.asarray(chol, dtype=np.complex128)).T     # eta_i = sum_k L[i, k] z_k
    return scale * np.moveaxis(z, -1, 1)


def sampled(mask, bt, h, w):
    """A mask (bt, h), (bt, h, w) or None as bool (bt, 1, h, w)."""
    if mask is None:
        return np.ones((bt, 1, h, w), dtype=bool)
    m = np.asarray(mask).astype(bool)
    m = m.reshape(bt, h, 1) if m.ndim == 2 else m.reshape(bt, h, w)
    return np.broadcast_to(m[:, None], (bt, 1, h, w))


def noise_add(kspace, mask, **kw):
    """kspace (bt, c, h, w) complex -> kspace + eta at the sampled points (complex128), and eta itself there (0 elsewhere)."""
    bt, c, h, w = kspace.shape
    eta = noise(bt, c, h, w, **kw) * sampled(mask, bt, h, w)
    return kspace.astype(np.complex128) + eta, eta


class Welford:
    """d = x - mean; mean += d / k; m2 += d * (x - mean), float64."""

    def __init__(self):
        self.k, self.mean, self.m2 = 0, None, None

    def add(self, x):
        x = np.asarray(x, dtype=np.float64)
        self.k += 1
        if self.k == 1:
            self.mean, self.m2 = x.copy(), np.zeros_like(x)
            return
        d = x - self.mean
        self.mean = self.mean + d / self.k
        self.m2 = self.m2 + d * (x - self.mean)

    def finish(self, pairs=False, ref_std=None, accel=None):
        """(mean, std, snr, g) in float64; pairs: the last axis of length 2 is (re, im)."""
        var = self.m2 / (self.k - 1)
        if pairs:
            var = var[..., 0] + var[..., 1]
            mean = np.hypot(self.mean[..., 0], self.mean[..., 1])
        else:
            mean = self.mean
        std = np.sqrt(var)
        with np.errstate(divide="ignore", invalid="ignore"):
            snr = np.where(std == 0, 0.0, np.abs(mean) / std)
            g = None
            if ref_std is not None:
                ref = np.asarray(ref_std, dtype=np.float64)
                g = np.where(ref == 0, 0.0, std / (ref * np.sqrt(float(accel))))
        return mean, std, snr, g


def random_chol(rs, c):
    """A well-conditioned lower-triangular complex64 L with a real positive diagonal, and Psi = L L^H (complex128)."""
    a = (rs.standard_normal((c, 2 * c)) + 1j * rs.standard_normal((c, 2 * c))) / np.sqrt(4 * c)
    psi = a @ a.conj().T + 0.25 * np.eye(c)
    low = np.linalg.cholesky(psi).astype(np.complex64)
    return low, low.astype(np.complex128) @ low.astype(np.complex128).conj().T
