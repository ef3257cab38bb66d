"""Pseudo-replica noise, on the host: the numpy restatement of the noise source (tests/noise_reference.py) against the Random123
known-answer vectors and against the law it claims, csrc/philox.h compiled with g++ against that restatement, the variance a linear
reconstruction must show, and the binding and argument refusals of cine_noise_add / cine_replica_accum / cine_replica_finish before
any launch.  Runs without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import noise_reference as R
from conftest import PKG, ROOT
from cine_hip import _lib
from kernel_sweep import BAR

EINVAL, EUNSUPPORTED = -1, -2
NAMES = ("cine_noise_add", "cine_replica_accum", "cine_replica_finish")

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_reference_reproduces_the_random123_vectors():
    for ctr, key, want in KAT:
        assert tuple(int(v) for v in R.philox4x32_10(ctr, key)) == want
    got = R.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))          # and vectorised
    assert np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint64))


def test_reference_uniforms_are_exact_float32_inside_their_ranges():
    a = np.array([0, 0x1ff, 0x200, 0xffffffff, 0x80000000], dtype=np.uint64)
    u1, u2 = R.uniforms(a, a)
    assert u1.min() == 2.0 ** -24 and u1.max() == 1 - 2.0 ** -24 and u2.min() == 0.0 and u2.max() == 1 - 2.0 ** -24
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)


def test_philox_header_host_check(tmp_path):
    """csrc/philox.h under g++: the three vectors, then 4096 points from point0 = 2^32 - 3 (the carry into the high counter word):
    words and uniforms identical to the restatement, normals within BAR of its float64 ones."""
    exe, dump = str(tmp_path / "philox_host_check"), str(tmp_path / "dump.bin")
    src = os.path.join(ROOT, "tests", "host", "philox_host_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(PKG, "csrc"), src, "-o", exe], check=True)
    seed, replica, point0, n, c = 0x123456789ABCDEF, 3, 2 ** 32 - 3, 4096, 5
    out = subprocess.run([exe, str(seed), str(replica), str(point0), str(n), str(c), dump], check=True, capture_output=True, text=True).stdout
    assert "known-answer vectors ok" in out and f"wrote {n} points x {c} coils" in out
    rec = np.fromfile(dump, dtype=np.dtype([("a", "<u4"), ("b", "<u4"), ("u1", "<f4"), ("u2", "<f4"), ("re", "<f4"), ("im", "<f4")])).reshape(n, c)
    p = np.uint64(point0) + np.arange(n, dtype=np.uint64)
    assert int(p[2]) >> 32 == 0 and int(p[3]) >> 32 == 1                      # the run crosses the carry
    a, b = R.words(seed, replica, p, c)
    assert np.array_equal(rec["a"].astype(np.uint64), a) and np.array_equal(rec["b"].astype(np.uint64), b)
    u1, u2 = R.uniforms(a, b)
    assert np.array_equal(rec["u1"].astype(np.float64), u1) and np.array_equal(rec["u2"].astype(np.float64), u2)
    z = R.normals(seed, replica, p, c)
    err = np.abs((rec["re"].astype(np.float64) + 1j * rec["im"].astype(np.float64)) - z).max() / np.abs(z).max()
    print(f"philox.h normals vs float64: {err:.3e} of the largest")
    assert err <= BAR
    # a point of the second 2^32 block is not the point 2^32 below it
    assert not np.array_equal(R.words(seed, replica, p[3:4], c)[0], R.words(seed, replica, p[3:4] - np.uint64(2 ** 32), c)[0])


@pytest.mark.parametrize("c,m", [(5, 2 ** 14), (8, 2 ** 16), (15, 2 ** 16)])
def test_reference_normals_are_white_with_unit_power(c, m):
    """z of M points x c coils: || z z^H / M - I ||_F <= 2 c / sqrt(M); the expectation is c / sqrt(M)."""
    z = R.normals(12345, 3, np.arange(m, dtype=np.uint64), c)                 # (M, c)
    cov = z.T @ z.conj() / m
    dev = np.linalg.norm(cov - np.eye(c)) * np.sqrt(m) / c
    print(f"c {c} M {m}: ||zz^H/M - I||_F = {dev:.3f} c/sqrt(M)")
    assert dev <= 2.0
    assert abs(np.mean(z * z)) <= 4.0 / np.sqrt(m * c)                        # circular: E z^2 = 0


def test_reference_streams_differ_by_seed_replica_point_and_coil():
    p = np.arange(64, dtype=np.uint64)
    base = R.words(7, 2, p, 4)[0]
    assert not (base == R.words(8, 2, p, 4)[0]).any() and not (base == R.words(7, 3, p, 4)[0]).any()
    assert not (base == R.words(7 + 2 ** 32, 2, p, 4)[0]).any()               # the seed's high half is in the key
    assert not (base[:-1] == base[1:]).any() and not (base[:, 0] == base[:, 1]).any() and not (base[:, 0] == base[:, 2]).any()
    assert np.array_equal(R.words(-1, 2, p, 4)[0], R.words(2 ** 64 - 1, 2, p, 4)[0])      # a negative long is its 64 bits


def linear_case(t, c, h, w, seed):
    """Random maps S (t-independent), a random Psi = L L^H, and S^H Psi S per pixel."""
    rs = np.random.RandomState(1000 + c * 31 + h)
    sens = (rs.standard_normal((c, h, w)) + 1j * rs.standard_normal((c, h, w))) / np.sqrt(2 * c)
    low, psi = R.random_chol(rs, c)
    want = np.einsum("chw,cd,dhw->hw", sens.conj(), psi, sens).real           # S^H Psi S with x = sum_c conj(S_c) n_c
    return sens, low, psi, want


def linear_recon(k, sens):
    """x = sum_c conj(S_c) IFFT2_ortho(k_c): (t, c, h, w) -> (t, h, w); uncentred transforms (unitary either way)."""
    return (sens.conj()[None] * np.fft.ifft2(k, norm="ortho")).sum(axis=1)


@pytest.mark.parametrize("t,c,h,w", [(4, 4, 16, 12), (3, 5, 7, 13)])
def test_variance_of_a_linear_reconstruction(t, c, h, w):
    """64 replicas of pure noise through a linear reconstruction: the mean over pixels of (sample variance / S^H Psi S) is within
    4 / sqrt(N P) of 1, P = t h w."""
    n_rep, seed = 64, 7
    sens, low, psi, want = linear_case(t, c, h, w, seed)
    acc = R.Welford()
    for r in range(n_rep):
        x = linear_recon(R.noise(t, c, h, w, seed=seed, replica=r, chol=low), sens)
        acc.add(np.stack([x.real, x.imag], axis=-1))
    _, std, _, _ = acc.finish(pairs=True)
    ratio = (std ** 2 / want[None]).mean()
    sigma = 1.0 / np.sqrt(n_rep * t * h * w)
    print(f"({t},{c},{h},{w}): mean var / S^H Psi S = {ratio:.5f}, {abs(ratio - 1) / sigma:.2f} of 1/sqrt(N P)")
    assert abs(ratio - 1.0) <= 4.0 * sigma


def test_welford_restatement_is_the_two_pass_variance():
    rs = np.random.RandomState(3)
    x = rs.standard_normal((9, 17)) * 3 + 50
    acc = R.Welford()
    for row in x:
        acc.add(row)
    mean, std, snr, g = acc.finish(ref_std=np.full(17, 2.0), accel=4.0)
    assert np.allclose(mean, x.mean(0), rtol=1e-13) and np.allclose(std, x.std(0, ddof=1), rtol=1e-12)
    assert np.allclose(snr, np.abs(mean) / std) and np.allclose(g, std / 4.0)


# ------------------------------------------------------------------ the three entry points through the library, before any launch
def test_symbols_are_declared_exported_and_bound():
    i, lg, f, p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(_lib.lib(), name)
    assert _lib._SIGS["cine_noise_add"] == (i, [p, p, p, i, p, f, lg, lg, p, lg, lg, i, i, i, p])
    assert _lib._SIGS["cine_replica_accum"] == (i, [p, p, p, lg, i, p])
    assert _lib._SIGS["cine_replica_finish"] == (i, [p, p, lg, i, i, p, f, p, p, p, p, p])


P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]                      # never dereferenced


def test_noise_add_rejects_bad_arguments_before_any_launch():
    L = _lib.lib()

    def call(k=P[0], out=P[1], mask=P[2], mask_w=1, chol=P[3], scale=1.0, seed=5, replica=0, rdev=None, point0=0, bt=2, c=4, h=8, w=6):
        return L.cine_noise_add(k, out, mask, mask_w, chol, scale, seed, replica, rdev, point0, bt, c, h, w, None)

    assert call(c=65) == EUNSUPPORTED and b"64" in L.cine_last_error() and L.cine_last_error().startswith(b"cine_noise_add")
    assert call(c=128, chol=None) == EUNSUPPORTED
    assert call(mask_w=2) == EINVAL and b"mask_w" in L.cine_last_error()
    assert call(mask_w=2, mask=None) == EINVAL and call(mask_w=0) == EINVAL
    assert call(replica=-1) == EINVAL and b"replica" in L.cine_last_error()
    assert call(replica=2 ** 32) == EINVAL and call(point0=-1) == EINVAL
    for kw in (dict(k=None), dict(out=None)):
        assert call(**kw) == EINVAL and b"null" in L.cine_last_error(), kw
    for kw in (dict(bt=0), dict(c=0), dict(h=0), dict(w=-1), dict(bt=-3)):
        assert call(**kw) == EINVAL, kw
    nbytes = 2 * 4 * 8 * 6 * 8
    assert call(out=ctypes.c_void_p(0x1000 + 8)) == EINVAL and b"overlaps" in L.cine_last_error()
    assert call(out=ctypes.c_void_p(0x1000 + nbytes - 8)) == EINVAL and call(k=ctypes.c_void_p(0x2000), out=ctypes.c_void_p(0x2000 - 8)) == EINVAL
    assert call(k=ctypes.c_void_p(0x1004)) == EINVAL and b"aligned" in L.cine_last_error()
    assert call(chol=ctypes.c_void_p(0x4004)) == EINVAL and call(rdev=ctypes.c_void_p(0x5004)) == EINVAL


def test_replica_statistics_reject_bad_arguments_before_any_launch():
    L = _lib.lib()

    def accum(x=P[0], mean=P[1], m2=P[2], n=10, k=1):
        return L.cine_replica_accum(x, mean, m2, n, k, None)

    for kw in (dict(x=None), dict(mean=None), dict(m2=None)):
        assert accum(**kw) == EINVAL and L.cine_last_error().startswith(b"cine_replica_accum"), kw
    assert accum(n=0) == EINVAL and accum(k=0) == EINVAL and accum(k=-2) == EINVAL and accum(m2=P[1]) == EINVAL

    def finish(mean=P[0], m2=P[1], n=10, k=2, pairs=0, ref=P[2], accel=4.0, o=(P[3], P[4], P[5], P[6])):
        return L.cine_replica_finish(mean, m2, n, k, pairs, ref, accel, *o, None)

    assert finish(k=1) == EINVAL and L.cine_last_error().startswith(b"cine_replica_finish") and b"two samples" in L.cine_last_error()
    assert finish(ref=None) == EINVAL and b"g_out needs ref_std" in L.cine_last_error()
    assert finish(accel=0.0) == EINVAL and finish(accel=-1.0) == EINVAL
    assert finish(mean=None) == EINVAL and finish(m2=None) == EINVAL and finish(n=0) == EINVAL
    assert finish(n=9, pairs=1) == EINVAL and b"odd" in L.cine_last_error()


def test_python_layer_refuses_without_a_gpu_or_with_bad_arguments():
    import torch
    from cine_hip import noise as N
    from cine_hip._lib import CineHipError
    import cine_hip
    assert cine_hip.noise is N
    assert N.noise_cholesky(sigma=0.5) == (None, 0.5)
    with pytest.raises(ValueError, match="one of the three"):
        N.noise_cholesky()
    with pytest.raises(ValueError, match="not finite"):
        N.noise_cholesky(torch.full((3, 3), float("nan"), dtype=torch.complex128))
    with pytest.raises(ValueError, match="not positive definite"):
        N.noise_cholesky(torch.ones(3, 3, dtype=torch.complex128))
    with pytest.raises(ValueError, match="not Hermitian"):
        N.noise_cholesky(torch.triu(torch.ones(3, 3, dtype=torch.complex128)))
    with pytest.raises(CineHipError, match="no CPU fallback"):
        N.add_noise(torch.zeros(2, 3, 4, 5, 2), None)
    with pytest.raises(CineHipError, match="requires grad"):
        N.add_noise(torch.zeros(2, 3, 4, 5, 2, requires_grad=True), None)
    assert N.NoiseSpec() == (None, 1.0, 0, 0) and N.NoiseSpec(seed=3, replica=9).replica == 9
    assert N._as_long(2 ** 64 - 1) == -1 and N._as_long(-1) == -1 and N._as_long(2 ** 63) == -2 ** 63 and N._as_long(5) == 5
