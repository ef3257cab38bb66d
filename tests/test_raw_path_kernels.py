"""The first kernels a raw scan meets -- cine_raw_ingest (csrc/raw_ingest_kernels.hip), cine_coil_compress and cine_coil_gram
(csrc/coil_kernels.hip), cine_raw_window_ifft2c (csrc/raw_window_kernels.hip) and cine_espirit_gram (csrc/espirit_kernels.hip) -- called one by
one through the C ABI over their whole documented domain, against the float64 references of tests/raw_path_reference.py (the case lists, the
inputs, the bars; test_raw_path_kernels_cpu.py asserts what the lists reach).

  ingest        bit equality with scale * raw in float64 rounded once: the header promises ONE fp32 product per component
  compress      kernel_sweep.BAR of the float64 peak (at most 128 terms); the identity and a coil selection as matrix give the bits of raw
  gram          1e-9 of max |G_ref|, exactly Hermitian, the diagonal's imaginary part exactly 0
  window        1e-5 of the peak (all lengths <= 1024)
  espirit gram  1e-12 of max |G_ref|, exactly Hermitian

Every case: outputs between guard values and pre-filled with NaN (no NaN may be left); workspaces of exactly the size the library reports
with a sentinel tail, once filled with 0xFF bytes, once with 0x00 and once at a base pointer 64 bytes past a 256-byte boundary, the same bits
each time; inputs proven unchanged; a second call and storage offsets of 0, 4 and 12 floats give the same bits (cine_raw_window_ifft2c, which
asks for no more than the 8 bytes of a complex value, also at 2).  What a call must not read holds NaN: frames >= t_out / t_use, every sample
outside the calibration block of the two Gram matrices, the neighbours of the compression matrix.  Refusals write nothing."""
import time

import numpy as np
import pytest
import torch

import raw_path_reference as R
from kernel_sweep import (BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, Worst, at_offsets, case_id, check, refused, same_bits, stream)

pytestmark = pytest.mark.gpu
WORST = Worst()
OFFS = (0, 4, 12)                              # storage offsets in floats: every pointer stays 16-byte aligned
CODES = dict(EINVAL=EINVAL, EUNSUPPORTED=EUNSUPPORTED, EWORKSPACE=EWORKSPACE)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    t0 = time.perf_counter()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    if WORST:
        WORST.report()
    print(f"test_raw_path_kernels.py: {time.perf_counter() - t0:.1f} s")


def _pairs(z):
    """complex64 array -> float32 (..., 2) tensor of the same bits (NaN included)."""
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(z, np.complex64))).contiguous()


def _cplx(t):
    """float32 or float64 (..., 2) tensor -> complex128 array."""
    a = t.detach().cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def _peak_err(got, want):
    """max |d| / peak over the real and imaginary parts (conftest.rel_err on the pairs); NaN if anything is NaN."""
    d = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
    return float(d / max(np.abs(want.real).max(), np.abs(want.imag).max()))


def _runs(dev, body, what, offs=OFFS, workspace=True):
    """body(k, fill, past256) makes the call on the operands of the Call k and returns its output tensors.  Twice at every storage offset with
    the workspace filled with 0xFF; then with 0x00, and at a base pointer 64 bytes past a 256-byte boundary: the bits of the first run."""
    first = at_offsets(dev, offs, lambda k: body(k, 0xFF, None), what)
    for fill, past in ((0x00, None), (0xFF, 64)) if workspace else ():
        k = Call(dev, 0)
        outs = body(k, fill, past)
        k.finish(what)
        for a, b in zip(first, outs):
            assert same_bits(a, b.cpu()), f"{what}: other bits with the workspace filled with {fill:#04x} at base + {past}"
    return first


# ================================================================== cine_raw_ingest
def _ingest(k, raw, c, shape):
    x, o = k.inp(raw), k.out(shape)
    check(L().cine_raw_ingest(x.data_ptr(), o.ptr(), c["t_in"], c["nx"], c["ny"], c["c"], c["t_out"], c["scale"], stream()), "cine_raw_ingest")
    return [o.t]


@pytest.mark.parametrize("c", R.INGEST_CASES, ids=case_id)
def test_raw_ingest(dev, c):
    name = "cine_raw_ingest"
    z = R.ingest_input(c)
    raw, ref = _pairs(z), torch.from_numpy(R.ingest_ref(z, c["t_out"], c["scale"]))
    out, = _runs(dev, lambda k, fill, past: _ingest(k, raw, c, ref.shape), name, workspace=False)
    assert not bool(torch.isnan(out).any()), f"{name} {case_id(c)}: an element was never written"
    wrong = int((out.view(torch.int32) != ref.view(torch.int32)).sum())
    WORST.record(name + " (wrong elements)", float(wrong), 0.5, case_id(c))
    assert same_bits(out, ref)


def test_raw_ingest_takes_the_largest_coil_count(dev):
    """510 coils run (the CPU file pins the refusal of 511), over more than one tile and with a ragged last one."""
    c = dict(c=R.INGEST_COILS_MAX, nx=5, ny=7, t_in=1, t_out=1, scale=1e6)
    z = R.ingest_input(c)
    ref = torch.from_numpy(R.ingest_ref(z, 1, 1e6))
    out, = _runs(dev, lambda k, fill, past: _ingest(k, _pairs(z), c, ref.shape), "cine_raw_ingest", offs=(0,), workspace=False)
    assert same_bits(out, ref)


# ================================================================== cine_coil_compress
def _compress(k, raw, matrix, c, v):
    x, m = k.inp(raw), k.inp_among_nan(matrix)
    o = k.out((c["t_out"], c["nx"], c["ny"], v, 2))
    check(L().cine_coil_compress(x.data_ptr(), m.data_ptr(), o.ptr(), c["t_in"], c["nx"], c["ny"], c["c"], c["t_out"], v, stream()),
          "cine_coil_compress")
    return [o.t]


@pytest.mark.parametrize("c", R.COMPRESS_CASES, ids=case_id)
def test_coil_compress(dev, c):
    name = "cine_coil_compress"
    z, a = R.compress_input(c)
    want = R.compress_want(c)
    raw, matrix = _pairs(z), _pairs(a)
    offs = OFFS if z.size <= 1 << 20 else (0, 4)                           # the multi-tile cases move up to 68 MB per call
    out, = _runs(dev, lambda k, fill, past: _compress(k, raw, matrix, c, c["v"]), name, offs=offs, workspace=False)
    got = _cplx(out)
    assert not np.isnan(got).any(), f"{name} {case_id(c)}: an element was never written, or something outside the operands was read"
    WORST.record(name, _peak_err(got, want), BAR, case_id(c))


@pytest.mark.parametrize("nc", [1, 3, 32])
def test_coil_compress_identity_returns_the_bits(dev, nc):
    """A k-ordered fmaf chain started from zero: with the identity every output is one product with 1 plus zeros."""
    c = dict(c=nc, v=nc, t_in=2, t_out=1, nx=7, ny=29)
    z = R.poison_frames(R.crandn(nc, 2, 7, 29, nc), 1)
    out, = _runs(dev, lambda k, fill, past: _compress(k, _pairs(z), _pairs(np.eye(nc, dtype=np.complex64)), c, nc), "cine_coil_compress",
                 workspace=False)
    assert same_bits(out, _pairs(z[:1]))


@pytest.mark.parametrize("nc,v", [(5, 2), (33, 17), (128, 32), (127, 16)])
def test_coil_compress_selection_is_bit_exact(dev, nc, v):
    c = dict(c=nc, v=v, t_in=3, t_out=2, nx=9, ny=11)
    z = R.poison_frames(R.crandn(nc + v, 3, 9, 11, nc), 2)
    m, pick = R.selection_matrix(v, nc, nc)
    out, = _runs(dev, lambda k, fill, past: _compress(k, _pairs(z), _pairs(m), c, v), "cine_coil_compress", workspace=False)
    assert same_bits(out, _pairs(z[:2][..., pick]))


# ================================================================== cine_coil_gram
def _gram(k, raw, c, fill, past):
    lib = L()
    need = lib.cine_coil_gram_ws_bytes(c["t_use"], c["nx"], c["ny"], c["c"], c["region"])
    assert need > 0
    x, g, w = k.inp(raw), k.out64(2 * c["c"] * c["c"]), k.ws(need, past, fill)
    check(lib.cine_coil_gram(x.data_ptr(), g.ptr(), w.ptr(), w.nbytes, c["t_in"], c["nx"], c["ny"], c["c"], c["t_use"], c["region"], stream()),
          "cine_coil_gram")
    return [g.t]


@pytest.mark.parametrize("c", R.GRAM_CASES, ids=case_id)
def test_coil_gram(dev, c):
    name = "cine_coil_gram"
    z = R.gram_input(c)
    want = R.gram_ref(z, c["t_use"], c["region"])
    raw = _pairs(z)
    out, = _runs(dev, lambda k, fill, past: _gram(k, raw, c, fill, past), name)
    got = _cplx(out.view(c["c"], c["c"], 2))
    assert np.isfinite(got).all(), f"{name} {case_id(c)}: an entry was never written, or a sample outside the block or a later frame was read"
    WORST.record(name, float(np.abs(got - want).max() / np.abs(want).max()), R.BAR_GRAM, case_id(c))
    assert np.array_equal(got, got.conj().T), f"{name}: not exactly Hermitian"
    assert (got.diagonal().imag == 0).all(), f"{name}: the diagonal has an imaginary part"


# ================================================================== cine_raw_window_ifft2c
def _window(k, raw, c, fill, past):
    lib = L()
    need = lib.cine_raw_window_ws_bytes(c["t_out"], c["nx"], c["ny"], c["c"], c["cx"], c["cy"])
    assert need > 0
    x, o, w = k.inp(raw), k.out((c["t_out"], c["c"], c["cx"], c["cy"], 2)), k.ws(need, past, fill)
    check(lib.cine_raw_window_ifft2c(x.data_ptr(), o.ptr(), w.ptr(), w.nbytes, c["t_in"], c["nx"], c["ny"], c["c"], c["t_out"], c["cx"], c["cy"],
                                     c["scale"], stream()), "cine_raw_window_ifft2c")
    return [o.t]


@pytest.mark.parametrize("c", R.WINDOW_CASES, ids=case_id)
def test_raw_window_ifft2c(dev, c):
    name = "cine_raw_window_ifft2c"
    raw, want = _pairs(R.window_input(c)), R.window_want(c)
    out, = _runs(dev, lambda k, fill, past: _window(k, raw, c, fill, past), name, offs=OFFS + (2,))
    got = _cplx(out)
    assert not np.isnan(got).any(), f"{name} {case_id(c)}: an element was never written, or a frame >= t_out was read"
    WORST.record(name, _peak_err(got, want), R.BAR_WINDOW, case_id(c))


# ================================================================== cine_espirit_gram
def _espirit(k, kavg, c, fill, past):
    lib = L()
    n = c["kk"] * c["kk"] * c["c"]
    need = lib.cine_espirit_gram_ws_bytes(c["c"], c["ny"], c["nx"], c["r"], c["kk"])
    assert need > 0
    x, g, w = k.inp(kavg), k.out64(2 * n * n), k.ws(need, past, fill)
    check(lib.cine_espirit_gram(x.data_ptr(), g.ptr(), w.ptr(), w.nbytes, c["c"], c["ny"], c["nx"], c["r"], c["kk"], stream()), "cine_espirit_gram")
    return [g.t]


@pytest.mark.parametrize("c", R.ESPIRIT_CASES, ids=case_id)
def test_espirit_gram(dev, c):
    name = "cine_espirit_gram"
    z = R.espirit_input(c)
    want = R.espirit_gram_ref(z, c["r"], c["kk"])
    kavg, n = _pairs(z), c["kk"] * c["kk"] * c["c"]
    out, = _runs(dev, lambda k, fill, past: _espirit(k, kavg, c, fill, past), name, offs=OFFS if n <= 800 else (0, 4))
    got = _cplx(out.view(n, n, 2))
    assert np.isfinite(got).all(), f"{name} {case_id(c)}: an entry was never written, or a sample outside the block was read"
    WORST.record(name, float(np.abs(got - want).max() / np.abs(want).max()), R.BAR_ESPIRIT, case_id(c))
    assert np.array_equal(got, got.conj().T), f"{name}: not exactly Hermitian"
    assert (got.diagonal().imag == 0).all(), f"{name}: the diagonal has an imaginary part"


# ================================================================== refusals: decided on the host, nothing is written
def test_raw_ingest_refusals(dev):
    """Buffers sized for 511 coils on 16 samples, so every refused call would have stayed inside them."""
    lib, st, name = L(), stream(), "cine_raw_ingest"
    nc = R.INGEST_COILS_MAX + 1
    z = _pairs(R.crandn(1, 2, 1, 16, nc))
    k, k8 = Call(dev, 0), Call(dev, 2)
    x, o = k.inp(z), k.out((2, nc, 1, 16, 2))
    x8, o8 = k8.inp(z), k8.out((2, nc, 1, 16, 2))
    X, O = x.data_ptr(), o.ptr()

    def f(raw=X, out=O, t_in=2, c=3, t_out=1):
        return lambda: lib.cine_raw_ingest(raw, out, t_in, 1, 16, c, t_out, 1.0, st)
    refused(f(raw=x8.data_ptr()), EINVAL, k, f"{name} raw 8-byte aligned")
    refused(f(out=o8.ptr()), EINVAL, k8, f"{name} out 8-byte aligned")
    refused(f(c=nc), EUNSUPPORTED, k, f"{name} {nc} coils")
    refused(f(t_out=3), EINVAL, k, f"{name} t_out > t_in")
    refused(f(out=X), EINVAL, k, f"{name} out == raw")
    refused(f(raw=None), EINVAL, k, f"{name} raw NULL")
    refused(f(out=None), EINVAL, k, f"{name} out NULL")
    refused(f(c=0), EINVAL, k, f"{name} c=0")


def test_coil_compress_refusals(dev):
    """Buffers sized for 129 coils onto 33 on 16 samples."""
    lib, st, name = L(), stream(), "cine_coil_compress"
    z, a = _pairs(R.crandn(1, 2, 4, 4, 129)), _pairs(R.crandn(2, 33, 129))
    k, k8 = Call(dev, 0), Call(dev, 2)
    x, m, o = k.inp(z), k.inp_among_nan(a), k.out((2, 4, 4, 33, 2))
    x8, o8 = k8.inp(z), k8.out((2, 4, 4, 33, 2))
    X, M, O = x.data_ptr(), m.data_ptr(), o.ptr()

    def f(raw=X, mat=M, out=O, c=3, t_out=1, v=2):
        return lambda: lib.cine_coil_compress(raw, mat, out, 2, 4, 4, c, t_out, v, st)
    refused(f(raw=x8.data_ptr()), EINVAL, k, f"{name} raw 8-byte aligned")
    refused(f(out=o8.ptr()), EINVAL, k8, f"{name} out 8-byte aligned")
    refused(f(c=129), EUNSUPPORTED, k, f"{name} 129 coils")
    refused(f(c=64, v=33), EUNSUPPORTED, k, f"{name} 33 virtual coils")
    refused(f(v=4), EINVAL, k, f"{name} v > c")
    refused(f(v=0), EINVAL, k, f"{name} v=0")
    refused(f(t_out=3), EINVAL, k, f"{name} t_out > t_in")
    refused(f(out=X), EINVAL, k, f"{name} out == raw")
    refused(f(out=M), EINVAL, k, f"{name} out == matrix")
    refused(f(mat=X), EINVAL, k, f"{name} matrix == raw")
    for null in ("raw", "mat", "out"):
        refused(f(**{null: None}), EINVAL, k, f"{name} {null} NULL")


def test_coil_gram_refusals(dev):
    """Buffers sized for 129 coils on 16 samples; the workspace is the one of 128 coils."""
    lib, st, name = L(), stream(), "cine_coil_gram"
    z = _pairs(R.crandn(1, 2, 4, 4, 129))
    k, k8 = Call(dev, 0), Call(dev, 2)
    x, g, w = k.inp(z), k.out64(2 * 129 * 129), k.ws(lib.cine_coil_gram_ws_bytes(2, 4, 4, 128, 0))
    x8, g8 = k8.inp(z), k8.out64(2 * 129 * 129)
    X, G, W = x.data_ptr(), g.ptr(), w.ptr()
    need = lib.cine_coil_gram_ws_bytes(1, 4, 4, 3, 0)
    assert 0 < need <= w.nbytes and lib.cine_coil_gram_ws_bytes(1, 4, 4, 129, 0) == 0

    def f(raw=X, gram=G, ws=W, nbytes=w.nbytes, c=3, t_use=1):
        return lambda: lib.cine_coil_gram(raw, gram, ws, nbytes, 2, 4, 4, c, t_use, 0, st)
    refused(f(raw=x8.data_ptr()), EINVAL, k, f"{name} raw 8-byte aligned")
    refused(f(gram=g8.ptr()), EINVAL, k8, f"{name} gram 8-byte aligned")
    refused(f(ws=W + 8), EINVAL, k, f"{name} ws 8-byte aligned")
    refused(f(nbytes=need - 1), EWORKSPACE, k, f"{name} workspace one byte short")
    refused(f(c=129), EUNSUPPORTED, k, f"{name} 129 coils")
    refused(f(t_use=3), EINVAL, k, f"{name} t_use > t_in")
    refused(f(gram=X), EINVAL, k, f"{name} gram == raw")
    refused(f(ws=X), EINVAL, k, f"{name} ws == raw")
    refused(f(ws=G), EINVAL, k, f"{name} ws == gram")
    for null in ("raw", "gram", "ws"):
        refused(f(**{null: None}), EINVAL, k, f"{name} {null} NULL")


def test_raw_window_refusals(dev):
    lib, st, name = L(), stream(), "cine_raw_window_ifft2c"
    k = Call(dev, 0)
    x, o = k.inp(_pairs(R.crandn(1, 2, 6, 5, 3))), k.out((2, 3, 6, 5, 2))
    need = lib.cine_raw_window_ws_bytes(1, 6, 5, 3, 4, 3)
    w = k.ws(lib.cine_raw_window_ws_bytes(2, 6, 5, 3, 6, 5))
    X, O, W = x.data_ptr(), o.ptr(), w.ptr()
    assert 0 < need <= w.nbytes

    def f(raw=X, out=O, ws=W, nbytes=w.nbytes, t_out=1, cx=4, cy=3, c=3):
        return lambda: lib.cine_raw_window_ifft2c(raw, out, ws, nbytes, 2, 6, 5, c, t_out, cx, cy, 1.0, st)
    refused(f(nbytes=need - 1), EWORKSPACE, k, f"{name} workspace one byte short")
    refused(f(t_out=3), EINVAL, k, f"{name} t_out > t_in")
    refused(f(cx=7), EINVAL, k, f"{name} cx > nx")
    refused(f(cy=6), EINVAL, k, f"{name} cy > ny")
    refused(f(c=0), EINVAL, k, f"{name} c=0")
    refused(f(out=X), EINVAL, k, f"{name} out == raw")
    for null in ("raw", "out", "ws"):
        refused(f(**{null: None}), EINVAL, k, f"{name} {null} NULL")


def test_espirit_gram_refusals(dev):
    """Buffers sized for the largest refused shape: 33 coils on 40 x 40, n = 7 * 7 * 32."""
    lib, st, name = L(), stream(), "cine_espirit_gram"
    nmax = max(c["kk"] ** 2 * c["c"] for c, _ in R.ESPIRIT_REFUSED)
    k, k8 = Call(dev, 0), Call(dev, 2)
    x, g, w = k.inp(_pairs(R.crandn(1, 33, 40, 40))), k.out64(2 * nmax * nmax), k.ws(40 * 40 * 33 * 16)
    g8 = k8.out64(2 * 8 * 8)
    X, G, W = x.data_ptr(), g.ptr(), w.ptr()
    need = lib.cine_espirit_gram_ws_bytes(2, 8, 8, 6, 2)
    assert need == 6 * 6 * 2 * 16

    def f(kavg=X, gram=G, ws=W, nbytes=w.nbytes, c=2, ny=8, nx=8, r=6, kk=2):
        return lambda: lib.cine_espirit_gram(kavg, gram, ws, nbytes, c, ny, nx, r, kk, st)
    for c, code in R.ESPIRIT_REFUSED:
        refused(f(c=c["c"], ny=c["ny"], nx=c["nx"], r=c["r"], kk=c["kk"]), CODES[code], k, f"{name} {case_id(c)}")
    refused(f(gram=g8.ptr()), EINVAL, k8, f"{name} gram 8-byte aligned")
    refused(f(ws=W + 8), EINVAL, k, f"{name} ws 8-byte aligned")
    refused(f(kavg=X + 4), EINVAL, k, f"{name} kavg 4-byte aligned")
    refused(f(nbytes=need - 1), EWORKSPACE, k, f"{name} workspace one byte short")
    refused(f(gram=X), EINVAL, k, f"{name} gram == kavg")
    refused(f(ws=X), EINVAL, k, f"{name} ws == kavg")
    refused(f(ws=G), EINVAL, k, f"{name} ws == gram")
    for null in ("kavg", "gram", "ws"):
        refused(f(**{null: None}), EINVAL, k, f"{name} {null} NULL")
