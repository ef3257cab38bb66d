"""The steps in front of the hot path, on the device.

``prepare_slice``   reference data/mri_data.py:283-293, 302-303: raw k-space -> image space -> crop, frame selection,
                    Gaussian filter (data/transforms.py:186-220) -> k-space of the filtered crop, and the coil-combined
                    magnitude target.
``coil_gram`` / ``coil_matrix_from_gram`` / ``compress_coils``
                    SVD coil compression of the raw data (Buehrer et al., MRM 57:1131, 2007; Huang et al., MRI 26:133, 2008): the c
                    physical coils projected onto V virtual coils BEFORE the inverse transform.  The reference has no such step; here
                    it gives every scan of a data set the same shape (one SlicePipeline graph set) and lifts the 32-coil cap of the
                    calibration.  ``prepare_slice(..., virtual_coils=V)`` runs it in place.  ``method="jacobi"`` takes the eigenvectors
                    from cine_coil_matrix (a Jacobi eigensolver in LDS) instead of torch.linalg.eigh: no host read, capturable, what
                    ``prepare_masked_slice(..., virtual_coils=V)`` and ``SlicePipeline.submit_raw(..., virtual_coils=V)`` run per slice.
``noise_covariance`` / ``noise_whitener``
                    noise pre-whitening, the first step of a raw-data front-end (Gadgetron, BART): from a scan's noise samples the
                    covariance Psi = L L^H and the whitener W = s L^-1, once per scan.  ``whitener=W`` folds it into the compression
                    matrix (``coil_matrix_from_gram``; "jacobi": cine_coil_matrix_whitened, per slice, no host read), so the one
                    pass of ``compress_coils`` whitens and compresses: SVD compression, ESPIRiT's threshold and the least-squares
                    data terms behind it all assume white noise.
``prepare_masked_slice``
                    prepare_slice's k-space with the row mask applied, device in, device out, capturable by a hipGraph: what
                    ``SlicePipeline.submit_raw`` runs per slice.  Line-engine raw sizes enter through ops.raw_ingest (kept frames only).
``espirit_maps``    what the reference gets from the BART toolbox (``bart ecalib -r N``, mri_data.py:296,
                    transforms.py:429): ESPIRiT sensitivity maps (Uecker et al., MRM 71:990-1001, 2014) with ecalib's
                    defaults -- 6 x 6 kernels, singular-value threshold 0.001, eigenvalue crop 0.8, first map.
                    ``method="sign"`` takes the projector from a matrix sign function on the float64 matrix cores instead of an
                    eigen-decomposition (``espirit_gram``, ``espirit_projector``): no host read, capturable, what ``SlicePipeline`` runs
                    for ``sens_maps="espirit"`` on ``time_average`` of the slice.
``ecalib``          the same behind ecalib's array convention ((1, x, y, coil) complex in, (x, y, coil) out), so the
                    reference's two call sites change by one line.

Arithmetic runs in libcine_hip.so (crop / filter / FFT / lag kernels / per-pixel eigen-iteration).  The two small dense
steps of the calibration -- the Gram matrix of the k-space patches and its Hermitian eigen-decomposition (k*k*coils square,
540 for 15 coils) -- are library calls on the same device (torch.matmul -> rocBLAS, torch.linalg.eigh -> hipSOLVER) in
complex128: the threshold keeps singular values down to 1e-3 of the largest, i.e. Gram eigenvalues down to 1e-6.
"""
from typing import Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import CineHipError, check, lib


def _c2r(x: torch.Tensor) -> torch.Tensor:
    """complex64 tensor -> float32 (..., 2) pairs (a view)."""
    return torch.view_as_real(x) if x.is_complex() else x


def crop_select(x: torch.Tensor, n_slices: int, shape: Sequence[int]) -> torch.Tensor:
    """x (t, c, h, w, 2) -> (n_slices, c, shape[0], shape[1], 2): data[:n_slices, :, centered crop] (transforms.py:209-214)."""
    x = ops._dev(x, "crop_select input")
    t, c, h, w, _ = x.shape
    if not (0 < shape[0] <= h and 0 < shape[1] <= w):
        raise ValueError("Invalid shapes.")                                  # transforms.py:206-207
    n_slices = min(int(n_slices), t)
    out = torch.empty((n_slices, c, shape[0], shape[1], 2), device=x.device, dtype=x.dtype)
    check(lib().cine_crop_select(x.data_ptr(), out.data_ptr(), t, c, h, w, n_slices, shape[0], shape[1], ops._stream()), "cine_crop_select")
    return out


def gaussian_filter(x: torch.Tensor, sigma: Sequence[float]) -> torch.Tensor:
    """scipy.ndimage.gaussian_filter(x.real / x.imag, sigma) over the leading len(sigma) axes of x (..., 2), as
    transforms.py:216-218 applies it (one pass per axis with sigma > 0, in axis order)."""
    x = ops._dev(x, "gaussian_filter input")
    if len(sigma) != x.dim() - 1:
        raise ValueError("one sigma per axis")
    cur = x
    for ax, s in enumerate(sigma):
        if float(s) <= 1e-15:
            continue
        outer = 1
        for d in cur.shape[:ax]:
            outer *= d
        inner = 1
        for d in cur.shape[ax + 1:-1]:
            inner *= d
        nxt = torch.empty_like(cur)
        check(lib().cine_gauss_axis(cur.data_ptr(), nxt.data_ptr(), outer, cur.shape[ax], inner, float(s), ops._stream()), "cine_gauss_axis")
        cur = nxt
    return cur.clone() if cur is x else cur


def filtered_crop_center_and_slices(data: torch.Tensor, shape, n_slices: int, filter_size) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device form of reference data/transforms.py:186-220 for (t, c, h, w, 2) float32 pairs."""
    crop = crop_select(data, n_slices, shape)
    return crop, gaussian_filter(crop, filter_size)


def combine_target(images: torch.Tensor, sens: torch.Tensor, crop_target: Sequence[int]) -> torch.Tensor:
    """center_crop(|sum_c images * conj(sens)|, crop_target) (mri_data.py:302-303): images (t, c, h, w, 2), sens (c, h, w, 2)."""
    images, sens = ops._dev(images, "images"), ops._dev(sens, "sens")
    t, c, h, w, _ = images.shape
    if tuple(sens.shape) != (c, h, w, 2):
        raise ValueError("sens must be (c, h, w, 2)")
    if not (0 < crop_target[0] <= h and 0 < crop_target[1] <= w):
        raise ValueError("Invalid shapes.")                                  # transforms.py:150-151
    out = torch.empty((t, crop_target[0], crop_target[1]), device=images.device, dtype=torch.float32)
    check(lib().cine_combine_target(images.data_ptr(), sens.data_ptr(), out.data_ptr(), t, c, h, w, crop_target[0], crop_target[1],
                                    ops._stream()), "cine_combine_target")
    return out


def _raw_pairs(raw: torch.Tensor, what: str) -> torch.Tensor:
    """raw (t, x, y, coil) complex64 or (t, x, y, coil, 2) float32 on the GPU -> contiguous, 16-byte aligned float32 pairs."""
    if not isinstance(raw, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor")
    if not raw.is_cuda:
        raise CineHipError(f"{what}: the HIP path needs a GPU tensor (no CPU fallback)")
    x = torch.view_as_real(raw.to(torch.complex64)) if raw.is_complex() else raw
    if x.dim() != 5 or x.shape[-1] != 2:
        raise ValueError(f"{what} expects (t, x, y, coil) complex or (t, x, y, coil, 2) pairs")
    x = ops._dev(x, what)
    return x.clone() if x.data_ptr() % 16 else x


def _kept_frames(n_frames, t: int) -> int:
    n = t if n_frames is None else min(int(n_frames), t)
    if n < 1:
        raise ValueError("Invalid shapes.")
    return n


def coil_gram(raw: torch.Tensor, n_frames: Optional[int] = None, region: int = 24, out: Optional[torch.Tensor] = None,
              ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Calibration Gram matrix of the coils: raw (t, x, y, coil) complex64 -> G (coil, coil) complex128,
    G[i, j] = sum over the first min(n_frames, t) frames and the central region x region block of k-space (clipped to the matrix, centred
    as espirit_maps centres its block; region 0 = the whole matrix) of raw[..., i] * conj(raw[..., j]).  Float64 sums of exact products
    in a fixed order: exactly Hermitian, bit-identical from call to call.  ``out``: a contiguous complex128 (coil, coil) GPU tensor to
    write into; ``ws``: a uint8 GPU buffer of at least ``coil_gram_ws_bytes(...)`` bytes (the pipeline's static buffers)."""
    x = _raw_pairs(raw, "coil_gram")
    t, nx, ny, c, _ = x.shape
    n = _kept_frames(n_frames, t)
    region = int(region)
    if region < 0:
        raise ValueError("coil_gram: region must be >= 0")
    if out is None:
        gram = torch.empty((c, c), device=x.device, dtype=torch.complex128)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.complex128 and tuple(out.shape) == (c, c) and out.is_contiguous()):
        raise CineHipError(f"coil_gram: out must be a contiguous complex128 GPU tensor of shape {(c, c)}")
    else:
        gram = out
    nbytes = lib().cine_coil_gram_ws_bytes(n, nx, ny, c, region)
    if ws is None:
        ws = torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)
    elif not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous() and ws.numel() >= nbytes):
        raise CineHipError(f"coil_gram: ws must be a contiguous uint8 GPU buffer of at least {nbytes} bytes")
    check(lib().cine_coil_gram(x.data_ptr(), gram.data_ptr(), ws.data_ptr(), nbytes, t, nx, ny, c, n, region, ops._stream()), "cine_coil_gram")
    return gram


def coil_gram_ws_bytes(n_frames: int, nx: int, ny: int, coils: int, region: int = 24) -> int:
    """Bytes of workspace coil_gram needs for n_frames kept frames of an (nx, ny) matrix with that many coils."""
    return int(lib().cine_coil_gram_ws_bytes(int(n_frames), int(nx), int(ny), int(coils), int(region)))


COIL_MATRIX_MAX_COILS = 64      # cine_coil_matrix: the two c x c float64 matrices of the eigensolver fill the LDS (include/cine_hip.h)
COIL_MATRIX_INFO = 4            # doubles per matrix: the Jacobi residual, the sweeps used, the kept share sum(lam[:V]) / sum(lam), lam[0]
COIL_MATRIX_METHODS = ("eigh", "jacobi")


def _cc_method(method) -> str:
    if method not in COIL_MATRIX_METHODS:
        raise ValueError(f"coil compression: method must be 'eigh' or 'jacobi', got {method!r}")
    return method


def _coil_matrix_jacobi(gram: torch.Tensor, v: int, matrix: Optional[torch.Tensor] = None, lam: Optional[torch.Tensor] = None,
                        info: Optional[torch.Tensor] = None, whitener: Optional[torch.Tensor] = None):
    """cine_coil_matrix on gram (n, c, c) complex128, contiguous, on the GPU -> (matrix (n, V, c, 2) float32, lam (n, c) float64, info
    (n, COIL_MATRIX_INFO) float64), written into the given contiguous tensors where they are passed.  No host read.
    ``whitener`` (c, c) complex128, contiguous, on the same GPU: cine_coil_matrix_whitened, one whitener for all n matrices."""
    if not (isinstance(gram, torch.Tensor) and gram.is_cuda and gram.dtype == torch.complex128 and gram.dim() == 3
            and gram.shape[1] == gram.shape[2] and gram.is_contiguous()):
        raise CineHipError("coil_matrix_from_gram(method='jacobi'): gram must be a contiguous complex128 GPU tensor (no CPU fallback)")
    n, c, _ = gram.shape
    dev = gram.device
    wanted = (("matrix", matrix, (n, v, c, 2), torch.float32), ("lam", lam, (n, c), torch.float64),
              ("info", info, (n, COIL_MATRIX_INFO), torch.float64))
    outs = []
    for name, x, shape, dtype in wanted:
        if x is None:
            x = torch.empty(shape, device=dev, dtype=dtype)
        elif not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and tuple(x.shape) == shape and x.is_contiguous()):
            raise CineHipError(f"coil_matrix_from_gram: {name} must be a contiguous {dtype} GPU tensor of shape {shape}")
        outs.append(x)
    if whitener is not None:
        if not (isinstance(whitener, torch.Tensor) and whitener.is_cuda and whitener.device == dev and whitener.dtype == torch.complex128
                and tuple(whitener.shape) == (c, c) and whitener.is_contiguous()):
            raise CineHipError(f"coil_matrix_from_gram: whitener must be a contiguous complex128 tensor of shape {(c, c)} on {dev}")
        check(lib().cine_coil_matrix_whitened(gram.data_ptr(), whitener.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                              outs[2].data_ptr(), n, c, v, ops._stream()), "cine_coil_matrix_whitened")
        return tuple(outs)
    check(lib().cine_coil_matrix(gram.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), n, c, v, ops._stream()),
          "cine_coil_matrix")
    return tuple(outs)


NOISE_MAX_COILS = 128           # cine_coil_gram's limit


def noise_covariance(noise: torch.Tensor) -> torch.Tensor:
    """Noise samples (..., coil) complex64 on the GPU (the noise scan of a raw file, any leading axes) -> their covariance Psi (coil,
    coil) complex128, Psi[i, j] = 1/n sum_s eta_s[i] conj(eta_s[j]) (the index convention of coil_gram): ``coil_gram`` of the samples
    viewed as (1, n, 1, coil) with region 0, divided by n -- float64 sums of exact products in a fixed order, exactly Hermitian,
    bit-identical from call to call.  At most 128 coils."""
    if not isinstance(noise, torch.Tensor) or not noise.is_complex() or noise.dim() < 1 or noise.shape[-1] < 1 or noise.numel() < 1:
        raise ValueError("noise_covariance: noise must be a complex tensor (..., coil) with at least one sample")
    if not noise.is_cuda:
        raise CineHipError("noise_covariance: the HIP path needs a GPU tensor (no CPU fallback)")
    c = noise.shape[-1]
    if c > NOISE_MAX_COILS:
        raise CineHipError(f"noise_covariance: {c} coils, at most {NOISE_MAX_COILS}")
    x = noise.to(torch.complex64).reshape(-1, c)
    n = x.shape[0]
    return coil_gram(x.view(1, n, 1, c), None, 0) / n


def _lower_real_diag(w: torch.Tensor) -> torch.Tensor:
    """What the kernel reads of a whitener: its lower triangle, the diagonal's imaginary part taken as 0 (a copy)."""
    w = torch.tril(w).contiguous()
    torch.view_as_real(w)[..., 1].diagonal().zero_()
    return w


def noise_whitener(noise: Optional[torch.Tensor] = None, *, cov: Optional[torch.Tensor] = None, preserve_scale: bool = True) -> torch.Tensor:
    """The whitener of a scan's noise, W (coil, coil) complex128 on the input's device: with Psi = ``noise_covariance(noise)`` (or ``cov``,
    a covariance computed elsewhere, GPU or CPU) = L L^H, L lower-triangular with a real positive diagonal, W = s L^-1 -- lower-triangular
    with a real positive diagonal, W Psi W^H = s^2 I.  ``preserve_scale`` (the default): s = sqrt(trace(Psi) / coil), so the whitened data
    d' = W d keep their overall level; otherwise s = 1 (unit noise variance per channel).  Once per scan: a small dense step
    (torch.linalg.cholesky_ex, solve_triangular in complex128) that waits for the device, like ``method="eigh"``.  Pass W as
    ``whitener=`` to coil_matrix_from_gram / coil_compression_matrix / prepare_slice / prepare_masked_slice /
    SlicePipeline.submit_raw.  ValueError when Psi is not finite or not positive definite."""
    if (noise is None) == (cov is None):
        raise ValueError("noise_whitener: pass the noise samples or cov=, one of the two")
    if cov is None:
        psi = noise_covariance(noise)
    else:
        if not isinstance(cov, torch.Tensor) or cov.dim() != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 1:
            raise ValueError("noise_whitener: cov must be a square matrix (coil, coil)")
        psi = cov.to(torch.complex128)
    c = psi.shape[0]
    short = ("the noise covariance is not positive definite: too few noise samples is the usual cause (fewer samples than coils give a "
             "rank-deficient matrix); pass more of the noise scan")
    if not bool(torch.isfinite(torch.view_as_real(psi)).all()):
        raise ValueError("noise_whitener: the noise covariance is not finite (NaN or Inf in the noise samples)")
    if float((psi - psi.conj().transpose(0, 1)).abs().max()) > 1e-12 * float(psi.abs().max()):
        raise ValueError("noise_whitener: the noise covariance is not Hermitian")
    low, info = torch.linalg.cholesky_ex(psi)
    if int(info) != 0:
        raise ValueError(f"noise_whitener: {short}")
    # A pivot L[i, i]^2 = Psi[i, i] - sum_k |L[i, k]|^2 carries the rounding of its c terms, about c eps Psi[i, i]: one that is no larger
    # is zero at float64 resolution, and rounding alone lets the factorisation of a rank-deficient matrix run through.
    d = low.diagonal().real
    if bool((d * d <= c * torch.finfo(torch.float64).eps * psi.diagonal().real).any()):
        raise ValueError(f"noise_whitener: {short}")
    w = torch.linalg.solve_triangular(low, torch.eye(c, dtype=torch.complex128, device=psi.device), upper=False)
    if preserve_scale:
        w = w * torch.sqrt(psi.diagonal().real.sum() / c)
    return _lower_real_diag(w)


def _whitener_for(whitener, c: int, device) -> torch.Tensor:
    """A given whitener as (c, c) complex128 on `device`."""
    if not isinstance(whitener, torch.Tensor) or whitener.dim() != 2 or tuple(whitener.shape) != (c, c):
        raise ValueError(f"whitener must be a ({c}, {c}) tensor for {c} coils (frontend.noise_whitener)")
    return whitener.to(device=device, dtype=torch.complex128)


def _hermitian_from_upper(g: torch.Tensor) -> torch.Tensor:
    """The Hermitian matrix the kernel makes of g: its upper triangle mirrored, the diagonal's imaginary part dropped."""
    up = torch.triu(g, 1)
    return up + up.conj().transpose(0, 1) + torch.diag(g.diagonal().real).to(g.dtype)


def _phase_rows(a: torch.Tensor) -> torch.Tensor:
    """Every row of a (V, c) complex128 times the unit phase that makes its largest-magnitude entry (the first of equal maxima) real and
    positive; that entry exactly real."""
    mag = a.abs()
    idx = mag.argmax(dim=1, keepdim=True)                                    # the first of equal maxima
    peak = a.gather(1, idx)
    a = a * (peak.conj() / peak.abs())
    a.scatter_(1, idx, mag.gather(1, idx).to(a.dtype))                       # exactly real there
    return a


def coil_matrix_from_gram(gram: torch.Tensor, virtual_coils: int, method: str = "eigh", whitener: Optional[torch.Tensor] = None):
    """G (c, c) Hermitian -> (A (V, c) complex64, lam (c,) float64 descending): G = U diag(lam) U^H, A[v] = conj(U[:, v]) times the unit
    phase that makes its largest-magnitude entry (lowest index on a tie) real and positive, rounded once to complex64.  Rows are
    orthonormal and A G A^H = diag(lam[:V]).  G (n, c, c): n matrices at once, every result with a leading n.
    ``method="eigh"`` (the default): a small dense step, torch.linalg.eigh in complex128 on the tensor's own device, behind a Hermitian
    check on the host (both wait for the device).
    ``method="jacobi"``: cine_coil_matrix, one launch for all n matrices, at most COIL_MATRIX_MAX_COILS coils and 32 virtual coils
    (CineHipError beyond).  It reads the upper triangle of G only, so there is nothing to check; no host read, capturable, bit-identical
    from call to call.  Returns (A, lam, info) with info (COIL_MATRIX_INFO,) float64 ON THE DEVICE: the residual max |off-diagonal| /
    max |diagonal| the eigensolver reached (at most 1e-14 unless its sweep cap was hit or G holds a NaN), the sweeps used, the kept
    share sum(lam[:V]) / sum(lam), lam[0].
    ``whitener=W`` (c, c), from ``noise_whitener``: noise pre-whitening folded into the matrix.  The decomposition is that of the
    whitened data's Gram matrix G' = W G W^H = U diag(lam) U^H, and A[v] = sum_k conj(U[k, v]) W[k, :], phased and rounded as above:
    ``compress_coils(raw, A)`` whitens and compresses in one pass.  A Psi A^H = s^2 I and A G A^H = diag(lam[:V]); the rows are no
    longer orthonormal.  Only the lower triangle of W is used, its diagonal taken as real.  "jacobi": cine_coil_matrix_whitened, one W
    for all n matrices; "eigh": the same mathematics with torch in complex128 on the tensor's own device.  ``whitener=None``: as
    before, bit for bit."""
    _cc_method(method)
    if gram.dim() not in (2, 3) or gram.shape[-2] != gram.shape[-1] or gram.shape[-1] < 1 or gram.shape[0] < 1:
        raise ValueError("coil_matrix_from_gram: gram must be a square matrix or a stack of them")
    c = gram.shape[-1]
    v = int(virtual_coils)
    if not 1 <= v <= c:
        raise ValueError(f"coil_matrix_from_gram: virtual_coils must be in 1..{c}")
    if method == "jacobi":
        if not gram.is_cuda:
            raise CineHipError("coil_matrix_from_gram(method='jacobi'): the HIP path needs a GPU tensor (no CPU fallback)")
        g = gram.to(torch.complex128).contiguous()
        w = None if whitener is None else _whitener_for(whitener, c, g.device).contiguous()
        a, lam, info = _coil_matrix_jacobi(g if g.dim() == 3 else g[None], v, whitener=w)
        a = torch.view_as_complex(a)
        return (a, lam, info) if gram.dim() == 3 else (a[0], lam[0], info[0])
    if gram.dim() == 3:
        each = [coil_matrix_from_gram(g, v, whitener=whitener) for g in gram]
        return torch.stack([a for a, _ in each]), torch.stack([lam for _, lam in each])
    g = gram.to(torch.complex128)
    if float((g - g.conj().transpose(0, 1)).abs().max()) > 1e-12 * float(g.abs().max()):
        raise ValueError("coil_matrix_from_gram: gram is not Hermitian")
    w = None
    if whitener is not None:
        w = _lower_real_diag(_whitener_for(whitener, c, g.device))
        g = _hermitian_from_upper(w @ _hermitian_from_upper(g) @ w.conj().transpose(0, 1))     # G' = W G W^H
    try:
        ev, vec = torch.linalg.eigh(g)                                       # ascending
    except RuntimeError as e:                                                # no silent host fallback
        raise CineHipError(f"coil_matrix_from_gram: torch.linalg.eigh failed on {g.device}: {e}") from e
    lam = ev.flip(0).contiguous()
    a = vec.flip(1)[:, :v].conj().transpose(0, 1).contiguous()               # (V, c)
    if w is not None:
        a = a @ w                                                            # U^H W
    return _phase_rows(a).to(torch.complex64), lam


def coil_compression_matrix(raw: torch.Tensor, virtual_coils: int, n_frames: Optional[int] = None,
                            region: int = 24, cc_method: str = "eigh", whitener: Optional[torch.Tensor] = None):
    """coil_matrix_from_gram(coil_gram(raw, n_frames, region), virtual_coils, cc_method, whitener): (A, lam), with "jacobi" (A, lam, info)."""
    return coil_matrix_from_gram(coil_gram(raw, n_frames, region), virtual_coils, _cc_method(cc_method), whitener)


def compress_coils(raw: torch.Tensor, matrix: torch.Tensor, n_frames: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t, x, y, v] = sum_c matrix[v, c] raw[t, x, y, c] for the first min(n_frames, t) frames: raw (t, x, y, coil) complex64, matrix
    (V, coil) complex64 -> (T, x, y, V) complex64, the layout prepare_slice and ops.raw_window_ifft2c take.  Exact fp32, bit-identical
    from call to call.  ``out``: a contiguous, 16-byte aligned float32 (T, x, y, V, 2) GPU tensor to write into."""
    x = _raw_pairs(raw, "compress_coils")
    t, nx, ny, c, _ = x.shape
    n = _kept_frames(n_frames, t)
    if not isinstance(matrix, torch.Tensor) or matrix.dim() != 2 or matrix.shape[1] != c:
        raise ValueError(f"compress_coils: matrix must be (V, {c})")
    v = matrix.shape[0]
    m = ops._dev(torch.view_as_real(matrix.to(torch.complex64)), "compress_coils matrix")
    if out is None:
        out = torch.empty((n, nx, ny, v, 2), device=x.device, dtype=torch.float32)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, nx, ny, v, 2)
              and out.is_contiguous()):
        raise CineHipError(f"compress_coils: out must be a contiguous float32 GPU tensor of shape {(n, nx, ny, v, 2)}")
    check(lib().cine_coil_compress(x.data_ptr(), m.data_ptr(), out.data_ptr(), t, nx, ny, c, n, v, ops._stream()), "cine_coil_compress")
    return torch.view_as_complex(out)


WHITENER_WITH_MATRIX = ("whitener and coil_matrix: a given matrix is applied as it is; fold the whitener into it, "
                        "coil_matrix_from_gram(..., whitener=W), and pass that matrix alone")


def _whitener_alone(whitener: torch.Tensor, c: int) -> torch.Tensor:
    """The whitener as the (c, c) complex64 matrix compress_coils applies when no compression is asked for."""
    if c > 32:
        raise CineHipError(f"whitener alone keeps all {c} channels, compress_coils writes at most 32: pass virtual_coils= as well (the "
                           f"whitener is then folded into the compression matrix)")
    return whitener.to(torch.complex64)


def _compressed(kspace_txyc: torch.Tensor, n_slices: int, virtual_coils, coil_matrix, cc_region: int, cc_method: str = "eigh",
                whitener=None) -> torch.Tensor:
    """The coil-compression leg of prepare_slice: the raw data on virtual coils (kept frames only), or the input itself where
    nothing is to be done."""
    _cc_method(cc_method)
    if whitener is not None:
        if coil_matrix is not None:
            raise ValueError(WHITENER_WITH_MATRIX)
        c = kspace_txyc.shape[3]
        w = _whitener_for(whitener, c, kspace_txyc.device)
        if virtual_coils is None:
            return compress_coils(kspace_txyc, _whitener_alone(w, c), n_slices)
        v = int(virtual_coils)
        if v < 1 or v > c:
            raise ValueError(f"virtual_coils must be in 1..{c} (the coil count of this scan)")
        a = coil_compression_matrix(kspace_txyc, v, n_slices, cc_region, cc_method, w)[0]      # V == c too: the data are whitened
        return compress_coils(kspace_txyc, a, n_slices)
    if virtual_coils is None and coil_matrix is None:
        return kspace_txyc
    c = kspace_txyc.shape[3]
    if coil_matrix is not None:
        if coil_matrix.dim() != 2 or coil_matrix.shape[1] != c:
            raise ValueError(f"coil_matrix must be (V, {c})")
        if virtual_coils is not None and coil_matrix.shape[0] != int(virtual_coils):
            raise ValueError(f"coil_matrix has {coil_matrix.shape[0]} rows, virtual_coils is {int(virtual_coils)}")
        return compress_coils(kspace_txyc, coil_matrix.to(kspace_txyc.device), n_slices)
    v = int(virtual_coils)
    if v < 1 or v > c:
        raise ValueError(f"virtual_coils must be in 1..{c} (the coil count of this scan)")
    if v == c:
        return kspace_txyc                                                   # already V coils: today's path and bits
    a = coil_compression_matrix(kspace_txyc, v, n_slices, cc_region, cc_method)[0]
    return compress_coils(kspace_txyc, a, n_slices)


def prepare_slice(kspace_txyc: torch.Tensor, crop_shape=(200, 200), n_slices: int = 15,
                  filter_size=(0.7, 0.0, 0.3, 0.3), scaling: float = 1e6, virtual_coils: Optional[int] = None,
                  coil_matrix: Optional[torch.Tensor] = None, cc_region: int = 24, cc_method: str = "eigh",
                  whitener: Optional[torch.Tensor] = None):
    """reference data/mri_data.py:283-293 on the device.  kspace_txyc: raw (t, x, y, coil) complex64 (the HDF5 ``y`` array)
    on the GPU.  Returns (kspace (t, coil, X, Y, 2) float32 of the filtered crop, filtered images (t, coil, X, Y, 2)).  Raw sizes the FFT
    line engines take go through the full-image cine_fft2c; any other raw size through the windowed transform (ops.raw_window_ifft2c),
    which computes only the kept frames and the crop.
    ``virtual_coils=V``: the coils are first compressed to V virtual coils with the matrix of this slice's kept frames
    (coil_compression_matrix, calibration block cc_region), and everything runs on V coils; V equal to the coil count passes the data
    through.  ``coil_matrix=A`` (V, coil): use a given matrix instead, e.g. one matrix for all slices of a scan.  ``cc_method``:
    ``coil_matrix_from_gram``'s ``method`` for the matrix of ``virtual_coils=``.
    ``whitener=W`` (coil, coil), from ``noise_whitener`` on the scan's noise samples: noise pre-whitening in front of everything.  With
    ``virtual_coils=V`` the whitened compression matrix of this slice's own calibration block (``coil_matrix_from_gram(...,
    whitener=W)``: one pass over the data, V equal to the coil count included); alone, ``compress_coils(raw, W)`` (at most 32 coils).
    Together with ``coil_matrix`` it raises: fold it into that matrix."""
    if not kspace_txyc.is_cuda:
        raise CineHipError("prepare_slice: the HIP path needs a GPU tensor (no CPU fallback)")
    kspace_txyc = _compressed(kspace_txyc, n_slices, virtual_coils, coil_matrix, cc_region, cc_method, whitener)
    t, nx, ny = kspace_txyc.shape[0], kspace_txyc.shape[1], kspace_txyc.shape[2]
    if ops.fft_line_supported(nx) and ops.fft_line_supported(ny):
        k = _c2r((kspace_txyc.to(torch.complex64) * scaling).permute(0, 3, 1, 2).contiguous())
        images = ops.fft2c(k, inverse=True)                                  # ifftn(norm=None) * sqrt(N) == ortho (:288-289)
        _, filt = filtered_crop_center_and_slices(images, crop_shape, n_slices, filter_size)
    else:
        # raw sizes the line engines refuse (e.g. 2x-oversampled readouts): only the kept frames and the centered crop of the image
        # are computed, straight from the raw layout (:288-289 then transforms.py:209-214)
        crop = ops.raw_window_ifft2c(kspace_txyc.to(torch.complex64), min(int(n_slices), t), crop_shape, scaling)
        filt = gaussian_filter(crop, filter_size)
    return _to_kspace(filt), filt


def _to_kspace(filt: torch.Tensor) -> torch.Tensor:
    """mri_data.py:291-292: the filtered crop (t, c, X, Y, 2) back to k-space with the reference's shift order."""
    # :291 transforms back with the shifts the other way round -- ifftshift(fftn(fftshift(x))) -- which differs from fft2c
    # (fftshift(fftn(ifftshift(x)))) along axes of ODD length by one sample on either side: fftshift(x) = roll(ifftshift(x), -1)
    # and ifftshift(y) = roll(fftshift(y), +1) there.  Even lengths (the reference's 200 x 200 crop): no difference.
    odd = [d for d, n in ((-3, filt.shape[-3]), (-2, filt.shape[-2])) if n % 2]
    x = torch.roll(filt, shifts=[-1] * len(odd), dims=odd).contiguous() if odd else filt
    kk = ops.fft2c(x)                                                        # fftn(norm=None) / sqrt(N) == ortho (:291-292)
    return torch.roll(kk, shifts=[1] * len(odd), dims=odd).contiguous() if odd else kk


def _to_kspace_hip(filt: torch.Tensor) -> torch.Tensor:
    """_to_kspace with the library's own roll kernel on both sides (a roll is a copy: the same bits)."""
    odd = [d for d, n in ((-3, filt.shape[-3]), (-2, filt.shape[-2])) if n % 2]
    x = ops.roll(filt, [-1] * len(odd), odd) if odd else filt
    kk = ops.fft2c(x)
    return ops.roll(kk, [1] * len(odd), odd) if odd else kk


def prepare_masked_slice(raw: torch.Tensor, mask: Optional[torch.Tensor], crop_shape=(200, 200), n_slices: int = 15,
                         filter_size=(0.7, 0.0, 0.3, 0.3), scaling: float = 1e6, coil_matrix: Optional[torch.Tensor] = None,
                         apply_mask: bool = True, out: Optional[torch.Tensor] = None, virtual_coils: Optional[int] = None,
                         cc_region: int = 24, whitener: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Raw k-space of one cine slice -> the model's input, device in, device out: ``ops.apply_mask(prepare_slice(raw, ...)[0], mask)[None]``
    bit for bit, without a host synchronisation, a data-dependent shape or a launch outside the current stream, so that
    ``torch.cuda.graph`` captures it on any stream (run it once eagerly on that stream first, like a model's forward).  This is what
    ``SlicePipeline.submit_raw`` replays per slice.

    raw   (t, x, y, coil) complex64 or (t, x, y, coil, 2) float32 on the GPU, 16-byte aligned.  Only the first min(n_slices, t) frames are
          read.  Sizes the FFT line engines take: ops.raw_ingest (scale, coils in front) -> ifft2c of the kept frames -> crop -> Gaussian
          filter; any other size: ops.raw_window_ifft2c -> filter, as in prepare_slice.  Then the forward transform of the crop with the
          reference's shift order (mri_data.py:291-292).
    mask  the mask on the crop grid, uint8 or bool on the GPU: a row mask (1, T | 1, 1, X, 1, 1) (or any shape with T X or X entries in
          that order), or one that varies along the second axis, (1, T | 1, 1, X, Y, 1) (cine_apply_mask2d).  ``apply_mask=False`` hands the k-space on unmasked -- prospectively undersampled data, where the reference also
          only passes the stored mask on (data/transforms.py:331-339); ``mask`` may then be None.
    coil_matrix  A (V, coil) complex64 ON THE GPU: compress_coils first, everything else on V virtual coils, e.g. one matrix per scan
          from coil_compression_matrix.
    virtual_coils  V: the matrix of THIS slice's kept frames, ``coil_matrix_from_gram(coil_gram(raw, n_slices, cc_region), V,
          method="jacobi")[0]`` (cine_coil_matrix: no host read), then as with ``coil_matrix``; at most 64 coils, V <= 32.  Unlike
          prepare_slice, V equal to the coil count is not passed through: the data change to the eigenbasis.  With ``coil_matrix``
          also given its V rows are checked against ``virtual_coils`` (ValueError) and it is used.
    whitener  W (coil, coil) complex128 ON THE GPU (``noise_whitener``): noise pre-whitening.  With ``virtual_coils=V`` the matrix is
          ``coil_matrix_from_gram(coil_gram(raw, n_slices, cc_region), V, method="jacobi", whitener=W)[0]`` (cine_coil_matrix_whitened: no
          host read, capturable); alone, ``coil_matrix=W.to(torch.complex64)`` (at most 32 coils).  With ``coil_matrix`` it raises.
    out   a contiguous float32 (1, T, C, X, Y, 2) GPU tensor to write the result into (the pipeline's static buffer).
    Returns masked k-space (1, T, C, X, Y, 2) float32."""
    x = torch.view_as_real(raw) if isinstance(raw, torch.Tensor) and raw.is_complex() and raw.dtype == torch.complex64 else raw
    if not isinstance(x, torch.Tensor):
        raise TypeError("prepare_masked_slice: expected a tensor")
    if not x.is_cuda:
        raise CineHipError("prepare_masked_slice: the HIP path needs a GPU tensor (no CPU fallback)")
    if x.dtype != torch.float32 or x.dim() != 5 or x.shape[-1] != 2:
        raise CineHipError(f"prepare_masked_slice: raw must be (t, x, y, coil) complex64 or (t, x, y, coil, 2) float32, got {tuple(raw.shape)} {raw.dtype}")
    if not x.is_contiguous() or x.data_ptr() % 16:
        raise CineHipError("prepare_masked_slice: raw must be contiguous and 16-byte aligned (a copy here would hide a launch from the caller)")
    t, nx, ny, c, _ = x.shape
    cx, cy = int(crop_shape[0]), int(crop_shape[1])
    if not (0 < cx <= nx and 0 < cy <= ny):
        raise ValueError("Invalid shapes.")                                  # transforms.py:206-207
    n = _kept_frames(n_slices, t)
    if whitener is not None:
        if coil_matrix is not None:
            raise ValueError(WHITENER_WITH_MATRIX)
        if not isinstance(whitener, torch.Tensor) or whitener.dim() != 2 or tuple(whitener.shape) != (c, c):
            raise ValueError(f"whitener must be a ({c}, {c}) tensor for {c} coils (frontend.noise_whitener)")
        if not whitener.is_cuda or whitener.dtype != torch.complex128 or not whitener.is_contiguous():
            raise CineHipError("prepare_masked_slice: whitener must be a contiguous complex128 GPU tensor (a host matrix would be copied "
                               "synchronously)")
        if virtual_coils is None:
            coil_matrix = _whitener_alone(whitener, c)
    if coil_matrix is not None:
        if not isinstance(coil_matrix, torch.Tensor) or coil_matrix.dim() != 2 or coil_matrix.shape[1] != c:
            raise ValueError(f"coil_matrix must be (V, {c})")
        if not coil_matrix.is_cuda or coil_matrix.dtype != torch.complex64:
            raise CineHipError("prepare_masked_slice: coil_matrix must be a complex64 GPU tensor (a host matrix would be copied synchronously)")
        if virtual_coils is not None and coil_matrix.shape[0] != int(virtual_coils):
            raise ValueError(f"coil_matrix has {coil_matrix.shape[0]} rows, virtual_coils is {int(virtual_coils)}")
        x = torch.view_as_real(compress_coils(x, coil_matrix, n))            # (n, x, y, V, 2)
        c = coil_matrix.shape[0]
    elif virtual_coils is not None:
        v = int(virtual_coils)
        if v < 1 or v > c:
            raise ValueError(f"virtual_coils must be in 1..{c} (the coil count of this scan)")
        a = _coil_matrix_jacobi(coil_gram(x, n, cc_region)[None], v, whitener=whitener)[0][0]      # (V, c, 2); refuses more than 64 coils / 32 virtual coils
        x = torch.view_as_real(compress_coils(x, torch.view_as_complex(a), n))
        c = v
    if ops.fft_line_supported(nx) and ops.fft_line_supported(ny):
        images = ops.fft2c(ops.raw_ingest(x, n, scaling), inverse=True)      # the kept frames only
        filt = gaussian_filter(crop_select(images, n, (cx, cy)), filter_size)
    else:
        filt = gaussian_filter(ops.raw_window_ifft2c(x, n, (cx, cy), scaling), filter_size)
    kk = _to_kspace_hip(filt)                                                # (n, c, cx, cy, 2)
    shape = (1, n, c, cx, cy, 2)
    if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == shape
                                and out.is_contiguous()):
        raise CineHipError(f"prepare_masked_slice: out must be a contiguous float32 GPU tensor of shape {shape}")
    if not apply_mask:
        return kk.view(shape) if out is None else out.copy_(kk.view(shape))
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype not in (torch.uint8, torch.bool):
        raise CineHipError("prepare_masked_slice: mask must be a uint8 or bool GPU tensor")
    m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    if cy > 1 and m.dim() == 6 and tuple(m.shape[2:]) == (1, cx, cy, 1) and m.shape[0] == 1 and m.shape[1] in (1, n):
        if m.shape[1] != n:
            m = m.expand(1, n, 1, cx, cy, 1).contiguous()                    # one pattern for all frames
        m = m.view(n, 1, cx, cy, 1)                                          # varies along y: one plane per frame
    elif m.numel() == cx and n > 1:
        m = m.reshape(1, cx).expand(n, cx).contiguous()                      # one pattern for all frames
    elif m.numel() != n * cx:
        raise ValueError(f"prepare_masked_slice: mask {tuple(mask.shape)} is not a row mask (1, {n} | 1, 1, {cx}, 1, 1) "
                         f"nor a mask (1, {n} | 1, 1, {cx}, {cy}, 1)")
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.float32)
    ops.apply_mask(kk, m, out=out.view(n, c, cx, cy, 2))
    return out


def time_average(masked_kspace: torch.Tensor) -> torch.Tensor:
    """masked k-space of one cine slice (t, coil, ny, nx, 2) -> its average over the frames (coil, ny, nx, 2), the input of the
    calibration (data/transforms.py:426-427).  This is the form ``SlicePipeline`` computes for ``sens_maps="espirit"``."""
    return masked_kspace.mean(dim=0)


def espirit_projector(gram: torch.Tensor, thresh: float = 1e-3, sign_iters: int = 60) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """gram (n, n) complex128 Hermitian on the GPU -> (P (n, n, 2) float32, lam_max (1,) float64, residual (1,) float64): the projector
    onto the eigenvectors with eigenvalue >= thresh^2 lam_max as 1/2 (I + sign(gram - thresh^2 lam_max I)), by Newton-Schulz steps on the
    float64 matrix cores (cine_espirit_projector).  residual = max |X^2 - I| of the sign matrix handed out.  No host read."""
    if not (isinstance(gram, torch.Tensor) and gram.is_cuda and gram.dtype == torch.complex128 and gram.dim() == 2
            and gram.shape[0] == gram.shape[1] and gram.is_contiguous()):
        raise CineHipError("espirit_projector: gram must be a contiguous square complex128 GPU tensor")
    n = gram.shape[0]
    dev = gram.device
    proj = torch.empty((n, n, 2), device=dev, dtype=torch.float32)
    lam = torch.empty(1, device=dev, dtype=torch.float64)
    resid = torch.empty(1, device=dev, dtype=torch.float64)
    nbytes = lib().cine_espirit_projector_ws_bytes(n)
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    check(lib().cine_espirit_projector(gram.data_ptr(), n, float(thresh), int(sign_iters), proj.data_ptr(), lam.data_ptr(), resid.data_ptr(),
                                       ws.data_ptr(), nbytes, ops._stream()), "cine_espirit_projector")
    return proj, lam, resid


def espirit_gram(kspace: torch.Tensor, r: int = 24, k: int = 6) -> torch.Tensor:
    """kspace (coil, ny, nx, 2) float32 -> the Gram matrix (k k coil square, complex128) of the k x k patches of its central
    min(r, ny) x min(r, nx) block, columns ordered (py, px, coil) (cine_espirit_gram)."""
    kspace = ops._dev(kspace, "espirit_gram kspace")
    c, ny, nx, _ = kspace.shape
    n = k * k * c
    gram = torch.empty((n, n), device=kspace.device, dtype=torch.complex128)
    nbytes = lib().cine_espirit_gram_ws_bytes(c, ny, nx, int(r), int(k))
    ws = torch.empty(max(nbytes, 16), device=kspace.device, dtype=torch.uint8)
    check(lib().cine_espirit_gram(kspace.data_ptr(), gram.data_ptr(), ws.data_ptr(), nbytes, c, ny, nx, int(r), int(k), ops._stream()),
          "cine_espirit_gram")
    return gram


def espirit_maps(kspace: torch.Tensor, r: int = 24, k: int = 6, thresh: float = 1e-3, crop: float = 0.8,
                 iters: int = 100, *, method: str = "eigh", sign_iters: int = 60, return_residual: bool = False):
    """kspace (coil, ny, nx, 2) float32 (centered, ortho; e.g. the time average of a cine slice) ->
    (maps (coil, ny, nx, 2), eigenvalue map (ny, nx)).  r: side of the central calibration region (ecalib -r).
    ``method="eigh"`` (the default): the Gram matrix and its eigen-decomposition are library calls in complex128
    (torch.linalg.eigh checks its result on the host, and the kept eigenvectors are selected by a boolean index).
    ``method="sign"``: cine_espirit_gram, then the projector as a matrix sign function (``espirit_projector``, ``sign_iters``
    Newton-Schulz steps): no host read, every shape fixed by the input's shape, so ``torch.cuda.graph`` captures the call and replays it
    on new data.  ``return_residual=True`` adds the device scalar max |X^2 - I| of the sign matrix ((1,) float64; "sign" only): above
    1e-6 an eigenvalue of the Gram matrix sits at the threshold and ``sign_iters`` has to be raised."""
    if method not in ("eigh", "sign"):
        raise ValueError(f"espirit_maps: method must be 'eigh' or 'sign', got {method!r}")
    if return_residual and method != "sign":
        raise ValueError("espirit_maps: return_residual needs method='sign'")
    kspace = ops._dev(kspace, "espirit_maps kspace")
    c, ny, nx, _ = kspace.shape
    if c > 32:
        raise CineHipError("espirit_maps: at most 32 coils")
    ry, rx = min(int(r), ny), min(int(r), nx)
    if ry < k or rx < k or ny < 2 * k - 1 or nx < 2 * k - 1:
        raise ValueError("calibration region / image smaller than the kernel")
    if method == "sign":
        proj, _, resid = espirit_projector(espirit_gram(kspace, r, k), thresh, sign_iters)
        maps, lam = _maps_from_projector(proj, c, k, ny, nx, iters, crop)
        return (maps, lam, resid) if return_residual else (maps, lam)
    y0, x0 = ny // 2 - ry // 2, nx // 2 - rx // 2
    acs = torch.view_as_complex(kspace)[:, y0:y0 + ry, x0:x0 + rx].to(torch.complex128)
    # rows = all k x k patches, columns ordered (py, px, coil)
    a = acs.unfold(1, k, 1).unfold(2, k, 1).permute(1, 2, 3, 4, 0).reshape((ry - k + 1) * (rx - k + 1), k * k * c)
    gram = a.conj().transpose(0, 1) @ a                                      # (k k c)^2, Hermitian
    try:
        ev, vec = torch.linalg.eigh(gram)
    except RuntimeError as e:                                                # no silent host fallback
        raise CineHipError(f"espirit_maps: torch.linalg.eigh failed on {gram.device}: {e}") from e
    keep = ev >= (thresh * thresh) * ev[-1]                                  # sigma >= thresh * sigma_max
    v = vec[:, keep]
    proj = torch.view_as_real((v @ v.conj().transpose(0, 1)).to(torch.complex64)).contiguous()
    return _maps_from_projector(proj, c, k, ny, nx, iters, crop)


def _maps_from_projector(proj: torch.Tensor, c: int, k: int, ny: int, nx: int, iters: int, crop: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """The image-space half of the calibration: lag kernels of the projector -> the c x c operator of every pixel -> its dominant
    eigenpair."""
    kpad = torch.empty((c * c, ny, nx, 2), device=proj.device, dtype=torch.float32)
    check(lib().cine_espirit_lag_kernels(proj.data_ptr(), kpad.data_ptr(), c, k, ny, nx, ops._stream()), "cine_espirit_lag_kernels")
    m = ops.fft2c(kpad, inverse=True)
    maps = torch.empty((c, ny, nx, 2), device=proj.device, dtype=torch.float32)
    lam = torch.empty((ny, nx), device=proj.device, dtype=torch.float32)
    check(lib().cine_espirit_eig(m.data_ptr(), maps.data_ptr(), lam.data_ptr(), c, ny * nx, int(iters), float(crop), ops._stream()),
          "cine_espirit_eig")
    return maps, lam


def ecalib(time_avg_kspace, *, r: int, method: str = "eigh"):
    """``r`` is required: the reference's two call sites differ (`-r 200`, mri_data.py:296; `-r 15`, transforms.py:429).
    Stand-in for ``bart.bart(2, 'ecalib -r N', time_avg_kspace)[0][..., 0]`` at the reference's call sites
    (mri_data.py:295-297, transforms.py:427-430): (1, x, y, coil) complex (numpy or tensor) -> (x, y, coil) complex of
    the same kind; the calibration itself runs on the GPU."""
    import numpy as np
    is_np = isinstance(time_avg_kspace, np.ndarray)
    t = torch.as_tensor(time_avg_kspace).to(torch.complex64)
    if t.dim() != 4 or t.shape[0] != 1:
        raise ValueError("ecalib expects (1, x, y, coil)")
    dev = t.device if t.is_cuda else torch.device("cuda")
    k = torch.view_as_real(t[0].permute(2, 0, 1).contiguous().to(dev)).contiguous()
    maps, _ = espirit_maps(k, r=r, method=method)
    out = torch.view_as_complex(maps).permute(1, 2, 0).contiguous()
    return out.cpu().numpy() if is_np else out.to(t.device)


def prepare_example(source, mask=None, sens=None, fname: str = "", crop_shape=(200, 200), crop_target=(180, 180), n_slices: int = 15,
                    filter_size=(0.7, 0.0, 0.3, 0.3), scaling: float = 1e6, ecalib_r: int = 200, virtual_coils: Optional[int] = None,
                    coil_matrix: Optional[torch.Tensor] = None, cc_region: int = 24, espirit_method: str = "eigh", cc_method: str = "eigh",
                    whitener: Optional[torch.Tensor] = None):
    """``SliceDataset.__getitem__`` of the reference (data/mri_data.py:267-311) in one piece, on the device: scale -> IFFT2 -> crop +
    frame selection + Gaussian filter -> FFT2 (k-space of the filtered crop) -> sensitivity maps from the time-averaged k-space
    (ESPIRiT, where the reference shells out to ``bart ecalib -r 200``; pass ``sens`` (coil, X, Y) complex to use given maps) ->
    coil-combined magnitude target -> center crop.  ``source``: the raw (t, x, y, coil) complex array / tensor, or an already-open
    h5py-like mapping holding it under ``"y"`` (and optionally ``"mask"``): the reader stays the caller's.
    Returns the reference's sample tuple (kspace (t, coil, X, Y) complex64, mask, target (t, cx, cy) float32, attrs, fname, dataslice)
    as numpy arrays, like the reference (the ``*DataTransform`` classes take it from there, data/transforms.py:300-352).
    ``virtual_coils`` / ``coil_matrix`` / ``cc_region``: as in prepare_slice; k-space, the calibration and ``sens`` are then on the V
    virtual coils, so raw data with more than 32 coils calibrates whenever V <= 32.  ``espirit_method``: ``espirit_maps``' ``method``;
    ``cc_method``: ``coil_matrix_from_gram``'s.  ``whitener``: as in prepare_slice (the calibration then sees white noise)."""
    import numpy as np
    if hasattr(source, "keys") and "y" in source:
        raw = np.asarray(source["y"])
        if mask is None and "mask" in source:
            mask = np.asarray(source["mask"])
    else:
        raw = source
    if not torch.cuda.is_available():
        raise CineHipError("prepare_example: the front-end kernels need a GPU (no CPU fallback)")
    y = torch.as_tensor(raw).to(torch.complex64).cuda()
    kspace, filt = prepare_slice(y, crop_shape, n_slices, filter_size, scaling, virtual_coils, coil_matrix, cc_region, cc_method,
                                 whitener)                                   # (t, c, X, Y, 2) each
    if sens is not None and (virtual_coils is not None or coil_matrix is not None) and tuple(sens.shape)[0] != kspace.shape[1]:
        raise ValueError(f"sens has {tuple(sens.shape)[0]} coils, the compressed data {kspace.shape[1]}")
    if sens is None:
        time_avg = torch.view_as_complex(kspace.mean(dim=0, keepdim=True).contiguous()).permute(0, 2, 3, 1)     # (1, X, Y, coil), :295
        smaps = ecalib(time_avg, r=ecalib_r, method=espirit_method).permute(2, 0, 1).contiguous()                  # (coil, X, Y), :297-298
    else:
        smaps = torch.as_tensor(sens).to(torch.complex64).cuda()
    target = combine_target(filt, torch.view_as_real(smaps).contiguous(), crop_target)      # :302-303
    k_np = torch.view_as_complex(kspace.contiguous()).cpu().numpy()
    return k_np, mask, target.cpu().numpy(), {}, fname, 0
