/* cine_hip.h -- C ABI of libcine_hip.so, the MI355X (gfx950) cine-MRI reconstruction kernels.
 *
 * The reference (f78bono/deep-cine-cardiac-mri) is pure Python on PyTorch and has no
 * FFI of its own: the boundary this library sits under is the ATen operator layer that
 * `reconstruction.models.*` / `reconstruction.utils.*` dispatch to.  Each entry point
 * below names the reference code it replaces (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative CINE_E* code; it never throws,
 *     aborts, allocates device memory or synchronises.  cine_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - all pointers are DEVICE pointers owned by the caller (except where noted), fp32,
 *     contiguous, in the reference's layouts: complex = trailing pair (re, im);
 *     k-space (b, t, coil, h, w, 2); image (b, t, h, w, 2); mask uint8 (b, t, 1, h, 1, 1).
 *     Complex operands must be 8-byte aligned (a whole (re, im) pair is loaded at once); 16-byte alignment is only needed where an
 *     entry point says so.
 *   - `stream` is the caller's hipStream_t passed as void* (NULL = default stream);
 *     every launch goes onto it, so the calls are hipGraph-capturable.
 *   - scratch comes from the caller: `ws`/`ws_bytes` with a matching *_ws_bytes() query.
 *   - re-entrant: what a call computes depends on its arguments only (activation slopes and ReLU switches are arguments, never
 *     library state).  State that outlives a call is limited to: the optional launch profiler (cine_profile_begin/end: a
 *     mutex-guarded event list, off by default) and per-(kernel, device) once-flags for the > 64 KB LDS opt-in -- process-wide,
 *     neither changes a result; and three settings of the CALLING THREAD, invisible to every other thread: its error string
 *     (cine_last_error), its optional side stream (cine_set_side_stream) and its diagnostic kernel-selection mask
 *     (cine_set_conv_plane: which of two bit-identical kernels a launch uses).  The library reads no environment variable.
 *     tests/test_hip_parity.py::test_two_threads_two_streams_are_independent runs two models on two threads and streams while
 *     one of them flips the diagnostic mask and uses another slope.
 *   - the library creates no streams.  The two backward entry points that overlap weight gradients with the input-gradient
 *     chain (cine_unet2d_backward, cine_unet3d_backward, cine_mwcnn_backward) create and destroy hipEvents (no timing) to order the two streams.
 *
 * The Python binding is generated from this file
 *   cine_hip/_lib.py parses every prototype below into its ctypes signature; there is no second table to keep in step.  So the
 *   declarations keep to one style, and the parser refuses anything else: every statement is a prototype `T cine_name(args);`,
 *   by-value arguments and returns are int, long, float, double or size_t (a leading const is allowed), every pointer argument is
 *   opaque to the binding (it passes an address, whatever the pointee type says), and the only pointer return is const char*.
 *   No other by-value type (uint8_t, unsigned, int64_t, bool, structs), no char* argument, no function pointer, array or `...`.
 */
#ifndef CINE_HIP_H
#define CINE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CINE_OK 0
#define CINE_EINVAL (-1)      /* bad argument (null pointer, non-positive size, bad enum)      */
#define CINE_EUNSUPPORTED (-2)/* size/shape outside what the kernels implement                 */
#define CINE_EWORKSPACE (-3)  /* workspace too small                                           */
#define CINE_EHIP (-4)        /* a HIP launch failed; see cine_last_error()                    */

/* library / build identification */
int cine_version(void);                 /* ABI version, currently 3 */
const char* cine_last_error(void);      /* thread-local, never NULL */
const char* cine_build_arch(void);      /* "gfx950" */

/* ------------------------------------------------------------------------------------------
 * Centered ortho FFTs                          reference: reconstruction/utils/fftc.py
 * ------------------------------------------------------------------------------------------ */

/* fft2c (fftc.py:59-83) / ifft2c (fftc.py:86-110) over the last two spatial dims of
 * `nimg` images of h x w complex.  inverse = 0 forward, 1 inverse.  in == out allowed.
 * Line lengths (every transform of this header except cine_raw_window_ifft2c, which has no length limit): 200 (the 10 x 20
 * engine), any 2^a 3^b 5^c <= 512 (mixed-radix Stockham engine), any other length <= 400 (direct DFT in LDS); CINE_EUNSUPPORTED
 * beyond.  cine_fft_line_supported(n) is 1 for the lengths these transforms take, 0 otherwise (n < 1 included). */
int cine_fft2c(const float* in, float* out, int nimg, int h, int w, int inverse, void* stream);
int cine_fft_line_supported(int n);

/* fft1c (fftc.py:5-29) / ifft1c (fftc.py:32-56): `nlines` contiguous lines of n complex.
 * variant 0 = fftc.py shift order (ifftshift, transform, fftshift);
 * variant 1 = XPDNet's order (xpdnet.py:466 / :500), which differs for odd n. */
int cine_fft1c(const float* in, float* out, long nlines, int n, int inverse, int variant, void* stream);

/* ------------------------------------------------------------------------------------------
 * Coil operators                               reference: reconstruction/models/varnet.py
 * ------------------------------------------------------------------------------------------ */

/* VarNetBlock.sens_reduce (varnet.py:187-194): out[b,t,h,w] = sum_c conj(S[b,c]) * ifft2c(k[b,t,c]).
 * sens (b, 1, c, h, w, 2).  out (b, t, 1, h, w, 2) complex, or with magnitude != 0 the
 * real (b, t, h, w) of VarNet.forward's final line (varnet.py:150-151, math.py:48-62).
 * `tmp` holds b*t*c*h*w complex (8 bytes each); tmp == k transforms k in place (k is destroyed). */
int cine_sens_reduce(const float* k, const float* sens, float* out, float* tmp,
                     int b, int t, int c, int h, int w, int magnitude, void* stream);

/* VarNetBlock.sens_expand (varnet.py:181-185) fused with the soft data-consistency of
 * VarNetBlock.forward (varnet.py:281-282):
 *   kth = fft2c(S * img);  out = mask ? (kth + v * kref) / (1 + v) : kth,  v = softplus(*lambda_dev)
 * img (b, t, 1, h, w, 2); kref (b, t, c, h, w, 2); mask uint8 (b, t, 1, h, 1, 1);
 * lambda_dev points to ONE float in device memory (cascades.N.lambda_reg).
 * kref == NULL  => plain sens_expand (no blend; mask / lambda_dev ignored).
 * hard_mask == 1 => out = mask ? kth : 0  (CineNet HOperator, cinenet.py:121-133; kref ignored).
 * hard_mask == 2 => out = mask ? kth - kref : 0  (XPDNet measurement residual of the masked forward
 *                   operator, xpdnet.py:128-131, 295-298). */
int cine_sens_expand_dc(const float* img, const float* sens, const float* kref, const uint8_t* mask,
                        const float* lambda_dev, float* out, int b, int t, int c, int h, int w,
                        int hard_mask, void* stream);

/* The same two operators split at "hybrid space" (image along h, k-space along w), so that a
 * cascade chain never writes k-space to HBM: the next cascade's sens_reduce (varnet.py:253) starts
 * with the column IFFT of exactly the tile the DC (varnet.py:281-282) just produced.
 *   cine_kspace_to_hybrid : centered column IFFT of nimg k-space images (first half of ifft2c)
 *   cine_hybrid_reduce    : row IFFT + conj(S) multiply + coil sum (second half of sens_reduce)
 *   cine_expand_dc_hybrid : sens_expand + DC as cine_sens_expand_dc, then the column IFFT, in one pass
 * cine_sens_reduce(k) == cine_hybrid_reduce(cine_kspace_to_hybrid(k)); and
 * cine_expand_dc_hybrid(...) == cine_kspace_to_hybrid(cine_sens_expand_dc(...)). hyb may alias k. */
int cine_kspace_to_hybrid(const float* k, float* hyb, long nimg, int h, int w, void* stream);
int cine_hybrid_reduce(const float* hyb, const float* sens, float* out,
                       int b, int t, int c, int h, int w, int magnitude, void* stream);
int cine_expand_dc_hybrid(const float* img, const float* sens, const float* kref, const uint8_t* mask,
                          const float* lambda_dev, float* hyb, int b, int t, int c, int h, int w,
                          int hard_mask, void* stream);

/* Image-space data consistency: one cascade's  sens_expand -> FFT2 -> DC -> [next cascade] IFFT2 -> sens_reduce
 * (models/varnet.py:181-194, 253, 281-282) as ONE operator on the coil-combined image, for Cartesian ROW masks
 * (mask (b, t, 1, h, 1, 1), the only layout the reference produces: data/transforms.py:341-343, subsample.py:146-150).
 * Mask and blend weights depend on the k-space row only, so they commute with the transform along w and
 *     out = sum_c conj(S_c) IFFT_h[ wgt(ky) * FFT_h(S_c img) ] + beta * zf,
 *     wgt = mask ? w_sampled : w_unsampled          (centered ortho 1-D transforms along h)
 * equals sens_reduce(DC(sens_expand(img))) with  zf = sens_reduce(mask * k_ref)  (constant over the cascades).
 *   lambda_dev != NULL : soft DC, v = softplus(*lambda_dev): w_sampled = 1/(1+v), w_unsampled = 1, beta = v/(1+v)
 *                        (the float arguments are ignored)
 *   lambda_dev == NULL : the float arguments are used as given, e.g. (1, 0, 0) = CineNet's normal operator A^H M A
 *                        (models/cinenet.py:121-133, 255-257), (1, 0, -1) = XPDNet's backward image A^H M (A x - k_ref)
 *                        (models/xpdnet.py:128-131, 161-167, 295-298).
 * img, zf (may be NULL), out: (b, t, h, w, 2); sens (b, 1, c, h, w, 2); mask uint8 (b, t, h).  magnitude != 0: out is
 * (b, t, h, w) = |result| (varnet.py:150-151).  out must not alias img.  ws: cine_image_dc_ws_bytes() of scratch
 * (per-coil-group partial sums of the h == 200 kernel; 0 bytes / NULL for other sizes or <= 4 coils). */
size_t cine_image_dc_ws_bytes(int b, int t, int c, int h, int w);
int cine_image_dc(const float* img, const float* sens, const float* zf, const uint8_t* mask,
                  const float* lambda_dev, float w_sampled, float w_unsampled, float beta,
                  float* out, int b, int t, int c, int h, int w, int magnitude,
                  void* ws, size_t ws_bytes, void* stream);
/* CineNet's normal operator with its regulariser weight (models/cinenet.py:121-133): out = A^H M A img + softplus(*lambda_dev) img
 * for a row mask -- cine_image_dc with weights (1, 0), zf = img and beta = softplus(lambda) read on the device.  Same
 * shapes / workspace as cine_image_dc. */
int cine_normal_op(const float* img, const float* sens, const uint8_t* mask, const float* lambda_dev,
                   float* out, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);
/* The sensitivities in column-tile-major order [b][c][ceil(w / 5)][200][5] (complex pairs; zero past the last column), for the h == 200
 * image-space operators: a workgroup of imgdc200_kernel then reads each coil's 200 rows as one contiguous run instead of 40 bytes out of
 * every 128-byte line (38 -> 34 us per launch at cfg 2 / cfg 4).  The maps are constant over a forward pass (varnet.py:144, cinenet.py
 * forward's argument), so one pack serves its 6 - 42 operator applications.  cine_sens_tile_floats() == 0 where no kernel reads them
 * (h != 200); the *_t entry points take the tiled copy beside the plain one (NULL = read the plain maps: identical results either way). */
size_t cine_sens_tile_floats(int b, int c, int h, int w);
int cine_sens_tile_pack(const float* sens, float* tiled, int b, int c, int h, int w, void* stream);
int cine_image_dc_t(const float* img, const float* sens, const float* sens_tiled, const float* zf, const uint8_t* mask,
                    const float* lambda_dev, float w_sampled, float w_unsampled, float beta,
                    float* out, int b, int t, int c, int h, int w, int magnitude,
                    void* ws, size_t ws_bytes, void* stream);
int cine_normal_op_t(const float* img, const float* sens, const float* sens_tiled, const uint8_t* mask, const float* lambda_dev,
                     float* out, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);
/* cine_normal_op that also leaves 256 partial sums of <img, out> in pd_part (device floats): the p.d of the conjugate-gradient step that
 * follows (models/cinenet.py:155-159), produced where `out` is produced instead of by a separate pass over both vectors; feed them to
 * cine_cg_step_pd (pd_part = the first 256 floats of its workspace).  CINE_EUNSUPPORTED where cine_image_dc_ws_bytes() is 0. */
int cine_normal_op_pd(const float* img, const float* sens, const uint8_t* mask, const float* lambda_dev,
                      float* out, float* pd_part, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);

/* cine_image_dc for a sampling mask that varies along w (partial-echo readouts, 2-D variable density, k-t patterns with a readout
 * cut-off: the reference's models accept (b|1, t|1, 1, h, w, 1), varnet.py:281-282).  The identity needs no row mask:
 *     out = sum_c conj(S_c) IFFT2[ wgt(ky, kx) * FFT2(S_c img) ] + beta * zf,   wgt = mask ? w_sampled : w_unsampled
 * equals sens_reduce(DC(sens_expand(img))) with zf = sens_reduce(mask * k_ref); only the weights no longer commute with the transform
 * along w, so each coil image takes both line passes: coil expand + row FFT into ws, column FFT -> weights -> column IFFT in place
 * (one kernel for h == 200), row IFFT + conj(S) + coil sum + beta * zf (+ magnitude) into out.  Same contract as cine_image_dc
 * (lambda_dev, zf may be NULL, magnitude, out must not alias img) except mask: uint8 (b, t, h, w).  ws: cine_image_dc_general_ws_bytes()
 * = the b*t*c*h*w complex hybrid-space coil images, always needed.  Both h and w may be any length cine_fft_line_supported() accepts
 * (CINE_EUNSUPPORTED otherwise); c <= 32768.  Every argument is checked before the first launch. */
size_t cine_image_dc_general_ws_bytes(int b, int t, int c, int h, int w);
int cine_image_dc_general(const float* img, const float* sens, const float* zf, const uint8_t* mask,
                          const float* lambda_dev, float w_sampled, float w_unsampled, float beta,
                          float* out, int b, int t, int c, int h, int w, int magnitude,
                          void* ws, size_t ws_bytes, void* stream);
/* cine_normal_op for such a mask: out = A^H M A img + softplus(*lambda_dev) img (models/cinenet.py:121-133), mask uint8 (b, t, h, w).
 * Shapes and workspace as cine_image_dc_general. */
int cine_normal_op_general(const float* img, const float* sens, const uint8_t* mask, const float* lambda_dev,
                           float* out, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);

/* cine_kspace_to_hybrid of (mask * k) without reading the rows the mask drops: the hybrid-space image of the
 * measured lines only (the zero-filled term zf above: cine_hybrid_reduce of it).  k, hyb (bt, c, h, w, 2); mask (bt, h). */
int cine_masked_kspace_to_hybrid(const float* k, const uint8_t* mask, float* hyb, int bt, int c, int h, int w,
                                 void* stream);

/* ---- the steps either side of the path ------------------------------------------------------------ */

/* out = kspace * mask + 0.0 for a Cartesian row mask (reference data/transforms.py:66-92 `apply_mask`, :91).
 * kspace, out (bt, c, h, w, 2) (may alias); mask uint8 (bt, h). */
int cine_apply_mask(const float* kspace, const uint8_t* mask, float* out, long bt, int c, int h, int w, void* stream);

/* The same for a mask that varies along w: mask uint8 (bt, h, w), one plane per frame.  Bit-equal to the torch expression
 * kspace * mask + 0.0 (-0.0 becomes +0.0); out may alias kspace. */
int cine_apply_mask2d(const float* kspace, const uint8_t* mask, float* out, long bt, int c, int h, int w, void* stream);

/* x[i] *= s, in place: the "backward" / "forward" normalisations of torch.fft on top of the ortho kernels
 * (reference utils/fftc.py:59-110 with norm=None, traintest_scripts/run_inference.py:66). */
int cine_scale(float* x, long n, float s, void* stream);

/* Zero-filled reconstruction of traintest_scripts/run_inference.py:64-67:
 * rss_complex(ifft2c(k, norm=None) * sqrt(h w), dim=coil) (utils/coil_combine.py:21-34) -> out (b, t, h, w).
 * k (b, t, c, h, w, 2); tmp: scratch of k's size (tmp == k destroys k). */
int cine_zero_filled_rss(const float* k, float* out, float* tmp, int b, int t, int c, int h, int w, void* stream);

/* SSIM / NMSE / PSNR / MSE of a reconstruction against its target, on the device (reference utils/evaluate.py:6-50 --
 * skimage structural_similarity / peak_signal_noise_ratio defaults -- after data/transforms.py:161-183
 * center_crop_to_smallest; utils/losses.py:25-58 for SSIMLoss's per-frame data range).  gt (t, hg, wg), pred (t, hp, wp)
 * float32; both are center-cropped to (min h, min w).  SSIM: win x win uniform window (odd, 3 .. 11; reference 7; one pixel has no
 * sample covariance and is refused, as skimage refuses it), sample
 * covariance, K1, K2, mean over the window-valid region, then over frames; float64 arithmetic like skimage.
 * range_mode 0: data range = max of the cropped gt volume (evaluate.py:31); 1: max of each gt frame (losses.py:34);
 * 2: `maxval`.  out (device, 4 + t doubles) = {ssim, nmse, psnr, mse, ssim of frame 0..t-1}. */
size_t cine_image_metrics_ws_bytes(int t, int hg, int wg, int hp, int wp, int win);
int cine_image_metrics(const float* gt, const float* pred, int t, int hg, int wg, int hp, int wp,
                       int win, double k1, double k2, int range_mode, double maxval,
                       double* out, void* ws, size_t ws_bytes, void* stream);

/* SensitivityModel prologue (varnet.py:62-74): mean over frames, keep rows [row_lo, row_hi) of
 * dim h (transforms.mask_center, data/transforms.py:95-108), ifft2c.  k (b,t,c,h,w,2) -> out (b,c,h,w,2). */
int cine_sens_prologue(const float* k, float* out, int b, int t, int c, int h, int w,
                       int row_lo, int row_hi, void* stream);
/* The same without a host read-back of the mask (the reference finds the window on the host, varnet.py:64-68): cine_acs_window finds the fully
 * sampled centre rows of a row mask on the device -- mask_rows: the 1-D pattern of frame 0, n >= h float32 entries, 0 = not sampled;
 * window[0..1] = {pad, pad + n_low} with left = the last unsampled row below h / 2 (-1: none), right = the first one at or above it (n: none),
 * n_low = right - left, pad = (h - n_low + 1) / 2; only the first h entries are read, and a mask with no unsampled row below or none at or
 * above h / 2 (the reference raises there) gives {0, h} -- and cine_sens_prologue_win reads {row_lo, row_hi} from that device buffer. */
int cine_acs_window(const float* mask_rows, int n, int h, int* window, void* stream);
int cine_sens_prologue_win(const float* k, float* out, int b, int t, int c, int h, int w, const int* window, void* stream);

/* SensitivityModel.divide_root_sum_of_squares (varnet.py:58-59, coil_combine.py:21-34), in place
 * on x (b, c, h, w, 2). */
int cine_rss_normalise(float* x, int b, int c, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------
 * NormUnet pre/post and the XT/XF rotations    reference: denoisers/norm_unet.py, varnet.py:196-241
 * ------------------------------------------------------------------------------------------ */

/* padded size of NormUnet.pad (norm_unet.py:76-86): ((n - 1) | 15) + 1 */
int cine_pad16(int n);

/* NormUnet front half on `n` complex images (n, h, w, 2): complex_to_chan_dim (:48-51), group
 * norm with unbiased std (:59-69), zero pad to x16 (:76-86).
 * planes (n, 2, hp, wp) fp32; stats (n, 2, 2) = {mean, std} per (sample, re|im).
 * norm == 0: just the (re, im) -> 2-channel repack with no normalisation and no padding, planes
 * (n, 2, h, w) -- the layout CineNet feeds its bare Unet (cinenet.py:242). */
int cine_normunet_pack(const float* x, float* planes, float* stats, int n, int h, int w, int norm, void* stream);

/* NormUnet back half (:88-96 unpad, :71-74 unnorm, :53-57 chan_complex_to_last_dim).
 * stats == NULL: inverse of the norm == 0 repack (cinenet.py:243-244). */
int cine_normunet_unpack(const float* planes, const float* stats, float* y, int n, int h, int w, void* stream);

/* VarNetBlock.xfyf_transform front half (varnet.py:202-217) + both NormUnet front halves:
 * temporal mean subtract, (xf != 0) centered temporal DFT, rotation into x-f / y-f planes,
 * group norm, pad.  img (b, t, h, w, 2).
 *   planes_xf (b*h, 2, pad16(w), pad16(t)), planes_yf (b*w, 2, pad16(h), pad16(t)),
 *   stats_xf (b*h, 2, 2), stats_yf (b*w, 2, 2), mean_img (b, h, w, 2).
 * ws: cine_xfyf_ws_bytes(b, t, h, w).  2 <= t <= 64 (more frames: CINE_EUNSUPPORTED), b <= 65535; cine_xfyf_unpack also h <= 65535. */
size_t cine_xfyf_ws_bytes(int b, int t, int h, int w);
int cine_xfyf_pack(const float* img, float* planes_xf, float* planes_yf, float* stats_xf, float* stats_yf,
                   float* mean_img, int b, int t, int h, int w, int xf, int norm, void* ws, size_t ws_bytes, void* stream);

/* norm == 0 gives CineNet's variant (cinenet.py:181-195): same rotation, planes (b*h, 2, w, t) /
 * (b*w, 2, h, t) unnormalised and unpadded; stats may then be NULL (also in cine_xfyf_unpack).
 * back half (varnet.py:229-241 / cinenet.py:206-219): unpad + unnorm both planes, un-rotate, average,
 * inverse temporal DFT, add the temporal mean.  out (b, t, 1, h, w, 2). */
int cine_xfyf_unpack(const float* planes_xf, const float* planes_yf, const float* stats_xf,
                     const float* stats_yf, const float* mean_img, float* out,
                     int b, int t, int h, int w, int xf, void* stream);

/* ------------------------------------------------------------------------------------------
 * U-Net regulariser                            reference: denoisers/unet.py
 * ------------------------------------------------------------------------------------------ */

/* Weight repacking into the MFMA staging layout [chunk][tap][ck][rows padded to 16]:
 *   conv3x3 (cout, cin, 3, 3) (unet.py:160,164); tconv (cin, cout, 2, 2) (unet.py:213-215) as a
 *   1x1 GEMM with 4*cout rows; conv1x1 (cout, cin) (unet.py:69).  *_packed_floats sizes `packed`. */
size_t cine_conv3x3_packed_floats(int cout, int cin);
size_t cine_tconv2x2_packed_floats(int cin, int cout);
size_t cine_conv1x1_packed_floats(int cout, int cin);
int cine_pack_conv3x3(const float* w, float* packed, int cout, int cin, void* stream);
int cine_pack_tconv2x2(const float* w, float* packed, int cin, int cout, void* stream);
int cine_pack_conv1x1(const float* w, float* packed, int cout, int cin, void* stream);

/* InstanceNorm statistics travel as PARTIAL records {count, mean, M2}: a tensor (n, c, h, w) carries
 * part (n, c, np, 3).  The conv / tconv kernels emit one record per (sample, channel, output tile)
 * (np = cine_conv_stat_partials(cout, h, w, is_tconv), h/w = the kernel's INPUT grid for tconv);
 * consumers merge them (Chan) into mean and rstd = 1/sqrt(M2/count + eps): biased variance, as
 * nn.InstanceNorm2d (unet.py:161,165,216). */
int cine_conv_stat_partials(int cout, int h, int w, int is_tconv);

/* One ConvBlock half (unet.py:159-162): y = conv3x3(X, pad 1, no bias) and the partial statistics of y.
 * The normalise + LeakyReLU(slope) of y is applied by whichever kernel consumes (y, part_y) next; 0 <= slope <= 1
 * (leaky_relu is evaluated as max(v, v * slope); other slopes are rejected with CINE_EINVAL).
 * X = channel concat (torch.cat, unet.py:122) of up to two sources; source s has c_s channels,
 * extent (h_s, w_s), np_s partial records and mode_s:
 *   0 = use as is;  1 = InstanceNorm + LeakyReLU on load;
 *   2 = mode 1 followed by 2x2 average pool (unet.py:97; the source extent is then ~(2h, 2w)).
 * A source smaller than (h, w) reads as zero outside its extent (up-path zero pad, unet.py:106-120).
 * wpacked2 != NULL: samples >= set_split use wpacked2 (two weight sets in one launch).
 * part_y may be NULL (no statistics). */
int cine_conv3x3_in(const float* x0, const float* part0, int np0, int c0, int mode0, int h0, int w0,
                    const float* x1, const float* part1, int np1, int c1, int mode1, int h1, int w1,
                    const float* wpacked, const float* wpacked2, int set_split,
                    float* y, float* part_y, int n, int cout, int h, int w, float eps, float slope, void* stream);

/* Extended form used by the wavelet CNN (denoisers/mwcnn.py): source modes additionally take
 *   3 = Haar DWT of the source (mwcnn.py:224-236): 4 c_s channels [LL, HL, LH, HH] at (h_s/2, w_s/2)
 *   4 = Haar IWT of the source (mwcnn.py:252-261): c_s/4 channels at (2 h_s, 2 w_s)
 * with bit 3 (| 8) set when the source is raw and must be InstanceNorm + LeakyReLU'd first;
 * add_src1 != 0 ADDS source 1 to source 0 channel-wise (the MWCNN skips, :164,172) instead of
 * concatenating; bias (cout) may be NULL.
 * Epilogue for the convolutional-RNN cells (models/recurrent_varnet.py:153-200): y = conv + bias + addend,
 * then ReLU when relu != 0; addend (n, cout, h, w) may be NULL.  A sum of convolutions of different inputs
 * (i2h + h2h + ih2ih, :172-178) is one convolution over the concatenated inputs with concatenated weights. */
int cine_conv3x3_ex(const float* x0, const float* part0, int np0, int c0, int mode0, int h0, int w0,
                    const float* x1, const float* part1, int np1, int c1, int mode1, int h1, int w1, int add_src1,
                    const float* wpacked, const float* bias, const float* addend, int relu,
                    float* y, float* part_y, int n, int cout, int h, int w, float eps, float slope, void* stream);
/* cine_conv3x3_ex with two weight / bias sets in one launch: samples [0, set_split) use (wpacked, bias), the rest (wpacked2, bias2)
 * (two networks of one topology on planes of equal shape: XPDNet's x-t / y-t MWCNNs, xpdnet.py:424-446). */
int cine_conv3x3_ex2(const float* x0, const float* part0, int np0, int c0, int mode0, int h0, int w0,
                     const float* x1, const float* part1, int np1, int c1, int mode1, int h1, int w1, int add_src1,
                     const float* wpacked, const float* bias, const float* wpacked2, const float* bias2, int set_split,
                     const float* addend, int relu,
                     float* y, float* part_y, int n, int cout, int h, int w, float eps, float slope, void* stream);

/* One step of a convolutional-RNN time sweep (reference models/recurrent_varnet.py:241-254, CRNNcell :172-178 with the
 * input terms precomputed): y = ReLU(conv3x3(x; wpacked) + addend), and accum += y when accum != NULL (the backward sweep
 * adding onto the forward sweep's outputs, :254).  x, addend, y, accum (n, c, h, w); wpacked = cine_pack_conv3x3 of the
 * (c, c, 3, 3) hidden-to-hidden weight (its bias belongs in addend).  y / accum must not alias x or each other. */
int cine_crnn_step(const float* x, const float* wpacked, const float* addend, float* y, float* accum,
                   int n, int c, int h, int w, int relu, void* stream);
/* Both directions of the BCRNN time sweep in one launch (recurrent_varnet.py:241-252: two independent chains, summed at :254):
 * set f and set b are each a cine_crnn_step on their own tensors; store_* != 0 writes accum_* = y_* instead of adding (the
 * first direction to reach a frame).  x_b == NULL runs set f alone.  The sets must not write what the other reads, and must
 * not accumulate into the same tensor. */
int cine_crnn_step2(const float* x_f, const float* addend_f, float* y_f, float* accum_f, int store_f,
                    const float* x_b, const float* addend_b, float* y_b, float* accum_b, int store_b,
                    const float* wpacked, int n, int c, int h, int w, int relu, void* stream);
/* `relu`: 1 = the cell's nn.ReLU (recurrent_varnet.py:178), 0 = no activation (the identity-activation gradient fixtures of
 * tests/test_hip_grad.py, made by the reference with F.relu patched out). */
/* BOTH time sweeps of a BCRNN layer (BCRNNlayer.forward, recurrent_varnet.py:236-254, batch 1) in one call -- the reference's two Python loops
 * over the frames: h_t = [ReLU](conv3x3(h_prev; W_h2h) + P_t) forward in time and backward in time, hid_init = `zero` ((c, h, w) zeros, read
 * only), one cine_crnn_step2 pair launch per step (T launches; T + 1 for odd T, where both chains reach the middle frame in the same step and
 * run one after the other) -- on shapes outside the pair configuration (more than 16 padded rows, ceil(c / 16) * 16 > 16, or a plane of
 * 2 * ceil(fragments / 52) >= 200, e.g. 400 x 208) TWO launches per step, 2 T in all, with the same results --,
 * out = hidden_f + hidden_b (the first chain to reach a frame stores, the second adds: no zero fill, no extra pass).  P (T, c, h, w) = the
 * input terms i2h(x_t) + ih2ih(hid_iter_t) + the three biases for ALL frames (:172-176, one batched launch by the caller), out (T, c, h, w).
 * keep != 0: hf / hb (T, c, h, w) receive every hidden state of the chain (training); keep == 0: hf / hb are (2, c, h, w) ping-pong buffers. */
int cine_bcrnn_sweep(const float* P, const float* wpacked_hh, const float* zero, float* hf, float* hb, float* out,
                     int T, int c, int h, int w, int relu, int keep, void* stream);
/* Back-propagation through time of cine_bcrnn_sweep (keep != 0) -- what torch.autograd unrolls over the reference's two loops: from gout =
 * d loss / d out,  gf[t] = [hf[t] > 0] (conv(gf[t + 1]; Wd) + gout[t]) for t = T-1 .. 0 and gb[t] = [hb[t] > 0] (conv(gb[t - 1]; Wd) + gout[t]) for
 * t = 0 .. T-1, Wd = cine_pack_conv3x3_dgrad of W_h2h (the forward conv kernel; gout rides in as the addend, the ReLU mask is the epilogue's
 * gate; relu == 0: no mask -- hf / hb are then not read but must still be non-NULL: NULL is refused with CINE_EINVAL either way), and gP = gf + gb = d loss / d P.  Launches per step as in cine_bcrnn_sweep; gf, gb, gP (T, c, h, w).  The weight gradients are the
 * caller's: dW_h2h from (hf[t - 1], gf[t]) and (hb[t + 1], gb[t]) with cine_conv3x3_wgrad, everything upstream of P from gP. */
int cine_bcrnn_sweep_bwd(const float* gout, const float* wpacked_hh_dgrad, const float* zero, const float* hf, const float* hb,
                         float* gf, float* gb, float* gP, int T, int c, int h, int w, int relu, void* stream);

/* TransposeConvBlock (unet.py:212-217): y (n, cout, 2h, 2w) = conv_transpose2d(act(x), k 2, s 2, no bias)
 * and the partial statistics of y.  x mode 0|1 as above. */
int cine_tconv2x2_in(const float* x, const float* part_x, int np_x, int mode,
                     const float* wpacked, const float* wpacked2, int set_split,
                     float* y, float* part_y, int n, int cin, int cout, int h, int w,
                     float eps, float slope, void* stream);

/* final 1x1 conv with bias (unet.py:69).  x mode 0|1 as above. */
int cine_conv1x1_bias(const float* x, const float* part_x, int np_x, int mode,
                      const float* wpacked, const float* bias, const float* wpacked2, const float* bias2,
                      int set_split, float* y, int n, int cin, int cout, int h, int w,
                      float eps, float slope, void* stream);

/* Stand-alone statistics of `planes` planes of plane_elems floats: part (planes, 1, 3). */
int cine_instnorm_partials(const float* x, float* part, long planes, long plane_elems, void* stream);
/* merge np partials per plane into stats (planes, 2) = {mean, rstd}. */
int cine_instnorm_finalize(const float* part, float* stats, long planes, int np, float eps, void* stream);
/* materialise act(x) = LeakyReLU((x - mean) * rstd) (block-level parity / debugging). */
int cine_instnorm_lrelu_apply(const float* x, const float* part, int np, float* y, long planes, long plane_elems,
                              float eps, float slope, void* stream);

/* Whole 2-D U-Net (unet.py:73-125) on n planes (n, in_ch, h, w) -> (n, out_ch, h, w).
 * `weights` is a HOST array of device pointers in this order:
 *   for d in 0..pools-1: down[d].conv1 (packed), down[d].conv2 (packed)
 *   bottleneck conv1 (packed), conv2 (packed)
 *   for u in 0..pools-1: tconv[u] (packed), up[u].conv1 (packed), up[u].conv2 (packed)
 *   final 1x1 weight (packed), final bias (out_ch)
 * i.e. 2*pools + 2 + 3*pools + 2 pointers.
 * `nsets` == 2 runs two weight sets over the two halves of the n planes in the SAME launches
 * (the xf and yf U-Nets of one cascade, varnet.py:224-226); `weights` then holds two such arrays
 * back to back.
 * Every cine_unet2d_* / cine_unet3d_* entry point accepts n, h, w (d), in_ch, out_ch, chans > 0, 1 <= pools <= 6 and extents that leave at least
 * one element after `pools` halvings (CINE_EUNSUPPORTED otherwise); the backward passes n <= 65535.  A *_ws_bytes query returns 0 for exactly
 * the shapes its entry point refuses. */
size_t cine_unet2d_ws_bytes(int n, int h, int w, int in_ch, int out_ch, int chans, int pools);
int cine_unet2d_forward(const float* x, float* y, const void* const* weights, int nsets,
                        int n, int h, int w, int in_ch, int out_ch, int chans, int pools, float slope,
                        void* ws, size_t ws_bytes, void* stream);
/* `slope`: the LeakyReLU slope of every ConvBlock (unet.py:162 hard-wires 0.2; 0 <= slope <= 1, 1 = identity -- how
 * tests/test_hip_grad.py compares full-size gradients with reference fixtures made without activation kinks). */

/* ---- 3-D variants (reference unet.py with dims = 3, norm_unet.py:117-219; VarNet / CineNet dynamic_type '3D') ----
 * Volumes are (n, c, d, h, w).  Conv3d 3x3x3 pad 1 (unet.py:48-49), ConvTranspose3d k2 s2 as a GEMM with 8*cout rows,
 * 1x1x1 conv + bias; on-load modes 0 / 1 / 2 (2 = avg_pool3d 2x2x2), concat of two sources, up-path zero pad, bias /
 * addend / ReLU epilogue as in 2-D.  A volume emits cine_conv_stat_partials3d() statistics records per (sample,
 * channel); cine_instnorm_merge folds np records into one. */
size_t cine_conv3d_packed_floats(int cout, int cin);
size_t cine_tconv3d_packed_floats(int cin, int cout);
int cine_pack_conv3d(const float* w, float* packed, int cout, int cin, void* stream);     /* (cout, cin, 3, 3, 3) */
int cine_pack_tconv3d(const float* w, float* packed, int cin, int cout, void* stream);    /* (cin, cout, 2, 2, 2) */
int cine_conv_stat_partials3d(int cout, int d, int h, int w, int is_tconv);
int cine_conv3d_in(const float* x0, const float* part0, int np0, int c0, int mode0, int d0, int h0, int w0,
                   const float* x1, const float* part1, int np1, int c1, int mode1, int d1, int h1, int w1,
                   const float* wpacked, const float* bias, const float* addend, int relu,
                   float* y, float* part_y, int n, int cout, int d, int h, int w, float eps, float slope, void* stream);
int cine_tconv3d_in(const float* x, const float* part_x, int np_x, int mode, const float* wpacked,
                    float* y, float* part_y, int n, int cin, int cout, int d, int h, int w,
                    float eps, float slope, void* stream);
int cine_conv1x1x1_bias(const float* x, const float* part_x, int np_x, int mode, const float* wpacked,
                        const float* bias, float* y, int n, int cin, int cout, int d, int h, int w,
                        float eps, float slope, void* stream);
int cine_instnorm_merge(const float* part, float* out, long planes, int np, void* stream);
/* y (planes, d/2, h/2, w/2) = avg_pool3d(LeakyReLU(InstanceNorm3d(x)), 2) (unet.py:88,97 with dims = 3; part: np statistics records per
 * plane), and the planning query that goes with it: cine_conv3d_pools_on_load() == 1 when cine_conv3d_in serves a mode-2 source of this
 * layer shape inside an efficient kernel (the coarse levels), 0 when the caller does better to pool once with cine_pool3d_act and pass
 * the result as a plain source (what cine_unet3d_forward does for its level 1; same arithmetic, same summation order). */
int cine_pool3d_act(const float* x, const float* part, int np, float* y, long planes, int d, int h, int w,
                    float eps, float slope, void* stream);
int cine_conv3d_pools_on_load(int cout, int d, int h, int w);
/* Whole 3-D U-Net (unet.py:73-125, dims = 3); weights ordered as for cine_unet2d_forward (one set), packed with
 * cine_pack_conv3d / cine_pack_tconv3d / cine_pack_conv1x1. */
size_t cine_unet3d_ws_bytes(int n, int d, int h, int w, int in_ch, int out_ch, int chans, int pools);
int cine_unet3d_forward(const float* x, float* y, const void* const* weights, int n, int d, int h, int w,
                        int in_ch, int out_ch, int chans, int pools, float slope, void* ws, size_t ws_bytes, void* stream);
/* NormUnet3D front / back halves (norm_unet.py:149-219): x (n, t, h, w, 2) -> planes (n, 2, pad16(t), pad16(h),
 * pad16(w)) with group norm (unbiased std) and stats (n, 2, 2); norm == 0 / stats == NULL: plain unpadded repack
 * (CineNet's bare 3-D Unet, cinenet.py:251-253). */
int cine_normunet3d_pack(const float* x, float* planes, float* stats, int n, int t, int h, int w, int norm, void* stream);
int cine_normunet3d_unpack(const float* planes, const float* stats, float* y, int n, int t, int h, int w, void* stream);

/* Whole MWCNN (denoisers/mwcnn.py:135-179) on n planes (n, in_ch, h, w) -> (n, out_ch, h, w); h, w
 * multiples of 2^n_scales (utils/padding.py pads before the call).  Handles the topology XPDNet builds
 * (n_first_convs = 1, res = False, xpdnet.py:251-262); others return CINE_EUNSUPPORTED.
 * `weights` (host array of device pointers, all 3x3 packed with cine_pack_conv3x3):
 *   first_convs[0]; conv_blocks_per_scale[s][i] for s, i in module order; first_convs[1] weight, bias.
 * A pointer may sit in several slots (tied modules); a second set is read slot by slot, whatever the first set ties.
 * Limits: 1 <= n_scales <= 6, 1 <= n_convs[s] <= 4, n_filters[s] > 0 (else CINE_EUNSUPPORTED), and out_ch <= first_filters: the reference
 * constructs a network with out_ch > first_filters (mwcnn.py:124-128) but its forward adds tensors of out_ch and first_filters channels
 * (:172) and raises, so there is nothing to reproduce -- every cine_mwcnn_* entry point returns CINE_EINVAL naming the two counts.  The
 * *_ws_bytes queries return 0 for any argument their entry point refuses by value (sizes, limits, out_ch > first_filters). */
size_t cine_mwcnn_ws_bytes(int n, int h, int w, int in_ch, int out_ch, int n_scales, const int* n_filters,
                           const int* n_convs, int first_filters);
int cine_mwcnn_forward(const float* x, float* y, const void* const* weights, int n, int h, int w,
                       int in_ch, int out_ch, int n_scales, const int* n_filters, const int* n_convs,
                       int n_first_convs, int first_filters, int res, float slope, void* ws, size_t ws_bytes, void* stream);
/* `slope`: the LeakyReLU slope of every conv block (mwcnn.py:204 hard-wires 0.2; 0 <= slope <= 1, 1 = identity). */
/* Two MWCNNs of one topology in ONE launch sequence: samples [0, set_split) through `weights`, the rest through `weights2`
 * (same pointer-array order).  XPDNet's image networks for the x-t and the y-t planes (xpdnet.py:424-446) when both plane sets
 * have the same shape. */
int cine_mwcnn_forward2(const float* x, float* y, const void* const* weights, const void* const* weights2, int set_split,
                        int n, int h, int w, int in_ch, int out_ch, int n_scales, const int* n_filters, const int* n_convs,
                        int n_first_convs, int first_filters, int res, float slope, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * XPDNet primal-buffer plumbing                reference: models/xpdnet.py:301-326, 406-509
 * ------------------------------------------------------------------------------------------ */
/* utils/padding.py:26-47 for one dimension: returns the padded size (multiple of 2^n_scales); odd sizes
 * get the extra element on the left. */
int cine_mwcnn_pad(int size, int n_scales, int* left, int* right);
/* I-step front half (:424-471): buf (b,t,1,h,w,2n) + backward-op image `extra` (b,t,1,h,w,2) as complex
 * channel n, temporal mean subtract, (xf) ifftshift(fft(fftshift(.))) over t, rotation into
 * planes_xf (b*h, 2(n+1), pad(w), pad(t)) / planes_yf (b*w, 2(n+1), pad(h), pad(t)); mean (b,h,w,n+1,2).
 * Limits: 2 <= t <= 64, 1 <= n_primal <= 15, b <= 65535, and one tile of 32 pixels x (n_primal + 1) channels x t frames plus the t
 * twiddles must fit 64 KiB of LDS: (32 t (n_primal + 1) + t) * 8 bytes <= 65536, i.e. t (n_primal + 1) <= 254 (255 with t <= 32; the
 * largest tile is t = 17, n_primal = 14 at 65 416 bytes), else CINE_EUNSUPPORTED.  The adjoint cine_xpd_pack_bwd keeps two such tiles and
 * accepts HALF of that: t (n_primal + 1) <= 127 -- a shape that runs in inference can be refused in training. */
size_t cine_xpd_ws_bytes(int b, int t, int h, int w, int n_primal);
int cine_xpd_pack(const float* buf, const float* extra, float* planes_xf, float* planes_yf, float* mean,
                  int b, int t, int h, int w, int n_primal, int n_scales, int xf, void* ws, size_t ws_bytes, void* stream);
/* I-step back half (:485-509) on the MWCNN outputs (2n channels): unpad, un-rotate, average, inverse
 * temporal transform, add the temporal mean of channels 0..n-1.  out (b,t,1,h,w,2n).
 * Limits: 2 <= t <= 64, b, h <= 65535, (32 t n_primal + t) * 8 bytes <= 65536 (t n_primal <= 254, 255 with t <= 32), else
 * CINE_EUNSUPPORTED; cine_xpd_unpack_bwd has the same tile and also asks for n_primal <= 15. */
int cine_xpd_unpack(const float* planes_xf, const float* planes_yf, const float* mean, float* out,
                    int b, int t, int h, int w, int n_primal, int n_scales, int xf, void* stream);
/* 2-D mode repacks (:442-444): channel-last (n, h, w, c) <-> zero-padded planes (n, c, pad(h), pad(w)). */
int cine_chanlast_to_planes(const float* x, float* planes, int n, int c, int h, int w, int n_scales, void* stream);
int cine_planes_to_chanlast(const float* planes, float* y, int n, int c, int h, int w, int n_scales, void* stream);
/* complex image from channels (c_re, c_im) of a channel-last buffer (:128, :161, :321-326); and
 * repeat_interleave of a complex image into an n-fold buffer (:306-307). */
int cine_extract_complex(const float* buf, float* out, long npix, int c, int c_re, int c_im, void* stream);
int cine_repeat_complex(const float* img, float* buf, long npix, int n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Conjugate-gradient vector ops                reference: reconstruction/models/cinenet.py:136-171
 * ------------------------------------------------------------------------------------------ */
/* *out_dev = sum_i a[i] * b[i] over n floats (torch.dot on the flattened (re, im) pairs, :148,155,163);
 * deterministic two-stage reduction; ws holds cine_dot_ws_bytes(). */
size_t cine_dot_ws_bytes(void);
int cine_dot(const float* a, const float* b, long n, float* out_dev, void* ws, void* stream);
/* out = a + sign * s * b with s read from DEVICE memory: s = *num_dev / *den_dev (den_dev NULL -> 1), or
 * s = softplus(*lambda_dev) when num_dev is NULL.  Covers x + alpha p, r - alpha d, r + beta p (:159-169),
 * the rhs x_ref + v x_reg (:255-257) and H's "+ v x" (:133) without the reference's .item() host syncs. */
int cine_axpby_dev(float* out, const float* a, const float* b, long n, const float* num_dev, const float* den_dev,
                   const float* lambda_dev, float sign, void* stream);
/* One conjugate-gradient iteration after d = H p (:155-169): alpha = rr_old / (p.d); x += alpha p; r -= alpha d; rr_new = r.r;
 * p = r + (rr_new / rr_old) p -- three launches, scalars in device memory, bit-identical to the cine_dot / cine_axpby_dev
 * sequence.  x, r, p updated in place; rr_old_dev != rr_new_dev; ws holds cine_cg_ws_bytes(). */
size_t cine_cg_ws_bytes(void);
int cine_cg_step(float* x, float* r, float* p, const float* d, long n, const float* rr_old_dev, float* rr_new_dev,
                 void* ws, void* stream);
/* cine_cg_step without its p.d pass: ws[0..256) floats already hold the partial sums (cine_normal_op_pd).  Two launches. */
int cine_cg_step_pd(float* x, float* r, float* p, const float* d, long n, const float* rr_old_dev, float* rr_new_dev,
                    void* ws, void* stream);
/* One whole conjugate-gradient iteration of models/cinenet.py:153-169 for a row mask in three launches (h == 200, more than 5 coils;
 * cine_cg_fused_ws_bytes() == 0 otherwise): the operator kernel leaves its coil groups' partial sums in ws_dc (cine_image_dc_ws_bytes) and
 * one partial sum of <p, H p> per workgroup in ws_cg; the update kernel adds the groups + softplus(lambda) p on the fly (H p is never
 * written), alpha, x += alpha p, r -= alpha H p, r.r; the direction kernel beta and p.  x, r, p in place; *pd_out_dev (may be NULL)
 * receives p.Hp.  Same values as cine_normal_op_pd + cine_cg_step_pd up to the summation order of p.Hp. */
size_t cine_cg_fused_ws_bytes(int b, int t, int c, int h, int w);
int cine_normal_op_cg_fused(float* x, float* r, float* p, const float* sens, const uint8_t* mask, const float* lambda_dev,
                            const float* rr_old_dev, float* rr_new_dev, float* pd_out_dev, int b, int t, int c, int h, int w,
                            void* ws_dc, size_t ws_dc_bytes, void* ws_cg, size_t ws_cg_bytes, void* stream);
int cine_normal_op_cg_fused_t(float* x, float* r, float* p, const float* sens, const float* sens_tiled, const uint8_t* mask,
                              const float* lambda_dev, const float* rr_old_dev, float* rr_new_dev, float* pd_out_dev,
                              int b, int t, int c, int h, int w, void* ws_dc, size_t ws_dc_bytes, void* ws_cg, size_t ws_cg_bytes, void* stream);
/* The WHOLE conjugate-gradient solve of CineNet's data-consistency block (models/cinenet.py:136-171: H x = b with exactly `iters`
 * iterations, H = A^H M A + softplus(lambda) I, row mask) in 2 + 2 * iters launches: x (b, t, 1, h, w, 2) holds the start value and
 * receives the solution, rhs = b -- or, with rhs_is_ref != 0, `rhs` holds x_ref and b = x_ref + softplus(lambda) x is formed inside
 * (cinenet.py:106-107: x is then the regulariser's output, start value and regularisation target at once).  Per iteration one operator kernel -- which forms the new direction p = r + beta p on load and
 * needs no direction pass -- and one update kernel (alpha, x, r, the partial sums of r.r).  Same arithmetic as cine_normal_op_cg_fused
 * iterated, except for the summation order of the first r.r.  h == 200 and more than 5 coils (else CINE_EUNSUPPORTED: iterate
 * cine_normal_op / cine_cg_step); sens_tiled: cine_sens_tile_pack's copy or NULL.  ws: cine_conj_grad_ws_bytes(), 8-byte aligned like any
 * complex operand (the coil groups' complex sums lie at its base); the 16-byte {p, r} pairs inside are placed at the next 256-byte
 * boundary by the call itself, whatever the base -- the size query includes those up to 255 bytes. */
size_t cine_conj_grad_ws_bytes(int b, int t, int c, int h, int w);
int cine_conj_grad(float* x, const float* rhs, int rhs_is_ref, const float* sens, const float* sens_tiled, const uint8_t* mask,
                   const float* lambda_dev, int iters, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);
/* cine_conj_grad for TRAINING: the same 2 + 2 * iters launches (+ one 1-block sum), recording what the adjoint recurrence of the iteration needs --
 * the reference detaches its step sizes (cinenet.py:159-169: alpha.item(), beta.item()), so what torch.autograd differentiates is linear in
 * (x0, b) with these constants: p_rec (iters, b, t, 1, h, w, 2) = every direction p_k, rr_rec (iters + 1) = r_k . r_k, pd_rec (iters) = p_k . H p_k. */
int cine_conj_grad_rec(float* x, const float* rhs, int rhs_is_ref, const float* sens, const float* sens_tiled, const uint8_t* mask,
                       const float* lambda_dev, int iters, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes,
                       float* p_rec, float* rr_rec, float* pd_rec, void* stream);
/* cine_cg_step_pd that also stores p.d into *pd_out_dev (training: the adjoint recurrence needs alpha_k = rr_k / pd_k). */
int cine_cg_step_pd2(float* x, float* r, float* p, const float* d, long n, const float* rr_old_dev, float* rr_new_dev,
                     float* pd_out_dev, void* ws, void* stream);
/* Adjoint of ONE conjugate-gradient iteration with recorded step sizes (the reference detaches alpha / beta, cinenet.py:159-169), run from
 * the last iteration to the first: with q = gr_{k+1} + gp_{k+1} and hg = H(q) (cine_normal_op),
 *     gp <- (rr_new / rr) gp + (rr / pd) gx - (rr / pd) hg;   part[0..256) <- partial sums of <q, p_k>;   q <- q + gp
 * in one launch, bit-identical to the cine_axpby_dev / cine_dot / add sequence.  cine_cg_adjoint_finish: gv = - sum_k (rr[k] / pd[k]) <q_k, p_k>
 * from `iters` consecutive partial-sum blocks of cine_cg_adjoint_part_floats() floats (d loss / d softplus(lambda) of the solve, without the
 * - <gb, x0> term). */
size_t cine_cg_adjoint_part_floats(void);
int cine_cg_adjoint_step(float* gp, float* q, const float* gx, const float* hg, const float* pk, long n, const float* rr_dev,
                         const float* pd_dev, const float* rr_new_dev, float* part, void* stream);
int cine_cg_adjoint_finish(const float* part, const float* rr_dev, const float* pd_dev, int iters, float* gv_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * data front-end + sensitivity calibration (the step BEFORE the path)
 *                                              reference: reconstruction/data/mri_data.py:283-303,
 *                                                         reconstruction/data/transforms.py:186-220, 425-432
 * ------------------------------------------------------------------------------------------ */
/* data[:t_out, :, y0:y0+hout, x0:x0+wout] with y0 = (hin - hout) / 2, x0 = (win - wout) / 2 (transforms.py:209-214):
 * in (t_in, c, hin, win, 2) -> out (t_out, c, hout, wout, 2). */
int cine_crop_select(const float* in, float* out, int t_in, int c, int hin, int win, int t_out, int hout, int wout, void* stream);
/* The first step of the front-end for raw k-space of ANY size (mri_data.py:283-289 followed by the crop and frame selection of
 * transforms.py:206-214), without the full image: raw (t_in, nx, ny, c) complex -- the HDF5 `y` layout, read in place -- ->
 * out (t_out, c, cx, cy, 2) = (fftshift o ifft2 o ifftshift)(scale * raw[:t_out]) in ortho normalisation (shifts by N / 2 on both
 * sides), rows x0 = (nx - cx) / 2 .. x0 + cx, columns y0 = (ny - cy) / 2 .. y0 + cy.  Two exact-fp32 complex GEMMs against window
 * DFT matrices built in `ws` on every call; no length limit: any nx, ny >= 1, 1 <= cx <= nx, 1 <= cy <= ny, 1 <= t_out <= t_in,
 * c >= 1 (else CINE_EINVAL), CINE_EUNSUPPORTED only past a grid limit (named in the message).  ws_bytes >= cine_raw_window_ws_bytes()
 * (0 for invalid shapes).  Repeated calls are bit-identical. */
int cine_raw_window_ifft2c(const float* raw, float* out, void* ws, size_t ws_bytes, int t_in, int nx, int ny, int c, int t_out,
                           int cx, int cy, float scale, void* stream);
size_t cine_raw_window_ws_bytes(int t_out, int nx, int ny, int c, int cx, int cy);
/* Scaling and coil-axis move in front of the inverse transform (mri_data.py:283-289: `kspace * scaling`, coils in front of the image
 * axes) for raw sizes the line engines take, kept frames only: raw (t_in, nx, ny, c, 2) -> out (t_out, c, nx, ny, 2),
 * out[t, k, x, y] = scale * raw[t, x, y, k] for t < t_out <= t_in, each component ONE fp32 product.  cine_fft2c on t_out * c images and
 * cine_crop_select follow.  One pass, 16-byte accesses on both sides for any c and ny.  Sizes >= 1, t_out <= t_in, distinct non-null
 * pointers, raw and out 16-byte aligned (else CINE_EINVAL); CINE_EUNSUPPORTED only past the grid limit or the LDS limit (510
 * coils), named in the message. */
int cine_raw_ingest(const float* raw, float* out, int t_in, int nx, int ny, int c, int t_out, float scale, void* stream);
/* SVD coil compression (Buehrer et al., MRM 57:1131, 2007; Huang et al., MRI 26:133, 2008; BART's `cc`) of raw (t_in, nx, ny, c)
 * complex in the HDF5 `y` layout, in front of everything above.  The reference has no such step: its loader takes the coil count
 * the file holds (mri_data.py:283); this engine captures graphs per shape, so a fixed number of virtual coils keeps one graph set.
 * cine_coil_gram: gram (c, c) complex128 (double pairs, row-major), gram[i][j] = sum_{t < t_use} sum_{(x, y) in R} raw[t, x, y, i] *
 * conj(raw[t, x, y, j]) over the central rx x ry block of k-space, rx = min(region, nx), ry = min(region, ny), x0 = nx / 2 - rx / 2,
 * y0 = ny / 2 - ry / 2; region 0 = the whole matrix.  Exact float32 products added in float64 in an order fixed by the shape (no
 * atomics): exactly Hermitian, repeated calls are bit-identical.  ws_bytes >= cine_coil_gram_ws_bytes(t_use, nx, ny, c, region)
 * (0 for invalid shapes and for more than 128 coils).
 * cine_coil_compress: out (t_out, nx, ny, v) complex, out[t, x, y, j] = sum_k matrix[j][k] raw[t, x, y, k] with matrix (v, c) complex
 * row-major (the leading eigenvectors of gram, conjugated; the eigen-decomposition itself is the caller's): one pass over the
 * samples, exact fp32 (a k-ordered fmaf chain on v_mfma_f32_16x16x4_f32), repeated calls are bit-identical.
 * Both: 1 <= t_use, t_out <= t_in, sizes >= 1, region >= 0, 1 <= v <= c, distinct non-null pointers, raw / gram / ws / out 16-byte
 * aligned (else CINE_EINVAL); at most 128 coils and 32 virtual coils (else CINE_EUNSUPPORTED, the limit is in the message). */
size_t cine_coil_gram_ws_bytes(int t, int nx, int ny, int c, int region);
int cine_coil_gram(const float* raw, double* gram, void* ws, size_t ws_bytes, int t_in, int nx, int ny, int c, int t_use, int region,
                   void* stream);
int cine_coil_compress(const float* raw, const float* matrix, float* out, int t_in, int nx, int ny, int c, int t_out, int v,
                       void* stream);
/* The eigen-decomposition between the two, on the device: gram (nb, c, c) complex128 as cine_coil_gram writes it -> matrix (nb, v, c)
 * complex64, lam (nb, c) doubles in descending order (equal values by column index), info (nb, 4) doubles.  With G = U diag(lam) U^H:
 * matrix[r] = conj(U[:, r]) times the unit phase that makes its largest-magnitude entry (float64 magnitudes, the lowest index among
 * equal ones) real and positive; that entry is stored with imaginary part 0, every entry is rounded once to complex64; a zero or NaN
 * peak leaves the row's phase alone.  Only the upper triangle of gram is read (mirrored, the diagonal's imaginary part taken as 0), so
 * the input is Hermitian by construction.  One workgroup per matrix, everything in LDS in float64: the cyclic Jacobi eigensolver of
 * cine_svt_weight (until max |off-diagonal| <= 1e-14 max |diagonal| or 40 sweeps; a NaN ends at the cap).  info: the residual max
 * |off-diagonal| / max |diagonal| reached, the sweeps used, the kept share sum(lam[:v]) / sum(lam) (1 for a zero matrix), lam[0].
 * nb >= 1, c >= 1, 1 <= v <= c, distinct non-null pointers, gram 16-byte and the outputs 8-byte aligned (else CINE_EINVAL); at most 64
 * coils (the two c x c float64 matrices fill the LDS; cine_coil_gram and cine_coil_compress go on to 128) and 32 virtual coils (else
 * CINE_EUNSUPPORTED, the limit is in the message).  Every argument is checked before the launch; no allocation, no host read, no
 * atomics: capturable, and the same bits on every call. */
int cine_coil_matrix(const double* gram, float* matrix, double* lam, double* info, int nb, int c, int v, void* stream);
/* Noise pre-whitening folded into the compression matrix.  Noise samples eta_s (c channels, s < n) have the covariance
 * Psi[i][j] = 1/n sum_s eta_s[i] conj(eta_s[j]) (the index convention of cine_coil_gram) = L L^H, L lower-triangular with a real positive
 * diagonal; the whitener is W = s L^-1 (s = sqrt(trace(Psi) / c) keeps the data's overall level, or s = 1), so W Psi W^H = s^2 I.  A
 * whitened sample is d' = W d and its calibration Gram matrix G' = W G W^H.  cine_coil_matrix_whitened is cine_coil_matrix of G' composed
 * with W: with G' = U diag(lam) U^H (lam descending, equal values by column index),
 *     matrix[r][:] = p_r sum_k conj(U[k][r]) W[k][:],  r < v,
 * p_r the unit phase that makes the row's largest-magnitude entry real and positive (float64 magnitudes, the lowest index among equal
 * ones; stored with imaginary part 0; every entry rounded once to complex64).  matrix Psi matrix^H = s^2 I_v and matrix G matrix^H =
 * diag(lam[:v]); the rows are not orthonormal.  cine_coil_compress with this matrix whitens and compresses in its one pass.
 * gram (nb, c, c) complex128 as cine_coil_gram writes it (the upper triangle is read); whitener (c, c) complex128 row-major, shared by
 * all nb matrices (one scan, many slices): only its lower triangle with the diagonal is read, the diagonal's imaginary part is taken as
 * 0.  Outputs, info, limits and checks as cine_coil_matrix, info for G'; whitener non-null, 16-byte aligned, aliasing nothing.  The same
 * kernel: B = W G, G' = B W^H (one triangle, mirrored: exactly Hermitian with a real diagonal) and the eigenvector accumulator started
 * at W^H instead of the identity, all within the two c x c float64 matrices in LDS; the identity as whitener gives the bits of
 * cine_coil_matrix.  No allocation, no host read, no atomics: capturable, and the same bits on every call. */
int cine_coil_matrix_whitened(const double* gram, const double* whitener, float* matrix, double* lam, double* info,
                              int nb, int c, int v, void* stream);
/* One axis pass of scipy.ndimage.gaussian_filter as transforms.py:216-217 calls it (mode 'reflect', truncate 4.0, weights and
 * accumulation in float64, float32 result) over a (outer, n, inner) array of complex pairs: the real and imaginary parts
 * are filtered alike.  The caller runs one pass per axis with sigma > 0, in axis order (mri_data.py:279: [0.7, 0, 0.3, 0.3]). */
int cine_gauss_axis(const float* in, float* out, long outer, int n, long inner, double sigma, void* stream);
/* target = center_crop(|sum_c img * conj(sens)|, (ch, cw))  (mri_data.py:302-303, transforms.py:136-158):
 * img (t, c, h, w, 2), sens (c, h, w, 2) -> out (t, ch, cw). */
int cine_combine_target(const float* img, const float* sens, float* out, int t, int c, int h, int w, int ch, int cw, void* stream);
/* ESPIRiT calibration in place of `bart ecalib` (mri_data.py:296 `-r 200`, transforms.py:429 `-r 15`; BART is a third-party
 * program the reference shells out to).  proj = V V^H (kk*kk*c square, complex pairs, index (py, px, coil)) is the
 * projector onto the row space of the calibration matrix; cine_espirit_lag_kernels writes the (2 kk - 1)^2 lag kernels of
 * every coil pair, centered and scaled, into kpad (c*c, ny, nx, 2) so that cine_fft2c(kpad, inverse) is the c x c
 * image-space operator M(r) of every pixel.  cine_espirit_eig: dominant eigenpair of M(r) by `iters` power iterations;
 * maps (c, npix, 2) unit norm with coil 0 real and non-negative, zero where the eigenvalue < crop; lam (npix). */
int cine_espirit_lag_kernels(const float* proj, float* kpad, int c, int kk, int ny, int nx, void* stream);
int cine_espirit_eig(const float* m, float* maps, float* lam, int c, long npix, int iters, float crop, void* stream);
/* The dense steps of that calibration without an eigensolver: a fixed launch sequence, no host read, capturable by a hipGraph.
 * cine_espirit_gram: kavg (c, ny, nx) complex64 -> gram (n, n) complex128 row-major, n = kk kk c, the Gram matrix A^H A of the kk x kk
 * patch matrix A of the central min(r, ny) x min(r, nx) block (origin ny / 2 - ry / 2, nx / 2 - rx / 2; columns ordered (py, px, coil)).
 * Exact float32 products added in float64 in patch order: the full matrix, exactly Hermitian, bit-identical from call to call.  Any
 * r >= 1; the block must hold one kernel (else CINE_EINVAL); c <= 32 and n <= 1152 (else CINE_EUNSUPPORTED, the limit is in the message);
 * ws_bytes >= cine_espirit_gram_ws_bytes() (0 for shapes it refuses), gram and ws 16-byte aligned.
 * cine_zgemm_f64: out = alpha a b + beta d for n x n row-major complex128 matrices (double pairs) on v_mfma_f64_16x16x4_f64, four real
 * MFMAs per complex product, k ascending: deterministic.  Any 1 <= n <= 1152 (ragged tiles are handled inside); d is not read when
 * beta == 0 (it may be NULL); out may be d, not a or b; 16-byte aligned.
 * cine_espirit_projector: proj_f32 (n, n) complex64 = 1/2 (I + sign(gram - thresh^2 lam I)), the projector onto the eigenvectors of
 * the Hermitian gram with eigenvalue >= thresh^2 lam_max, which is what cine_espirit_lag_kernels takes.  lam_dev: the largest eigenvalue
 * (8 squarings of gram, renormalised by the Frobenius norm after each, then the Rayleigh quotient of the row sums).  The sign: `iters`
 * Newton-Schulz steps X <- 1.5 X - 0.5 X X^2 from X_0 = (gram - thresh^2 lam I) / (1.0001 lam), two GEMMs each.  resid_dev:
 * max |X^2 - I| of the X handed out, from one more GEMM behind the last step (NaN if the iteration left the finite numbers): above
 * 1e-6 an eigenvalue sits at the threshold and `iters` is too small.  iters >= 1, thresh > 0, non-null distinct pointers (else
 * CINE_EINVAL); n <= 1152 (else CINE_EUNSUPPORTED); ws_bytes >= cine_espirit_projector_ws_bytes(n) (else CINE_EWORKSPACE).
 * All three: every argument is checked before the first launch; no allocation, no synchronisation, no atomics. */
size_t cine_espirit_gram_ws_bytes(int c, int ny, int nx, int r, int kk);
int cine_espirit_gram(const float* kavg, double* gram, void* ws, size_t ws_bytes, int c, int ny, int nx, int r, int kk, void* stream);
int cine_zgemm_f64(const double* a, const double* b, const double* d, double* out, int n, double alpha_re, double alpha_im,
                   double beta_re, double beta_im, void* stream);
size_t cine_espirit_projector_ws_bytes(int n);
int cine_espirit_projector(const double* gram, int n, double thresh, int iters, float* proj_f32, double* lam_dev, double* resid_dev,
                           void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * small element-wise helpers                   reference: reconstruction/utils/math.py
 * ------------------------------------------------------------------------------------------ */
int cine_complex_abs(const float* x, float* y, long n, void* stream);          /* math.py:48-62 */

/* ------------------------------------------------------------------------------------------
 * Training: gradients through the path
 *   reference: what torch.autograd differentiates in reconstruction/pl_modules/varnet_module.py:97-113 (training_step:
 *   forward + SSIMLoss) -- models/varnet.py:143-151, 181-282; denoisers/norm_unet.py:59-114; denoisers/unet.py:73-125, 159-218
 * Conventions: the gradient of a complex tensor is the pair (d loss / d re, d loss / d im), i.e. d loss = Re(conj(g) dx);
 * weight gradients are ACCUMULATED (+=) into caller-zeroed tensors in the parameters' own layouts; every reduction runs in a
 * fixed order (no atomics): two backward passes over the same data give bit-identical gradients.
 * ------------------------------------------------------------------------------------------ */

/* Input-gradient packings of the U-Net weights: the gradient of a convolution with respect to its input is a convolution of the
 * output gradient -- conv3x3 with (cout, cin) swapped and the taps flipped (unet.py:160,164); the k2 s2 transpose conv with its
 * (cin, 4 cout) weight matrix over the space-to-depth view of the output gradient (unet.py:213-215); the 1x1 conv with the
 * transposed matrix (unet.py:69).  `w` are the parameters in their own layouts. */
size_t cine_conv3x3_dgrad_packed_floats(int cout, int cin);
size_t cine_tconv2x2_dgrad_packed_floats(int cin, int cout);
size_t cine_conv1x1_dgrad_packed_floats(int cout, int cin);
int cine_pack_conv3x3_dgrad(const float* w, float* packed, int cout, int cin, void* stream);
int cine_pack_tconv2x2_dgrad(const float* w, float* packed, int cin, int cout, void* stream);
int cine_pack_conv1x1_dgrad(const float* w, float* packed, int cout, int cin, void* stream);
/* Batched packing (training re-packs every weight after every optimiser step: hundreds of 4-us launches per step otherwise).  cine_pack_desc writes
 * into HOST memory (cine_pack_desc_bytes() each) the descriptor of one tensor: op 0 = cine_pack_conv3x3 (n1 = cout, n2 = cin), 1 = cine_pack_tconv2x2
 * (cin, cout), 2 = cine_pack_conv1x1 (cout, cin), 3 = cine_pack_conv3x3_dgrad (cout, cin), 4 = cine_pack_tconv2x2_dgrad (cin, cout),
 * 5 = cine_pack_conv1x1_dgrad (cout, cin): the same arguments, layout and size as that entry point.  The caller copies the array to the device once
 * (parameters and packed buffers keep their addresses across steps); cine_pack_batch re-packs all n of them in ONE launch (max_total: the largest
 * packed size in floats, for the grid). */
size_t cine_pack_desc_bytes(void);
int cine_pack_desc(void* desc_host, int op, const float* w, float* packed, int n1, int n2);
int cine_pack_batch(const void* descs_dev, int n, long max_total, void* stream);
/* gx = d loss / d (conv input) from gy = d loss / d (raw conv output); wpacked* from the packings above (two sets: samples
 * >= set_split use wpacked2, NULL = one set).  conv3x3: gy (n, cout, h, w) -> gx (n, cin, h, w); tconv: gy (n, cout, 2h, 2w) ->
 * gx (n, cin, h, w); conv1x1: gy (n, cout, h, w) -> gx (n, cin, h, w). */
int cine_conv3x3_dgrad(const float* gy, const float* wpacked, const float* wpacked2, int set_split,
                       float* gx, int n, int cout, int cin, int h, int w, void* stream);
int cine_tconv2x2_dgrad(const float* gy, const float* wpacked, const float* wpacked2, int set_split,
                        float* gx, int n, int cin, int cout, int h, int w, void* stream);
/* cine_conv3x3_dgrad with the chain rule of a ReLU'd input in the epilogue: gx = gate > 0 ? (conv(gy) + addend) : 0, where gate (n, cin, h, w)
 * is the stored ReLU output that was the conv's input and addend (n, cin, h, w) the gradient it receives from its other consumers (either
 * may be NULL).  The conv blocks of the CRNN body (reference recurrent_varnet.py:122-134): x_k feeds conv_{k+1}_x AND the next cascade's
 * conv_k_h, torch.autograd adds the two gradients and applies the ReLU mask in separate kernels. */
int cine_conv3x3_dgrad_gated(const float* gy, const float* wpacked, const float* addend, const float* gate,
                             float* gx, int n, int cout, int cin, int h, int w, void* stream);
int cine_conv1x1_dgrad(const float* gy, const float* wpacked, const float* wpacked2, int set_split,
                       float* gx, int n, int cout, int cin, int h, int w, void* stream);

/* cine_unet2d_forward that KEEPS every layer's raw output and statistics in `ws` (cine_unet2d_train_ws_bytes) for the backward
 * pass; same arguments and results as cine_unet2d_forward. */
size_t cine_unet2d_train_ws_bytes(int n, int h, int w, int in_ch, int out_ch, int chans, int pools);
int cine_unet2d_forward_train(const float* x, float* y, const void* const* weights, int nsets,
                              int n, int h, int w, int in_ch, int out_ch, int chans, int pools, float slope,
                              void* ws, size_t ws_bytes, void* stream);
/* cine_unet2d_forward / cine_unet2d_forward_train (`train` != 0) with the n planes cut into nside + 1 contiguous runs that go through the
 * SAME launch sequence concurrently: run 0 on `stream`, run k on side[k - 1] (HOST array of caller-owned streams, none of them `stream`),
 * forked from `stream` and joined back into it with events before the call returns -- on return everything is ordered on `stream`
 * again.  The planes of a U-Net pass are independent (the x-f and y-f networks of a cascade, reference varnet.py:216-232, meet only in
 * the sum behind them; the coils of the sensitivity network, varnet.py:76-86, only in the RSS), but on one stream every layer boundary
 * drains the chip (a cfg-2 level-1 layer is 800 workgroups on 768 resident slots): with two runs each one's next layer fills the slots
 * the other's last round leaves empty.  Same kernels, tiles and per-plane statistics records: outputs are BIT-IDENTICAL to the
 * one-stream call.  nsets == 2: nside + 1 must be even (a run never spans both weight sets).  Workspace: cine_unet2d_branch_ws_bytes
 * (inference: one private workspace per run; training: the layout of cine_unet2d_train_ws_bytes, which cine_unet2d_backward reads).
 * Capturable: inside a stream capture the side streams join the capture through the fork event.  The reference runs the two networks
 * one after the other on torch's current stream.
 * nside > 0 (inference) also tells the dispatcher that this slice runs beside nothing but its own branches: the 128-channel bottleneck
 * then launches two 64-row workgroups per plane instead of one of 128 rows (same pixel tiling, same statistics records, same bits; faster
 * for a slice alone, slower with many slices in flight -- which run one stream each and pass nside == 0). */
size_t cine_unet2d_branch_ws_bytes(int n, int h, int w, int in_ch, int out_ch, int chans, int pools, int nsets, int nbranch, int train);
int cine_unet2d_forward_branches(const float* x, float* y, const void* const* weights, int nsets,
                                 int n, int h, int w, int in_ch, int out_ch, int chans, int pools, float slope,
                                 void* ws, size_t ws_bytes, void* stream, void* const* side, int nside, int train, const float* drop);
/* Dropout (unet.py:22,40,159-168: Dropout2d behind every LeakyReLU of a ConvBlock, active in training mode with drop_prob > 0).  `drop` of
 * cine_unet2d_forward_branches (train != 0 only; NULL = none) holds the multiplier d of every (3x3 conv, sample, channel) plane -- 0 for a
 * dropped channel, 1 / (1 - p) for a kept one -- drawn by the CALLER (the binding uses torch's generator, like nn.Dropout2d): one (n, ch) block
 * per 3x3 conv in launch order (down path and bottleneck level d: two blocks of chans << d channels; up path from the coarsest level: two blocks
 * each; the transpose-conv blocks have no dropout), cine_unet2d_drop_floats(n, chans, pools) floats in all.  d >= 0 commutes with LeakyReLU, so
 * the forward folds it into the plane's InstanceNorm statistics records and no activation is ever rewritten; cine_unet2d_backward_drop is
 * cine_unet2d_backward with the same array. */
size_t cine_unet2d_drop_floats(int n, int chans, int pools);
/* The same for the 3-D U-Net (Dropout3d: whole (sample, channel) volumes): cine_unet3d_forward_train / cine_unet3d_backward with `drop` in the layout above. */
int cine_unet3d_forward_train_drop(const float* x, float* y, const void* const* weights, int n, int d, int h, int w,
                                   int in_ch, int out_ch, int chans, int pools, float slope, void* ws, size_t ws_bytes, const float* drop, void* stream);
int cine_unet3d_backward_drop(const float* x, const float* gy, const void* const* wdgrad, void* const* grads,
                              int n, int d, int h, int w, int in_ch, int out_ch, int chans, int pools, float slope,
                              const void* fwd_ws, size_t fwd_ws_bytes, void* ws, size_t ws_bytes, float* gx, const float* drop, void* stream);
int cine_unet2d_backward_drop(const float* x, const float* gy, const void* const* wdgrad, void* const* grads, int nsets,
                              int n, int h, int w, int in_ch, int out_ch, int chans, int pools, float slope,
                              const void* fwd_ws, size_t fwd_ws_bytes, void* ws, size_t ws_bytes, float* gx, const float* drop, void* stream);
/* The reference's small tensor helpers as device kernels, for user code written against its utils (the fused path never calls
 * them).  utils/math.py:20-44: complex_mul with broadcasting -- `shape` = the broadcast result's dimensions WITHOUT the trailing
 * complex pair (at most 6), `xstride` / `ystride` the operands' strides in complex elements, 0 on broadcast dimensions; out is dense.
 * complex_conj, complex_abs_sq: n complex elements.  utils/coil_combine.py: out (outer, inner) = sqrt(sum_k v(x[outer][k][inner])),
 * v = x^2 or, with is_complex, re^2 + im^2 of (outer, k, inner, 2).  utils/fftc.py:141-213 roll along one dimension:
 * out[o][(j + shift) mod n][i] = x[o][j][i] (out of place; fftshift = shift n / 2, ifftshift = (n + 1) / 2).
 * utils/padding.py:22-47: zero padding of `planes` (h, w) planes to (hp, wp) with the data at (top, left). */
int cine_complex_mul(const float* x, const float* y, float* out, int ndim, const int* shape, const long* xstride, const long* ystride, void* stream);
int cine_complex_conj(const float* x, float* out, long n, void* stream);
int cine_complex_abs_sq(const float* x, float* out, long n, void* stream);
int cine_rss(const float* x, float* out, long outer, int k, long inner, int is_complex, void* stream);
int cine_roll(const float* x, float* out, long outer, int n, long inner, int shift, void* stream);
int cine_pad2d(const float* x, float* out, long planes, int h, int w, int top, int left, int hp, int wp, void* stream);

/* Diagnostics.  3x3 convolutions whose tile spans the plane's width (the x-f / y-f planes of the cascade U-Nets, reference
 * denoisers/unet.py:159-168) and the k2 s2 transpose convs between them (unet.py:212-218) run on lean kernels (csrc/conv_plane.hip)
 * that are BIT-IDENTICAL to the general one (except a Haar-DWT source, mode 3, whose K chunks the lean kernel forms from two source
 * channels x four bands instead of eight channels of one band: the same sums in another order), and so do the 3x3 (x3) convolutions of
 * wider planes and volumes in 16-wide column
 * tiles (sensitivity network, CRNN cells, 3-D U-Net); `on` is a mask -- bit 0 the plane-wide 3x3 convolutions, bit 1 the
 * transpose convolutions, bit 2 the wide planes / volumes; a cleared bit routes that kind through the general kernel (the
 * bit-identity tests, A/B timing).  Bit 3 SET makes the plane-wide 3x3 convolutions of 2-wide planes (the U-Net bottleneck, the MWCNN's
 * coarsest scale) sweep all nine taps over fragments of 8 rows x both columns, the form before the column-pure sweep that skips the taps
 * which only read the zero halo column, and those of 4-wide planes with 33 .. 64 output rows (U-Net level 2: one wave per 52-row plane tile)
 * sweep all nine taps over fragments of 4 rows x all four columns instead of 12 column-pure fragments of 16 rows + one canonical fragment
 * (bit-identical; 15 = every lean kernel in that older form).  Bit 4 SET routes the plane-wide weight gradients of training (grad_kernels.hip:
 * wgrad_plane_kernel, also bit-identical) through the general weight-gradient kernel.  A setting of the CALLING THREAD (default 7
 * in every thread): it selects kernels for the launches that thread enqueues afterwards and changes no result but for that
 * summation order. */
int cine_set_conv_plane(int on);

/* A second stream of the CALLING THREAD for the weight-gradient launches of cine_unet2d_backward / cine_unet3d_backward / cine_mwcnn_backward (they
 * depend only on a layer's output gradient, not on the input-gradient chain behind it): the calls fork onto it with events
 * and join before returning, so on return everything is ordered on `stream` again and the results do not depend on timing.
 * NULL (the default) or the same stream as `stream`: every launch stays on `stream`.  Replaces nothing in the reference
 * (torch.autograd runs its backward nodes on one stream); it is how `loss.backward()` (pl_modules/varnet_module.py:97-113) fills
 * the chip. */
int cine_set_side_stream(void* side_stream);
/* Backward pass of the U-Net (the autograd graph of unet.py:73-125): from gy = d loss / d y, the forward's input x and its
 * filled workspace `fwd_ws`.  `wdgrad`: HOST array of device pointers ordered like `weights` of the forward, holding the
 * input-gradient packings (the bias slot is ignored).  `grads`: HOST array in the same order of device pointers to the weight
 * gradients ((cout, cin, 3, 3) / (cin, cout, 2, 2) / (out_ch, chans) / (out_ch)), accumulated into.  nsets == 2: both arrays
 * hold two such lists back to back.  gx (n, in_ch, h, w) may be NULL (the sensitivity network's input needs no gradient).
 * ws: cine_unet2d_backward_ws_bytes() of scratch. */
size_t cine_unet2d_backward_ws_bytes(int n, int h, int w, int in_ch, int out_ch, int chans, int pools);
int cine_unet2d_backward(const float* x, const float* gy, const void* const* wdgrad, void* const* grads, int nsets,
                         int n, int h, int w, int in_ch, int out_ch, int chans, int pools, float slope,
                         const void* fwd_ws, size_t fwd_ws_bytes, void* ws, size_t ws_bytes, float* gx, void* stream);

/* The same for the 3-D U-Net (unet.py:73-125 with dims = 3; CineNet's regulariser, cinenet.py:98-116): cine_unet3d_forward_train is
 * cine_unet3d_forward with every raw layer output and its merged statistics record kept in `ws` (cine_unet3d_train_ws_bytes), and
 * cine_unet3d_backward walks it in reverse.  `wdgrad` (order of `weights`, bias slot ignored): cine_pack_conv3d of each 3x3x3 weight with its taps
 * flipped and (cout, cin) transposed; cine_pack_conv1x1 of a transpose conv's weight (cin, cout, 2, 2, 2) read as the (cin, 8 cout) matrix;
 * cine_pack_conv1x1 of the final conv's matrix transposed (chans, out_ch).  The pack calls take the ROWS of the packed matrix first: for a 3x3x3
 * weight (cout, cin, 3, 3, 3) cine_pack_conv3d(flipped and transposed weight (cin, cout, 3, 3, 3), packed, cin, cout); for a transpose conv (cin, cout,
 * 2, 2, 2) cine_pack_conv1x1(w, packed, cin, 8 cout); for the final conv cine_pack_conv1x1(transposed matrix, packed, chans, out_ch); sizes from
 * cine_conv3d_packed_floats / cine_conv1x1_packed_floats with the same two counts.  `grads`: the parameters' own layouts ((cout, cin, 3, 3, 3) /
 * (cin, cout, 2, 2, 2) / (out_ch, chans) / (out_ch)), accumulated into.  One weight set.  gx (n, in_ch, d, h, w) may be NULL.
 * Weight gradients run on the calling thread's side stream (cine_set_side_stream) when it has one. */
size_t cine_unet3d_train_ws_bytes(int n, int d, int h, int w, int in_ch, int out_ch, int chans, int pools);
int cine_unet3d_forward_train(const float* x, float* y, const void* const* weights, int n, int d, int h, int w,
                              int in_ch, int out_ch, int chans, int pools, float slope, void* ws, size_t ws_bytes, void* stream);
size_t cine_unet3d_backward_ws_bytes(int n, int d, int h, int w, int in_ch, int out_ch, int chans, int pools);
int cine_unet3d_backward(const float* x, const float* gy, const void* const* wdgrad, void* const* grads,
                         int n, int d, int h, int w, int in_ch, int out_ch, int chans, int pools, float slope,
                         const void* fwd_ws, size_t fwd_ws_bytes, void* ws, size_t ws_bytes, float* gx, void* stream);

/* The same for the wavelet CNN (denoisers/mwcnn.py:135-179): a forward that keeps every feature map, and the backward pass -- InstanceNorm +
 * LeakyReLU backward with the Haar DWT / IWT adjoints (the transforms are orthogonal: each one's adjoint is the other) and the additive
 * skips gathered on load, input gradients on the forward conv kernel, weight gradients with the wavelet / summed sources re-staged.
 * weights / weights2, set_split as cine_mwcnn_forward2 (weights2 NULL: one network); wdgrad*: the cine_pack_conv3x3_dgrad packings in the
 * order of `weights` (bias slot ignored); grads*: the parameters' own layouts, accumulated into.  cine_mwcnn_backward: n <= 65535, h and w
 * multiples of 2^n_scales and out_ch <= first_filters as in the forward (CINE_EINVAL otherwise, before anything is launched); gx may be NULL;
 * x, gy and fwd_ws are only read. */
size_t cine_mwcnn_train_ws_bytes(int n, int h, int w, int in_ch, int out_ch, int n_scales, const int* n_filters,
                                 const int* n_convs, int first_filters);
int cine_mwcnn_forward_train(const float* x, float* y, const void* const* weights, const void* const* weights2, int set_split,
                             int n, int h, int w, int in_ch, int out_ch, int n_scales, const int* n_filters, const int* n_convs,
                             int n_first_convs, int first_filters, int res, float slope, void* ws, size_t ws_bytes, void* stream);
size_t cine_mwcnn_backward_ws_bytes(int n, int h, int w, int in_ch, int out_ch, int n_scales, const int* n_filters,
                                    const int* n_convs, int first_filters);
int cine_mwcnn_backward(const float* x, const float* gy, const void* const* wdgrad, const void* const* wdgrad2, void* const* grads,
                        void* const* grads2, int set_split, int n, int h, int w, int in_ch, int out_ch, int n_scales,
                        const int* n_filters, const int* n_convs, int first_filters, float slope, const void* fwd_ws, size_t fwd_ws_bytes,
                        void* ws, size_t ws_bytes, float* gx, void* stream);

/* Adjoints of cine_normunet_unpack / cine_normunet_pack (norm_unet.py:59-96).
 *   unpack_bwd: gout (n, h, w, 2), the U-Net output planes_q -> gq (planes, zero on the pad frame) and dstats (n, 2, 2) =
 *               {d/d mean, d/d std} per (sample, re|im) from the un-normalisation x * std + mean.
 *   pack_bwd  : gp (gradient of the U-Net input planes), the planes themselves, stats, dstats -> gz (n, h, w, 2), through
 *               (x - mean) / std with the unbiased std.  stats == NULL: the plain repack (cinenet.py:242-244). */
int cine_normunet_unpack_bwd(const float* gout, const float* planes_q, const float* stats, float* gq, float* dstats,
                             int n, int h, int w, void* stream);
int cine_normunet_pack_bwd(const float* gp, const float* planes_p, const float* stats, const float* dstats, float* gz,
                           int n, int h, int w, void* stream);
/* Adjoints of cine_xfyf_unpack / cine_xfyf_pack (varnet.py:196-241): gout (b, t, 1, h, w, 2) -> gradients of the two U-Nets'
 * output planes (+ dstats, and gmean (b, h, w, 2) = the gradient of the temporal mean image); then from the gradients of the
 * U-Nets' input planes -> gimg (b, t, h, w, 2).  The temporal DFT is unitary: its adjoint is the inverse transform.
 * ws: cine_xfyf_bwd_ws_bytes(). */
size_t cine_xfyf_bwd_ws_bytes(int b, int t, int h, int w);
int cine_xfyf_unpack_bwd(const float* gout, const float* q_xf, const float* q_yf, const float* stats_xf, const float* stats_yf,
                         float* gq_xf, float* gq_yf, float* dstats_xf, float* dstats_yf, float* gmean,
                         int b, int t, int h, int w, int xf, void* ws, size_t ws_bytes, void* stream);
int cine_xfyf_pack_bwd(const float* gp_xf, const float* gp_yf, const float* p_xf, const float* p_yf,
                       const float* stats_xf, const float* stats_yf, const float* dstats_xf, const float* dstats_yf,
                       const float* gmean, float* gimg, int b, int t, int h, int w, int xf,
                       void* ws, size_t ws_bytes, void* stream);

/* Backward pieces of the convolutional-RNN cells (models/recurrent_varnet.py:153-259: sums of plain 3x3 convolutions + bias, ReLU).
 * cine_relu_mask: g *= (y > 0) in place, y = the stored ReLU output.  cine_conv3x3_wgrad: gw (cout, c0 + c1, 3, 3) += the weight
 * gradient of y = conv3x3(cat(x0, x1); W) from g = d loss / d y (x1 NULL / c1 0: one input), gb (cout) += the bias gradient when
 * not NULL; deterministic (partial sums in `ws`, fixed-order reduction).  The input gradient is cine_conv3x3_dgrad, or
 * cine_conv3x3_ex on the cine_pack_conv3x3_dgrad packing when an addend rides along (the time sweep's chain rule). */
int cine_relu_mask(float* g, const float* y, long n, void* stream);
size_t cine_conv3x3_wgrad_ws_bytes(int cout, int cin, int n);
int cine_conv3x3_wgrad(const float* x0, int c0, const float* x1, int c1, const float* g, float* gw, float* gb,
                       int n, int cout, int h, int w, void* ws, size_t ws_bytes, void* stream);

/* Layer-level backward pieces (the 3-D U-Net's backward pass is composed from these, cine_hip/autograd.py: Unet3dFn).
 * cine_conv1x1_wgrad: gw (cout, cin) += weight gradient of a 1x1(x1) convolution, gb (cout) += bias gradient when not NULL.
 * cine_in_lrelu_bwd: d loss / d raw from d loss / d LeakyReLU(InstanceNorm(raw)) (unet.py:159-168) for planes (n, c) of h * w
 * elements with statistics records part (n, c, np, 3).  Volumes pass (d h, w). */
size_t cine_conv1x1_wgrad_ws_bytes(int cout, int cin, int n);
int cine_conv1x1_wgrad(const float* x, int cin, const float* g, float* gw, float* gb, int n, int cout, int h, int w,
                       void* ws, size_t ws_bytes, void* stream);
size_t cine_in_lrelu_bwd_ws_bytes(int n, int c, int h, int w);      /* 0 for small planes; large ones are cut into chunks (ws may be NULL then: one workgroup per plane) */
int cine_in_lrelu_bwd(const float* r, const float* part, int np, const float* g, float* gr, int n, int c, int h, int w,
                      float eps, float slope, void* ws, size_t ws_bytes, void* stream);

/* Adjoints of cine_xpd_unpack / cine_xpd_pack (models/xpdnet.py:424-509): gout (b, t, 1, h, w, 2n) -> the gradients of the two MWCNNs' output
 * planes (2n channels, zero on the pad frames) and gmean (b, h, w, n + 1, 2) (the temporal mean of channels < n is added back, :504-509); then
 * from the gradients of the MWCNNs' input planes (2 (n + 1) channels) -> gbuf (b, t, 1, h, w, 2n) and gextra (b, t, 1, h, w, 2) (the
 * backward-operator image).  XPDNet's temporal transforms (:466, :500) are unitary: each adjoint is the inverse with the same shifts.
 * LDS limits (CINE_EUNSUPPORTED above them): cine_xpd_unpack_bwd as cine_xpd_unpack, (32 t n_primal + t) * 8 <= 65536 bytes;
 * cine_xpd_pack_bwd (64 t (n_primal + 1) + t) * 8 <= 65536 bytes, i.e. t (n_primal + 1) <= 127, half of what cine_xpd_pack accepts (the
 * largest tile is t = 9, n_primal = 13 at 64 584 bytes). */
int cine_xpd_unpack_bwd(const float* gout, float* gplanes_xf, float* gplanes_yf, float* gmean,
                        int b, int t, int h, int w, int n_primal, int n_scales, int xf, void* stream);
int cine_xpd_pack_bwd(const float* gplanes_xf, const float* gplanes_yf, const float* gmean, float* gbuf, float* gextra,
                      int b, int t, int h, int w, int n_primal, int n_scales, int xf, void* stream);

/* cine_image_dc is self-adjoint in the image (T = IFFT_h W FFT_h is Hermitian): its image gradient is cine_image_dc of the output
 * gradient (zf = NULL).  With respect to the maps it gives, per frame, part (b, t, c, h, w) = conj(g) T(S_c img) + T(S_c g) conj(img)
 * (varnet.py:181-194, 281-282); add the frames with cine_coil_accum(NULL, part, ...).  Weights as cine_image_dc. */
int cine_image_dc_sens_grad(const float* img, const float* gout, const float* sens, const uint8_t* mask,
                            const float* lambda_dev, float w_sampled, float w_unsampled,
                            float* part, int b, int t, int c, int h, int w, void* stream);
/* The same for a sampling mask that varies along w (cine_image_dc_general; mask uint8 (b, t, h, w)): part (b, t, c, h, w) =
 * conj(g) T(S_c img) + T(S_c g) conj(img) with T = IFFT2 [mask(ky, kx) ? w_sampled : w_unsampled] FFT2 (lambda_dev != NULL: the soft-DC
 * pair); add the frames with cine_coil_accum(NULL, part, ...).  The two operands take the three stages of cine_image_dc_general one after
 * the other through ONE workspace of cine_image_dc_general_sens_grad_ws_bytes() = b*t*c*h*w complex values (what cine_image_dc_general
 * needs: the callers share the buffer); the row IFFT of the first writes part, that of the second adds onto it.  h, w: any length
 * cine_fft_line_supported() accepts (CINE_EUNSUPPORTED otherwise); c <= 32768 (CINE_EINVAL), b*t <= 65535 (CINE_EUNSUPPORTED); part must not
 * alias img, gout, sens or ws (CINE_EINVAL); a short workspace is CINE_EWORKSPACE.  Every argument is checked before the first launch; no
 * allocation, no synchronisation, capturable. */
size_t cine_image_dc_general_sens_grad_ws_bytes(int b, int t, int c, int h, int w);
int cine_image_dc_general_sens_grad(const float* img, const float* gout, const float* sens, const uint8_t* mask,
                                    const float* lambda_dev, float w_sampled, float w_unsampled,
                                    float* part, int b, int t, int c, int h, int w,
                                    void* ws, size_t ws_bytes, void* stream);
/* Self-supervised k-space loss on held-out samples (SSDU, Yaman et al., MRM 2020; no reference counterpart: the reference trains against a
 * fully sampled target only).  img (b, t, h, w, 2), sens (b, c, h, w, 2), kspace (b, t, c, h, w, 2), mask uint8 (b, t, h, w): with
 * u = FFT2(S_c img) (sens_expand, varnet.py:181-185), r = mask (u - kspace), v = mask kspace,
 *     L = 1/2 ||r||_2 / ||v||_2 + 1/2 ||r||_1 / ||v||_1,
 * both norms over every real component of the batch (||.||_1 = sum |re| + |im|, sign(0) = 0).  cine_kspace_loss takes the first two stages of
 * cine_image_dc_general (S x -> row FFT -> ws, column FFT) and leaves, per column workgroup, four partial sums in ws (no atomics; the split
 * depends on the shape only); a one-workgroup kernel adds them in a fixed order in float64 and writes rec (8 floats, device):
 * sum r^2, sum |r|_1, sum kspace^2, sum |kspace|_1 (on the mask), L, a = 1 / (2 ||r||_2 ||v||_2) (0 where r = 0), b = 1 / (2 ||v||_1), 0.
 * Results are bit-identical from call to call; an empty mask gives the IEEE result of the expression (no host check).  kspace is used at
 * the mask's points only: what it holds elsewhere (NaN included) changes no output (off the mask the h == 200 kernels re-read one cached
 * element per image and discard it, the others read nothing).  cine_kspace_loss_grad recomputes both stages (nothing coil-wise is kept), forms g_k = *gloss mask (a r +
 * b sign(r)) with a, b read from rec, and continues as cine_image_dc_general: column IFFT, then gimg (b, t, h, w, 2) = sum_c conj(S_c)
 * IFFT_w(.) and / or gsens_part (b, t, c, h, w, 2) = IFFT2(g_k)_c conj(img), the maps' gradient per frame (add the frames with
 * cine_coil_accum(NULL, part, ...)); either output may be NULL, not both.  Workspace: cine_kspace_loss_ws_bytes() =
 * cine_image_dc_general_ws_bytes().  h, w: any length cine_fft_line_supported() accepts (CINE_EUNSUPPORTED otherwise, and for h == 1 with
 * w % 8 == 1, whose last column tile cannot hold its partial sums: the size function returns 0 there); c <= 32768 (CINE_EINVAL),
 * b*t <= 65535 (CINE_EUNSUPPORTED); rec, ws and the outputs must not alias an input or each other (CINE_EINVAL); a short workspace is
 * CINE_EWORKSPACE.  Every argument is checked before the first launch; no allocation, no synchronisation, capturable.
 * cine_diag_counter(32) counts the column-pass launches of both entry points. */
size_t cine_kspace_loss_ws_bytes(int b, int t, int c, int h, int w);
int cine_kspace_loss(const float* img, const float* sens, const float* kspace, const uint8_t* mask, float* rec,
                     int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);
int cine_kspace_loss_grad(const float* img, const float* sens, const float* kspace, const uint8_t* mask, const float* rec,
                          const float* gloss, float* gimg, float* gsens_part, int b, int t, int c, int h, int w,
                          void* ws, size_t ws_bytes, void* stream);
/* gs (b, c, h, w, 2) (+)= sum_t conj(g[b, t]) z[b, t, c]: gradient of sens_reduce's coil sum sum_c conj(S_c) z_c (varnet.py:187-194)
 * with respect to S; z (b, t, c, h, w, 2) are the coil images.  g == NULL: gs (+)= sum_t z.  accumulate == 0 overwrites gs. */
int cine_coil_accum(const float* g, const float* z, float* gs, int b, int t, int c, int h, int w, int accumulate, void* stream);
/* gx of y = x / rss(x, coil) (varnet.py:58-59) from gy and the UN-normalised x (b, c, h, w, 2). */
int cine_rss_normalise_bwd(const float* gy, const float* x, float* gx, int b, int c, int h, int w, void* stream);
/* gx (n, 2) of y = |x| (math.py:48-62). */
int cine_complex_abs_bwd(const float* gy, const float* x, float* gx, long n, void* stream);
/* out = a + sign * f(v) * b with v = softplus(*lambda_dev) (varnet.py:281-282): kind 0 f = v; 1 f = v / (1 + v); 2 f = 1 / (1 + v)^2;
 * 3 f = 1 / (1 + v).  a == NULL: out = sign * f(v) * b. */
int cine_axpby_lam(float* out, const float* a, const float* b, long n, const float* lambda_dev, int kind, float sign, void* stream);

/* SSIMLoss (utils/losses.py:25-58): loss = mean over frames of (1 - mean SSIM over the win x win windows of the valid region), sample
 * covariance, K1 / K2, the data range of every frame = the maximum of that TARGET frame (losses.py:34).  x = reconstruction, y = target,
 * both (t, h, w) float32; *loss_dev one float; win 2 .. 11 (a window of one pixel has no sample covariance: refused, and the size query
 * returns 0).  The forward keeps the per-window derivatives in `ws` (cine_ssim_loss_ws_bytes) for
 * cine_ssim_loss_bwd: gx (t, h, w) = d loss / d x scaled by the upstream gradient *gloss_dev.  Window sums in float64.
 * Workspace (8-byte aligned), with No = (h - win + 1) (w - win + 1) windows per frame in tiles of 16 x 16: t * tiles + 2 doubles (the tile
 * sums of S), then dS/d(ux), dS/d(uxx), dS/d(uxy) as three arrays of t * No doubles -- doubles because in a smooth window their weighted
 * sum cancels by three orders of magnitude --, then t + 16 floats (the frame maxima).  The backward reads the workspace only, and depends
 * on nothing but its bytes. */
size_t cine_ssim_loss_ws_bytes(int t, int h, int w, int win);
int cine_ssim_loss(const float* x, const float* y, int t, int h, int w, int win, double k1, double k2,
                   float* loss_dev, void* ws, size_t ws_bytes, void* stream);
int cine_ssim_loss_bwd(const float* x, const float* y, int t, int h, int w, int win, const float* gloss_dev,
                       const void* ws, size_t ws_bytes, float* gx, void* stream);

/* ------------------------------------------------------------------------------------------
 * k-t SPARSE-SENSE: FISTA with a temporal-sparsity penalty (no reference counterpart: a reconstruction that needs no trained
 * weights, the compressed-sensing baseline on the same operators)
 * ------------------------------------------------------------------------------------------ */
/* The second half of one proximal-gradient iteration, in one launch.  z, g, xprev, xnew, znew: (b, t, h, w, 2); g = A^H M A z - zf is the
 * data term's gradient (cine_image_dc with weights (1, 0, -1)).  With F_t the centered ortho transform along t (cine_fft1c variant 0: the
 * temporal DC bin is index t / 2) and soft(c, th) = c max(|c| - th, 0) / |c| (0 at c = 0):
 *     v = z - (*step_dev) g;   xnew = F_t^H soft(F_t v, (*step_dev) (*thresh_dev) w_f);   znew = xnew + beta (xnew - xprev)
 * w_f = 1, or with penalise_dc == 0, 0 at the DC bin.  step_dev, thresh_dev: one float each in device memory (nothing waits for the host).
 * rec != NULL: 4 device floats = sum |xnew - xprev|^2, sum |xnew|^2, sum_f w_f |F_t xnew|, 0 -- per-workgroup partial sums in ws
 * (cine_kt_prox_ws_bytes; ws may be NULL without rec), added in float64 in a fixed order by a second launch: the same bits on every call.
 * A workgroup owns all frames of cine_kt_prox_pixels() consecutive pixels and reads before it writes: znew may alias z and xnew may alias
 * xprev (z == xprev is fine too); any other aliasing of an output, and g == z or g == xprev, is CINE_EINVAL, as are null pointers and
 * non-positive sizes.  2 <= t <= 64 and b <= 65535, else CINE_EUNSUPPORTED; a short workspace is CINE_EWORKSPACE.  Every argument is
 * checked before the first launch; no allocation, no synchronisation, no atomics. */
int cine_kt_prox_pixels(void);
size_t cine_kt_prox_ws_bytes(int b, int t, int h, int w);
int cine_kt_prox(const float* z, const float* g, const float* xprev, const float* step_dev, const float* thresh_dev,
                 float beta, int penalise_dc, float* xnew, float* znew, float* rec,
                 int b, int t, int h, int w, void* ws, size_t ws_bytes, void* stream);
/* The whole solve in one call: x_0 = z_0 = zf, s_0 = 1, and for k = 0 .. iters - 1
 *     g = A^H M A z_k - zf   (cine_image_dc_t for a row mask, mask_w == 1: mask (b, t, h); cine_image_dc_general for mask_w == w: (b, t, h, w))
 *     (x_{k+1}, z_{k+1}) = cine_kt_prox(z_k, g, x_k, beta_k),   s_{k+1} = (1 + sqrt(1 + 4 s_k^2)) / 2,  beta_k = float((s_k - 1) / s_{k+1})
 * with the momentum computed on the host in double.  x (out), zf: (b, t, h, w, 2); sens (b, c, h, w, 2); sens_tiled: cine_sens_tile_pack's
 * copy or NULL (row masks, h == 200; same results).  rec: (iters, 4) device floats, one row of cine_kt_prox's record per iteration (all rows
 * are added up in one launch at the end), or NULL.  x and rec equal, bit for bit, what the caller gets from the two entry points iterated by
 * hand.  ws: cine_kt_fista_ws_bytes() = the operator's scratch, g, z and the partial sums.  iters >= 1, c > 0, mask_w in {1, w}, x / rec / ws
 * aliasing nothing (CINE_EINVAL); t and b as cine_kt_prox; h, w, c: what the operator accepts -- it is called first and refuses before
 * anything is launched. */
size_t cine_kt_fista_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int iters);
int cine_kt_fista(float* x, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask, int mask_w,
                  const float* step_dev, const float* thresh_dev, int iters, int penalise_dc, float* rec,
                  int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Low-rank plus sparse (L+S, Otazo et al. 2015; no reference counterpart): singular-value thresholding of the (h w) x t Casorati
 * matrix through its t x t Gram matrix, on the device
 *     minimise over L, S   1/2 || M A (L + S) - y ||^2 + lam_L || C(L) ||_* + lam_S || F_t S ||_1
 *     g = A^H M A (L_k + S_k) - zf;   L_{k+1} = SVT(L_k - step g, step lam_L);   S_{k+1} = F_t^H soft(F_t (S_k - step g), step lam_S)
 * With X = C(v) and G = X^H X = V diag(lam) V^H: SVT(X, th) = X W, W = V diag(h(lam)) V^H, h(lam) = 1 - th / sqrt(lam) for
 * lam > th^2, else 0.  Limits of all entry points: 2 <= t <= 64 and b <= 65535, else CINE_EUNSUPPORTED; null pointers and non-positive
 * sizes are CINE_EINVAL, a short workspace CINE_EWORKSPACE.  Every argument is checked before the first launch; no allocation, no
 * synchronisation, no atomics: capturable, and the same bits on every call.
 * ------------------------------------------------------------------------------------------ */
/* gram (b, t, t) complex128 (double pairs, row-major), gram[i][j] = sum over the h w pixels of conj(v_i) v_j with v = a - (*step_dev) g
 * formed in float32 and never written (g == NULL: v = a, step_dev may be NULL too); a, g: (b, t, h, w, 2).  Every product of two floats
 * is exact in float64, the sums run in float64 in an order that depends on the shape only (the scheme of cine_coil_gram): exactly
 * Hermitian with a real diagonal.  A workgroup stages cine_casorati_gram_pixels(t) pixels at a time and the number of workgroups that
 * leave a record in ws is capped (256 over the batch), so ws stays below 8.2 MiB at t = 64.  gram and ws: 16-byte aligned, aliasing
 * nothing (CINE_EINVAL). */
int cine_casorati_gram_pixels(int t);
size_t cine_casorati_gram_ws_bytes(int b, int t, int h, int w);
int cine_casorati_gram(const float* a, const float* g, const float* step_dev, double* gram, int b, int t, int h, int w,
                       void* ws, size_t ws_bytes, void* stream);
/* weight (b, t, t) complex64 = W of gram (b, t, t) complex128 for th = (*step_dev) (*thresh_dev) (step_dev == NULL: th = *thresh_dev).
 * One workgroup per batch element: the matrix and the eigenvector accumulator in LDS in float64, a cyclic Jacobi eigensolver for complex
 * Hermitian matrices with round-robin pairs, sweeping until max |off-diagonal| <= 1e-14 max |diagonal| or 40 sweeps (a NaN input ends at
 * the cap).  info (b, 4) doubles: sigma_max = sqrt(lam_max), the nuclear norm sum_i sqrt(lam_i) h(lam_i) of X W, the residual
 * max |off-diagonal| / max |diagonal| reached, the sweeps used.  W is exactly Hermitian; it is unique only off the null space of gram. */
int cine_svt_weight(const double* gram, const float* thresh_dev, const float* step_dev, float* weight, double* info, int b, int t,
                    void* stream);
/* The proximal half of an iteration in one launch.  l, s, g, lnew, snew, xsum: (b, t, h, w, 2); weight: cine_svt_weight's W of
 * cine_casorati_gram(l, g, step_dev).  Per pixel, with v_L = l - (*step_dev) g and v_S = s - (*step_dev) g:
 *     lnew[t'] = sum_t v_L[t] W[t][t'];   snew = F_t^H soft(F_t v_S, (*step_dev) (*thresh_s_dev));   xsum = lnew + snew
 * rec != NULL: 4 device floats = sum |xsum - (l + s)|^2, sum |xsum|^2, sum |F_t snew|, 0, from per-workgroup partial sums in ws
 * (cine_ls_prox_ws_bytes; ws may be NULL without rec) added in float64 in a fixed order by a second launch.  A workgroup owns all
 * frames of cine_ls_prox_pixels() consecutive pixels and reads before it writes: lnew may alias l and snew may alias s; any other
 * aliasing of an output is CINE_EINVAL. */
int cine_ls_prox_pixels(void);
size_t cine_ls_prox_ws_bytes(int b, int t, int h, int w);
int cine_ls_prox(const float* l, const float* s, const float* g, const float* weight, const float* step_dev,
                 const float* thresh_s_dev, float* lnew, float* snew, float* xsum, float* rec,
                 int b, int t, int h, int w, void* ws, size_t ws_bytes, void* stream);
/* The whole solve in one call: L_0 = zf, S_0 = 0, and for k = 0 .. iters - 1 the operator (cine_image_dc_t for mask_w == 1,
 * cine_image_dc_general for mask_w == w; sens_tiled as cine_kt_fista), cine_casorati_gram(L_k, g), cine_svt_weight with thresh_l_dev,
 * cine_ls_prox with thresh_s_dev.  x (out) = L + S; l_out, s_out: the components, or NULL; rec: (iters, 4) floats or NULL, a row of
 * cine_ls_prox's record per iteration with column 3 = the nuclear norm of L_{k+1} (info, added over the batch); resid: (iters) doubles or
 * NULL (only with rec), the worst Jacobi residual of each iteration.  x, l_out, s_out and rec equal, bit for bit, what the caller gets
 * from the entry points iterated by hand.  ws: cine_ls_solve_ws_bytes(), 16-byte aligned.  The operator is called first and refuses what
 * it does not accept (h, w, c) before anything is launched. */
size_t cine_ls_solve_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int iters);
int cine_ls_solve(float* x, float* l_out, float* s_out, const float* zf, const float* sens, const float* sens_tiled,
                  const uint8_t* mask, int mask_w, const float* step_dev, const float* thresh_l_dev, const float* thresh_s_dev,
                  int iters, float* rec, double* resid, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * spatio-temporal total variation (no reference counterpart: the third weight-free baseline, on the same operators)
 *     minimise  1/2 || M A x - y ||^2  +  lam_t || D_t x ||_1  +  lam_s sum_pixels sqrt(|D_h x|^2 + |D_w x|^2)
 * D_t: x[t + 1] - x[t], wrapping from the last frame to the first with periodic != 0, 0 at the last frame otherwise; D_h, D_w: forward
 * differences, 0 at the last row / column.  The dual variable p = (p_t, p_h, p_w) is (3, b, t, h, w, 2).
 * ------------------------------------------------------------------------------------------ */
/* One Condat-Vu primal-dual iteration after the data term's gradient g = A^H M A x - zf, in one launch:
 *     xnew = x - tau (g + D^H p);   pnew = P(p + sigma D (2 xnew - x))
 *     P: p_t <- p_t / max(1, |p_t| / lam_t);   (p_h, p_w) <- (p_h, p_w) / max(1, sqrt(|p_h|^2 + |p_w|^2) / lam_s)
 * with D^H the exact adjoint of D.  x, g, xnew: (b, t, h, w, 2); p, pnew: (3, b, t, h, w, 2); tau_dev, sigma_dev, lam_t_dev, lam_s_dev:
 * one float each in device memory (nothing waits for the host).  terms: 1 = temporal, 2 = spatial, 3 = both; the planes of p and pnew
 * of a term that is off are neither read nor written, and its lam pointer may be NULL.
 * rec != NULL: 4 device floats = sum |xnew - x|^2, sum |xnew|^2, sum |D_t xnew|, sum sqrt(|D_h xnew|^2 + |D_w xnew|^2) (the sum of a
 * term that is off is 0) -- per-workgroup partial sums over the pixels a workgroup owns in ws (cine_tv_pd_ws_bytes; ws may be NULL
 * without rec), added in float64 in a fixed order by a second launch: the same bits on every call.
 * A workgroup owns a tile of cine_tv_pd_tile() pixels and recomputes xnew on a one-pixel halo from x, g and p across the seams, so
 * nothing is in place: xnew and pnew aliasing an operand or each other is CINE_EINVAL, as are null pointers, non-positive sizes and
 * terms outside 1 .. 3.  2 <= t <= 64 and b <= 65535, else CINE_EUNSUPPORTED; any h, w >= 1; a short workspace is CINE_EWORKSPACE.
 * Every argument is checked before the first launch; no allocation, no synchronisation, no atomics. */
int cine_tv_pd_tile(int* th, int* tw);
size_t cine_tv_pd_ws_bytes(int b, int t, int h, int w);
int cine_tv_pd_step(const float* x, const float* g, const float* p, const float* tau_dev, const float* sigma_dev,
                    const float* lam_t_dev, const float* lam_s_dev, int terms, int periodic, float* xnew, float* pnew, float* rec,
                    int b, int t, int h, int w, void* ws, size_t ws_bytes, void* stream);
/* The whole solve in one call: x_0 = zf, p_0 = 0, and for k = 0 .. iters - 1 the operator (cine_image_dc_t for mask_w == 1: mask
 * (b, t, h); cine_image_dc_general for mask_w == w: (b, t, h, w); sens_tiled as cine_kt_fista) and cine_tv_pd_step.  x (out), zf:
 * (b, t, h, w, 2).  The iterates alternate between x and the workspace, the duals between two sets of planes in the workspace that hold
 * only the planes of the terms that are on.  rec: (iters, 4) device floats, one row of cine_tv_pd_step's record per iteration (all
 * rows are added up in one launch at the end), or NULL.  p_out: the final dual (3, b, t, h, w, 2) with zeros in the planes of a term
 * that is off, or NULL.  x, rec and p_out equal, bit for bit, what the caller gets from the two entry points iterated by hand.
 * ws: cine_tv_solve_ws_bytes() = the operator's scratch, g, one image, two sets of three planes and the partial sums.  iters >= 1,
 * c > 0, mask_w in {1, w}, terms in 1 .. 3, x / rec / p_out / ws aliasing nothing (CINE_EINVAL); t and b as cine_tv_pd_step; h, w, c:
 * what the operator accepts -- it is called first and refuses before anything is launched. */
size_t cine_tv_solve_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int iters);
int cine_tv_solve(float* x, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask, int mask_w,
                  const float* tau_dev, const float* sigma_dev, const float* lam_t_dev, const float* lam_s_dev, int terms, int periodic,
                  int iters, float* rec, float* p_out, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Locally low-rank (LLR; Trzasko & Manduca 2011, Zhang et al. 2015; no reference counterpart): singular-value thresholding of every
 * small spatial block of the Casorati matrix, the fourth weight-free baseline, on the same operators
 *     minimise over x   1/2 || M A x - y ||^2  +  lam sum over the blocks beta of a partition P of || C_beta(x) ||_*
 * C_beta(x): the (pixels of beta) x t Casorati matrix of block beta.  P: block x block squares on a grid whose origin lies at
 * (-shift_h, -shift_w), 0 <= shift < block, clipped to the image (no wrap-around): ceil((h + shift_h) / block) x
 * ceil((w + shift_w) / block) blocks per image, the ones at the border as small as one pixel.  Proximal gradient without momentum,
 *     g = A^H M A x_k - zf;   x_{k+1} = BlockSVT_{P_k}(x_k - step g, step lam)
 * with the shift of P_k changing from iteration to iteration.  Per block, with X = C_beta(v) and G = X^H X = V diag(lam) V^H (t x t):
 * SVT(X, th) = X W, W = V diag(h(lam)) V^H, h(lam) = 1 - th / sqrt(lam) for lam > th^2, else 0 -- the route of cine_svt_weight, here
 * with one workgroup per (block, batch element) that forms G, diagonalises it and applies W in ONE launch.
 * Limits of both entry points: 2 <= t <= 64, 2 <= block <= 16 (any value, no power of two needed), b <= 65535, else
 * CINE_EUNSUPPORTED; any h, w >= 1 (the solve: what the operator accepts).  Null x, non-positive sizes and a shift outside [0, block)
 * are CINE_EINVAL, a short workspace CINE_EWORKSPACE.  Every argument is checked before the first launch; no allocation, no
 * synchronisation, no atomics: capturable, and the same bits on every call.
 * ------------------------------------------------------------------------------------------ */
/* The proximal half of an iteration in one launch.  x, g, xnew: (b, t, h, w, 2).  v = x - (*step_dev) g is formed in float32 and never
 * written; g == NULL: v = x, and step_dev may be NULL too.  th = (*step_dev) (*thresh_dev), or *thresh_dev with step_dev == NULL.
 * Per block: G in float64 from exact float32 products in an order that depends on the shape only (bitwise Hermitian, a real diagonal),
 * the cyclic Jacobi eigensolver of cine_svt_weight in LDS (until max |off-diagonal| <= 1e-14 max |diagonal| or 40 sweeps; a NaN ends at
 * the cap), W, and xnew = v W per pixel.
 * xnew == NULL: nothing is written to an image, only rec and info are produced (the scale of lam is formed this way).  xnew may be x
 * (a workgroup owns its block over all frames and reads before it writes); any other aliasing of an output is CINE_EINVAL.
 * rec (or NULL): 4 device floats = sum |xnew - x|^2, sum |xnew|^2, sum over the blocks of || C_beta(xnew) ||_* (the thresholded singular
 * values), 0.  info (or NULL): 4 device doubles over the whole call = the largest block sigma_max of v, the worst Jacobi residual
 * max |off-diagonal| / max |diagonal| any block reached, the most sweeps any block used, the number of blocks (b times the blocks per
 * image).  Both come from one record per workgroup in ws (cine_llr_prox_ws_bytes for exactly this shift; 16-byte aligned; ws may be
 * NULL without rec and info), added in float64 in a fixed order by a second launch. */
size_t cine_llr_prox_ws_bytes(int b, int t, int h, int w, int block, int shift_h, int shift_w);
int cine_llr_prox(const float* x, const float* g, const float* step_dev, const float* thresh_dev, int block, int shift_h, int shift_w,
                  float* xnew, float* rec, double* info, int b, int t, int h, int w, void* ws, size_t ws_bytes, void* stream);
/* The whole solve in one call: x_0 = zf, and for k = 0 .. iters - 1 the operator (cine_image_dc_t for mask_w == 1: mask (b, t, h);
 * cine_image_dc_general for mask_w == w: (b, t, h, w); sens_tiled as cine_kt_fista) with weights (1, 0, -1) and cine_llr_prox in place
 * with the shift (shifts[2 k], shifts[2 k + 1]).  shifts: a HOST array of iters x 2 ints read during the call and checked in full
 * before the first launch, or NULL for no shift.  x (out), zf: (b, t, h, w, 2).  rec: (iters, 4) floats, info: (iters, 4) doubles, a
 * row of cine_llr_prox's per iteration, or NULL (all rows are added up in one launch at the end).  x, rec and info equal, bit for bit,
 * what the caller gets from the two entry points iterated by hand.  ws: cine_llr_solve_ws_bytes() = the operator's scratch, g and
 * iters rows of records sized for the WORST CASE over all shifts (ceil((h + block - 1) / block) x ceil((w + block - 1) / block)
 * blocks per image), whatever shifts the call is given; 16-byte aligned.  iters >= 1, c > 0, mask_w in {1, w}, x / rec / info / ws
 * aliasing nothing (CINE_EINVAL); h, w, c: what the operator accepts -- it is called first and refuses before anything is launched. */
size_t cine_llr_solve_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int block, int iters);
int cine_llr_solve(float* x, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask, int mask_w,
                   const float* step_dev, const float* thresh_dev, int block, const int* shifts, int iters,
                   float* rec, double* info, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * noise propagation by pseudo multiple replicas (no reference counterpart; Robson et al., MRM 60:895-907, 2008: add synthetic noise
 * of the scanner's covariance to the measured k-space, reconstruct N times, take the per-pixel standard deviation).
 *
 * The noise source is Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), and its definition is part of this interface -- the tests
 * restate it independently (tests/noise_reference.py); csrc/philox.h is its one implementation, for the device and the host.
 *
 *   multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57
 *   Weyl increments W0 = 0x9E3779B9, W1 = 0xBB67AE85
 *
 *   (c0,c1,c2,c3) -> (hi(M1*c2)^c1^k0, lo(M1*c2), hi(M0*c0)^c3^k1, lo(M0*c0))
 *   (k0,k1) += (W0,W1) after every round                                          ten rounds
 *
 *   key     = (seed & 0xffffffff, seed >> 32)                                     the 64 bits of the long, the shift logical
 *   counter = (p & 0xffffffff, p >> 32, replica, j)
 *   p = point0 + ((bt * h + y) * w + x)      // 64-bit index of the k-space point
 *   j = coil pair index
 *
 * One call yields x0..x3.  Coil 2j uses (x0, x1) and coil 2j+1 uses (x2, x3).  An odd last coil discards the second half.
 * From words to a complex normal with E|z|^2 = 1, for the words (a, b) of one coil:
 *
 *   u1 = ((a >> 9) + 0.5f) * 2^-23     // in [2^-24, 1 - 2^-24], every step exact in float32
 *   u2 = (b >> 8) * 2^-24              // in [0, 1), exact
 *   z  = sqrtf(-logf(u1)) * (cospif(2 u2) + i sinpif(2 u2))
 *
 * with logf, sqrtf and sincospif, not their fast forms.  Correlated noise: eta_i = scale * sum_{k <= i} L[i,k] z_k, ascending k, an
 * fmaf chain from 0 (per term: re = fmaf(L.re, z.re, re), re = fmaf(-L.im, z.im, re), im = fmaf(L.re, z.im, im), im = fmaf(L.im, z.re,
 * im)); L is lower-triangular complex64 with Psi = L L^H, Psi as frontend.noise_covariance defines it (Psi[i, j] = E eta_i conj(eta_j)).
 * A value depends only on (seed, replica, p, coil), never on grid, tile or launch shape.
 * ------------------------------------------------------------------------------------------ */
/* out = kspace + eta at the sampled points, out = kspace at the others.  kspace, out: (bt, c, h, w, 2); out == kspace is allowed (in
 * place: nothing is read or written at a point that is not sampled), any other overlap of the two is CINE_EINVAL.  mask: uint8 (bt, h)
 * for mask_w == 1 or (bt, h, w) for mask_w == w, the convention of cine_kt_fista; NULL: every point (mask_w is still checked: pass 1).
 * chol: (c, c) complex64 pairs, the lower triangle read, the diagonal as stored; NULL: white noise, eta = scale * z.  replica in
 * [0, 2^32); replica_dev, if non-NULL, is a device long the kernel reads in its place, so that a captured graph draws fresh noise on
 * every replay once the caller bumps the counter.  point0 >= 0 places the call's first point on the 64-bit point axis: a stack of
 * frames equals its frames noised one by one with point0 advanced by h * w each.  At most 64 coils (CINE_EUNSUPPORTED).
 * CINE_EINVAL: null kspace / out, non-positive sizes, mask_w outside {1, w}, replica outside its range, a negative point0, a pointer
 * off its 8-byte alignment.  Every argument is checked before the launch; no allocation, no host read, no atomics: capturable, and
 * the same bits on every call. */
int cine_noise_add(const float* kspace, float* out, const uint8_t* mask, int mask_w, const float* chol, float scale,
                   long seed, long replica, const long* replica_dev, long point0, long bt, int c, int h, int w, void* stream);
/* The same noise on RAW data, in front of the front-end: raw, out (t, nx, ny, c, 2) with the coil index fastest, the layout
 * cine_raw_ingest and cine_coil_compress read.  The k-space point of a sample is p = point0 + (frame * nx + x) * ny + y, and the value
 * added to coil i of it is the eta_i defined above for (seed, replica, p, i): permute any input to (t, c, h = nx, w = ny), call
 * cine_noise_add with the same (seed, replica, point0, chol, scale, mask), permute back, and the bits are these.  mask: uint8 (t, nx)
 * for mask_ny == 1 (the acquired lines) or (t, nx, ny) for mask_ny == ny; NULL: every sample (mask_ny is still checked: pass 1).
 * out == raw works in place and neither reads nor writes a sample that is not sampled; out of place those are copied bit for bit; any
 * other overlap is CINE_EINVAL.  chol, replica, replica_dev, point0: as for cine_noise_add.  A workgroup owns 64 consecutive points,
 * whose 64 * c values are one contiguous span of raw, and walks it with consecutive lanes on consecutive 8-byte elements.
 * CINE_EINVAL: null raw / out, non-positive sizes, mask_ny outside {1, ny}, replica outside [0, 2^32), a negative point0, a pointer
 * off its 8-byte alignment.  CINE_EUNSUPPORTED: more than 64 coils, more than 64 * (2^31 - 1) points.  Every argument is checked
 * before the launch; no allocation, no host read, no atomics: capturable, and the same bits on every call. */
int cine_noise_add_raw(const float* raw, float* out, const uint8_t* mask, int mask_ny, const float* chol, float scale,
                       long seed, long replica, const long* replica_dev, long point0, long t, int nx, int ny, int c, void* stream);
/* Retrospective gating: the acquired readouts of a scan, sorted and averaged / interpolated into the raw (t, x, y, coil) array.
 * lines (n_lines, row_elems, 2): the readouts in acquisition order, row_elems = ny * coil complex samples each, coil fastest.
 * out (rows, row_elems, 2), rows = n_frames * nx: the layout cine_raw_ingest, cine_coil_gram, cine_coil_compress and
 * cine_noise_add_raw read.  row_ptr (rows + 1 ints), index, weight: a CSR matrix in device memory, and
 *   out[r] = sum_j weight[j] * lines[index[j]],  j = row_ptr[r] .. row_ptr[r + 1] - 1, in that order:
 * the first term is one fp32 product, every further term one fmaf per real component, so a row with the single weight 1.0 is its
 * line bit for bit (finite data).  A row without entries is written as zeros: EVERY element of out is written by the call, no memset
 * is needed and what out held does not matter.  A workgroup owns a chunk of one output row, reads the row's CSR entries once
 * (uniform loads), streams the contributing spans with consecutive lanes on consecutive 16-byte accesses (8-byte ones when
 * row_elems is odd or lines / out sit off a 16-byte boundary), accumulates in registers and stores once.
 * The CSR arrays are DEVICE data and the call trusts them: row_ptr non-decreasing from row_ptr[0] >= 0, 0 <= index[j] < n_lines.
 * cine_hip.gating.GatingPlan validates them on the host when it is built; n_lines serves the overlap check only.
 * CINE_EINVAL: a null pointer, rows <= 0, row_elems <= 0, n_lines < 0, sizes whose byte count overflows, out overlapping lines,
 * lines / out off their 8-byte alignment, row_ptr / index / weight off their 4-byte alignment.  CINE_EUNSUPPORTED: more than
 * 2^31 - 1 workgroups (rows * ceil(accesses of a row / 512)), the grid limit.  Every argument is checked before the launch; no
 * allocation, no host read, no atomics: capturable, and the same bits on every call. */
int cine_gate_readouts(const float* lines, float* out, const int* row_ptr, const int* index, const float* weight,
                       long n_lines, long rows, long row_elems, void* stream);
/* Training augmentation (cine_hip.augment; no reference counterpart): in resampled under one inverse affine map, with a cyclic shift /
 * reversal of the frames.  in, out (frames, inner, h, w, 2) float32 complex pairs, out of place only; inner is the coil axis (or 1).
 * Output frame f reads source frame g = (f + t_shift) mod frames, or with t_reverse != 0 g = (t_shift - f) mod frames (the mathematical
 * mod).  Every plane shares the map: for the output pixel (yo, xo), centred on the image centre cy = (h - 1) / 2, cx = (w - 1) / 2,
 *   ys = a_yy (yo - cy) + a_yx (xo - cx) + b_y + cy,   xs = a_xy (yo - cy) + a_xx (xo - cx) + b_x + cx
 * in float64 (as fma(a_yy, yo - cy, fma(a_yx, xo - cx, b_y + cy)): exact for flips, quarter turns and integer shifts), i0 = floor(.),
 * and the fraction rounded to float32 once.  Float32 weights: mode 0 bilinear, (1 - f, f) on the taps i0, i0 + 1; mode 1 bicubic, the
 * cubic-convolution kernel with A = -0.75 on the taps i0 - 1 .. i0 + 2, in the Horner forms ((A + 2) x - (A + 3)) x^2 + 1 on [0, 1] and
 * ((A x - 5 A) x + 8 A) x - 4 A on [1, 2], which are exactly 1 and 0 at integer fractions.  border 0: a tap outside the plane counts as
 * 0 and is not read; border 1: every tap index is reflected half-sample symmetrically with period 2 n (.., 1, 0 | 0, 1, .., n - 1 |
 * n - 1, n - 2, ..), as often as it takes.  This is torch.nn.functional.grid_sample(align_corners=False, padding_mode "zeros" /
 * "reflection") behind affine_grid([[a_xx, a_xy h / w, 2 b_x / w], [a_yx w / h, a_yy, 2 b_y / h]]).
 * The sum: per tap row, ascending, s_r = the fmaf chain from 0 of wx[k] v[r][k] over the tap columns, ascending; the pixel is the fmaf
 * chain from 0 of wy[r] s_r; real and imaginary parts apart.  The same bits on every call and from every launch shape; with integral
 * coordinates the pixel is its tap bit for bit (finite data).  A lane computes coordinates, taps and weights once and walks the inner
 * planes with them.
 * CINE_EINVAL: a null pointer, a size below 1, mode / border outside {0, 1}, a matrix entry or offset that is not finite, |a| > 1024,
 * |b| > 2^20 (within these limits every coordinate fits an int with room), t_shift outside [0, frames), in / out off their 8-byte
 * alignment, sizes whose byte count overflows, in and out overlapping.  CINE_EUNSUPPORTED: h or w above 4096, more than 2^31 - 1
 * workgroups (frames * ceil(inner / 4) * ceil(h / 8) * ceil(w / 32); bicubic: inner / 2).  Every argument is checked on the host before the launch; no allocation, no host
 * read, no atomics: capturable. */
int cine_affine_warp(const float* in, float* out, int frames, int inner, int h, int w,
                     double a_yy, double a_yx, double b_y, double a_xy, double a_xx, double b_x,
                     int mode, int border, int t_shift, int t_reverse, void* stream);
/* GRAPPA / TGRAPPA (cine_hip.grappa; no reference counterpart): k-space kernels fitted on a calibration array and applied coil by coil to
 * the rows a frame did not acquire.  k-space of a slice is (t, c, h, w) complex64, h the phase-encode axis; the mask is (t, h) bytes.
 * Acceleration 2 <= R <= 8; the kernel is ky x kx, ky in {2, 4} source rows R apart, kx in {3, 5, 7} columns, hx = kx / 2;
 * ns = ky kx c sources in the order (j, dx, coil), j the source row, dx the column tap, the coil fastest; span = (ky - 1) R + 1,
 * base = (ky / 2 - 1) R.  Limits: c <= 32 and n_aug = ns + (R - 1) c <= 1152 (else CINE_EUNSUPPORTED); R, ky, kx outside their sets:
 * CINE_EINVAL.
 * Lattice offset of a frame: the lowest r in [0, R) such that the rows r, r + R, ... are all acquired; none: offset -1, status 1.  A
 * fully sampled frame has offset 0 and nothing to fill.  Every row of a frame that is not acquired is a target of type
 * m = (y - off) mod R in [1, R); its source rows are y - m - base + j R, j < ky; source samples outside [0, h) x [0, w) are zero.
 * Acquired rows (ACS rows and stray extra rows among them) are never written.
 *   out[f, q, y, x] = sum_{j, dx, k} W[m - 1][(j, dx, k)][q] in[f, k, row_j, x + dx - hx]
 * Calibration: from cal (c, hc, w) every window position y in [0, hc - span], x in [hx, w - hx) gives one row of the augmented patch
 * matrix P = [sources | targets of types 1 .. R - 1], the target of type m being cal[:, y + base + m, x].  G = P^H P (n_aug x n_aug);
 * G_ss = G[:ns, :ns], G_st = G[:ns, ns:], tau = lam trace(G_ss) / ns, and (G_ss + tau I) W = G_st.
 *
 * cine_grappa_offsets: mask (t, h) -> offsets (t) and status (t) int32 by the rule above, one workgroup per frame.
 * cine_grappa_gram: G in complex128, row-major.  Products of floats are exact in float64 and the sums run in float64 in an order fixed by the
 * shape (eight threads per entry add every eighth window row in window order, their sums are added in that order), so
 * G is exactly Hermitian with a real diagonal and the same on every call.  hc < span or w < kx: CINE_EINVAL; gram and ws 16-byte
 * aligned, cal 8-byte aligned (else CINE_EINVAL); ws_bytes >= cine_grappa_gram_ws_bytes() (0 for shapes it refuses), else
 * CINE_EWORKSPACE; more than 2^22 calibration positions hc w: CINE_EUNSUPPORTED.
 * cine_grappa_weights: weights (R - 1, ns, c) complex64, each entry rounded once from the float64 solution; info, 4 doubles: the relative
 * residual |(G_ss + tau I) W - G_st|_F / |G_st|_F of the float64 solution (0 when G_st = 0), tau, the calibration fit
 * sqrt(trace(G_tt - W^H G_st) / trace(G_tt)) clamped at 0 (0 when trace(G_tt) = 0), trace(G_ss).  The solve is a Newton-Schulz inverse
 * X <- X (2 I - A X) of A = G_ss + tau I from X_0 = I / |A|_F on cine_zgemm_f64, ceil(log2(sqrt(ns) (ns / lam + 1))) + 6 steps (at most
 * 100; A's condition number is at most ns / lam + 1), W = X G_st and one step of iterative refinement; the launch sequence depends on
 * (ns, lam) only.  trace(G_ss) = 0 (an all-zero calibration array): the weights are exactly zero, the residual 0.  A NaN in the Gram
 * matrix gives a NaN residual.  lam must be positive and finite, gram and ws 16-byte aligned, weights and info 8-byte aligned (else
 * CINE_EINVAL); ws_bytes >= cine_grappa_weights_ws_bytes() (0 for shapes it refuses), else CINE_EWORKSPACE.
 * cine_grappa_apply: the application above.  A workgroup owns 64 x-points of one lattice gap of one frame and computes all R - 1 target
 * rows of the gap from the ky source rows, staged once in LDS; a skinny complex GEMM (M the x-points, K = ns, N = (R - 1) c) in exact
 * fp32 on v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain per output with the accumulators of cine_coil_compress (Cr += Ar Br - Ai Bi,
 * Ci += Ar Bi + Ai Br), the weights staged in chunks of 64 k-values.  Targets that are acquired are skipped; frames whose offset is
 * outside [0, R) are left alone.  out == in works in place (sources are acquired rows and targets are not) and gives the bits of the
 * out-of-place call; with out != in the acquired rows, and every row of a frame that is left alone, are copied bit for bit; any other
 * overlap is CINE_EINVAL.  in, out, weights 8-byte aligned, offsets 4-byte aligned (else CINE_EINVAL); more than 65535 frames or
 * lattice gaps, more than 2^31 - 1 rows t c h: CINE_EUNSUPPORTED.
 * Every entry checks every argument before the first launch; no allocation, no host read, no synchronisation, no atomics: capturable,
 * and the same bits on every call. */
int cine_grappa_offsets(const uint8_t* mask, int* offsets, int* status, int t, int h, int R, void* stream);
size_t cine_grappa_gram_ws_bytes(int c, int hc, int w, int R, int ky, int kx);
int cine_grappa_gram(const float* cal, double* gram, void* ws, size_t ws_bytes, int c, int hc, int w, int R, int ky, int kx, void* stream);
size_t cine_grappa_weights_ws_bytes(int c, int R, int ky, int kx);
int cine_grappa_weights(const double* gram, float* weights, double* info, void* ws, size_t ws_bytes, int c, int R, int ky, int kx,
                        double lam, void* stream);
int cine_grappa_apply(const float* in, const float* weights, const uint8_t* mask, const int* offsets, float* out, int t, int c, int h,
                      int w, int R, int ky, int kx, void* stream);
/* GRAPPA on unevenly spaced rows (a frame that is no lattice, e.g. the reference's equispaced masks with their rounded non-integer
 * step): a frame is a list of gaps, and a gap of step G is filled with the lattice weights of R = G.  Only ky = 2: the sources of a
 * missing row are its two acquired neighbours.
 * The rule, per frame, with a_0 < ... < a_{n-1} the acquired rows, max_gap <= 8 and `allowed` the set of steps that have weights:
 *   interior gap   consecutive acquired rows G = a_{i+1} - a_i >= 2 apart: the gap (lo = a_i, G); targets lo + m, m = 1 .. G - 1, of
 *                  type m; sources lo and lo + G.
 *   leading end    the rows [0, a_0), e > 0 of them: G = max(nb, e + 1), nb = a_1 - a_0 if n >= 2 and that spacing is >= 2, else 0;
 *                  the gap (a_0 - G, G).  Its lower source row is outside the frame and reads as zero; targets below row 0 are skipped.
 *   trailing end   the mirror image: nb = a_{n-1} - a_{n-2}, the gap (a_{n-1}, G), the upper source row outside the frame.
 *   unfilled       a gap or end with G > max_gap or G not in `allowed` is not listed; its rows stay as they are and are counted in
 *                  unfilled[f].  A frame with n = 0 is left alone: count 0, unfilled = h.
 *   order          ascending lo, the leading end first.
 *   out[f, q, lo + m, x] = sum_{j, dx, k} W_G[m - 1][(j, dx, k)][q] in[f, k, lo + j G, x + dx - hx]
 * with W_G the weights of cine_grappa_weights(R = G, ky = 2, kx), source samples outside [0, h) x [0, w) zero, acquired rows never
 * written.  A frame that is a lattice of step R, 2 <= R <= 8, has every gap, both ends included, of step R, and the gap path then
 * gives the bits of cine_grappa_apply; next to an ACS block or a stray extra row the two differ by design: the gap path predicts from
 * the nearer rows.
 *
 * cine_grappa_gaps_cap: the entries per frame of a gap table of h rows, h / 2 + 1 (a gap owns a run of missing rows); 0 for h < 1.
 * cine_grappa_gaps: mask (t, h) -> gaps (t, cap, 2) int32 pairs (lo, G), cap = cine_grappa_gaps_cap(h), count (t) and unfilled (t)
 * int32.  allowed_bits: bit G set for every step G in `allowed` (bits outside 2 .. 8: CINE_EINVAL).  One workgroup per frame; each
 * acquired row finds its neighbours within max_gap rows, and the entries are placed by an LDS prefix sum over the rows in row order:
 * no atomics, the same table on every call; entries at and beyond count[f] are (0, 0).  max_gap outside 2 .. 8, null or aliased
 * pointers, outputs off their 4-byte alignment: CINE_EINVAL; h above 2^20: CINE_EUNSUPPORTED.
 * cine_grappa_apply_gaps: the application above.  weights: one buffer that holds the (G - 1, ns, c) complex64 blocks of the steps with
 * weights, each as cine_grappa_weights wrote it; woff: 9 ints on the host, woff[G] the offset of the block of step G in complex
 * elements or -1 (woff[0], woff[1] are not read; a value below -1, or no step with weights: CINE_EINVAL).  The workgroup is that of
 * cine_grappa_apply: 64 x-points of one table entry of one frame, the two source rows staged once, all G - 1 target rows on
 * v_mfma_f32_16x16x4_f32 with the same k-ordered chain per output; N = (G - 1) c, the tile grouping, the skip tables and the LDS
 * layout follow the entry, the LDS is sized for the largest step with weights.  A workgroup whose entry index is >= count[f] ends
 * before it stages anything; an entry whose step has no weights, or that lies outside the frame, is left alone.  out == in works in
 * place and gives the bits of the out-of-place call; with out != in every row that is not written (acquired rows, unfilled rows, empty
 * frames) is copied bit for bit first; any other overlap is CINE_EINVAL.  Limits and alignment as cine_grappa_apply: c <= 32 and
 * ns + (G_max - 1) c <= 1152 for the largest step with weights (else CINE_EUNSUPPORTED), in, out, weights 8-byte aligned, gaps and
 * count 4-byte aligned, kx outside {3, 5, 7}: CINE_EINVAL; more than 65535 frames or table entries per frame, more than 2^31 - 1 rows:
 * CINE_EUNSUPPORTED.  Both entries check every argument before the first launch; no allocation, no host read, no synchronisation, no
 * atomics: capturable. */
int cine_grappa_gaps_cap(int h);
int cine_grappa_gaps(const uint8_t* mask, int* gaps, int* count, int* unfilled, int t, int h, int max_gap, int allowed_bits,
                     void* stream);
int cine_grappa_apply_gaps(const float* in, const float* weights, const int* woff, const uint8_t* mask, const int* gaps,
                           const int* count, float* out, int t, int c, int h, int w, int cap, int kx, void* stream);
/* The analytic noise map of the lattice reconstruction (Breuer et al., MRM 62:739, 2009).  On a zero-filled lattice z of ANY offset
 * cine_grappa_apply is one convolution, out[q, y, x] = sum K[q, k, dy, dx] z[k, y + dy, x + dx], with the combined kernel
 *   K[., ., 0, 0] = I;   K[q, k, -m - base + j R, dx - hx] = W[m - 1][(j, dx, k)][q],   m = 1 .. R - 1, j < ky, dx < kx
 * (1 + (R - 1) ky distinct row offsets, kx column offsets; W as cine_grappa_weights writes it).  With the package's centred orthonormal
 * transform, rho_y = y - h / 2, rho_x = x - w / 2 (integer division), the image-domain weights are, without any scale factor,
 *   Wimg[q, k](y, x) = sum_{dy, dx} K[q, k, dy, dx] exp(-2 pi i (dy rho_y / h + dx rho_x / w))
 * and ifft2c(K applied circularly to z)[q] = sum_k Wimg[q, k] ifft2c(z)[k].  With noise of covariance scale^2 Psi, Psi = L L^H, on
 * every acquired sample (cine_noise_add), a linear combination sum_q p_q(y, x) x_q of the coil images has
 *   amp^2 = p Wimg Psi Wimg^H p^H = sum_j |sum_{q, k} p_q Wimg[q, k] L[k, j]|^2,     std = scale sqrt(amp^2 / R)
 * (std of the complex pixel, var_re + var_im: cine_replica_finish with pairs) and the g-factor std_accel / (std_full sqrt(R)) is
 *   g = sqrt(amp^2 / (p Psi p^H)) / R,   0 where p Psi p^H is not positive;      per coil, p = e_q: g_q = sqrt((Wimg Psi Wimg^H)_qq / Psi_qq) / R.
 * What the closed form leaves out: the application treats rows and columns outside the frame as zero where the formula wraps around;
 * ACS rows and stray extra rows are kept as acquired where the formula knows the lattice only; and h need not be a multiple of R.
 *
 * cine_grappa_image_weights: weights (R - 1, ns, c) complex64 -> out (c, c, h, w) complex64, out[q][k][y][x] = Wimg[q, k](y, x).
 * cine_grappa_gfactor: the fused form, Wimg is never written to memory.  chol: L (c, c) complex64, row-major, of which the lower
 * triangle is read (noise_cholesky's), or NULL for Psi = I.  coef: p (n, c, h, w) complex64, or NULL for the c unit vectors (n is then
 * not used but must still be >= 1).  g and amp = sqrt(amp^2): float32 (n, h, w) with coef, (c, h, w) without; either may be NULL,
 * not both.
 * A workgroup of 256 lanes owns 256 pixels of one row y: it contracts the row offsets with their phases into B[dx][q][k] in LDS (kx c^2
 * complex, (R - 1) ky terms each, (m, j) ascending, on top of the identity tap), multiplies every row B[dx][q][:] by L in place, and each
 * lane then forms sum_dx B[dx][q][j] e_x(dx) for its pixel, dx ascending, and sums over q (ascending, with coef) and the squares over j
 * (ascending) in fp32 fmaf chains.  A phase factor is sincospif(-2 r / n) of the exactly reduced integer r = d rho mod n folded into
 * (-n / 2, n / 2].  No atomics, a fixed order: the same bits on every call.  LDS: ((kx + 1) c (c + 1) + (R - 1) ky + c) 8 bytes, 68 KB
 * at the limits.
 * Limits as cine_grappa_apply: 2 <= R <= 8, ky in {2, 4}, kx in {3, 5, 7} (else CINE_EINVAL); c <= 32, ns + (R - 1) c <= 1152, h and w
 * at most 2^20 (else CINE_EUNSUPPORTED).  A null weights / out, g and amp both null, sizes below 1, weights, chol, coef or out off
 * their 8-byte alignment, g or amp off their 4-byte alignment, an output that overlaps an input or the other output: CINE_EINVAL.
 * Every argument is checked before the launch; one launch, no allocation, no host read, no synchronisation: capturable. */
int cine_grappa_image_weights(const float* weights, float* out, int c, int h, int w, int R, int ky, int kx, void* stream);
int cine_grappa_gfactor(const float* weights, const float* chol, const float* coef, float* g, float* amp, int n, int c, int h, int w,
                        int R, int ky, int kx, void* stream);
/* Welford's update of (mean, m2) with the k-th sample x, k >= 1, element-wise over n floats, in float64:
 *   d = x - mean;  mean += d / k;  m2 += d * (x - mean)
 * k == 1 initialises both buffers (they are not read and need not be zeroed).  Null pointers, n <= 0, k < 1, mean == m2: CINE_EINVAL. */
int cine_replica_accum(const float* x, double* mean, double* m2, long n, int k, void* stream);
/* The maps of k >= 2 accumulated samples: var = m2 / (k - 1), std = sqrt(var), mean_out = mean, snr = |mean| / std (0 where std == 0),
 * g = std / (ref_std * sqrt(accel)) (0 where ref_std == 0).  pairs != 0: the n floats are n / 2 complex values, var = var_re + var_im,
 * the mean's magnitude |mean| takes the place of the mean, and every map (ref_std too) has n / 2 elements; n must then be even.  Any
 * output may be NULL; g_out needs ref_std and accel > 0.  Computed in float64, rounded once.  CINE_EINVAL for what is stated above,
 * null mean / m2, n <= 0 and k < 2. */
int cine_replica_finish(const double* mean, const double* m2, long n, int k, int pairs, const float* ref_std, float accel,
                        float* mean_out, float* std_out, float* snr_out, float* g_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * measurement aid (no reference counterpart; the reference only wraps time.time() around the
 * model call, traintest_scripts/run_inference.py:53-61)
 * ------------------------------------------------------------------------------------------ */
/* Between cine_profile_begin() and cine_profile_end() every kernel launch made through this
 * library is bracketed by a hipEvent pair on the stream it is launched on.  cine_profile_end()
 * waits for them and returns, per kernel family i < nfam, the summed device time in ms and the
 * launch count.  Not for use during graph capture. */
int cine_profile_begin(void);
/* Diagnostics: process-wide counts of launches that took one of two interchangeable routes, so that a test can prove WHICH ran
 * (`which`: 0 plane-wide weight gradients on the lean kernel, 1 on the general kernel, 2 U-Net passes run as concurrent branches,
 * 3 BCRNN layers run by the C time-sweep entry points; the forward-convolution launches, counted where each is committed:
 * 4 the lean plane-wide 3x3 kernel, 5 the plane-wide transpose-conv kernel, 6 the 16-wide column-tile kernel on 2-D planes,
 * 7 the same in its three-pass volume form, 8 the coarse K-split kernel, 9 the streaming 1x1 kernel of cine_conv1x1_bias,
 * 10 the general kernel's two-set pair form, 11 the general kernel with vectorised staging, 12 the general kernel with element-wise
 * staging -- input-gradient launches on the general kernel count in 10 .. 12 too; 13 / 14 cine_pool3d_act on its float4 / scalar
 * kernel; 15 column-pass launches that weight by a mask plane: cine_image_dc_general / cine_normal_op_general /
 * cine_image_dc_general_sens_grad; 32 column-pass launches of cine_kspace_loss / cine_kspace_loss_grad -- counters added after the
 * first block take ids from 32 on, 16 .. 31 stay unknown).  reset != 0 returns the count and zeroes it; -1 for an unknown counter. */
long cine_diag_counter(int which, int reset);
/* Diagnostics: a one-workgroup kernel that runs for `microseconds` (1 .. 100 000; clock-bounded AND iteration-bounded: it always ends).  The
 * binding times two of them on two streams to learn whether the streams share a hardware queue (GPU_MAX_HW_QUEUES): streams on one queue run
 * one after the other, and a side stream chosen that way would serialise with its main stream. */
int cine_spin(int microseconds, void* stream);
int cine_profile_end(double* ms, long* launches, int nfam);
int cine_profile_families(void);
const char* cine_profile_family_name(int family);

#ifdef __cplusplus
}
#endif
#endif /* CINE_HIP_H */
