// kt_kernels.hip -- k-t SPARSE-SENSE: the proximal half of a FISTA iteration with a temporal-sparsity penalty, and the whole solve.
//
// No reference counterpart (the reference has no weight-free reconstruction beyond the zero-filled image); the iteration is the
// compressed-sensing baseline of the cine literature (Lustig et al., k-t SPARSE, ISMRM 2006; Otazo et al., MRM 2010) on this library's own
// operators:
//     g = A^H M A z - zf                          cine_image_dc_t / cine_image_dc_general, weights (1, 0, -1)
//     v = z - step g
//     xnew = F_t^H soft(F_t v, step * thresh * w_f)     F_t = fft1c variant 0 along t, w_f = 1 (0 at the DC bin t / 2 with penalise_dc == 0)
//     znew = xnew + beta (xnew - xprev)
// kt_prox_kernel is everything after g, in one launch.  Its shape is temporal_fwd_kernel / xfyf_unpack_kernel of pack_kernels.hip: one
// workgroup = kKtPix consecutive pixels of (b, h*w) with all T frames in LDS ([T][kKtPix] complex, 32 KiB at T = 64, plus T twiddles), loads
// and stores with the pixel on the lanes, a direct DFT per (pixel, bin) and per (pixel, frame).  The thresholded coefficients ride in
// registers across the barrier and go back into the SAME tile, so the tile never doubles and the kernel needs no large-LDS opt-in.
// A workgroup owns all frames of its pixels and has read z (all of it) and xprev (the element it is about to write) before it stores:
// znew may alias z and xnew may alias xprev.
#include "solve.h"

namespace cine {

constexpr int kKtPix = 64;           // pixels per workgroup: one wavefront = one bin / frame of the tile, so twiddle reads are broadcasts
constexpr int kKtThreads = kSolveThreads;
constexpr int kKtMaxT = 64;
constexpr int kKtItems = kKtMaxT * kKtPix / kKtThreads;       // (pixel, bin) pairs per thread at T = 64: the register stage

struct KtProxArgs {
    const cf* z; const cf* g; const cf* xprev;
    const float* step; const float* thresh;
    cf* xnew; cf* znew;
    float* part;                     // 4 floats per workgroup, or NULL
    float beta;
    int T, penalise_dc;
    long HW;
};

__global__ __launch_bounds__(kKtThreads) void kt_prox_kernel(KtProxArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float red[3 * kKtThreads / 64];
    cf* buf = reinterpret_cast<cf*>(smem);          // [T][kKtPix]
    cf* tw = buf + a.T * kKtPix;                    // [T]: temporal_twiddles
    const int T = a.T, tid = threadIdx.x;
    const int b = blockIdx.y;
    const long HW = a.HW;
    const long p0 = (long)blockIdx.x * kKtPix;
    const int np = (int)min((long)kKtPix, HW - p0);
    const int total = T * kKtPix;
    const float step = *a.step;
    const float theta = step * *a.thresh;
    temporal_twiddles(tw, T, tid);
    // v = z - step g, pixels on the lanes; the columns past the image hold zeros (they transform to zeros and add nothing to the sums)
    for (int e = tid; e < total; e += kKtThreads) {
        const int t = e / kKtPix, p = e - t * kKtPix;
        cf v = mk(0.f, 0.f);
        if (p < np) {
            const long q = ((long)b * T + t) * HW + p0 + p;
            v = solve_v(a.z[q], a.g[q], step);
        }
        buf[e] = v;
    }
    __syncthreads();
    // centered forward DFT per (pixel, bin) and the soft threshold; the results wait in registers until every thread has read the tile
    cf coef[kKtItems];
    float s_l1 = 0.f;
#pragma unroll
    for (int j = 0; j < kKtItems; ++j) {
        const int e = tid + j * kKtThreads;
        coef[j] = mk(0.f, 0.f);
        if (e < total) {
            const int i = e / kKtPix, p = e - i * kKtPix;
            const bool weighted = a.penalise_dc || i != T / 2;
            float left;
            coef[j] = soft_threshold(temporal_dft_fwd<kKtPix>(buf, tw, T, i, p), weighted ? theta : 0.f, left);
            if (weighted) s_l1 += left;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kKtItems; ++j) {
        const int e = tid + j * kKtThreads;
        if (e < total) buf[e] = coef[j];
    }
    __syncthreads();
    // centered inverse DFT per (pixel, frame), the extrapolation, stores with the pixel on the lanes
    float s_dx = 0.f, s_x2 = 0.f;
    for (int e = tid; e < total; e += kKtThreads) {
        const int i = e / kKtPix, p = e - i * kKtPix;
        if (p >= np) continue;
        const cf xn = temporal_dft_inv<kKtPix>(buf, tw, T, i, p);
        const long q = ((long)b * T + i) * HW + p0 + p;
        const cf xp = a.xprev[q];
        const float dx = xn.x - xp.x, dy = xn.y - xp.y;
        a.xnew[q] = xn;
        a.znew[q] = mk(xn.x + a.beta * dx, xn.y + a.beta * dy);
        s_dx += dx * dx + dy * dy;
        s_x2 += xn.x * xn.x + xn.y * xn.y;
    }
    if (a.part) {
        float s[3] = {s_dx, s_x2, s_l1};
        block_record(s, red, a.part, tid);
    }
}

static long kt_blocks(int b, int h, int w) { return ceil_div((long)h * w, (long)kKtPix) * b; }

// sizes of one prox launch: everything cine_kt_prox and cine_kt_fista refuse about (b, t, h, w)
static int kt_prox_sizes(const char* what, int b, int t, int h, int w) {
    return solve_sizes(what, b, t, h, w, kKtMaxT, ceil_div((long)h * w, (long)kKtPix));
}

static int kt_prox_launch(const float* z, const float* g, const float* xprev, const float* step_dev, const float* thresh_dev, float beta,
                          int penalise_dc, float* xnew, float* znew, float* part, int b, int t, int h, int w, hipStream_t st) {
    KtProxArgs a{};
    a.z = reinterpret_cast<const cf*>(z); a.g = reinterpret_cast<const cf*>(g); a.xprev = reinterpret_cast<const cf*>(xprev);
    a.step = step_dev; a.thresh = thresh_dev; a.xnew = reinterpret_cast<cf*>(xnew); a.znew = reinterpret_cast<cf*>(znew);
    a.part = part; a.beta = beta; a.T = t; a.penalise_dc = penalise_dc != 0; a.HW = (long)h * w;
    const size_t lds = ((size_t)t * kKtPix + t) * sizeof(cf);
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(kt_prox_kernel, dim3((unsigned)ceil_div(a.HW, (long)kKtPix), b), dim3(kKtThreads), lds, st, a);
    return check_launch("kt_prox_kernel");
}

// workspace of the solve: [operator scratch | g | z | iters rows of per-workgroup records]
struct KtSolveWs { size_t op_bytes, total; void* op; float* g; float* z; float* part; };

static KtSolveWs kt_solve_ws(void* ws, int b, int t, int c, int h, int w, int mask_w, int iters) {
    KtSolveWs y{};
    WsCursor at{static_cast<unsigned char*>(ws)};
    const size_t img = (size_t)b * t * h * w * sizeof(cf);
    y.op_bytes = dc_ws_bytes(mask_w, b, t, c, h, w);
    y.op = y.op_bytes ? at.take<void>(y.op_bytes) : nullptr;
    y.g = at.take<float>(img);
    y.z = at.take<float>(img);
    y.part = at.take<float>((size_t)iters * cine_kt_prox_ws_bytes(b, t, h, w));
    y.total = at.end;
    return y;
}

}  // namespace cine

using namespace cine;

extern "C" int cine_kt_prox_pixels(void) { return kKtPix; }

extern "C" size_t cine_kt_prox_ws_bytes(int b, int t, int h, int w) {
    if (b <= 0 || t <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)kt_blocks(b, h, w) * 4 * sizeof(float);
}

extern "C" int cine_kt_prox(const float* z, const float* g, const float* xprev, const float* step_dev, const float* thresh_dev,
                            float beta, int penalise_dc, float* xnew, float* znew, float* rec,
                            int b, int t, int h, int w, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_kt_prox";
    CINE_REQUIRE(z && g && xprev && step_dev && thresh_dev && xnew && znew && (!rec || ws), CINE_EINVAL, "%s: null pointer", what);
    if (int e = kt_prox_sizes(what, b, t, h, w)) return e;
    // an output may be the operand it replaces (xnew: xprev, znew: z) and nothing else
    CINE_REQUIRE(g != z && g != xprev && xnew != znew && xnew != g && znew != g && (xnew != z || z == xprev) && (znew != xprev || z == xprev) &&
                 xnew != step_dev && xnew != thresh_dev && znew != step_dev && znew != thresh_dev, CINE_EINVAL,
                 "%s: only znew == z and xnew == xprev may alias", what);
    if (rec) {
        const void* const outs[] = {rec};
        const void* const ins[] = {z, g, xprev, xnew, znew, step_dev, thresh_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, ws), CINE_EINVAL, "%s: rec and ws must not alias an operand or each other", what);
        const size_t need = cine_kt_prox_ws_bytes(b, t, h, w);
        CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    }
    hipStream_t st = as_stream(stream);
    float* part = rec ? reinterpret_cast<float*>(ws) : nullptr;
    if (int e = kt_prox_launch(z, g, xprev, step_dev, thresh_dev, beta, penalise_dc, xnew, znew, part, b, t, h, w, st)) return e;
    return rec ? solve_record_launch(part, kt_blocks(b, h, w), rec, 1, st) : CINE_OK;
}

extern "C" size_t cine_kt_fista_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int iters) {
    if (b <= 0 || t <= 0 || c <= 0 || h <= 0 || w <= 0 || iters <= 0) return 0;
    return kt_solve_ws(nullptr, b, t, c, h, w, mask_w, iters).total;
}

extern "C" int cine_kt_fista(float* x, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask, int mask_w,
                             const float* step_dev, const float* thresh_dev, int iters, int penalise_dc, float* rec,
                             int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_kt_fista";
    CINE_REQUIRE(x && zf && sens && mask && step_dev && thresh_dev && ws, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(c > 0 && iters >= 1, CINE_EINVAL, "%s: bad sizes", what);
    if (int e = kt_prox_sizes(what, b, t, h, w)) return e;
    CINE_REQUIRE(mask_w == 1 || mask_w == w, CINE_EINVAL, "%s: mask_w %d is neither 1 (row mask) nor w", what, mask_w);
    {
        const void* const outs[] = {x, rec};
        const void* const ins[] = {zf, sens, sens_tiled, mask, step_dev, thresh_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, ws), CINE_EINVAL, "%s: x, rec and ws must not alias an operand or each other", what);
    }
    const size_t need = cine_kt_fista_ws_bytes(b, t, c, h, w, mask_w, iters);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    const KtSolveWs y = kt_solve_ws(ws, b, t, c, h, w, mask_w, iters);
    const long nblk = kt_blocks(b, h, w);
    hipStream_t st = as_stream(stream);
    double s = 1.0;
    for (int k = 0; k < iters; ++k) {
        const float* zk = k == 0 ? zf : y.z;        // x_0 = z_0 = zf without a copy
        const float* xk = k == 0 ? zf : x;
        if (int e = solve_gradient(what, zk, zf, sens, sens_tiled, mask, mask_w, y.g, b, t, c, h, w, y.op, y.op_bytes, stream)) return e;
        const double s1 = 0.5 * (1.0 + sqrt(1.0 + 4.0 * s * s));
        const float beta = (float)((s - 1.0) / s1);
        s = s1;
        if (int e = kt_prox_launch(zk, y.g, xk, step_dev, thresh_dev, beta, penalise_dc, x, y.z, rec ? y.part + (size_t)k * nblk * 4 : nullptr,
                                   b, t, h, w, st))
            return e;
    }
    return rec ? solve_record_launch(y.part, nblk, rec, iters, st) : CINE_OK;
}
