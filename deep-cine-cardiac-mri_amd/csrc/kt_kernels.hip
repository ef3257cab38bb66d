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
#include <string>
#include "common.h"
#include "fft_core.h"

namespace cine {

constexpr int kKtPix = 64;           // pixels per workgroup: one wavefront = one bin / frame of the tile, so twiddle reads are broadcasts
constexpr int kKtThreads = 256;
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

__device__ __forceinline__ float kt_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kKtThreads) void kt_prox_kernel(KtProxArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float red[3][kKtThreads / 64];
    cf* buf = reinterpret_cast<cf*>(smem);          // [T][kKtPix]
    cf* tw = buf + a.T * kKtPix;                    // [T]: exp(-2 pi i j / T) / sqrt(T)
    const int T = a.T, tid = threadIdx.x;
    const int b = blockIdx.y;
    const long HW = a.HW;
    const long p0 = (long)blockIdx.x * kKtPix;
    const int np = (int)min((long)kKtPix, HW - p0);
    const int total = T * kKtPix;
    const float step = *a.step;
    const float theta = step * *a.thresh;
    {
        const double s = 1.0 / sqrt((double)T);
        for (int j = tid; j < T; j += kKtThreads) {
            double sn, cs;
            sincospi(2.0 * (double)j / (double)T, &sn, &cs);
            tw[j] = mk((float)(cs * s), (float)(-sn * s));
        }
    }
    // v = z - step g, pixels on the lanes; the columns past the image hold zeros (they transform to zeros and add nothing to the sums)
    for (int e = tid; e < total; e += kKtThreads) {
        const int t = e / kKtPix, p = e - t * kKtPix;
        cf v = mk(0.f, 0.f);
        if (p < np) {
            const long q = ((long)b * T + t) * HW + p0 + p;
            const cf zz = a.z[q], gg = a.g[q];
            v = mk(zz.x - step * gg.x, zz.y - step * gg.y);
        }
        buf[e] = v;
    }
    __syncthreads();
    const int s_in = (T + 1) / 2, s_out = T / 2;
    // centered forward DFT per (pixel, bin) and the soft threshold; the results wait in registers until every thread has read the tile
    cf coef[kKtItems];
    float s_l1 = 0.f;
#pragma unroll
    for (int j = 0; j < kKtItems; ++j) {
        const int e = tid + j * kKtThreads;
        coef[j] = mk(0.f, 0.f);
        if (e < total) {
            const int i = e / kKtPix, p = e - i * kKtPix;
            int k = i - s_out; if (k < 0) k += T;
            float ax = 0.f, ay = 0.f;
            int idx = (s_in * k) % T;                // n = (g + s_in) % T  ->  (n * k) % T
            for (int g = 0; g < T; ++g) {
                const cf w = tw[idx];
                const cf x = buf[g * kKtPix + p];
                ax += x.x * w.x - x.y * w.y; ay += x.x * w.y + x.y * w.x;
                idx += k; if (idx >= T) idx -= T;
            }
            const bool weighted = a.penalise_dc || i != s_out;
            const float th = weighted ? theta : 0.f;
            const float mag = sqrtf(ax * ax + ay * ay);
            const float sc = mag > th ? (mag - th) / mag : 0.f;      // soft(c, th) = c max(|c| - th, 0) / |c|, 0 at c = 0
            coef[j] = mk(ax * sc, ay * sc);
            if (weighted) s_l1 += mag > th ? mag - th : 0.f;
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
        int k = i - s_out; if (k < 0) k += T;
        float ax = 0.f, ay = 0.f;
        int idx = (s_in * k) % T;
        for (int g = 0; g < T; ++g) {
            const cf w = tw[idx];
            const cf x = buf[g * kKtPix + p];
            ax += x.x * w.x + x.y * w.y; ay += x.y * w.x - x.x * w.y;         // x * conj(w)
            idx += k; if (idx >= T) idx -= T;
        }
        const long q = ((long)b * T + i) * HW + p0 + p;
        const cf xp = a.xprev[q];
        const float dx = ax - xp.x, dy = ay - xp.y;
        a.xnew[q] = mk(ax, ay);
        a.znew[q] = mk(ax + a.beta * dx, ay + a.beta * dy);
        s_dx += dx * dx + dy * dy;
        s_x2 += ax * ax + ay * ay;
    }
    if (a.part) {                                   // one record per workgroup; kt_record_kernel adds them in a fixed order
        const float v0 = kt_wave_sum(s_dx), v1 = kt_wave_sum(s_x2), v2 = kt_wave_sum(s_l1);
        if ((tid & 63) == 0) { red[0][tid >> 6] = v0; red[1][tid >> 6] = v1; red[2][tid >> 6] = v2; }
        __syncthreads();
        if (tid == 0) {
            float r[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) r[q] = (red[q][0] + red[q][1]) + (red[q][2] + red[q][3]);
            float* o = a.part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = 0.f;
        }
    }
}

// rows of nblk records each -> rec (rows, 4): the records of a row added in float64 in a fixed order (one workgroup per row)
__global__ __launch_bounds__(256) void kt_record_kernel(const float* part, long nblk, float* rec) {
    __shared__ double red[3][256];
    const int tid = threadIdx.x;
    const float* p = part + (long)blockIdx.x * nblk * 4;
    double s[3] = {0.0, 0.0, 0.0};
    for (long e = tid; e < nblk; e += 256) {
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += (double)p[e * 4 + q];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) red[q][tid] = s[q];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        float* o = rec + (long)blockIdx.x * 4;
        o[0] = (float)red[0][0]; o[1] = (float)red[1][0]; o[2] = (float)red[2][0]; o[3] = 0.f;
    }
}

static long kt_blocks(int b, int h, int w) { return ceil_div((long)h * w, (long)kKtPix) * b; }

// sizes of one prox launch: everything cine_kt_prox and cine_kt_fista refuse about (b, t, h, w)
static int kt_prox_sizes(const char* what, int b, int t, int h, int w) {
    CINE_REQUIRE(b > 0 && t > 0 && h > 0 && w > 0, CINE_EINVAL, "%s: bad sizes", what);
    CINE_REQUIRE(t >= 2 && t <= kKtMaxT, CINE_EUNSUPPORTED, "%s: %d frames, 2 .. %d are supported", what, t, kKtMaxT);
    CINE_REQUIRE(b <= 65535, CINE_EUNSUPPORTED, "%s: b > 65535", what);                    // b rides on grid.y
    CINE_REQUIRE(ceil_div((long)h * w, (long)kKtPix) <= 2147483647L, CINE_EUNSUPPORTED, "%s: h*w too large", what);
    return CINE_OK;
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

static int kt_record_launch(const float* part, long nblk, float* rec, int rows, hipStream_t st) {
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(kt_record_kernel, dim3(rows), dim3(256), 0, st, part, nblk, rec);
    return check_launch("kt_record_kernel");
}

static size_t kt_align(size_t n) { return (n + 255) & ~(size_t)255; }

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
        const void* r = rec;
        CINE_REQUIRE(r != z && r != g && r != xprev && r != xnew && r != znew && r != step_dev && r != thresh_dev && r != ws &&
                     ws != (const void*)z && ws != (const void*)g && ws != (const void*)xprev && ws != (const void*)xnew && ws != (const void*)znew &&
                     ws != (const void*)step_dev && ws != (const void*)thresh_dev, CINE_EINVAL, "%s: rec and ws must not alias an operand or each other", what);
        const size_t need = cine_kt_prox_ws_bytes(b, t, h, w);
        CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    }
    hipStream_t st = as_stream(stream);
    float* part = rec ? reinterpret_cast<float*>(ws) : nullptr;
    if (int e = kt_prox_launch(z, g, xprev, step_dev, thresh_dev, beta, penalise_dc, xnew, znew, part, b, t, h, w, st)) return e;
    return rec ? kt_record_launch(part, kt_blocks(b, h, w), rec, 1, st) : CINE_OK;
}

// workspace of the solve: [operator scratch | g | z | iters rows of per-workgroup records], each part on a 256-byte boundary
extern "C" size_t cine_kt_fista_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int iters) {
    if (b <= 0 || t <= 0 || c <= 0 || h <= 0 || w <= 0 || iters <= 0) return 0;
    const size_t op = mask_w == 1 ? cine_image_dc_ws_bytes(b, t, c, h, w) : cine_image_dc_general_ws_bytes(b, t, c, h, w);
    const size_t img = kt_align((size_t)b * t * h * w * sizeof(cf));
    return kt_align(op) + 2 * img + (size_t)iters * cine_kt_prox_ws_bytes(b, t, h, w);
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
        const void* o = x; const void* r = rec;
        CINE_REQUIRE(o != zf && o != sens && o != sens_tiled && o != mask && o != step_dev && o != thresh_dev && o != ws && o != r, CINE_EINVAL,
                     "%s: x must not alias another operand", what);
        CINE_REQUIRE(!r || (r != zf && r != sens && r != sens_tiled && r != mask && r != step_dev && r != thresh_dev && r != ws), CINE_EINVAL,
                     "%s: rec must not alias another operand", what);
        CINE_REQUIRE(ws != (const void*)zf && ws != (const void*)sens && ws != (const void*)sens_tiled && ws != (const void*)mask &&
                     ws != (const void*)step_dev && ws != (const void*)thresh_dev, CINE_EINVAL, "%s: ws must not alias an operand", what);
    }
    const size_t need = cine_kt_fista_ws_bytes(b, t, c, h, w, mask_w, iters);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    const bool row = mask_w == 1;
    const size_t op_bytes = row ? cine_image_dc_ws_bytes(b, t, c, h, w) : cine_image_dc_general_ws_bytes(b, t, c, h, w);
    const size_t img_bytes = kt_align((size_t)b * t * h * w * sizeof(cf));
    unsigned char* base = reinterpret_cast<unsigned char*>(ws);
    void* op_ws = op_bytes ? base : nullptr;
    float* g = reinterpret_cast<float*>(base + kt_align(op_bytes));
    float* z = reinterpret_cast<float*>(base + kt_align(op_bytes) + img_bytes);
    float* part = reinterpret_cast<float*>(base + kt_align(op_bytes) + 2 * img_bytes);
    const long nblk = kt_blocks(b, h, w);
    hipStream_t st = as_stream(stream);
    double s = 1.0;
    for (int k = 0; k < iters; ++k) {
        const float* zk = k == 0 ? zf : z;          // x_0 = z_0 = zf without a copy
        const float* xk = k == 0 ? zf : x;
        const int e = row ? cine_image_dc_t(zk, sens, sens_tiled, zf, mask, nullptr, 1.f, 0.f, -1.f, g, b, t, c, h, w, 0, op_ws, op_bytes, stream)
                          : cine_image_dc_general(zk, sens, zf, mask, nullptr, 1.f, 0.f, -1.f, g, b, t, c, h, w, 0, op_ws, op_bytes, stream);
        if (e) {                                    // at k == 0 nothing has been launched yet: the operator's own refusal of a size
            const std::string why = cine_last_error();
            set_error("%s: %s", what, why.c_str());
            return e;
        }
        const double s1 = 0.5 * (1.0 + sqrt(1.0 + 4.0 * s * s));
        const float beta = (float)((s - 1.0) / s1);
        s = s1;
        if (int e2 = kt_prox_launch(zk, g, xk, step_dev, thresh_dev, beta, penalise_dc, x, z, rec ? part + (size_t)k * nblk * 4 : nullptr,
                                    b, t, h, w, st))
            return e2;
    }
    return rec ? kt_record_launch(part, nblk, rec, iters, st) : CINE_OK;
}
