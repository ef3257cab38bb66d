// grappa_gfactor_kernels.hip -- the analytic noise map of a lattice GRAPPA reconstruction (Breuer et al., MRM 62:739, 2009) from the
// weights of cine_grappa_weights: the R - 1 k-space kernels are one convolution kernel K[q][k][dy][dx], its transform is a c x c matrix
// Wimg(y, x) per pixel, and the noise variance of a linear coil combination p is p Wimg Psi Wimg^H p^H.  The contract is in
// include/cine_hip.h.
//
//   cine_grappa_image_weights   Wimg itself, (c, c, h, w).
//   cine_grappa_gfactor         the hot path: g and the noise amplitude with Wimg never leaving the chip.
//
// Both share one workgroup shape: 256 lanes own 256 pixels x of one image row y.
//   stage 1   the row's phase factors e(dy) = exp(-2 pi i dy (y - h / 2) / h) of the (R - 1) ky row offsets, then
//             B[dx][q][k] = [dx = hx, q = k] + sum_{m, j} W[m - 1][(j, dx, k)][q] e(-m - base + j R) into LDS, (m, j) ascending: kx c^2
//             entries of (R - 1) ky terms each, the thread index runs over q first so that the weights are read in their own order.
//   stage 1b  (gfactor, chol given) every row B[dx][q][:] becomes B[dx][q][:] L in place: entry j needs the entries k >= j only, so one
//             thread walks its row in ascending j.  Rows are c + 1 elements apart: the 32 lanes of an LDS access group hit 32 bank pairs.
//   stage 2   a lane forms u = sum_dx B[dx][q][j] e_x(dx) from its own kx column phases; every lane of a wave reads the same LDS address
//             (a broadcast).  Per coil it adds |u|^2 over j; with coefficients it keeps p[q] in registers (32 named slots), forms
//             t_j = sum_q p_q u, four coils' reads in flight at a time, and adds |t_j|^2 over j.  A lane never holds more than c values and nothing is exchanged between lanes.
// The work is about c^2 kx complex fmaf per pixel (1 GFLOP at 15 coils, 200 x 200), a few microseconds of the vector units: putting stage
// 2 on the matrix cores would need the per-pixel phases as an operand tile and buy nothing measurable, so this is plain fp32 VALU code.
// Phases come from sincospif of the exactly reduced integer (d rho mod n): no drift however large rho is.  Every sum runs in a fixed
// order, there are no atomics and nothing is read by the host.
#include <cmath>
#include <cstdint>
#include <mutex>
#include "common.h"
#include "solve.h"                   // large_lds_opt_in

namespace cine {

namespace gf {
constexpr int kMaxCoils = 32, kMaxAug = 1152;
constexpr int kThreads = 256;
constexpr int kMaxDim = 1 << 20;              // h, w: 2 r of the reduced phase integer is exact in fp32 far beyond this
}

struct GfactorArgs {
    const float2* weights;                       // (R - 1, ns, c)
    const float2* chol;                          // (c, c) or null
    const float2* coef;                          // (n, c, h, w) or null
    float* g;                                    // (n or c, h, w) or null
    float* amp;                                  // likewise
    float2* wimg;                                // image weights (c, c, h, w): the other kernel's output
    int n, c, h, w, R, ky, kx, ns;
};

// exp(-2 pi i d rho / n) from r = d rho mod n, folded into (-n / 2, n / 2]
__device__ __forceinline__ float2 gf_phase(int d, int rho, int n) {
    long r = ((long)d * rho) % n;
    if (r < 0) r += n;
    if (2 * r > n) r -= n;
    float s, c;
    sincospif(-(float)(2 * r) / (float)n, &s, &c);
    return make_float2(c, s);
}

__device__ __forceinline__ void gf_cfma(float2& acc, const float2 a, const float2 b) {
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.x = fmaf(-a.y, b.y, acc.x);
    acc.y = fmaf(a.x, b.y, acc.y);
    acc.y = fmaf(a.y, b.x, acc.y);
}

// LDS of one workgroup in float2 elements: B [kx c][c + 1] | L [c][c + 1] | ey [(R - 1) ky] | psi [c] (as floats in float2 slots)
__host__ __device__ inline size_t gf_lds_elems(int c, int R, int ky, int kx) {
    return (size_t)(kx * c + c) * (c + 1) + (size_t)(R - 1) * ky + (size_t)c;
}

// stages 1 and 1b for row y; returns with the LDS staged and the workgroup synchronised
__device__ __forceinline__ void gf_stage_row(const GfactorArgs& a, int y, bool with_chol, float2* B, float2* Ls, float2* ey, float* psi) {
    const int tid = threadIdx.x, c = a.c, R = a.R, ky = a.ky, kx = a.kx, S = c + 1;
    const int base = (ky / 2 - 1) * R, hx = kx / 2;
    const int rho = y - a.h / 2;
    for (int e = tid; e < (R - 1) * ky; e += gf::kThreads) {
        const int m1 = e / ky, j = e - m1 * ky;
        ey[e] = gf_phase(-(m1 + 1) - base + j * R, rho, a.h);
    }
    if (with_chol) {
        for (int e = tid; e < c * c; e += gf::kThreads) {
            const int k = e / c, j = e - k * c;
            Ls[k * S + j] = j <= k ? a.chol[e] : make_float2(0.f, 0.f);
        }
    }
    __syncthreads();
    for (int e = tid; e < kx * c * c; e += gf::kThreads) {
        const int q = e % c, r = e / c, k = r % c, dx = r / c;
        float2 acc = make_float2((dx == hx && q == k) ? 1.f : 0.f, 0.f);
        for (int m1 = 0; m1 < R - 1; ++m1)
            for (int j = 0; j < ky; ++j)
                gf_cfma(acc, a.weights[((long)m1 * a.ns + (j * kx + dx) * c + k) * c + q], ey[m1 * ky + j]);
        B[(dx * c + q) * S + k] = acc;
    }
    if (with_chol && tid < c) {                  // Psi_qq = sum_{j <= q} |L[q][j]|^2
        float s = 0.f;
        for (int j = 0; j <= tid; ++j) {
            const float2 v = Ls[tid * S + j];
            s = fmaf(v.x, v.x, s);
            s = fmaf(v.y, v.y, s);
        }
        psi[tid] = s;
    }
    __syncthreads();
    if (!with_chol) return;
    for (int row = tid; row < kx * c; row += gf::kThreads) {
        float2* b = B + row * S;
        for (int j = 0; j < c; ++j) {
            float2 acc = make_float2(0.f, 0.f);
            for (int k = j; k < c; ++k) gf_cfma(acc, b[k], Ls[k * S + j]);
            b[j] = acc;
        }
    }
    __syncthreads();
}

#define GF_LDS_VIEWS(a)                                                             \
    extern __shared__ __attribute__((aligned(16))) unsigned char gf_lds[];          \
    float2* B = reinterpret_cast<float2*>(gf_lds);                                  \
    float2* Ls = B + (a).kx * (a).c * ((a).c + 1);                                  \
    float2* ey = Ls + (a).c * ((a).c + 1);                                          \
    float* psi = reinterpret_cast<float*>(ey + ((a).R - 1) * (a).ky)

// Workgroup: pixels x = 256 blockIdx.y + tid of row blockIdx.x.  out[q][k][y][x] = sum_dx B[dx][q][k] e_x(dx), dx ascending.
template <int KX>
__global__ __launch_bounds__(gf::kThreads) void grappa_image_weights_kernel(GfactorArgs a) {
    GF_LDS_VIEWS(a);
    const int y = blockIdx.x, c = a.c, S = c + 1;
    gf_stage_row(a, y, false, B, Ls, ey, psi);
    const int x = blockIdx.y * gf::kThreads + threadIdx.x;
    if (x >= a.w) return;
    float2 ex[KX];
#pragma unroll
    for (int dx = 0; dx < KX; ++dx) ex[dx] = gf_phase(dx - KX / 2, x - a.w / 2, a.w);
    const long plane = (long)a.h * a.w;
    float2* dst = a.wimg + (long)y * a.w + x;
#pragma unroll 4
    for (int qk = 0; qk < c * c; ++qk) {
        const int q = qk / c, k = qk - q * c;
        float2 u = make_float2(0.f, 0.f);
#pragma unroll
        for (int dx = 0; dx < KX; ++dx) gf_cfma(u, B[(dx * c + q) * S + k], ex[dx]);
        dst[(long)qk * plane] = u;
    }
}

// Workgroup: pixels x = 256 blockIdx.y + tid of row blockIdx.x, every coil (COEF = false) or every coefficient set (COEF = true).
template <int KX, bool COEF>
__global__ __launch_bounds__(gf::kThreads) void grappa_gfactor_kernel(GfactorArgs a) {
    GF_LDS_VIEWS(a);
    const int y = blockIdx.x, c = a.c, S = c + 1;
    const bool with_chol = a.chol != nullptr;
    gf_stage_row(a, y, with_chol, B, Ls, ey, psi);
    const int x = blockIdx.y * gf::kThreads + threadIdx.x;
    if (x >= a.w) return;
    float2 ex[KX];
#pragma unroll
    for (int dx = 0; dx < KX; ++dx) ex[dx] = gf_phase(dx - KX / 2, x - a.w / 2, a.w);
    const long plane = (long)a.h * a.w, pix = (long)y * a.w + x;
    const float inv_r = 1.f / (float)a.R;
    if (!COEF) {
        for (int q = 0; q < c; ++q) {
            float amp2 = 0.f;
#pragma unroll 4
            for (int j = 0; j < c; ++j) {        // four j at a time: their LDS reads are in flight together
                float2 u = make_float2(0.f, 0.f);
#pragma unroll
                for (int dx = 0; dx < KX; ++dx) gf_cfma(u, B[(dx * c + q) * S + j], ex[dx]);
                amp2 = fmaf(u.x, u.x, amp2);
                amp2 = fmaf(u.y, u.y, amp2);
            }
            const float den2 = with_chol ? psi[q] : 1.f;
            if (a.amp) a.amp[q * plane + pix] = sqrtf(amp2);
            if (a.g) a.g[q * plane + pix] = den2 > 0.f ? sqrtf(amp2 / den2) * inv_r : 0.f;
        }
        return;
    }
    for (int i = 0; i < a.n; ++i) {
        const float2* cp = a.coef + (long)i * c * plane + pix;
        float2 p[gf::kMaxCoils];                 // constant indices only: the slots stay in registers
#pragma unroll
        for (int q = 0; q < gf::kMaxCoils; ++q) {   // every load is issued, from a clamped address: none waits for a branch
            const float2 v = cp[(q < c ? q : c - 1) * plane];
            p[q] = q < c ? v : make_float2(0.f, 0.f);
        }
        float amp2 = 0.f, den2 = 0.f;
        for (int j = 0; j < c; ++j) {
            float2 t = make_float2(0.f, 0.f), d = make_float2(0.f, 0.f);
#pragma unroll
            for (int q0 = 0; q0 < gf::kMaxCoils; q0 += 4) {
                if (q0 < c) {                    // uniform; constant trip counts, so that the loops unroll and p[q] is a register.  Four
                    float2 u[4];                 // coils at a time: their 4 KX LDS reads are in flight together.  A coil at or beyond c
#pragma unroll
                    for (int i = 0; i < 4; ++i) {   // reads coil c - 1 instead and has p = 0: it adds an exact zero
                        const int qa = q0 + i < c ? q0 + i : c - 1;
                        u[i] = make_float2(0.f, 0.f);
#pragma unroll
                        for (int dx = 0; dx < KX; ++dx) gf_cfma(u[i], B[(dx * c + qa) * S + j], ex[dx]);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) gf_cfma(t, p[q0 + i], u[i]);
                    if (with_chol) {             // L is zero above the diagonal: the terms q < j add exact zeros
#pragma unroll
                        for (int i = 0; i < 4; ++i) gf_cfma(d, p[q0 + i], Ls[(q0 + i < c ? q0 + i : c - 1) * S + j]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) d = q0 + i == j ? p[q0 + i] : d;
                    }
                }
            }
            amp2 = fmaf(t.x, t.x, amp2);
            amp2 = fmaf(t.y, t.y, amp2);
            den2 = fmaf(d.x, d.x, den2);
            den2 = fmaf(d.y, d.y, den2);
        }
        if (a.amp) a.amp[i * plane + pix] = sqrtf(amp2);
        if (a.g) a.g[i * plane + pix] = den2 > 0.f ? sqrtf(amp2 / den2) * inv_r : 0.f;
    }
}

namespace {

bool gf_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// [p, p + bytes) and [q, q + qbytes) share a byte; a null pointer overlaps nothing
bool gf_overlap(const void* p, size_t bytes, const void* q, size_t qbytes) {
    if (!p || !q) return false;
    const char *a = static_cast<const char*>(p), *b = static_cast<const char*>(q);
    return a < b + qbytes && b < a + bytes;
}

// the checks both entries share: 0, or the code with the message set
int gf_shapes(const char* what, int c, int h, int w, int R, int ky, int kx) {
    CINE_REQUIRE(c >= 1 && h >= 1 && w >= 1, CINE_EINVAL, "%s: Invalid shapes. (coils %d, %d x %d)", what, c, h, w);
    CINE_REQUIRE(R >= 2 && R <= 8 && (ky == 2 || ky == 4) && (kx == 3 || kx == 5 || kx == 7), CINE_EINVAL,
                 "%s: acceleration %d (2 .. 8), kernel %d x %d (2 or 4 rows, 3, 5 or 7 columns)", what, R, ky, kx);
    CINE_REQUIRE(c <= gf::kMaxCoils, CINE_EUNSUPPORTED, "%s: %d coils, at most %d", what, c, gf::kMaxCoils);
    CINE_REQUIRE(ky * kx * c + (R - 1) * c <= gf::kMaxAug, CINE_EUNSUPPORTED, "%s: n_aug = %d x %d x %d coils + %d x %d coils = %d, at most %d", what,
                 ky, kx, c, R - 1, c, ky * kx * c + (R - 1) * c, gf::kMaxAug);
    CINE_REQUIRE(h <= gf::kMaxDim && w <= gf::kMaxDim, CINE_EUNSUPPORTED, "%s: %d x %d pixels, at most 2^20 each", what, h, w);
    return CINE_OK;
}

template <typename Kern>
int gf_launch(Kern kern, const char* what, const GfactorArgs& a, std::once_flag* once, hipError_t* status, hipStream_t st) {
    const size_t lds = gf_lds_elems(a.c, a.R, a.ky, a.kx) * sizeof(float2);
    if (lds >= 64 * 1024)
        if (int e = large_lds_opt_in(reinterpret_cast<const void*>(kern), what, once, status)) return e;
    const dim3 grid((unsigned)a.h, (unsigned)ceil_div(a.w, gf::kThreads));
    hipLaunchKernelGGL(kern, grid, dim3(gf::kThreads), lds, st, a);
    return check_launch(what);
}

}  // namespace
}  // namespace cine

using namespace cine;

extern "C" int cine_grappa_image_weights(const float* weights, float* out, int c, int h, int w, int R, int ky, int kx, void* stream) {
    CINE_REQUIRE(weights && out, CINE_EINVAL, "cine_grappa_image_weights: null pointer");
    if (int e = gf_shapes("cine_grappa_image_weights", c, h, w, R, ky, kx)) return e;
    CINE_REQUIRE(gf_aligned(weights, 8) && gf_aligned(out, 8), CINE_EINVAL, "cine_grappa_image_weights: weights and out must be 8-byte aligned");
    const size_t wbytes = (size_t)(R - 1) * ky * kx * c * c * sizeof(float2), obytes = (size_t)c * c * h * w * sizeof(float2);
    CINE_REQUIRE(!gf_overlap(out, obytes, weights, wbytes), CINE_EINVAL, "cine_grappa_image_weights: out overlaps weights");
    GfactorArgs a{};
    a.weights = reinterpret_cast<const float2*>(weights);
    a.wimg = reinterpret_cast<float2*>(out);
    a.n = 1; a.c = c; a.h = h; a.w = w; a.R = R; a.ky = ky; a.kx = kx; a.ns = ky * kx * c;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    static std::once_flag once[3][64];
    static hipError_t status[3][64];
    switch (kx) {
        case 3: return gf_launch(grappa_image_weights_kernel<3>, "cine_grappa_image_weights", a, once[0], status[0], st);
        case 5: return gf_launch(grappa_image_weights_kernel<5>, "cine_grappa_image_weights", a, once[1], status[1], st);
        default: return gf_launch(grappa_image_weights_kernel<7>, "cine_grappa_image_weights", a, once[2], status[2], st);
    }
}

extern "C" int cine_grappa_gfactor(const float* weights, const float* chol, const float* coef, float* g, float* amp, int n, int c, int h, int w,
                                   int R, int ky, int kx, void* stream) {
    CINE_REQUIRE(weights && (g || amp), CINE_EINVAL, "cine_grappa_gfactor: null weights, or neither g nor amp");
    if (int e = gf_shapes("cine_grappa_gfactor", c, h, w, R, ky, kx)) return e;
    CINE_REQUIRE(n >= 1, CINE_EINVAL, "cine_grappa_gfactor: Invalid shapes. (%d coefficient sets)", n);
    CINE_REQUIRE(gf_aligned(weights, 8) && gf_aligned(chol, 8) && gf_aligned(coef, 8) && gf_aligned(g, 4) && gf_aligned(amp, 4), CINE_EINVAL,
                 "cine_grappa_gfactor: weights, chol and coef must be 8-byte aligned, g and amp 4-byte aligned");
    const size_t maps = coef ? (size_t)n : (size_t)c;
    const size_t wbytes = (size_t)(R - 1) * ky * kx * c * c * sizeof(float2), lbytes = (size_t)c * c * sizeof(float2);
    const size_t cbytes = (size_t)n * c * h * w * sizeof(float2), obytes = maps * h * w * sizeof(float);
    float* const outs[2] = {g, amp};
    for (float* o : outs)
        CINE_REQUIRE(!gf_overlap(o, obytes, weights, wbytes) && !gf_overlap(o, obytes, chol, lbytes) && !gf_overlap(o, obytes, coef, cbytes), CINE_EINVAL,
                     "cine_grappa_gfactor: an output overlaps an input");
    CINE_REQUIRE(!gf_overlap(g, obytes, amp, obytes), CINE_EINVAL, "cine_grappa_gfactor: g overlaps amp");
    GfactorArgs a{};
    a.weights = reinterpret_cast<const float2*>(weights);
    a.chol = reinterpret_cast<const float2*>(chol);
    a.coef = reinterpret_cast<const float2*>(coef);
    a.g = g; a.amp = amp;
    a.n = n; a.c = c; a.h = h; a.w = w; a.R = R; a.ky = ky; a.kx = kx; a.ns = ky * kx * c;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    static std::once_flag once[6][64];
    static hipError_t status[6][64];
    const char* what = "cine_grappa_gfactor";
    if (coef) {
        switch (kx) {
            case 3: return gf_launch(grappa_gfactor_kernel<3, true>, what, a, once[0], status[0], st);
            case 5: return gf_launch(grappa_gfactor_kernel<5, true>, what, a, once[1], status[1], st);
            default: return gf_launch(grappa_gfactor_kernel<7, true>, what, a, once[2], status[2], st);
        }
    }
    switch (kx) {
        case 3: return gf_launch(grappa_gfactor_kernel<3, false>, what, a, once[3], status[3], st);
        case 5: return gf_launch(grappa_gfactor_kernel<5, false>, what, a, once[4], status[4], st);
        default: return gf_launch(grappa_gfactor_kernel<7, false>, what, a, once[5], status[5], st);
    }
}
