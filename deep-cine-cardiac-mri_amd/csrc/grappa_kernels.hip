// grappa_kernels.hip -- GRAPPA / TGRAPPA (Griswold et al., MRM 47:1202, 2002; Breuer et al., MRM 53:981, 2005) on the device: the lattice
// offset of every frame, the Gram matrix of the calibration patches, the k-space kernels from it, and their application to the rows a
// frame did not acquire.  The reference has no such step.  The contract (layouts, source order, limits) is in include/cine_hip.h.
//
//   cine_grappa_offsets   one workgroup per frame: lane r < R walks rows r, r + R, ...; lane 0 takes the lowest residue whose rows are
//                         all acquired.
//   cine_grappa_gram      G = P^H P of the augmented patch matrix P = [sources | targets], as cine_espirit_gram: the calibration array
//                         is copied to [y][x][coil] float64 (cal_stage_kernel), then eight threads per entry of the upper triangle add the
//                         exact products of every eighth window row in float64 in window order, the eight sums are added in slice
//                         order, and G[a][b] and G[b][a] = conj are written.
//   cine_grappa_weights   (G_ss + tau I) W = G_st in float64 by a Newton-Schulz inverse on cine_zgemm_f64: X_0 = I / |A|_F,
//                         X <- X (2 I - A X), a number of steps fixed by ns and lam (the condition number is at most ns / lam + 1 by
//                         construction); W = X G_st, one step of iterative refinement W += X (G_st - A W), and the residual of the W
//                         that is handed out.  Every sum runs in a fixed order: the same bits on every call.
//   cine_grappa_apply     the hot path: a skinny complex GEMM per lattice gap on v_mfma_f32_16x16x4_f32, see grappa_apply_kernel.
#include <cmath>
#include <cstdint>
#include <mutex>
#include "common.h"
#include "conv_src.h"                // f32x4
#include "solve.h"                   // large_lds_opt_in

namespace cine {

namespace gr {
constexpr int kMaxCoils = 32, kMaxAug = 1152;
constexpr int kThreads = 256;
constexpr int kParts = 256;                   // partial sums of the reductions
constexpr int kMaxIters = 100;
constexpr int kGramSlices = 8;                // gram: slices of the window rows of one entry, added in slice order
constexpr int TX = 64;                        // apply: x-points of a tile, 16 per wave
constexpr int PX = 80;                        // apply: LDS row of one (source row, coil) in complex elements: TX + 6 halo, = 16 (mod 32)
constexpr int KC = 64;                        // apply: k-values of one staged weight chunk
}

// what the four entries share: the kernel geometry of (c, R, ky, kx), or false
struct GrappaGeom {
    int ns, nr, n_aug, span, base, hx;
};

static bool grappa_geom(int c, int R, int ky, int kx, GrappaGeom& g) {
    if (c < 1 || c > gr::kMaxCoils || R < 2 || R > 8 || (ky != 2 && ky != 4) || (kx != 3 && kx != 5 && kx != 7)) return false;
    g.ns = ky * kx * c;
    g.nr = (R - 1) * c;
    g.n_aug = g.ns + g.nr;
    g.span = (ky - 1) * R + 1;
    g.base = (ky / 2 - 1) * R;
    g.hx = kx / 2;
    return g.n_aug <= gr::kMaxAug;
}

// ------------------------------------------------------------------ lattice offsets
__global__ __launch_bounds__(64) void grappa_offsets_kernel(const uint8_t* __restrict__ mask, int* __restrict__ offsets, int* __restrict__ status,
                                                            int h, int R) {
    __shared__ int ok[8];
    const int f = blockIdx.x, r = threadIdx.x;
    if (r < R) {
        int all = 1;
        for (int y = r; y < h; y += R) all &= mask[(long)f * h + y] != 0;
        ok[r] = all;
    }
    __syncthreads();
    if (r != 0) return;
    int off = -1;
    for (int k = R - 1; k >= 0; --k)
        if (ok[k]) off = k;
    offsets[f] = off;
    status[f] = off < 0 ? 1 : 0;
}

// ------------------------------------------------------------------ Gram matrix of the augmented patch matrix
__global__ __launch_bounds__(256) void grappa_cal_stage_kernel(const float2* __restrict__ cal, double2* __restrict__ st, int c, int hc, int w) {
    const long total = (long)hc * w * c;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int coil = (int)(e % c);
        const long p = e / c;
        const int x = (int)(p % w), y = (int)(p / w);
        const float2 v = cal[((long)coil * hc + y) * w + x];
        st[e] = make_double2((double)v.x, (double)v.y);
    }
}

// column a of P -> (row offset, column offset, coil) within the window
__device__ __forceinline__ void grappa_column(int a, int c, int R, int kx, int ns, int base, int hx, int& dy, int& dx, int& coil) {
    if (a < ns) {
        const int tap = a / c, j = tap / kx;
        coil = a - tap * c;
        dx = tap - j * kx;
        dy = j * R;
    } else {
        const int e = a - ns, m1 = e / c;
        coil = e - m1 * c;
        dx = hx;
        dy = base + m1 + 1;
    }
}

// thread: entry (a = blockIdx.y, b = 32 blockIdx.x + (tid & 31)), b >= a, window rows y = s, s + 8, ... of slice s = tid >> 5; the eight
// slices of an entry are added in slice order by the thread of slice 0: an order fixed by the shape
__global__ __launch_bounds__(256) void grappa_gram_kernel(const double2* __restrict__ st, double2* __restrict__ gram, int c, int hc, int w, int R,
                                                          int ky, int kx, int ns, int n) {
    __shared__ double2 part[gr::kGramSlices][32];
    const int a = blockIdx.y;
    if ((int)blockIdx.x * 32 + 31 < a) return;   // uniform: the tile lies below the diagonal
    const int bl = threadIdx.x & 31, s = threadIdx.x >> 5;
    const int b = blockIdx.x * 32 + bl;
    const bool mine = b < n && b >= a;
    double re = 0.0, im = 0.0;                   // conj(u) v = (ur vr + ui vi) + i (ur vi - ui vr)
    if (mine) {
        const int span = (ky - 1) * R + 1, base = (ky / 2 - 1) * R, hx = kx / 2;
        int ay, ax, i, by, bx, j;
        grappa_column(a, c, R, kx, ns, base, hx, ay, ax, i);
        grappa_column(b, c, R, kx, ns, base, hx, by, bx, j);
        const int my = hc - span + 1, mx = w - kx + 1;
        for (int y = s; y < my; y += gr::kGramSlices) {
            const double2* ua = st + ((long)(y + ay) * w + ax) * c + i;
            const double2* vb = st + ((long)(y + by) * w + bx) * c + j;
#pragma unroll 4
            for (int x = 0; x < mx; ++x) {
                const double2 u = ua[(long)x * c], v = vb[(long)x * c];
                re = fma(u.x, v.x, re);
                re = fma(u.y, v.y, re);
                im = fma(u.x, v.y, im);
                im = fma(-u.y, v.x, im);
            }
        }
    }
    part[s][bl] = make_double2(re, im);
    __syncthreads();
    if (!mine || s != 0) return;
    for (int k = 1; k < gr::kGramSlices; ++k) {
        re += part[k][bl].x;
        im += part[k][bl].y;
    }
    if (a == b) im = 0.0;
    gram[(long)a * n + b] = make_double2(re, im);
    if (a != b) gram[(long)b * n + a] = make_double2(re, -im);
}

// ------------------------------------------------------------------ weights: Newton-Schulz inverse in float64
__device__ __forceinline__ double gw_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// scal[0] = trace(G_ss), scal[1] = tau, scal[2] = trace(G_tt)
__global__ __launch_bounds__(256) void gw_trace_kernel(const double2* __restrict__ G, int n, int ns, double lam, double* __restrict__ scal) {
    __shared__ double sh[256];
    double s = 0.0, t = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double d = G[(long)i * n + i].x;
        if (i < ns) s += d; else t += d;
    }
    s = gw_block_sum(s, sh);
    t = gw_block_sum(t, sh);
    if (threadIdx.x == 0) {
        scal[0] = s;
        scal[1] = lam * s / ns;
        scal[2] = t;
    }
}

// A = G_ss + tau I (ns x ns), B = G_st (ns x nr)
__global__ __launch_bounds__(256) void gw_form_kernel(const double2* __restrict__ G, double2* __restrict__ A, double2* __restrict__ B, int n, int ns,
                                                      const double* __restrict__ scal) {
    const double tau = scal[1];
    const long total = (long)ns * n;
    const int nr = n - ns;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int i = (int)(e / n), j = (int)(e - (long)i * n);
        double2 v = G[e];
        if (j < ns) {
            if (i == j) v.x += tau;
            A[(long)i * ns + j] = v;
        } else {
            B[(long)i * nr + (j - ns)] = v;
        }
    }
}

// part[blockIdx.x] = this workgroup's share of sum |m|^2, elements in a fixed order
__global__ __launch_bounds__(256) void gw_frob_partial_kernel(const double2* __restrict__ m, long total, double* __restrict__ part) {
    __shared__ double sh[256];
    double s = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gr::kParts * 256) {
        const double2 v = m[e];
        s = fma(v.x, v.x, s);
        s = fma(v.y, v.y, s);
    }
    s = gw_block_sum(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// X_0 = I / |A|_F (0 for the zero matrix)
__global__ __launch_bounds__(256) void gw_start_kernel(const double* __restrict__ part, double2* __restrict__ X, int ns) {
    __shared__ double sh[256];
    const double s = gw_block_sum(part[threadIdx.x], sh);
    const double d = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
    const long total = (long)ns * ns;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
        X[e] = make_double2((e / ns) == (e % ns) ? d : 0.0, 0.0);
}

// C = beta D + alpha A B: A (ns x ns), B, D, C (ns x nr).  Thread (row blockIdx.y, column 64 blockIdx.x + tid), k ascending.
__global__ __launch_bounds__(64) void gw_rect_kernel(const double2* __restrict__ A, const double2* __restrict__ B, const double2* __restrict__ D,
                                                     double2* __restrict__ C, int ns, int nr, double alpha, double beta) {
    const int i = blockIdx.y, q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nr) return;
    const double2* arow = A + (long)i * ns;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < ns; ++k) {
        const double2 a = arow[k], b = B[(long)k * nr + q];
        re = fma(a.x, b.x, re);
        re = fma(-a.y, b.y, re);
        im = fma(a.x, b.y, im);
        im = fma(a.y, b.x, im);
    }
    double2 d = make_double2(0.0, 0.0);
    if (beta != 0.0) d = D[(long)i * nr + q];  // beta == 0: D is not read
    C[(long)i * nr + q] = make_double2(beta * d.x + alpha * re, beta * d.y + alpha * im);
}

// part[0][.] sum |Rm|^2, part[1][.] sum |B|^2, part[2][.] sum Re(conj(W) B)
__global__ __launch_bounds__(256) void gw_sums_kernel(const double2* __restrict__ Rm, const double2* __restrict__ B, const double2* __restrict__ W,
                                                      long total, double* __restrict__ part) {
    __shared__ double sh[256];
    double r2 = 0.0, b2 = 0.0, wb = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gr::kParts * 256) {
        const double2 r = Rm[e], b = B[e], w = W[e];
        r2 = fma(r.x, r.x, r2);
        r2 = fma(r.y, r.y, r2);
        b2 = fma(b.x, b.x, b2);
        b2 = fma(b.y, b.y, b2);
        wb = fma(w.x, b.x, wb);
        wb = fma(w.y, b.y, wb);
    }
    r2 = gw_block_sum(r2, sh);
    b2 = gw_block_sum(b2, sh);
    wb = gw_block_sum(wb, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = r2;
        part[gr::kParts + blockIdx.x] = b2;
        part[2 * gr::kParts + blockIdx.x] = wb;
    }
}

__global__ __launch_bounds__(256) void gw_info_kernel(const double* __restrict__ part, const double* __restrict__ scal, double* __restrict__ info) {
    __shared__ double sh[256];
    const double r2 = gw_block_sum(part[threadIdx.x], sh);
    const double b2 = gw_block_sum(part[gr::kParts + threadIdx.x], sh);
    const double wb = gw_block_sum(part[2 * gr::kParts + threadIdx.x], sh);
    if (threadIdx.x != 0) return;
    const double ttr = scal[2];
    const double num = ttr - wb;
    info[0] = b2 > 0.0 ? sqrt(r2 / b2) : (r2 == 0.0 ? 0.0 : r2);      // a NaN residual stays a NaN
    info[1] = scal[1];
    info[2] = ttr > 0.0 ? (num > 0.0 ? sqrt(num / ttr) : (num != num ? num : 0.0)) : 0.0;
    info[3] = scal[0];
}

// weights[m - 1][k][q] = W[k][(m - 1) c + q], rounded once
__global__ __launch_bounds__(256) void gw_round_kernel(const double2* __restrict__ W, float2* __restrict__ weights, int ns, int nr, int c) {
    const long total = (long)ns * nr;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int k = (int)(e / nr), col = (int)(e - (long)k * nr);
        const int m1 = col / c, q = col - m1 * c;
        const double2 v = W[e];
        weights[((long)m1 * ns + k) * c + q] = make_float2((float)v.x, (float)v.y);
    }
}

// ------------------------------------------------------------------ application
struct GrappaApplyArgs {
    const float2* in;
    const float2* weights;
    const uint8_t* mask;
    const int* offsets;
    float2* out;
    int c, h, w, R, ky, kx, ns, nsp, nr, groups;   // nsp: ns rounded up to 4
};

// the acquired rows (and every row of a frame without a lattice) of an out-of-place call, bit for bit
__global__ __launch_bounds__(256) void grappa_copy_kernel(const float2* __restrict__ in, float2* __restrict__ out, const uint8_t* __restrict__ mask,
                                                          const int* __restrict__ offsets, long rows, int c, int h, int w, int R) {
    const long row = blockIdx.x;                 // (frame, coil, y)
    if (row >= rows) return;
    const int y = (int)(row % h);
    const long f = row / h / c;
    const int off = offsets[f];
    if (off >= 0 && off < R && !mask[f * h + y]) return;
    const float2* src = in + row * w;
    float2* dst = out + row * w;
    for (int x = threadIdx.x; x < w; x += 256) dst[x] = src[x];
}

// Workgroup: x-tile blockIdx.x of lattice gap blockIdx.y - 1 of frame blockIdx.z; gap g holds the rows off + g R + m, m = 1 .. R - 1
// (g = -1: the rows above the first lattice row).  All R - 1 target rows come from the ky source rows off + g R - base + j R, staged once:
//   out[x][n = (m - 1) c + q] = sum_k S[x][k] W[k][n],   k = (j, dx, coil),  S[x][k] = in[coil][row_j][x + dx - hx]
// M = TX x-points (16 per wave), K = ns, N = (R - 1) c in `groups` groups of NTG 16-column tiles with accumulators of their own.
// LDS (dynamic): S [ky c][PX] | Bs [KC][PB] float2 | koff [nsp] | noff, nrow, ncoil [groups 16 NTG] ints.
// The A fragment of v_mfma_f32_16x16x4_f32 takes element [x = l & 15][k = 4 q + (l >> 4)] as one 8-byte access at S[koff[k] + x]:
// 16 consecutive x are 16 consecutive 8-byte slots, and two k of a 32-lane group that are neighbouring coils lie PX = 16 (mod 32) slots
// apart, so the group covers 32 distinct slots (a group that straddles the last coil of a tap takes a two-way conflict).  The B fragment
// [k = 4 q + (l >> 4)][n = l & 15] reads Bs[k PB + n] with PB = 16 (mod 32) likewise.  Weights come in chunks of KC k-values, whatever
// ns is: at the upper limits one type is 229 KB.  Per output the k-ordered chain of cine_coil_compress: Cr += Ar Br, Ci += Ar Bi,
// Cr += (-Ai) Bi, Ci += Ai Br, the chunks in ascending k into the same accumulators.
template <int NTG>
__global__ __launch_bounds__(gr::kThreads) void grappa_apply_kernel(GrappaApplyArgs g) {
    using namespace gr;
    constexpr int NCOL = 16 * NTG;
    constexpr int PB = (NCOL % 32 == 16) ? NCOL : NCOL + 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char grappa_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = g.c, h = g.h, w = g.w, R = g.R, ns = g.ns, nsp = g.nsp;
    const long f = blockIdx.z;
    const int off = g.offsets[f];
    if (off < 0 || off >= R) return;             // no lattice: the frame is left alone
    const int y0 = off + ((int)blockIdx.y - 1) * R;
    const uint8_t* mrow = g.mask + f * h;
    bool any = false;
    for (int m = 1; m < R; ++m) {
        const int y = y0 + m;
        any = any || (y >= 0 && y < h && !mrow[y]);
    }
    if (!any) return;                            // uniform: nothing to fill in this gap

    float2* S = reinterpret_cast<float2*>(grappa_lds);
    float2* Bs = S + g.ky * c * PX;
    int* koff = reinterpret_cast<int*>(Bs + KC * PB);
    int* noff = koff + nsp;
    int* nrow = noff + g.groups * NCOL;
    int* ncoil = nrow + g.groups * NCOL;
    const int hx = g.kx / 2, base = (g.ky / 2 - 1) * R;
    const int x0 = blockIdx.x * TX;

    for (int k = tid; k < nsp; k += kThreads) {
        int o = -1;
        if (k < ns) {
            const int tap = k / c, coil = k - tap * c, j = tap / g.kx, dx = tap - j * g.kx;
            o = (j * c + coil) * PX + dx;
        }
        koff[k] = o;
    }
    for (int n = tid; n < g.groups * NCOL; n += kThreads) {
        int o = -1, row = -1, q = 0;
        if (n < g.nr) {
            const int m1 = n / c;
            q = n - m1 * c;
            const int y = y0 + m1 + 1;
            o = m1 * ns * c + q;
            row = (y >= 0 && y < h && !mrow[y]) ? y : -1;
        }
        noff[n] = o;
        nrow[n] = row;
        ncoil[n] = q;
    }
    const float2 zero = make_float2(0.f, 0.f);
    for (int e = tid; e < g.ky * c * PX; e += kThreads) {
        const int rc = e / PX, xx = e - rc * PX;
        const int j = rc / c, coil = rc - j * c;
        const int row = y0 - base + j * R, x = x0 - hx + xx;
        float2 v = zero;
        if (row >= 0 && row < h && x >= 0 && x < w && xx < TX + g.kx - 1) v = g.in[((f * c + coil) * h + row) * w + x];
        S[e] = v;
    }

    const int fc = lane & 15, fr = lane >> 4;
    const bool active = x0 + 16 * wave < w;
    const float2* srow = S + 16 * wave + fc;
    for (int grp = 0; grp < g.groups; ++grp) {
        f32x4 accr[NTG], acci[NTG];
#pragma unroll
        for (int n = 0; n < NTG; ++n) {
            accr[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            acci[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int k0 = 0; k0 < nsp; k0 += KC) {
            const int kc = nsp - k0 < KC ? nsp - k0 : KC;
            __syncthreads();                     // the tables and S are staged; the previous chunk's reads are done
            for (int e = tid; e < kc * NCOL; e += kThreads) {
                const int kk = e / NCOL, n = e - kk * NCOL;
                const int o = noff[grp * NCOL + n], kg = k0 + kk;
                Bs[kk * PB + n] = (o >= 0 && kg < ns) ? g.weights[o + (long)kg * c] : zero;
            }
            __syncthreads();
            if (active) {
                for (int q = 0; q < kc / 4; ++q) {
                    const int kk = 4 * q + fr;
                    const int ko = koff[k0 + kk];
                    const float2 x = ko >= 0 ? srow[ko] : zero;
                    float2 b[NTG];
#pragma unroll
                    for (int n = 0; n < NTG; ++n) b[n] = Bs[kk * PB + 16 * n + fc];
#pragma unroll
                    for (int n = 0; n < NTG; ++n) {
                        accr[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b[n].x, accr[n], 0, 0, 0);
                        acci[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b[n].y, acci[n], 0, 0, 0);
                    }
#pragma unroll
                    for (int n = 0; n < NTG; ++n) {
                        accr[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(-x.y, b[n].y, accr[n], 0, 0, 0);
                        acci[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b[n].x, acci[n], 0, 0, 0);
                    }
                }
            }
        }
        if (!active) continue;
        // lane holds out[x = x0 + 16 wave + 4 fr + r][column 16 n + fc of the group]
#pragma unroll
        for (int n = 0; n < NTG; ++n) {
            const int col = grp * NCOL + 16 * n + fc;
            const int row = nrow[col];
            if (row < 0) continue;               // beyond (R - 1) c, outside the frame, or acquired
            float2* dst = g.out + ((f * c + ncoil[col]) * h + row) * w;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = x0 + 16 * wave + 4 * fr + r;
                if (x < w) dst[x] = make_float2(accr[n][r], acci[n][r]);
            }
        }
    }
}

namespace {

bool gr_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

unsigned gr_blocks(long total) {
    const long b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// workspace of cine_grappa_weights: A, X, T, Xn (ns x ns) | B, W1, Rm, W2 (ns x nr) | 3 kParts partials | 4 scalars
size_t gw_ws_bytes(int ns, int nr) {
    return ((size_t)4 * ns * ns + (size_t)4 * ns * nr) * sizeof(double2) + (size_t)3 * gr::kParts * sizeof(double) + 4 * sizeof(double);
}

int gw_iters(int ns, double lam) {
    const double it = std::ceil(std::log2(std::sqrt((double)ns) * ((double)ns / lam + 1.0))) + 6.0;
    return it < 8.0 ? 8 : (it > (double)gr::kMaxIters ? gr::kMaxIters : (int)it);
}

template <int NTG>
int launch_apply(const GrappaApplyArgs& g, dim3 grid, hipStream_t st) {
    constexpr int NCOL = 16 * NTG;
    constexpr int PB = (NCOL % 32 == 16) ? NCOL : NCOL + 16;
    auto kern = grappa_apply_kernel<NTG>;
    const size_t lds = ((size_t)g.ky * g.c * gr::PX + (size_t)gr::KC * PB) * sizeof(float2) + ((size_t)g.nsp + (size_t)3 * g.groups * NCOL) * sizeof(int);
    if (lds >= 64 * 1024) {
        static std::once_flag once[64];
        static hipError_t status[64];
        if (int e = large_lds_opt_in(reinterpret_cast<const void*>(kern), "cine_grappa_apply", once, status)) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(gr::kThreads), lds, st, g);
    return check_launch("grappa_apply_kernel");
}

}  // namespace
}  // namespace cine

using namespace cine;

extern "C" int cine_grappa_offsets(const uint8_t* mask, int* offsets, int* status, int t, int h, int R, void* stream) {
    CINE_REQUIRE(mask && offsets && status && offsets != status, CINE_EINVAL, "cine_grappa_offsets: null or aliased pointers");
    CINE_REQUIRE(t >= 1 && h >= 1, CINE_EINVAL, "cine_grappa_offsets: Invalid shapes. (frames %d, rows %d)", t, h);
    CINE_REQUIRE(R >= 2 && R <= 8, CINE_EINVAL, "cine_grappa_offsets: acceleration %d, 2 .. 8 are supported", R);
    CINE_REQUIRE(gr_aligned(offsets, 4) && gr_aligned(status, 4), CINE_EINVAL, "cine_grappa_offsets: offsets and status must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(grappa_offsets_kernel, dim3((unsigned)t), dim3(64), 0, st, mask, offsets, status, h, R);
    return check_launch("grappa_offsets_kernel");
}

extern "C" size_t cine_grappa_gram_ws_bytes(int c, int hc, int w, int R, int ky, int kx) {
    GrappaGeom q;
    if (!grappa_geom(c, R, ky, kx, q) || hc < q.span || w < kx) return 0;
    return (size_t)hc * w * c * sizeof(double2);
}

extern "C" int cine_grappa_gram(const float* cal, double* gram, void* ws, size_t ws_bytes, int c, int hc, int w, int R, int ky, int kx,
                                void* stream) {
    CINE_REQUIRE(cal && gram && ws && (const void*)cal != (const void*)gram && (const void*)cal != (const void*)ws &&
                     (const void*)gram != (const void*)ws,
                 CINE_EINVAL, "cine_grappa_gram: null or aliased pointers");
    CINE_REQUIRE(c >= 1 && hc >= 1 && w >= 1, CINE_EINVAL, "cine_grappa_gram: Invalid shapes. (coils %d, rows %d, columns %d)", c, hc, w);
    CINE_REQUIRE(R >= 2 && R <= 8 && (ky == 2 || ky == 4) && (kx == 3 || kx == 5 || kx == 7), CINE_EINVAL,
                 "cine_grappa_gram: acceleration %d (2 .. 8), kernel %d x %d (2 or 4 rows, 3, 5 or 7 columns)", R, ky, kx);
    CINE_REQUIRE(c <= gr::kMaxCoils, CINE_EUNSUPPORTED, "cine_grappa_gram: %d coils, at most %d", c, gr::kMaxCoils);
    GrappaGeom q;
    CINE_REQUIRE(grappa_geom(c, R, ky, kx, q), CINE_EUNSUPPORTED, "cine_grappa_gram: n_aug = %d x %d x %d coils + %d x %d coils = %d, at most %d",
                 ky, kx, c, R - 1, c, ky * kx * c + (R - 1) * c, gr::kMaxAug);
    CINE_REQUIRE(hc >= q.span && w >= kx, CINE_EINVAL, "cine_grappa_gram: the %d x %d calibration array is smaller than the %d x %d window", hc, w,
                 q.span, kx);
    CINE_REQUIRE((long)hc * w <= (1L << 31) / (16 * gr::kMaxCoils), CINE_EUNSUPPORTED, "cine_grappa_gram: %d x %d calibration samples, at most 2^22", hc,
                 w);
    CINE_REQUIRE(gr_aligned(gram, 16) && gr_aligned(ws, 16) && gr_aligned(cal, 8), CINE_EINVAL,
                 "cine_grappa_gram: gram and ws must be 16-byte aligned, cal 8-byte aligned");
    const size_t need = cine_grappa_gram_ws_bytes(c, hc, w, R, ky, kx);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "cine_grappa_gram: workspace %zu bytes, needs %zu", ws_bytes, need);

    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    double2* stage = static_cast<double2*>(ws);
    hipLaunchKernelGGL(grappa_cal_stage_kernel, dim3(gr_blocks((long)hc * w * c)), dim3(256), 0, st, reinterpret_cast<const float2*>(cal), stage, c,
                       hc, w);
    if (int e = check_launch("grappa_cal_stage_kernel")) return e;
    const int n = q.n_aug;
    hipLaunchKernelGGL(grappa_gram_kernel, dim3((unsigned)ceil_div(n, 32), (unsigned)n), dim3(256), 0, st, (const double2*)stage,
                       reinterpret_cast<double2*>(gram), c, hc, w, R, ky, kx, q.ns, n);
    return check_launch("grappa_gram_kernel");
}

extern "C" size_t cine_grappa_weights_ws_bytes(int c, int R, int ky, int kx) {
    GrappaGeom q;
    if (!grappa_geom(c, R, ky, kx, q)) return 0;
    return gw_ws_bytes(q.ns, q.nr);
}

extern "C" int cine_grappa_weights(const double* gram, float* weights, double* info, void* ws, size_t ws_bytes, int c, int R, int ky, int kx,
                                   double lam, void* stream) {
    CINE_REQUIRE(gram && weights && info && ws, CINE_EINVAL, "cine_grappa_weights: null pointer");
    CINE_REQUIRE((const void*)gram != ws && (const void*)weights != ws && (const void*)info != ws && (const void*)gram != (const void*)weights &&
                     (const void*)gram != (const void*)info && (const void*)weights != (const void*)info,
                 CINE_EINVAL, "cine_grappa_weights: aliased pointers");
    CINE_REQUIRE(c >= 1, CINE_EINVAL, "cine_grappa_weights: Invalid shapes. (coils %d)", c);
    CINE_REQUIRE(R >= 2 && R <= 8 && (ky == 2 || ky == 4) && (kx == 3 || kx == 5 || kx == 7), CINE_EINVAL,
                 "cine_grappa_weights: acceleration %d (2 .. 8), kernel %d x %d (2 or 4 rows, 3, 5 or 7 columns)", R, ky, kx);
    CINE_REQUIRE(lam > 0.0 && std::isfinite(lam), CINE_EINVAL, "cine_grappa_weights: lam = %g, must be positive and finite", lam);
    CINE_REQUIRE(c <= gr::kMaxCoils, CINE_EUNSUPPORTED, "cine_grappa_weights: %d coils, at most %d", c, gr::kMaxCoils);
    GrappaGeom q;
    CINE_REQUIRE(grappa_geom(c, R, ky, kx, q), CINE_EUNSUPPORTED,
                 "cine_grappa_weights: n_aug = %d x %d x %d coils + %d x %d coils = %d, at most %d", ky, kx, c, R - 1, c,
                 ky * kx * c + (R - 1) * c, gr::kMaxAug);
    CINE_REQUIRE(gr_aligned(gram, 16) && gr_aligned(ws, 16) && gr_aligned(weights, 8) && gr_aligned(info, 8), CINE_EINVAL,
                 "cine_grappa_weights: gram and ws must be 16-byte aligned, weights and info 8-byte aligned");
    const size_t need = gw_ws_bytes(q.ns, q.nr);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "cine_grappa_weights: workspace %zu bytes, needs %zu", ws_bytes, need);

    hipStream_t st = as_stream(stream);
    const int ns = q.ns, nr = q.nr, n = q.n_aug;
    const size_t sq = (size_t)ns * ns, rc = (size_t)ns * nr;
    double2* A = static_cast<double2*>(ws);
    double2 *X = A + sq, *T = X + sq, *Xn = T + sq;
    double2 *B = Xn + sq, *W1 = B + rc, *Rm = W1 + rc, *W2 = Rm + rc;
    double* part = reinterpret_cast<double*>(W2 + rc);
    double* scal = part + 3 * gr::kParts;
    const double2* G = reinterpret_cast<const double2*>(gram);

    hipLaunchKernelGGL(gw_trace_kernel, dim3(1), dim3(256), 0, st, G, n, ns, lam, scal);
    if (int e = check_launch("gw_trace_kernel")) return e;
    hipLaunchKernelGGL(gw_form_kernel, dim3(gr_blocks((long)ns * n)), dim3(256), 0, st, G, A, B, n, ns, (const double*)scal);
    if (int e = check_launch("gw_form_kernel")) return e;
    hipLaunchKernelGGL(gw_frob_partial_kernel, dim3(gr::kParts), dim3(256), 0, st, (const double2*)A, (long)sq, part);
    if (int e = check_launch("gw_frob_partial_kernel")) return e;
    hipLaunchKernelGGL(gw_start_kernel, dim3(gr_blocks((long)sq)), dim3(256), 0, st, (const double*)part, X, ns);
    if (int e = check_launch("gw_start_kernel")) return e;
    const int iters = gw_iters(ns, lam);
    for (int it = 0; it < iters; ++it) {         // T = A X;  X' = 2 X - X T
        if (int e = cine_zgemm_f64(reinterpret_cast<const double*>(A), reinterpret_cast<const double*>(X), nullptr, reinterpret_cast<double*>(T), ns,
                                   1.0, 0.0, 0.0, 0.0, stream))
            return e;
        if (int e = cine_zgemm_f64(reinterpret_cast<const double*>(X), reinterpret_cast<const double*>(T), reinterpret_cast<const double*>(X),
                                   reinterpret_cast<double*>(Xn), ns, -1.0, 0.0, 2.0, 0.0, stream))
            return e;
        double2* s = X;
        X = Xn;
        Xn = s;
    }
    const dim3 rgrid((unsigned)ceil_div(nr, 64), (unsigned)ns);
    auto rect = [&](const double2* a, const double2* b, const double2* d, double2* cc, double alpha, double beta) {
        hipLaunchKernelGGL(gw_rect_kernel, rgrid, dim3(64), 0, st, a, b, d, cc, ns, nr, alpha, beta);
        return check_launch("gw_rect_kernel");
    };
    if (int e = rect(X, B, B, W1, 1.0, 0.0)) return e;        // W1 = X B
    if (int e = rect(A, W1, B, Rm, -1.0, 1.0)) return e;      // Rm = B - A W1
    if (int e = rect(X, Rm, W1, W2, 1.0, 1.0)) return e;      // W2 = W1 + X Rm
    if (int e = rect(A, W2, B, Rm, -1.0, 1.0)) return e;      // Rm = B - A W2, the residual of what is handed out
    hipLaunchKernelGGL(gw_sums_kernel, dim3(gr::kParts), dim3(256), 0, st, (const double2*)Rm, (const double2*)B, (const double2*)W2, (long)rc, part);
    if (int e = check_launch("gw_sums_kernel")) return e;
    hipLaunchKernelGGL(gw_info_kernel, dim3(1), dim3(256), 0, st, (const double*)part, (const double*)scal, info);
    if (int e = check_launch("gw_info_kernel")) return e;
    hipLaunchKernelGGL(gw_round_kernel, dim3(gr_blocks((long)rc)), dim3(256), 0, st, (const double2*)W2, reinterpret_cast<float2*>(weights), ns, nr, c);
    return check_launch("gw_round_kernel");
}

extern "C" int cine_grappa_apply(const float* in, const float* weights, const uint8_t* mask, const int* offsets, float* out, int t, int c, int h,
                                 int w, int R, int ky, int kx, void* stream) {
    CINE_REQUIRE(in && weights && mask && offsets && out, CINE_EINVAL, "cine_grappa_apply: null pointer");
    CINE_REQUIRE(t >= 1 && c >= 1 && h >= 1 && w >= 1, CINE_EINVAL, "cine_grappa_apply: Invalid shapes. (frames %d, coils %d, %d x %d)", t, c, h, w);
    CINE_REQUIRE(R >= 2 && R <= 8 && (ky == 2 || ky == 4) && (kx == 3 || kx == 5 || kx == 7), CINE_EINVAL,
                 "cine_grappa_apply: acceleration %d (2 .. 8), kernel %d x %d (2 or 4 rows, 3, 5 or 7 columns)", R, ky, kx);
    CINE_REQUIRE(c <= gr::kMaxCoils, CINE_EUNSUPPORTED, "cine_grappa_apply: %d coils, at most %d", c, gr::kMaxCoils);
    GrappaGeom q;
    CINE_REQUIRE(grappa_geom(c, R, ky, kx, q), CINE_EUNSUPPORTED, "cine_grappa_apply: n_aug = %d x %d x %d coils + %d x %d coils = %d, at most %d",
                 ky, kx, c, R - 1, c, ky * kx * c + (R - 1) * c, gr::kMaxAug);
    CINE_REQUIRE(gr_aligned(in, 8) && gr_aligned(out, 8) && gr_aligned(weights, 8) && gr_aligned(offsets, 4), CINE_EINVAL,
                 "cine_grappa_apply: in, out and weights must be 8-byte aligned, offsets 4-byte aligned");
    const int gaps = (h - 1) / R + 2;
    CINE_REQUIRE(t <= 65535 && gaps <= 65535, CINE_EUNSUPPORTED, "cine_grappa_apply: %d frames, %d lattice gaps, at most 65535 each", t, gaps);
    const long rows = (long)t * c * h;
    CINE_REQUIRE(rows <= 2147483647L, CINE_EUNSUPPORTED, "cine_grappa_apply: %ld rows, at most 2^31 - 1", rows);
    const size_t bytes = (size_t)rows * w * sizeof(float2);
    const char *ib = reinterpret_cast<const char*>(in), *ob = reinterpret_cast<const char*>(out);
    CINE_REQUIRE(in == out || ib + bytes <= ob || ob + bytes <= ib, CINE_EINVAL, "cine_grappa_apply: out overlaps in (out == in is the in-place call)");

    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    if (in != out) {
        hipLaunchKernelGGL(grappa_copy_kernel, dim3((unsigned)rows), dim3(256), 0, st, reinterpret_cast<const float2*>(in), reinterpret_cast<float2*>(out),
                           mask, offsets, rows, c, h, w, R);
        if (int e = check_launch("grappa_copy_kernel")) return e;
    }
    GrappaApplyArgs g{};
    g.in = reinterpret_cast<const float2*>(in);
    g.weights = reinterpret_cast<const float2*>(weights);
    g.mask = mask; g.offsets = offsets;
    g.out = reinterpret_cast<float2*>(out);
    g.c = c; g.h = h; g.w = w; g.R = R; g.ky = ky; g.kx = kx;
    g.ns = q.ns; g.nsp = (q.ns + 3) & ~3; g.nr = q.nr;
    // N tiles of 16 in groups of at most 4: the fewest tiles computed, then the fewest groups
    const int nt = ceil_div(q.nr, 16);
    int ntg = 1, best = 1 << 30;
    for (int k = 4; k >= 1; --k) {
        const int padded = ceil_div(nt, k) * k;
        if (padded < best) { best = padded; ntg = k; }
    }
    g.groups = ceil_div(nt, ntg);
    const dim3 grid((unsigned)ceil_div(w, gr::TX), (unsigned)gaps, (unsigned)t);
    switch (ntg) {
        case 1: return launch_apply<1>(g, grid, st);
        case 2: return launch_apply<2>(g, grid, st);
        case 3: return launch_apply<3>(g, grid, st);
        default: return launch_apply<4>(g, grid, st);
    }
}
