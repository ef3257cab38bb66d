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
//   cine_grappa_apply     the hot path: a skinny complex GEMM per lattice gap on v_mfma_f32_16x16x4_f32, see grappa_fill_gap.
//   cine_grappa_gaps      unevenly spaced rows: one workgroup per frame lists the frame's gaps (lower source row, step) in ascending order,
//                         an ordered compaction through an LDS prefix sum, no atomics.
//   cine_grappa_apply_gaps  the hot path of those: the workgroup of cine_grappa_apply, its step and its weights taken from the gap.
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

// N tiles of 16 columns in groups of at most 4 with accumulators of their own: the fewest tiles computed, then the fewest groups
__host__ __device__ inline void grappa_tiling(int nr, int& ntg, int& groups) {
    const int nt = (nr + 15) / 16;
    int best = 1 << 30;
    ntg = 1;
    for (int k = 4; k >= 1; --k) {
        const int padded = (nt + k - 1) / k * k;
        if (padded < best) { best = padded; ntg = k; }
    }
    groups = (nt + ntg - 1) / ntg;
}

// dynamic LDS of one workgroup of grappa_fill_gap<ntg>
__host__ __device__ inline size_t grappa_apply_lds(int ntg, int groups, int ky, int c, int nsp) {
    const int ncol = 16 * ntg, pb = (ncol % 32 == 16) ? ncol : ncol + 16;
    return ((size_t)ky * c * gr::PX + (size_t)gr::KC * pb) * sizeof(float2) + ((size_t)nsp + (size_t)3 * groups * ncol) * sizeof(int);
}

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

// One gap of one frame, what the workgroups of cine_grappa_apply and of cine_grappa_apply_gaps share.
struct GrappaGap {
    const float2* in;                            // the frame (c, h, w)
    const float2* weights;                       // (R - 1, ns, c) of this gap's step
    const uint8_t* mrow;                         // the frame's mask row (h)
    float2* out;                                 // the frame
    int c, h, w, R, ky, kx, ns, nsp, nr, groups; // R: the step of this gap; nsp: ns rounded up to 4
    int y0;                                      // the targets are the rows y0 + m, m = 1 .. R - 1
};

// Workgroup: x-tile blockIdx.x of the gap.  All R - 1 target rows come from the ky source rows y0 - base + j R, staged once:
//   out[x][n = (m - 1) c + q] = sum_k S[x][k] W[k][n],   k = (j, dx, coil),  S[x][k] = in[coil][row_j][x + dx - hx]
// M = TX x-points (16 per wave), K = ns, N = (R - 1) c in `groups` groups of NTG 16-column tiles with accumulators of their own.
// LDS (dynamic): S [ky c][PX] | Bs [KC][PB] float2 | koff [nsp] | noff, nrow, ncoil [groups 16 NTG] ints.
// The A fragment of v_mfma_f32_16x16x4_f32 takes element [x = l & 15][k = 4 q + (l >> 4)] as one 8-byte access at S[koff[k] + x]:
// 16 consecutive x are 16 consecutive 8-byte slots, and two k of a 32-lane group that are neighbouring coils lie PX = 16 (mod 32) slots
// apart, so the group covers 32 distinct slots (a group that straddles the last coil of a tap takes a two-way conflict).  The B fragment
// [k = 4 q + (l >> 4)][n = l & 15] reads Bs[k PB + n] with PB = 16 (mod 32) likewise.  Weights come in chunks of KC k-values, whatever
// ns is: at the upper limits one type is 229 KB.  Per output the k-ordered chain of cine_coil_compress: Cr += Ar Br, Ci += Ar Bi,
// Cr += (-Ai) Bi, Ci += Ai Br, the chunks in ascending k into the same accumulators: the bits of an output depend on its sources and
// its weights alone, not on NTG or on the grouping.
template <int NTG>
__device__ __forceinline__ void grappa_fill_gap(const GrappaGap& g) {
    using namespace gr;
    constexpr int NCOL = 16 * NTG;
    constexpr int PB = (NCOL % 32 == 16) ? NCOL : NCOL + 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char grappa_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = g.c, h = g.h, w = g.w, R = g.R, ns = g.ns, nsp = g.nsp;
    const int y0 = g.y0;
    const uint8_t* mrow = g.mrow;

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
        if (row >= 0 && row < h && x >= 0 && x < w && xx < TX + g.kx - 1) v = g.in[((long)coil * h + row) * w + x];
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
            float2* dst = g.out + ((long)ncoil[col] * h + row) * w;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = x0 + 16 * wave + 4 * fr + r;
                if (x < w) dst[x] = make_float2(accr[n][r], acci[n][r]);
            }
        }
    }
}

// Workgroup: x-tile blockIdx.x of lattice gap blockIdx.y - 1 of frame blockIdx.z; gap g holds the rows off + g R + m, m = 1 .. R - 1
// (g = -1: the rows above the first lattice row), filled from the ky source rows off + g R - base + j R.
template <int NTG>
__global__ __launch_bounds__(gr::kThreads) void grappa_apply_kernel(GrappaApplyArgs g) {
    const int h = g.h, R = g.R;
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
    const long frame = f * g.c * h * g.w;
    GrappaGap q;
    q.in = g.in + frame; q.weights = g.weights; q.mrow = mrow; q.out = g.out + frame;
    q.c = g.c; q.h = h; q.w = g.w; q.R = R; q.ky = g.ky; q.kx = g.kx;
    q.ns = g.ns; q.nsp = g.nsp; q.nr = g.nr; q.groups = g.groups; q.y0 = y0;
    grappa_fill_gap<NTG>(q);
}

// ------------------------------------------------------------------ unevenly spaced rows: the gap table and its application
// Workgroup: frame blockIdx.x.  The acquired rows a_0 < ... < a_{n-1}; row a_i lists the leading end (i = 0), then the gap to a_{i+1} or
// the trailing end (i = n - 1): at most two entries per row, placed by an exclusive prefix sum over the rows in chunks of 256.
__global__ __launch_bounds__(256) void grappa_gaps_kernel(const uint8_t* __restrict__ mask, int* __restrict__ gaps, int* __restrict__ count,
                                                          int* __restrict__ unfilled, int h, int cap, int max_gap, int allowed) {
    __shared__ int sa[256], sb[256], sc[256];
    const int tid = threadIdx.x;
    const long f = blockIdx.x;
    const uint8_t* m = mask + f * h;
    int* tab = gaps + f * cap * 2;
    int first = h, last = -1, n = 0;
    for (int y = tid; y < h; y += 256)
        if (m[y]) {
            first = y < first ? y : first;
            last = y > last ? y : last;
            ++n;
        }
    sa[tid] = first; sb[tid] = last; sc[tid] = n;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            sa[tid] = sa[tid + s] < sa[tid] ? sa[tid + s] : sa[tid];
            sb[tid] = sb[tid + s] > sb[tid] ? sb[tid + s] : sb[tid];
            sc[tid] += sc[tid + s];
        }
        __syncthreads();
    }
    first = sa[0]; last = sb[0]; n = sc[0];
    __syncthreads();
    auto ok = [&](int G) { return G >= 2 && G <= max_gap && ((allowed >> G) & 1); };
    int placed = 0, filled = 0;                  // entries placed so far (uniform); target rows of this thread's entries
    for (int yb = 0; yb < h && n > 0; yb += 256) {
        const int y = yb + tid;
        int ne = 0, elo[2], eg[2];
        if (y < h && m[y]) {
            int d = 0;                           // the distance to the next acquired row, 0: none within max_gap
            for (int k = 1; k <= max_gap && y + k < h; ++k)
                if (m[y + k]) { d = k; break; }
            if (y == first && y > 0) {           // the leading end: n >= 2 and no row within reach is a spacing above max_gap
                int nb = n >= 2 ? (d ? d : max_gap + 1) : 0;
                if (nb < 2) nb = 0;
                const int G = nb > y + 1 ? nb : y + 1;
                if (ok(G)) { elo[ne] = y - G; eg[ne] = G; ++ne; filled += y; }
            }
            if (y != last) {
                if (ok(d)) { elo[ne] = y; eg[ne] = d; ++ne; filled += d - 1; }
            } else if (y < h - 1) {              // the trailing end
                const int e = h - 1 - y;
                int b = 0;
                for (int k = 1; k <= max_gap && y - k >= 0; ++k)
                    if (m[y - k]) { b = k; break; }
                int nb = n >= 2 ? (b ? b : max_gap + 1) : 0;
                if (nb < 2) nb = 0;
                const int G = nb > e + 1 ? nb : e + 1;
                if (ok(G)) { elo[ne] = y; eg[ne] = G; ++ne; filled += e; }
            }
        }
        sa[tid] = ne;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {      // inclusive prefix sum
            const int v = tid >= s ? sa[tid - s] : 0;
            __syncthreads();
            sa[tid] += v;
            __syncthreads();
        }
        int pos = placed + sa[tid] - ne;
        for (int i = 0; i < ne; ++i, ++pos)
            if (pos < cap) { tab[2 * pos] = elo[i]; tab[2 * pos + 1] = eg[i]; }
        placed += sa[255];
        __syncthreads();
    }
    if (placed > cap) placed = cap;              // cannot happen: a gap owns a run of missing rows, and there are at most (h + 1) / 2
    for (int i = placed + tid; i < cap; i += 256) { tab[2 * i] = 0; tab[2 * i + 1] = 0; }
    sc[tid] = filled;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sc[tid] += sc[tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        count[f] = placed;
        unfilled[f] = h - n - sc[0];
    }
}

struct GrappaGapsArgs {
    const float2* in;
    const float2* weights;
    const uint8_t* mask;
    const int* gaps;
    const int* count;
    float2* out;
    int c, h, w, cap, kx, ns, nsp;
    int woff[9];                                 // per step: the offset of its (G - 1, ns, c) block in `weights`, or -1
};

// woff[G] of a step read from the table, -1 for a step outside 2 .. 8 (constant indices: the argument stays in scalar registers)
__device__ __forceinline__ int grappa_gap_woff(const GrappaGapsArgs& a, int G) {
    int o = -1;
#pragma unroll
    for (int k = 2; k <= 8; ++k) o = G == k ? a.woff[k] : o;
    return o;
}

// every row that cine_grappa_apply_gaps does not write, bit for bit: acquired rows, rows of no listed gap, rows of a gap without weights
__global__ __launch_bounds__(256) void grappa_copy_gaps_kernel(GrappaGapsArgs a, long rows) {
    const long row = blockIdx.x;                 // (frame, coil, y)
    if (row >= rows) return;
    const int h = a.h, w = a.w;
    const int y = (int)(row % h);
    const long f = row / h / a.c;
    int target = 0;
    if (!a.mask[f * h + y]) {
        int n = a.count[f];
        n = n < a.cap ? n : a.cap;
        const int* tab = a.gaps + f * a.cap * 2;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int lo = tab[2 * i], G = tab[2 * i + 1];
            if (grappa_gap_woff(a, G) >= 0 && y > lo && y < lo + G) target = 1;
        }
    }
    if (__syncthreads_or(target)) return;
    const float2* src = a.in + row * w;
    float2* dst = a.out + row * w;
    for (int x = threadIdx.x; x < w; x += 256) dst[x] = src[x];
}

// Workgroup: x-tile blockIdx.x of gap blockIdx.y of frame blockIdx.z.  The step G, and with it N = (G - 1) c, the tile grouping, the
// skip tables and the LDS layout, are the gap's; the launch sizes the LDS for the largest step that has weights.
__global__ __launch_bounds__(gr::kThreads) void grappa_apply_gaps_kernel(GrappaGapsArgs a) {
    const long f = blockIdx.z;
    const int gi = blockIdx.y;
    if (gi >= a.count[f]) return;                // uniform, before anything is staged
    const int* entry = a.gaps + (f * a.cap + gi) * 2;
    const int lo = entry[0], G = entry[1];
    const int wo = grappa_gap_woff(a, G);
    if (wo < 0 || lo <= -G || lo >= a.h) return; // no weights for this step, or a gap outside the frame: left alone
    const long frame = f * a.c * a.h * a.w;
    GrappaGap q;
    q.in = a.in + frame; q.weights = a.weights + wo; q.mrow = a.mask + f * a.h; q.out = a.out + frame;
    q.c = a.c; q.h = a.h; q.w = a.w; q.R = G; q.ky = 2; q.kx = a.kx;
    q.ns = a.ns; q.nsp = a.nsp; q.nr = (G - 1) * a.c; q.y0 = lo;
    int ntg;
    grappa_tiling(q.nr, ntg, q.groups);
    switch (ntg) {
        case 1: grappa_fill_gap<1>(q); break;
        case 2: grappa_fill_gap<2>(q); break;
        case 3: grappa_fill_gap<3>(q); break;
        default: grappa_fill_gap<4>(q); break;
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
    auto kern = grappa_apply_kernel<NTG>;
    const size_t lds = grappa_apply_lds(NTG, g.groups, g.ky, g.c, g.nsp);
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
    int ntg;
    grappa_tiling(q.nr, ntg, g.groups);
    const dim3 grid((unsigned)ceil_div(w, gr::TX), (unsigned)gaps, (unsigned)t);
    switch (ntg) {
        case 1: return launch_apply<1>(g, grid, st);
        case 2: return launch_apply<2>(g, grid, st);
        case 3: return launch_apply<3>(g, grid, st);
        default: return launch_apply<4>(g, grid, st);
    }
}

extern "C" int cine_grappa_gaps_cap(int h) { return h < 1 ? 0 : h / 2 + 1; }

extern "C" int cine_grappa_gaps(const uint8_t* mask, int* gaps, int* count, int* unfilled, int t, int h, int max_gap, int allowed_bits,
                                void* stream) {
    CINE_REQUIRE(mask && gaps && count && unfilled && gaps != count && gaps != unfilled && count != unfilled, CINE_EINVAL,
                 "cine_grappa_gaps: null or aliased pointers");
    CINE_REQUIRE(t >= 1 && h >= 1, CINE_EINVAL, "cine_grappa_gaps: Invalid shapes. (frames %d, rows %d)", t, h);
    CINE_REQUIRE(max_gap >= 2 && max_gap <= 8, CINE_EINVAL, "cine_grappa_gaps: max_gap %d, 2 .. 8 are supported", max_gap);
    CINE_REQUIRE((allowed_bits & ~0x1FC) == 0, CINE_EINVAL, "cine_grappa_gaps: allowed_bits 0x%x, bit G stands for the step G in 2 .. 8", allowed_bits);
    CINE_REQUIRE(gr_aligned(gaps, 4) && gr_aligned(count, 4) && gr_aligned(unfilled, 4), CINE_EINVAL,
                 "cine_grappa_gaps: gaps, count and unfilled must be 4-byte aligned");
    CINE_REQUIRE(h <= (1 << 20), CINE_EUNSUPPORTED, "cine_grappa_gaps: %d rows, at most 2^20", h);
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(grappa_gaps_kernel, dim3((unsigned)t), dim3(256), 0, st, mask, gaps, count, unfilled, h, cine_grappa_gaps_cap(h), max_gap,
                       allowed_bits);
    return check_launch("grappa_gaps_kernel");
}

extern "C" int cine_grappa_apply_gaps(const float* in, const float* weights, const int* woff, const uint8_t* mask, const int* gaps, const int* count,
                                      float* out, int t, int c, int h, int w, int cap, int kx, void* stream) {
    CINE_REQUIRE(in && weights && woff && mask && gaps && count && out, CINE_EINVAL, "cine_grappa_apply_gaps: null pointer");
    CINE_REQUIRE(t >= 1 && c >= 1 && h >= 1 && w >= 1 && cap >= 1, CINE_EINVAL,
                 "cine_grappa_apply_gaps: Invalid shapes. (frames %d, coils %d, %d x %d, %d table entries per frame)", t, c, h, w, cap);
    CINE_REQUIRE(kx == 3 || kx == 5 || kx == 7, CINE_EINVAL,
                 "cine_grappa_apply_gaps: kernel 2 x %d (3, 5 or 7 columns; two source rows, the neighbours of the gap, is all there is)", kx);
    CINE_REQUIRE(c <= gr::kMaxCoils, CINE_EUNSUPPORTED, "cine_grappa_apply_gaps: %d coils, at most %d", c, gr::kMaxCoils);
    int g_max = 0;
    for (int G = 2; G <= 8; ++G) {
        CINE_REQUIRE(woff[G] >= -1, CINE_EINVAL, "cine_grappa_apply_gaps: woff[%d] = %d, an offset in complex elements or -1", G, woff[G]);
        if (woff[G] >= 0) g_max = G;
    }
    CINE_REQUIRE(g_max >= 2, CINE_EINVAL, "cine_grappa_apply_gaps: woff names no step 2 .. 8 with weights");
    GrappaGeom q;
    CINE_REQUIRE(grappa_geom(c, g_max, 2, kx, q), CINE_EUNSUPPORTED,
                 "cine_grappa_apply_gaps: n_aug = 2 x %d x %d coils + %d x %d coils = %d, at most %d", kx, c, g_max - 1, c,
                 2 * kx * c + (g_max - 1) * c, gr::kMaxAug);
    CINE_REQUIRE(gr_aligned(in, 8) && gr_aligned(out, 8) && gr_aligned(weights, 8) && gr_aligned(gaps, 4) && gr_aligned(count, 4), CINE_EINVAL,
                 "cine_grappa_apply_gaps: in, out and weights must be 8-byte aligned, gaps and count 4-byte aligned");
    CINE_REQUIRE(t <= 65535 && cap <= 65535, CINE_EUNSUPPORTED, "cine_grappa_apply_gaps: %d frames, %d table entries per frame, at most 65535 each", t,
                 cap);
    const long rows = (long)t * c * h;
    CINE_REQUIRE(rows <= 2147483647L, CINE_EUNSUPPORTED, "cine_grappa_apply_gaps: %ld rows, at most 2^31 - 1", rows);
    const size_t bytes = (size_t)rows * w * sizeof(float2);
    const char *ib = reinterpret_cast<const char*>(in), *ob = reinterpret_cast<const char*>(out);
    CINE_REQUIRE(in == out || ib + bytes <= ob || ob + bytes <= ib, CINE_EINVAL,
                 "cine_grappa_apply_gaps: out overlaps in (out == in is the in-place call)");

    GrappaGapsArgs a{};
    a.in = reinterpret_cast<const float2*>(in);
    a.weights = reinterpret_cast<const float2*>(weights);
    a.mask = mask; a.gaps = gaps; a.count = count;
    a.out = reinterpret_cast<float2*>(out);
    a.c = c; a.h = h; a.w = w; a.cap = cap; a.kx = kx;
    a.ns = q.ns; a.nsp = (q.ns + 3) & ~3;
    size_t lds = 0;                              // of the largest layout among the steps that have weights
    for (int G = 0; G <= 8; ++G) {
        a.woff[G] = G >= 2 ? woff[G] : -1;
        if (a.woff[G] < 0) continue;
        int ntg, groups;
        grappa_tiling((G - 1) * c, ntg, groups);
        const size_t need = grappa_apply_lds(ntg, groups, 2, c, a.nsp);
        lds = need > lds ? need : lds;
    }
    auto kern = grappa_apply_gaps_kernel;
    if (lds >= 64 * 1024) {
        static std::once_flag once[64];
        static hipError_t status[64];
        if (int e = large_lds_opt_in(reinterpret_cast<const void*>(kern), "cine_grappa_apply_gaps", once, status)) return e;
    }
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    if (in != out) {
        hipLaunchKernelGGL(grappa_copy_gaps_kernel, dim3((unsigned)rows), dim3(256), 0, st, a, rows);
        if (int e = check_launch("grappa_copy_gaps_kernel")) return e;
    }
    const dim3 grid((unsigned)ceil_div(w, gr::TX), (unsigned)cap, (unsigned)t);
    hipLaunchKernelGGL(kern, grid, dim3(gr::kThreads), lds, st, a);
    return check_launch("grappa_apply_gaps_kernel");
}
