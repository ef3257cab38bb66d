// coil_kernels.hip -- SVD coil compression in front of the data front-end (Buehrer et al., MRM 57:1131, 2007; Huang et al., MRI 26:133,
// 2008): the c physical coils of raw k-space (t_in, nx, ny, c) -- the HDF5 `y` layout, the coil axis at unit stride -- are projected onto
// V virtual coils.  The reference has no such step (its loader takes whatever coil count the file holds).
//
//   cine_coil_gram       G[i][j] = sum_{t < t_use} sum_{(x, y) in R} raw[t, x, y, i] conj(raw[t, x, y, j])      c x c, complex128
//                        R = the central rx x ry block, rx = min(region, nx), x0 = nx / 2 - rx / 2 (region 0: the whole matrix).
//                        Every product of two floats is exact in float64; the sums run in float64 in an order that depends on the
//                        shape only: workgroup w sums samples [w run, (w + 1) run) in sample order (coil_gram_partial_kernel, the
//                        upper triangle, one slot of the workspace per workgroup), coil_gram_reduce_kernel adds the slots in a
//                        fixed order and writes the full Hermitian matrix.  No atomics: repeated calls are bit-identical.
//   cine_coil_compress   out[t, x, y, v] = sum_k A[v][k] raw[t, x, y, k], t < t_out: a skinny complex GEMM (M = t_out nx ny samples,
//                        K = c, N = V) on v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered fmaf chain per output as in
//                        raw_window_gemm_kernel: Cr += Ar Br - Ai Bi, Ci += Ar Bi + Ai Br).  The samples of a tile are one
//                        contiguous run of raw and of out, so both move with 16-byte accesses whatever c and V are; all of K is
//                        resident in LDS, A is staged once per workgroup, one pass over the samples; the next tile's loads are
//                        issued into registers before the current tile's MFMAs, so they overlap its compute and stores.
//   cine_coil_matrix     the step between the two: G = U diag(lam) U^H, A[r] = conj(U[:, rank r]) times the unit phase that makes its
//                        largest entry real and positive, r < V.  One workgroup per Gram matrix, G and U in LDS in float64, the cyclic
//                        Jacobi eigensolver of the singular-value-thresholding kernels (ls_jacobi in ls_jacobi.h, unchanged).  Only the
//                        upper triangle of G is read (mirrored, the diagonal's imaginary part dropped): Hermitian by construction, so
//                        no check on the host.  No host read, no atomics: capturable, repeated calls are bit-identical.
//   cine_coil_matrix_whitened
//                        noise pre-whitening folded into that matrix: with the lower-triangular whitener W = s L^-1 of the noise
//                        covariance Psi = L L^H (one per scan, computed by the caller) the same kernel decomposes G' = W G W^H =
//                        U diag(lam) U^H and writes A = U^H W, phased like the rows above: A Psi A^H = s^2 I, A G A^H = diag(lam).
//                        Three more c^3 float64 products in the same LDS, W read from global memory (its lower triangle only);
//                        cine_coil_compress then whitens and compresses in its one pass over the samples.
#include <cstdint>
#include <mutex>
#include "common.h"
#include "conv_src.h"
#include "ls_jacobi.h"
#include "solve.h"                   // large_lds_opt_in

namespace cine {

namespace cc {
constexpr int kMaxCoils = 128, kMaxVirtual = 32;
constexpr int kThreads = 256;
constexpr int TS = 64;                        // compress: samples per tile (16 per wave)
constexpr int kTilesPerWg = 8;                // compress: tiles per workgroup at most (A is staged once for all of them)
constexpr int kGramTile = 2048;               // gram: complex128 entries of one staged sample tile (32 KB)
constexpr int kGramMaxPartials = 1024;
constexpr size_t kGramWsBudget = 64u << 20;   // gram: the partial sums stay below this many bytes
}

// ------------------------------------------------------------------ Gram matrix
struct GramArgs {
    long N, run;                               // samples in the region, samples per workgroup
    int nx, ny, c, rx, ry, x0, y0, S, P;       // S samples per staged tile, P = c (c + 1) / 2 upper-triangle entries
};

__device__ __forceinline__ int gram_row_start(int i, int c) { return i * c - i * (i - 1) / 2; }

// entry p of the row-major upper triangle -> (i, j), i <= j
__device__ __forceinline__ void gram_pair(int p, int c, int& i, int& j) {
    const float b = 2.f * c + 1.f;
    int r = (int)((b - sqrtf(fmaxf(b * b - 8.f * p, 0.f))) * 0.5f);
    r = r < 0 ? 0 : (r > c - 1 ? c - 1 : r);
    while (r > 0 && gram_row_start(r, c) > p) --r;
    while (r + 1 < c && gram_row_start(r + 1, c) <= p) ++r;
    i = r;
    j = r + (p - gram_row_start(r, c));
}

__global__ __launch_bounds__(cc::kThreads) void coil_gram_partial_kernel(const float2* __restrict__ raw, double2* __restrict__ ws, GramArgs g) {
    __shared__ double2 tile[cc::kGramTile];      // [sample][coil], converted to float64 once
    __shared__ long offs[64];                    // element offset of each staged sample
    const int tid = threadIdx.x, c = g.c;
    const long n_begin = (long)blockIdx.x * g.run;
    const long n_end = n_begin + g.run < g.N ? n_begin + g.run : g.N;
    double2* slot = ws + (long)blockIdx.x * g.P;
    bool first = true;
    for (long n0 = n_begin; n0 < n_end; n0 += g.S) {
        const int ns = (int)(n_end - n0 < g.S ? n_end - n0 : g.S);
        if (tid < ns) {
            const long n = n0 + tid;
            const long r = n / g.ry;
            const int yy = (int)(n - r * g.ry), xx = (int)(r % g.rx);
            const long t = r / g.rx;
            offs[tid] = ((t * g.nx + g.x0 + xx) * g.ny + g.y0 + yy) * c;
        }
        __syncthreads();
        if ((c & 1) == 0) {                      // a sample starts on a 16-byte boundary: two coils per load
            const int half = c >> 1;
            for (int e = tid; e < ns * half; e += cc::kThreads) {
                const int s = e / half, k = 2 * (e - s * half);
                const float4 v = *reinterpret_cast<const float4*>(raw + offs[s] + k);
                tile[s * c + k] = make_double2((double)v.x, (double)v.y);
                tile[s * c + k + 1] = make_double2((double)v.z, (double)v.w);
            }
        } else {
            for (int e = tid; e < ns * c; e += cc::kThreads) {
                const int s = e / c, k = e - s * c;
                const float2 v = raw[offs[s] + k];
                tile[s * c + k] = make_double2((double)v.x, (double)v.y);
            }
        }
        __syncthreads();
        for (int p = tid; p < g.P; p += cc::kThreads) {
            int i, j;
            gram_pair(p, c, i, j);
            double re = 0.0, im = 0.0;           // a conj(b) = (ar br + ai bi) + i (ai br - ar bi)
            for (int s = 0; s < ns; ++s) {
                const double2 a = tile[s * c + i], b = tile[s * c + j];
                re = fma(a.x, b.x, re);
                re = fma(a.y, b.y, re);
                im = fma(a.y, b.x, im);
                im = fma(-a.x, b.y, im);
            }
            if (!first) {                        // this thread's own entry of this workgroup's own slot
                const double2 prev = slot[p];
                re += prev.x;
                im += prev.y;
            }
            slot[p] = make_double2(re, im);
        }
        first = false;
        __syncthreads();
    }
}

// 16 entries per workgroup; thread (pl, wl) adds slots wl, wl + 16, ... in that order, thread (pl, 0) then adds the 16 sums in wl order
__global__ __launch_bounds__(256) void coil_gram_reduce_kernel(const double2* __restrict__ ws, double2* __restrict__ gram, int c, int P, int nwg) {
    __shared__ double2 part[16][16];
    const int pl = threadIdx.x & 15, wl = threadIdx.x >> 4;
    const int p = blockIdx.x * 16 + pl;
    double re = 0.0, im = 0.0;
    if (p < P) {
#pragma unroll 4
        for (int w = wl; w < nwg; w += 16) {
            const double2 v = ws[(long)w * P + p];
            re += v.x;
            im += v.y;
        }
    }
    part[wl][pl] = make_double2(re, im);
    __syncthreads();
    if (wl != 0 || p >= P) return;
    for (int w = 1; w < 16; ++w) {
        re += part[w][pl].x;
        im += part[w][pl].y;
    }
    int i, j;
    gram_pair(p, c, i, j);
    if (i == j) im = 0.0;
    gram[(long)i * c + j] = make_double2(re, im);
    gram[(long)j * c + i] = make_double2(re, -im);
}

// ------------------------------------------------------------------ compression
struct CompressArgs {
    long M;                                    // samples
    long tiles;                                // ceil(M / TS)
    int c, v, ldc, tiles_per_wg;               // ldc: LDS row in complex elements (>= c rounded up to 4, = 2 mod 4)
};

// LDS (dynamic): Am [16 NCT][ldc] | X [TS][ldc] | O [TS v], float2 each.  A fragment read takes element [l & 15][4 q + (l >> 4)] as one
// 8-byte access: with ldc = 2 (mod 4) the 16 rows of a 32-lane group start on 16 different 4-bank slots and its two k on the two
// halves of a slot, so the read is conflict-free.  Columns c .. ldc of Am and X, and rows v .. 16 NCT of Am, stay zero.
// QMAX: 16-byte pieces of a tile per thread, TS c / (2 kThreads) rounded up.
template <int NCT, int QMAX>
__global__ __launch_bounds__(cc::kThreads) void coil_compress_kernel(const float2* __restrict__ raw, const float2* __restrict__ mat,
                                                                      float2* __restrict__ out, CompressArgs g) {
    using namespace cc;
    extern __shared__ __attribute__((aligned(16))) float2 cc_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = g.c, V = g.v, ldc = g.ldc;
    float2* Am = cc_lds;
    float2* X = Am + 16 * NCT * ldc;
    float2* O = X + TS * ldc;                    // (16 NCT + TS) ldc is even: O is 16-byte aligned

    for (int e = tid; e < (16 * NCT + TS) * ldc; e += kThreads) cc_lds[e] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int e = tid; e < V * c; e += kThreads) {
        const int r = e / c, k = e - r * c;
        Am[r * ldc + k] = mat[e];
    }

    // the walk of this thread over a tile's flat (sample, coil) elements, two per 16-byte load, 2 * kThreads apart
    const int s_init = (2 * tid) / c, k_init = 2 * tid - s_init * c;
    const int ds = (2 * kThreads) / c, dk = 2 * kThreads - ds * c;

    const int fr = lane >> 4, fc = lane & 15;
    const int nkq = (c + 3) >> 2;
    const long tile_end = (long)(blockIdx.x + 1) * g.tiles_per_wg < g.tiles ? (long)(blockIdx.x + 1) * g.tiles_per_wg : g.tiles;
    long tile = (long)blockIdx.x * g.tiles_per_wg;

    // a tile's 16-byte pieces of this thread, loaded one tile ahead: the next tile's loads fly during this tile's MFMAs and stores
    float4 pre[QMAX];
    auto fetch = [&](long tl) {
        const long s0 = tl * TS;
        const int nq = ((int)(g.M - s0 < TS ? g.M - s0 : TS) * c) >> 1;
        const float4* src4 = reinterpret_cast<const float4*>(raw + s0 * c);
#pragma unroll
        for (int j = 0; j < QMAX; ++j) {
            const int q = tid + j * kThreads;
            if (q < nq) pre[j] = src4[q];
        }
    };
    fetch(tile);
    for (; tile < tile_end; ++tile) {
        const long s0 = tile * TS;
        const int ns = (int)(g.M - s0 < TS ? g.M - s0 : TS);
        const float2* src = raw + s0 * c;
        const int ne = ns * c, nq = ne >> 1;
        {
            int s = s_init, k = k_init;
#pragma unroll
            for (int j = 0; j < QMAX; ++j) {
                if (tid + j * kThreads < nq) {
                    const float4 v = pre[j];
                    X[s * ldc + k] = make_float2(v.x, v.y);
                    const bool wrap = k + 1 == c;
                    X[(wrap ? s + 1 : s) * ldc + (wrap ? 0 : k + 1)] = make_float2(v.z, v.w);
                    k += dk; s += ds;
                    if (k >= c) { k -= c; ++s; }
                }
            }
            if ((ne & 1) && tid == 0) X[(ns - 1) * ldc + c - 1] = src[ne - 1];
        }
        __syncthreads();                         // X (and, the first time, Am) is staged; the previous tile's O has been copied out
        if (tile + 1 < tile_end) fetch(tile + 1);

        if (16 * wave < ns) {
            f32x4 accr[NCT], acci[NCT];
#pragma unroll
            for (int n = 0; n < NCT; ++n) {
                accr[n] = f32x4{0.f, 0.f, 0.f, 0.f};
                acci[n] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float2* xrow = X + (16 * wave + fc) * ldc + fr;
            const float2* arow = Am + fc * ldc + fr;
            for (int q = 0; q < nkq; ++q) {
                const float2 x = xrow[4 * q];
                float2 a[NCT];
#pragma unroll
                for (int n = 0; n < NCT; ++n) a[n] = arow[16 * n * ldc + 4 * q];
#pragma unroll
                for (int n = 0; n < NCT; ++n) {
                    accr[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, a[n].x, accr[n], 0, 0, 0);
                    acci[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, a[n].y, acci[n], 0, 0, 0);
                }
#pragma unroll
                for (int n = 0; n < NCT; ++n) {
                    accr[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(-x.y, a[n].y, accr[n], 0, 0, 0);
                    acci[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, a[n].x, acci[n], 0, 0, 0);
                }
            }
            // lane holds out[sample 16 wave + 4 fr + r][virtual coil 16 n + fc]
#pragma unroll
            for (int n = 0; n < NCT; ++n) {
                const int vc = 16 * n + fc;
                if (vc < V) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) O[(16 * wave + 4 * fr + r) * V + vc] = make_float2(accr[n][r], acci[n][r]);
                }
            }
        }
        __syncthreads();                         // O is complete; every wave is done with X

        float2* dst = out + s0 * V;
        const int no = ns * V, nqo = no >> 1;
        for (int q = tid; q < nqo; q += kThreads) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(O)[q];
        if ((no & 1) && tid == 0) dst[no - 1] = O[no - 1];
    }
}

// ------------------------------------------------------------------ compression matrix from the Gram matrix
struct CoilMatrixArgs {
    const double2* gram;
    const double2* whitener;                   // coil_matrix_kernel<true> only
    float2* matrix;
    double* lam;
    double* info;
    int c, v;
};

// the order of the eigenvalues: descending, a NaN in front of every number (a total order, so the ranks are a permutation whatever the
// input holds), equal values by column index
__device__ __forceinline__ bool cm_before(double a, int ia, double b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an != bn) return an;
    if (!an && a != b) return a > b;
    return ia < ib;
}

// entry [i][k], k <= i, of the lower-triangular whitener: the diagonal's imaginary part is taken as 0
__device__ __forceinline__ double2 cm_whitener(const double2* __restrict__ W, int T, int i, int k) {
    double2 w = W[i * T + k];
    if (i == k) w.y = 0.0;
    return w;
}

// LDS (dynamic): A [c][c] | U [c][c] double2, rot [kLsRotDoubles], red [kLsRedDoubles] doubles.  After ls_jacobi red is reused:
// [c] eigenvalues in rank order, then [c] ints, the column of every rank.
// kWhiten: the eigen-decomposition is that of G' = W G W^H, W the lower-triangular whitener (read from global memory: c x c doubles
// shared by every workgroup stay in L2), within the same two slots: B = W G into U, G' = B W^H back into A (the upper triangle,
// mirrored: exactly Hermitian with a real diagonal), then U = W^H in place of the identity.  ls_jacobi multiplies U by its rotations
// from the right, so U ends as W^H U' and the extraction below writes conj((W^H U')[:, r]) = the rows of U'^H W.  With W = I every
// product is one with 1 or 0 and every sum one with 0: the bits of the plain kernel.
template <bool kWhiten>
__global__ __launch_bounds__(kLsThreads) void coil_matrix_kernel(CoilMatrixArgs a) {
    extern __shared__ __align__(16) unsigned char cm_lds[];
    const int T = a.c, nv = a.v, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    double2* A = reinterpret_cast<double2*>(cm_lds);
    double2* U = A + T * T;
    double* rot = reinterpret_cast<double*>(U + T * T);
    double* red = rot + kLsRotDoubles;
    const double2* G = a.gram + b * T * T;
    for (int e = tid; e < T * T; e += kLsThreads) {
        const int i = e / T, j = e - i * T;
        double2 g = i <= j ? G[e] : G[j * T + i];             // the upper triangle only
        g.y = i < j ? g.y : (i == j ? 0.0 : -g.y);
        A[e] = g;
        if constexpr (!kWhiten) U[e] = make_double2(i == j ? 1.0 : 0.0, 0.0);
    }
    __syncthreads();
    if constexpr (kWhiten) {
        const double2* __restrict__ W = a.whitener;
        for (int e = tid; e < T * T; e += kLsThreads) {        // B[i][j] = sum_{k <= i} W[i][k] G[k][j]
            const int i = e / T, j = e - i * T;
            double re = 0.0, im = 0.0;
            for (int k = 0; k <= i; ++k) {
                const double2 w = cm_whitener(W, T, i, k), g = A[k * T + j];
                re = fma(w.x, g.x, re);
                re = fma(-w.y, g.y, re);
                im = fma(w.x, g.y, im);
                im = fma(w.y, g.x, im);
            }
            U[e] = make_double2(re, im);
        }
        __syncthreads();
        for (int e = tid; e < T * T; e += kLsThreads) {        // G'[i][j] = sum_{k <= j} B[i][k] conj(W[j][k]), i <= j, and its mirror
            const int i = e / T, j = e - i * T;
            if (i > j) continue;
            double re = 0.0, im = 0.0;
            for (int k = 0; k <= j; ++k) {
                const double2 b = U[i * T + k], w = cm_whitener(W, T, j, k);
                re = fma(b.x, w.x, re);
                re = fma(b.y, w.y, re);
                im = fma(b.y, w.x, im);
                im = fma(-b.x, w.y, im);
            }
            if (i == j) {
                A[e] = make_double2(re, 0.0);
            } else {
                A[e] = make_double2(re, im);
                A[j * T + i] = make_double2(re, -im);
            }
        }
        __syncthreads();                                       // every thread is done with B
        for (int e = tid; e < T * T; e += kLsThreads) {        // U = W^H
            const int i = e / T, j = e - i * T;
            double2 u = make_double2(0.0, 0.0);
            if (i <= j) {
                const double2 w = cm_whitener(W, T, j, i);
                u = make_double2(w.x, 0.0 - w.y);
            }
            U[e] = u;
        }
        __syncthreads();
    }
    double off, diag;
    const int sweeps = ls_jacobi(A, U, rot, red, T, tid, off, diag);     // ends behind a barrier: rot and red are free
    double* lams = red;
    int* col_of = reinterpret_cast<int*>(red + kLsMaxT);
    if (tid < T) {
        const double l = A[tid * T + tid].x;
        int rank = 0;
        for (int j = 0; j < T; ++j) rank += (j != tid && cm_before(A[j * T + j].x, j, l, tid)) ? 1 : 0;
        lams[rank] = l;
        col_of[rank] = tid;
        a.lam[b * T + rank] = l;
    }
    __syncthreads();
    if (tid == 0) {
        double kept = 0.0, all = 0.0;
        for (int k = 0; k < T; ++k) { all += lams[k]; if (k == nv - 1) kept = all; }
        double* o = a.info + b * 4;
        o[0] = diag > 0.0 ? off / diag : off;
        o[1] = (double)sweeps;
        o[2] = all == 0.0 ? 1.0 : kept / all;
        o[3] = lams[0];
    }
    // one wavefront per row, the coil on the lanes (c <= 64)
    float2* M = a.matrix + b * nv * T;
    for (int r = wave; r < nv; r += kLsThreads / 64) {
        const int k = col_of[r];
        const double2 u = lane < T ? U[lane * T + k] : make_double2(0.0, 0.0);
        double m = lane < T ? hypot(u.x, u.y) : -1.0;
        int at = lane;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                     // the largest magnitude, the lowest index among equal ones
            const double mo = __shfl_xor(m, o, 64);
            const int ao = __shfl_xor(at, o, 64);
            if (mo > m || (mo == m && ao < at)) { m = mo; at = ao; }
        }
        at = __shfl(at, 0, 64);                                // with a NaN in the row the lanes may disagree: lane 0 decides
        at = at < 0 ? 0 : (at > T - 1 ? T - 1 : at);
        const double2 pk = U[at * T + k];
        const double pm = hypot(pk.x, pk.y);
        const bool ok = pm > 0.0 && pm <= 1.79769313486231570e308;          // a zero or NaN peak does not divide
        const double cx = ok ? pk.x / pm : 1.0, cy = ok ? pk.y / pm : 0.0;    // conj(conj(pk)) / |pk|
        if (lane < T) {
            // conj(u) (cx + i cy)
            float2 w = make_float2((float)(u.x * cx + u.y * cy), (float)(u.x * cy - u.y * cx));
            if (ok && lane == at) w = make_float2((float)pm, 0.f);
            M[r * T + lane] = w;
        }
    }
}

namespace {

struct GramPlan {
    long N, run;
    int rx, ry, x0, y0, S, P, nwg;
    size_t bytes;
};

bool gram_shapes_ok(int t, int nx, int ny, int c, int region) {
    return t >= 1 && nx >= 1 && ny >= 1 && c >= 1 && region >= 0;
}

GramPlan gram_plan(int t, int nx, int ny, int c, int region) {
    GramPlan p{};
    p.rx = region == 0 || region > nx ? nx : region;
    p.ry = region == 0 || region > ny ? ny : region;
    p.x0 = nx / 2 - p.rx / 2;
    p.y0 = ny / 2 - p.ry / 2;
    p.N = (long)t * p.rx * p.ry;
    p.P = c * (c + 1) / 2;
    p.S = cc::kGramTile / c < 64 ? cc::kGramTile / c : 64;
    long maxp = (long)(cc::kGramWsBudget / ((size_t)p.P * sizeof(double2)));
    maxp = maxp < 1 ? 1 : (maxp > cc::kGramMaxPartials ? cc::kGramMaxPartials : maxp);
    const long per = (p.N + maxp - 1) / maxp;
    p.run = (per + p.S - 1) / p.S * p.S;
    p.nwg = (int)((p.N + p.run - 1) / p.run);
    p.bytes = (size_t)p.nwg * p.P * sizeof(double2);
    return p;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int NCT, int QMAX>
int launch_compress(const float2* raw, const float2* mat, float2* out, const CompressArgs& g, hipStream_t st) {
    auto kern = coil_compress_kernel<NCT, QMAX>;
    const size_t lds = ((size_t)(16 * NCT + cc::TS) * g.ldc + (size_t)cc::TS * g.v) * sizeof(float2);
    static std::once_flag once[64];
    static hipError_t status[64];
    if (lds > 64 * 1024) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        CINE_REQUIRE(dev >= 0 && dev < 64, CINE_EUNSUPPORTED, "coil_compress_kernel: device index %d", dev);
        std::call_once(once[dev], [&] {
            status[dev] = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        });
        CINE_REQUIRE(status[dev] == hipSuccess, CINE_EHIP, "coil_compress_kernel: hipFuncSetAttribute: %s", hipGetErrorString(status[dev]));
    }
    CINE_REQUIRE(lds <= 160 * 1024, CINE_EUNSUPPORTED, "coil_compress_kernel: %d coils need %zu bytes of LDS", g.c, lds);
    const long wgs = (g.tiles + g.tiles_per_wg - 1) / g.tiles_per_wg;
    CINE_REQUIRE(wgs <= INT32_MAX, CINE_EUNSUPPORTED, "cine_coil_compress: %ld workgroups exceed the grid limit %d", wgs, INT32_MAX);
    hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(cc::kThreads), lds, st, raw, mat, out, g);
    return check_launch("coil_compress_kernel");
}

}  // namespace
}  // namespace cine

using namespace cine;

extern "C" size_t cine_coil_gram_ws_bytes(int t, int nx, int ny, int c, int region) {
    if (!gram_shapes_ok(t, nx, ny, c, region) || c > cc::kMaxCoils) return 0;
    return gram_plan(t, nx, ny, c, region).bytes;
}

extern "C" int cine_coil_gram(const float* raw, double* gram, void* ws, size_t ws_bytes, int t_in, int nx, int ny, int c, int t_use,
                              int region, void* stream) {
    CINE_REQUIRE(raw && gram && ws && (const void*)raw != (const void*)gram && (const void*)raw != (const void*)ws && (const void*)gram != (const void*)ws,
                 CINE_EINVAL, "cine_coil_gram: null or aliased pointers");
    CINE_REQUIRE(t_in >= 1 && t_use <= t_in && gram_shapes_ok(t_use, nx, ny, c, region), CINE_EINVAL,
                 "cine_coil_gram: Invalid shapes. (t_in %d, nx %d, ny %d, coils %d, t_use %d, region %d)", t_in, nx, ny, c, t_use, region);
    CINE_REQUIRE(c <= cc::kMaxCoils, CINE_EUNSUPPORTED, "cine_coil_gram: %d coils, at most %d", c, cc::kMaxCoils);
    CINE_REQUIRE(aligned16(raw) && aligned16(gram) && aligned16(ws), CINE_EINVAL, "cine_coil_gram: raw, gram and ws must be 16-byte aligned");
    const GramPlan p = gram_plan(t_use, nx, ny, c, region);
    CINE_REQUIRE(ws_bytes >= p.bytes, CINE_EWORKSPACE, "cine_coil_gram: workspace %zu bytes, needs %zu", ws_bytes, p.bytes);

    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    GramArgs g{};
    g.N = p.N; g.run = p.run;
    g.nx = nx; g.ny = ny; g.c = c; g.rx = p.rx; g.ry = p.ry; g.x0 = p.x0; g.y0 = p.y0; g.S = p.S; g.P = p.P;
    double2* w = static_cast<double2*>(ws);
    hipLaunchKernelGGL(coil_gram_partial_kernel, dim3((unsigned)p.nwg), dim3(cc::kThreads), 0, st, reinterpret_cast<const float2*>(raw), w, g);
    if (int e = check_launch("coil_gram_partial_kernel")) return e;
    hipLaunchKernelGGL(coil_gram_reduce_kernel, dim3((unsigned)((p.P + 15) / 16)), dim3(256), 0, st, w, reinterpret_cast<double2*>(gram), c,
                       p.P, p.nwg);
    return check_launch("coil_gram_reduce_kernel");
}

extern "C" int cine_coil_compress(const float* raw, const float* matrix, float* out, int t_in, int nx, int ny, int c, int t_out, int v,
                                  void* stream) {
    CINE_REQUIRE(raw && matrix && out && (const void*)raw != (const void*)out && (const void*)raw != (const void*)matrix &&
                     (const void*)matrix != (const void*)out,
                 CINE_EINVAL, "cine_coil_compress: null or aliased pointers");
    CINE_REQUIRE(t_in >= 1 && nx >= 1 && ny >= 1 && c >= 1 && t_out >= 1 && t_out <= t_in && v >= 1 && v <= c, CINE_EINVAL,
                 "cine_coil_compress: Invalid shapes. (t_in %d, nx %d, ny %d, coils %d, t_out %d, virtual coils %d)", t_in, nx, ny, c, t_out, v);
    CINE_REQUIRE(c <= cc::kMaxCoils, CINE_EUNSUPPORTED, "cine_coil_compress: %d coils, at most %d", c, cc::kMaxCoils);
    CINE_REQUIRE(v <= cc::kMaxVirtual, CINE_EUNSUPPORTED, "cine_coil_compress: %d virtual coils, at most %d", v, cc::kMaxVirtual);
    CINE_REQUIRE(aligned16(raw) && aligned16(out), CINE_EINVAL, "cine_coil_compress: raw and out must be 16-byte aligned");

    CompressArgs g{};
    g.M = (long)t_out * nx * ny;
    g.tiles = (g.M + cc::TS - 1) / cc::TS;
    g.c = c;
    g.v = v;
    g.ldc = (c + 3) / 4 * 4 + 2;
    const long want = g.tiles / 1024;              // a shape-only split: enough workgroups first, then up to kTilesPerWg tiles each
    g.tiles_per_wg = (int)(want < 1 ? 1 : (want > cc::kTilesPerWg ? cc::kTilesPerWg : want));
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    const float2* r = reinterpret_cast<const float2*>(raw);
    const float2* m = reinterpret_cast<const float2*>(matrix);
    float2* o = reinterpret_cast<float2*>(out);
    if (c <= 32) return v <= 16 ? launch_compress<1, 4>(r, m, o, g, st) : launch_compress<2, 4>(r, m, o, g, st);
    if (c <= 64) return v <= 16 ? launch_compress<1, 8>(r, m, o, g, st) : launch_compress<2, 8>(r, m, o, g, st);
    return v <= 16 ? launch_compress<1, 16>(r, m, o, g, st) : launch_compress<2, 16>(r, m, o, g, st);
}

namespace {

// cine_coil_matrix (whitener == nullptr, whitened == false) and cine_coil_matrix_whitened: every check, then the one launch
int coil_matrix_run(const char* what, bool whitened, const double* gram, const double* whitener, float* matrix, double* lam, double* info,
                    int nb, int c, int v, void* stream) {
    CINE_REQUIRE(gram && matrix && lam && info && (whitener || !whitened), CINE_EINVAL, "%s: null pointer", what);
    {
        const void* g = gram; const void* m = matrix; const void* l = lam; const void* f = info; const void* w = whitener;
        CINE_REQUIRE(g != m && g != l && g != f && m != l && m != f && l != f, CINE_EINVAL, "%s: aliased pointers", what);
        CINE_REQUIRE(!whitened || (w != g && w != m && w != l && w != f), CINE_EINVAL, "%s: aliased pointers", what);
    }
    CINE_REQUIRE(nb >= 1 && c >= 1 && v >= 1 && v <= c, CINE_EINVAL, "%s: Invalid shapes. (matrices %d, coils %d, virtual coils %d)", what, nb, c, v);
    CINE_REQUIRE(c <= kLsMaxT, CINE_EUNSUPPORTED, "%s: %d coils, at most %d", what, c, kLsMaxT);
    CINE_REQUIRE(v <= cc::kMaxVirtual, CINE_EUNSUPPORTED, "%s: %d virtual coils, at most %d", what, v, cc::kMaxVirtual);
    const bool outs8 = (reinterpret_cast<uintptr_t>(matrix) & 7u) == 0 && (reinterpret_cast<uintptr_t>(lam) & 7u) == 0 &&
                       (reinterpret_cast<uintptr_t>(info) & 7u) == 0;
    if (whitened)
        CINE_REQUIRE(aligned16(gram) && aligned16(whitener) && outs8, CINE_EINVAL,
                     "%s: gram and whitener must be 16-byte aligned, matrix, lam and info 8-byte aligned", what);
    else
        CINE_REQUIRE(aligned16(gram) && outs8, CINE_EINVAL, "%s: gram must be 16-byte aligned, matrix, lam and info 8-byte aligned", what);
    const size_t lds = (size_t)2 * c * c * sizeof(double2) + (size_t)(kLsRotDoubles + kLsRedDoubles) * sizeof(double);
    auto kern = whitened ? coil_matrix_kernel<true> : coil_matrix_kernel<false>;
    if (lds >= 64 * 1024) {
        static std::once_flag once[2][64];
        static hipError_t status[2][64];
        if (int e = large_lds_opt_in(reinterpret_cast<const void*>(kern), "coil_matrix_kernel", once[whitened], status[whitened])) return e;
    }
    CoilMatrixArgs a{};
    a.gram = reinterpret_cast<const double2*>(gram); a.whitener = reinterpret_cast<const double2*>(whitener);
    a.matrix = reinterpret_cast<float2*>(matrix); a.lam = lam; a.info = info;
    a.c = c; a.v = v;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(kLsThreads), lds, st, a);
    return check_launch("coil_matrix_kernel");
}

}  // namespace

extern "C" int cine_coil_matrix(const double* gram, float* matrix, double* lam, double* info, int nb, int c, int v, void* stream) {
    return coil_matrix_run("cine_coil_matrix", false, gram, nullptr, matrix, lam, info, nb, c, v, stream);
}

extern "C" int cine_coil_matrix_whitened(const double* gram, const double* whitener, float* matrix, double* lam, double* info,
                                         int nb, int c, int v, void* stream) {
    return coil_matrix_run("cine_coil_matrix_whitened", true, gram, whitener, matrix, lam, info, nb, c, v, stream);
}
