// ls_kernels.hip -- low-rank plus sparse (L+S, Otazo et al., MRM 73:1125, 2015): singular-value thresholding of the (h w) x t Casorati
// matrix on the device, the proximal half of an iteration in one launch, and the whole solve.
//
// No reference counterpart.  Per batch element, over L and S (both (t, h, w) complex):
//     minimise  1/2 || M A (L + S) - y ||^2  +  lam_L || C(L) ||_*  +  lam_S || F_t S ||_1
// by proximal gradient from L_0 = zf, S_0 = 0:
//     g = A^H M A (L_k + S_k) - zf                      cine_image_dc_t / cine_image_dc_general, weights (1, 0, -1)
//     L_{k+1} = SVT(L_k - step g, step lam_L)           cine_casorati_gram, cine_svt_weight, then the weight applied in cine_ls_prox
//     S_{k+1} = F_t^H soft(F_t (S_k - step g), step lam_S)
// SVT without an SVD: t <= 64, so with X = C(v), G = X^H X = V diag(lam) V^H (t x t), SVT(X, th) = X W with W = V diag(h(lam)) V^H and
// h(lam) = 1 - th / sqrt(lam) for lam > th^2, else 0 (never a division by a small number).
//   ls_gram_partial_kernel / ls_gram_reduce_kernel   G in float64 from exact float32 products, in an order fixed by the shape (the scheme
//                        of cine_coil_gram): a workgroup stages [t][S] pixels of v = a - step g in LDS as float64 (32 KiB), thread
//                        (entry, pixel slice) sums its slice, a capped number of workgroups leaves one upper-triangle record each.
//   ls_svt_kernel        one workgroup per batch element; G and the eigenvector accumulator in LDS in float64 (2 x 16 t^2 bytes: 128 KiB
//                        at t = 64, the large-LDS opt-in above 64 KiB); cyclic Jacobi for a complex Hermitian matrix, round-robin pairs
//                        (the t / 2 rotations of a round are disjoint: column phase, barrier, row phase), bounded sweeps: ls_jacobi in
//                        ls_jacobi.h, which llr_kernels.hip runs per spatial block.
//   ls_prox_kernel       one workgroup = kLsPix consecutive pixels, all frames: W in LDS, L' = v_L W, then the W region is reused for the
//                        twiddles and the tile for the temporal prox of kt_prox_kernel; 64 KiB of LDS at t = 64, no scratch.
#include "solve.h"
#include "ls_jacobi.h"

namespace cine {

constexpr int kLsPix = 64;                     // prox: pixels per workgroup (one wavefront = one frame / bin of the tile)
constexpr int kLsItems = kLsMaxT * kLsPix / kLsThreads;
constexpr int kLsGramTile = 2048;               // gram: complex128 entries of one staged tile (32 KiB)
constexpr int kLsGramRecords = 256;             // gram: records (workgroups) over the whole batch, unless b itself is larger
constexpr int kLsGramItems = (kLsMaxT * (kLsMaxT + 1) / 2 + kLsThreads - 1) / kLsThreads;     // entries per thread at t = 64

// ------------------------------------------------------------------ Gram matrix of the Casorati matrix
struct LsGramArgs {
    const cf* a; const cf* g; const float* step;
    double2* ws;
    long HW, run;                               // pixels, pixels per workgroup (a multiple of S)
    int T, S, P, nq;                            // S pixels per staged tile, P = T (T + 1) / 2 entries, nq pixel slices per entry
};

__global__ __launch_bounds__(kLsThreads) void ls_gram_partial_kernel(LsGramArgs a) {
    __shared__ double2 tile[kLsGramTile + kLsMaxT];           // [T][S + 1], converted to float64 once
    __shared__ double2 red[kLsThreads];
    const int T = a.T, S = a.S, ld = S + 1, P = a.P, nq = a.nq, tid = threadIdx.x, b = blockIdx.y;
    const int nitems = P * nq;
    const float step = a.g ? *a.step : 0.f;
    int oi[kLsGramItems], oj[kLsGramItems], q0[kLsGramItems];
    double re[kLsGramItems], im[kLsGramItems];
#pragma unroll
    for (int k = 0; k < kLsGramItems; ++k) {
        const int idx = tid + k * kLsThreads;
        oi[k] = oj[k] = q0[k] = 0; re[k] = im[k] = 0.0;
        if (idx < nitems) {
            int i, j;
            ls_pair_of(idx % P, T, i, j);
            oi[k] = i * ld; oj[k] = j * ld; q0[k] = idx / P;
        }
    }
    const long p_begin = (long)blockIdx.x * a.run;
    const long p_end = p_begin + a.run < a.HW ? p_begin + a.run : a.HW;
    for (long p0 = p_begin; p0 < p_end; p0 += S) {
        const int ns = (int)(p_end - p0 < S ? p_end - p0 : S);
        for (int e = tid; e < T * S; e += kLsThreads) {
            const int f = e / S, s = e - f * S;
            if (s < ns) {
                const long q = ((long)b * T + f) * a.HW + p0 + s;
                cf v = a.a[q];
                if (a.g) v = solve_v(v, a.g[q], step);
                tile[f * ld + s] = make_double2((double)v.x, (double)v.y);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kLsGramItems; ++k) {
            if (tid + k * kLsThreads < nitems) {
                const double2* ri = tile + oi[k];
                const double2* rj = tile + oj[k];
                double r = re[k], m = im[k];                  // conj(x) y = (xr yr + xi yi) + i (xr yi - xi yr)
                for (int s = q0[k]; s < ns; s += nq) {
                    const double2 x = ri[s], y = rj[s];
                    r = fma(x.x, y.x, r);
                    r = fma(x.y, y.y, r);
                    m = fma(x.x, y.y, m);
                    m = fma(-x.y, y.x, m);
                }
                re[k] = r; im[k] = m;
            }
        }
        __syncthreads();
    }
    double2* slot = a.ws + ((long)b * gridDim.x + blockIdx.x) * P;
    if (nq == 1) {
#pragma unroll
        for (int k = 0; k < kLsGramItems; ++k) {
            const int idx = tid + k * kLsThreads;
            if (idx < P) slot[idx] = make_double2(re[k], im[k]);
        }
    } else {                                                  // P nq <= 256: the slices of an entry, added in slice order
        if (tid < nitems) red[tid] = make_double2(re[0], im[0]);
        __syncthreads();
        if (tid < P) {
            double r = red[tid].x, m = red[tid].y;
            for (int q = 1; q < nq; ++q) { r += red[q * P + tid].x; m += red[q * P + tid].y; }
            slot[tid] = make_double2(r, m);
        }
    }
}

// 16 entries per workgroup; thread (pl, wl) adds records wl, wl + 16, ... in that order, thread (pl, 0) then adds the 16 sums in wl order
__global__ __launch_bounds__(256) void ls_gram_reduce_kernel(const double2* __restrict__ ws, double2* __restrict__ gram, int t, int P, int nwg) {
    __shared__ double2 part[16][16];
    const int pl = threadIdx.x & 15, wl = threadIdx.x >> 4, b = blockIdx.y;
    const int p = blockIdx.x * 16 + pl;
    double re = 0.0, im = 0.0;
    if (p < P) {
        for (int w = wl; w < nwg; w += 16) {
            const double2 v = ws[((long)b * nwg + w) * P + p];
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
    ls_pair_of(p, t, i, j);
    if (i == j) im = 0.0;
    double2* G = gram + (long)b * t * t;
    G[i * t + j] = make_double2(re, im);
    G[j * t + i] = make_double2(re, -im);
}

struct LsGramPlan { int S, P, nq, nwg; long run; size_t bytes; };

static LsGramPlan ls_gram_plan(int b, int t, int h, int w) {
    LsGramPlan p{};
    const long HW = (long)h * w;
    p.S = kLsGramTile / t;
    p.P = t * (t + 1) / 2;
    p.nq = p.P >= kLsThreads ? 1 : kLsThreads / p.P;
    const long tiles = ceil_div(HW, (long)p.S);
    const long cap = kLsGramRecords / b > 1 ? kLsGramRecords / b : 1;
    const long per = ceil_div(tiles, tiles < cap ? tiles : cap);          // tiles per workgroup
    p.nwg = (int)ceil_div(tiles, per);
    p.run = per * p.S;
    p.bytes = (size_t)b * p.nwg * p.P * sizeof(double2);
    return p;
}

static int ls_sizes(const char* what, int b, int t, int h, int w) {
    return solve_sizes(what, b, t, h, w, kLsMaxT, ceil_div((long)h * w, (long)kLsPix));
}

static int ls_gram_launch(const float* a, const float* g, const float* step_dev, double* gram, int b, int t, int h, int w, void* ws,
                          hipStream_t st) {
    const LsGramPlan p = ls_gram_plan(b, t, h, w);
    LsGramArgs k{};
    k.a = reinterpret_cast<const cf*>(a); k.g = reinterpret_cast<const cf*>(g); k.step = step_dev; k.ws = static_cast<double2*>(ws);
    k.HW = (long)h * w; k.run = p.run; k.T = t; k.S = p.S; k.P = p.P; k.nq = p.nq;
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(ls_gram_partial_kernel, dim3((unsigned)p.nwg, b), dim3(kLsThreads), 0, st, k);
    if (int e = check_launch("ls_gram_partial_kernel")) return e;
    hipLaunchKernelGGL(ls_gram_reduce_kernel, dim3((unsigned)((p.P + 15) / 16), b), dim3(256), 0, st, k.ws, reinterpret_cast<double2*>(gram), t,
                       p.P, p.nwg);
    return check_launch("ls_gram_reduce_kernel");
}

// ------------------------------------------------------------------ the weight W = V diag(h(lam)) V^H by a Jacobi eigensolver
struct LsSvtArgs {
    const double2* gram; const float* thresh; const float* step;
    cf* weight; double* info;
    int T;
};

__global__ __launch_bounds__(kLsThreads) void ls_svt_kernel(LsSvtArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = a.T, tid = threadIdx.x, b = blockIdx.x;
    double2* A = reinterpret_cast<double2*>(smem);            // [T][T]: the matrix, in the end its diagonal = the eigenvalues
    double2* V = A + T * T;                                   // [T][T]: the product of the rotations, columns = eigenvectors
    double* rot = reinterpret_cast<double*>(V + T * T);       // [kLsMaxT / 2][8]: c, s, e^{i phi}, the new diagonal pair, on / off
    double* red = rot + kLsRotDoubles;                        // [2][kLsThreads]
    const double2* G = a.gram + (long)b * T * T;
    for (int e = tid; e < T * T; e += kLsThreads) {
        A[e] = G[e];
        V[e] = make_double2((e / T == e % T) ? 1.0 : 0.0, 0.0);
    }
    __syncthreads();
    double off, diag;
    const int sweeps = ls_jacobi(A, V, rot, red, T, tid, off, diag);
    // h(lam) per eigenvalue; A's off-diagonal part is dead now and takes conj(V)^T diag(h)
    const float thf = a.step ? *a.step * *a.thresh : *a.thresh;
    const double th = (double)thf;
    double* hk = rot;                                         // [T] h, then [T] sqrt(lam) h
    if (tid < T) {
        const double lam = A[tid * T + tid].x;
        double hv = 0.0, sv = 0.0;
        if (lam > th * th) { const double sq = sqrt(lam); hv = 1.0 - th / sq; sv = sq - th; }
        hk[tid] = hv; hk[kLsMaxT + tid] = sv; hk[2 * kLsMaxT + tid] = lam;
    }
    __syncthreads();
    if (tid == 0) {
        double lmax = hk[2 * kLsMaxT], nuc = 0.0;
        for (int k = 0; k < T; ++k) { lmax = ls_nanmax(lmax, hk[2 * kLsMaxT + k]); nuc += hk[kLsMaxT + k]; }
        double* o = a.info + (long)b * 4;
        o[0] = lmax > 0.0 ? sqrt(lmax) : (lmax != lmax ? lmax : 0.0);
        o[1] = nuc;
        o[2] = diag > 0.0 ? off / diag : off;
        o[3] = (double)sweeps;
    }
    for (int e = tid; e < T * T; e += kLsThreads) {           // U[k][j] = h_k conj(V[j][k])
        const int k = e / T, j = e - k * T;
        const double2 v = V[j * T + k];
        A[e] = make_double2(hk[k] * v.x, -hk[k] * v.y);
    }
    __syncthreads();
    cf* W = a.weight + (long)b * T * T;
    for (int e = tid; e < T * T; e += kLsThreads) {           // W[i][j] = sum_k V[i][k] U[k][j], the upper triangle, mirrored
        const int i = e / T, j = e - i * T;
        if (j < i) continue;
        double re = 0.0, im = 0.0;
        for (int k = 0; k < T; ++k) {
            const double2 x = V[i * T + k], y = A[k * T + j];
            re += x.x * y.x - x.y * y.y;
            im += x.x * y.y + x.y * y.x;
        }
        if (i == j) im = 0.0;
        W[i * T + j] = mk((float)re, (float)im);
        W[j * T + i] = mk((float)re, -(float)im);
    }
}

static size_t ls_svt_lds(int t) { return (size_t)2 * t * t * sizeof(double2) + ((kLsMaxT / 2) * 8 + 2 * kLsThreads) * sizeof(double); }

// before the first launch of a call: the opt-in of the weight kernel for this t
static int ls_svt_prepare(int t) {
    static std::once_flag once[64];
    static hipError_t status[64];
    return ls_svt_lds(t) >= 64 * 1024 ? large_lds_opt_in(reinterpret_cast<const void*>(ls_svt_kernel), "ls_svt_kernel", once, status) : CINE_OK;
}

static int ls_svt_launch(const double* gram, const float* thresh_dev, const float* step_dev, float* weight, double* info, int b, int t,
                         hipStream_t st) {
    LsSvtArgs k{};
    k.gram = reinterpret_cast<const double2*>(gram); k.thresh = thresh_dev; k.step = step_dev; k.weight = reinterpret_cast<cf*>(weight);
    k.info = info; k.T = t;
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(ls_svt_kernel, dim3(b), dim3(kLsThreads), ls_svt_lds(t), st, k);
    return check_launch("ls_svt_kernel");
}

// ------------------------------------------------------------------ the proximal half of an iteration
struct LsProxArgs {
    const cf* l; const cf* s; const cf* g; const cf* weight;
    const float* step; const float* thresh;
    cf* lnew; cf* snew; cf* xsum;
    float* part;                                // 4 floats per workgroup, or NULL
    int T;
    long HW;
};

__global__ __launch_bounds__(kLsThreads) void ls_prox_kernel(LsProxArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    cf* buf = reinterpret_cast<cf*>(smem);          // [T][kLsPix]
    cf* wl = buf + a.T * kLsPix;                    // [T][T]: W; after the low-rank half [T] twiddles and the 12 floats of the reduction
    const int T = a.T, tid = threadIdx.x;
    const int b = blockIdx.y;
    const long HW = a.HW;
    const long p0 = (long)blockIdx.x * kLsPix;
    const int np = (int)min((long)kLsPix, HW - p0);
    const int total = T * kLsPix;
    const float step = *a.step;
    const float theta = step * *a.thresh;
    for (int e = tid; e < T * T; e += kLsThreads) wl[e] = a.weight[(long)b * T * T + e];
    for (int e = tid; e < total; e += kLsThreads) {
        const int t = e / kLsPix, p = e - t * kLsPix;
        cf v = mk(0.f, 0.f);
        if (p < np) {
            const long q = ((long)b * T + t) * HW + p0 + p;
            v = solve_v(a.l[q], a.g[q], step);
        }
        buf[e] = v;
    }
    __syncthreads();
    // L' [i] = sum_t v[t] W[t][i] per (pixel, frame); the frame is one per wavefront, so W is read as a broadcast
    cf lacc[kLsItems];
#pragma unroll
    for (int j = 0; j < kLsItems; ++j) {
        const int e = tid + j * kLsThreads;
        lacc[j] = mk(0.f, 0.f);
        if (e < total) {
            const int i = e / kLsPix, p = e - i * kLsPix;
            float ax = 0.f, ay = 0.f;
            for (int t = 0; t < T; ++t) {
                const cf w = wl[t * T + i];
                const cf x = buf[t * kLsPix + p];
                ax += x.x * w.x - x.y * w.y; ay += x.x * w.y + x.y * w.x;
            }
            lacc[j] = mk(ax, ay);
        }
    }
    __syncthreads();
    // A DELIBERATE COPY: from here on this is temporal_twiddles, temporal_dft_fwd + soft_threshold, temporal_dft_inv and block_record of
    // solve.h written out -- a change there has to be made here as well.  With the helpers the outputs keep their bits, but the
    // compiler schedules this 16-fold unrolled kernel differently (9558 instead of 9721 instructions, 119 instead of 118 VGPRs) and
    // tools/ls_rate.py measured 50 iterations at 12.137 / 12.102 ms against 12.054 / 12.078 ms (row mask) and 15.029 / 14.989 ms against
    // 14.959 / 14.932 ms (plane mask), parent - new - parent - new on one card: 0.4 % slower, outside the parent's own spread.
    cf* tw = wl;                                    // [T]: exp(-2 pi i j / T) / sqrt(T)
    float* red = reinterpret_cast<float*>(wl + T);  // [3][kLsThreads / 64]
    {
        const double s = 1.0 / sqrt((double)T);
        for (int j = tid; j < T; j += kLsThreads) {
            double sn, cs;
            sincospi(2.0 * (double)j / (double)T, &sn, &cs);
            tw[j] = mk((float)(cs * s), (float)(-sn * s));
        }
    }
    for (int e = tid; e < total; e += kLsThreads) {
        const int t = e / kLsPix, p = e - t * kLsPix;
        cf v = mk(0.f, 0.f);
        if (p < np) {
            const long q = ((long)b * T + t) * HW + p0 + p;
            v = solve_v(a.s ? a.s[q] : mk(0.f, 0.f), a.g[q], step);           // s == NULL (the solve's first iteration): S = 0
        }
        buf[e] = v;
    }
    __syncthreads();
    const int s_in = (T + 1) / 2, s_out = T / 2;
    // centered forward DFT per (pixel, bin) and the soft threshold; the results wait in registers until every thread has read the tile
    cf coef[kLsItems];
    float s_l1 = 0.f;
#pragma unroll
    for (int j = 0; j < kLsItems; ++j) {
        const int e = tid + j * kLsThreads;
        coef[j] = mk(0.f, 0.f);
        if (e < total) {
            const int i = e / kLsPix, p = e - i * kLsPix;
            int k = i - s_out; if (k < 0) k += T;
            float ax = 0.f, ay = 0.f;
            int idx = (s_in * k) % T;
            for (int g = 0; g < T; ++g) {
                const cf w = tw[idx];
                const cf x = buf[g * kLsPix + p];
                ax += x.x * w.x - x.y * w.y; ay += x.x * w.y + x.y * w.x;
                idx += k; if (idx >= T) idx -= T;
            }
            const float mag = sqrtf(ax * ax + ay * ay);
            const float sc = mag > theta ? (mag - theta) / mag : 0.f;
            coef[j] = mk(ax * sc, ay * sc);
            s_l1 += mag > theta ? mag - theta : 0.f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kLsItems; ++j) {
        const int e = tid + j * kLsThreads;
        if (e < total) buf[e] = coef[j];
    }
    __syncthreads();
    // centered inverse DFT per (pixel, frame), the sum, stores with the pixel on the lanes
    float s_dx = 0.f, s_x2 = 0.f;
#pragma unroll
    for (int j = 0; j < kLsItems; ++j) {
        const int e = tid + j * kLsThreads;
        if (e >= total) continue;
        const int i = e / kLsPix, p = e - i * kLsPix;
        if (p >= np) continue;
        int k = i - s_out; if (k < 0) k += T;
        float ax = 0.f, ay = 0.f;
        int idx = (s_in * k) % T;
        for (int g = 0; g < T; ++g) {
            const cf w = tw[idx];
            const cf x = buf[g * kLsPix + p];
            ax += x.x * w.x + x.y * w.y; ay += x.y * w.x - x.x * w.y;         // x * conj(w)
            idx += k; if (idx >= T) idx -= T;
        }
        const long q = ((long)b * T + i) * HW + p0 + p;
        const cf lo = a.l[q], so = a.s ? a.s[q] : mk(0.f, 0.f);
        const float xx = lacc[j].x + ax, xy = lacc[j].y + ay;
        const float dx = xx - (lo.x + so.x), dy = xy - (lo.y + so.y);
        a.lnew[q] = lacc[j];
        a.snew[q] = mk(ax, ay);
        a.xsum[q] = mk(xx, xy);
        s_dx += dx * dx + dy * dy;
        s_x2 += xx * xx + xy * xy;
    }
    if (a.part) {                                   // one record per workgroup; solve_record_kernel adds them in a fixed order
        const float v0 = wave_sum(s_dx), v1 = wave_sum(s_x2), v2 = wave_sum(s_l1);
        if ((tid & 63) == 0) { red[tid >> 6] = v0; red[4 + (tid >> 6)] = v1; red[8 + (tid >> 6)] = v2; }
        __syncthreads();
        if (tid == 0) {
            float r[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) r[q] = (red[4 * q] + red[4 * q + 1]) + (red[4 * q + 2] + red[4 * q + 3]);
            float* o = a.part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = 0.f;
        }
    }
}

static long ls_blocks(int b, int h, int w) { return ceil_div((long)h * w, (long)kLsPix) * b; }

static size_t ls_prox_lds(int t) {
    const size_t region = (size_t)t * t > (size_t)t + 6 ? (size_t)t * t : (size_t)t + 6;
    return ((size_t)t * kLsPix + region) * sizeof(cf);
}

static int ls_prox_prepare(int t) {
    static std::once_flag once[64];
    static hipError_t status[64];
    return ls_prox_lds(t) >= 64 * 1024 ? large_lds_opt_in(reinterpret_cast<const void*>(ls_prox_kernel), "ls_prox_kernel", once, status) : CINE_OK;
}

static int ls_prox_launch(const float* l, const float* s, const float* g, const float* weight, const float* step_dev, const float* thresh_dev,
                          float* lnew, float* snew, float* xsum, float* part, int b, int t, int h, int w, hipStream_t st) {
    LsProxArgs a{};
    a.l = reinterpret_cast<const cf*>(l); a.s = reinterpret_cast<const cf*>(s); a.g = reinterpret_cast<const cf*>(g);
    a.weight = reinterpret_cast<const cf*>(weight); a.step = step_dev; a.thresh = thresh_dev;
    a.lnew = reinterpret_cast<cf*>(lnew); a.snew = reinterpret_cast<cf*>(snew); a.xsum = reinterpret_cast<cf*>(xsum);
    a.part = part; a.T = t; a.HW = (long)h * w;
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(ls_prox_kernel, dim3((unsigned)ceil_div(a.HW, (long)kLsPix), b), dim3(kLsThreads), ls_prox_lds(t), st, a);
    return check_launch("ls_prox_kernel");
}

// workspace of the solve:
// [operator scratch | g | L | S | gram | gram records | weight | iters rows of info | iters rows of per-workgroup records]
struct LsSolveWs { size_t op_bytes, total; void* op; float* g; float* L; float* S; double* gram; void* gram_ws; float* weight; double* info; float* part; };

static LsSolveWs ls_solve_ws(void* ws, int b, int t, int c, int h, int w, int mask_w, int iters) {
    LsSolveWs y{};
    WsCursor at{static_cast<unsigned char*>(ws)};
    const size_t img = (size_t)b * t * h * w * sizeof(cf);
    y.op_bytes = dc_ws_bytes(mask_w, b, t, c, h, w);
    y.op = y.op_bytes ? at.take<void>(y.op_bytes) : nullptr;
    y.g = at.take<float>(img);
    y.L = at.take<float>(img);
    y.S = at.take<float>(img);
    y.gram = at.take<double>((size_t)b * t * t * sizeof(double2));
    y.gram_ws = at.take<void>(cine_casorati_gram_ws_bytes(b, t, h, w));
    y.weight = at.take<float>((size_t)b * t * t * sizeof(cf));
    y.info = at.take<double>((size_t)iters * b * 4 * sizeof(double));
    y.part = at.take<float>((size_t)iters * cine_ls_prox_ws_bytes(b, t, h, w));
    y.total = at.end;
    return y;
}

}  // namespace cine

using namespace cine;

extern "C" int cine_casorati_gram_pixels(int t) { return t >= 2 && t <= kLsMaxT ? kLsGramTile / t : 0; }

extern "C" size_t cine_casorati_gram_ws_bytes(int b, int t, int h, int w) {
    if (b <= 0 || t < 2 || t > kLsMaxT || h <= 0 || w <= 0 || b > 65535) return 0;
    return ls_gram_plan(b, t, h, w).bytes;
}

extern "C" int cine_casorati_gram(const float* a, const float* g, const float* step_dev, double* gram, int b, int t, int h, int w,
                                  void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_casorati_gram";
    CINE_REQUIRE(a && gram && ws && (!g || step_dev), CINE_EINVAL, "%s: null pointer", what);
    if (int e = ls_sizes(what, b, t, h, w)) return e;
    {
        const void* const outs[] = {gram};
        const void* const ins[] = {a, g, step_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, ws) && (const void*)a != (const void*)step_dev, CINE_EINVAL,
                     "%s: gram and ws must not alias an operand or each other", what);
    }
    CINE_REQUIRE(solve_aligned16(gram) && solve_aligned16(ws), CINE_EINVAL, "%s: gram and ws must be 16-byte aligned", what);
    const size_t need = cine_casorati_gram_ws_bytes(b, t, h, w);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    return ls_gram_launch(a, g, step_dev, gram, b, t, h, w, ws, as_stream(stream));
}

extern "C" int cine_svt_weight(const double* gram, const float* thresh_dev, const float* step_dev, float* weight, double* info, int b, int t,
                               void* stream) {
    const char* what = "cine_svt_weight";
    CINE_REQUIRE(gram && thresh_dev && weight && info, CINE_EINVAL, "%s: null pointer", what);
    if (int e = ls_sizes(what, b, t, 1, 1)) return e;
    {
        const void* const outs[] = {weight, info};
        const void* const ins[] = {gram, thresh_dev, step_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, nullptr), CINE_EINVAL, "%s: weight and info must not alias an operand or each other", what);
    }
    CINE_REQUIRE(solve_aligned16(gram) && (reinterpret_cast<uintptr_t>(info) & 7u) == 0, CINE_EINVAL,
                 "%s: gram must be 16-byte aligned and info 8-byte aligned", what);
    if (int e = ls_svt_prepare(t)) return e;
    return ls_svt_launch(gram, thresh_dev, step_dev, weight, info, b, t, as_stream(stream));
}

extern "C" int cine_ls_prox_pixels(void) { return kLsPix; }

extern "C" size_t cine_ls_prox_ws_bytes(int b, int t, int h, int w) {
    if (b <= 0 || t <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)ls_blocks(b, h, w) * 4 * sizeof(float);
}

extern "C" int cine_ls_prox(const float* l, const float* s, const float* g, const float* weight, const float* step_dev,
                            const float* thresh_s_dev, float* lnew, float* snew, float* xsum, float* rec,
                            int b, int t, int h, int w, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_ls_prox";
    CINE_REQUIRE(l && s && g && weight && step_dev && thresh_s_dev && lnew && snew && xsum && (!rec || ws), CINE_EINVAL, "%s: null pointer", what);
    if (int e = ls_sizes(what, b, t, h, w)) return e;
    {
        // an output may be the operand it replaces (lnew: l, snew: s) and nothing else
        const float* ins[6] = {l, s, g, weight, step_dev, thresh_s_dev};
        bool ok = lnew != snew && lnew != xsum && snew != xsum;
        for (int i = 0; i < 6; ++i) {
            ok = ok && (lnew != ins[i] || i == 0) && (snew != ins[i] || i == 1) && xsum != ins[i];
        }
        CINE_REQUIRE(ok, CINE_EINVAL, "%s: only lnew == l and snew == s may alias", what);
    }
    if (rec) {
        const void* const outs[] = {rec};
        const void* const ins[] = {l, s, g, weight, step_dev, thresh_s_dev, lnew, snew, xsum};
        CINE_REQUIRE(solve_no_alias(outs, ins, ws), CINE_EINVAL, "%s: rec and ws must not alias an operand or each other", what);
        const size_t need = cine_ls_prox_ws_bytes(b, t, h, w);
        CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    }
    if (int e = ls_prox_prepare(t)) return e;
    hipStream_t st = as_stream(stream);
    float* part = rec ? reinterpret_cast<float*>(ws) : nullptr;
    if (int e = ls_prox_launch(l, s, g, weight, step_dev, thresh_s_dev, lnew, snew, xsum, part, b, t, h, w, st)) return e;
    return rec ? solve_record_launch(part, ls_blocks(b, h, w), rec, 1, st) : CINE_OK;
}

extern "C" size_t cine_ls_solve_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int iters) {
    if (b <= 0 || t < 2 || t > kLsMaxT || c <= 0 || h <= 0 || w <= 0 || iters <= 0 || b > 65535) return 0;
    return ls_solve_ws(nullptr, b, t, c, h, w, mask_w, iters).total;
}

extern "C" int cine_ls_solve(float* x, float* l_out, float* s_out, const float* zf, const float* sens, const float* sens_tiled,
                             const uint8_t* mask, int mask_w, const float* step_dev, const float* thresh_l_dev, const float* thresh_s_dev,
                             int iters, float* rec, double* resid, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_ls_solve";
    CINE_REQUIRE(x && zf && sens && mask && step_dev && thresh_l_dev && thresh_s_dev && ws, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(!resid || rec, CINE_EINVAL, "%s: resid comes with rec", what);
    CINE_REQUIRE(c > 0 && iters >= 1, CINE_EINVAL, "%s: bad sizes", what);
    if (int e = ls_sizes(what, b, t, h, w)) return e;
    CINE_REQUIRE(mask_w == 1 || mask_w == w, CINE_EINVAL, "%s: mask_w %d is neither 1 (row mask) nor w", what, mask_w);
    {
        const void* const outs[] = {x, l_out, s_out, rec, resid};
        const void* const ins[] = {zf, sens, sens_tiled, mask, step_dev, thresh_l_dev, thresh_s_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, ws), CINE_EINVAL, "%s: x, l, s, rec, resid and ws must not alias an operand or each other", what);
    }
    CINE_REQUIRE(solve_aligned16(ws), CINE_EINVAL, "%s: ws must be 16-byte aligned", what);
    CINE_REQUIRE(!resid || (reinterpret_cast<uintptr_t>(resid) & 7u) == 0, CINE_EINVAL, "%s: resid must be 8-byte aligned", what);
    const size_t need = cine_ls_solve_ws_bytes(b, t, c, h, w, mask_w, iters);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    const LsSolveWs y = ls_solve_ws(ws, b, t, c, h, w, mask_w, iters);
    if (int e = ls_svt_prepare(t)) return e;
    if (int e = ls_prox_prepare(t)) return e;
    float* L = l_out ? l_out : y.L;
    float* S = s_out ? s_out : y.S;
    const long nblk = ls_blocks(b, h, w);
    hipStream_t st = as_stream(stream);
    for (int k = 0; k < iters; ++k) {
        const float* xk = k == 0 ? zf : x;          // L_0 + S_0 = zf without a copy
        const float* lk = k == 0 ? zf : L;          // and S_0 = 0 without a buffer of zeros: the prox kernel takes s == NULL
        if (int e = solve_gradient(what, xk, zf, sens, sens_tiled, mask, mask_w, y.g, b, t, c, h, w, y.op, y.op_bytes, stream)) return e;
        if (int e = ls_gram_launch(lk, y.g, step_dev, y.gram, b, t, h, w, y.gram_ws, st)) return e;
        if (int e = ls_svt_launch(y.gram, thresh_l_dev, step_dev, y.weight, y.info + (size_t)k * b * 4, b, t, st)) return e;
        if (int e = ls_prox_launch(lk, k == 0 ? nullptr : S, y.g, y.weight, step_dev, thresh_s_dev, L, S, x,
                                   rec ? y.part + (size_t)k * nblk * 4 : nullptr, b, t, h, w, st))
            return e;
    }
    return rec ? solve_record_launch(y.part, nblk, rec, iters, st, y.info, b, resid) : CINE_OK;
}
