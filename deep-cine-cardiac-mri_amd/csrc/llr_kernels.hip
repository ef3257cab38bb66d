// llr_kernels.hip -- locally low-rank regularisation (LLR; Trzasko & Manduca 2011, Zhang et al. 2015): singular-value thresholding of
// every small spatial block of the Casorati matrix in ONE launch, and the whole solve.
//
// No reference counterpart.  Per batch element, over x ((t, h, w) complex):
//     minimise  1/2 || M A x - y ||^2  +  lam sum over the blocks beta of P of || C_beta(x) ||_*
// with P a partition into block x block squares whose grid origin lies at (-shift_h, -shift_w), clipped to the image, by proximal
// gradient from x_0 = zf with the shift changing per iteration:
//     g = A^H M A x_k - zf                              cine_image_dc_t / cine_image_dc_general, weights (1, 0, -1)
//     x_{k+1} = BlockSVT_{P_k}(x_k - step g, step lam)  cine_llr_prox
// Block SVT by the route of ls_kernels.hip (X = C_beta(v), G = X^H X = V diag(lam) V^H, SVT(X, th) = X W, W = V diag(h(lam)) V^H), but
// with a t x t problem per block instead of one per image, so hundreds of workgroups run their eigensolvers side by side:
//   llr_prox_kernel    one workgroup per (block, batch element).  The block's pixels are staged [t][S] in LDS as float32, S pixels at a
//                      time; thread (entry, pixel slice) adds exact float32 products in float64 into the upper triangle of G (registers);
//                      G and the identity go to LDS, ls_jacobi (ls_jacobi.h) diagonalises; h(lam), then W through registers into the dead
//                      matrix storage as float32; xnew = v W per (pixel, frame) from the staged tile -- still there when the block fits in
//                      one tile, staged again from global memory (L2-hot) tile by tile otherwise.  A tile is read completely before any of
//                      its pixels is written and tiles do not share pixels, so xnew may be x.
//                      LDS: 32 t^2 (G and V) + 6 KiB (rotations, reductions) + 8 t (S + 1) (tile); see llr_plan.
//   llr_record_kernel  one 64-byte record per workgroup behind a header that holds their number -> rec and info, in float64 in a fixed order.
#include "solve.h"
#include "ls_jacobi.h"

namespace cine {

static_assert(kLsThreads == kSolveThreads, "block_sums is written for the workgroup of the Jacobi kernels");
constexpr int kLlrMinBlock = 2, kLlrMaxBlock = 16;
constexpr int kLlrGramItems = (kLsMaxT * (kLsMaxT + 1) / 2 + kLsThreads - 1) / kLsThreads;     // Gram entries per thread at t = 64
constexpr int kLlrWItems = kLsMaxT * kLsMaxT / kLsThreads;                                     // entries of W per thread at t = 64
constexpr int kLlrRecord = 8;                   // doubles per workgroup: sum |dx|^2, sum |x|^2, nuclear norm, sigma_max, residual, sweeps, 0, 0
constexpr size_t kLlrSmallLds = 64 * 1024;      // what a kernel may take without the opt-in
constexpr size_t kLlrLargeLds = 156 * 1024;     // the budget with it (the CU has 160 KiB)

struct LlrArgs {
    const cf* x; const cf* g; const float* step; const float* thresh;
    cf* xnew;
    double* part;                               // header + one record per workgroup, or NULL
    int T, H, W, block, sh, sw, nbw;            // nbw: blocks along w
    int S, P2, nq;                              // S pixels per staged tile, P2 = T (T + 1) / 2 entries, nq pixel slices per entry
};

// pixels [p0, p0 + ns) of the block, all frames, as v = x - step g -> tile [T][ld]
__device__ __forceinline__ void llr_stage(const LlrArgs& a, cf* tile, int ld, long base, long HW, int bw, int p0, int ns, float step, int tid) {
    for (int e = tid; e < a.T * ns; e += kLsThreads) {
        const int f = e / ns, s = e - f * ns, p = p0 + s;
        const int r = p / bw, c = p - r * bw;
        const long q = base + (long)f * HW + (long)r * a.W + c;
        cf v = a.x[q];
        if (a.g) v = solve_v(v, a.g[q], step);
        tile[f * ld + s] = v;
    }
}

__global__ __launch_bounds__(kLsThreads) void llr_prox_kernel(LlrArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = a.T, tid = threadIdx.x, b = blockIdx.y;
    double2* A = reinterpret_cast<double2*>(smem);            // [T][T]: G, then its eigenvalues on the diagonal, then U, then W as float32
    double2* V = A + T * T;                                   // [T][T]: the eigenvectors
    double* rot = reinterpret_cast<double*>(V + T * T);       // ls_jacobi's; afterwards h, the thresholded singular values, lam
    double* red = rot + kLsRotDoubles;                        // ls_jacobi's; before it the pixel slices of G, at the end the sums of the record
    cf* tile = reinterpret_cast<cf*>(red + kLsRedDoubles);    // [T][S + 1]
    const int S = a.S, ld = S + 1, P2 = a.P2, nq = a.nq;
    // the block: rows [r0, r1), columns [c0, c1) of the image
    const int bi = blockIdx.x / a.nbw, bj = blockIdx.x - bi * a.nbw;
    const int r0 = max(bi * a.block - a.sh, 0), r1 = min((bi + 1) * a.block - a.sh, a.H);
    const int c0 = max(bj * a.block - a.sw, 0), c1 = min((bj + 1) * a.block - a.sw, a.W);
    const int bw = c1 - c0, P = (r1 - r0) * bw;
    const long HW = (long)a.H * a.W;
    const long base = (long)b * T * HW + (long)r0 * a.W + c0;
    const float step = a.g ? *a.step : 0.f;
    const float thf = a.step ? *a.step * *a.thresh : *a.thresh;

    // ---- G = X^H X, the upper triangle in registers
    const int nitems = P2 * nq;
    int oi[kLlrGramItems], oj[kLlrGramItems], q0[kLlrGramItems];
    double re[kLlrGramItems], im[kLlrGramItems];
#pragma unroll
    for (int k = 0; k < kLlrGramItems; ++k) {
        const int idx = tid + k * kLsThreads;
        oi[k] = oj[k] = q0[k] = 0; re[k] = im[k] = 0.0;
        if (idx < nitems) {
            int i, j;
            ls_pair_of(idx % P2, T, i, j);
            oi[k] = i * ld; oj[k] = j * ld; q0[k] = idx / P2;
        }
    }
    for (int p0 = 0; p0 < P; p0 += S) {
        const int ns = min(S, P - p0);
        llr_stage(a, tile, ld, base, HW, bw, p0, ns, step, tid);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kLlrGramItems; ++k) {
            if (tid + k * kLsThreads < nitems) {
                const cf* ri = tile + oi[k];
                const cf* rj = tile + oj[k];
                double r = re[k], m = im[k];                  // conj(x) y = (xr yr + xi yi) + i (xr yi - xi yr)
                for (int s = q0[k]; s < ns; s += nq) {
                    const cf xf = ri[s], yf = rj[s];
                    const double xr = (double)xf.x, xi = (double)xf.y, yr = (double)yf.x, yi = (double)yf.y;
                    r = fma(xr, yr, r);
                    r = fma(xi, yi, r);
                    m = fma(xr, yi, m);
                    m = fma(-xi, yr, m);
                }
                re[k] = r; im[k] = m;
            }
        }
        if (p0 + S < P) __syncthreads();                      // the next tile overwrites this one; the last one stays for the application
    }
    if (nq > 1) {                                             // P2 nq <= 256: the slices of an entry, added in slice order
        double2* sl = reinterpret_cast<double2*>(red);
        if (tid < nitems) sl[tid] = make_double2(re[0], im[0]);
        __syncthreads();
        if (tid < P2) {
            double r = sl[tid].x, m = sl[tid].y;
            for (int q = 1; q < nq; ++q) { r += sl[q * P2 + tid].x; m += sl[q * P2 + tid].y; }
            re[0] = r; im[0] = m;
        }
        __syncthreads();                                      // red is ls_jacobi's from here on
    }
#pragma unroll
    for (int k = 0; k < kLlrGramItems; ++k) {
        const int idx = tid + k * kLsThreads;
        if (idx < P2) {
            int i, j;
            ls_pair_of(idx, T, i, j);
            const double m = i == j ? 0.0 : im[k];
            A[i * T + j] = make_double2(re[k], m);
            A[j * T + i] = make_double2(re[k], -m);
        }
    }
    for (int e = tid; e < T * T; e += kLsThreads) V[e] = make_double2((e / T == e % T) ? 1.0 : 0.0, 0.0);
    __syncthreads();

    // ---- G = V diag(lam) V^H
    double off, diag;
    const int sweeps = ls_jacobi(A, V, rot, red, T, tid, off, diag);

    // ---- h(lam) per eigenvalue; A's off-diagonal part is dead now and takes U = diag(h) V^H, then W = V U as float32
    const double th = (double)thf;
    double* hk = rot;                                         // [T] h, then [T] sqrt(lam) h, then [T] lam
    if (tid < T) {
        const double lam = A[tid * T + tid].x;
        double hv = 0.0, sv = 0.0;
        if (lam > th * th) { const double sq = sqrt(lam); hv = 1.0 - th / sq; sv = sq - th; }
        hk[tid] = hv; hk[kLsMaxT + tid] = sv; hk[2 * kLsMaxT + tid] = lam;
    }
    __syncthreads();
    double smax = 0.0, nuc = 0.0;                             // thread 0 keeps them for the record
    if (tid == 0) {
        double lmax = hk[2 * kLsMaxT];
        for (int k = 0; k < T; ++k) { lmax = ls_nanmax(lmax, hk[2 * kLsMaxT + k]); nuc += hk[kLsMaxT + k]; }
        smax = lmax > 0.0 ? sqrt(lmax) : (lmax != lmax ? lmax : 0.0);
    }
    for (int e = tid; e < T * T; e += kLsThreads) {           // U[k][j] = h_k conj(V[j][k])
        const int k = e / T, j = e - k * T;
        const double2 v = V[j * T + k];
        A[e] = make_double2(hk[k] * v.x, -hk[k] * v.y);
    }
    __syncthreads();
    cf wacc[kLlrWItems];
#pragma unroll
    for (int k = 0; k < kLlrWItems; ++k) {                    // W[i][j] = sum_k V[i][k] U[k][j]
        const int e = tid + k * kLsThreads;
        wacc[k] = mk(0.f, 0.f);
        if (e < T * T) {
            const int i = e / T, j = e - i * T;
            double wr = 0.0, wi = 0.0;
            for (int kk = 0; kk < T; ++kk) {
                const double2 x = V[i * T + kk], y = A[kk * T + j];
                wr += x.x * y.x - x.y * y.y;
                wi += x.x * y.y + x.y * y.x;
            }
            wacc[k] = mk((float)wr, (float)wi);
        }
    }
    __syncthreads();
    cf* Wl = reinterpret_cast<cf*>(A);                        // [T][T] float32 over the dead U
#pragma unroll
    for (int k = 0; k < kLlrWItems; ++k) {
        const int e = tid + k * kLsThreads;
        if (e < T * T) Wl[e] = wacc[k];
    }
    __syncthreads();

    // ---- xnew[i] = sum_t v[t] W[t][i] per (pixel, frame), the pixel on the lanes
    const bool staged = P <= S;                               // the one tile of the Gram pass is still there
    float s_dx = 0.f, s_x2 = 0.f;
    for (int p0 = 0; p0 < P; p0 += S) {
        const int ns = min(S, P - p0);
        if (!staged) {
            if (p0 > 0) __syncthreads();                      // every thread has read the tile before
            llr_stage(a, tile, ld, base, HW, bw, p0, ns, step, tid);
            __syncthreads();
        }
        for (int e = tid; e < T * ns; e += kLsThreads) {
            const int i = e / ns, s = e - i * ns, p = p0 + s;
            float ax = 0.f, ay = 0.f;
            for (int t = 0; t < T; ++t) {
                const cf w = Wl[t * T + i];
                const cf x = tile[t * ld + s];
                ax += x.x * w.x - x.y * w.y; ay += x.x * w.y + x.y * w.x;
            }
            const int r = p / bw, c = p - r * bw;
            const long q = base + (long)i * HW + (long)r * a.W + c;
            const cf xo = a.x[q];
            const float dx = ax - xo.x, dy = ay - xo.y;
            s_dx += dx * dx + dy * dy;
            s_x2 += ax * ax + ay * ay;
            if (a.xnew) a.xnew[q] = mk(ax, ay);
        }
    }
    if (a.part) {                                             // one record per workgroup; llr_record_kernel adds them in a fixed order
        float s[2] = {s_dx, s_x2};
        block_sums(s, reinterpret_cast<float*>(red), tid);
        if (tid == 0) {
            const long wg = (long)blockIdx.y * gridDim.x + blockIdx.x;
            double* o = a.part + (1 + wg) * kLlrRecord;
            o[0] = (double)s[0];
            o[1] = (double)s[1];
            o[2] = nuc; o[3] = smax;
            o[4] = diag > 0.0 ? off / diag : off;
            o[5] = (double)sweeps;
            o[6] = o[7] = 0.0;
            if (wg == 0) {                                    // the header: how many records follow
                a.part[0] = (double)((long)gridDim.x * gridDim.y);
#pragma unroll
                for (int k = 1; k < kLlrRecord; ++k) a.part[k] = 0.0;
            }
        }
    }
}

// One workgroup per row of `stride` doubles (a header with the number of records, then the records): rec (rows, 4) floats = the three sums
// and 0, info (rows, 4) doubles = the largest sigma_max, the worst residual, the most sweeps, the number of records.  Thread q adds or
// compares records q, q + 256, ... in that order, then a tree over the threads: float64 in an order that depends on the number only.
__global__ __launch_bounds__(256) void llr_record_kernel(const double* part, long stride, float* rec, double* info) {
    __shared__ double red[6][256];
    const int tid = threadIdx.x;
    const double* row = part + (long)blockIdx.x * stride;
    const long n = (long)row[0];
    const double* p = row + kLlrRecord;
    double s[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
    for (long e = tid; e < n; e += 256) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { s[q] += p[e * kLlrRecord + q]; m[q] = ls_nanmax(m[q], p[e * kLlrRecord + 3 + q]); }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { red[q][tid] = s[q]; red[3 + q][tid] = m[q]; }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                red[q][tid] += red[q][tid + st];
                red[3 + q][tid] = ls_nanmax(red[3 + q][tid], red[3 + q][tid + st]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (rec) {
            float* o = rec + (long)blockIdx.x * 4;
            o[0] = (float)red[0][0]; o[1] = (float)red[1][0]; o[2] = (float)red[2][0]; o[3] = 0.f;
        }
        if (info) {
            double* o = info + (long)blockIdx.x * 4;
            o[0] = red[3][0]; o[1] = red[4][0]; o[2] = red[5][0]; o[3] = (double)n;
        }
    }
}

// The LDS layout per (t, block).  fixed = G, V, the rotations and the reductions.  While fixed + a tile of the whole block stays within
// 64 KiB (t <= 35 at block 8, t <= 21 at block 16) that is the layout: one tile, several workgroups per CU.  Beyond it the kernel
// opts into the large LDS and takes the largest tile that fits beside the matrices -- the whole block up to t = 61 at block 8 and
// t = 44 at block 16, 43 pixels at t = 64 -- and where the block is larger than the tile the application stages it again tile by tile.
struct LlrPlan { int S; size_t lds; bool large; };

static LlrPlan llr_plan(int t, int block) {
    LlrPlan p{};
    const size_t fixed = (size_t)2 * t * t * sizeof(double2) + (kLsRotDoubles + kLsRedDoubles) * sizeof(double);
    const int pmax = block * block;
    const size_t full = fixed + (size_t)t * (pmax + 1) * sizeof(cf);
    if (full < kLlrSmallLds) { p.S = pmax; p.lds = full; p.large = false; return p; }
    const long fit = (long)((kLlrLargeLds - fixed) / ((size_t)t * sizeof(cf))) - 1;
    p.S = (int)(fit < pmax ? fit : pmax);
    p.lds = fixed + (size_t)t * (p.S + 1) * sizeof(cf);
    p.large = true;
    return p;
}

static long llr_blocks_along(int n, int block, int shift) { return ((long)n + shift + block - 1) / block; }

static int llr_prepare(int t, int block) {
    static std::once_flag once[64];
    static hipError_t status[64];
    return llr_plan(t, block).large ? large_lds_opt_in(reinterpret_cast<const void*>(llr_prox_kernel), "llr_prox_kernel", once, status) : CINE_OK;
}

// the limits both entry points share; shifts are checked by the caller
static int llr_sizes(const char* what, int b, int t, int h, int w, int block) {
    CINE_REQUIRE(b > 0 && t > 0 && h > 0 && w > 0 && block > 0, CINE_EINVAL, "%s: bad sizes", what);
    CINE_REQUIRE(t >= 2 && t <= kLsMaxT, CINE_EUNSUPPORTED, "%s: %d frames, 2 .. %d are supported", what, t, kLsMaxT);
    CINE_REQUIRE(block >= kLlrMinBlock && block <= kLlrMaxBlock, CINE_EUNSUPPORTED, "%s: block %d, %d .. %d are supported", what, block,
                 kLlrMinBlock, kLlrMaxBlock);
    CINE_REQUIRE(b <= 65535, CINE_EUNSUPPORTED, "%s: b > 65535", what);
    CINE_REQUIRE(llr_blocks_along(h, block, block - 1) * llr_blocks_along(w, block, block - 1) <= 2147483647L, CINE_EUNSUPPORTED,
                 "%s: too many blocks per image", what);
    return CINE_OK;
}

static bool llr_shift_ok(int block, int sh, int sw) { return sh >= 0 && sh < block && sw >= 0 && sw < block; }

static size_t llr_part_bytes(long nblk, int b) { return (size_t)(1 + nblk * b) * kLlrRecord * sizeof(double); }

static int llr_prox_launch(const float* x, const float* g, const float* step_dev, const float* thresh_dev, int block, int sh, int sw,
                           float* xnew, double* part, int b, int t, int h, int w, hipStream_t st) {
    const LlrPlan p = llr_plan(t, block);
    LlrArgs a{};
    a.x = reinterpret_cast<const cf*>(x); a.g = reinterpret_cast<const cf*>(g); a.step = step_dev; a.thresh = thresh_dev;
    a.xnew = reinterpret_cast<cf*>(xnew); a.part = part;
    a.T = t; a.H = h; a.W = w; a.block = block; a.sh = sh; a.sw = sw;
    a.nbw = (int)llr_blocks_along(w, block, sw);
    a.S = p.S; a.P2 = t * (t + 1) / 2; a.nq = a.P2 >= kLsThreads ? 1 : kLsThreads / a.P2;
    const long nblk = llr_blocks_along(h, block, sh) * a.nbw;
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(llr_prox_kernel, dim3((unsigned)nblk, b), dim3(kLsThreads), p.lds, st, a);
    return check_launch("llr_prox_kernel");
}

static int llr_record_launch(const double* part, long stride, float* rec, double* info, int rows, hipStream_t st) {
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(llr_record_kernel, dim3(rows), dim3(256), 0, st, part, stride, rec, info);
    return check_launch("llr_record_kernel");
}

}  // namespace cine

using namespace cine;

extern "C" size_t cine_llr_prox_ws_bytes(int b, int t, int h, int w, int block, int shift_h, int shift_w) {
    if (b <= 0 || b > 65535 || t < 2 || t > kLsMaxT || h <= 0 || w <= 0 || block < kLlrMinBlock || block > kLlrMaxBlock ||
        !llr_shift_ok(block, shift_h, shift_w))
        return 0;
    return llr_part_bytes(llr_blocks_along(h, block, shift_h) * llr_blocks_along(w, block, shift_w), b);
}

extern "C" int cine_llr_prox(const float* x, const float* g, const float* step_dev, const float* thresh_dev, int block, int shift_h,
                             int shift_w, float* xnew, float* rec, double* info, int b, int t, int h, int w, void* ws, size_t ws_bytes,
                             void* stream) {
    const char* what = "cine_llr_prox";
    CINE_REQUIRE(x && thresh_dev && (!g || step_dev), CINE_EINVAL, "%s: null pointer", what);
    if (int e = llr_sizes(what, b, t, h, w, block)) return e;
    CINE_REQUIRE(llr_shift_ok(block, shift_h, shift_w), CINE_EINVAL, "%s: shift (%d, %d) outside [0, %d)", what, shift_h, shift_w, block);
    const bool records = rec || info;
    CINE_REQUIRE(!records || ws, CINE_EINVAL, "%s: rec and info come with ws", what);
    {
        // xnew may be x and nothing else; rec, info and ws alias nothing
        const void* ins[4] = {x, g, step_dev, thresh_dev};
        const void* outs[4] = {xnew, rec, info, records ? ws : nullptr};
        bool ok = true;
        for (int i = 0; i < 4; ++i) {
            if (!outs[i]) continue;
            for (int j = 0; j < 4; ++j) ok = ok && (outs[i] != ins[j] || (i == 0 && j == 0));
            for (int j = 0; j < i; ++j) ok = ok && outs[i] != outs[j];
        }
        CINE_REQUIRE(ok, CINE_EINVAL, "%s: only xnew == x may alias", what);
    }
    CINE_REQUIRE(!info || (reinterpret_cast<uintptr_t>(info) & 7u) == 0, CINE_EINVAL, "%s: info must be 8-byte aligned", what);
    if (records) {
        CINE_REQUIRE(solve_aligned16(ws), CINE_EINVAL, "%s: ws must be 16-byte aligned", what);
        const size_t need = cine_llr_prox_ws_bytes(b, t, h, w, block, shift_h, shift_w);
        CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    }
    if (int e = llr_prepare(t, block)) return e;
    hipStream_t st = as_stream(stream);
    double* part = records ? reinterpret_cast<double*>(ws) : nullptr;
    if (int e = llr_prox_launch(x, g, step_dev, thresh_dev, block, shift_h, shift_w, xnew, part, b, t, h, w, st)) return e;
    return records ? llr_record_launch(part, 0, rec, info, 1, st) : CINE_OK;
}

namespace {
// workspace of the solve: [operator scratch | g | iters rows of records, each for the worst case over all shifts]
struct LlrSolveWs { size_t op_bytes, total; long stride; void* op; float* g; double* part; };      // stride: doubles per row of records

LlrSolveWs llr_solve_ws(void* ws, int b, int t, int c, int h, int w, int mask_w, int block, int iters) {
    LlrSolveWs y{};
    WsCursor at{static_cast<unsigned char*>(ws)};
    const size_t row = llr_part_bytes(llr_blocks_along(h, block, block - 1) * llr_blocks_along(w, block, block - 1), b);
    y.stride = (long)(row / sizeof(double));
    y.op_bytes = dc_ws_bytes(mask_w, b, t, c, h, w);
    y.op = y.op_bytes ? at.take<void>(y.op_bytes) : nullptr;
    y.g = at.take<float>((size_t)b * t * h * w * sizeof(cf));
    y.part = at.take<double>((size_t)iters * row);
    y.total = at.end;
    return y;
}
}  // namespace

extern "C" size_t cine_llr_solve_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int block, int iters) {
    if (b <= 0 || b > 65535 || t < 2 || t > kLsMaxT || c <= 0 || h <= 0 || w <= 0 || iters <= 0 || block < kLlrMinBlock || block > kLlrMaxBlock)
        return 0;
    return llr_solve_ws(nullptr, b, t, c, h, w, mask_w, block, iters).total;
}

extern "C" int cine_llr_solve(float* x, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask, int mask_w,
                              const float* step_dev, const float* thresh_dev, int block, const int* shifts, int iters, float* rec,
                              double* info, int b, int t, int c, int h, int w, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_llr_solve";
    CINE_REQUIRE(x && zf && sens && mask && step_dev && thresh_dev && ws, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(c > 0 && iters >= 1, CINE_EINVAL, "%s: bad sizes", what);
    if (int e = llr_sizes(what, b, t, h, w, block)) return e;
    CINE_REQUIRE(mask_w == 1 || mask_w == w, CINE_EINVAL, "%s: mask_w %d is neither 1 (row mask) nor w", what, mask_w);
    if (shifts) {
        for (int k = 0; k < iters; ++k)
            CINE_REQUIRE(llr_shift_ok(block, shifts[2 * k], shifts[2 * k + 1]), CINE_EINVAL, "%s: shift (%d, %d) of iteration %d outside [0, %d)",
                         what, shifts[2 * k], shifts[2 * k + 1], k, block);
    }
    {
        const void* const outs[] = {x, rec, info};
        const void* const ins[] = {zf, sens, sens_tiled, mask, step_dev, thresh_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, ws), CINE_EINVAL, "%s: x, rec, info and ws must not alias an operand or each other", what);
    }
    CINE_REQUIRE(solve_aligned16(ws), CINE_EINVAL, "%s: ws must be 16-byte aligned", what);
    CINE_REQUIRE(!info || (reinterpret_cast<uintptr_t>(info) & 7u) == 0, CINE_EINVAL, "%s: info must be 8-byte aligned", what);
    const size_t need = cine_llr_solve_ws_bytes(b, t, c, h, w, mask_w, block, iters);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    const LlrSolveWs y = llr_solve_ws(ws, b, t, c, h, w, mask_w, block, iters);
    const bool records = rec || info;
    hipStream_t st = as_stream(stream);
    for (int k = 0; k < iters; ++k) {
        const float* xk = k == 0 ? zf : x;          // x_0 = zf without a copy; from then on the prox works in place
        if (int e = solve_gradient(what, xk, zf, sens, sens_tiled, mask, mask_w, y.g, b, t, c, h, w, y.op, y.op_bytes, stream)) return e;
        if (k == 0) {                               // the opt-in only after the operator has accepted the sizes
            if (int e = llr_prepare(t, block)) return e;
        }
        const int sh = shifts ? shifts[2 * k] : 0, sw = shifts ? shifts[2 * k + 1] : 0;
        if (int e = llr_prox_launch(xk, y.g, step_dev, thresh_dev, block, sh, sw, x, records ? y.part + (size_t)k * y.stride : nullptr,
                                    b, t, h, w, st))
            return e;
    }
    return records ? llr_record_launch(y.part, y.stride, rec, info, iters, st) : CINE_OK;
}
