// espirit_kernels.hip -- the dense steps of the ESPIRiT calibration (Uecker et al., MRM 71:990-1001, 2014) on the device, without an
// eigensolver, so that the whole calibration is a fixed launch sequence a hipGraph can hold.
//
//   cine_espirit_gram       G = A^H A of the kk x kk patch matrix A of the central min(r, ny) x min(r, nx) block of kavg (c, ny, nx),
//                           n = kk kk c square, columns ordered (py, px, coil).  The block is first copied to [y][x][coil] float64
//                           (acs_stage_kernel); then one thread per entry of the upper triangle adds its exact float32 x float32
//                           products in float64 in patch order (espirit_gram_kernel) and writes G[a][b] and G[b][a] = conj.  The
//                           order depends on the shape only: bit-identical from call to call, exactly Hermitian.
//   cine_zgemm_f64          C = alpha A B + beta D, n x n row-major complex128, on v_mfma_f64_16x16x4_f64: four real MFMAs per
//                           complex product (Cr += Ar Br, Cr += (-Ai) Bi, Ci += Ar Bi, Ci += Ai Br), k ascending in one accumulator per
//                           output: deterministic.  32 x 32 output tile per workgroup, 16 x 16 per wave, K in steps of 16 through LDS,
//                           the next step's operands in flight in registers.  Ragged tiles are zero-filled in LDS and masked on store.
//   cine_espirit_projector  P = 1/2 (I + sign(G - mu I)), mu = thresh^2 lam_max: the projector onto the eigenvectors of G with
//                           eigenvalue >= mu, which is all ESPIRiT takes from the eigen-decomposition.
//                             lam^:  M_0 = G, M_{j+1} = (M_j / |M_j|_F)^2, 8 times (the norm: frob_partial_kernel + frob_final_kernel
//                                    into a device scalar that the next GEMM applies to alpha); v = M_8 1; lam^ = v^H G v / v^H v.
//                             X_0 = (G - thresh^2 lam^ I) / (1.0001 lam^);  X <- 1.5 X - 0.5 X X^2, `iters` times (two GEMMs each).
//                             resid = max |X^2 - I| from one more GEMM after the last step;  proj = 1/2 (I + X) rounded once to complex64.
#include <cstdint>
#include "common.h"

namespace cine {

namespace esp {
constexpr int kMaxCoils = 32, kMaxN = 1152;
constexpr int TM = 32, TN = 32, TK = 16;      // zgemm: output tile, K step
constexpr int PITCH = 48;                     // zgemm: LDS row of one k in doubles (= 16 mod 32: the two k of a 32-lane group on distinct banks)
constexpr int kThreads = 256;
constexpr int kParts = 256;                   // partial sums of the reductions
constexpr int kSquarings = 8;
}

using f64x4 = __attribute__((ext_vector_type(4))) double;

// ------------------------------------------------------------------ Gram matrix of the patch matrix
__global__ __launch_bounds__(256) void acs_stage_kernel(const float2* __restrict__ kavg, double2* __restrict__ acs, int c, int ny, int nx,
                                                        int ry, int rx, int y0, int x0) {
    const long total = (long)ry * rx * c;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int coil = (int)(e % c);
        const long p = e / c;
        const int x = (int)(p % rx), y = (int)(p / rx);
        const float2 v = kavg[((long)coil * ny + y0 + y) * nx + x0 + x];
        acs[e] = make_double2((double)v.x, (double)v.y);
    }
}

// thread: entry (a = blockIdx.y, b = 64 blockIdx.x + tid), b >= a; a = (py kk + px) c + i
__global__ __launch_bounds__(64) void espirit_gram_kernel(const double2* __restrict__ acs, double2* __restrict__ gram, int c, int kk, int ry,
                                                          int rx, int n) {
    const int a = blockIdx.y;
    if ((int)blockIdx.x * 64 + 63 < a) return;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n || b < a) return;
    const int i = a % c, pa = a / c, py = pa / kk, px = pa % kk;
    const int j = b % c, pb = b / c, qy = pb / kk, qx = pb % kk;
    const int my = ry - kk + 1, mx = rx - kk + 1;
    double re = 0.0, im = 0.0;                   // conj(u) v = (ur vr + ui vi) + i (ur vi - ui vr)
    for (int y = 0; y < my; ++y) {
        const double2* ua = acs + ((long)(y + py) * rx + px) * c + i;
        const double2* vb = acs + ((long)(y + qy) * rx + qx) * c + j;
        for (int x = 0; x < mx; ++x) {
            const double2 u = ua[(long)x * c], v = vb[(long)x * c];
            re = fma(u.x, v.x, re);
            re = fma(u.y, v.y, re);
            im = fma(u.x, v.y, im);
            im = fma(-u.y, v.x, im);
        }
    }
    if (a == b) im = 0.0;
    gram[(long)a * n + b] = make_double2(re, im);
    if (a != b) gram[(long)b * n + a] = make_double2(re, -im);
}

// ------------------------------------------------------------------ complex128 GEMM on the f64 MFMA
struct ZgemmArgs {
    const double2 *A, *B, *D;
    double2* C;
    const double* scale;                       // optional device scalar s: alpha / s^2 is applied
    int n;
    double ar, ai, br, bi;
};

// LDS: real and imaginary planes of the A tile as [k][row] and of the B tile as [k][col], PITCH doubles per k.  A fragment read of
// v_mfma_f64_16x16x4_f64 takes element [k = 4 q + (l >> 4)][l & 15] as one 8-byte access: lanes 0-15 and 16-31 of a 32-lane group read two k
// whose rows start 48 = 16 (mod 32) 8-byte slots apart, so the group covers 32 distinct slots.  The stores put 32 consecutive rows
// (columns) of one k side by side.
__global__ __launch_bounds__(esp::kThreads) void zgemm_f64_kernel(ZgemmArgs g) {
    using namespace esp;
    __shared__ double Ar[TK * PITCH], Ai[TK * PITCH], Br[TK * PITCH], Bi[TK * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = g.n;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int lr = tid & 31, lk = tid >> 5;      // loads: row (column) of the tile, k pair (A) / k and k + 8 (B)
    const int wm = (wave >> 1) * 16, wn = (wave & 1) * 16;
    const int fr = lane & 15, fk = lane >> 4;

    const double2 zero = make_double2(0.0, 0.0);
    double2 pa0, pa1, pb0, pb1;
    auto fetch = [&](int k0) {
        const int row = m0 + lr, ka = k0 + 2 * lk;
        const double2* ap = g.A + (long)row * n + ka;
        pa0 = row < n && ka < n ? ap[0] : zero;
        pa1 = row < n && ka + 1 < n ? ap[1] : zero;
        const int col = n0 + lr, kb = k0 + lk;
        pb0 = col < n && kb < n ? g.B[(long)kb * n + col] : zero;
        pb1 = col < n && kb + 8 < n ? g.B[(long)(kb + 8) * n + col] : zero;
    };

    f64x4 accr = {0.0, 0.0, 0.0, 0.0}, acci = {0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int k0 = 0; k0 < n; k0 += TK) {
        __syncthreads();                         // the previous step's reads are done
        Ar[(2 * lk) * PITCH + lr] = pa0.x;
        Ai[(2 * lk) * PITCH + lr] = pa0.y;
        Ar[(2 * lk + 1) * PITCH + lr] = pa1.x;
        Ai[(2 * lk + 1) * PITCH + lr] = pa1.y;
        Br[lk * PITCH + lr] = pb0.x;
        Bi[lk * PITCH + lr] = pb0.y;
        Br[(lk + 8) * PITCH + lr] = pb1.x;
        Bi[(lk + 8) * PITCH + lr] = pb1.y;
        __syncthreads();
        if (k0 + TK < n) fetch(k0 + TK);
#pragma unroll
        for (int q = 0; q < TK / 4; ++q) {
            const int k = 4 * q + fk;
            const double xr = Ar[k * PITCH + wm + fr], xi = Ai[k * PITCH + wm + fr];
            const double yr = Br[k * PITCH + wn + fr], yi = Bi[k * PITCH + wn + fr];
            accr = __builtin_amdgcn_mfma_f64_16x16x4f64(xr, yr, accr, 0, 0, 0);
            acci = __builtin_amdgcn_mfma_f64_16x16x4f64(xr, yi, acci, 0, 0, 0);
            accr = __builtin_amdgcn_mfma_f64_16x16x4f64(-xi, yi, accr, 0, 0, 0);
            acci = __builtin_amdgcn_mfma_f64_16x16x4f64(xi, yr, acci, 0, 0, 0);
        }
    }

    double ar = g.ar, ai = g.ai;
    if (g.scale) {
        const double s = *g.scale;
        const double inv = 1.0 / (s * s);
        ar *= inv;
        ai *= inv;
    }
    const bool has_d = g.br != 0.0 || g.bi != 0.0;
    const int col = n0 + wn + fr;
    if (col >= n) return;
    // the f64 result map: register i of lane l is row (l >> 4) + 4 i, column l & 15
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = m0 + wm + fk + 4 * i;
        if (row >= n) continue;
        const long e = (long)row * n + col;
        double re = ar * accr[i] - ai * acci[i], im = ar * acci[i] + ai * accr[i];
        if (has_d) {
            const double2 d = g.D[e];
            re += g.br * d.x - g.bi * d.y;
            im += g.br * d.y + g.bi * d.x;
        }
        g.C[e] = make_double2(re, im);
    }
}

// ------------------------------------------------------------------ reductions and element-wise steps of the projector
// sum in a fixed order: thread partials (stride kParts * 256), then a tree in LDS
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
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

__device__ __forceinline__ double nan_max(double m, double v) { return (v > m || v != v) ? v : m; }   // a NaN stays

__device__ __forceinline__ double block_max_256(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = nan_max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void frob_partial_kernel(const double2* __restrict__ m, long total, double* __restrict__ part) {
    __shared__ double sh[256];
    double s = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)esp::kParts * 256) {
        const double2 v = m[e];
        s = fma(v.x, v.x, s);
        s = fma(v.y, v.y, s);
    }
    s = block_sum_256(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void frob_final_kernel(const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[256];
    const double s = block_sum_256(part[threadIdx.x], sh);
    if (threadIdx.x == 0) *out = sqrt(s);
}

// deviation of Y from the identity, max of the complex moduli
__global__ __launch_bounds__(256) void dev_partial_kernel(const double2* __restrict__ y, int n, double* __restrict__ part) {
    __shared__ double sh[256];
    const long total = (long)n * n;
    double m = 0.0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)esp::kParts * 256) {
        const double2 v = y[e];
        const double dr = v.x - ((e / n) == (e % n) ? 1.0 : 0.0);
        m = nan_max(m, sqrt(dr * dr + v.y * v.y));
    }
    m = block_max_256(m, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void dev_final_kernel(const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[256];
    const double m = block_max_256(part[threadIdx.x], sh);
    if (threadIdx.x == 0) *out = m;
}

// out[i] = sum_j M[i][j] v[j] (v == nullptr: v = 1); workgroup i, lane partials in j order, then a tree
__global__ __launch_bounds__(256) void matvec_kernel(const double2* __restrict__ m, const double2* __restrict__ v, double2* __restrict__ out,
                                                     int n) {
    __shared__ double sh[256];
    const int i = blockIdx.x;
    double re = 0.0, im = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double2 a = m[(long)i * n + j];
        if (v) {
            const double2 b = v[j];
            re += a.x * b.x - a.y * b.y;
            im += a.x * b.y + a.y * b.x;
        } else {
            re += a.x;
            im += a.y;
        }
    }
    re = block_sum_256(re, sh);
    im = block_sum_256(im, sh);
    if (threadIdx.x == 0) out[i] = make_double2(re, im);
}

// lam = Re(v^H w) / (v^H v)
__global__ __launch_bounds__(256) void rayleigh_kernel(const double2* __restrict__ v, const double2* __restrict__ w, int n,
                                                       double* __restrict__ lam) {
    __shared__ double sh[256];
    double p = 0.0, q = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double2 a = v[j], b = w[j];
        p += a.x * b.x + a.y * b.y;
        q += a.x * a.x + a.y * a.y;
    }
    p = block_sum_256(p, sh);
    q = block_sum_256(q, sh);
    if (threadIdx.x == 0) *lam = p / q;
}

__global__ __launch_bounds__(256) void sign_start_kernel(const double2* __restrict__ gram, double2* __restrict__ x, int n, double thresh,
                                                         const double* __restrict__ lam) {
    const long total = (long)n * n;
    const double l = *lam, mu = thresh * thresh * l, inv = 1.0 / (1.0001 * l);
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const double2 v = gram[e];
        const bool diag = (e / n) == (e % n);
        x[e] = make_double2((diag ? v.x - mu : v.x) * inv, v.y * inv);
    }
}

__global__ __launch_bounds__(256) void projector_out_kernel(const double2* __restrict__ x, float2* __restrict__ proj, int n) {
    const long total = (long)n * n;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const double2 v = x[e];
        const bool diag = (e / n) == (e % n);
        proj[e] = make_float2((float)(0.5 * ((diag ? 1.0 : 0.0) + v.x)), (float)(0.5 * v.y));
    }
}

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int launch_zgemm(const double2* a, const double2* b, const double2* d, double2* c, int n, double ar, double ai, double br, double bi,
                 const double* scale, hipStream_t st) {
    ZgemmArgs g{};
    g.A = a; g.B = b; g.D = d; g.C = c; g.scale = scale; g.n = n;
    g.ar = ar; g.ai = ai; g.br = br; g.bi = bi;
    hipLaunchKernelGGL(zgemm_f64_kernel, dim3((unsigned)ceil_div(n, esp::TN), (unsigned)ceil_div(n, esp::TM)), dim3(esp::kThreads), 0, st, g);
    return check_launch("zgemm_f64_kernel");
}

unsigned ew_blocks(long total) {
    const long b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// workspace of the projector: three n x n matrices | kParts partials | 2 scalars (padded to 16 bytes) | two n-vectors
struct ProjWs {
    double2 *m0, *m1, *m2, *v, *w;
    double *part, *scal;
};

size_t proj_ws_bytes(int n) {
    return (size_t)3 * n * n * sizeof(double2) + (size_t)esp::kParts * sizeof(double) + 16 + (size_t)2 * n * sizeof(double2);
}

ProjWs proj_ws(void* ws, int n) {
    ProjWs p{};
    char* c = static_cast<char*>(ws);
    const size_t mat = (size_t)n * n * sizeof(double2);
    p.m0 = reinterpret_cast<double2*>(c);
    p.m1 = reinterpret_cast<double2*>(c + mat);
    p.m2 = reinterpret_cast<double2*>(c + 2 * mat);
    c += 3 * mat;
    p.part = reinterpret_cast<double*>(c);
    c += esp::kParts * sizeof(double);
    p.scal = reinterpret_cast<double*>(c);
    c += 16;
    p.v = reinterpret_cast<double2*>(c);
    p.w = p.v + n;
    return p;
}

}  // namespace
}  // namespace cine

using namespace cine;

extern "C" size_t cine_espirit_gram_ws_bytes(int c, int ny, int nx, int r, int kk) {
    if (c < 1 || c > esp::kMaxCoils || ny < 1 || nx < 1 || r < 1 || kk < 1 || (long)kk * kk * c > esp::kMaxN) return 0;
    const int ry = r < ny ? r : ny, rx = r < nx ? r : nx;
    if (ry < kk || rx < kk) return 0;
    return (size_t)ry * rx * c * sizeof(double2);
}

extern "C" int cine_espirit_gram(const float* kavg, double* gram, void* ws, size_t ws_bytes, int c, int ny, int nx, int r, int kk,
                                 void* stream) {
    CINE_REQUIRE(kavg && gram && ws && (const void*)kavg != (const void*)gram && (const void*)kavg != (const void*)ws &&
                     (const void*)gram != (const void*)ws,
                 CINE_EINVAL, "cine_espirit_gram: null or aliased pointers");
    CINE_REQUIRE(c >= 1 && ny >= 1 && nx >= 1 && r >= 1 && kk >= 1, CINE_EINVAL,
                 "cine_espirit_gram: Invalid shapes. (coils %d, ny %d, nx %d, r %d, kernel %d)", c, ny, nx, r, kk);
    CINE_REQUIRE(c <= esp::kMaxCoils, CINE_EUNSUPPORTED, "cine_espirit_gram: %d coils, at most %d", c, esp::kMaxCoils);
    CINE_REQUIRE((long)kk * kk * c <= esp::kMaxN, CINE_EUNSUPPORTED, "cine_espirit_gram: n = %d x %d x %d coils = %ld, at most %d", kk, kk, c,
                 (long)kk * kk * c, esp::kMaxN);
    const int ry = r < ny ? r : ny, rx = r < nx ? r : nx;
    CINE_REQUIRE(ry >= kk && rx >= kk, CINE_EINVAL, "cine_espirit_gram: the %d x %d calibration block is smaller than the %d x %d kernel", ry, rx,
                 kk, kk);
    CINE_REQUIRE(aligned16(gram) && aligned16(ws) && (reinterpret_cast<uintptr_t>(kavg) & 7u) == 0, CINE_EINVAL,
                 "cine_espirit_gram: gram and ws must be 16-byte aligned, kavg 8-byte aligned");
    const size_t need = cine_espirit_gram_ws_bytes(c, ny, nx, r, kk);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "cine_espirit_gram: workspace %zu bytes, needs %zu", ws_bytes, need);

    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    const int n = kk * kk * c;
    double2* acs = static_cast<double2*>(ws);
    hipLaunchKernelGGL(acs_stage_kernel, dim3(ew_blocks((long)ry * rx * c)), dim3(256), 0, st, reinterpret_cast<const float2*>(kavg), acs, c, ny,
                       nx, ry, rx, ny / 2 - ry / 2, nx / 2 - rx / 2);
    if (int e = check_launch("acs_stage_kernel")) return e;
    hipLaunchKernelGGL(espirit_gram_kernel, dim3((unsigned)ceil_div(n, 64), (unsigned)n), dim3(64), 0, st, acs, reinterpret_cast<double2*>(gram),
                       c, kk, ry, rx, n);
    return check_launch("espirit_gram_kernel");
}

extern "C" int cine_zgemm_f64(const double* a, const double* b, const double* d, double* out, int n, double alpha_re, double alpha_im,
                              double beta_re, double beta_im, void* stream) {
    const bool has_d = beta_re != 0.0 || beta_im != 0.0;
    CINE_REQUIRE(a && b && out && (d || !has_d), CINE_EINVAL, "cine_zgemm_f64: null pointer");
    CINE_REQUIRE(out != a && out != b, CINE_EINVAL, "cine_zgemm_f64: out must not alias a or b");
    CINE_REQUIRE(n >= 1, CINE_EINVAL, "cine_zgemm_f64: n = %d", n);
    CINE_REQUIRE(n <= esp::kMaxN, CINE_EUNSUPPORTED, "cine_zgemm_f64: n = %d, at most %d", n, esp::kMaxN);
    CINE_REQUIRE(aligned16(a) && aligned16(b) && aligned16(d) && aligned16(out), CINE_EINVAL, "cine_zgemm_f64: operands must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    return launch_zgemm(reinterpret_cast<const double2*>(a), reinterpret_cast<const double2*>(b), reinterpret_cast<const double2*>(d),
                        reinterpret_cast<double2*>(out), n, alpha_re, alpha_im, beta_re, beta_im, nullptr, st);
}

extern "C" size_t cine_espirit_projector_ws_bytes(int n) {
    if (n < 1 || n > esp::kMaxN) return 0;
    return proj_ws_bytes(n);
}

extern "C" int cine_espirit_projector(const double* gram, int n, double thresh, int iters, float* proj_f32, double* lam_dev,
                                      double* resid_dev, void* ws, size_t ws_bytes, void* stream) {
    CINE_REQUIRE(gram && proj_f32 && lam_dev && resid_dev && ws, CINE_EINVAL, "cine_espirit_projector: null pointer");
    CINE_REQUIRE(n >= 1, CINE_EINVAL, "cine_espirit_projector: n = %d", n);
    CINE_REQUIRE(iters >= 1, CINE_EINVAL, "cine_espirit_projector: iters = %d, at least 1", iters);
    CINE_REQUIRE(thresh > 0.0, CINE_EINVAL, "cine_espirit_projector: thresh = %g, must be > 0", thresh);
    CINE_REQUIRE(n <= esp::kMaxN, CINE_EUNSUPPORTED, "cine_espirit_projector: n = %d, at most %d", n, esp::kMaxN);
    CINE_REQUIRE(aligned16(gram) && aligned16(ws) && (reinterpret_cast<uintptr_t>(proj_f32) & 7u) == 0 &&
                     (reinterpret_cast<uintptr_t>(lam_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(resid_dev) & 7u) == 0,
                 CINE_EINVAL, "cine_espirit_projector: gram and ws must be 16-byte aligned, the outputs 8-byte aligned");
    CINE_REQUIRE((const void*)gram != ws && (const void*)proj_f32 != ws && (const void*)gram != (const void*)proj_f32 && lam_dev != resid_dev,
                 CINE_EINVAL, "cine_espirit_projector: aliased pointers");
    const size_t need = proj_ws_bytes(n);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "cine_espirit_projector: workspace %zu bytes, needs %zu", ws_bytes, need);

    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    const ProjWs w = proj_ws(ws, n);
    const double2* G = reinterpret_cast<const double2*>(gram);
    const long total = (long)n * n;
    double* fro = w.scal;

    // lam^: 8 squarings, each operand divided by its Frobenius norm on load (alpha / s^2)
    const double2* cur = G;
    double2* nxt = w.m0;
    for (int j = 0; j < esp::kSquarings; ++j) {
        hipLaunchKernelGGL(frob_partial_kernel, dim3(esp::kParts), dim3(256), 0, st, cur, total, w.part);
        if (int e = check_launch("frob_partial_kernel")) return e;
        hipLaunchKernelGGL(frob_final_kernel, dim3(1), dim3(256), 0, st, w.part, fro);
        if (int e = check_launch("frob_final_kernel")) return e;
        if (int e = launch_zgemm(cur, cur, nullptr, nxt, n, 1.0, 0.0, 0.0, 0.0, fro, st)) return e;
        cur = nxt;
        nxt = nxt == w.m0 ? w.m1 : w.m0;
    }
    hipLaunchKernelGGL(matvec_kernel, dim3((unsigned)n), dim3(256), 0, st, cur, (const double2*)nullptr, w.v, n);
    if (int e = check_launch("matvec_kernel")) return e;
    hipLaunchKernelGGL(matvec_kernel, dim3((unsigned)n), dim3(256), 0, st, G, (const double2*)w.v, w.w, n);
    if (int e = check_launch("matvec_kernel")) return e;
    hipLaunchKernelGGL(rayleigh_kernel, dim3(1), dim3(256), 0, st, (const double2*)w.v, (const double2*)w.w, n, lam_dev);
    if (int e = check_launch("rayleigh_kernel")) return e;

    // Newton-Schulz: Y = X X, X' = -0.5 X Y + 1.5 X
    double2 *X = w.m0, *Y = w.m1, *Xn = w.m2;
    hipLaunchKernelGGL(sign_start_kernel, dim3(ew_blocks(total)), dim3(256), 0, st, G, X, n, thresh, (const double*)lam_dev);
    if (int e = check_launch("sign_start_kernel")) return e;
    for (int it = 0; it < iters; ++it) {
        if (int e = launch_zgemm(X, X, nullptr, Y, n, 1.0, 0.0, 0.0, 0.0, nullptr, st)) return e;
        if (int e = launch_zgemm(X, Y, X, Xn, n, -0.5, 0.0, 1.5, 0.0, nullptr, st)) return e;
        double2* t = X;
        X = Xn;
        Xn = t;
    }
    // the residual of the iterate that is handed out: one more product
    if (int e = launch_zgemm(X, X, nullptr, Y, n, 1.0, 0.0, 0.0, 0.0, nullptr, st)) return e;
    hipLaunchKernelGGL(dev_partial_kernel, dim3(esp::kParts), dim3(256), 0, st, (const double2*)Y, n, w.part);
    if (int e = check_launch("dev_partial_kernel")) return e;
    hipLaunchKernelGGL(dev_final_kernel, dim3(1), dim3(256), 0, st, (const double*)w.part, resid_dev);
    if (int e = check_launch("dev_final_kernel")) return e;
    hipLaunchKernelGGL(projector_out_kernel, dim3(ew_blocks(total)), dim3(256), 0, st, (const double2*)X, reinterpret_cast<float2*>(proj_f32), n);
    return check_launch("projector_out_kernel");
}
