// raw_window_kernels.hip -- the data front-end's first step for raw k-space of ANY matrix size (reference data/mri_data.py:283-289,
// data/transforms.py:206-214): only the centered crop window of the centered ortho IDFT is computed, straight from the HDF5 `y`
// layout (t_in, nx, ny, coil).
//
//   out[t, c, i, j] = sum_{x, y} Dx[i, x] Dy[j, y] raw[t, x, y, c]           t < t_out, i < cx, j < cy
//   D[i, n]        = s N^{-1/2} exp(+2 pi i (n - h)(m0 + i - h) / N)         h = N / 2, m0 = (N - cw) / 2
//
// which is (fftshift o ifft2 o ifftshift)(scale * raw[:t_out]) (shifts by N / 2 on both sides, ortho) restricted to rows
// x0 .. x0 + cx and columns y0 .. y0 + cy.  No FFT plan: two complex GEMMs against window DFT matrices (cx x nx, cy x ny) that
// raw_window_matrix_kernel builds in the caller's workspace on every call -- (n - h)(m - h) mod N reduced exactly in 64-bit
// integers, sincospi in double, `scale` folded into Dx, rounded to float once.  The axis that costs fewer complex MACs in total
// goes first (x first: nx ny cx + ny cx cy per image, y first: nx ny cy + nx cy cx); the intermediate sits in the workspace.
//
// raw_window_gemm_kernel: C[b][m][n] = sum_k A[b][m][k] B[b][k][n], complex, exact fp32 on v_mfma_f32_16x16x4_f32 (a k-ordered
// fmaf chain, no atomics, fixed k order: repeated calls are bit-identical).  Every operand is addressed as
//   base + b * bat + (i / div) * s1 + (i % div) * s0 (+ k * sk)
// so the same kernel reads the raw layout, the intermediate and the matrices and writes the (t_out, coil, cx, cy) output directly.
// Workgroup: 256 threads, 64 x 64 complex outputs, 16 complex k per LDS stage (double-buffered, re and im planes); wave (wm, wn)
// owns 32 x 32 = 2 x 2 MFMA tiles with two accumulators each,
//   Cr += Ar Br - Ai Bi,   Ci += Ar Bi + Ai Br,
// 16-row / 16-column MFMA tiles wholly outside M or N are skipped (a 200-wide window costs 208 rows, not 256).
#include <climits>
#include "common.h"
#include "conv_src.h"

namespace cine {

namespace rw {
constexpr int TM = 64, TN = 64, TK = 16;     // complex outputs / k per workgroup tile
constexpr int LD = 64 + 16;                  // LDS row (floats): the four 16-lane groups of a fragment read hit disjoint banks
constexpr int kThreads = 256;
constexpr size_t kAlign = 256;
}

struct RwOperand {                             // element (i, k) of a batch b: p[b * bat + (i / div) * s1 + (i % div) * s0 + k * sk]
    const float2* p;
    long bat, s1, s0, sk;
    int div;
};

struct RwGemmArgs {
    RwOperand a, b;                           // A: i = m; B: i = n
    float2* c;
    long c_bat, cm_s1, cm_s0, cn_s1, cn_s0;   // C[b][m][n] = c[b * c_bat + (m / cm_div) * cm_s1 + (m % cm_div) * cm_s0 + (n / cn_div) * cn_s1 + (n % cn_div) * cn_s0]
    int cm_div, cn_div;
    long M, N, K;
    int tiles_m, tiles_n;
    int m_fast;                               // tile order: m fastest (the data operand B is shared by consecutive tiles) or n fastest
};

__device__ __forceinline__ long rw_off(long i, int div, long s1, long s0) { return (i / div) * s1 + (i % div) * s0; }

// One operand's 64 x 16 stage, four elements per thread.  KC: k is the unit-stride index (the matrices, a single-coil intermediate):
// a lane walks k; otherwise a lane walks i (raw rows, the intermediate), which is the contiguous one there.
template <bool KC>
struct RwStage {
    long off[4];                               // element offsets without the k term
    bool iok[4];
    int kk[4];
    __device__ void init(const RwOperand& o, long i0, long ext, long bat_off, int tid) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = KC ? i0 + (tid >> 4) + 16 * j : i0 + (tid & 63);
            kk[j] = KC ? (tid & 15) : (tid >> 6) + 4 * j;
            iok[j] = i < ext;
            off[j] = bat_off + (iok[j] ? rw_off(i, o.div, o.s1, o.s0) : 0);
        }
    }
    __device__ void load(const RwOperand& o, long k0, long K, float2 (&v)[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long k = k0 + kk[j];
            v[j] = (iok[j] && k < K) ? o.p[off[j] + k * o.sk] : make_float2(0.f, 0.f);
        }
    }
    __device__ void store(float* re, float* im, const float2 (&v)[4], int tid) const {   // planes [TK][LD], index [k][i]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = KC ? (tid >> 4) + 16 * j : (tid & 63);
            re[kk[j] * rw::LD + i] = v[j].x;
            im[kk[j] * rw::LD + i] = v[j].y;
        }
    }
};

template <bool AK, bool BK>
__global__ __launch_bounds__(rw::kThreads) void raw_window_gemm_kernel(RwGemmArgs g) {
    using namespace rw;
    __shared__ float lds[2][4][TK * LD];          // [buffer][A re, A im, B re, B im][k][i]: 40 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // tile of this workgroup; the first 8 * floor(G / 8) tiles are regrouped so that the tiles sharing a data tile run on one XCD
    const int G = g.tiles_m * g.tiles_n, G8 = (G / 8) * 8;
    const int bid = blockIdx.x;
    const int lt = bid < G8 ? (bid % 8) * (G8 / 8) + bid / 8 : bid;
    const int tm = g.m_fast ? lt % g.tiles_m : lt / g.tiles_n;
    const int tn = g.m_fast ? lt / g.tiles_m : lt % g.tiles_n;
    const long m0 = (long)tm * TM, n0 = (long)tn * TN;
    const long b = blockIdx.y;

    RwStage<AK> sa;
    RwStage<BK> sb;
    sa.init(g.a, m0, g.M, b * g.a.bat, tid);
    sb.init(g.b, n0, g.N, b * g.b.bat, tid);

    bool mv[2], nv[2];                            // wave-uniform: does MFMA tile (ms) / (ns) hold any valid row / column
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        mv[s] = m0 + 32 * wm + 16 * s < g.M;
        nv[s] = n0 + 32 * wn + 16 * s < g.N;
    }

    f32x4 accr[2][2], acci[2][2];
#pragma unroll
    for (int ms = 0; ms < 2; ++ms)
#pragma unroll
        for (int ns = 0; ns < 2; ++ns) {
            accr[ms][ns] = f32x4{0.f, 0.f, 0.f, 0.f};
            acci[ms][ns] = f32x4{0.f, 0.f, 0.f, 0.f};
        }

    const int nkt = (int)((g.K + TK - 1) / TK);
    float2 va[4], vb[4];
    sa.load(g.a, 0, g.K, va);
    sb.load(g.b, 0, g.K, vb);
    sa.store(lds[0][0], lds[0][1], va, tid);
    sb.store(lds[0][2], lds[0][3], vb, tid);
    __syncthreads();

    const int fr = lane >> 4, fc = lane & 15;    // fragment read: row k = 4 q + fr, column i = 16 s + fc
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        const bool more = kt + 1 < nkt;
        if (more) {                               // next stage's global loads fly during this stage's MFMAs
            sa.load(g.a, (long)(kt + 1) * TK, g.K, va);
            sb.load(g.b, (long)(kt + 1) * TK, g.K, vb);
        }
        const float* Ar = lds[buf][0];
        const float* Ai = lds[buf][1];
        const float* Br = lds[buf][2];
        const float* Bi = lds[buf][3];
#pragma unroll
        for (int q = 0; q < TK / 4; ++q) {
            float ar[2], ai[2], an[2], br[2], bi[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int ra = (4 * q + fr) * LD + 32 * wm + 16 * s + fc;
                const int rb = (4 * q + fr) * LD + 32 * wn + 16 * s + fc;
                ar[s] = Ar[ra]; ai[s] = Ai[ra]; an[s] = -ai[s];
                br[s] = Br[rb]; bi[s] = Bi[rb];
            }
#pragma unroll
            for (int ms = 0; ms < 2; ++ms)
#pragma unroll
                for (int ns = 0; ns < 2; ++ns) {
                    if (!(mv[ms] && nv[ns])) continue;
                    accr[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[ms], br[ns], accr[ms][ns], 0, 0, 0);
                    accr[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(an[ms], bi[ns], accr[ms][ns], 0, 0, 0);
                    acci[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[ms], bi[ns], acci[ms][ns], 0, 0, 0);
                    acci[ms][ns] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai[ms], br[ns], acci[ms][ns], 0, 0, 0);
                }
        }
        if (more) {                               // the other buffer was last read before the previous barrier
            sa.store(lds[buf ^ 1][0], lds[buf ^ 1][1], va, tid);
            sb.store(lds[buf ^ 1][2], lds[buf ^ 1][3], vb, tid);
        }
        __syncthreads();
    }

    // epilogue: lane holds C[m = 32 wm + 16 ms + 4 fr + r][n = 32 wn + 16 ns + fc]
    float2* cb = g.c + b * g.c_bat;
#pragma unroll
    for (int ns = 0; ns < 2; ++ns) {
        const long n = n0 + 32 * wn + 16 * ns + fc;
        if (!nv[ns] || n >= g.N) continue;
        const long noff = rw_off(n, g.cn_div, g.cn_s1, g.cn_s0);
#pragma unroll
        for (int ms = 0; ms < 2; ++ms) {
            if (!mv[ms]) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + 32 * wm + 16 * ms + 4 * fr + r;
                if (m < g.M) cb[rw_off(m, g.cm_div, g.cm_s1, g.cm_s0) + noff] = make_float2(accr[ms][ns][r], acci[ms][ns][r]);
            }
        }
    }
}

// Dx (cx x nx) then Dy (cy x ny), row-major, complex: D[i][n] = s exp(+2 pi i (n - h)(m0 + i - h) / N)
__global__ void raw_window_matrix_kernel(float2* __restrict__ dx, float2* __restrict__ dy, int nx, int cx, int ny, int cy,
                                         double sx, double sy) {
    const long nxe = (long)cx * nx, total = nxe + (long)cy * ny;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const bool isx = e < nxe;
        const long f = isx ? e : e - nxe;
        const int N = isx ? nx : ny, cw = isx ? cx : cy;
        const long i = f / N, n = f % N;
        const long h = N / 2, m = (N - cw) / 2 + i;
        long r = ((n - h) * (m - h)) % N;        // |(n - h)(m - h)| < N^2: exact in 64 bits
        if (r < 0) r += N;
        double sn, cs;
        sincospi(2.0 * (double)r / (double)N, &sn, &cs);
        const double s = isx ? sx : sy;
        (isx ? dx : dy)[f] = make_float2((float)(s * cs), (float)(s * sn));
    }
}

namespace {

struct RwPlan {
    bool x_first;
    size_t off_dx, off_dy, off_z, bytes;
};

size_t rw_round(size_t n) { return (n + rw::kAlign - 1) / rw::kAlign * rw::kAlign; }

bool rw_shapes_ok(int t_in, int nx, int ny, int c, int t_out, int cx, int cy) {
    return nx >= 1 && ny >= 1 && c >= 1 && cx >= 1 && cx <= nx && cy >= 1 && cy <= ny && t_out >= 1 && t_out <= t_in;
}

RwPlan rw_plan(int t_out, int nx, int ny, int c, int cx, int cy) {
    RwPlan p{};
    const double cost_x = (double)nx * ny * cx + (double)ny * cx * cy;    // complex MACs per image, x transformed first
    const double cost_y = (double)nx * ny * cy + (double)nx * cy * cx;
    p.x_first = cost_x <= cost_y;
    const size_t z = p.x_first ? (size_t)t_out * cx * ny * c : (size_t)t_out * nx * c * cy;
    p.off_dx = 0;
    p.off_dy = rw_round((size_t)cx * nx * sizeof(float2));
    p.off_z = p.off_dy + rw_round((size_t)cy * ny * sizeof(float2));
    p.bytes = p.off_z + rw_round(z * sizeof(float2));
    return p;
}

RwOperand rw_operand(const float2* p, long bat, long s1, long s0, long sk, int div) { return RwOperand{p, bat, s1, s0, sk, div}; }

int rw_gemm(RwGemmArgs g, int batch, hipStream_t st) {
    const long tm = (g.M + rw::TM - 1) / rw::TM, tn = (g.N + rw::TN - 1) / rw::TN;
    constexpr long kMaxBlocks = (1L << 32) / rw::kThreads - 1;                 // grid.x * block.x < 2^32
    CINE_REQUIRE(tm * tn <= kMaxBlocks, CINE_EUNSUPPORTED, "cine_raw_window_ifft2c: %ld x %ld output tiles exceed the grid limit of %ld workgroups",
                 tm, tn, kMaxBlocks);
    g.tiles_m = (int)tm;
    g.tiles_n = (int)tn;
    const dim3 grid((unsigned)(tm * tn), (unsigned)batch), block(rw::kThreads);
    const bool ak = g.a.sk == 1, bk = g.b.sk == 1;
    if (ak && bk) hipLaunchKernelGGL((raw_window_gemm_kernel<true, true>), grid, block, 0, st, g);
    else if (ak) hipLaunchKernelGGL((raw_window_gemm_kernel<true, false>), grid, block, 0, st, g);
    else if (bk) hipLaunchKernelGGL((raw_window_gemm_kernel<false, true>), grid, block, 0, st, g);
    else hipLaunchKernelGGL((raw_window_gemm_kernel<false, false>), grid, block, 0, st, g);
    return check_launch("raw_window_gemm_kernel");
}

}  // namespace
}  // namespace cine

using namespace cine;

extern "C" size_t cine_raw_window_ws_bytes(int t_out, int nx, int ny, int c, int cx, int cy) {
    if (!rw_shapes_ok(t_out, nx, ny, c, t_out, cx, cy)) return 0;
    return rw_plan(t_out, nx, ny, c, cx, cy).bytes;
}

extern "C" int cine_raw_window_ifft2c(const float* raw, float* out, void* ws, size_t ws_bytes, int t_in, int nx, int ny, int c,
                                      int t_out, int cx, int cy, float scale, void* stream) {
    CINE_REQUIRE(raw && out && ws && (const void*)raw != (const void*)out, CINE_EINVAL, "cine_raw_window_ifft2c: null or aliased pointers");
    CINE_REQUIRE(rw_shapes_ok(t_in, nx, ny, c, t_out, cx, cy), CINE_EINVAL,
                 "cine_raw_window_ifft2c: Invalid shapes. (t_in %d, nx %d, ny %d, coils %d, t_out %d, window %d x %d)",
                 t_in, nx, ny, c, t_out, cx, cy);
    const RwPlan p = rw_plan(t_out, nx, ny, c, cx, cy);
    CINE_REQUIRE(ws_bytes >= p.bytes, CINE_EWORKSPACE, "cine_raw_window_ifft2c: workspace %zu bytes, needs %zu", ws_bytes, p.bytes);
    CINE_REQUIRE(t_out <= 65535, CINE_EUNSUPPORTED, "cine_raw_window_ifft2c: %d frames exceed the grid limit 65535", t_out);
    const long M1 = p.x_first ? cx : (long)nx * c, N2 = p.x_first ? cy : (long)c * cy;
    CINE_REQUIRE(M1 <= INT_MAX && N2 <= INT_MAX && (long)ny * c <= INT_MAX, CINE_EUNSUPPORTED,
                 "cine_raw_window_ifft2c: a GEMM extent exceeds the grid limit %d", INT_MAX);

    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    char* w = static_cast<char*>(ws);
    float2* dx = reinterpret_cast<float2*>(w + p.off_dx);
    float2* dy = reinterpret_cast<float2*>(w + p.off_dy);
    float2* z = reinterpret_cast<float2*>(w + p.off_z);
    const float2* r = reinterpret_cast<const float2*>(raw);
    float2* o = reinterpret_cast<float2*>(out);

    {
        const long total = (long)cx * nx + (long)cy * ny;
        const long blocks = (total + 255) / 256;
        hipLaunchKernelGGL(raw_window_matrix_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, st, dx, dy, nx, cx, ny,
                           cy, (double)scale / sqrt((double)nx), 1.0 / sqrt((double)ny));
        if (int e = check_launch("raw_window_matrix_kernel")) return e;
    }

    const long img = (long)nx * ny * c;            // one raw frame
    const long oimg = (long)c * cx * cy;           // one output frame
    RwGemmArgs g1{}, g2{};
    if (p.x_first) {
        // Z[t][i][(y, coil)] = sum_x Dx[i][x] raw[t][x][(y, coil)]
        const long zimg = (long)cx * ny * c;
        g1.a = rw_operand(dx, 0, nx, 0, 1, 1);
        g1.b = rw_operand(r, img, 1, 0, (long)ny * c, 1);
        g1.c = z; g1.c_bat = zimg; g1.cm_s1 = (long)ny * c; g1.cm_div = 1; g1.cn_s1 = 1; g1.cn_div = 1;
        g1.M = cx; g1.N = (long)ny * c; g1.K = nx; g1.m_fast = 1;
        // out[t][coil][i][j] = sum_y Z[t][i][(y, coil)] Dy[j][y]; rows m = (i, coil)
        g2.a = rw_operand(z, zimg, (long)ny * c, 1, c, c);
        g2.b = rw_operand(dy, 0, ny, 0, 1, 1);
        g2.c = o; g2.c_bat = oimg; g2.cm_s1 = cy; g2.cm_s0 = (long)cx * cy; g2.cm_div = c; g2.cn_s1 = 1; g2.cn_div = 1;
        g2.M = (long)cx * c; g2.N = cy; g2.K = ny; g2.m_fast = 0;
    } else {
        // Z[t][(x, coil)][j] = sum_y raw[t][x][y][coil] Dy[j][y]; rows m = (x, coil)
        const long zimg = (long)nx * c * cy;
        g1.a = rw_operand(r, img, (long)ny * c, 1, c, c);
        g1.b = rw_operand(dy, 0, ny, 0, 1, 1);
        g1.c = z; g1.c_bat = zimg; g1.cm_s1 = cy; g1.cm_div = 1; g1.cn_s1 = 1; g1.cn_div = 1;
        g1.M = (long)nx * c; g1.N = cy; g1.K = ny; g1.m_fast = 0;
        // out[t][coil][i][j] = sum_x Dx[i][x] Z[t][(x, coil)][j]; columns n = (coil, j)
        g2.a = rw_operand(dx, 0, nx, 0, 1, 1);
        g2.b = rw_operand(z, zimg, cy, 1, (long)c * cy, cy);
        g2.c = o; g2.c_bat = oimg; g2.cm_s1 = cy; g2.cm_div = 1; g2.cn_s1 = (long)cx * cy; g2.cn_s0 = 1; g2.cn_div = cy;
        g2.M = cx; g2.N = (long)c * cy; g2.K = nx; g2.m_fast = 1;
    }
    if (int e = rw_gemm(g1, t_out, st)) return e;
    return rw_gemm(g2, t_out, st);
}
