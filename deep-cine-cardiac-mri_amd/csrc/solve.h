// solve.h -- what the four weight-free proximal solvers share (kt_kernels.hip, ls_kernels.hip, tv_kernels.hip, llr_kernels.hip).  All of
// them iterate on the data term's gradient g = A^H M A x - zf and differ in the proximal step alone, so this header holds the rest:
//   device   v = a - step g, the temporal-sparsity prox piece by piece (twiddles, centered forward DFT, soft threshold, centered
//            inverse DFT), the per-workgroup record of an iteration;
//   host     the gradient by the row or plane operator (solve_gradient), the rule about aliasing, the workspace cursor, the size
//            checks, the large-LDS opt-in; solve_kernels.hip: the record reduction.
// A new solver is its prox kernel, a workspace struct carved by WsCursor and a loop of solve_gradient + its prox launch.
// Who uses the device half: kt_prox_kernel all of it; tv_pd_kernel block_record; llr_prox_kernel solve_v and block_sums (its record
// is doubles); ls_prox_kernel solve_v and wave_sum ONLY -- the second half of that kernel is a deliberate copy of temporal_twiddles,
// temporal_dft_fwd, soft_threshold, temporal_dft_inv and block_record (the helpers made its solves measurably slower, the figures
// stand at the copy in ls_kernels.hip), so a change to one of these five has to be made there as well.
#pragma once
#include <cstdint>
#include <mutex>
#include "common.h"
#include "fft_core.h"

namespace cine {

constexpr int kSolveThreads = 256;                // workgroup size of every kernel that uses block_sums / block_record

// ------------------------------------------------------------------ device
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// v = a - step g in float32: ONE expression for every kernel that forms it, so that a Gram matrix and a prox see the same v
__device__ __forceinline__ cf solve_v(cf a, cf g, float step) { return mk(fmaf(-step, g.x, a.x), fmaf(-step, g.y, a.y)); }

// tw [T] = exp(-2 pi i j / T) / sqrt(T): the twiddles of fft1c variant 0 along t; a barrier must follow before they are read
__device__ __forceinline__ void temporal_twiddles(cf* tw, int T, int tid) {
    const double s = 1.0 / sqrt((double)T);
    for (int j = tid; j < T; j += kSolveThreads) {
        double sn, cs;
        sincospi(2.0 * (double)j / (double)T, &sn, &cs);
        tw[j] = mk((float)(cs * s), (float)(-sn * s));
    }
}

// Centered DFT along t of pixel p of the tile buf [T][PIX] at bin / frame i, directly: input index n = (g + ceil(T / 2)) % T, output
// index k = i - floor(T / 2) mod T, twiddle (n k) % T stepped without a multiplication.  One wavefront shares i, so tw is a broadcast.
template <int PIX>
__device__ __forceinline__ cf temporal_dft_fwd(const cf* buf, const cf* tw, int T, int i, int p) {
    int k = i - T / 2; if (k < 0) k += T;
    float ax = 0.f, ay = 0.f;
    int idx = ((T + 1) / 2 * k) % T;
    for (int g = 0; g < T; ++g) {
        const cf w = tw[idx];
        const cf x = buf[g * PIX + p];
        ax += x.x * w.x - x.y * w.y; ay += x.x * w.y + x.y * w.x;
        idx += k; if (idx >= T) idx -= T;
    }
    return mk(ax, ay);
}

template <int PIX>
__device__ __forceinline__ cf temporal_dft_inv(const cf* buf, const cf* tw, int T, int i, int p) {
    int k = i - T / 2; if (k < 0) k += T;
    float ax = 0.f, ay = 0.f;
    int idx = ((T + 1) / 2 * k) % T;
    for (int g = 0; g < T; ++g) {
        const cf w = tw[idx];
        const cf x = buf[g * PIX + p];
        ax += x.x * w.x + x.y * w.y; ay += x.y * w.x - x.x * w.y;         // x * conj(w)
        idx += k; if (idx >= T) idx -= T;
    }
    return mk(ax, ay);
}

// soft(c, th) = c max(|c| - th, 0) / |c|, 0 at c = 0; left: its magnitude max(|c| - th, 0)
__device__ __forceinline__ cf soft_threshold(cf c, float th, float& left) {
    const float mag = sqrtf(c.x * c.x + c.y * c.y);
    const float sc = mag > th ? (mag - th) / mag : 0.f;
    left = mag > th ? mag - th : 0.f;
    return mk(c.x * sc, c.y * sc);
}

// v [q] summed over the kSolveThreads threads of a workgroup, for thread 0 alone: wave sums, then the four waves pairwise.  Every thread
// calls it (it holds a barrier); red: 4 N floats of LDS.
template <int N>
__device__ __forceinline__ void block_sums(float (&v)[N], float* red, int tid) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = wave_sum(v[q]);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) red[4 * q + (tid >> 6)] = v[q];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = (red[4 * q] + red[4 * q + 1]) + (red[4 * q + 2] + red[4 * q + 3]);
    }
}

// The record of a workgroup of a (gridDim.x, gridDim.y) launch: the N <= 4 sums of block_sums and zeros, 4 floats at the workgroup's
// place in part.  solve_record_kernel adds the records of a launch in a fixed order.
template <int N>
__device__ __forceinline__ void block_record(float (&v)[N], float* red, float* part, int tid) {
    block_sums(v, red, tid);
    if (tid == 0) {
        float* o = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 4;
#pragma unroll
        for (int q = 0; q < N; ++q) o[q] = v[q];
#pragma unroll
        for (int q = N; q < 4; ++q) o[q] = 0.f;
    }
}

// ------------------------------------------------------------------ host
inline size_t solve_align(size_t n) { return (n + 255) & ~(size_t)255; }
inline bool solve_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// hipFuncAttributeMaxDynamicSharedMemorySize is per device: raise it once per (kernel, device) and keep the result
static int large_lds_opt_in(const void* kern, const char* what, std::once_flag* once, hipError_t* status) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    CINE_REQUIRE(dev >= 0 && dev < 64, CINE_EUNSUPPORTED, "%s: device index %d", what, dev);
    std::call_once(once[dev], [&] { status[dev] = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    CINE_REQUIRE(status[dev] == hipSuccess, CINE_EHIP, "%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize): %s", what, hipGetErrorString(status[dev]));
    return CINE_OK;
}

// what every prox kernel with b on grid.y refuses about (b, t, h, w); grid_x: its workgroups per batch element
inline int solve_sizes(const char* what, int b, int t, int h, int w, int max_t, long grid_x) {
    CINE_REQUIRE(b > 0 && t > 0 && h > 0 && w > 0, CINE_EINVAL, "%s: bad sizes", what);
    CINE_REQUIRE(t >= 2 && t <= max_t, CINE_EUNSUPPORTED, "%s: %d frames, 2 .. %d are supported", what, t, max_t);
    CINE_REQUIRE(b <= 65535, CINE_EUNSUPPORTED, "%s: b > 65535", what);
    CINE_REQUIRE(grid_x <= 2147483647L, CINE_EUNSUPPORTED, "%s: h*w too large", what);
    return CINE_OK;
}

// The one rule about aliasing: no output is an operand, another output or ws, and ws is no operand.  Null entries (an optional output
// or operand that is absent, no ws) are skipped.
template <int NO, int NI>
inline bool solve_no_alias(const void* const (&outs)[NO], const void* const (&ins)[NI], const void* ws) {
    bool ok = true;
    for (int i = 0; i < NO; ++i) {
        if (!outs[i]) continue;
        ok = ok && outs[i] != ws;
        for (int j = 0; j < NI; ++j) ok = ok && outs[i] != ins[j];
        for (int j = 0; j < i; ++j) ok = ok && outs[i] != outs[j];
    }
    for (int j = 0; ws && j < NI; ++j) ok = ok && ws != ins[j];
    return ok;
}

// scratch of the operator behind solve_gradient: the row operator for mask_w == 1, the plane operator for mask_w == w
inline size_t dc_ws_bytes(int mask_w, int b, int t, int c, int h, int w) {
    return mask_w == 1 ? cine_image_dc_ws_bytes(b, t, c, h, w) : cine_image_dc_general_ws_bytes(b, t, c, h, w);
}

// g = A^H M A x_k - zf by cine_image_dc_t / cine_image_dc_general with weights (1, 0, -1).  A refusal of the operator (of a size: it
// comes before its first launch) is returned with its message behind `what`.
int solve_gradient(const char* what, const float* x_k, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask,
                   int mask_w, float* g, int b, int t, int c, int h, int w, void* op_ws, size_t op_bytes, void* stream);

// rows of nblk 4-float records each -> rec (rows, 4); with info (rows, nb, 4) and resid (rows), L+S's: see solve_kernels.hip
int solve_record_launch(const float* part, long nblk, float* rec, int rows, hipStream_t st, const double* info = nullptr, int nb = 0,
                        double* resid = nullptr);

// Carves a workspace into parts that each begin on a 256-byte boundary.  base == NULL: nothing is pointed at, the sizes alone are
// added up (the *_ws_bytes functions).  end: the bytes used so far -- the last part is not padded.
struct WsCursor {
    unsigned char* base;
    size_t at = 0, end = 0;
    template <typename T> T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        end = at + bytes;
        at = solve_align(end);
        return p;
    }
};

}  // namespace cine
