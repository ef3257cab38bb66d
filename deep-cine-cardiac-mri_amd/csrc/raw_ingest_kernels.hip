// raw_ingest_kernels.hip -- the first step of the in-flight front-end (SlicePipeline.submit_raw) for raw sizes the FFT line engines
// take: reference data/mri_data.py:283-289 scales the raw (t, x, y, coil) array of the HDF5 file and moves the coil axis in front of
// the image axes before the inverse transform.
//
//   cine_raw_ingest      out[t, k, x, y] = scale * raw[t, x, y, k], t < t_out: per frame a transpose of a (P = nx ny, c) complex matrix
//                        with the coil axis at unit stride into c planes of P samples.  A workgroup takes TP consecutive samples of
//                        one frame with all their coils: ONE contiguous run of raw (TP c complex) and, per coil, one contiguous run of
//                        TP complex of out.  TP is a multiple of 16 samples (128 bytes), so whenever P is a multiple of 16 -- every
//                        even matrix of practical size -- each 128-byte line of a coil plane is written whole by one workgroup.
//                        Both sides move 16 bytes per lane: the run of raw and each run of out start on an 8-byte boundary at least,
//                        an odd first (last) element is moved alone and everything between in aligned pairs, for any c and any ny.
//                        The tile is staged in LDS as [sample][ldc] float2 with ldc odd and >= c + 1; the row of sample p is shifted by
//                        one element when bit 5 of p is set.  A lane reads the two samples 2 j, 2 j + 1 of one coil as two 8-byte
//                        accesses: rows 2 j are 4 ldc dwords apart (16 distinct 4-bank slots for 16 lanes, ldc being odd) and the
//                        lanes j, j + 16 of a 32-lane group differ in bit 5 of the sample, which puts them on the two halves of a
//                        slot: the column reads do not collide (TP >= 32; at TP = 16, for more than 64 coils, up to 2-way).
//                        Pure streaming: 16 bytes per sample and coil, no reuse; up to 8 workgroups of 256 threads per CU keep
//                        the loads of other tiles in flight behind a tile's barrier.
#include <cstdint>
#include "common.h"

namespace cine {

namespace ri {
constexpr int kThreads = 256;
constexpr int kLdsBudget = 18 * 1024;          // bytes of LDS per workgroup: 8 workgroups per CU
}

struct IngestArgs {
    long P;                                    // samples per frame and coil (nx ny)
    long tiles_per_frame;                      // ceil(P / TP)
    int c, ldc, TP;
    float scale;
};

__device__ __forceinline__ int ingest_row(int p, int ldc) { return p * ldc + ((p >> 5) & 1); }

__global__ __launch_bounds__(ri::kThreads) void raw_ingest_kernel(const float2* __restrict__ raw, float2* __restrict__ out, IngestArgs g) {
    extern __shared__ __attribute__((aligned(16))) float2 ri_lds[];
    const int tid = threadIdx.x, c = g.c, ldc = g.ldc;
    const long t = (long)blockIdx.x / g.tiles_per_frame;
    const long p0 = ((long)blockIdx.x - t * g.tiles_per_frame) * g.TP;
    const int np = (int)(g.P - p0 < g.TP ? g.P - p0 : g.TP);
    const float s = g.scale;

    // in: elements [base, base + ne) of raw, as aligned pairs; slot q holds elements 2 q - hb and 2 q - hb + 1 of the run
    {
        const long base = (t * g.P + p0) * c;
        const int ne = np * c, hb = (int)(base & 1);
        const int nslots = (ne + hb + 1) >> 1;
        const float2* src = raw + base;
        for (int q = tid; q < nslots; q += ri::kThreads) {
            const int a0 = 2 * q - hb, a1 = a0 + 1;
            if (a0 >= 0 && a1 < ne) {
                const float4 v = *reinterpret_cast<const float4*>(src + a0);
                const int pa = a0 / c, ka = a0 - pa * c;
                const bool wrap = ka + 1 == c;
                ri_lds[ingest_row(pa, ldc) + ka] = make_float2(s * v.x, s * v.y);
                ri_lds[wrap ? ingest_row(pa + 1, ldc) : ingest_row(pa, ldc) + ka + 1] = make_float2(s * v.z, s * v.w);
            } else {
                const int a = a0 >= 0 ? a0 : a1;               // the odd element at either end of the run
                const float2 v = src[a];
                const int pa = a / c, ka = a - pa * c;
                ri_lds[ingest_row(pa, ldc) + ka] = make_float2(s * v.x, s * v.y);
            }
        }
    }
    __syncthreads();

    // out: per coil the run [dst0, dst0 + np) of its plane; slot j holds samples 2 j - ho and 2 j - ho + 1 of the tile
    {
        const int half = g.TP >> 1;                             // a power of two >= 8
        const int total = c * half;
        for (int e = tid; e < total; e += ri::kThreads) {
            const int k = e / half, j = e - k * half;
            const long dst0 = (t * c + k) * g.P + p0;
            const int ho = (int)(dst0 & 1);
            float2* dst = out + dst0;
            const int b0 = 2 * j - ho, b1 = b0 + 1;
            if (b0 >= 0 && b1 < np) {
                const float2 u = ri_lds[ingest_row(b0, ldc) + k], w = ri_lds[ingest_row(b1, ldc) + k];
                *reinterpret_cast<float4*>(dst + b0) = make_float4(u.x, u.y, w.x, w.y);
            } else {
                const int b = b0 >= 0 ? b0 : b1;
                if (b < np) dst[b] = ri_lds[ingest_row(b, ldc) + k];
            }
            // with ho = 1 the last sample of a full tile has no slot of its own (2 half - 1 = TP - 1 is slot `half`)
            if (ho && j == half - 1 && g.TP - 1 < np) dst[g.TP - 1] = ri_lds[ingest_row(g.TP - 1, ldc) + k];
        }
    }
}

}  // namespace cine

using namespace cine;

extern "C" int cine_raw_ingest(const float* raw, float* out, int t_in, int nx, int ny, int c, int t_out, float scale, void* stream) {
    CINE_REQUIRE(raw && out && raw != out, CINE_EINVAL, "cine_raw_ingest: null or aliased pointers");
    CINE_REQUIRE(t_in >= 1 && nx >= 1 && ny >= 1 && c >= 1 && t_out >= 1 && t_out <= t_in, CINE_EINVAL,
                 "cine_raw_ingest: Invalid shapes. (t_in %d, nx %d, ny %d, coils %d, t_out %d)", t_in, nx, ny, c, t_out);
    CINE_REQUIRE((reinterpret_cast<uintptr_t>(raw) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0, CINE_EINVAL,
                 "cine_raw_ingest: raw and out must be 16-byte aligned");
    IngestArgs g{};
    g.P = (long)nx * ny;
    g.c = c;
    g.ldc = (c + 1) | 1;
    g.scale = scale;
    // the widest tile of 16 .. 128 samples (a power of two) whose staged image stays inside the LDS budget; 16 samples at least
    g.TP = 128;
    while (g.TP > 16 && ((size_t)g.TP * g.ldc + 1) * sizeof(float2) > (size_t)ri::kLdsBudget) g.TP >>= 1;
    const size_t lds = ((size_t)g.TP * g.ldc + 1) * sizeof(float2);
    CINE_REQUIRE(lds <= 64 * 1024, CINE_EUNSUPPORTED, "cine_raw_ingest: %d coils need %zu bytes of LDS (limit 65536)", c, lds);
    g.tiles_per_frame = (g.P + g.TP - 1) / g.TP;
    const long wgs = g.tiles_per_frame * t_out;
    CINE_REQUIRE(wgs <= INT32_MAX, CINE_EUNSUPPORTED, "cine_raw_ingest: %ld workgroups exceed the grid limit %d", wgs, INT32_MAX);
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_PACK, st);
    hipLaunchKernelGGL(raw_ingest_kernel, dim3((unsigned)wgs), dim3(ri::kThreads), lds, st, reinterpret_cast<const float2*>(raw),
                       reinterpret_cast<float2*>(out), g);
    return check_launch("raw_ingest_kernel");
}
