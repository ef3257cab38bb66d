// gating_kernels.hip -- retrospective cardiac gating, the step in front of the raw path (SlicePipeline.submit_readouts).  No reference
// counterpart: the reference starts from binned HDF5 arrays.
//
//   cine_gate_readouts   out[r] = sum_j weight[j] * lines[index[j]], j in [row_ptr[r], row_ptr[r + 1]), in CSR order: a sparse matrix
//                        (rows = n_frames nx output lines, columns = the acquired readouts) times a dense matrix whose rows are whole
//                        readouts of row_elems = ny c complex samples.  The output is the (t, x, y, coil) array of cine_raw_ingest.
//                        A workgroup owns one chunk of one output line: 256 lanes x kSlots accesses of 16 bytes (8 where row_elems
//                        is odd or a base pointer sits on an odd element), consecutive lanes on consecutive accesses.  The row's few
//                        CSR entries are uniform over the workgroup (scalar loads); per entry every lane issues its kSlots loads of
//                        the contributing readout back to back, folds them into registers -- the first term one product, every
//                        further one an fmaf per real component -- and stores once.  A row without entries stores zeros, so every
//                        element of out is written and nothing has to be cleared.  Pure streaming: 8 bytes written per sample and
//                        8 k read; no LDS, no barrier, no atomics, and the order of the terms is the CSR order on every call.
#include <climits>
#include <cstdint>
#include <type_traits>
#include "common.h"

namespace cine {

namespace gate {
constexpr int kThreads = 256;
constexpr int kSlots = 2;                      // accesses a lane holds: 2 x 16 bytes in flight per contributing readout
}

struct GateArgs {
    const float2* lines; float2* out; const int* row_ptr; const int* index; const float* weight;
    long row_elems;                            // complex samples of a readout
    unsigned chunks;                           // workgroups per output line
};

// kVec: complex samples per access, 2 (16 bytes) or 1 (8 bytes)
template <int kVec>
__global__ __launch_bounds__(gate::kThreads) void gate_readouts_kernel(GateArgs a) {
    using V = typename std::conditional<kVec == 2, float4, float2>::type;
    constexpr int kChunk = gate::kThreads * gate::kSlots;                    // accesses of a chunk
    const unsigned row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks;
    const long nacc = a.row_elems / kVec;                                    // accesses of a line (kVec == 2: row_elems is even)
    const long first = (long)chunk * kChunk + threadIdx.x;
    const int j0 = a.row_ptr[row], j1 = a.row_ptr[row + 1];
    V acc[gate::kSlots];
#pragma unroll
    for (int s = 0; s < gate::kSlots; ++s) {
        if constexpr (kVec == 2) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        else acc[s] = make_float2(0.f, 0.f);
    }
    for (int j = j0; j < j1; ++j) {
        const float w = a.weight[j];
        const V* src = reinterpret_cast<const V*>(a.lines + (long)a.index[j] * a.row_elems);
        V x[gate::kSlots];
#pragma unroll
        for (int s = 0; s < gate::kSlots; ++s) {
            const long e = first + (long)s * gate::kThreads;
            if (e < nacc) x[s] = src[e];
            else if constexpr (kVec == 2) x[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            else x[s] = make_float2(0.f, 0.f);
        }
        if (j == j0) {
#pragma unroll
            for (int s = 0; s < gate::kSlots; ++s) {
                acc[s].x = __fmul_rn(w, x[s].x);
                acc[s].y = __fmul_rn(w, x[s].y);
                if constexpr (kVec == 2) {
                    acc[s].z = __fmul_rn(w, x[s].z);
                    acc[s].w = __fmul_rn(w, x[s].w);
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < gate::kSlots; ++s) {
                acc[s].x = fmaf(w, x[s].x, acc[s].x);
                acc[s].y = fmaf(w, x[s].y, acc[s].y);
                if constexpr (kVec == 2) {
                    acc[s].z = fmaf(w, x[s].z, acc[s].z);
                    acc[s].w = fmaf(w, x[s].w, acc[s].w);
                }
            }
        }
    }
    V* dst = reinterpret_cast<V*>(a.out + (long)row * a.row_elems);
#pragma unroll
    for (int s = 0; s < gate::kSlots; ++s) {
        const long e = first + (long)s * gate::kThreads;
        if (e < nacc) dst[e] = acc[s];
    }
}

}  // namespace cine

using namespace cine;

extern "C" int cine_gate_readouts(const float* lines, float* out, const int* row_ptr, const int* index, const float* weight,
                                  long n_lines, long rows, long row_elems, void* stream) {
    const char* what = "cine_gate_readouts";
    CINE_REQUIRE(lines && out && row_ptr && index && weight, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(rows > 0 && row_elems > 0 && n_lines >= 0, CINE_EINVAL, "%s: Invalid shapes rows %ld row_elems %ld n_lines %ld", what, rows,
                 row_elems, n_lines);
    CINE_REQUIRE(((uintptr_t)lines | (uintptr_t)out) % 8 == 0, CINE_EINVAL, "%s: lines and out must be 8-byte aligned", what);
    CINE_REQUIRE(((uintptr_t)row_ptr | (uintptr_t)index | (uintptr_t)weight) % 4 == 0, CINE_EINVAL,
                 "%s: row_ptr, index and weight must be 4-byte aligned", what);
    CINE_REQUIRE(row_elems <= LONG_MAX / 8 / rows && (n_lines == 0 || row_elems <= LONG_MAX / 8 / n_lines), CINE_EINVAL,
                 "%s: rows %ld (n_lines %ld) x row_elems %ld overflow a byte count", what, rows, n_lines, row_elems);
    const uintptr_t l0 = (uintptr_t)lines, o0 = (uintptr_t)out;
    const size_t lbytes = (size_t)n_lines * row_elems * 8, obytes = (size_t)rows * row_elems * 8;
    CINE_REQUIRE(l0 + lbytes <= o0 || o0 + obytes <= l0, CINE_EINVAL, "%s: out overlaps lines", what);
    // 16-byte accesses when every line of both arrays starts on a 16-byte boundary
    const bool wide = row_elems % 2 == 0 && (l0 | o0) % 16 == 0;
    const long nacc = wide ? row_elems / 2 : row_elems;
    const long chunks = ceil_div(nacc, (long)gate::kThreads * gate::kSlots);
    CINE_REQUIRE(chunks <= INT_MAX / rows, CINE_EUNSUPPORTED, "%s: %ld rows x %ld chunks of %d accesses exceed the grid limit %d workgroups",
                 what, rows, chunks, gate::kThreads * gate::kSlots, INT_MAX);
    GateArgs a;
    a.lines = reinterpret_cast<const float2*>(lines); a.out = reinterpret_cast<float2*>(out);
    a.row_ptr = row_ptr; a.index = index; a.weight = weight; a.row_elems = row_elems; a.chunks = (unsigned)chunks;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_PACK, st);
    const dim3 grid((unsigned)(rows * chunks));
    if (wide)
        hipLaunchKernelGGL(gate_readouts_kernel<2>, grid, dim3(gate::kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(gate_readouts_kernel<1>, grid, dim3(gate::kThreads), 0, st, a);
    return check_launch("gate_readouts_kernel");
}
