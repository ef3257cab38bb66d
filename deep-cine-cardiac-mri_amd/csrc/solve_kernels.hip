// solve_kernels.hip -- the host half of solve.h that is more than a line, and the record reduction of the proximal solvers.
#include <string>
#include "solve.h"
#include "ls_jacobi.h"

namespace cine {

// rows of nblk records each -> rec (rows, 4): the records of a row added in float64 in a fixed order (one workgroup per row; thread q
// takes records q, q + 256, ..., then a tree).  With info (rows, nb, 4), L+S's: column 3 = the nuclear norms of the row added over the
// batch instead, and resid (rows) = the worst Jacobi residual of the row.
__global__ __launch_bounds__(256) void solve_record_kernel(const float* part, long nblk, float* rec, const double* info, int nb, double* resid) {
    __shared__ double red[4][256];
    const int tid = threadIdx.x;
    const float* p = part + (long)blockIdx.x * nblk * 4;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long e = tid; e < nblk; e += 256) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += (double)p[e * 4 + q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) red[q][tid] = s[q];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double last = red[3][0], worst = 0.0;
        if (info) {
            const double* f = info + (long)blockIdx.x * nb * 4;
            last = 0.0;
            for (int i = 0; i < nb; ++i) { last += f[i * 4 + 1]; worst = ls_nanmax(worst, f[i * 4 + 2]); }
            if (resid) resid[blockIdx.x] = worst;
        }
        float* o = rec + (long)blockIdx.x * 4;
        o[0] = (float)red[0][0]; o[1] = (float)red[1][0]; o[2] = (float)red[2][0]; o[3] = (float)last;
    }
}

int solve_record_launch(const float* part, long nblk, float* rec, int rows, hipStream_t st, const double* info, int nb, double* resid) {
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(solve_record_kernel, dim3(rows), dim3(256), 0, st, part, nblk, rec, info, nb, resid);
    return check_launch("solve_record_kernel");
}

int solve_gradient(const char* what, const float* x_k, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask,
                   int mask_w, float* g, int b, int t, int c, int h, int w, void* op_ws, size_t op_bytes, void* stream) {
    const int e = mask_w == 1 ? cine_image_dc_t(x_k, sens, sens_tiled, zf, mask, nullptr, 1.f, 0.f, -1.f, g, b, t, c, h, w, 0, op_ws, op_bytes, stream)
                              : cine_image_dc_general(x_k, sens, zf, mask, nullptr, 1.f, 0.f, -1.f, g, b, t, c, h, w, 0, op_ws, op_bytes, stream);
    if (e) {
        const std::string why = cine_last_error();
        set_error("%s: %s", what, why.c_str());
    }
    return e;
}

}  // namespace cine
