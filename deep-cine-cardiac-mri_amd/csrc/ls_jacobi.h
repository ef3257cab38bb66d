// ls_jacobi.h -- what the two singular-value-thresholding files share (ls_kernels.hip: one Casorati matrix per batch element;
// llr_kernels.hip: one per spatial block) and the coil-compression matrix (coil_kernels.hip): the limits, the upper-triangle indexing of
// a Gram matrix, and the cyclic Jacobi eigensolver for a complex Hermitian matrix in LDS.
#pragma once
#include "common.h"

namespace cine {

constexpr int kLsMaxT = 64;
constexpr int kLsThreads = 256;
constexpr int kLsMaxSweeps = 40;
constexpr double kLsJacobiTol = 1e-14;
constexpr int kLsRotDoubles = (kLsMaxT / 2) * 8;            // ls_jacobi's rot: c, s, e^{i phi}, the new diagonal pair, on / off per pair
constexpr int kLsRedDoubles = 2 * kLsThreads;               // ls_jacobi's red

__host__ __device__ __forceinline__ int ls_row_start(int i, int t) { return i * t - i * (i - 1) / 2; }

// entry p of the row-major upper triangle -> (i, j), i <= j
__device__ __forceinline__ void ls_pair_of(int p, int t, int& i, int& j) {
    int r = 0;
    while (r + 1 < t && ls_row_start(r + 1, t) <= p) ++r;
    i = r;
    j = r + (p - ls_row_start(r, t));
}

// round r of the round-robin schedule on n (even) players, pair k: player n - 1 stays, the others rotate
__device__ __forceinline__ void ls_round_pair(int n, int r, int k, int& p, int& q) {
    const int m = n - 1;
    int x, y;
    if (k == 0) { x = m; y = r; }
    else { x = (r + k) % m; y = (r - k + m) % m; }
    p = x < y ? x : y;
    q = x < y ? y : x;
}

// max that keeps a NaN once it has seen one
__device__ __forceinline__ double ls_nanmax(double m, double v) { return (v > m || v != v) ? v : m; }

// Cyclic Jacobi for the complex Hermitian A [T][T] in LDS, by all kLsThreads threads of a workgroup: round-robin pairs (the T / 2
// rotations of a round are disjoint: column phase, barrier, row phase), until max |off-diagonal| <= kLsJacobiTol max |diagonal| or
// kLsMaxSweeps sweeps.  V [T][T] takes the product of the rotations (the caller sets it to the identity; columns = eigenvectors), A ends
// with the eigenvalues on its diagonal.  rot: kLsRotDoubles, red: kLsRedDoubles doubles of LDS.  A and V must be visible to the workgroup
// (a barrier after they were written).  Returns the sweeps used; off, diag: the largest |off-diagonal| and |diagonal| reached.
__device__ __forceinline__ int ls_jacobi(double2* A, double2* V, double* rot, double* red, int T, int tid, double& off, double& diag) {
    const int n = (T + 1) & ~1, nh = n >> 1;
    off = 0.0; diag = 0.0;
    int sweeps = 0;
    for (int sweep = 0; sweep <= kLsMaxSweeps; ++sweep) {     // bounded: a NaN never satisfies the test and ends at the cap
        double mo = 0.0, md = 0.0;
        for (int e = tid; e < T * T; e += kLsThreads) {
            const int i = e / T, j = e - i * T;
            const double2 v = A[e];
            if (i == j) md = ls_nanmax(md, fabs(v.x));
            else mo = ls_nanmax(mo, hypot(v.x, v.y));
        }
        red[tid] = mo; red[kLsThreads + tid] = md;
        __syncthreads();
        for (int st = kLsThreads / 2; st > 0; st >>= 1) {
            if (tid < st) {
                red[tid] = ls_nanmax(red[tid], red[tid + st]);
                red[kLsThreads + tid] = ls_nanmax(red[kLsThreads + tid], red[kLsThreads + tid + st]);
            }
            __syncthreads();
        }
        off = red[0]; diag = red[kLsThreads];
        __syncthreads();
        sweeps = sweep;
        if (off <= kLsJacobiTol * diag || sweep == kLsMaxSweeps) break;
        for (int r = 0; r < n - 1; ++r) {
            if (tid < nh) {                                   // the rotation of pair tid from the 2 x 2 block [[al, be], [conj(be), ga]]
                int p, q;
                ls_round_pair(n, r, tid, p, q);
                double* o = rot + tid * 8;
                o[6] = 0.0;
                if (q < T) {
                    const double al = A[p * T + p].x, ga = A[q * T + q].x;
                    const double2 be = A[p * T + q];
                    const double bm = hypot(be.x, be.y);
                    // an element a tenth of the stopping bar below its own diagonal pair is left alone: inside a cluster of equal
                    // eigenvalues its rotation would be 45 degrees of noise, which slows the sweeps to linear convergence
                    if (!(bm <= 0.1 * kLsJacobiTol * sqrt(fabs(al * ga)))) {
                        // t = sgn(d) / (|z| + sqrt(1 + z^2)), z = d / (2 |be|), written without z: no overflow for a tiny |be|, no 0 / 0
                        const double d = ga - al;
                        const double tt = (d < 0.0 ? -2.0 : 2.0) * bm / (fabs(d) + hypot(d, 2.0 * bm));
                        const double c = 1.0 / sqrt(1.0 + tt * tt);
                        o[0] = c; o[1] = c * tt; o[2] = be.x / bm; o[3] = be.y / bm;
                        o[4] = al - tt * bm; o[5] = ga + tt * bm; o[6] = 1.0;
                    }
                }
            }
            __syncthreads();
            // columns: M <- M J for M = A and V, J = [[c, s], [-s e^{-i phi}, c e^{-i phi}]] on (p, q); the pair on the lanes
            for (int it = tid; it < nh * T * 2; it += kLsThreads) {
                const int k = it % nh, rest = it / nh;
                const int row = rest % T;
                const double* o = rot + k * 8;
                if (o[6] == 0.0) continue;
                int p, q;
                ls_round_pair(n, r, k, p, q);
                double2* M = rest >= T ? V : A;
                const double c = o[0], s = o[1], ex = o[2], ey = o[3];
                const double2 x = M[row * T + p], y = M[row * T + q];
                const double yx = ex * y.x + ey * y.y, yy = ex * y.y - ey * y.x;          // e^{-i phi} y
                M[row * T + p] = make_double2(c * x.x - s * yx, c * x.y - s * yy);
                M[row * T + q] = make_double2(s * x.x + c * yx, s * x.y + c * yy);
            }
            __syncthreads();
            // rows: A <- J^H A; the 2 x 2 block itself takes its closed form (zero off the diagonal, a real diagonal)
            for (int it = tid; it < nh * T; it += kLsThreads) {
                const int k = it / T, col = it - k * T;
                const double* o = rot + k * 8;
                if (o[6] == 0.0) continue;
                int p, q;
                ls_round_pair(n, r, k, p, q);
                const double c = o[0], s = o[1], ex = o[2], ey = o[3];
                const double2 x = A[p * T + col], y = A[q * T + col];
                const double yx = ex * y.x - ey * y.y, yy = ex * y.y + ey * y.x;          // e^{i phi} y
                double2 xn = make_double2(c * x.x - s * yx, c * x.y - s * yy);
                double2 yn = make_double2(s * x.x + c * yx, s * x.y + c * yy);
                if (col == p) { xn = make_double2(o[4], 0.0); yn = make_double2(0.0, 0.0); }
                if (col == q) { xn = make_double2(0.0, 0.0); yn = make_double2(o[5], 0.0); }
                A[p * T + col] = xn;
                A[q * T + col] = yn;
            }
            __syncthreads();
        }
    }
    return sweeps;
}

}  // namespace cine
