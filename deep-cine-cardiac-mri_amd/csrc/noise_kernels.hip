// noise_kernels.hip -- noise propagation by the pseudo multiple replica method (Robson et al., MRM 60:895, 2008); no reference
// counterpart (the reference has no noise model):
//   cine_noise_add       : out = kspace + eta at the sampled points, eta complex normal with covariance scale^2 L L^H, drawn from
//                          Philox4x32-10 keyed by (seed, replica, k-space point, coil) -- philox.h, the definition in include/cine_hip.h
//   cine_noise_add_raw   : the same values on raw data (t, nx, ny, c), coil fastest, in front of the front-end
//   cine_replica_accum   : Welford's running mean / sum of squared deviations over the replicas, float64
//   cine_replica_finish  : mean, standard deviation, SNR and g-factor maps from the two
// One pass over the sampled points.  A workgroup owns 64 consecutive points of one row (lanes along w, 8-byte accesses, a wave reads
// 512 contiguous bytes per coil) and has four waves, one per coil group: wave g draws the normals of the coil pairs j = g, g + 4, ...
// into LDS (z[coil][point]: conflict-free), and after the one barrier forms eta of the coils i = g, g + 4, ... from them with L read
// from LDS (the same address over the wave).  The kernel is bound by its arithmetic (the 64-bit multiplies of Philox, logf and
// sincospif), not by memory or latency: one lane per point with all coils in the lane runs in the same time.
// White noise needs neither LDS nor the barrier.  A workgroup of a row the row mask leaves out ends at once (in place) or copies it.
#include <climits>
#include "common.h"
#include "philox.h"

namespace cine {

constexpr int kNoiseMaxCoils = 64;

struct NoiseArgs {
    const float2* k; float2* out; const uint8_t* mask; const float2* chol; const long* replica_dev;
    float scale; long seed, replica; uint64_t point0;
    int mask_w, c, h, w;
};

constexpr int kNoisePoints = 64, kNoiseGroups = 4, kNoiseThreads = kNoisePoints * kNoiseGroups;

__global__ __launch_bounds__(kNoiseThreads) void noise_add_kernel(NoiseArgs a) {
    extern __shared__ float2 noise_lds[];                    // with chol: L (c x c), then z[c][64]
    const int tid = threadIdx.x, pt = tid & (kNoisePoints - 1), g = tid / kNoisePoints, c = a.c, h = a.h, w = a.w;
    const long row = blockIdx.x;                             // frame * h + y
    const int x = blockIdx.y * kNoisePoints + pt;
    const long frame = row / h;
    const int y = (int)(row - frame * h);
    const long plane = (long)h * w;
    const long first = (frame * c * h + y) * (long)w + x;    // coil 0 of this lane's point; coil i is i * plane further
    const bool inplace = a.out == a.k, live = x < w;
    if (a.mask && a.mask_w == 1 && !a.mask[row]) {           // the whole row is not sampled (uniform over the workgroup)
        if (!inplace && live)
            for (int i = g; i < c; i += kNoiseGroups) a.out[first + i * plane] = a.k[first + i * plane];
        return;
    }
    const bool on = live && !(a.mask && a.mask_w != 1 && !a.mask[row * w + x]);
    const long replica = a.replica_dev ? *a.replica_dev : a.replica;
    const uint64_t p = a.point0 + (uint64_t)(row * w + x);
    const float scale = a.scale;
    if (!a.chol) {                                           // white: eta_i = scale z_i
        if (!live) return;
        if (!on) {
            if (!inplace)
                for (int i = g; i < c; i += kNoiseGroups) a.out[first + i * plane] = a.k[first + i * plane];
            return;
        }
        for (int j = g; 2 * j < c; j += kNoiseGroups) {
            const Philox4 v = philox_point(a.seed, replica, p, j);
            const PhiloxNormal z0 = philox_normal(v.x[0], v.x[1]);
            const long e0 = first + 2 * j * plane;
            const float2 k0 = a.k[e0];
            const float er0 = scale * z0.re, ei0 = scale * z0.im;
            a.out[e0] = make_float2(k0.x + er0, k0.y + ei0);
            if (2 * j + 1 < c) {
                const PhiloxNormal z1 = philox_normal(v.x[2], v.x[3]);
                const float2 k1 = a.k[e0 + plane];
                const float er1 = scale * z1.re, ei1 = scale * z1.im;
                a.out[e0 + plane] = make_float2(k1.x + er1, k1.y + ei1);
            }
        }
        return;
    }
    const float2* L = noise_lds;
    float2* z = noise_lds + (long)c * c;
    for (int i = tid; i < c * c; i += kNoiseThreads) noise_lds[i] = a.chol[i];
    if (on)
        for (int j = g; 2 * j < c; j += kNoiseGroups) {
            const Philox4 v = philox_point(a.seed, replica, p, j);
            const PhiloxNormal z0 = philox_normal(v.x[0], v.x[1]);
            z[(2 * j) * kNoisePoints + pt] = make_float2(z0.re, z0.im);
            if (2 * j + 1 < c) {
                const PhiloxNormal z1 = philox_normal(v.x[2], v.x[3]);
                z[(2 * j + 1) * kNoisePoints + pt] = make_float2(z1.re, z1.im);
            }
        }
    __syncthreads();                                         // L and the normals of every coil of the 64 points
    if (!live) return;
    if (!on) {
        if (!inplace)
            for (int i = g; i < c; i += kNoiseGroups) a.out[first + i * plane] = a.k[first + i * plane];
        return;
    }
    for (int i = g; i < c; i += kNoiseGroups) {
        const float2 kv = a.k[first + i * plane];            // issued ahead of the chain it is added to
        float re = 0.f, im = 0.f;
        for (int kk = 0; kk <= i; ++kk) {
            const float2 l = L[i * c + kk], zz = z[kk * kNoisePoints + pt];
            PhiloxNormal zn;
            zn.re = zz.x; zn.im = zz.y;
            philox_cfma(re, im, l.x, l.y, zn);
        }
        const float er = scale * re, ei = scale * im;
        a.out[first + i * plane] = make_float2(kv.x + er, kv.y + ei);
    }
}

// The same noise on the raw layout (t, nx, ny, c) with the coil index fastest.  Lanes along the points with a coil stride of one
// element would store 8 bytes at a stride of 8 c, so the values go through LDS: a workgroup owns 64 consecutive flat points, whose
// 64 c values are ONE contiguous span.  Phases one and two are those of noise_add_kernel (wave g draws the pairs g, g + 4, ... into
// z[coil][point], then lane = point forms eta_i, i = g, g + 4, ..., in registers); L and z are dead after the chain, so behind a
// barrier the etas are written over them as eta[point][coil] with the row padded to an odd number of 8-byte words (lanes along the
// points: conflict-free), and behind another the four waves walk the span, consecutive lanes on consecutive elements.  The span's
// values are loaded into registers in that order before anything else, so their latency lies under the arithmetic.  A run may
// straddle lines and frames: the mask is looked up per point, and the ballot of the 64 flags is the same in every wave.
struct NoiseRawArgs {
    const float2* raw; float2* out; const uint8_t* mask; const float2* chol; const long* replica_dev;
    float scale, inv_c; long seed, replica; uint64_t point0; long npoints;
    int mask_ny, c, ny;
};

// kSlots: the coils a lane holds between the two barriers and the span elements it holds from the start, 8 up to 32 coils and 16 up to
// 64 (where the LDS, not the registers, bounds the residency).
template <int kSlots>
__global__ __launch_bounds__(kNoiseThreads) void noise_add_raw_kernel(NoiseRawArgs a) {
    extern __shared__ float2 noise_lds[];                    // with chol: L (c x c), then z[c][64]; then eta[64][c | 1] over both
    const int tid = threadIdx.x, pt = tid & (kNoisePoints - 1), g = tid / kNoisePoints, c = a.c, cs = c | 1;
    const long base = (long)blockIdx.x * kNoisePoints;       // the first flat point (frame * nx + x) * ny + y of the run
    const long q = base + pt;
    const long left = a.npoints - base;
    const int count = (int)(left < kNoisePoints ? left : kNoisePoints) * c;       // elements of the span
    const long span = base * c;
    const bool inplace = a.out == a.raw;
    bool on = q < a.npoints;
    if (on && a.mask) on = a.mask[a.mask_ny == 1 ? (long)((uint64_t)q / (uint32_t)a.ny) : q] != 0;
    const unsigned long long flags = __ballot(on);           // lane = point in every wave: uniform over the workgroup
    if (!flags) {                                            // nothing sampled in the run
        if (!inplace)
            for (int e = tid; e < count; e += kNoiseThreads) a.out[span + e] = a.raw[span + e];
        return;
    }
    // the lane's elements of the span, loaded ahead of the arithmetic they are added to (in place: the sampled ones only)
    // e / c for e < 64 * 64, c <= 64: (e + 0.5) / c is at least 1 / 128 away from an integer, the two roundings move it by < 1e-5
    const float inv_c = a.inv_c;
    float2 kv[kSlots];
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int e = tid + s * kNoiseThreads;
        kv[s] = make_float2(0.f, 0.f);
        if (e < count && (!inplace || ((flags >> (int)(((float)e + 0.5f) * inv_c)) & 1))) kv[s] = a.raw[span + e];
    }
    const long replica = a.replica_dev ? *a.replica_dev : a.replica;
    const uint64_t p = a.point0 + (uint64_t)q;
    const float scale = a.scale;
    float2* eta = noise_lds;
    if (!a.chol) {                                           // white: eta_i = scale z_i
        if (on)
            for (int j = g; 2 * j < c; j += kNoiseGroups) {
                const Philox4 v = philox_point(a.seed, replica, p, j);
                const PhiloxNormal z0 = philox_normal(v.x[0], v.x[1]);
                const float er0 = scale * z0.re, ei0 = scale * z0.im;
                eta[pt * cs + 2 * j] = make_float2(er0, ei0);
                if (2 * j + 1 < c) {
                    const PhiloxNormal z1 = philox_normal(v.x[2], v.x[3]);
                    const float er1 = scale * z1.re, ei1 = scale * z1.im;
                    eta[pt * cs + 2 * j + 1] = make_float2(er1, ei1);
                }
            }
    } else {
        const float2* L = noise_lds;
        float2* z = noise_lds + c * c;
        for (int i = tid; i < c * c; i += kNoiseThreads) noise_lds[i] = a.chol[i];
        if (on)
            for (int j = g; 2 * j < c; j += kNoiseGroups) {
                const Philox4 v = philox_point(a.seed, replica, p, j);
                const PhiloxNormal z0 = philox_normal(v.x[0], v.x[1]);
                z[(2 * j) * kNoisePoints + pt] = make_float2(z0.re, z0.im);
                if (2 * j + 1 < c) {
                    const PhiloxNormal z1 = philox_normal(v.x[2], v.x[3]);
                    z[(2 * j + 1) * kNoisePoints + pt] = make_float2(z1.re, z1.im);
                }
            }
        __syncthreads();                                     // L and the normals of every coil of the 64 points
        float2 mine[kSlots];
#pragma unroll
        for (int s = 0; s < kSlots; ++s) {
            const int i = g + s * kNoiseGroups;
            float re = 0.f, im = 0.f;
            if (on && i < c)
                for (int kk = 0; kk <= i; ++kk) {
                    const float2 l = L[i * c + kk], zz = z[kk * kNoisePoints + pt];
                    PhiloxNormal zn;
                    zn.re = zz.x; zn.im = zz.y;
                    philox_cfma(re, im, l.x, l.y, zn);
                }
            const float er = scale * re, ei = scale * im;
            mine[s] = make_float2(er, ei);
        }
        __syncthreads();                                     // L and z are read: eta goes over them
        if (on) {
#pragma unroll
            for (int s = 0; s < kSlots; ++s) {
                const int i = g + s * kNoiseGroups;
                if (i < c) eta[pt * cs + i] = mine[s];
            }
        }
    }
    __syncthreads();                                         // eta[point][coil] of the sampled points
#pragma unroll
    for (int s = 0; s < kSlots; ++s) {
        const int e = tid + s * kNoiseThreads;
        if (e < count) {
            const int ep = (int)(((float)e + 0.5f) * inv_c), coil = e - ep * c;
            if ((flags >> ep) & 1) {
                const float2 et = eta[ep * cs + coil];
                a.out[span + e] = make_float2(kv[s].x + et.x, kv[s].y + et.y);
            } else if (!inplace) {
                a.out[span + e] = kv[s];
            }
        }
    }
}

__global__ void replica_accum_kernel(const float* x, double* mean, double* m2, long n, int k) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const double v = (double)x[e];
        if (k == 1) {                                        // initialises: the buffers are not read
            mean[e] = v; m2[e] = 0.0;
        } else {
            double m = mean[e];
            const double d = v - m;
            m += d / (double)k;
            mean[e] = m;
            m2[e] += d * (v - m);
        }
    }
}

struct FinishArgs {
    const double* mean; const double* m2; const float* ref_std;
    float* mean_out; float* std_out; float* snr_out; float* g_out;
    long ne; int k, pairs; float accel;
};

__global__ void replica_finish_kernel(FinishArgs a) {
    const double inv = 1.0 / (double)(a.k - 1);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < a.ne; e += (long)gridDim.x * blockDim.x) {
        double var, mag, mean;
        if (a.pairs) {
            const double mr = a.mean[2 * e], mi = a.mean[2 * e + 1];
            var = a.m2[2 * e] * inv + a.m2[2 * e + 1] * inv;
            mag = mean = sqrt(mr * mr + mi * mi);
        } else {
            mean = a.mean[e];
            var = a.m2[e] * inv;
            mag = fabs(mean);
        }
        const double sd = sqrt(var);
        if (a.mean_out) a.mean_out[e] = (float)mean;
        if (a.std_out) a.std_out[e] = (float)sd;
        if (a.snr_out) a.snr_out[e] = sd == 0.0 ? 0.f : (float)(mag / sd);
        if (a.g_out) {
            const double rs = (double)a.ref_std[e];
            a.g_out[e] = rs == 0.0 ? 0.f : (float)(sd / (rs * sqrt((double)a.accel)));
        }
    }
}

static unsigned noise_grid1(long n, int threads, long cap = 4096) {
    long g = (n + threads - 1) / threads;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

static void noise_launch(const NoiseArgs& a, long rows, hipStream_t st) {
    // L and z[c][64] fit the 64 KB of LDS a launch gets without opting in: 32 KB + 32 KB at 64 coils
    const size_t lds = a.chol ? ((size_t)a.c * a.c + (size_t)a.c * kNoisePoints) * sizeof(float2) : 0;
    hipLaunchKernelGGL(noise_add_kernel, dim3((unsigned)rows, (unsigned)ceil_div(a.w, kNoisePoints)), dim3(kNoiseThreads), lds, st, a);
}

}  // namespace cine

using namespace cine;

extern "C" int cine_noise_add(const float* kspace, float* out, const uint8_t* mask, int mask_w, const float* chol, float scale,
                              long seed, long replica, const long* replica_dev, long point0, long bt, int c, int h, int w, void* stream) {
    const char* what = "cine_noise_add";
    CINE_REQUIRE(kspace && out, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(bt > 0 && c > 0 && h > 0 && w > 0, CINE_EINVAL, "%s: Invalid shapes bt %ld c %d h %d w %d", what, bt, c, h, w);
    CINE_REQUIRE(c <= kNoiseMaxCoils, CINE_EUNSUPPORTED, "%s: %d coils, at most %d", what, c, kNoiseMaxCoils);
    CINE_REQUIRE(bt <= INT_MAX / h, CINE_EUNSUPPORTED, "%s: bt * h = %ld * %d rows, at most %d", what, bt, h, INT_MAX);
    CINE_REQUIRE(mask_w == 1 || mask_w == w, CINE_EINVAL, "%s: mask_w %d is neither 1 nor w = %d", what, mask_w, w);
    CINE_REQUIRE(replica >= 0 && replica <= 0xffffffffL, CINE_EINVAL, "%s: replica %ld outside [0, 2^32)", what, replica);
    CINE_REQUIRE(point0 >= 0, CINE_EINVAL, "%s: point0 %ld is negative", what, point0);
    CINE_REQUIRE(((uintptr_t)kspace | (uintptr_t)out | (uintptr_t)chol) % 8 == 0, CINE_EINVAL, "%s: kspace, out and chol must be 8-byte aligned", what);
    CINE_REQUIRE(!replica_dev || (uintptr_t)replica_dev % 8 == 0, CINE_EINVAL, "%s: replica_dev must be 8-byte aligned", what);
    const size_t bytes = (size_t)bt * c * h * w * 2 * sizeof(float);
    const uintptr_t k0 = (uintptr_t)kspace, o0 = (uintptr_t)out;
    CINE_REQUIRE(k0 == o0 || k0 + bytes <= o0 || o0 + bytes <= k0, CINE_EINVAL, "%s: out overlaps kspace without being kspace", what);
    NoiseArgs a;
    a.k = reinterpret_cast<const float2*>(kspace); a.out = reinterpret_cast<float2*>(out); a.mask = mask;
    a.chol = reinterpret_cast<const float2*>(chol); a.replica_dev = replica_dev;
    a.scale = scale; a.seed = seed; a.replica = replica; a.point0 = (uint64_t)point0;
    a.mask_w = mask ? mask_w : 1; a.c = c; a.h = h; a.w = w;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    const long rows = bt * h;
    noise_launch(a, rows, st);
    return check_launch("noise_add_kernel");
}

extern "C" int cine_noise_add_raw(const float* raw, float* out, const uint8_t* mask, int mask_ny, const float* chol, float scale,
                                  long seed, long replica, const long* replica_dev, long point0, long t, int nx, int ny, int c, void* stream) {
    const char* what = "cine_noise_add_raw";
    constexpr long kMaxPoints = (long)INT_MAX * kNoisePoints;                // one workgroup per 64 points, the grid's x limit
    CINE_REQUIRE(raw && out, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(t > 0 && nx > 0 && ny > 0 && c > 0, CINE_EINVAL, "%s: Invalid shapes t %ld nx %d ny %d c %d", what, t, nx, ny, c);
    CINE_REQUIRE(c <= kNoiseMaxCoils, CINE_EUNSUPPORTED, "%s: %d coils, at most %d", what, c, kNoiseMaxCoils);
    CINE_REQUIRE(t <= kMaxPoints / ((long)nx * ny), CINE_EUNSUPPORTED, "%s: t * nx * ny = %ld * %d * %d points, at most %ld", what, t, nx, ny,
                 kMaxPoints);
    CINE_REQUIRE(mask_ny == 1 || mask_ny == ny, CINE_EINVAL, "%s: mask_ny %d is neither 1 nor ny = %d", what, mask_ny, ny);
    CINE_REQUIRE(replica >= 0 && replica <= 0xffffffffL, CINE_EINVAL, "%s: replica %ld outside [0, 2^32)", what, replica);
    CINE_REQUIRE(point0 >= 0, CINE_EINVAL, "%s: point0 %ld is negative", what, point0);
    CINE_REQUIRE(((uintptr_t)raw | (uintptr_t)out | (uintptr_t)chol) % 8 == 0, CINE_EINVAL, "%s: raw, out and chol must be 8-byte aligned", what);
    CINE_REQUIRE(!replica_dev || (uintptr_t)replica_dev % 8 == 0, CINE_EINVAL, "%s: replica_dev must be 8-byte aligned", what);
    const long npoints = t * nx * ny;
    const size_t bytes = (size_t)npoints * c * 2 * sizeof(float);
    const uintptr_t r0 = (uintptr_t)raw, o0 = (uintptr_t)out;
    CINE_REQUIRE(r0 == o0 || r0 + bytes <= o0 || o0 + bytes <= r0, CINE_EINVAL, "%s: out overlaps raw without being raw", what);
    NoiseRawArgs a;
    a.raw = reinterpret_cast<const float2*>(raw); a.out = reinterpret_cast<float2*>(out); a.mask = mask;
    a.chol = reinterpret_cast<const float2*>(chol); a.replica_dev = replica_dev;
    a.scale = scale; a.inv_c = 1.0f / (float)c; a.seed = seed; a.replica = replica; a.point0 = (uint64_t)point0; a.npoints = npoints;
    a.mask_ny = mask ? mask_ny : 1; a.c = c; a.ny = ny;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    // eta[64][c | 1] lies over L and z[c][64]: 64 KB at 64 coils, what a launch gets without opting in
    const size_t eta = (size_t)kNoisePoints * (c | 1), chain = chol ? (size_t)c * c + (size_t)c * kNoisePoints : 0;
    const dim3 grid((unsigned)ceil_div(npoints, (long)kNoisePoints));
    const size_t lds = (eta > chain ? eta : chain) * sizeof(float2);
    if (c <= 8 * kNoiseGroups)
        hipLaunchKernelGGL(noise_add_raw_kernel<8>, grid, dim3(kNoiseThreads), lds, st, a);
    else
        hipLaunchKernelGGL(noise_add_raw_kernel<16>, grid, dim3(kNoiseThreads), lds, st, a);
    return check_launch("noise_add_raw_kernel");
}

extern "C" int cine_replica_accum(const float* x, double* mean, double* m2, long n, int k, void* stream) {
    const char* what = "cine_replica_accum";
    CINE_REQUIRE(x && mean && m2, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(n > 0 && k >= 1, CINE_EINVAL, "%s: n %ld, k %d (n > 0, k >= 1)", what, n, k);
    CINE_REQUIRE(mean != m2, CINE_EINVAL, "%s: mean and m2 are aliased", what);
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(replica_accum_kernel, dim3(noise_grid1(n, 256)), dim3(256), 0, st, x, mean, m2, n, k);
    return check_launch("replica_accum_kernel");
}

extern "C" int cine_replica_finish(const double* mean, const double* m2, long n, int k, int pairs, const float* ref_std, float accel,
                                   float* mean_out, float* std_out, float* snr_out, float* g_out, void* stream) {
    const char* what = "cine_replica_finish";
    CINE_REQUIRE(mean && m2, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(n > 0 && k >= 2, CINE_EINVAL, "%s: n %ld, k %d (n > 0, and at least two samples)", what, n, k);
    CINE_REQUIRE(!pairs || n % 2 == 0, CINE_EINVAL, "%s: pairs with an odd n = %ld", what, n);
    CINE_REQUIRE(!g_out || ref_std, CINE_EINVAL, "%s: g_out needs ref_std", what);
    CINE_REQUIRE(!g_out || accel > 0.f, CINE_EINVAL, "%s: g_out needs accel > 0, got %g", what, (double)accel);
    FinishArgs a;
    a.mean = mean; a.m2 = m2; a.ref_std = ref_std; a.mean_out = mean_out; a.std_out = std_out; a.snr_out = snr_out; a.g_out = g_out;
    a.ne = pairs ? n / 2 : n; a.k = k; a.pairs = pairs != 0; a.accel = accel;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(replica_finish_kernel, dim3(noise_grid1(a.ne, 256)), dim3(256), 0, st, a);
    return check_launch("replica_finish_kernel");
}
