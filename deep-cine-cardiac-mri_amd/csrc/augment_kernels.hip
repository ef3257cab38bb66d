// augment_kernels.hip -- training augmentation on the device (cine_hip.augment).  No reference counterpart: the reference has no
// augmentation.
//
//   cine_affine_warp     out[f, c] = in[g(f), c] resampled under one inverse affine map, g a cyclic shift / reversal of the frames.
//                        A workgroup owns a 32 x 8 tile of the output pixels of 4 (bilinear) or 2 (bicubic) planes of one frame: a lane
//                        owns one pixel, computes its source coordinate in float64 (two DFMAs per axis), the tap indices under the
//                        border rule and the float32 weights ONCE, issues the 16 / 32 8-byte loads of all its planes, then runs the
//                        fmaf chains and stores 8 bytes per plane -- 32 consecutive lanes on 256 consecutive bytes of an output row.
//                        (One workgroup per tile walking all 15 coils left 2 625 workgroups for 2 048 resident ones at 15 x 15 x 200
//                        x 200, a second round a quarter full, and one plane's loads in flight per lane.)  For the
//                        near-identity maps of an augmentation a tile's footprint is a slightly sheared tile of the source, whose
//                        lines the neighbouring lanes and tiles share through L1 / L2.  No LDS, no barrier, no atomics; the value
//                        of a pixel depends on its coordinates and taps only, never on the tile or the launch shape.
//
//   The chain: per tap row r (ascending) s_r = sum over the tap columns k (ascending) of wx[k] * v[r][k], an fmaf chain from 0; the
//   pixel is the fmaf chain from 0 of wy[r] * s_r over the rows.  Real and imaginary parts separately.  A tap outside the image under
//   border 0 enters as the value 0 (it is not read).  With weights (0, 1, 0, 0) / (1, 0) the pixel is its tap bit for bit (finite data).
#include <climits>
#include <cmath>
#include <cstdint>
#include "common.h"

namespace cine {

namespace warp {
constexpr int kTileW = 32, kTileH = 8;
constexpr int kThreads = kTileW * kTileH;
constexpr int kMaxSide = 4096;
constexpr double kMaxA = 1024.0, kMaxB = 1048576.0;     // |a| and |b| limits: every source coordinate then stays below 2^24
// planes of one frame a workgroup resamples, all their loads in flight at once: 4 x 4 (bilinear) or 2 x 16 (bicubic) 8-byte loads a lane
constexpr int chunk_of(int taps) { return taps == 2 ? 4 : 2; }
}

struct WarpArgs {
    const float2* in; float2* out;
    int frames, inner, h, w;
    double ayy, ayx, oy, axy, axx, ox;                   // oy = b_y + cy, ox = b_x + cx
    int t_shift, t_reverse;
    unsigned tiles_x, tiles_y, chunks;                   // chunks: workgroups per tile and frame, ceil(inner / chunk_of(taps))
};

// the cubic-convolution kernel with A = -0.75 on [0, 1] and on [1, 2]: exactly 1 and 0 at the integers
__device__ __forceinline__ float cubic_near(float x) { return fmaf(fmaf(1.25f, x, -2.25f) * x, x, 1.0f); }
__device__ __forceinline__ float cubic_far(float x) { return fmaf(fmaf(fmaf(-0.75f, x, 3.75f), x, -6.0f), x, 3.0f); }

template <int kTaps>
__device__ __forceinline__ void tap_weights(float f, float (&wt)[kTaps]) {
    if constexpr (kTaps == 2) {
        wt[0] = 1.0f - f; wt[1] = f;
    } else {
        wt[0] = cubic_far(1.0f + f); wt[1] = cubic_near(f); wt[2] = cubic_near(1.0f - f); wt[3] = cubic_far(2.0f - f);
    }
}

// The index a tap reads and whether it counts.  kReflect: half-sample symmetric reflection with period 2 n (always counts); otherwise
// the index clamped into the plane, counting only where it was inside.
template <bool kReflect>
__device__ __forceinline__ int tap_index(int i, int n, bool& ok) {
    if constexpr (kReflect) {
        const int p = 2 * n;
        int m = i % p;
        if (m < 0) m += p;
        ok = true;
        return m < n ? m : p - 1 - m;
    } else {
        ok = (unsigned)i < (unsigned)n;
        return min(max(i, 0), n - 1);
    }
}

// kTaps: 2 bilinear (taps from i0), 4 bicubic (taps from i0 - 1)
template <int kTaps, bool kReflect>
__global__ __launch_bounds__(warp::kThreads) void affine_warp_kernel(WarpArgs a) {
    constexpr int kChunk = warp::chunk_of(kTaps);
    unsigned b = blockIdx.x;
    const unsigned tx = b % a.tiles_x; b /= a.tiles_x;
    const unsigned ty = b % a.tiles_y; b /= a.tiles_y;
    const unsigned chunk = b % a.chunks;
    const unsigned f = b / a.chunks;
    const int xo = (int)(tx * warp::kTileW + (threadIdx.x % warp::kTileW));
    const int yo = (int)(ty * warp::kTileH + (threadIdx.x / warp::kTileW));
    if (xo >= a.w || yo >= a.h) return;
    // source frame: (f + t_shift) mod frames, or (t_shift - f) mod frames
    unsigned g;
    if (a.t_reverse) g = (unsigned)a.t_shift >= f ? (unsigned)a.t_shift - f : (unsigned)a.t_shift + (unsigned)a.frames - f;
    else { g = f + (unsigned)a.t_shift; if (g >= (unsigned)a.frames) g -= (unsigned)a.frames; }

    const double dy = (double)yo - 0.5 * (double)(a.h - 1), dx = (double)xo - 0.5 * (double)(a.w - 1);
    const double ys = fma(a.ayy, dy, fma(a.ayx, dx, a.oy));
    const double xs = fma(a.axy, dy, fma(a.axx, dx, a.ox));
    const double yfl = floor(ys), xfl = floor(xs);
    float wy[kTaps], wx[kTaps];
    tap_weights<kTaps>((float)(ys - yfl), wy);
    tap_weights<kTaps>((float)(xs - xfl), wx);
    const int iy = (int)yfl - (kTaps == 4), ix = (int)xfl - (kTaps == 4);
    int ro[kTaps], co[kTaps];
    bool oky[kTaps], okx[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        ro[k] = tap_index<kReflect>(iy + k, a.h, oky[k]) * a.w;
        co[k] = tap_index<kReflect>(ix + k, a.w, okx[k]);
    }
    // the chunk's planes: every load of the chunk is issued before the first sum (a ragged last chunk re-reads its last plane and
    // stores nothing for it)
    const long plane = (long)a.h * a.w;
    const int c0 = (int)chunk * kChunk;
    const float2* src = a.in + (long)g * a.inner * plane;
    float2* dst = a.out + ((long)f * a.inner * plane + (long)yo * a.w + xo);
    float2 v[kChunk][kTaps][kTaps];
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
        const float2* sp = src + (long)min(c0 + j, a.inner - 1) * plane;
#pragma unroll
        for (int r = 0; r < kTaps; ++r)
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                v[j][r][k] = sp[ro[r] + co[k]];
                if constexpr (!kReflect)
                    if (!(oky[r] && okx[k])) v[j][r][k] = make_float2(0.f, 0.f);
            }
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j) {
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int r = 0; r < kTaps; ++r) {
            float sr = 0.f, si = 0.f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                sr = fmaf(wx[k], v[j][r][k].x, sr);
                si = fmaf(wx[k], v[j][r][k].y, si);
            }
            re = fmaf(wy[r], sr, re);
            im = fmaf(wy[r], si, im);
        }
        if (c0 + j < a.inner) dst[(long)(c0 + j) * plane] = make_float2(re, im);
    }
}

}  // namespace cine

using namespace cine;

extern "C" int cine_affine_warp(const float* in, float* out, int frames, int inner, int h, int w,
                                double a_yy, double a_yx, double b_y, double a_xy, double a_xx, double b_x,
                                int mode, int border, int t_shift, int t_reverse, void* stream) {
    const char* what = "cine_affine_warp";
    CINE_REQUIRE(in && out, CINE_EINVAL, "%s: null pointer", what);
    CINE_REQUIRE(frames >= 1 && inner >= 1 && h >= 1 && w >= 1, CINE_EINVAL, "%s: Invalid shapes frames %d inner %d h %d w %d", what, frames,
                 inner, h, w);
    CINE_REQUIRE(h <= warp::kMaxSide && w <= warp::kMaxSide, CINE_EUNSUPPORTED, "%s: h %d w %d: planes of at most %d x %d", what, h, w,
                 warp::kMaxSide, warp::kMaxSide);
    CINE_REQUIRE(mode == 0 || mode == 1, CINE_EINVAL, "%s: mode %d is neither 0 (bilinear) nor 1 (bicubic)", what, mode);
    CINE_REQUIRE(border == 0 || border == 1, CINE_EINVAL, "%s: border %d is neither 0 (zeros) nor 1 (reflect)", what, border);
    const double m[4] = {a_yy, a_yx, a_xy, a_xx}, t[2] = {b_y, b_x};
    for (double v : m)
        CINE_REQUIRE(std::isfinite(v) && std::fabs(v) <= warp::kMaxA, CINE_EINVAL, "%s: matrix entry %g is not finite or above %g in size", what,
                     v, warp::kMaxA);
    for (double v : t)
        CINE_REQUIRE(std::isfinite(v) && std::fabs(v) <= warp::kMaxB, CINE_EINVAL, "%s: offset %g is not finite or above %g in size", what, v,
                     warp::kMaxB);
    CINE_REQUIRE(t_shift >= 0 && t_shift < frames, CINE_EINVAL, "%s: t_shift %d outside [0, %d)", what, t_shift, frames);
    CINE_REQUIRE(((uintptr_t)in | (uintptr_t)out) % 8 == 0, CINE_EINVAL, "%s: in and out must be 8-byte aligned", what);
    const long plane = (long)h * w;
    CINE_REQUIRE((long)frames * inner <= LONG_MAX / 8 / plane, CINE_EINVAL, "%s: %d x %d planes of %d x %d overflow a byte count", what, frames,
                 inner, h, w);
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
    const size_t bytes = (size_t)frames * inner * plane * 8;
    CINE_REQUIRE(i0 + bytes <= o0 || o0 + bytes <= i0, CINE_EINVAL, "%s: out overlaps in (out of place only)", what);
    const long tiles_x = ceil_div(w, warp::kTileW), tiles_y = ceil_div(h, warp::kTileH);
    const long chunks = ceil_div(inner, warp::chunk_of(mode == 0 ? 2 : 4));
    CINE_REQUIRE(tiles_x * tiles_y <= INT_MAX / (long)frames / chunks, CINE_EUNSUPPORTED,
                 "%s: %d frames x %ld plane chunks x %ld tiles exceed the grid limit %d workgroups", what, frames, chunks, tiles_x * tiles_y, INT_MAX);
    WarpArgs a;
    a.in = reinterpret_cast<const float2*>(in); a.out = reinterpret_cast<float2*>(out);
    a.frames = frames; a.inner = inner; a.h = h; a.w = w;
    a.ayy = a_yy; a.ayx = a_yx; a.oy = b_y + 0.5 * (double)(h - 1);
    a.axy = a_xy; a.axx = a_xx; a.ox = b_x + 0.5 * (double)(w - 1);
    a.t_shift = t_shift; a.t_reverse = t_reverse != 0;
    a.tiles_x = (unsigned)tiles_x; a.tiles_y = (unsigned)tiles_y; a.chunks = (unsigned)chunks;
    hipStream_t st = as_stream(stream);
    ProfScope prof(F_PACK, st);
    const dim3 grid((unsigned)(tiles_x * tiles_y * chunks * frames)), block(warp::kThreads);
    if (mode == 0 && border == 0) hipLaunchKernelGGL((affine_warp_kernel<2, false>), grid, block, 0, st, a);
    else if (mode == 0) hipLaunchKernelGGL((affine_warp_kernel<2, true>), grid, block, 0, st, a);
    else if (border == 0) hipLaunchKernelGGL((affine_warp_kernel<4, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((affine_warp_kernel<4, true>), grid, block, 0, st, a);
    return check_launch("affine_warp_kernel");
}
