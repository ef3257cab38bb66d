// tv_kernels.hip -- spatio-temporal total variation: one Condat-Vu primal-dual iteration after the data term's gradient, and the whole solve.
//
// No reference counterpart (the reference has no weight-free reconstruction beyond the zero-filled image); the iteration is the primal-dual
// splitting of Condat (JOTA 2013) and Vu (Adv. Comput. Math. 2013) on this library's own operators:
//     g = A^H M A x - zf                          cine_image_dc_t / cine_image_dc_general, weights (1, 0, -1)
//     xnew = x - tau (g + D^H p)
//     pnew = P(p + sigma D (2 xnew - x))           P: p_t onto the complex ball of radius lam_t, (p_h, p_w) jointly onto the ball of radius lam_s
// with D = (D_t, D_h, D_w) forward differences (D_t periodic or 0 at the last frame, D_h / D_w 0 at the last row / column).
// tv_pd_kernel is everything after g, in one launch.  pnew at a pixel needs xnew at its +h and +w neighbours and in the next frame, so a
// workgroup owns kTvTh x kTvTw pixels of up to kTvFrames consecutive frames and evaluates xnew on its tile plus a one-pixel halo on the high
// side (the right column and the bottom row: (kTvTh + 1) (kTvTw + 1) points) and in one frame past its last; an evaluation reads p one point
// further on the low side straight from memory.  The frames are walked with a rolling window of two LDS slots, {xnew, 2 xnew - x} per point
// (2 x 297 x 16 B = 9.3 KiB): the slot of frame f + 1 is filled, then the duals of frame f are formed from both.  Halo values are
// recomputed, never exchanged: every workgroup reads x, g, p and writes xnew, pnew, so no output may alias an input.
#include "solve.h"

namespace cine {

constexpr int kTvTh = 8;             // tile rows
constexpr int kTvTw = 32;            // tile columns: 256 B of one image row per tile row
constexpr int kTvThreads = kTvTh * kTvTw;
static_assert(kTvThreads == kSolveThreads, "block_record is written for this workgroup");
constexpr int kTvFrames = 2;         // frames per workgroup (plus one evaluated for D_t of the last); the fastest of 1 .. 16 at 15 x 200 x 200
constexpr int kTvMaxT = 64;
constexpr int kTvRow = kTvTw + 1;    // LDS row: the tile's columns and the halo column
constexpr int kTvSlot = (kTvTh + 1) * kTvRow;
constexpr int kTvHalo = kTvTh + kTvRow;          // halo points: the right column, then the bottom row with its corner

struct TvArgs {
    const cf* x; const cf* g;
    const cf* pt; const cf* ph; const cf* pw;    // the planes of p; those of a term that is off are never dereferenced
    const float* tau; const float* sigma; const float* lam_t; const float* lam_s;
    cf* xnew; cf* pnt; cf* pnh; cf* pnw;
    float* part;                     // 4 floats per workgroup, or NULL
    int T, H, W, tiles_w, tiles, temporal, spatial, periodic;
    int pzero;                       // p is zero and is not read: the first iteration of the solve
};

struct TvOwn { cf pt, ph, pw; };     // the duals at an evaluated point, kept for the projection of that point

// xnew and 2 xnew - x at (f, i, j) of batch element b, which lies inside the image
__device__ __forceinline__ float4 tv_eval(const TvArgs& a, int b, int f, int i, int j, float tau, TvOwn& own, cf& xold) {
    const int T = a.T, H = a.H, W = a.W;
    const long q = (((long)b * T + f) * H + i) * W + j;
    const cf xx = a.x[q], gg = a.g[q];
    float sx = gg.x, sy = gg.y;
    own.pt = own.ph = own.pw = mk(0.f, 0.f);
    auto ld = [&](const cf* p, long e) { return a.pzero ? mk(0.f, 0.f) : p[e]; };
    if (a.temporal) {                // (D_t^H p)[f] = p[f - 1] - p[f]; periodic: the indices wrap; otherwise p[T - 1] does not exist
        own.pt = ld(a.pt, q);
        const long HW = (long)H * W;
        if (a.periodic) {
            const cf lo = ld(a.pt, f > 0 ? q - HW : q + (long)(T - 1) * HW);
            sx += lo.x - own.pt.x; sy += lo.y - own.pt.y;
        } else {
            cf lo = mk(0.f, 0.f), hi = mk(0.f, 0.f);
            if (f > 0) lo = ld(a.pt, q - HW);
            if (f < T - 1) hi = own.pt;
            sx += lo.x - hi.x; sy += lo.y - hi.y;
        }
    }
    if (a.spatial) {
        own.ph = ld(a.ph, q); own.pw = ld(a.pw, q);
        cf lo = mk(0.f, 0.f), hi = mk(0.f, 0.f);
        if (i > 0) lo = ld(a.ph, q - W);
        if (i < H - 1) hi = own.ph;
        sx += lo.x - hi.x; sy += lo.y - hi.y;
        lo = mk(0.f, 0.f); hi = mk(0.f, 0.f);
        if (j > 0) lo = ld(a.pw, q - 1);
        if (j < W - 1) hi = own.pw;
        sx += lo.x - hi.x; sy += lo.y - hi.y;
    }
    const float nx = xx.x - tau * sx, ny = xx.y - tau * sy;
    xold = xx;
    return make_float4(nx, ny, 2.f * nx - xx.x, 2.f * ny - xx.y);
}

__global__ __launch_bounds__(kTvThreads) void tv_pd_kernel(TvArgs a) {
    __shared__ float4 slot[2][kTvSlot];
    __shared__ float red[4 * kTvThreads / 64];
    const int tid = threadIdx.x;
    const int T = a.T, H = a.H, W = a.W;
    const int b = blockIdx.y;
    const int chunk = blockIdx.x / a.tiles, tile = blockIdx.x - chunk * a.tiles;
    const int ti = tile / a.tiles_w, tj = tile - ti * a.tiles_w;
    const int i0 = ti * kTvTh, j0 = tj * kTvTw;
    const int t0 = chunk * kTvFrames;
    const int n = min(kTvFrames, T - t0);
    const float tau = *a.tau, sigma = *a.sigma;
    const float lam_t = a.temporal ? *a.lam_t : 0.f, lam_s = a.spatial ? *a.lam_s : 0.f;
    // the owned point of this thread, and the halo point of the first kTvHalo threads
    const int li = tid / kTvTw, lj = tid - li * kTvTw;
    const int i = i0 + li, j = j0 + lj;
    const bool inside = i < H && j < W;
    int hi_ = 0, hj_ = 0;
    bool halo = false;
    if (a.spatial && tid < kTvHalo) {
        hi_ = tid < kTvTh ? tid : kTvTh;
        hj_ = tid < kTvTh ? kTvTw : tid - kTvTh;
        halo = i0 + hi_ < H && j0 + hj_ < W;
    }
    const int me = li * kTvRow + lj;
    float s_dx = 0.f, s_x2 = 0.f, s_dt = 0.f, s_ds = 0.f;
    TvOwn own_cur{}, own_nxt{};

    // frame f into slot s; store: f is one of this workgroup's frames, so its xnew is written and counted here
    auto fill = [&](int f, int s, bool store, TvOwn& own) {
        if (inside) {
            cf xo;
            const float4 v = tv_eval(a, b, f, i, j, tau, own, xo);
            slot[s][me] = v;
            if (store) {
                a.xnew[(((long)b * T + f) * H + i) * W + j] = mk(v.x, v.y);
                const float dx = v.x - xo.x, dy = v.y - xo.y;
                s_dx += dx * dx + dy * dy;
                s_x2 += v.x * v.x + v.y * v.y;
            }
        }
        if (halo) {
            cf xo; TvOwn o;
            slot[s][hi_ * kTvRow + hj_] = tv_eval(a, b, f, i0 + hi_, j0 + hj_, tau, o, xo);
        }
    };

    fill(t0, 0, true, own_cur);
    for (int k = 0; k < n; ++k) {
        const int f = t0 + k, cur = k & 1, nxt = cur ^ 1;
        const bool has_dt = a.temporal && (f + 1 < T || a.periodic);
        if (k + 1 < n || has_dt) fill(f + 1 < T ? f + 1 : 0, nxt, k + 1 < n, own_nxt);
        __syncthreads();
        if (inside) {
            const long q = (((long)b * T + f) * H + i) * W + j;
            const float4 c = slot[cur][me];
            if (a.temporal) {
                float dx = 0.f, dy = 0.f;
                if (has_dt) {
                    const float4 nx = slot[nxt][me];
                    dx = nx.z - c.z; dy = nx.w - c.w;
                    const float ex = nx.x - c.x, ey = nx.y - c.y;
                    s_dt += sqrtf(ex * ex + ey * ey);
                }
                const float vx = own_cur.pt.x + sigma * dx, vy = own_cur.pt.y + sigma * dy;
                const float m = fmaxf(1.f, sqrtf(vx * vx + vy * vy) / lam_t);
                a.pnt[q] = mk(vx / m, vy / m);
            }
            if (a.spatial) {
                float hx = 0.f, hy = 0.f, wx = 0.f, wy = 0.f, e2 = 0.f;
                if (i < H - 1) {
                    const float4 d = slot[cur][me + kTvRow];
                    hx = d.z - c.z; hy = d.w - c.w;
                    const float ex = d.x - c.x, ey = d.y - c.y;
                    e2 += ex * ex + ey * ey;
                }
                if (j < W - 1) {
                    const float4 d = slot[cur][me + 1];
                    wx = d.z - c.z; wy = d.w - c.w;
                    const float ex = d.x - c.x, ey = d.y - c.y;
                    e2 += ex * ex + ey * ey;
                }
                s_ds += sqrtf(e2);
                const float ax = own_cur.ph.x + sigma * hx, ay = own_cur.ph.y + sigma * hy;
                const float bx = own_cur.pw.x + sigma * wx, by = own_cur.pw.y + sigma * wy;
                const float m = fmaxf(1.f, sqrtf((ax * ax + ay * ay) + (bx * bx + by * by)) / lam_s);
                a.pnh[q] = mk(ax / m, ay / m);
                a.pnw[q] = mk(bx / m, by / m);
            }
        }
        own_cur = own_nxt;
        __syncthreads();                            // slot cur is the next iteration's nxt
    }
    if (a.part) {
        float s[4] = {s_dx, s_x2, s_dt, s_ds};
        block_record(s, red, a.part, tid);
    }
}

__global__ __launch_bounds__(256) void tv_zero_kernel(float* p, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) p[e] = 0.f;
}

static long tv_tiles(int h, int w) { return (long)ceil_div(h, kTvTh) * ceil_div(w, kTvTw); }
static long tv_blocks(int b, int t, int h, int w) { return tv_tiles(h, w) * ceil_div(t, kTvFrames) * b; }

// sizes of one step launch: everything cine_tv_pd_step and cine_tv_solve refuse about (b, t, h, w)
static int tv_sizes(const char* what, int b, int t, int h, int w) {
    return solve_sizes(what, b, t, h, w, kTvMaxT, tv_tiles(h, w) * ceil_div(t, kTvFrames));
}

// p / pnew: the three planes given one by one (the solve keeps only the planes of the terms that are on)
static int tv_launch(const float* x, const float* g, const float* const p[3], const float* tau, const float* sigma, const float* lam_t,
                     const float* lam_s, int terms, int periodic, float* xnew, float* const pnew[3], float* part,
                     int b, int t, int h, int w, hipStream_t st, bool pzero = false) {
    TvArgs a{};
    a.x = reinterpret_cast<const cf*>(x); a.g = reinterpret_cast<const cf*>(g);
    a.pt = reinterpret_cast<const cf*>(p[0]); a.ph = reinterpret_cast<const cf*>(p[1]); a.pw = reinterpret_cast<const cf*>(p[2]);
    a.tau = tau; a.sigma = sigma; a.lam_t = lam_t; a.lam_s = lam_s;
    a.xnew = reinterpret_cast<cf*>(xnew);
    a.pnt = reinterpret_cast<cf*>(pnew[0]); a.pnh = reinterpret_cast<cf*>(pnew[1]); a.pnw = reinterpret_cast<cf*>(pnew[2]);
    a.part = part; a.T = t; a.H = h; a.W = w; a.tiles_w = ceil_div(w, kTvTw); a.tiles = (int)tv_tiles(h, w);
    a.temporal = (terms & 1) != 0; a.spatial = (terms & 2) != 0; a.periodic = periodic != 0; a.pzero = pzero;
    ProfScope prof(F_MISC, st);
    hipLaunchKernelGGL(tv_pd_kernel, dim3((unsigned)(tv_tiles(h, w) * ceil_div(t, kTvFrames)), b), dim3(kTvThreads), 0, st, a);
    return check_launch("tv_pd_kernel");
}

// workspace of the solve: [operator scratch | g | x' | two dual buffers of three planes each | iters rows of per-workgroup records].
// The terms are not among the arguments of cine_tv_solve_ws_bytes, so the duals are sized for all three planes; a solve with one term
// packs the planes that are on at the front of p[0] and behind them p[1].
struct TvSolveWs { size_t op_bytes, total, plane_floats; void* op; float* g; float* xtmp; float* p; float* part; };

static TvSolveWs tv_solve_ws(void* ws, int b, int t, int c, int h, int w, int mask_w, int iters) {
    TvSolveWs y{};
    WsCursor at{static_cast<unsigned char*>(ws)};
    const size_t img = solve_align((size_t)b * t * h * w * sizeof(cf));
    y.plane_floats = img / sizeof(float);
    y.op_bytes = dc_ws_bytes(mask_w, b, t, c, h, w);
    y.op = y.op_bytes ? at.take<void>(y.op_bytes) : nullptr;
    y.g = at.take<float>(img);
    y.xtmp = at.take<float>(img);
    y.p = at.take<float>(6 * img);
    y.part = at.take<float>((size_t)iters * cine_tv_pd_ws_bytes(b, t, h, w));
    y.total = at.end;
    return y;
}

static int tv_planes(int terms) { return ((terms & 1) ? 1 : 0) + ((terms & 2) ? 2 : 0); }

}  // namespace cine

using namespace cine;

extern "C" int cine_tv_pd_tile(int* th, int* tw) {
    CINE_REQUIRE(th && tw, CINE_EINVAL, "cine_tv_pd_tile: null pointer");
    *th = kTvTh; *tw = kTvTw;
    return CINE_OK;
}

extern "C" size_t cine_tv_pd_ws_bytes(int b, int t, int h, int w) {
    if (b <= 0 || t <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)tv_blocks(b, t, h, w) * 4 * sizeof(float);
}

extern "C" int cine_tv_pd_step(const float* x, const float* g, const float* p, const float* tau_dev, const float* sigma_dev,
                               const float* lam_t_dev, const float* lam_s_dev, int terms, int periodic, float* xnew, float* pnew, float* rec,
                               int b, int t, int h, int w, void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_tv_pd_step";
    CINE_REQUIRE(terms >= 1 && terms <= 3, CINE_EINVAL, "%s: terms %d is not 1 (temporal), 2 (spatial) or 3", what, terms);
    CINE_REQUIRE(x && g && p && tau_dev && sigma_dev && xnew && pnew && (!(terms & 1) || lam_t_dev) && (!(terms & 2) || lam_s_dev) && (!rec || ws),
                 CINE_EINVAL, "%s: null pointer", what);
    if (int e = tv_sizes(what, b, t, h, w)) return e;
    // workgroups read x, g and p across each other's seams: an output is no operand
    {
        const void* const outs[] = {xnew, pnew, rec};
        const void* const ins[] = {x, g, p, tau_dev, sigma_dev, lam_t_dev, lam_s_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, rec ? ws : nullptr), CINE_EINVAL,
                     "%s: xnew, pnew, rec and ws must not alias an operand or each other", what);
        const size_t need = rec ? cine_tv_pd_ws_bytes(b, t, h, w) : 0;
        CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    }
    hipStream_t st = as_stream(stream);
    const size_t plane = (size_t)b * t * h * w * 2;
    const float* pin[3] = {p, p + plane, p + 2 * plane};
    float* pout[3] = {pnew, pnew + plane, pnew + 2 * plane};
    float* part = rec ? reinterpret_cast<float*>(ws) : nullptr;
    if (int e = tv_launch(x, g, pin, tau_dev, sigma_dev, lam_t_dev, lam_s_dev, terms, periodic, xnew, pout, part, b, t, h, w, st)) return e;
    return rec ? solve_record_launch(part, tv_blocks(b, t, h, w), rec, 1, st) : CINE_OK;
}

extern "C" size_t cine_tv_solve_ws_bytes(int b, int t, int c, int h, int w, int mask_w, int iters) {
    if (b <= 0 || t <= 0 || c <= 0 || h <= 0 || w <= 0 || iters <= 0) return 0;
    return tv_solve_ws(nullptr, b, t, c, h, w, mask_w, iters).total;
}

extern "C" int cine_tv_solve(float* x, const float* zf, const float* sens, const float* sens_tiled, const uint8_t* mask, int mask_w,
                             const float* tau_dev, const float* sigma_dev, const float* lam_t_dev, const float* lam_s_dev, int terms,
                             int periodic, int iters, float* rec, float* p_out, int b, int t, int c, int h, int w,
                             void* ws, size_t ws_bytes, void* stream) {
    const char* what = "cine_tv_solve";
    CINE_REQUIRE(terms >= 1 && terms <= 3, CINE_EINVAL, "%s: terms %d is not 1 (temporal), 2 (spatial) or 3", what, terms);
    CINE_REQUIRE(x && zf && sens && mask && tau_dev && sigma_dev && (!(terms & 1) || lam_t_dev) && (!(terms & 2) || lam_s_dev) && ws, CINE_EINVAL,
                 "%s: null pointer", what);
    CINE_REQUIRE(c > 0 && iters >= 1, CINE_EINVAL, "%s: bad sizes", what);
    if (int e = tv_sizes(what, b, t, h, w)) return e;
    CINE_REQUIRE(mask_w == 1 || mask_w == w, CINE_EINVAL, "%s: mask_w %d is neither 1 (row mask) nor w", what, mask_w);
    {
        const void* const outs[] = {x, rec, p_out};
        const void* const ins[] = {zf, sens, sens_tiled, mask, tau_dev, sigma_dev, lam_t_dev, lam_s_dev};
        CINE_REQUIRE(solve_no_alias(outs, ins, ws), CINE_EINVAL, "%s: x, rec, p_out and ws must not alias an operand or each other", what);
    }
    const size_t need = cine_tv_solve_ws_bytes(b, t, c, h, w, mask_w, iters);
    CINE_REQUIRE(ws_bytes >= need, CINE_EWORKSPACE, "%s: workspace %zu < %zu", what, ws_bytes, need);
    const TvSolveWs y = tv_solve_ws(ws, b, t, c, h, w, mask_w, iters);
    float* pbuf[2] = {y.p, y.p + (size_t)tv_planes(terms) * y.plane_floats};
    const long nblk = tv_blocks(b, t, h, w);
    const size_t plane = (size_t)b * t * h * w * 2;
    hipStream_t st = as_stream(stream);
    // the planes of a buffer, in the order (t, h, w); a plane that is off is a null pointer
    auto planes = [&](float* buf, float* out[3]) {
        for (int q = 0; q < 3; ++q) {
            const bool on = (terms & (q == 0 ? 1 : 2)) != 0;
            out[q] = on ? buf : nullptr;
            if (on) buf += y.plane_floats;
        }
    };
    for (int k = 0; k < iters; ++k) {
        // the iterates alternate between x and x' so that the last one lands in x; x_0 = zf without a copy
        float* xout = (iters - 1 - k) % 2 == 0 ? x : y.xtmp;
        const float* xin = k == 0 ? zf : (xout == x ? y.xtmp : x);
        if (int e = solve_gradient(what, xin, zf, sens, sens_tiled, mask, mask_w, y.g, b, t, c, h, w, y.op, y.op_bytes, stream)) return e;
        float* pin[3]; float* pout[3];
        planes(pbuf[k & 1], pin);
        planes(pbuf[(k & 1) ^ 1], pout);
        if (k == iters - 1 && p_out) {              // the last duals go straight to the caller, at their places among the three planes
            for (int q = 0; q < 3; ++q) pout[q] = p_out + (size_t)q * plane;
        }
        if (int e = tv_launch(xin, y.g, pin, tau_dev, sigma_dev, lam_t_dev, lam_s_dev, terms, periodic, xout, pout,
                              rec ? y.part + (size_t)k * nblk * 4 : nullptr, b, t, h, w, st, k == 0))       // p_0 = 0 is told, not read
            return e;
    }
    if (p_out && terms != 3) {                      // the planes of the term that is off: zeros
        float* off = (terms & 1) ? p_out + plane : p_out;
        const long n = (long)((terms & 1) ? 2 : 1) * (long)plane;
        ProfScope prof(F_MISC, st);
        hipLaunchKernelGGL(tv_zero_kernel, dim3((unsigned)min(ceil_div(n, 256L), 65536L)), dim3(256), 0, st, off, n);
        if (int e = check_launch("tv_zero_kernel")) return e;
    }
    return rec ? solve_record_launch(y.part, nblk, rec, iters, st) : CINE_OK;
}
