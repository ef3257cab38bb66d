"""cine_affine_warp restated in float64 numpy from the convention in include/cine_hip.h: centred float64 source coordinates, floor,
bilinear or cubic-convolution (A = -0.75) weights, zero or half-sample symmetric reflecting borders, the cyclic frame remap.
test_augment_cpu.py holds it against torch.nn.functional.grid_sample in float64; test_augment_kernels.py holds the kernel against it."""
import numpy as np

A = -0.75
U = 2.0 ** -24                                   # float32 unit roundoff
C_BAR = {0: 8.0, 1: 24.0}                        # the kernel's bar in units of U * sum |taps| (test_augment_kernels.py derives them)


def reflect(i, n):
    """Half-sample symmetric reflection with period 2 n: ..., 1, 0 | 0, 1, ..., n - 1 | n - 1, n - 2, ..."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def weights(f, mode):
    """(taps, ...) float64 weights for the fraction f; bilinear taps start at i0, bicubic at i0 - 1."""
    if mode == 0:
        return np.stack([1.0 - f, f])
    near = lambda x: ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = lambda x: ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return np.stack([far(1.0 + f), near(f), near(1.0 - f), far(2.0 - f)])


def axis_taps(s, n, mode, border):
    """Source coordinate s (any shape) on an axis of n samples -> (index (taps, ...) inside the axis, weight, counts (bool))."""
    i0 = np.floor(s)
    w = weights(s - i0, mode)
    taps = 2 if mode == 0 else 4
    i = i0.astype(np.int64)[None] + np.arange(taps).reshape((taps,) + (1,) * s.ndim) - (mode == 1)
    if border == 1:
        return reflect(i, n), w, np.ones(i.shape, bool)
    ok = (i >= 0) & (i < n)
    return np.clip(i, 0, n - 1), w, ok


def source_coords(h, w, m):
    """m = ((a_yy, a_yx, b_y), (a_xy, a_xx, b_x)) -> (ys, xs), each (h, w) float64."""
    (ayy, ayx, by), (axy, axx, bx) = m
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    yo, xo = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return ayy * (yo - cy) + ayx * (xo - cx) + by + cy, axy * (yo - cy) + axx * (xo - cx) + bx + cx


def frame_map(frames, t_shift, t_reverse):
    f = np.arange(frames)
    return np.mod(t_shift - f if t_reverse else f + t_shift, frames)


def warp_planes(x, m, mode, border):
    """x (planes, h, w, 2) -> (out, foot), both (planes, h, w, 2) float64: the resampled planes, and per output component the sum of
    |tap value| over the taps of its footprint that count (reflected taps where they land, taps outside under border 0 nothing)."""
    x = np.asarray(x, dtype=np.float64)
    p, h, w, _ = x.shape
    ys, xs = source_coords(h, w, m)
    iy, wy, oky = axis_taps(ys, h, mode, border)
    ix, wx, okx = axis_taps(xs, w, mode, border)
    flat = x.reshape(p, h * w, 2)
    out = np.zeros((p, h * w, 2))
    foot = np.zeros((p, h * w, 2))
    for r in range(iy.shape[0]):
        for k in range(ix.shape[0]):
            ok = (oky[r] & okx[k]).reshape(-1)
            v = np.take(flat, (iy[r] * w + ix[k]).reshape(-1), axis=1) * ok[None, :, None]
            out += v * (wy[r] * wx[k]).reshape(1, -1, 1)
            foot += np.abs(v)
    return out.reshape(p, h, w, 2), foot.reshape(p, h, w, 2)


def warp_reference(x, m, mode, border, t_shift=0, t_reverse=False):
    """x (frames, inner, h, w, 2) -> (out, foot) float64 of cine_affine_warp."""
    x = np.asarray(x)
    frames, inner, h, w, _ = x.shape
    out, foot = warp_planes(x.reshape(frames * inner, h, w, 2), m, mode, border)
    g = frame_map(frames, t_shift, t_reverse)
    return out.reshape(x.shape)[g], foot.reshape(x.shape)[g]


def theta_of(m, h, w):
    """The affine_grid theta (2, 3) whose grid_sample(align_corners=False) is the map m on an h x w plane."""
    (ayy, ayx, by), (axy, axx, bx) = m
    return np.array([[axx, axy * h / w, 2.0 * bx / w], [ayx * w / h, ayy, 2.0 * by / h]])


def matrices(h, w):
    """The named maps of the sweeps for an h x w plane (rot90 on square planes only)."""
    cs, sn = np.cos(np.radians(37.0)), np.sin(np.radians(37.0))
    out = {
        "identity": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
        "flip_h": ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0)),
        "flip_v": ((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
        "shift_int": ((1.0, 0.0, 2.0), (0.0, 1.0, -3.0)),
        "shift_far": ((1.0, 0.0, 2.5 * h), (0.0, 1.0, -3.7 * w)),
        "shift_far_b": ((1.0, 0.0, 3.7 * h), (0.0, 1.0, 2.5 * w)),
        "rot37":((cs, sn, 0.0), (-sn, cs, 0.0)),
        "scale_shear": ((0.6, 0.21, 0.3), (-0.13, 1.7, -0.45)),
        "zero": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    }
    if h == w:
        out["rot90"] = ((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0))
    return out
