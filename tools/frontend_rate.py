#!/usr/bin/env python3
"""Device time of the data front-end (cine_hip.frontend.prepare_slice) at raw k-space sizes the FFT line engines refuse, printed as
JSON (one object per raw shape, and the list written to --out).

    python tools/frontend_rate.py [--repeats 10] [--warmup 3] [--out profiles/frontend_any_size_rate.json] [--no-oracle]
                                  [--virtual-coils V]

Raw shapes (t, x, y, coil) = (25, 416, 208, 30), (25, 768, 384, 30), (25, 832, 416, 30), each with the reference's 200 x 200 crop
and 15 frames.  Per shape: hipEvent times (median over --repeats, after --warmup calls) of the whole prepare_slice and of the windowed
IDFT alone (ops.raw_window_ifft2c: matrix build + two GEMM launches, kernels raw_window_matrix_kernel / raw_window_gemm_kernel), the
window transform's algorithmic FLOPs (8 per complex MAC, the cheaper axis order, as the library picks it), its rate and its share of
the f32 MFMA peak (157.3 TFLOP/s), and the CPU oracle's time for one prepare_slice (oracle/frontend_ref.py, numpy) for scale.

--virtual-coils V (off by default: the output above is then unchanged) adds a "coil_compression" object per shape: the device time of
the Gram matrix (frontend.coil_gram, kept frames, 24 x 24 block), of the compression (frontend.compress_coils; with the bytes it reads
and writes per second, next to the measured float4 copy rate of 6.29 TB/s), the host-visible time of the eigen step
(frontend.coil_matrix_from_gram, a library call, synchronised), the device time of the rest of prepare_slice on V coils and of the window
transform on V coils, and of prepare_slice(virtual_coils=V) as a whole.  "gram_plus_compress_below_window_saving" compares Gram + compress
with what the window transform saves by running on V coils instead of all of them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-cine-cardiac-mri_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_F32_TFLOPS = 157.3
COPY_TBPS = 6.29                       # measured float4 copy rate of the device
SHAPES = [(25, 416, 208, 30), (25, 768, 384, 30), (25, 832, 416, 30)]
CROP, FRAMES = (200, 200), 15


def window_flops(t_out, nx, ny, c, cx, cy):
    """8 FLOPs per complex MAC, the axis order the library picks (x first: nx ny cx + ny cx cy per image; y first: nx ny cy + nx cy cx)."""
    return 8 * t_out * c * min(nx * ny * cx + ny * cx * cy, nx * ny * cy + nx * cy * cx)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def coil_compression_leg(FE, ops, x, v, win_ms, warmup, repeats):
    t, nx, ny, c = x.shape
    gram_ms, _ = timed(lambda: FE.coil_gram(x, FRAMES), warmup, repeats)
    gram = FE.coil_gram(x, FRAMES)
    eig = []
    for _ in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, _ = FE.coil_matrix_from_gram(gram, v)
        torch.cuda.synchronize()
        eig.append((time.perf_counter() - t0) * 1e3)
    comp_ms, comp_min = timed(lambda: FE.compress_coils(x, a, FRAMES), warmup, repeats)
    y = FE.compress_coils(x, a, FRAMES)
    rest_ms, _ = timed(lambda: FE.prepare_slice(y, CROP, FRAMES), warmup, repeats)
    win_v_ms, _ = timed(lambda: ops.raw_window_ifft2c(y, FRAMES, CROP, 1e6), warmup, repeats)
    whole_ms, _ = timed(lambda: FE.prepare_slice(x, CROP, FRAMES, coil_matrix=a), warmup, repeats)
    nbytes = 8 * min(FRAMES, t) * nx * ny * (c + v)
    return {"virtual_coils": v, "gram_ms": round(gram_ms, 4), "compress_ms": round(comp_ms, 4), "compress_min_ms": round(comp_min, 4),
            "compress_bytes": nbytes, "compress_tbps": round(nbytes / comp_ms / 1e9, 3),
            "compress_frac_of_copy_rate": round(nbytes / comp_ms / 1e9 / COPY_TBPS, 3),
            "eigen_host_ms": round(float(np.median(eig[warmup:])), 4),
            "rest_of_prepare_slice_ms": round(rest_ms, 4), "window_ms_virtual": round(win_v_ms, 4),
            "window_saving_ms": round(win_ms - win_v_ms, 4),
            "prepare_slice_given_matrix_ms": round(whole_ms, 4),
            "gram_plus_compress_below_window_saving": bool(gram_ms + comp_ms < win_ms - win_v_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--virtual-coils", type=int, default=0)
    args = ap.parse_args()
    from cine_hip import frontend as FE, ops
    dev = torch.device("cuda:0")
    rows = []
    for shape in SHAPES:
        t, nx, ny, c = shape
        rs = np.random.RandomState(0)
        raw = (rs.standard_normal(shape).astype(np.float32) + 1j * rs.standard_normal(shape).astype(np.float32)).astype(np.complex64)
        x = torch.from_numpy(raw).to(dev)
        assert not (ops.fft_line_supported(nx) and ops.fft_line_supported(ny)), shape
        slice_ms, slice_min = timed(lambda: FE.prepare_slice(x, CROP, FRAMES), args.warmup, args.repeats)
        win_ms, win_min = timed(lambda: ops.raw_window_ifft2c(x, FRAMES, CROP, 1e6), args.warmup, args.repeats)
        flops = window_flops(FRAMES, nx, ny, c, *CROP)
        row = {"raw_shape": list(shape), "crop": list(CROP), "frames": FRAMES,
               "prepare_slice_ms": round(slice_ms, 4), "prepare_slice_min_ms": round(slice_min, 4),
               "window_ms": round(win_ms, 4), "window_min_ms": round(win_min, 4),
               "window_gflop": round(flops / 1e9, 3), "window_tflops": round(flops / win_ms / 1e9, 2),
               "window_frac_of_f32_peak": round(flops / win_ms / 1e9 / PEAK_F32_TFLOPS, 3),
               "x_first": nx * ny * CROP[0] + ny * CROP[0] * CROP[1] <= nx * ny * CROP[1] + nx * CROP[1] * CROP[0],
               "ws_bytes": int(ops.lib().cine_raw_window_ws_bytes(FRAMES, nx, ny, c, *CROP))}
        if args.virtual_coils:
            row["coil_compression"] = coil_compression_leg(FE, ops, x, args.virtual_coils, win_ms, args.warmup, args.repeats)
        if not args.no_oracle:
            from oracle import frontend_ref as F
            t0 = time.perf_counter()
            F.prepare_slice(raw, CROP, FRAMES)
            row["oracle_cpu_s"] = round(time.perf_counter() - t0, 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup, "shapes": rows}, f, indent=1)


if __name__ == "__main__":
    main()
