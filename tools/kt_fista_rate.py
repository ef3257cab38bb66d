#!/usr/bin/env python3
"""What k-t SPARSE-SENSE costs at 1 x 15 frames x 15 coils x 200 x 200, R = 4, fused against composed, in ONE process.

    python tools/kt_fista_rate.py [--out profiles/kt_fista_rate.json] [--commit SHA]

Masks: "row" = every fourth row, shifted per frame, plus 16 centre rows; "plane" = the same with the first fifth of every readout dropped
outside the centre rows (a partial echo), so the mask varies along w and the operator takes both line passes.
Timed, for 1 and for 30 iterations, hipEvent medians of 10 solves each:
  * fused    : ``ops.kt_fista`` (cine_kt_fista: per iteration the operator launch(es) and ONE proximal launch);
  * composed : what was available before it -- ``ops.image_dc``, an axpy, a permute-copy that brings t to dim -2, ``ops.fft1c``, the soft
               threshold with torch element-wise ops, ``ops.fft1c`` back, a permute back and the extrapolation.
Peak memory of each: ``torch.cuda.max_memory_allocated`` over the warm-up and the timed solves above what was allocated before the variant's
first solve (cached workspaces dropped first), so the fused solve's workspace, which the binding keeps per stream, counts in full.
Then slices per second of ``KtSparseSense(iters=30)`` through ``SlicePipeline`` (graphs, 4 slots, device inputs, row mask).
--out writes the document, stamped with the commit and a sha256 over csrc/."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-cine-cardiac-mri_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

T, C, H, W = 15, 15, 200, 200
STEPS, ITERS, LAM = 10, 30, 0.02
SLOTS, SLICES = 4, 48


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def measure(solve, dev):
    """(hipEvent times of STEPS solves in ms, peak bytes above the bytes allocated before the first solve, warm-up included)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    for _ in range(3):
        solve()
    torch.cuda.synchronize()
    ms = []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); solve(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    return ms, torch.cuda.max_memory_allocated(dev) - base


def masks(dev):
    row = torch.zeros(1, T, 1, H, 1, 1, dtype=torch.uint8)
    for f in range(T):
        row[0, f, 0, f % 4::4] = 1
    row[:, :, :, H // 2 - 8:H // 2 + 8] = 1
    plane = row.expand(1, T, 1, H, W, 1).clone()
    plane[:, :, :, :H // 2 - 8, :W // 5] = 0
    plane[:, :, :, H // 2 + 8:, :W // 5] = 0
    return {"row": row.to(dev), "plane": plane.contiguous().to(dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit to stamp the result with (default: git rev-parse HEAD)")
    args = ap.parse_args()
    from cine_hip import classical, dc, ops, synth
    from cine_hip.pipeline import SlicePipeline
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    ex = synth.make_cine_slice(T, C, H, W, accel=4, seed=0, noise_std=0.01)
    kspace, sens = ex["kspace"].to(dev), ex["sens_maps"].to(dev)
    commit, csrc = _stamp(args.commit)
    doc = {"shape": [1, T, C, H, W], "masks": "R = 4 rows shifted per frame + 16 centre rows; plane: the first fifth of the readout dropped outside them",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS, "lam": LAM,
           "commit": commit, "csrc_sha256": csrc, "image_bytes": T * H * W * 8}
    step = classical.default_step(sens)
    with torch.no_grad():
        for name, mask in masks(dev).items():
            mk = ops.apply_mask(kspace, mask)
            acq = dc.Acquisition(mk, mask, sens)
            zf, tiled = acq.zero_filled(), acq.tiled
            thresh = classical.temporal_peak(zf) * LAM
            theta = (step * thresh).reshape(1, 1, 1, 1)

            def composed(iters):
                betas = classical.fista_momentum(iters)
                x = z = zf
                for k in range(iters):
                    g = ops.image_dc(z, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled)
                    v = z - step * g
                    c = ops.fft1c(v.reshape(1, T, H * W, 2).permute(0, 2, 1, 3).contiguous())
                    mag = (c * c).sum(dim=-1, keepdim=True).sqrt()
                    c = c * ((mag - theta).clamp_min(0.0) / mag.clamp_min(1e-30))
                    xn = ops.fft1c(c, inverse=True).permute(0, 2, 1, 3).reshape(zf.shape)
                    z = xn + float(betas[k]) * (xn - x)
                    x = xn
                return x

            def fused(iters):
                return ops.kt_fista(zf, sens, mask, step, thresh, iters, sens_tiled=tiled)
            xf, xc = fused(ITERS), composed(ITERS)
            res = {"mask_fraction": float(mask.float().mean()), "fused_workspace_bytes": int(ops.lib().cine_kt_fista_ws_bytes(1, T, C, H, W, mask.shape[4], ITERS)),
                   "fused_vs_composed_max_abs_over_peak": float((xf - xc).abs().max() / xc.abs().max())}
            del xf, xc
            for iters in (1, ITERS):
                for variant, fn in (("fused", fused), ("composed", composed), ("fused_again", fused), ("composed_again", composed)):
                    ops.release_general_workspaces()
                    torch.cuda.empty_cache()
                    ms, peak = measure(lambda: fn(iters), dev)
                    res[f"{variant}_{iters}"] = {"median_ms": median(ms), "ms": ms, "peak_bytes": peak}
                    print(json.dumps({name: {f"{variant}_{iters}": res[f"{variant}_{iters}"]}}), flush=True)
                res[f"composed_over_fused_{iters}"] = res[f"composed_{iters}"]["median_ms"] / res[f"fused_{iters}"]["median_ms"]
                res[f"peak_fused_over_composed_{iters}"] = res[f"fused_{iters}"]["peak_bytes"] / res[f"composed_{iters}"]["peak_bytes"]
            res["fused_us_per_iteration"] = 1e3 * (res[f"fused_{ITERS}"]["median_ms"] - res["fused_1"]["median_ms"]) / (ITERS - 1)
            res["composed_us_per_iteration"] = 1e3 * (res[f"composed_{ITERS}"]["median_ms"] - res["composed_1"]["median_ms"]) / (ITERS - 1)
            doc[name] = res
            print(json.dumps({name: {k: v for k, v in res.items() if not isinstance(v, dict)}}), flush=True)
        # KtSparseSense through SlicePipeline: slices per second, wall clock from the first submit to the last result
        mask = masks(dev)["row"]
        mk = ops.apply_mask(kspace, mask)
        model = classical.KtSparseSense(iters=ITERS, lam=LAM).eval()
        with SlicePipeline(model, slots=SLOTS) as pipe:
            pipe.submit(mk, mask, sens, tag="build")
            list(pipe.drain())
            rates = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for j in range(SLICES):
                    pipe.submit(mk, mask, sens, tag=j)
                    for _ in pipe.results():
                        pass
                list(pipe.drain())
                torch.cuda.synchronize()
                rates.append(SLICES / (time.perf_counter() - t0))
        doc["pipeline"] = {"model": f"KtSparseSense(iters={ITERS})", "slots": SLOTS, "slices": SLICES, "slices_per_s": median(rates), "runs": rates}
        print(json.dumps({"pipeline": doc["pipeline"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
