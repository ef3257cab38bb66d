#!/usr/bin/env python3
"""What spatio-temporal total variation costs at 1 x 15 frames x 15 coils x 200 x 200, R = 4, fused against composed, in ONE process.

    python tools/tv_rate.py [--out profiles/tv_rate.json] [--commit SHA]

Masks: "row" = every fourth row, shifted per frame, plus 16 centre rows; "plane" = the same with the first fifth of every readout dropped
outside the centre rows (a partial echo), so the mask varies along w and the operator takes both line passes.
Timed, for 1 and for 50 iterations, hipEvent medians of 10 solves each (temporal + spatial, periodic):
  * fused    : ``ops.tv_solve`` (cine_tv_solve: per iteration the operator launch(es) and ONE primal-dual launch);
  * composed : what was available before it -- ``ops.image_dc``, then D, D^H and the two projections with torch slicing, padding and
               element-wise ops.
Peak memory of each: ``torch.cuda.max_memory_allocated`` over the warm-up and the timed solves above what was allocated before the variant's
first solve (cached workspaces dropped first), so the fused solve's workspace, which the binding keeps per stream, counts in full.
The step kernel alone (``ops.tv_pd_step`` into preallocated outputs, LAUNCHES launches captured into one graph, median of 10 replays) for
terms 3, 1 and 2, with the bytes it algorithmically moves: read x, g and the planes that are on, write x and those planes.
Then slices per second of ``TotalVariation(iters=50)`` through ``SlicePipeline`` (graphs, 4 slots, device inputs, row mask).
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
import torch.nn.functional as F  # noqa: E402

T, C, H, W = 15, 15, 200, 200
STEPS, ITERS, LAM_T, LAM_S = 10, 50, 0.02, 0.01
SLOTS, SLICES = 4, 48
LAUNCHES = 20


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


# D, D^H and P of the composed path on (1, T, 1, H, W, 2) tensors: frames on dim 1, rows on dim 3, columns on dim 4
def diff(x, dim):
    n = x.shape[dim]
    d = x.narrow(dim, 1, n - 1) - x.narrow(dim, 0, n - 1)
    pad = [0, 0] * (x.dim() - 1 - dim) + [0, 1]
    return F.pad(d, pad)


def diff_adj(p, dim):
    n = p.shape[dim]
    q = p.narrow(dim, 0, n - 1)
    back, front = [0, 0] * (p.dim() - 1 - dim) + [0, 1], [0, 0] * (p.dim() - 1 - dim) + [1, 0]
    return F.pad(q, front) - F.pad(q, back)


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
    image_bytes = T * H * W * 8
    doc = {"shape": [1, T, C, H, W], "masks": "R = 4 rows shifted per frame + 16 centre rows; plane: the first fifth of the readout dropped outside them",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS,
           "lam_t": LAM_T, "lam_s": LAM_S, "tile": list(ops.tv_pd_tile()), "commit": commit, "csrc_sha256": csrc, "image_bytes": image_bytes}
    tau = classical.default_step(sens)
    sigma = (24.0 * tau).reciprocal()
    with torch.no_grad():
        for name, mask in masks(dev).items():
            mk = ops.apply_mask(kspace, mask)
            acq = dc.Acquisition(mk, mask, sens)
            zf, tiled = acq.zero_filled(), acq.tiled
            peak_t, peak_s = classical.tv_peaks(zf, True)
            lam_t, lam_s = peak_t * LAM_T, peak_s * LAM_S

            def composed(iters):
                x = zf
                pt, ph, pw = torch.zeros_like(zf), torch.zeros_like(zf), torch.zeros_like(zf)
                for _ in range(iters):
                    g = ops.image_dc(x, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled)
                    xn = x - tau * (g + (pt.roll(1, dims=1) - pt) + diff_adj(ph, 3) + diff_adj(pw, 4))
                    xb = 2.0 * xn - x
                    vt = pt + sigma * (xb.roll(-1, dims=1) - xb)
                    vh, vw = ph + sigma * diff(xb, 3), pw + sigma * diff(xb, 4)
                    pt = vt / ((vt * vt).sum(dim=-1, keepdim=True).sqrt() / lam_t).clamp_min(1.0)
                    s = (((vh * vh).sum(dim=-1, keepdim=True) + (vw * vw).sum(dim=-1, keepdim=True)).sqrt() / lam_s).clamp_min(1.0)
                    ph, pw = vh / s, vw / s
                    x = xn
                return x

            def fused(iters):
                return ops.tv_solve(zf, sens, mask, tau, sigma, lam_t, lam_s, iters, sens_tiled=tiled)
            xf, xc = fused(ITERS), composed(ITERS)
            res = {"mask_fraction": float(mask.float().mean()), "fused_workspace_bytes": int(ops.lib().cine_tv_solve_ws_bytes(1, T, C, H, W, mask.shape[4], ITERS)),
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
        # the step kernel alone, on the iterates of a solve that is under way (duals inside and on their balls)
        mask = masks(dev)["row"]
        mk = ops.apply_mask(kspace, mask)
        acq = dc.Acquisition(mk, mask, sens)
        zf = acq.zero_filled()
        peak_t, peak_s = classical.tv_peaks(zf, True)
        lam_t, lam_s = peak_t * LAM_T, peak_s * LAM_S
        x, p = ops.tv_solve(zf, sens, mask, tau, sigma, lam_t, lam_s, 10, sens_tiled=acq.tiled, dual=True)
        g = ops.image_dc(x, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=acq.tiled)
        xnew, pnew = torch.empty_like(x), torch.empty_like(p)
        doc["step_kernel"] = {"launches_per_sample": LAUNCHES}
        for terms, images in ((3, 9), (1, 5), (2, 7)):
            def launches():
                for _ in range(LAUNCHES):
                    ops.tv_pd_step(x, g, p, tau, sigma, lam_t, lam_s, terms=terms, xnew=xnew, pnew=pnew)
            graph = torch.cuda.CUDAGraph()                        # replayed as a graph: the host's call overhead stays out of the figure
            with torch.cuda.graph(graph):
                launches()
            ms, _ = measure(graph.replay, dev)
            us = 1e3 * median(ms) / LAUNCHES
            doc["step_kernel"][f"terms_{terms}"] = {"us": us, "images_moved": images, "bytes_moved": images * image_bytes,
                                                    "tb_per_s": images * image_bytes / (us * 1e-6) / 1e12, "us_per_launch_samples": [1e3 * m / LAUNCHES for m in ms]}
            print(json.dumps({"step_kernel": {f"terms_{terms}": doc["step_kernel"][f"terms_{terms}"]}}), flush=True)
        # TotalVariation through SlicePipeline: slices per second, wall clock from the first submit to the last result
        model = classical.TotalVariation(iters=ITERS, lam_t=LAM_T, lam_s=LAM_S).eval()
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
        doc["pipeline"] = {"model": f"TotalVariation(iters={ITERS})", "slots": SLOTS, "slices": SLICES, "slices_per_s": median(rates), "runs": rates}
        print(json.dumps({"pipeline": doc["pipeline"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
