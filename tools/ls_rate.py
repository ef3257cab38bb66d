#!/usr/bin/env python3
"""What low-rank plus sparse (L+S) costs at 1 x 15 frames x 15 coils x 200 x 200, R = 4, fused against composed, in ONE process.

    python tools/ls_rate.py [--out profiles/ls_rate.json] [--commit SHA]

Masks: those of tools/kt_fista_rate.py -- "row" = every fourth row, shifted per frame, plus 16 centre rows; "plane" = the same with the
first fifth of every readout dropped outside the centre rows, so the mask varies along w.
Timed, for 1 and for 50 iterations, hipEvent medians of 10 solves each, the two variants in two alternating regions:
  * fused    : ``ops.ls_solve`` (cine_ls_solve: per iteration the operator, the Gram matrix, the Jacobi weight kernel, ONE proximal launch);
  * composed : what the package offered before it -- ``ops.image_dc``, torch element-wise ops, ``torch.linalg.svd`` of the (h w) x t Casorati
               matrix on the device (``torch.linalg.eigh`` of its Gram matrix where this torch build has no device SVD; the output says
               which), a permute-copy, ``ops.fft1c``, the soft threshold with torch ops, ``ops.fft1c`` back and a permute back.
Then the time of each kernel of one iteration on the first iteration's operands (operator, Gram matrix, weight, prox; the weight kernel is
one workgroup and latency-bound, its share is the number to watch), peak memory above the baseline as in kt_fista_rate.py, and slices per
second of ``LowRankPlusSparse(iters=50)`` through ``SlicePipeline`` (graphs, 4 slots, device inputs, row mask).
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

from kt_fista_rate import C, H, SLICES, SLOTS, STEPS, T, W, masks, measure, median  # noqa: E402

ITERS, LAM_L, LAM_S = 50, 0.01, 0.01


def device_svd_works(dev):
    try:
        a = torch.randn(64, 5, dtype=torch.complex64, device=dev)
        u, s, vh = torch.linalg.svd(a, full_matrices=False)
        torch.cuda.synchronize()
        return bool(((u * s) @ vh - a).abs().max() < 1e-4)
    except Exception as e:                              # a build without the solver library
        print(json.dumps({"device_svd": f"unavailable: {type(e).__name__}: {e}"[:300]}), flush=True)
        return False


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
    svd_ok = device_svd_works(dev)
    doc = {"shape": [1, T, C, H, W], "masks": "R = 4 rows shifted per frame + 16 centre rows; plane: the first fifth of the readout dropped outside them",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS, "iters": ITERS,
           "lam_l": LAM_L, "lam_s": LAM_S, "commit": commit, "csrc_sha256": csrc, "image_bytes": T * H * W * 8,
           "composed_svt": "torch.linalg.svd of the Casorati matrix on the device" if svd_ok else
           "torch.linalg.eigh of the Gram matrix on the device (this torch build has no working device SVD)"}
    step = 0.5 * classical.default_step(sens)
    with torch.no_grad():
        for name, mask in masks(dev).items():
            mk = ops.apply_mask(kspace, mask)
            acq = dc.Acquisition(mk, mask, sens)
            zf, tiled = acq.zero_filled(), acq.tiled
            thl = classical.casorati_sigma_max(zf) * LAM_L
            ths = classical.temporal_peak(zf) * LAM_S
            th_l, th_s = step * thl, (step * ths).reshape(1, 1, 1, 1)

            def svt(v):
                x = torch.view_as_complex(v.reshape(T, H * W, 2)).transpose(0, 1)              # (h w, t)
                if svd_ok:
                    u, s, vh = torch.linalg.svd(x, full_matrices=False)
                    y = (u * (s - th_l).clamp_min(0.0)) @ vh
                else:
                    lam, vec = torch.linalg.eigh(x.conj().transpose(0, 1) @ x)
                    sq = lam.clamp_min(0.0).sqrt()
                    hh = torch.where(sq > th_l, 1.0 - th_l / sq.clamp_min(1e-30), torch.zeros_like(sq))
                    y = x @ ((vec * hh) @ vec.conj().transpose(0, 1))
                return torch.view_as_real(y.transpose(0, 1).contiguous()).reshape(v.shape)

            def composed(iters):
                lo, so, x = zf, torch.zeros_like(zf), zf
                for _ in range(iters):
                    g = ops.image_dc(x, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled)
                    lo = svt(lo - step * g)
                    c = ops.fft1c((so - step * g).reshape(1, T, H * W, 2).permute(0, 2, 1, 3).contiguous())
                    mag = (c * c).sum(dim=-1, keepdim=True).sqrt()
                    c = c * ((mag - th_s).clamp_min(0.0) / mag.clamp_min(1e-30))
                    so = ops.fft1c(c, inverse=True).permute(0, 2, 1, 3).reshape(zf.shape)
                    x = lo + so
                return x

            def fused(iters):
                return ops.ls_solve(zf, sens, mask, step, thl, ths, iters, sens_tiled=tiled)
            xf, xc = fused(ITERS), composed(ITERS)
            _, rec, resid = ops.ls_solve(zf, sens, mask, step, thl, ths, ITERS, sens_tiled=tiled, record=True)
            res = {"mask_fraction": float(mask.float().mean()),
                   "fused_workspace_bytes": int(ops.lib().cine_ls_solve_ws_bytes(1, T, C, H, W, mask.shape[4], ITERS)),
                   "fused_vs_composed_max_abs_over_peak": float((xf - xc).abs().max() / xc.abs().max()),
                   "worst_jacobi_residual": float(resid.max())}
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
            # the kernels of one iteration, each alone, on the first iteration's operands
            g = ops.image_dc(zf, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled)
            gram = ops.casorati_gram(zf, g, step)
            wgt, info = ops.svt_weight(gram, thl, step)
            zero = torch.zeros_like(zf)
            parts = {"operator": lambda: ops.image_dc(zf, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled),
                     "gram": lambda: ops.casorati_gram(zf, g, step),
                     "weight": lambda: ops.svt_weight(gram, thl, step),
                     "prox": lambda: ops.ls_prox(zf, zero, g, wgt, step, ths)}
            split = {k: median(measure(fn, dev)[0]) * 1e3 for k, fn in parts.items()}
            total = sum(split.values())
            res["kernel_us"] = split
            res["kernel_share"] = {k: v / total for k, v in split.items()}
            res["weight_sweeps"] = int(info[0, 3])
            doc[name] = res
            print(json.dumps({name: {k: v for k, v in res.items() if not (isinstance(v, dict) and "ms" in v)}}), flush=True)
        mask = masks(dev)["row"]
        mk = ops.apply_mask(kspace, mask)
        model = classical.LowRankPlusSparse(iters=ITERS, lam_l=LAM_L, lam_s=LAM_S).eval()
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
        doc["pipeline"] = {"model": f"LowRankPlusSparse(iters={ITERS})", "slots": SLOTS, "slices": SLICES, "slices_per_s": median(rates), "runs": rates}
        print(json.dumps({"pipeline": doc["pipeline"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
