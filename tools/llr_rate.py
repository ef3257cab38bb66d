#!/usr/bin/env python3
"""What the locally low-rank baseline (LLR) costs at 1 x 15 frames x 15 coils x 200 x 200, R = 4, fused against composed, in ONE process.

    python tools/llr_rate.py [--out profiles/llr_rate.json] [--commit SHA]

Masks: those of tools/kt_fista_rate.py -- "row" = every fourth row, shifted per frame, plus 16 centre rows; "plane" = the same with the
first fifth of every readout dropped outside the centre rows, so the mask varies along w.  8 x 8 blocks, the seed-0 shifts of
``classical.llr_shifts``, lam = 0.005 of the largest block singular value of the zero-filled image.
Timed, for 1 and for 30 iterations, hipEvent medians of 10 solves each, the two variants in two alternating regions:
  * fused    : ``ops.llr_solve`` (cine_llr_solve: per iteration the operator and ONE proximal launch with a workgroup per block);
  * composed : the loop a user of the package would write without it -- ``ops.image_dc``, torch element-wise ops, zero padding to the
               shifted block grid, a reshape / permute into (blocks, block^2, t) matrices, batched ``torch.linalg.svd`` on the device
               (``torch.linalg.eigh`` of the blocks' Gram matrices where this torch build has no device SVD; the output says which),
               the fold back and the crop.
Then the proximal launch alone on the first iteration's operands (with its sweeps and block count; unshifted and shifted), the operator
alone, peak memory above the baseline as in kt_fista_rate.py, and slices per second of ``LocallyLowRank(iters=30)`` through
``SlicePipeline`` (graphs, 4 slots, device inputs, row mask).  The per-iteration time of L+S from profiles/ls_rate.json is copied next to
LLR's where that file exists, so a reader can compare.
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
from ls_rate import device_svd_works  # noqa: E402

ITERS, LAM, BLOCK = 30, 0.005, 8


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
    shifts = classical.llr_shifts(ITERS, BLOCK, 0)
    doc = {"shape": [1, T, C, H, W], "masks": "R = 4 rows shifted per frame + 16 centre rows; plane: the first fifth of the readout dropped outside them",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS, "iters": ITERS,
           "lam": LAM, "block": BLOCK, "shifts": "classical.llr_shifts(iters, block, 0)", "commit": commit, "csrc_sha256": csrc,
           "image_bytes": T * H * W * 8,
           "composed_svt": "batched torch.linalg.svd of the blocks' Casorati matrices on the device" if svd_ok else
           "batched torch.linalg.eigh of the blocks' Gram matrices on the device (this torch build has no working device SVD)"}
    step = classical.default_step(sens)
    with torch.no_grad():
        for name, mask in masks(dev).items():
            mk = ops.apply_mask(kspace, mask)
            acq = dc.Acquisition(mk, mask, sens)
            zf, tiled = acq.zero_filled(), acq.tiled
            thresh = classical.block_sigma_max(zf, BLOCK) * LAM
            theta = step * thresh

            def block_svt(v, sh, sw):
                nbh, nbw = -(-(H + sh) // BLOCK), -(-(W + sw) // BLOCK)
                x = torch.zeros((T, nbh * BLOCK, nbw * BLOCK), dtype=torch.complex64, device=v.device)
                x[:, sh:sh + H, sw:sw + W] = torch.view_as_complex(v.reshape(T, H, W, 2))
                m = x.reshape(T, nbh, BLOCK, nbw, BLOCK).permute(1, 3, 2, 4, 0).reshape(nbh * nbw, BLOCK * BLOCK, T)
                if svd_ok:
                    u, s, vh = torch.linalg.svd(m, full_matrices=False)
                    y = (u * (s - theta).clamp_min(0.0).unsqueeze(1)) @ vh
                else:
                    lam, vec = torch.linalg.eigh(m.conj().transpose(1, 2) @ m)
                    sq = lam.clamp_min(0.0).sqrt()
                    hh = torch.where(sq > theta, 1.0 - theta / sq.clamp_min(1e-30), torch.zeros_like(sq))
                    y = m @ ((vec * hh.unsqueeze(1)) @ vec.conj().transpose(1, 2))
                y = y.reshape(nbh, nbw, BLOCK, BLOCK, T).permute(4, 0, 2, 1, 3).reshape(T, nbh * BLOCK, nbw * BLOCK)
                return torch.view_as_real(y[:, sh:sh + H, sw:sw + W].contiguous()).reshape(v.shape)

            def composed(iters):
                x = zf
                for k in range(iters):
                    g = ops.image_dc(x, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled)
                    x = block_svt(x - step * g, int(shifts[k, 0]), int(shifts[k, 1]))
                return x

            def fused(iters):
                return ops.llr_solve(zf, sens, mask, step, thresh, BLOCK, iters, shifts=shifts[:iters], sens_tiled=tiled)
            xf, xc = fused(ITERS), composed(ITERS)
            _, rec, info = ops.llr_solve(zf, sens, mask, step, thresh, BLOCK, ITERS, shifts=shifts, sens_tiled=tiled, record=True)
            res = {"mask_fraction": float(mask.float().mean()),
                   "fused_workspace_bytes": int(ops.lib().cine_llr_solve_ws_bytes(1, T, C, H, W, mask.shape[4], BLOCK, ITERS)),
                   "fused_vs_composed_max_abs_over_peak": float((xf - xc).abs().max() / xc.abs().max()),
                   "worst_jacobi_residual": float(info[:, 1].max()), "most_sweeps": int(info[:, 2].max()),
                   "blocks_per_iteration": [int(info[:, 3].min()), int(info[:, 3].max())]}
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
            # the launches of one iteration, each alone, on the first iteration's operands
            g = ops.image_dc(zf, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled)
            out = torch.empty_like(zf)
            parts = {"operator": lambda: ops.image_dc(zf, sens, zf, mask, weights=(1.0, 0.0, -1.0), sens_tiled=tiled),
                     "prox_unshifted": lambda: ops.llr_prox(zf, g, step, thresh, BLOCK, (0, 0), xnew=out),
                     "prox_shifted": lambda: ops.llr_prox(zf, g, step, thresh, BLOCK, (3, 5), xnew=out),
                     "prox_shifted_with_records": lambda: ops.llr_prox(zf, g, step, thresh, BLOCK, (3, 5), xnew=out, record=True)}
            res["launch_us"] = {k: median(measure(fn, dev)[0]) * 1e3 for k, fn in parts.items()}
            _, _, one = ops.llr_prox(zf, g, step, thresh, BLOCK, (3, 5), record=True)
            res["prox_shifted_sweeps"], res["prox_shifted_blocks"] = int(one[2]), int(one[3])
            doc[name] = res
            print(json.dumps({name: {k: v for k, v in res.items() if not (isinstance(v, dict) and "ms" in v)}}), flush=True)
        mask = masks(dev)["row"]
        mk = ops.apply_mask(kspace, mask)
        model = classical.LocallyLowRank(iters=ITERS, lam=LAM, block=BLOCK).eval()
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
        doc["pipeline"] = {"model": f"LocallyLowRank(iters={ITERS})", "slots": SLOTS, "slices": SLICES, "slices_per_s": median(rates), "runs": rates}
        print(json.dumps({"pipeline": doc["pipeline"]}), flush=True)
    ls_path = os.path.join(ROOT, "profiles", "ls_rate.json")
    if os.path.exists(ls_path):                              # L+S's iteration, measured by tools/ls_rate.py at its own commit
        with open(ls_path) as f:
            ls = json.load(f)
        doc["ls_rate_for_comparison"] = {"commit": ls.get("commit"), **{n: ls[n].get("fused_us_per_iteration") for n in ("row", "plane") if n in ls}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
