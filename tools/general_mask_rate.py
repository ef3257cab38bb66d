#!/usr/bin/env python3
"""What a sampling mask that varies along w costs at 1 x 15 coils x 15 frames x 200 x 200, fused against literal, in ONE process.

    python tools/general_mask_rate.py [--out profiles/general_mask_rate.json] [--slots 4] [--slices 40] [--regions 3]

Mask: an R = 4 row pattern (every fourth row, shifted per frame, plus 16 centre rows) times a 75 % readout window (the first quarter of
every readout is missing: a partial echo).  ``ops.GENERAL_MASK_FUSED`` switches between the image-space operator with both line passes
(cine_image_dc_general) and the literal chain on the coil-wise k-space (sens_expand -> torch elementwise DC line -> sens_reduce).
Reported, each as hipEvent medians of 20 calls per region, `--regions` regions with the variants alternating, and the spread
(max - min) / median of the regions' medians:
  * one cascade's data-consistency step: fused, literal, and beside them the row-mask operator (cine_image_dc_t) on the row pattern alone;
  * a config-2 VarNet slice (bench.py's model, the caller's sensitivity maps) alone, eager: fused, literal, row mask;
  * SlicePipeline slices/s (device-resident inputs): fused, literal, row mask.
One JSON line per block; --out writes the whole document."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-cine-cardiac-mri_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # before the first HIP call, as bench.py does

import torch  # noqa: E402

T, C, H, W = 15, 15, 200, 200


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def event_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def regions(fns, n):
    """n regions of 20 timed calls of every variant in `fns` (name -> callable), the variants alternating region by region:
    name -> {median_ms (of the regions' medians), regions_ms, spread}."""
    meds = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            meds[k].append(median(event_ms(fn)))
    return {k: {"median_ms": median(v), "regions_ms": v, "spread": (max(v) - min(v)) / median(v)} for k, v in meds.items()}


def masks(dev):
    row = torch.zeros(1, T, 1, H, 1, 1, dtype=torch.uint8)
    for f in range(T):
        row[0, f, 0, f % 4::4] = 1
    row[:, :, :, H // 2 - 8:H // 2 + 8] = 1
    general = row.expand(1, T, 1, H, W, 1).clone()
    general[:, :, :, :, :W // 4] = 0                    # 75 % readout window
    return row.to(dev), general.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--regions", type=int, default=3)
    args = ap.parse_args()
    import bench
    from cine_hip import ops, synth
    from cine_hip._lib import lib
    from cine_hip.pipeline import SlicePipeline
    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS[2]()
    net = cfg["hip"]().eval()
    synth.fill_parameters_(net, cfg["wseed"], keep=cfg["keep"])
    net = net.to(dev)
    ex = bench.make_slices(cfg, [0])[0]
    sens, kfull = ex["sens_maps"].to(dev), ex["kspace"].to(dev)
    row, general = masks(dev)
    mk_row, mk_gen = ops.apply_mask(kfull, row), ops.apply_mask(kfull, general)
    doc = {"shape": [1, T, C, H, W], "mask": "R = 4 rows (+ 16 centre rows) x 75 % readout window",
           "sampled_fraction": float(general.float().mean()), "device": torch.cuda.get_device_name(dev),
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "calls_per_region": 20, "regions": args.regions}

    # ---- one cascade's DC step
    lam = net.cascades[0].lambda_reg.detach()
    with torch.no_grad():
        x = ops.sens_reduce(mk_gen, sens)
        zf_gen = ops.sens_reduce(ops.apply_mask(mk_gen, general), sens, destroy_input=True)
        zf_row = ops.sens_reduce(ops.apply_mask(mk_row, row), sens, destroy_input=True)
        tiled = ops.sens_tile_pack(sens)

        def fused():
            return ops.image_dc(x, sens, zf_gen, general, lam)

        def literal():
            k = ops.soft_dc_blend(ops.sens_expand_dc(x, sens), mk_gen, general, lam)
            return ops.sens_reduce(k, sens, destroy_input=True)

        def rowmask():
            return ops.image_dc(x, sens, zf_row, row, lam, sens_tiled=tiled)
        lib().cine_diag_counter(15, 1)
        a, b = fused(), literal()
        assert lib().cine_diag_counter(15, 1) == 1
        peak = float(b.abs().max())
        dc = {"block": "dc_step", "fused_vs_literal_max_abs_over_peak": float((a - b).abs().max()) / peak}
        dc.update(regions({"fused": fused, "literal": literal, "row_mask": rowmask}, args.regions))
    dc["literal_over_fused"] = dc["literal"]["median_ms"] / dc["fused"]["median_ms"]
    doc["dc_step"] = dc
    print(json.dumps(dc), flush=True)

    # ---- a config-2 slice alone
    def forward(mk, m):
        with torch.no_grad():
            return net(mk, m, sens)
    def flagged(flag, mk, m):
        def run():
            ops.GENERAL_MASK_FUSED = flag
            try:
                return forward(mk, m)
            finally:
                ops.GENERAL_MASK_FUSED = True
        return run
    sl = {"block": "cfg2_slice_eager"}
    of, ol = flagged(True, mk_gen, general)().clone(), flagged(False, mk_gen, general)().clone()
    sl.update(regions({"fused": flagged(True, mk_gen, general), "literal": flagged(False, mk_gen, general),
                       "row_mask": flagged(True, mk_row, row)}, args.regions))
    sl["fused_vs_literal_max_abs_over_peak"] = float((of - ol).abs().max() / ol.abs().max())
    sl["literal_over_fused"] = sl["literal"]["median_ms"] / sl["fused"]["median_ms"]
    doc["cfg2_slice_eager"] = sl
    print(json.dumps(sl), flush=True)

    # ---- SlicePipeline: one pipeline per variant (the switch is read when a set's graphs are captured), regions alternating
    def region(pipe, mk, m, n):
        got = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            pipe.submit(mk, m, sens)
            got += len(list(pipe.results()))
        got += len(list(pipe.drain()))
        torch.cuda.synchronize()
        assert got == n
        return n / (time.perf_counter() - t0)
    variants = {"fused": (True, mk_gen, general), "literal": (False, mk_gen, general), "row_mask": (True, mk_row, row)}
    pipes, rates = {}, {k: [] for k in variants}
    try:
        for k, (flag, mk, m) in variants.items():
            ops.GENERAL_MASK_FUSED = flag
            pipes[k] = SlicePipeline(net, slots=args.slots)
            region(pipes[k], mk, m, 2 * args.slots)                 # builds the set, warm-up
            ops.GENERAL_MASK_FUSED = True
        for _ in range(args.regions):
            for k, (_, mk, m) in variants.items():
                rates[k].append(region(pipes[k], mk, m, args.slices))
    finally:
        ops.GENERAL_MASK_FUSED = True
        for p_ in pipes.values():
            p_.close()
    pl = {"block": "slice_pipeline", "slots": args.slots, "slices_per_region": args.slices}
    for k, rs in rates.items():
        pl[k] = {"slices_per_s": median(rs), "regions": rs, "spread": (max(rs) - min(rs)) / median(rs)}
    pl["fused_over_literal"] = pl["fused"]["slices_per_s"] / pl["literal"]["slices_per_s"]
    doc["slice_pipeline"] = pl
    print(json.dumps(pl), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
