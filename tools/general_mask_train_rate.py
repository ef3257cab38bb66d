#!/usr/bin/env python3
"""What one TRAINING step costs with a sampling mask that varies along w, literal chain against image-space operators, in ONE process.

    python tools/general_mask_train_rate.py [--config 2|3|4|5 ...] [--steps 10] [--regions 3] [--out profiles/general_mask_train.json] [--commit SHA]

A training step is forward + SSIMLoss + backward + Adam on a BASELINE configuration (tools/train_bench.py's models) at 1 x 15 coils x 15 frames
x 200 x 200.  Mask: tools/general_mask_rate.py's -- an R = 4 row pattern (every fourth row, shifted per frame, plus 16 centre rows) times a
75 % readout window.  Per configuration, three settings, each with a model and an optimiser of its own (the same seed):
  * literal   ops.GENERAL_MASK_FUSED_TRAIN off: the coil-wise k-space chain (SensExpandFn, soft_dc_blend / masked_residual_backward, SensReduceFn);
  * fused     both switches on: ImageDcFn / ImageDcFixedFn / ConjGradFn on cine_normal_op_general, cine_image_dc_general_sens_grad for the maps;
  * row_mask  the row pattern alone, for scale (ImageDcFn on cine_image_dc, cine_conj_grad_rec).
The settings ALTERNATE over `--regions` regions (the first stretch of a process runs slow, and a card's clocks drift: no setting owns a
position).  A region of a setting: the general-mask workspaces of the previous setting released, 3 warm-up steps, then `--steps` (>= 10)
steps, every step between two stream synchronisations (wall clock), and torch.cuda.max_memory_allocated over the timed steps (the peak
statistics reset after the warm-up).  Reported per setting: the median of the regions' medians, every region's median, their spread
(max - min) / median, every region's peak, and as `peak_bytes` the peak of the LAST region: the three models stay resident, and only once
every one of them has stepped is what they hold between steps -- weights, Adam state, gradients -- the same baseline for all settings (with
one region the later settings carry more of it than the first).  Counter 15 of
cine_diag_counter confirms the route of every region, and counts per step how many of its passes ran; cine_image_dc_general_sens_grad runs
only where the maps have a gradient (cfg 3 and 5: the sensitivity network trains; cfg 2 and 4 get the caller's maps).  The sensitivity networks read
their ACS window off a row mask, so the models get `acs=` (the 16 centre rows) or the caller's maps, the same in all three settings.
One JSON line per configuration; --out writes the whole document, stamped with the commit and a sha256 over csrc/."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-cine-cardiac-mri_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")        # before the first HIP call, as bench.py does

import torch  # noqa: E402

T, C, H, W = 15, 15, 200, 200
ACS = (H // 2 - 8, 16)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def measure(step, steps, dev):
    """One region: (the timed steps in ms, the peak over them, the last loss)."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, torch.cuda.max_memory_allocated(dev), float(loss.detach())


def run_config(cfg, steps, nregions, dev):
    import reconstruction.models as M
    from reconstruction.utils import SSIMLoss
    from cine_hip import ops, synth
    from cine_hip._lib import lib
    from general_mask_rate import masks
    ex = synth.make_cine_slice(T, C, H, W, accel={2: 4, 3: 8, 4: 6, 5: 8}[cfg], seed=0)
    make = {2: lambda: M.VarNet(6, 8, 3, 16, 3, "XF"), 3: lambda: M.XPDNet(num_cascades=10, sens_chans=8, sens_pools=3, n_primal=5, dynamic_type="XT"),
            4: lambda: M.CineNet(6, 6, 16, 3, "3D"), 5: lambda: M.VarNet_RNN(5, 8, 3, 16)}[cfg]
    row, general = masks(dev)
    kfull, target, sens = ex["kspace"].to(dev), ex["target"].to(dev), ex["sens_maps"].to(dev)
    lossf = SSIMLoss().to(dev)
    res = {"config": cfg, "model": {2: "VarNet XF, caller's maps", 3: "XPDNet XT", 4: "CineNet 3D", 5: "VarNet_RNN"}[cfg]}
    settings = {}
    for name, mask, train_on in (("literal", general, False), ("fused", general, True), ("row_mask", row, True)):
        torch.manual_seed(0)
        net = make()
        synth.fill_parameters_(net, 1)
        net = net.to(dev).train()
        mk = ops.apply_mask(kfull, mask)
        settings[name] = (net, torch.optim.Adam(net.parameters(), lr=3e-4), train_on,
                          ((mk, mask, sens), {}) if cfg in (2, 4) else ((mk, mask), {"acs": ACS}))
        res[name] = {"regions_ms": [], "regions_peak_bytes": [], "steps_ms": []}

    def stepper(net, opt, args, kw):
        def step():
            opt.zero_grad(set_to_none=True)
            out = net(*args, **kw)
            loss = lossf(out.unsqueeze(1), target.unsqueeze(1), target.max())
            loss.backward()
            opt.step()
            return loss
        return step
    for _ in range(nregions):
        for name, (net, opt, train_on, (args, kw)) in settings.items():
            ops.GENERAL_MASK_FUSED_TRAIN = train_on
            ops.release_general_workspaces()
            try:
                lib().cine_diag_counter(15, 1)
                ms, peak, loss = measure(stepper(net, opt, args, kw), steps, dev)
                passes = lib().cine_diag_counter(15, 1) / (steps + 3)
            finally:
                ops.GENERAL_MASK_FUSED_TRAIN = False
            assert (passes > 0) == (name == "fused"), (name, passes)
            r = res[name]
            r["regions_ms"].append(median(ms)); r["regions_peak_bytes"].append(peak); r["steps_ms"].extend(ms)
            r["mask_plane_column_passes_per_step"], r["loss_after"] = passes, loss
    for name in settings:
        r, v = res[name], res[name]["regions_ms"]
        r.update(median_ms=median(v), spread=(max(v) - min(v)) / median(v), peak_bytes=r["regions_peak_bytes"][-1])
    del settings
    ops.release_general_workspaces()
    res["literal_over_fused_time"] = res["literal"]["median_ms"] / res["fused"]["median_ms"]
    res["literal_minus_fused_peak_bytes"] = res["literal"]["peak_bytes"] - res["fused"]["peak_bytes"]
    res["fused_over_row_mask_time"] = res["fused"]["median_ms"] / res["row_mask"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, nargs="+", default=[2], choices=[2, 3, 4, 5])
    ap.add_argument("--steps", type=int, default=10, help="timed steps per region (at least 10)")
    ap.add_argument("--regions", type=int, default=3, help="regions per setting, the settings alternating")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit to stamp the result with (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps: at least 10")
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    commit, csrc = _stamp(args.commit)
    doc = {"shape": [1, T, C, H, W], "mask": "R = 4 rows (+ 16 centre rows) x 75 % readout window", "kspace_bytes": T * C * H * W * 8,
           "step": "forward + SSIMLoss + backward + Adam, wall clock between two stream synchronisations", "warmup_steps": 3, "steps": args.steps, "regions": args.regions,
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "commit": commit,
           "csrc_sha256": csrc, "configs": {}}
    for cfg in args.config:
        res = run_config(cfg, args.steps, args.regions, dev)
        doc["configs"][str(cfg)] = res
        print(json.dumps({k: (v if not isinstance(v, dict) else {kk: vv for kk, vv in v.items() if kk != "steps_ms"}) for k, v in res.items()}), flush=True)
        if args.out:                                                    # after every configuration: a later one that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
