#!/usr/bin/env python3
"""What the ESPIRiT calibration costs at 15 coils x 200 x 200, stage by stage, and what it does to SlicePipeline's rate, in ONE process.

    python tools/espirit_rate.py [--out profiles/espirit_inflight_rate.json] [--slots 4] [--slices 24] [--regions 3]

For r = 15 and r = 24 (``ecalib -r``), hipEvent medians of 20 calls per region:
  * gram        cine_espirit_gram
  * projector   cine_espirit_projector with 60 and with 1 Newton-Schulz steps.  ``sign_ms`` = (t60 - t1) * 60 / 59 is the 120 GEMMs of
                the iteration; ``lam_ms`` = t60 - sign_ms is the rest of the entry point (8 squarings with their norms, the Rayleigh
                quotient, the start, the residual's GEMM and reduction, the rounding to complex64)
  * lag_ifft    cine_espirit_lag_kernels + the inverse transform of the c x c operator
  * eig         cine_espirit_eig, 100 power iterations per pixel
  * sign_call   the whole ``espirit_maps(method="sign")``, device time, and ``eigh_call_host_ms``: the whole ``method="eigh"`` call as
                the host sees it (it waits for the device inside torch.linalg.eigh and the boolean index)
Then SlicePipeline slices/s of the config-4 CineNet (bench.py's model, 15 coils x 15 frames x 200 x 200, device-resident inputs,
``ecalib_r=15``), the variants alternating region by region:
  * espirit       ``submit(mk, mask, "espirit")``: the calibration inside the slot's graph
  * given_maps    ``submit(mk, mask, maps)``: the caller's maps, no calibration at all
  * ecalib_loop   today's loop: ``frontend.ecalib`` (method "eigh") on the slice's time average, then ``submit`` with its maps
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
K, THRESH, CROP = 6, 1e-3, 0.8


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
    meds = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            meds[k].append(median(event_ms(fn)))
    return {k: {"median_ms": median(v), "regions_ms": v, "spread": (max(v) - min(v)) / median(v)} for k, v in meds.items()}


def stages(kavg, r, nreg):
    from cine_hip import frontend as FE, ops
    from cine_hip._lib import check, lib
    dev = kavg.device
    gram = FE.espirit_gram(kavg, r, K)
    proj, _, resid = FE.espirit_projector(gram, THRESH, 60)
    kpad = torch.empty((C * C, H, W, 2), device=dev)
    maps, lam = torch.empty((C, H, W, 2), device=dev), torch.empty((H, W), device=dev)

    def lag_ifft():
        check(lib().cine_espirit_lag_kernels(proj.data_ptr(), kpad.data_ptr(), C, K, H, W, ops._stream()))
        return ops.fft2c(kpad, inverse=True)

    m = lag_ifft()

    def eig():
        check(lib().cine_espirit_eig(m.data_ptr(), maps.data_ptr(), lam.data_ptr(), C, H * W, 100, CROP, ops._stream()))

    out = regions({"gram": lambda: FE.espirit_gram(kavg, r, K),
                   "projector_60": lambda: FE.espirit_projector(gram, THRESH, 60),
                   "projector_1": lambda: FE.espirit_projector(gram, THRESH, 1),
                   "lag_ifft": lag_ifft, "eig": eig,
                   "sign_call": lambda: FE.espirit_maps(kavg, r=r, method="sign")}, nreg)
    t60, t1 = out["projector_60"]["median_ms"], out["projector_1"]["median_ms"]
    out["sign_ms"] = (t60 - t1) * 60.0 / 59.0
    out["lam_ms"] = t60 - out["sign_ms"]
    host = []
    for _ in range(2 + 5 * nreg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        FE.espirit_maps(kavg, r=r, method="eigh")
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    out["eigh_call_host_ms"] = median(host[2:])
    out["residual"] = float(resid.cpu()[0])
    out["r"], out["n"] = r, K * K * C
    return out


def pipeline(dev, slots, n_slices, nreg, r):
    import reconstruction.models as M
    from cine_hip import frontend as FE, synth
    from cine_hip.pipeline import SlicePipeline
    net = M.CineNet(6, 6, 16, 3, "3D").eval()                # bench.py's config 4
    synth.fill_parameters_(net, 7, keep=("lambda",))
    net = net.to(dev)
    exs = [synth.make_cine_slice(T, C, H, W, accel=6, seed=s) for s in range(4)]
    ins = [(e["masked_kspace"].to(dev), e["mask"].to(torch.uint8).to(dev), e["sens_maps"].to(dev)) for e in exs]

    def run(pipe, feed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(n_slices):
            feed(pipe, j, *ins[j % len(ins)])
            for _ in pipe.results():
                pass
        for _ in pipe.drain():
            pass
        torch.cuda.synchronize()
        return n_slices / (time.perf_counter() - t0)

    def loop(pipe, j, mk, mask, _):
        avg = torch.view_as_complex(FE.time_average(mk[0])).permute(1, 2, 0)[None]           # (1, x, y, coil), transforms.py:427
        maps = FE.ecalib(avg, r=r).permute(2, 0, 1).contiguous()
        pipe.submit(mk, mask, torch.view_as_real(maps)[None, None], tag=j)

    feeds = {"espirit": lambda p, j, mk, mask, _: p.submit(mk, mask, "espirit", tag=j, ecalib_r=r),
             "given_maps": lambda p, j, mk, mask, s: p.submit(mk, mask, s, tag=j),
             "ecalib_loop": loop}
    pipes = {k: SlicePipeline(net, slots=slots) for k in feeds}
    rates = {k: [] for k in feeds}
    try:
        for k in feeds:
            run(pipes[k], feeds[k])                          # builds the set
        for _ in range(nreg):
            for k in feeds:
                rates[k].append(run(pipes[k], feeds[k]))
    finally:
        for p in pipes.values():
            p.close()
    out = {k: {"slices_per_s": median(v), "regions": v, "spread": (max(v) - min(v)) / median(v)} for k, v in rates.items()}
    out["espirit_over_ecalib_loop"] = out["espirit"]["slices_per_s"] / out["ecalib_loop"]["slices_per_s"]
    out["espirit_over_given_maps"] = out["espirit"]["slices_per_s"] / out["given_maps"]["slices_per_s"]
    out.update(model="CineNet(6, 6, 16, 3, '3D') (config 4)", slots=slots, slices_per_region=n_slices, ecalib_r=r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--slices", type=int, default=24)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    from cine_hip import synth
    dev = torch.device("cuda:0")
    ex = synth.make_cine_slice(T, C, H, W, accel=4, center_lines=10, seed=2)
    kavg = ex["masked_kspace"][0].mean(0).contiguous().to(dev)
    doc = {"shape": [C, H, W], "device": torch.cuda.get_device_name(0), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
           "calls_per_region": 20, "regions": a.regions, "stages": {}}
    for r in (15, 24):
        doc["stages"][f"r{r}"] = stages(kavg, r, a.regions)
        print(json.dumps({"block": f"stages_r{r}", **doc["stages"][f"r{r}"]}), flush=True)
    if not a.no_pipeline:
        doc["pipeline"] = pipeline(dev, a.slots, a.slices, a.regions, 15)
        print(json.dumps({"block": "pipeline", **doc["pipeline"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
