#!/usr/bin/env python3
"""Cine slices/s through the public SlicePipeline (cine_hip.pipeline), printed as one JSON line.

    python tools/pipeline_rate.py [--config {2,3,4,5}] [--slots 10] [--slices 300] [--warmup 20]

The model and the synthetic slices are bench.py's (CONFIGS, make_slices): `slots` different slices, submitted round-robin.
Three input forms -- k-space resident in HBM, pinned host tensors, pageable numpy arrays (complex64) -- each with the
outputs returned as device tensors and as pinned host tensors (out="host").  One pipeline per output form (captured
once); every region submits `slices` slices, takes the finished ones as it goes (results()), drains, and is timed from
the first submit to the last result.  Compare `value_device_in` with bench.py's `value` and `value_pinned_in` with
its `value_with_h2d` (run bench.py --full beside it).  `host_copy_GBps` is the host memcpy rate of one slice's
k-space from a numpy array into a pinned buffer (what a pageable input costs inside submit)."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402


def region(pipe, inputs, n):
    """Submit n slices cycling over `inputs`; returns (seconds, slices handed out)."""
    got = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        mk, mask, sens = inputs[k % len(inputs)]
        pipe.submit(mk, mask, sens)
        for _ in pipe.results():
            got += 1
    for _ in pipe.drain():
        got += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4, 5))
    ap.add_argument("--slots", type=int, default=10)
    ap.add_argument("--slices", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import bench
    from cine_hip import synth
    from cine_hip.pipeline import SlicePipeline

    cfg = bench.CONFIGS[args.config]()
    dev = torch.device("cuda:0")
    S = args.slots
    exs = bench.make_slices(cfg, list(range(S)))
    net = cfg["hip"]().eval()
    synth.fill_parameters_(net, cfg["wseed"], keep=cfg["keep"])
    net = net.to(dev)
    sens = cfg["needs_sens"]
    as_c = lambda x: np.ascontiguousarray(torch.view_as_complex(x).numpy())
    forms = {
        "device": [(e["masked_kspace"].to(dev), e["mask"].to(dev), e["sens_maps"].to(dev) if sens else None) for e in exs],
        "pinned": [(e["masked_kspace"].pin_memory(), e["mask"].pin_memory(), e["sens_maps"].pin_memory() if sens else None) for e in exs],
        "numpy": [(as_c(e["masked_kspace"]), e["mask"].numpy(), as_c(e["sens_maps"]) if sens else None) for e in exs],
    }
    with torch.no_grad():
        d = forms["device"][0]
        want = (net(*d) if sens else net(d[0], d[1])).cpu()

    line = {"metric": "cine slices/sec through SlicePipeline", "config": args.config, "name": cfg["name"], "slots": S,
            "slices_per_region": args.slices, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
            "device": torch.cuda.get_device_name(dev)}
    for out in ("device", "host"):
        t_build = time.perf_counter()
        with SlicePipeline(net, slots=S, out=out) as pipe:
            first = forms["device"][0]
            pipe.submit(*first)
            (_, o0), = list(pipe.drain())
            line[f"setup_s_out_{out}"] = time.perf_counter() - t_build
            line[f"bit_identical_to_eager_out_{out}"] = bool(torch.equal(o0.cpu(), want))
            for form, inputs in forms.items():
                region(pipe, inputs, args.warmup)
                dt, got = region(pipe, inputs, args.slices)
                assert got == args.slices, (got, args.slices)
                key = f"value_{form}_in" + ("_host_out" if out == "host" else "")
                line[key] = args.slices / dt
    # what a pageable input costs on the host: numpy -> pinned copy of one slice's k-space, over the `slots` different arrays
    # into two alternating pinned buffers as submit does (one array alone would stay in the host's last-level cache)
    srcs = [torch.from_numpy(a.view(np.float32).reshape(a.shape + (2,))) for a, _, _ in forms["numpy"]]
    ring = [torch.empty(srcs[0].shape, dtype=torch.float32, pin_memory=True) for _ in range(2)]
    for i, x in enumerate(srcs):
        ring[i & 1].copy_(x)
    reps = 3 * len(srcs)
    t0 = time.perf_counter()
    for i in range(reps):
        ring[i & 1].copy_(srcs[i % len(srcs)])
    dt = (time.perf_counter() - t0) / reps
    dst = ring[0]
    line["host_copy_MB_per_slice"] = dst.numel() * 4 / 1e6
    line["host_copy_ms_per_slice"] = dt * 1e3
    line["host_copy_GBps"] = dst.numel() * 4 / dt / 1e9
    line["host_copy_bound_slices_per_s"] = 1.0 / dt
    line["torch_threads"] = torch.get_num_threads()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
