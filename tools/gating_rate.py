#!/usr/bin/env python3
"""What retrospective gating on the device costs and what it saves, in ONE process.

    python tools/gating_rate.py [--out profiles/gating_rate.json] [--commit SHA] [--no-pipeline] [--hw-queues 16]

The kernel alone, at 15 x 384 x 144 x 15 and 15 x 416 x 208 x 30 (frames, x, y, coil), hipEvent medians of 10 single calls (and the time
per call of 50 calls enqueued back to back), with three plans:
  * "r4_nearest": every fourth line, shifted from frame to frame, plus 16 centre lines, one readout per acquired line (weight 1);
  * "linear": the same number of readouts at random cardiac phases, four or so per line, interpolated onto every frame (two entries per
    row: the kernel reads twice what it writes);
  * "full": every line of every frame acquired once.
Beside each, in the same run and timed in turn, cine_raw_ingest at the same output size -- the existing one-pass kernel over the same
array, which reads and writes every byte -- with its own spread (min and max of its 10 calls).
Through the pipeline (cfg-2 model, 10 slots, pinned host memory, GPU_MAX_HW_QUEUES=16 set by the tool): slices per second
of ``submit_readouts(lines, plan, ...)`` against ``submit_raw(host-gated array, apply_mask=False)`` for the same r4_nearest scans, medians
of 3 regions of 40 slices, the two in turn, and the bytes either copies per slice.
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
os.environ["GPU_MAX_HW_QUEUES"] = "16"                  # before the first HIP call: the 10 slot streams and the copy stream get queues of their own
if "--hw-queues" in sys.argv[1:-1]:                     # another count (at most 32)
    os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, int(sys.argv[sys.argv.index("--hw-queues") + 1])))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((15, 384, 144, 15), (15, 416, 208, 30))
STEPS, BURST, SLOTS, SLICES, WARM, REGIONS, SCANS = 10, 50, 10, 40, 8, 3, 4
FILTER, SCALING = (0.7, 0.0, 0.3, 0.3), 1e6


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def r4_lines(t, nx, shift=0):
    """uint8 (t, nx): every fourth line, shifted per frame, plus 16 centre lines."""
    a = np.zeros((t, nx), dtype=np.uint8)
    for f in range(t):
        a[f, (f + shift) % 4::4] = 1
    a[:, nx // 2 - 8:nx // 2 + 8] = 1
    return a


def make_plan(pattern, t, nx, rng):
    """(plan, n_lines) of a pattern, from schedules only."""
    from cine_hip import gating as G
    if pattern == "linear":
        n = int(r4_lines(t, nx).sum())
        pe = np.concatenate((np.arange(nx), rng.integers(0, nx, size=n - nx)))           # every line at least once
        trig = rng.uniform(0.0, 1000.0, size=n)
        return G.plan_gating(pe, trig, 1000.0, t, nx, mode="linear")
    acq = np.ones((t, nx), dtype=np.uint8) if pattern == "full" else r4_lines(t, nx)
    f, x = np.nonzero(acq)
    return G.plan_gating(x, (f + 0.5) / t * 1000.0, 1000.0, t, nx, mode="nearest")


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_pair(fa, fb):
    """The two calls timed in turn, so that a drift of the machine's load falls on both: STEPS single calls each between an event pair of
    their own, then 5 bursts each of BURST calls back to back between one pair."""
    for _ in range(3):
        fa(); fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(STEPS):
        ms[0].append(event_ms(fa)); ms[1].append(event_ms(fb))
    bursts = ([], [])
    for _ in range(5):
        for k, fn in enumerate((fa, fb)):
            bursts[k].append(event_ms(lambda: [fn() for _ in range(BURST)]) / BURST)
    return [{"median_us": 1e3 * median(m), "min_us": 1e3 * min(m), "max_us": 1e3 * max(m), "burst_us": 1e3 * median(b)} for m, b in zip(ms, bursts)]


def kernel_rows(dev):
    from cine_hip import gating as G, ops
    rows = []
    rng = np.random.default_rng(7)
    for t, nx, ny, c in SHAPES:
        out = torch.empty((t, nx, ny, c, 2), dtype=torch.float32, device=dev)
        ing_in = torch.empty((t, nx, ny, c, 2), dtype=torch.float32, device=dev).normal_()
        ing_out = torch.empty((t, c, nx, ny, 2), dtype=torch.float32, device=dev)
        nbytes = out.numel() * 4
        for pattern in ("r4_nearest", "linear", "full"):
            plan = make_plan(pattern, t, nx, rng)
            lines = torch.empty((plan.n_lines, ny, c, 2), dtype=torch.float32, device=dev).normal_()
            csr = plan.to(dev)
            gate, ingest = timed_pair(lambda: G.gate_into(lines, *csr, plan.n_lines, out),
                                      lambda: ops.raw_ingest(ing_in, t, SCALING, out=ing_out))
            read = plan.entries * ny * c * 8
            row = {"shape": [t, nx, ny, c], "pattern": pattern, "n_lines": plan.n_lines, "entries": plan.entries,
                   "acquired_rows": int(plan.acquired.sum()), "rows": plan.rows, "bytes_written": nbytes, "bytes_read": read,
                   "gate": gate, "raw_ingest": ingest, "raw_ingest_bytes": 2 * nbytes,
                   "gate_TBps": (nbytes + read) / gate["median_us"] / 1e6, "raw_ingest_TBps": 2 * nbytes / ingest["median_us"] / 1e6,
                   "gate_over_ingest": gate["median_us"] / ingest["median_us"],
                   "ingest_spread": ingest["max_us"] / ingest["min_us"]}
            row["no_slower_than_ingest_beyond_its_spread"] = bool(gate["median_us"] <= ingest["max_us"])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del lines, csr
        del out, ing_in, ing_out
        torch.cuda.empty_cache()
    return rows


def pipeline_rows(dev):
    import bench
    from cine_hip import gating as G, synth
    from cine_hip.pipeline import SlicePipeline
    cfg = bench.CONFIGS[2]()
    net = cfg["hip"]().eval()
    synth.fill_parameters_(net, cfg["wseed"], keep=cfg["keep"])
    net = net.to(dev)
    rows = []
    for t, nx, ny, c in SHAPES:
        crop = (min(200, nx), min(200, ny))
        rng = np.random.default_rng(nx + c)
        scans = []
        for j in range(SCANS):
            acq = r4_lines(t, nx, shift=j)
            f, x = np.nonzero(acq)
            lines = (1e-6 * rng.standard_normal((f.shape[0], ny, c, 2), dtype=np.float32)).view(np.complex64)[..., 0]
            plan = G.plan_gating(x, (f + 0.5) / t * 1000.0, 1000.0, t, nx)
            gated = np.zeros((t, nx, ny, c), dtype=np.complex64)                       # today's way: gated on the host, mostly zeros
            gated[f, x] = lines
            m = (rng.uniform(size=(1, t, 1, crop[0], 1, 1)) < 0.25).astype(np.uint8)
            m[:, :, :, crop[0] // 2 - 8 - j:crop[0] // 2 + 8 + j] = 1
            scans.append((torch.from_numpy(lines).pin_memory(), plan, torch.from_numpy(gated).pin_memory(), torch.from_numpy(m).to(dev)))
        kw = dict(crop_shape=crop, filter_size=FILTER, scaling=SCALING)
        plan0 = scans[0][1]
        row = {"shape": [t, nx, ny, c], "crop": list(crop), "pattern": "r4_nearest", "slots": SLOTS, "slices_per_region": SLICES,
               "h2d_bytes_per_slice_readouts": scans[0][0].numel() * 8 + 4 * (plan0.rows + 1) + 8 * plan0.entries,
               "h2d_bytes_per_slice_raw": scans[0][2].numel() * 8}

        def run(pipe, readouts, count):
            got = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(count):
                lines, plan, gated, mask = scans[k % SCANS]
                if readouts:
                    pipe.submit_readouts(lines, plan, mask, **kw)
                else:
                    pipe.submit_raw(gated, mask, apply_mask=False, n_frames=t, **kw)
                for _ in pipe.results():
                    got += 1
            for _ in pipe.drain():
                got += 1
            torch.cuda.synchronize()
            assert got == count
            return count / (time.perf_counter() - t0)

        with SlicePipeline(net, slots=SLOTS) as pipe:
            lines, plan, gated, mask = scans[0]
            pipe.submit_readouts(lines, plan, mask, tag="a", **kw)
            pipe.submit_raw(gated, mask, tag="b", apply_mask=False, n_frames=t, **kw)
            got = dict(pipe.drain())
            row["bit_identical"] = bool(torch.equal(got["a"], got["b"]))
            run(pipe, True, WARM); run(pipe, False, WARM)
            rs = ([], [])
            for _ in range(REGIONS):                                                   # the two in turn
                rs[0].append(run(pipe, True, SLICES)); rs[1].append(run(pipe, False, SLICES))
            assert pipe.set_builds == 1
        row["submit_readouts_slices_per_s"], row["regions_submit_readouts"] = median(rs[0]), rs[0]
        row["submit_raw_slices_per_s"], row["regions_submit_raw"] = median(rs[1]), rs[1]
        row["readouts_over_raw"] = row["submit_readouts_slices_per_s"] / row["submit_raw_slices_per_s"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del scans
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-pipeline", action="store_true", help="the kernel rows only")
    ap.add_argument("--hw-queues", type=int, default=16, help="GPU_MAX_HW_QUEUES of this process (<= 32; read before torch is imported)")
    args = ap.parse_args()
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    commit, csrc = _stamp(args.commit)
    doc = {"what": "cine_gate_readouts beside cine_raw_ingest at equal output size; submit_readouts against submit_raw of the host-gated array",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS,
           "statistic": "hipEvent median of the single calls; pipeline: median of the regions", "commit": commit, "csrc_sha256": csrc}
    doc["kernels"] = kernel_rows(dev)
    if not args.no_pipeline:
        doc["pipeline"] = pipeline_rows(dev)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k not in ("kernels", "pipeline")}), flush=True)


if __name__ == "__main__":
    main()
