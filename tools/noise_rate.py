#!/usr/bin/env python3
"""What a pseudo replica costs at 1 x 15 frames x 15 coils x 200 x 200, R = 4, in ONE process.

    python tools/noise_rate.py [--out profiles/noise_rate.json] [--commit SHA]

Masks: "row" = every fourth row, shifted per frame, plus 16 centre rows; "plane" = the same with the first fifth of every readout dropped
outside the centre rows, so the mask varies along w; "none" = every point.  hipEvent medians of 10 calls each:
  * (every single call is timed between two events, and so is a one-float cine_scale: the floor of that way of timing; next to each median
    stands the time per call of 50 calls enqueued back to back between one event pair)
  * cine_noise_add in place with a Cholesky factor (and, for the row mask, white), beside cine_apply_mask / cine_apply_mask2d at the same
    shape -- the existing one-pass kernel over the coil-wise k-space, the yardstick -- with the bytes each moves: the noise kernel reads
    and writes the sampled points only, the mask kernel reads and writes every point;
  * the composed torch path of one replica: torch.randn + einsum with L + mask multiply + add;
  * replicas per second for 64 replicas of the cfg-2 model (XF-VarNet, 6 cascades) through a 10-slot SlicePipeline with ``noise=``,
    the same 64 submissions without it, and the sequential loop (``pseudo_replica`` without a pipeline).
--out writes the document, stamped with the commit and a sha256 over csrc/.

    python tools/noise_rate.py --raw [--out profiles/noise_raw_rate.json] [--commit SHA]

Noise on RAW data, in front of the front-end (``raw_main``): cine_noise_add_raw against cine_noise_add at equal element counts, and the
replicas of a raw scan through ``submit_raw(..., noise=)``."""
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
STEPS, SLOTS, REPLICAS, BURST = 10, 10, 64, 50


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def measure(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def burst(fn, n=BURST):
    """ms per call of n calls enqueued back to back between one event pair (median of 5 bursts): a single short call between two events
    is mostly the cost of the pair and of an idle queue starting up, which this takes out."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / n)
    return median(ms)


def masks(dev):
    row = torch.zeros(1, T, 1, H, 1, 1, dtype=torch.uint8)
    for f in range(T):
        row[0, f, 0, f % 4::4] = 1
    row[:, :, :, H // 2 - 8:H // 2 + 8] = 1
    plane = row.expand(1, T, 1, H, W, 1).clone()
    plane[:, :, :, :H // 2 - 8, :W // 5] = 0
    plane[:, :, :, H // 2 + 8:, :W // 5] = 0
    return {"row": row.to(dev), "plane": plane.contiguous().to(dev), "none": None}


RAW_SHAPES = ((15, 416, 208, 30), (15, 384, 144, 15))       # (t, x, y, coil): the two raw matrix sizes of tools/pipeline_rate.py --raw
RAW_SCAN, RAW_CROP = (15, 384, 144, 15), (200, 144)         # the scan the replicas of the pipeline start from


def raw_main(args):
    """--raw: noise in front of the front-end.  cine_noise_add_raw alone, in place, coloured and white, every sample acquired, at the two
    raw sizes; in the same run cine_noise_add with every point sampled at the same element count ((t, c, h = x, w = y), what the raw
    kernel's values are defined by), the two timed in turn, and the composed torch path (randn + einsum + add) on the raw layout; then replicas per second of
    the cfg-2 model through a 10-slot pipeline from device-resident raw data, with and without ``noise=``."""
    import numpy as np
    import reconstruction.models as M
    from cine_hip import noise as N, ops, synth
    from cine_hip.pipeline import SlicePipeline
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    commit, csrc = _stamp(args.commit)
    doc = {"what": "cine_noise_add_raw on (t, x, y, coil) raw data beside cine_noise_add on (t, coil, x, y) at equal element counts",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS,
           "commit": commit, "csrc_sha256": csrc, "margin": 1.25, "kernels": []}

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def timed_pair(fa, fb, moved):
        """The two calls timed in turn, so that a drift of the clocks or of the machine's load falls on both: STEPS single calls each
        between an event pair of their own, then 5 bursts each of BURST calls back to back between one pair."""
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
        out = []
        for k in (0, 1):
            r = {"median_ms": median(ms[k]), "ms": ms[k], "bytes_moved": moved, "burst_ms_per_call": median(bursts[k])}
            r["burst_tb_per_s"] = moved / (r["burst_ms_per_call"] * 1e-3) / 1e12
            out.append(r)
        return out

    with torch.no_grad():
        one = torch.ones(1, device=dev)
        doc["event_pair_floor"] = {"median_ms": median(measure(lambda: ops.scale_(one, 1.0))), "burst_ms_per_call": burst(lambda: ops.scale_(one, 1.0))}
        for t, nx, ny, c in RAW_SHAPES:
            rs = np.random.RandomState(c)
            a = (rs.standard_normal((c, 2 * c)) + 1j * rs.standard_normal((c, 2 * c))) / np.sqrt(4 * c)
            low = N.noise_cholesky(torch.from_numpy(a @ a.conj().T + 0.25 * np.eye(c)))
            raw = torch.empty((t, nx, ny, c, 2), dtype=torch.float32, device=dev).normal_()
            planar = torch.empty((t, c, nx, ny, 2), dtype=torch.float32, device=dev).normal_()
            moved = 2 * raw.numel() * 4
            row = {"raw_shape": [t, nx, ny, c], "elements": raw.numel() // 2, "bytes": raw.numel() * 4}
            for key, chol in (("coloured", low), ("white", None)):
                row[f"noise_add_raw_{key}"], row[f"noise_add_{key}"] = timed_pair(
                    lambda: N.add_noise_raw(raw, chol, scale=0.01, seed=1, replica=2, out=raw),
                    lambda: N.add_noise(planar, None, chol, scale=0.01, seed=1, replica=2, out=planar), moved)
                for stat in ("median_ms", "burst_ms_per_call"):
                    row[f"raw_over_planar_{key}_{stat}"] = row[f"noise_add_raw_{key}"][stat] / row[f"noise_add_{key}"][stat]
            row["within_margin"] = bool(max(row["raw_over_planar_coloured_median_ms"], row["raw_over_planar_white_median_ms"]) <= doc["margin"])
            lc = torch.view_as_complex(N._chol_pairs(low, c, dev)).tril()
            rc = torch.view_as_complex(raw)

            def composed():
                z = torch.view_as_complex(torch.randn(t, nx, ny, c, 2, device=dev)) * (0.5 ** 0.5)
                return rc + torch.einsum("ij,txyj->txyi", lc, z) * 0.01
            ms = measure(composed)
            row["composed_torch"] = {"median_ms": median(ms), "ms": ms}
            row["composed_over_noise_add_raw"] = row["composed_torch"]["median_ms"] / row["noise_add_raw_coloured"]["median_ms"]
            doc["kernels"].append(row)
            print(json.dumps({"kernel": row}), flush=True)
            del raw, planar, rc
        # replicas of one raw scan through the pipeline: the same submissions with and without noise=
        t, nx, ny, c = RAW_SCAN
        rs = np.random.RandomState(1)
        raw = torch.from_numpy((1e-6 * rs.standard_normal(RAW_SCAN + (2,))).astype(np.float32)).to(dev)
        a = (rs.standard_normal((c, 2 * c)) + 1j * rs.standard_normal((c, 2 * c))) / np.sqrt(4 * c)
        low = N.noise_cholesky(torch.from_numpy(a @ a.conj().T + 0.25 * np.eye(c)))
        mask = torch.zeros(1, t, 1, RAW_CROP[0], 1, 1, dtype=torch.uint8)
        for f in range(t):
            mask[0, f, 0, f % 4::4] = 1
        mask[:, :, :, RAW_CROP[0] // 2 - 8:RAW_CROP[0] // 2 + 8] = 1
        mask = mask.to(dev)
        model = M.VarNet(6, 8, 3, 16, 3, "XF").eval()
        synth.fill_parameters_(model, 1, keep=("lambda",))
        model = model.to(dev)
        kw = dict(crop_shape=RAW_CROP, n_frames=t)
        runs = {"in_flight_noise": [], "in_flight_plain": []}
        with SlicePipeline(model, slots=SLOTS) as pipe:
            pipe.submit_raw(raw, mask, tag="build", **kw)
            list(pipe.drain())
            for _ in range(3):
                for key in runs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for r in range(REPLICAS):
                        pipe.submit_raw(raw, mask, tag=r, noise=N.NoiseSpec(low, 1e-8, 1, r) if key == "in_flight_noise" else None, **kw)
                        for _ in pipe.results():
                            pass
                    list(pipe.drain())
                    torch.cuda.synchronize()
                    runs[key].append(REPLICAS / (time.perf_counter() - t0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            maps = N.pseudo_replica_raw(model, raw, mask, chol=low, scale=1e-8, replicas=REPLICAS, seed=1, pipeline=pipe, **kw)
            torch.cuda.synchronize()
            runs["pseudo_replica_raw_in_flight"] = [REPLICAS / (time.perf_counter() - t0)]
            assert pipe.set_builds == 1
        doc["replicas"] = {"model": "XF-VarNet cfg 2 (6 cascades)", "raw_shape": list(RAW_SCAN), "crop": list(RAW_CROP), "slots": SLOTS,
                           "replicas": REPLICAS, "raw_from": "device", "replicas_per_s": {k: median(v) for k, v in runs.items()}, "runs": runs,
                           "noise_over_plain": median(runs["in_flight_noise"]) / median(runs["in_flight_plain"]),
                           "median_snr": float(maps.snr.median())}
        print(json.dumps({"replicas": doc["replicas"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit to stamp the result with (default: git rev-parse HEAD)")
    ap.add_argument("--raw", action="store_true", help="noise on raw data, in front of the front-end (profiles/noise_raw_rate.json)")
    args = ap.parse_args()
    if args.raw:
        return raw_main(args)
    import numpy as np
    import reconstruction.models as M
    from cine_hip import noise as N, ops, synth
    from cine_hip.pipeline import SlicePipeline
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    ex = synth.make_cine_slice(T, C, H, W, accel=4, seed=0)
    kspace = ex["kspace"].to(dev)
    rs = np.random.RandomState(0)
    a = (rs.standard_normal((C, 2 * C)) + 1j * rs.standard_normal((C, 2 * C))) / np.sqrt(4 * C)
    psi = torch.from_numpy(a @ a.conj().T + 0.25 * np.eye(C))
    low = N.noise_cholesky(psi)
    scale = 0.01 * float(kspace.abs().max())
    commit, csrc = _stamp(args.commit)
    point_bytes = C * 8
    doc = {"shape": [1, T, C, H, W], "masks": "R = 4 rows shifted per frame + 16 centre rows; plane: the first fifth of the readout dropped outside them",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS,
           "commit": commit, "csrc_sha256": csrc, "kspace_bytes": T * H * W * point_bytes}
    with torch.no_grad():
        one = torch.ones(1, device=dev)
        floor = measure(lambda: ops.scale_(one, 1.0))
        doc["event_pair_floor"] = {"what": "cine_scale on one float between two events, the way every single call below is timed",
                                   "median_ms": median(floor), "burst_ms_per_call": burst(lambda: ops.scale_(one, 1.0))}
        print(json.dumps({"event_pair_floor": doc["event_pair_floor"]}), flush=True)
        for name, mask in masks(dev).items():
            points = T * H * W if mask is None else int(mask.sum()) * (W if mask.shape[4] == 1 else 1)
            buf = kspace.clone()
            res = {"sampled_points": points, "sampled_fraction": points / (T * H * W)}
            variants = [("noise_add_coloured", low)] + ([("noise_add_white", None)] if name == "row" else [])
            for key, chol in variants:
                fn = lambda: N.add_noise(buf, mask, chol, scale=scale, seed=1, replica=2, out=buf)   # noqa: E731
                ms = measure(fn)
                moved = 2 * points * point_bytes
                res[key] = {"median_ms": median(ms), "ms": ms, "bytes_moved": moved, "ns_per_kb": 1e6 * median(ms) / (moved / 1e3),
                            "burst_ms_per_call": burst(fn)}
                res[key]["burst_tb_per_s"] = moved / (res[key]["burst_ms_per_call"] * 1e-3) / 1e12
                buf.copy_(kspace)
            if mask is not None:
                out = torch.empty_like(kspace)
                fn = lambda: ops.apply_mask(kspace, mask, out=out)   # noqa: E731
                ms = measure(fn)
                moved = 2 * T * H * W * point_bytes
                res["apply_mask"] = {"median_ms": median(ms), "ms": ms, "bytes_moved": moved, "ns_per_kb": 1e6 * median(ms) / (moved / 1e3),
                                     "burst_ms_per_call": burst(fn)}
                res["apply_mask"]["burst_tb_per_s"] = moved / (res["apply_mask"]["burst_ms_per_call"] * 1e-3) / 1e12
                res["noise_over_apply_mask_per_byte_burst"] = (res["noise_add_coloured"]["burst_ms_per_call"] / res["noise_add_coloured"]["bytes_moved"]) / \
                    (res["apply_mask"]["burst_ms_per_call"] / moved)
                res["noise_over_apply_mask_time"] = res["noise_add_coloured"]["median_ms"] / res["apply_mask"]["median_ms"]
                res["noise_over_apply_mask_per_byte"] = res["noise_add_coloured"]["ns_per_kb"] / res["apply_mask"]["ns_per_kb"]
            lc = torch.view_as_complex(N._chol_pairs(low, C, dev)).tril()
            mf = None if mask is None else mask.to(torch.float32)

            def composed():
                z = torch.view_as_complex(torch.randn(1, T, C, H, W, 2, device=dev)) * (0.5 ** 0.5)
                eta = torch.view_as_real(torch.einsum("ij,btjhw->btihw", lc, z)) * scale
                if mf is not None:
                    eta = eta * mf
                return kspace + eta
            ms = measure(composed)
            res["composed_torch"] = {"median_ms": median(ms), "ms": ms}
            res["composed_over_noise_add"] = res["composed_torch"]["median_ms"] / res["noise_add_coloured"]["median_ms"]
            doc[name] = res
            print(json.dumps({name: res}), flush=True)
        # 64 replicas of the cfg-2 model: in flight with noise=, the same submissions without it, the sequential loop
        mask = masks(dev)["row"]
        mk = ops.apply_mask(kspace, mask)
        model = M.VarNet(6, 8, 3, 16, 3, "XF").eval()
        synth.fill_parameters_(model, 1, keep=("lambda",))
        model = model.to(dev)
        runs = {"in_flight_noise": [], "in_flight_plain": [], "sequential": []}
        with SlicePipeline(model, slots=SLOTS) as pipe:
            pipe.submit(mk, mask, tag="build")
            list(pipe.drain())
            for _ in range(3):
                for key in ("in_flight_noise", "in_flight_plain"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for r in range(REPLICAS):
                        pipe.submit(mk, mask, tag=r, noise=N.NoiseSpec(low, scale, 1, r) if key == "in_flight_noise" else None)
                        for _ in pipe.results():
                            pass
                    list(pipe.drain())
                    torch.cuda.synchronize()
                    runs[key].append(REPLICAS / (time.perf_counter() - t0))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            maps = N.pseudo_replica(model, mk, mask, chol=low, scale=scale, replicas=REPLICAS, seed=1, pipeline=pipe)
            torch.cuda.synchronize()
            runs["pseudo_replica_in_flight"] = [REPLICAS / (time.perf_counter() - t0)]
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seq = N.pseudo_replica(model, mk, mask, chol=low, scale=scale, replicas=REPLICAS, seed=1)
            torch.cuda.synchronize()
            runs["sequential"].append(REPLICAS / (time.perf_counter() - t0))
        doc["replicas"] = {"model": "XF-VarNet cfg 2 (6 cascades)", "slots": SLOTS, "replicas": REPLICAS,
                           "replicas_per_s": {k: median(v) for k, v in runs.items()}, "runs": runs,
                           "in_flight_equals_sequential_bits": bool(all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                                                                        for x, y in zip(maps[:3], seq[:3]))),
                           "median_snr": float(seq.snr.median())}
        print(json.dumps({"replicas": doc["replicas"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
