#!/usr/bin/env python3
"""Cine slices/s through the public SlicePipeline (cine_hip.pipeline), printed as one JSON line.

    python tools/pipeline_rate.py [--config {2,3,4,5}] [--slots 10] [--slices 300] [--warmup 20]

The model and the synthetic slices are bench.py's (CONFIGS, make_slices): `slots` different slices, submitted round-robin.
Three input forms -- k-space resident in HBM, pinned host tensors, pageable numpy arrays (complex64) -- each with the
outputs returned as device tensors and as pinned host tensors (out="host").  One pipeline per output form (captured
once); every region submits `slices` slices, takes the finished ones as it goes (results()), drains, and is timed from
the first submit to the last result.  Compare `value_device_in` with bench.py's `value` and `value_pinned_in` with
its `value_with_h2d` (run bench.py --full beside it).  `host_copy_GBps` is the host memcpy rate of one slice's
k-space from a numpy array into a pinned buffer (what a pageable input costs inside submit).

    python tools/pipeline_rate.py --raw [--slots 10] [--slices 40] [--warmup 8] [--repeats 3] [--out profiles/raw_pipeline_rate.json]

RAW k-space in, reconstruction out (``SlicePipeline.submit_raw``), config 2's model, three scans: 25 x 384 x 144 x 15 (the FFT line
engines; crop 200 x 144), 25 x 416 x 208 x 30 (the windowed transform; crop 200 x 200) and the latter compressed 30 -> 15 coils with a
given matrix.  Per scan, slices/s (median of --repeats regions, warm-up outside the clock) for pinned, numpy and device-resident
raw, and beside them "today's way" in the same process: ``torch.as_tensor(raw).cuda()`` -> ``prepare_slice`` -> ``ops.apply_mask`` ->
``submit``.  ``h2d_*``: the bytes one slice moves to the device and the rate that copy ALONE allows (pinned -> HBM on one stream,
nothing else running); ``bound``: which of the two, that copy or the GPU (the device-resident rate), is the lower and so limits a
pinned input, and ``pinned_over_limit`` how close the pinned rate comes to it.  Also the ingest kernel alone (hipEvent median) as a
fraction of the device's copy rate measured in the same run.  Without --raw the output is unchanged.

    python tools/pipeline_rate.py --raw --virtual-coils 15 [--hw-queues 16] [--out profiles/virtual_coils_inflight_rate.json]

Per-slice coil compression, 30 -> V coils, on 15 x 384 x 144 x 30 and 15 x 416 x 208 x 30 (pinned raw data with a designed coil
spectrum, every slice its own): ``submit_raw(..., virtual_coils=V)`` ("in flight"), beside it today's way -- per slice a copy to the
device, ``frontend.coil_compression_matrix`` (torch.linalg.eigh behind a host check), ``submit_raw(..., coil_matrix=A)`` -- and, as the
ceiling, ``coil_matrix=`` with one matrix per scan computed beforehand.  Medians of --repeats regions, warm-up outside the clock; the
spread of a line is max - min of its regions.  Also cine_coil_matrix alone (hipEvent, median of 20) at 15, 30 and 64 coils, and the
Jacobi sweeps every slice took.

    python tools/pipeline_rate.py --raw --virtual-coils 15 --whiten [--out profiles/noise_whitening_rate.json]

Noise pre-whitening folded into the per-slice matrix, in ONE session: ``submit_raw(pinned, virtual_coils=V)`` with and without
``whitener=W`` (W from ``frontend.noise_whitener`` on a synthetic noise scan with a designed covariance of condition number 100) on the
two scans above, interleaved region by region, medians of --repeats regions; and cine_coil_matrix_whitened beside cine_coil_matrix alone
(hipEvent, median of 20) at 15, 30 and 64 coils.  What to hold the result against: the whitened kernel adds three c^3 float64 products
to a Jacobi solve of 8-11 sweeps, and the pass over the data is unchanged."""
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
if "--hw-queues" in sys.argv[1:-1]:                     # an explicit count (at most 32) overrides the environment's
    os.environ["GPU_MAX_HW_QUEUES"] = str(min(32, int(sys.argv[sys.argv.index("--hw-queues") + 1])))

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


RAW_SCANS = (("line_384x144x15", (25, 384, 144, 15), None), ("window_416x208x30", (25, 416, 208, 30), None),
             ("window_416x208x30_to_15", (25, 416, 208, 30), 15))
FRAMES, FILTER, SCALING = 15, (0.7, 0.0, 0.3, 0.3), 1e6


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def _event_ms(fn, reps, warmup=3):
    """hipEvent times of `reps` calls of fn on the current stream, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def _stamp(commit):
    """(commit, sha256 over the sources under csrc/): which code the numbers belong to."""
    import hashlib
    import subprocess
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
        except Exception:
            commit = None
    csrc = os.path.join(ROOT, "deep-cine-cardiac-mri_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(csrc)):
        path = os.path.join(csrc, name)
        if os.path.isfile(path):
            h.update(name.encode()); h.update(open(path, "rb").read())
    return commit, h.hexdigest()


def raw_main(args):
    import bench
    from cine_hip import frontend as FE, ops, synth
    from cine_hip.pipeline import SlicePipeline
    cfg = bench.CONFIGS[2]()
    dev = torch.device("cuda:0")
    S, n, warm, reps = args.slots, args.slices or 40, args.warmup if args.warmup is not None else 8, args.repeats
    net = cfg["hip"]().eval()
    synth.fill_parameters_(net, cfg["wseed"], keep=cfg["keep"])
    net = net.to(dev)
    commit, csrc = _stamp(args.commit)
    want_forms = set(args.forms.split(","))
    doc = {"metric": "cine slices/sec from raw k-space through SlicePipeline.submit_raw", "config": 2, "name": cfg["name"], "slots": S,
           "slices_per_region": n, "warmup_slices": warm, "regions": reps, "statistic": "median of the regions",
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "device": torch.cuda.get_device_name(dev), "commit": commit,
           "csrc_sha256": csrc, "torch_threads": torch.get_num_threads(), "scans": []}

    # the device's copy rate (read + write bytes of a 1 GiB device-to-device copy), then the ingest kernel against it
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    copy_ms = _median(_event_ms(lambda: dst.copy_(src), 10))
    doc["device_copy_TBps"] = 2 * src.numel() * 4 / copy_ms / 1e9
    del src, dst
    doc["ingest_kernel"] = []
    for shape in ((15, 384, 144, 15), (15, 200, 200, 30)):
        x = torch.empty(shape + (2,), dtype=torch.float32, device=dev).normal_()
        out = torch.empty((shape[0], shape[3], shape[1], shape[2], 2), dtype=torch.float32, device=dev)
        ms = _event_ms(lambda: ops.raw_ingest(x, shape[0], SCALING, out=out), 20)
        tbps = 2 * x.numel() * 4 / _median(ms) / 1e9
        doc["ingest_kernel"].append({"shape": list(shape), "median_ms": _median(ms), "min_ms": min(ms), "launches": len(ms), "TBps": tbps,
                                     "frac_of_device_copy_rate": tbps / doc["device_copy_TBps"]})
        del x, out

    n_raws = 4                                                   # distinct scans cycled through (519 MB each on the host at 416 x 208 x 30)
    for name, shape, V in RAW_SCANS:
        t, nx, ny, c = shape
        crop = (min(200, nx), min(200, ny))
        rng = np.random.default_rng(nx + c)
        raws = [(1e-6 * rng.standard_normal(shape + (2,), dtype=np.float32)).view(np.complex64)[..., 0] for _ in range(n_raws)]
        masks = []
        for j in range(n_raws):
            m = (rng.uniform(size=(1, FRAMES, 1, crop[0], 1, 1)) < 0.25).astype(np.uint8)
            m[:, :, :, crop[0] // 2 - 8 - j:crop[0] // 2 + 8 + j] = 1
            masks.append(torch.from_numpy(m))
        mats = [FE.coil_compression_matrix(torch.from_numpy(r[:FRAMES]).to(dev), V, FRAMES)[0] for r in raws] if V else [None] * n_raws
        kw = dict(crop_shape=crop, n_frames=FRAMES, filter_size=FILTER, scaling=SCALING)
        kept = [torch.from_numpy(r[:FRAMES]) for r in raws]
        forms = {"pinned": [k.pin_memory() for k in kept], "numpy": raws, "device": [k.to(dev) for k in kept]}
        dmasks = [m.to(dev) for m in masks]
        row = {"scan": name, "raw_shape": list(shape), "crop": list(crop), "frames": FRAMES, "virtual_coils": V,
               "h2d_bytes_per_slice": kept[0].numel() * 8, "h2d_bytes_per_slice_todays_way": raws[0].size * 8}

        # the copy alone: the kept frames, pinned -> HBM, one stream, nothing else running
        buf = [torch.empty_like(forms["device"][0]) for _ in range(2)]
        cs = torch.cuda.Stream()
        rates = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(cs):
                for k in range(12):
                    buf[k & 1].copy_(forms["pinned"][k % n_raws], non_blocking=True)
            torch.cuda.synchronize()
            rates.append(12 / (time.perf_counter() - t0))
        del buf
        row["h2d_alone_slices_per_s"] = _median(rates[1:])
        row["h2d_alone_GBps"] = row["h2d_alone_slices_per_s"] * row["h2d_bytes_per_slice"] / 1e9

        def run_raw(pipe, inputs, count):
            got = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(count):
                j = k % n_raws
                pipe.submit_raw(inputs[j], dmasks[j], coil_matrix=mats[j], **kw)
                for _ in pipe.results():
                    got += 1
            for _ in pipe.drain():
                got += 1
            torch.cuda.synchronize()
            assert got == count
            return count / (time.perf_counter() - t0)

        def run_today(pipe, count):
            got = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(count):
                j = k % n_raws
                y = torch.as_tensor(raws[j]).cuda()
                ksp, _ = FE.prepare_slice(y, crop, FRAMES, FILTER, SCALING, coil_matrix=mats[j])
                pipe.submit(ops.apply_mask(ksp, dmasks[j])[None], dmasks[j])
                for _ in pipe.results():
                    got += 1
            for _ in pipe.drain():
                got += 1
            torch.cuda.synchronize()
            assert got == count
            return count / (time.perf_counter() - t0)

        with torch.no_grad():
            want = net(FE.prepare_masked_slice(forms["device"][0], dmasks[0], crop, FRAMES, FILTER, SCALING, coil_matrix=mats[0]), dmasks[0]).cpu()
        with SlicePipeline(net, slots=S) as pipe:
            t_build = time.perf_counter()
            pipe.submit_raw(forms["device"][0], dmasks[0], coil_matrix=mats[0], **kw)
            (_, o0), = list(pipe.drain())
            row["setup_s"] = time.perf_counter() - t_build
            row["bit_identical_to_sequential"] = bool(torch.equal(o0.cpu(), want))
            for form, inputs in forms.items():
                if form not in want_forms:
                    continue
                run_raw(pipe, inputs, warm)
                rs = [run_raw(pipe, inputs, n) for _ in range(reps)]
                row[f"value_{form}_raw"], row[f"regions_{form}_raw"] = _median(rs), rs
            assert pipe.set_builds == 1
        if "today" in want_forms:
            with SlicePipeline(net, slots=S) as pipe:
                run_today(pipe, warm)
                rs = [run_today(pipe, n) for _ in range(reps)]
                row["value_todays_way"], row["regions_todays_way"] = _median(rs), rs
        if "device" in want_forms and "pinned" in want_forms:
            limit = min(row["h2d_alone_slices_per_s"], row["value_device_raw"])
            row["bound"] = "host-to-device copy" if row["h2d_alone_slices_per_s"] < row["value_device_raw"] else "GPU"
            row["limit_slices_per_s"] = limit
            row["pinned_over_limit"] = row["value_pinned_raw"] / limit
        if "today" in want_forms and "pinned" in want_forms:
            row["pinned_over_todays_way"] = row["value_pinned_raw"] / row["value_todays_way"]
        doc["scans"].append(row)
        print(json.dumps(row), flush=True)
        del forms, kept, raws, dmasks, mats
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "scans"}), flush=True)


def _designed(shape, seed, dev):
    """Complex64 (t, x, y, coil) on the host at the amplitude of a k-space: white samples scaled per coil by sigma_i^2 =
    1e-4^(i / (c - 1)) and mixed by a seeded random unitary matrix (the designed input of tests/test_coil_compress.py)."""
    c = shape[3]
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c)))
    sigma = np.sqrt(1e-4 ** (np.arange(c) / max(c - 1, 1)))
    g = torch.Generator(device=dev).manual_seed(seed)
    w = torch.view_as_complex(torch.randn(shape + (2,), generator=g, device=dev, dtype=torch.float32))
    mix = torch.from_numpy((sigma[:, None] * q.T).astype(np.complex64)).to(dev)
    return (1e-6 * (w @ mix)).cpu()


def virtual_coils_main(args):
    import bench
    from cine_hip import frontend as FE, synth
    from cine_hip.pipeline import SlicePipeline
    cfg = bench.CONFIGS[2]()
    dev = torch.device("cuda:0")
    V, S, n, warm, reps = args.virtual_coils, args.slots, args.slices or 40, args.warmup if args.warmup is not None else 8, args.repeats
    net = cfg["hip"]().eval()
    synth.fill_parameters_(net, cfg["wseed"], keep=cfg["keep"])
    net = net.to(dev)
    commit, csrc = _stamp(args.commit)
    doc = {"metric": "cine slices/sec from raw k-space with per-slice coil compression (SlicePipeline.submit_raw)", "config": 2,
           "name": cfg["name"], "virtual_coils": V, "cc_region": 24, "slots": S, "slices_per_region": n, "warmup_slices": warm,
           "regions": reps, "statistic": "median of the regions; spread = max - min of the regions",
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "device": torch.cuda.get_device_name(dev), "commit": commit,
           "csrc_sha256": csrc, "lines": {"in_flight": "submit_raw(pinned, virtual_coils=V)",
                                          "todays_way": "per slice: pinned.cuda(), coil_compression_matrix (eigh), submit_raw(device, coil_matrix=A)",
                                          "ceiling": "submit_raw(pinned, coil_matrix=A), one matrix per scan computed beforehand"},
           "coil_matrix_kernel": [], "scans": []}

    for c in (15, 30, 64):                                       # the kernel alone, on the Gram matrix of a designed input
        g = FE.coil_gram(_designed((2, 24, 24, c), 9, dev).to(dev), 2, 24)[None].contiguous()
        v = min(V, c)
        outs = FE._coil_matrix_jacobi(g, v)
        ms = _event_ms(lambda: FE._coil_matrix_jacobi(g, v, *outs), 20)
        info = outs[2][0].tolist()
        doc["coil_matrix_kernel"].append({"coils": c, "virtual_coils": v, "median_ms": _median(ms), "min_ms": min(ms), "launches": len(ms),
                                          "sweeps": int(info[1]), "residual": info[0]})
    print(json.dumps(doc["coil_matrix_kernel"]), flush=True)

    n_raws = 4
    for name, shape in (("line_384x144x30", (FRAMES, 384, 144, 30)), ("window_416x208x30", (FRAMES, 416, 208, 30))):
        t, nx, ny, c = shape
        crop = (min(200, nx), min(200, ny))
        rng = np.random.default_rng(nx + c)
        pinned = [_designed(shape, 100 + nx + j, dev).pin_memory() for j in range(n_raws)]
        dmasks = []
        for j in range(n_raws):
            m = (rng.uniform(size=(1, FRAMES, 1, crop[0], 1, 1)) < 0.25).astype(np.uint8)
            m[:, :, :, crop[0] // 2 - 8 - j:crop[0] // 2 + 8 + j] = 1
            dmasks.append(torch.from_numpy(m).to(dev))
        scan_matrix = FE.coil_compression_matrix(pinned[0].to(dev), V, FRAMES)[0]
        kw = dict(crop_shape=crop, n_frames=FRAMES, filter_size=FILTER, scaling=SCALING)
        row = {"scan": name, "raw_shape": list(shape), "crop": list(crop), "frames": FRAMES, "h2d_bytes_per_slice": pinned[0].numel() * 8}

        def submit(line, pipe, j):
            if line == "in_flight":
                pipe.submit_raw(pinned[j], dmasks[j], virtual_coils=V, **kw)
            elif line == "ceiling":
                pipe.submit_raw(pinned[j], dmasks[j], coil_matrix=scan_matrix, **kw)
            else:
                y = pinned[j].cuda()
                a, _ = FE.coil_compression_matrix(y, V, FRAMES)
                pipe.submit_raw(y, dmasks[j], coil_matrix=a, **kw)

        def run(line, pipe, count):
            got = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(count):
                submit(line, pipe, k % n_raws)
                for _ in pipe.results():
                    got += 1
            for _ in pipe.drain():
                got += 1
            torch.cuda.synchronize()
            assert got == count
            return count / (time.perf_counter() - t0)

        with torch.no_grad():
            a0 = FE.coil_matrix_from_gram(FE.coil_gram(pinned[0].to(dev), FRAMES, 24), V, method="jacobi")[0]
            want = net(FE.prepare_masked_slice(pinned[0].to(dev), dmasks[0], crop, FRAMES, FILTER, SCALING, coil_matrix=a0), dmasks[0]).cpu()
        for line in ("in_flight", "todays_way", "ceiling"):
            with SlicePipeline(net, slots=S) as pipe:
                if line == "in_flight":
                    pipe.submit_raw(pinned[0], dmasks[0], virtual_coils=V, **kw)
                    (_, o0), = list(pipe.drain())
                    row["bit_identical_to_sequential"] = bool(torch.equal(o0.cpu(), want))
                run(line, pipe, warm)
                rs = [run(line, pipe, n) for _ in range(reps)]
                assert pipe.set_builds == 1
                row[f"value_{line}"], row[f"regions_{line}"], row[f"spread_{line}"] = _median(rs), rs, max(rs) - min(rs)
                if line == "in_flight":
                    recs = list(pipe.last_coil_info.values())
                    row["sweeps_min"], row["sweeps_max"] = min(r.sweeps for r in recs), max(r.sweeps for r in recs)
                    row["kept_share_min"], row["residual_max"] = min(r.kept for r in recs), max(r.residual for r in recs)
        row["in_flight_over_todays_way"] = row["value_in_flight"] / row["value_todays_way"]
        row["in_flight_over_ceiling"] = row["value_in_flight"] / row["value_ceiling"]
        row["in_flight_not_below_todays_way_by_more_than_the_spread"] = bool(
            row["value_in_flight"] >= row["value_todays_way"] - max(row["spread_in_flight"], row["spread_todays_way"]))
        doc["scans"].append(row)
        print(json.dumps(row), flush=True)
        del pinned, dmasks
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "scans"}), flush=True)


def _noise_scan(c, seed, dev, n=16384):
    """Noise samples (n, c) complex64 on the device with the covariance Q diag(1e-12 100^(-k / (c - 1))) Q^H: unequal, correlated channels at
    the amplitude of the raw data above."""
    rs = np.random.RandomState(1000 + seed)
    q, _ = np.linalg.qr(rs.standard_normal((c, c)) + 1j * rs.standard_normal((c, c)))
    d = 1e-12 * 100.0 ** (-np.arange(c) / max(c - 1, 1))
    low = np.linalg.cholesky((q * d) @ q.conj().T)
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.view_as_complex(torch.randn((n, c, 2), generator=g, device=dev, dtype=torch.float32)) * (0.5 ** 0.5)
    return z @ torch.from_numpy(low.T.astype(np.complex64)).to(dev)


def whitened_main(args):
    import bench
    from cine_hip import frontend as FE, synth
    from cine_hip.pipeline import SlicePipeline
    cfg = bench.CONFIGS[2]()
    dev = torch.device("cuda:0")
    V, S, n, warm, reps = args.virtual_coils, args.slots, args.slices or 40, args.warmup if args.warmup is not None else 8, args.repeats
    net = cfg["hip"]().eval()
    synth.fill_parameters_(net, cfg["wseed"], keep=cfg["keep"])
    net = net.to(dev)
    commit, csrc = _stamp(args.commit)
    doc = {"metric": "cine slices/sec from raw k-space with per-slice coil compression, with and without noise pre-whitening "
                     "(SlicePipeline.submit_raw)", "config": 2, "name": cfg["name"], "virtual_coils": V, "cc_region": 24, "slots": S,
           "slices_per_region": n, "warmup_slices": warm, "regions": reps,
           "statistic": "median of the regions, the two lines interleaved region by region; spread = max - min of the regions",
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "device": torch.cuda.get_device_name(dev), "commit": commit,
           "csrc_sha256": csrc, "lines": {"plain": "submit_raw(pinned, virtual_coils=V)",
                                          "whitened": "submit_raw(pinned, virtual_coils=V, whitener=W), W on the device"},
           "coil_matrix_kernel": [], "scans": []}

    for c in (15, 30, 64):                                       # the two kernels alone, on the Gram matrix of a designed input
        g = FE.coil_gram(_designed((2, 24, 24, c), 9, dev).to(dev), 2, 24)[None].contiguous()
        w = FE.noise_whitener(_noise_scan(c, 9, dev))
        v = min(V, c)
        outs, outs_w = FE._coil_matrix_jacobi(g, v), FE._coil_matrix_jacobi(g, v, whitener=w)
        ms = _event_ms(lambda: FE._coil_matrix_jacobi(g, v, *outs), 20)
        ms_w = _event_ms(lambda: FE._coil_matrix_jacobi(g, v, *outs_w, whitener=w), 20)
        info, info_w = outs[2][0].tolist(), outs_w[2][0].tolist()
        doc["coil_matrix_kernel"].append({"coils": c, "virtual_coils": v, "launches": len(ms),
                                          "plain_median_ms": _median(ms), "plain_min_ms": min(ms), "plain_sweeps": int(info[1]),
                                          "whitened_median_ms": _median(ms_w), "whitened_min_ms": min(ms_w), "whitened_sweeps": int(info_w[1]),
                                          "whitened_residual": info_w[0], "whitened_over_plain": _median(ms_w) / _median(ms)})
    print(json.dumps(doc["coil_matrix_kernel"]), flush=True)

    n_raws = 4
    for name, shape in (("line_384x144x30", (FRAMES, 384, 144, 30)), ("window_416x208x30", (FRAMES, 416, 208, 30))):
        t, nx, ny, c = shape
        crop = (min(200, nx), min(200, ny))
        rng = np.random.default_rng(nx + c)
        pinned = [_designed(shape, 100 + nx + j, dev).pin_memory() for j in range(n_raws)]
        dmasks = []
        for j in range(n_raws):
            m = (rng.uniform(size=(1, FRAMES, 1, crop[0], 1, 1)) < 0.25).astype(np.uint8)
            m[:, :, :, crop[0] // 2 - 8 - j:crop[0] // 2 + 8 + j] = 1
            dmasks.append(torch.from_numpy(m).to(dev))
        w = FE.noise_whitener(_noise_scan(c, nx, dev))
        kw = dict(crop_shape=crop, n_frames=FRAMES, filter_size=FILTER, scaling=SCALING)
        row = {"scan": name, "raw_shape": list(shape), "crop": list(crop), "frames": FRAMES, "h2d_bytes_per_slice": pinned[0].numel() * 8}
        extra = {"plain": {}, "whitened": {"whitener": w}}

        def run(line, pipe, count):
            got = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(count):
                pipe.submit_raw(pinned[k % n_raws], dmasks[k % n_raws], virtual_coils=V, **extra[line], **kw)
                for _ in pipe.results():
                    got += 1
            for _ in pipe.drain():
                got += 1
            torch.cuda.synchronize()
            assert got == count
            return count / (time.perf_counter() - t0)

        with torch.no_grad():
            a0 = FE.coil_matrix_from_gram(FE.coil_gram(pinned[0].to(dev), FRAMES, 24), V, method="jacobi", whitener=w)[0]
            want = net(FE.prepare_masked_slice(pinned[0].to(dev), dmasks[0], crop, FRAMES, FILTER, SCALING, coil_matrix=a0), dmasks[0]).cpu()
        pipes = {line: SlicePipeline(net, slots=S) for line in extra}        # one set each, alive side by side
        try:
            pipes["whitened"].submit_raw(pinned[0], dmasks[0], virtual_coils=V, whitener=w, **kw)
            (_, o0), = list(pipes["whitened"].drain())
            row["bit_identical_to_sequential"] = bool(torch.equal(o0.cpu(), want))
            rs = {line: [] for line in extra}
            for line in extra:
                run(line, pipes[line], warm)
            for _ in range(reps):
                for line in extra:
                    rs[line].append(run(line, pipes[line], n))
            for line in extra:
                assert pipes[line].set_builds == 1
                row[f"value_{line}"], row[f"regions_{line}"], row[f"spread_{line}"] = _median(rs[line]), rs[line], max(rs[line]) - min(rs[line])
                recs = list(pipes[line].last_coil_info.values())
                row[f"sweeps_{line}"] = [min(r.sweeps for r in recs), max(r.sweeps for r in recs)]
                row[f"residual_max_{line}"] = max(r.residual for r in recs)
        finally:
            for pipe in pipes.values():
                pipe.close()
        row["whitened_over_plain"] = row["value_whitened"] / row["value_plain"]
        doc["scans"].append(row)
        print(json.dumps(row), flush=True)
        del pinned, dmasks, pipes
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k != "scans"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4, 5))
    ap.add_argument("--slots", type=int, default=10)
    ap.add_argument("--slices", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--hw-queues", type=int, default=None, help="set GPU_MAX_HW_QUEUES to this (<= 32) instead of keeping the environment's")
    ap.add_argument("--raw", action="store_true", help="raw k-space through submit_raw (see the module docstring)")
    ap.add_argument("--forms", default="pinned,numpy,device,today", help="--raw: which of pinned, numpy, device, today to run (a trace of one form)")
    ap.add_argument("--repeats", type=int, default=3, help="--raw: timed regions per input form")
    ap.add_argument("--out", default=None, help="--raw: also write the whole result to this JSON file")
    ap.add_argument("--commit", default=None, help="--raw: the commit to stamp the result with (default: git rev-parse HEAD)")
    ap.add_argument("--virtual-coils", type=int, default=None, help="--raw: per-slice coil compression to this many virtual coils, in flight "
                    "beside today's way and the coil_matrix= ceiling (see the module docstring)")
    ap.add_argument("--whiten", action="store_true", help="--raw --virtual-coils V: the in-flight rate with and without noise pre-whitening "
                    "(whitener=W) in one session, and the two matrix kernels alone (see the module docstring)")
    args = ap.parse_args()
    if args.virtual_coils is not None and not args.raw:
        ap.error("--virtual-coils goes with --raw")
    if args.whiten and args.virtual_coils is None:
        ap.error("--whiten goes with --raw --virtual-coils V")
    if args.raw and args.whiten:
        args.out = args.out or os.path.join(ROOT, "profiles", "noise_whitening_rate.json")
        return whitened_main(args)
    if args.raw:
        return virtual_coils_main(args) if args.virtual_coils is not None else raw_main(args)
    args.slices = 300 if args.slices is None else args.slices
    args.warmup = 20 if args.warmup is None else args.warmup
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
