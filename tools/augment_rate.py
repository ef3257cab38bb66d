#!/usr/bin/env python3
"""What the training augmentation costs on the device, in ONE process.

    python tools/augment_rate.py [--out profiles/augment_rate.json] [--commit SHA] [--maps]

At 15 frames x 15 coils x 200 x 200 complex, a rotation by 10 degrees with scale 1.1 (reflecting border), bilinear and bicubic, hipEvent
medians of 10 single calls each, timed in turn in pairs:
  * cine_affine_warp (``augment.warp`` into a preallocated result) beside a device-to-device copy of the same tensor (``Tensor.copy_``),
    the floor of any out-of-place pass, one read and one write: both find the input in the Infinity Cache;
  * cine_affine_warp beside the composed torch path, the only way without the kernel: permute to (N, C, H, W), ``affine_grid``,
    ``grid_sample``, permute back to the (t, c, h, w, 2) layout -- the kernel then runs behind 400 MB of other traffic, from a cold
    input ("kernel_behind_torch") -- and how far the torch result is from the kernel's;
  * ``augment.augment_example`` (given maps, a row mask) beside the same chain without the warp (k-space of the images, mask, target);
  * the peak device memory either allocates above what was held before the call.
--maps adds the kernel alone under seven maps from the identity to a quarter turn, both modes and borders.
--out writes the document, stamped with the commit and a sha256 over csrc/."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-cine-cardiac-mri_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

T, C, H, W = 15, 15, 200, 200
CROP_TARGET = (180, 180)
STEPS = 10


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed_in_turn(fns):
    """{name: stats} of the calls, timed in turn so that a drift of the machine's load falls on all of them."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(STEPS):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    return {k: {"median_us": 1e3 * median(v), "min_us": 1e3 * min(v), "max_us": 1e3 * max(v)} for k, v in ms.items()}


def peak_above(fn):
    """Peak bytes allocated during fn() above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def torch_path(x, theta, mode):
    """(t, c, h, w, 2) -> the same through grid_sample: the pairs become channels, and back."""
    t, c, h, w, _ = x.shape
    n = x.permute(0, 1, 4, 2, 3).reshape(1, t * c * 2, h, w)
    grid = torch.nn.functional.affine_grid(theta, (1, t * c * 2, h, w), align_corners=False)
    y = torch.nn.functional.grid_sample(n, grid, mode=mode, padding_mode="reflection", align_corners=False)
    return y.reshape(t, c, 2, h, w).permute(0, 1, 3, 4, 2).contiguous()


MAPS = {"identity": {}, "shift_half_pixel": dict(translate=(0.5, 0.5)), "scale_1.1": dict(scale=(1.1, 1.1)), "rot_2": dict(rotation_deg=2.0),
        "rot_10_scale_1.1": dict(rotation_deg=10.0, scale=(1.1, 1.1)), "rot_45": dict(rotation_deg=45.0), "rot_90": dict(rotation_deg=90.0)}


def by_map_rows(x, out, cp):
    """The kernel alone per map, each call behind a device copy of the input (so the input is read from the Infinity Cache): how the
    time grows with the number of cache lines a wave's loads touch (a row of 32 lanes reads along x for the identity, along y for a
    quarter turn)."""
    from cine_hip import augment as A
    rows = []
    for mode in ("bilinear", "bicubic"):
        for border in ("reflect", "zeros"):
            for name, kw in MAPS.items():
                aug = A.Augmentation.from_params(H, W, mode=mode, border=border, **kw)
                for _ in range(3):
                    A.warp(x, aug, out=out)
                torch.cuda.synchronize()
                ms = []
                for _ in range(STEPS):
                    ms.append(event_ms(lambda: A.warp(x, aug, out=out)))
                    cp.copy_(x)
                rows.append({"mode": mode, "border": border, "map": name, "median_us": 1e3 * median(ms), "min_us": 1e3 * min(ms), "max_us": 1e3 * max(ms)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--maps", action="store_true", help="also the kernel alone under maps whose footprints differ (identity .. a quarter turn)")
    args = ap.parse_args()
    from pipeline_rate import _stamp
    from cine_hip import augment as A, frontend as FE, ops
    dev = torch.device("cuda:0")
    commit, csrc = _stamp(args.commit)
    doc = {"what": "cine_affine_warp beside a device copy and the composed torch path; augment_example beside the chain without the warp",
           "device": torch.cuda.get_device_name(dev), "shape": [T, C, H, W], "transform": "rotation 10 degrees, scale 1.1, reflecting border",
           "steps": STEPS, "statistic": "hipEvent median of single calls, timed in turn", "commit": commit, "csrc_sha256": csrc}
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn((T, C, H, W, 2), generator=g).to(dev)
    nbytes = x.numel() * 4
    out = torch.empty_like(x)
    cp = torch.empty_like(x)
    rows = []
    for mode in ("bilinear", "bicubic"):
        aug = A.Augmentation.from_params(H, W, rotation_deg=10.0, scale=(1.1, 1.1), mode=mode, border="reflect")
        (ayy, ayx, by), (axy, axx, bx) = aug.matrix
        theta = torch.tensor([[[axx, axy * H / W, 2 * bx / W], [ayx * W / H, ayy, 2 * by / H]]], dtype=torch.float32, device=dev)
        # Two pairs, each timed in turn, because what ran before decides where the 72 MB input is read from: beside the copy (216 MB
        # live in all) it stays in the Infinity Cache for both; the torch path moves over 400 MB and leaves the kernel a cold input.
        st = timed_in_turn({"kernel": lambda: A.warp(x, aug, out=out), "copy": lambda: cp.copy_(x)})
        st2 = timed_in_turn({"kernel_behind_torch": lambda: A.warp(x, aug, out=out), "torch": lambda: torch_path(x, theta, mode)})
        st.update(st2)
        diff = float((A.warp(x, aug) - torch_path(x, theta, mode)).abs().max())
        st["kernel_over_torch_cold"] = st["kernel_behind_torch"]["median_us"] / st["torch"]["median_us"]
        row = {"mode": mode, "bytes_in": nbytes, "bytes_out": nbytes, **st,
               "kernel_TBps": 2 * nbytes / st["kernel"]["median_us"] / 1e6, "copy_TBps": 2 * nbytes / st["copy"]["median_us"] / 1e6,
               "kernel_over_copy": st["kernel"]["median_us"] / st["copy"]["median_us"],
               "kernel_over_torch": st["kernel"]["median_us"] / st["torch"]["median_us"],
               "max_abs_diff_to_torch_float32": diff,
               "peak_bytes_kernel": peak_above(lambda: A.warp(x, aug)), "peak_bytes_torch": peak_above(lambda: torch_path(x, theta, mode))}
        row["kernel_beats_torch"] = bool(row["kernel_over_torch_cold"] < 1.0)
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc["warp"] = rows
    # the example chain: given maps of unit RSS, a row mask (R = 4 plus 16 centre lines)
    s = torch.randn((C, H, W, 2), generator=g)
    sens = (s / s.square().sum(dim=(0, 3), keepdim=True).sqrt()).to(dev)
    m = np.zeros((T, 1, H, 1, 1), dtype=np.uint8)
    for f in range(T):
        m[f, 0, f % 4::4] = 1
    m[:, :, H // 2 - 8:H // 2 + 8] = 1
    mask = torch.from_numpy(m).to(dev)

    def plain():
        k = ops.apply_mask(FE._to_kspace_hip(x), mask)
        return k, FE.combine_target(x, sens, CROP_TARGET)

    rows = []
    for mode in ("bilinear", "bicubic"):
        aug = A.Augmentation.from_params(H, W, rotation_deg=10.0, scale=(1.1, 1.1), t_shift=3, mode=mode, border="reflect")
        st = timed_in_turn({"augment_example": lambda: A.augment_example(x, aug, mask, sens, CROP_TARGET), "without_warp": plain})
        row = {"mode": mode, **st, "augmented_over_plain": st["augment_example"]["median_us"] / st["without_warp"]["median_us"],
               "peak_bytes_augment_example": peak_above(lambda: A.augment_example(x, aug, mask, sens, CROP_TARGET)),
               "peak_bytes_without_warp": peak_above(plain)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc["example"] = rows
    if args.maps:
        doc["by_map"] = by_map_rows(x, out, cp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({k: v for k, v in doc.items() if k not in ("warp", "example")}), flush=True)


if __name__ == "__main__":
    main()
