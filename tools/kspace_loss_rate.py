#!/usr/bin/env python3
"""What the self-supervised k-space loss costs at 1 x 15 frames x 15 coils x 200 x 200, fused against composed, in ONE process.

    python tools/kspace_loss_rate.py [--out profiles/kspace_loss_rate.json] [--commit SHA]

Mask: R = 4 rows (shifted per frame, plus 16 centre rows), split by ``cine_hip.selfsup.split_mask`` with rho = 0.4; the loss runs on Lambda.
Timed: forward + backward (gradient to the image) of
  * fused    : ``cine_hip.selfsup.kspace_loss`` (cine_kspace_loss + cine_kspace_loss_grad);
  * composed : what was available before it -- ``SensExpandFn``, ``* mask``, the four torch norms and their autograd.
hipEvent medians of 10 steps each, both in this process, and the peak memory of each: ``torch.cuda.max_memory_allocated`` over the warm-up
and the timed steps, above what was allocated before the variant's first step (its cached buffers dropped first) -- so the fused operator's
workspace, which the binding keeps per stream, counts in full.  One stream: the figures do not depend on the number of hardware queues.
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
STEPS = 10


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def measure(step, dev):
    """(hipEvent times of STEPS steps in ms, peak bytes above the bytes allocated before the first step -- warm-up included, so buffers the
    variant creates once and keeps are counted --, the bytes it still holds afterwards, the loss)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(STEPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); loss = step(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    return ms, torch.cuda.max_memory_allocated(dev) - base, torch.cuda.memory_allocated(dev) - base, float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit to stamp the result with (default: git rev-parse HEAD)")
    args = ap.parse_args()
    from cine_hip import autograd as ag, ops, synth
    from cine_hip._lib import lib
    from cine_hip.selfsup import kspace_loss, split_mask
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    ex = synth.make_cine_slice(T, C, H, W, accel=4, seed=0)
    kspace, sens = ex["kspace"].to(dev), ex["sens_maps"].to(dev)
    omega = torch.zeros(1, T, 1, H, 1, 1, dtype=torch.uint8)
    for f in range(T):
        omega[0, f, 0, f % 4::4] = 1
    omega[:, :, :, H // 2 - 8:H // 2 + 8] = 1
    theta, lam = split_mask(omega, rho=0.4, rng=np.random.default_rng(0))
    lam = ops.as_mask_u8(lam.to(dev), kspace)
    y = ops.apply_mask(kspace, ops.as_mask_u8(omega.to(dev), kspace))
    with torch.no_grad():
        image = ops.sens_reduce(ops.apply_mask(kspace, ops.as_mask_u8(theta.to(dev), kspace)), sens)
    image = image.detach().requires_grad_(True)
    lam_f = lam.to(torch.float32)

    def fused():
        image.grad = None
        with torch.enable_grad():
            loss = kspace_loss(image, sens, y, lam)
            loss.backward()
        return loss

    def composed():
        image.grad = None
        with torch.enable_grad():
            u = ag.SensExpandFn.apply(image, sens, None)
            r, v = (u - y) * lam_f, y * lam_f
            loss = 0.5 * torch.linalg.vector_norm(r) / torch.linalg.vector_norm(v) + 0.5 * torch.linalg.vector_norm(r, 1) / torch.linalg.vector_norm(v, 1)
            loss.backward()
        return loss
    lib().cine_diag_counter(ops.D_KSPACE_LOSS, 1)
    fused(); gf = image.grad.clone()
    assert lib().cine_diag_counter(ops.D_KSPACE_LOSS, 1) == 2
    composed(); gc = image.grad.clone()
    commit, csrc = _stamp(args.commit)
    doc = {"shape": [1, T, C, H, W], "mask": "R = 4 rows (+ 16 centre rows), split_mask rho = 0.4", "lambda_fraction": float(lam_f.mean()),
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS,
           "commit": commit, "csrc_sha256": csrc, "kspace_bytes": kspace.numel() * 4, "fused_workspace_bytes": int(lib().cine_kspace_loss_ws_bytes(1, T, C, H, W)),
           "image_gradient_fused_vs_composed_max_abs_over_peak": float((gf - gc).abs().max() / gc.abs().max())}
    for name, fn in (("fused", fused), ("composed", composed), ("fused_again", fused), ("composed_again", composed)):
        ops.release_general_workspaces()
        image.grad = None
        torch.cuda.empty_cache()
        ms, peak, held, loss = measure(fn, dev)
        doc[name] = {"median_ms": median(ms), "ms": ms, "peak_bytes": peak, "held_bytes": held, "loss": loss}
        print(json.dumps({name: doc[name]}), flush=True)
    doc["composed_over_fused"] = doc["composed"]["median_ms"] / doc["fused"]["median_ms"]
    doc["peak_fused_over_composed"] = doc["fused"]["peak_bytes"] / doc["composed"]["peak_bytes"]
    print(json.dumps({k: doc[k] for k in ("composed_over_fused", "peak_fused_over_composed", "image_gradient_fused_vs_composed_max_abs_over_peak")}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
