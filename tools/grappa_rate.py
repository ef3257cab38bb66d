#!/usr/bin/env python3
"""What GRAPPA / TGRAPPA (cine_hip.grappa) costs at 1 x 15 frames x 15 coils x 200 x 200, R = 4, kernel 2 x 5, in ONE process.

    python tools/grappa_rate.py [--out profiles/grappa_rate.json] [--commit SHA]
    python tools/grappa_rate.py --gaps [--out profiles/grappa_gaps_rate.json] [--commit SHA]
    python tools/grappa_rate.py --gfactor [--out profiles/grappa_gfactor_rate.json] [--commit SHA]

Mask: an interleaved lattice of step 4 without ACS lines; TGRAPPA on the central 32 rows of the temporal average; lam = 1e-4.
hipEvent medians of 10 calls each:
  * the four entry points alone (cine_grappa_offsets, cine_grappa_gram, cine_grappa_weights, cine_grappa_apply); for the apply kernel its
    FLOP rate (8 FLOP per complex multiply-add, targets only) and the bytes it has to move (acquired rows read once, targets written once,
    the weights once);
  * the whole ``grappa(...)`` call (check off: nothing read by the host) in turn with a composed torch path: the temporal average, the
    patch matrix by slicing, ``torch.linalg.solve`` in complex128 on the device (on the host where this torch build has no device solver;
    the output says which), the application as ``torch.nn.functional.conv2d`` with dilation (R, 1) on the 2c real channels, one call per
    type over every row of every frame, and a ``torch.where`` scatter of the target rows;
  * peak memory of both above the baseline, and slices per second of ``Grappa`` through ``SlicePipeline`` (graphs, 4 slots, device inputs).
--out writes the document, stamped with the commit and a sha256 over csrc/.

--gaps measures the path for unevenly spaced rows (``accel=None``) instead, same shape, kernel and lam, hipEvent medians of 10:
  (a) on the pure lattice of step 4, ``cine_grappa_apply_gaps`` beside ``cine_grappa_apply`` with the same weights (equal work: the gap
      kernel adds one table read per workgroup and a weight base per gap), and the figure of profiles/grappa_rate.json if it is there;
  (b) on the mask of ``synth.EquispacedMaskFunc([0.08], [4])`` (seed 0; calibrated on its centre block): ``cine_grappa_gaps``, the fit of
      the steps that occur and of the module's default steps (one Gram matrix and one solve per step), ``cine_grappa_apply_gaps`` and the whole ``grappa(accel=None)`` call (check off)
      in turn with a composed torch path -- per step the patch matrix, ``torch.linalg.solve`` and one dilated ``conv2d`` plus
      ``torch.where`` per row type -- with the peak memory of both;
  (c) slices per second of ``Grappa(accel=None)`` through a 4-slot ``SlicePipeline``.

--gfactor measures the analytic noise maps instead, same shape, kernel and lam, hipEvent medians of 10, each with its peak memory:
  ``cine_grappa_gfactor`` per coil and with maps (p = conj(S)), white noise and with a Cholesky factor; ``cine_grappa_image_weights``;
  a composed torch path (the combined kernel zero-padded to c^2 planes of h x w, ``torch.fft.fft2``, ``einsum`` with L and with the
  maps); ``Grappa.noise_maps`` (calibration included); and ``noise.pseudo_replica`` of ``Grappa`` with 64 replicas under the lattice
  mask and under the full one, which is what a measured g-factor map costs."""
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
import torch.nn.functional as F  # noqa: E402

from kt_fista_rate import C, H, SLICES, SLOTS, STEPS, T, W, measure, median  # noqa: E402

R, KY, KX, LAM, CALIB_ROWS = 4, 2, 5, 1e-4, 32


def device_solve_works(dev):
    try:
        a = torch.eye(4, dtype=torch.complex128, device=dev) * 2
        x = torch.linalg.solve(a, torch.ones(4, 2, dtype=torch.complex128, device=dev))
        torch.cuda.synchronize()
        return bool(torch.isfinite(x.real).all())
    except Exception:
        return False


def pipeline_rate(model, mk, mask):
    from cine_hip.pipeline import SlicePipeline
    with SlicePipeline(model, slots=SLOTS) as pipe:
        pipe.submit(mk, mask, tag="build")
        list(pipe.drain())
        rates = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(SLICES):
                pipe.submit(mk, mask, tag=j)
                for _ in pipe.results():
                    pass
            list(pipe.drain())
            torch.cuda.synchronize()
            rates.append(SLICES / (time.perf_counter() - t0))
    return {"slots": SLOTS, "slices": SLICES, "slices_per_s": median(rates), "runs": rates}


def gaps_main(args):
    import numpy as np
    from cine_hip import grappa as G, ops, synth
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    ex = synth.make_cine_slice(T, C, H, W, accel=4, seed=0, noise_std=0.01)
    commit, csrc = _stamp(args.commit)
    solve_on_device = device_solve_works(dev)
    ns, hx = KY * KX * C, KX // 2
    doc = {"shape": [1, T, C, H, W], "kernel": [KY, KX], "lam": LAM, "device": torch.cuda.get_device_name(dev),
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS, "commit": commit, "csrc_sha256": csrc, "ns": ns,
           "composed_solve": "torch.linalg.solve in complex128 on the " + ("device" if solve_on_device else "host")}
    st = ops._stream
    with torch.no_grad():
        full = ex["kspace"].to(dev)

        # ---- (a) equal work on the pure lattice of step 4
        lat = G.lattice_mask(T, H, R).to(dev)
        mk = ops.apply_mask(full, lat)
        off, _ = G.lattice_offsets(lat, R)
        cal = G.calibration_data(mk, lat, "tgrappa", None, CALIB_ROWS)
        weights, _ = G.grappa_weights(cal[0], R, (KY, KX), LAM)
        table, count, unfilled = G.gap_table(lat, (R,))
        assert not bool(unfilled.any())
        out_l, out_g = torch.empty_like(mk), torch.empty_like(mk)
        m2 = lat.view(T, H)
        parts = {
            "cine_grappa_apply": lambda: G.grappa_apply(mk[0], weights, m2, off[0], R, (KY, KX), out=out_l[0]),
            "cine_grappa_apply_gaps": lambda: G.grappa_apply_gaps(mk[0], weights, (R,), m2, table[0], count[0], (KY, KX), out=out_g[0]),
            "cine_grappa_apply_in_place": lambda: G.grappa_apply(out_l[0], weights, m2, off[0], R, (KY, KX), out=out_l[0]),
            "cine_grappa_apply_gaps_in_place": lambda: G.grappa_apply_gaps(out_g[0], weights, (R,), m2, table[0], count[0], (KY, KX), out=out_g[0]),
        }
        us = {}
        for rnd in range(2):                                             # in turn, twice: the second round is what is reported
            for k, fn in parts.items():
                us[k] = median(measure(fn, dev)[0]) * 1e3
        assert torch.equal(out_l, out_g)
        a = {"mask": "interleaved lattice of step 4, no ACS lines", "entry_us": us,
             "gaps_over_lattice": us["cine_grappa_apply_gaps"] / us["cine_grappa_apply"],
             "gaps_over_lattice_in_place": us["cine_grappa_apply_gaps_in_place"] / us["cine_grappa_apply_in_place"]}
        published = os.path.join(ROOT, "profiles", "grappa_rate.json")
        if os.path.exists(published):
            with open(published) as f:
                old = json.load(f)
            a["published_lattice_us"] = {k: old["entry_us"][k] for k in ("cine_grappa_apply", "cine_grappa_apply_in_place")}
            a["published_commit"] = old.get("commit")
            a["gaps_over_published_lattice"] = us["cine_grappa_apply_gaps"] / old["entry_us"]["cine_grappa_apply"]
        doc["lattice"] = a
        print(json.dumps({"lattice": a}), flush=True)

        # ---- (b) the reference's equispaced mask
        row = synth.EquispacedMaskFunc([0.08], [4])((T, 1, H, 1, 2), seed=0).numpy().reshape(H) != 0
        n_low = int(round(H * 0.08))
        acs = ((H - n_low + 1) // 2, (H - n_low + 1) // 2 + n_low)
        mask = torch.from_numpy(np.repeat(row[None], T, 0).astype(np.uint8).reshape(1, T, 1, H, 1, 1)).to(dev)
        plan, sizes, left = G.plan_gaps(mask)
        assert not left.any()
        mk = ops.apply_mask(full, mask)
        m2 = mask.view(T, H)
        cal = G.calibration_data(mk, mask, "acs", acs)
        weights, info = G.grappa_weights_gaps(cal[0], sizes, (KY, KX), LAM)
        table, count, _ = G.gap_table(mask, sizes)
        out = torch.empty_like(mk)
        n_targets = int((~row).sum()) * T
        parts = {
            "cine_grappa_gaps": lambda: G.gap_table(mask, sizes),
            "fit_all_steps": lambda: G.grappa_weights_gaps(cal[0], sizes, (KY, KX), LAM),
            "cine_grappa_apply_gaps": lambda: G.grappa_apply_gaps(mk[0], weights, sizes, m2, table[0], count[0], (KY, KX), out=out[0]),
            "cine_grappa_apply_gaps_in_place": lambda: G.grappa_apply_gaps(out[0], weights, sizes, m2, table[0], count[0], (KY, KX), out=out[0]),
        }
        default = G.Grappa().gaps                                       # the steps of the module's default: five Gram / solve pairs
        parts["fit_steps_" + "_".join(map(str, default))] = lambda: G.grappa_weights_gaps(cal[0], default, (KY, KX), LAM)
        for G_ in sizes:
            parts[f"fit_step_{G_}"] = (lambda g: (lambda: G.grappa_weights(cal[0], g, (KY, KX), LAM)))(G_)
        us = {k: median(measure(fn, dev)[0]) * 1e3 for k, fn in parts.items()}
        b = {"mask": "EquispacedMaskFunc([0.08], [4]), seed 0, the same for every frame", "acs": list(acs), "gap_steps": list(sizes),
             "gaps_per_frame": len(plan[0][0]), "target_rows": n_targets, "entry_us": us, "weights_info": info.cpu().tolist()}
        flops = 8.0 * n_targets * W * ns * C
        b["apply_tflops"] = flops / us["cine_grappa_apply_gaps_in_place"] * 1e-6
        print(json.dumps({"equispaced": b}), flush=True)

        def fused():
            return G.grappa(mk, mask, None, kernel=(KY, KX), lam=LAM, acs=acs, output="kspace", check=False, gaps=sizes)

        rows_t = torch.from_numpy(row).to(dev)
        targets = {}                                                     # (step, type) -> (h,) rows of that type
        for lo, g in plan[0][0]:
            for m in range(1, g):
                if 0 <= lo + m < H:
                    targets.setdefault((g, m), torch.zeros(H, dtype=torch.bool, device=dev))[lo + m] = True

        def composed():
            k = torch.view_as_complex(mk[0])                             # (t, c, h, w)
            cb = k[:, :, acs[0]:acs[1]].mean(0).to(torch.complex128)     # every frame acquired the block
            x = torch.cat((k.real, k.imag), 1)
            filled = x
            for g in sizes:
                my, mx = (acs[1] - acs[0]) - g, W - KX + 1
                cols = [cb[:, j * g:j * g + my, dx:dx + mx] for j in range(KY) for dx in range(KX)]
                cols += [cb[:, m:m + my, hx:hx + mx] for m in range(1, g)]
                P = torch.stack(cols, 0).reshape(-1, my * mx).transpose(0, 1)
                Gm = P.conj().transpose(0, 1) @ P
                A = Gm[:ns, :ns] + LAM * Gm[:ns, :ns].diagonal().real.sum() / ns * torch.eye(ns, dtype=torch.complex128, device=dev)
                Wc = torch.linalg.solve(A, Gm[:ns, ns:]) if solve_on_device else torch.linalg.solve(A.cpu(), Gm[:ns, ns:].cpu()).to(dev)
                Wc = Wc.to(torch.complex64).reshape(KY, KX, C, g - 1, C)
                for m in range(1, g):
                    if (g, m) not in targets:
                        continue
                    wq = Wc[:, :, :, m - 1].permute(3, 2, 0, 1)
                    wt = torch.cat((torch.cat((wq.real, -wq.imag), 1), torch.cat((wq.imag, wq.real), 1)), 0).contiguous()
                    y = F.conv2d(F.pad(x, (hx, hx, m, g - m)), wt, dilation=(g, 1))
                    filled = torch.where(targets[(g, m)][None, None, :, None], y, filled)
            return torch.stack((filled[:, :C], filled[:, C:]), -1)[None]

        kf, kc = fused(), composed()
        b["fused_vs_composed_max_abs_over_peak"] = float((kf - kc).abs().max() / kc.abs().max())
        del kf, kc
        for variant, fn in (("fused", fused), ("composed", composed), ("fused_again", fused), ("composed_again", composed)):
            G.release_workspaces()
            torch.cuda.empty_cache()
            ms, peak = measure(fn, dev)
            b[variant] = {"median_ms": median(ms), "ms": ms, "peak_bytes": peak}
            print(json.dumps({variant: b[variant]}), flush=True)
        ms, _ = measure(lambda: G.grappa(mk, mask, None, kernel=(KY, KX), lam=LAM, acs=acs, output="kspace", check=False, gaps=default), dev)
        b["fused_default_steps"] = {"gaps": list(default), "median_ms": median(ms), "ms": ms}
        b["composed_over_fused"] = b["composed"]["median_ms"] / b["fused"]["median_ms"]
        b["peak_fused_over_composed"] = b["fused"]["peak_bytes"] / b["composed"]["peak_bytes"]
        doc["equispaced"] = b

        # ---- (c) through the pipeline
        model = G.Grappa(accel=None, gaps=sizes, kernel=(KY, KX), lam=LAM, acs=acs).eval()
        doc["pipeline"] = dict(pipeline_rate(model, mk, mask), model=f"Grappa(accel=None, gaps={tuple(sizes)})")
        print(json.dumps({"pipeline": doc["pipeline"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


def gfactor_main(args):
    import numpy as np
    from cine_hip import grappa as G, noise as N, ops, synth
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    ex = synth.make_cine_slice(T, C, H, W, accel=4, seed=0, noise_std=0.01)
    commit, csrc = _stamp(args.commit)
    ns, base, hx = KY * KX * C, (KY // 2 - 1) * R, KX // 2
    replicas = 64
    doc = {"shape": [1, T, C, H, W], "accel": R, "kernel": [KY, KX], "lam": LAM, "calib": f"tgrappa, calib_rows={CALIB_ROWS}",
           "device": torch.cuda.get_device_name(dev), "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS,
           "commit": commit, "csrc_sha256": csrc, "replicas": replicas}
    with torch.no_grad():
        full = ex["kspace"].to(dev)
        mask = G.lattice_mask(T, H, R).to(dev)
        ones = torch.ones_like(mask)
        mk = ops.apply_mask(full, mask)
        sens = ex["sens_maps"].to(dev) if "sens_maps" in ex else None
        if sens is None:
            sm = synth.coil_maps(C, H, W)
            sens = torch.from_numpy(np.stack((sm.real, sm.imag), -1).astype(np.float32))[None, None].to(dev)
        coef = sens[0].clone()
        coef[..., 1].neg_()                                                                                   # p = conj(S), (1, c, h, w, 2)
        rs = np.random.RandomState(0)
        M = rs.standard_normal((C, C)) + 1j * rs.standard_normal((C, C))
        chol = N.noise_cholesky(torch.from_numpy(M @ M.conj().T / C + np.eye(C))).to(dev)
        cal = G.calibration_data(mk, mask, "tgrappa", None, CALIB_ROWS)
        weights, _ = G.grappa_weights(cal[0], R, (KY, KX), LAM)
        model = G.Grappa(accel=R, kernel=(KY, KX), lam=LAM, calib="tgrappa", calib_rows=CALIB_ROWS).eval()

        def composed(low, p):
            wc = torch.view_as_complex(weights).reshape(R - 1, KY, KX, C, C)                                  # (m - 1, j, dx, k, q)
            kpad = torch.zeros(C, C, H, W, dtype=torch.complex64, device=dev)
            kpad[:, :, 0, 0] = torch.eye(C, dtype=torch.complex64, device=dev)
            for m in range(1, R):
                for j in range(KY):
                    for dx in range(KX):
                        kpad[:, :, (-m - base + j * R) % H, (dx - hx) % W] = wc[m - 1, j, dx].transpose(0, 1)
            wimg = torch.fft.fftshift(torch.fft.fft2(kpad), dim=(-2, -1))
            lc = torch.eye(C, dtype=torch.complex64, device=dev) if low is None else torch.view_as_complex(low.contiguous()).tril()
            if p is None:
                t_ = torch.einsum("qkyx,kj->qjyx", wimg, lc)
                den = (lc.abs() ** 2).sum(1)[:, None, None]
            else:
                pc = torch.view_as_complex(p)
                t_ = torch.einsum("nqyx,qkyx,kj->njyx", pc, wimg, lc)
                den = (torch.einsum("nqyx,qj->njyx", pc, lc).abs() ** 2).sum(1)
            amp2 = (t_.abs() ** 2).sum(1)
            return torch.sqrt(amp2 / den) / R, torch.sqrt(amp2)

        low = torch.view_as_real(chol).contiguous()
        fused = G.grappa_gfactor_from_weights(weights, R, (KY, KX), H, W, chol=chol, coef=coef)
        g_c, _ = composed(low, coef)
        doc["fused_vs_composed_max_rel_g"] = float(((fused.g - g_c).abs() / g_c).max())
        doc["g_maps"] = {"min": float(fused.g.min()), "median": float(fused.g.median()), "max": float(fused.g.max())}
        del g_c, fused
        from cine_hip._lib import lib
        g_pc, a_pc = torch.empty(C, H, W, device=dev), torch.empty(C, H, W, device=dev)
        g_m, a_m = torch.empty(1, H, W, device=dev), torch.empty(1, H, W, device=dev)
        wp, lp, cp, st = weights.data_ptr(), low.data_ptr(), coef.data_ptr(), ops._stream

        def entry(l_ptr, c_ptr, g_t, a_t):                                                                    # the C entry alone, outputs in place
            return lambda: lib().cine_grappa_gfactor(wp, l_ptr, c_ptr, g_t.data_ptr(), a_t.data_ptr(), 1, C, H, W, R, KY, KX, st())
        parts = {
            "entry_gfactor_per_coil": entry(None, None, g_pc, a_pc),
            "entry_gfactor_per_coil_chol": entry(lp, None, g_pc, a_pc),
            "entry_gfactor_maps": entry(None, cp, g_m, a_m),
            "entry_gfactor_maps_chol": entry(lp, cp, g_m, a_m),
            "cine_grappa_gfactor_per_coil": lambda: G.grappa_gfactor_from_weights(weights, R, (KY, KX), H, W),
            "cine_grappa_gfactor_per_coil_chol": lambda: G.grappa_gfactor_from_weights(weights, R, (KY, KX), H, W, chol=chol),
            "cine_grappa_gfactor_maps": lambda: G.grappa_gfactor_from_weights(weights, R, (KY, KX), H, W, coef=coef),
            "cine_grappa_gfactor_maps_chol": lambda: G.grappa_gfactor_from_weights(weights, R, (KY, KX), H, W, chol=chol, coef=coef),
            "cine_grappa_image_weights": lambda: G.grappa_image_weights(weights, R, (KY, KX), H, W),
            "composed_per_coil_chol": lambda: composed(low, None),
            "composed_maps_chol": lambda: composed(low, coef),
            "grappa_noise_maps_with_calibration": lambda: model.noise_maps(mk, mask, sens, chol=chol),
            "pseudo_replica_lattice": lambda: N.pseudo_replica(model, mk, mask, sens, chol=chol, replicas=replicas, output="complex"),
            "pseudo_replica_full": lambda: N.pseudo_replica(model, full, ones, sens, chol=chol, replicas=replicas, output="complex"),
        }
        doc["entry_ms"], doc["peak_bytes"] = {}, {}
        for name, fn in parts.items():
            G.release_workspaces()
            torch.cuda.empty_cache()
            ms, peak = measure(fn, dev)
            doc["entry_ms"][name], doc["peak_bytes"][name] = median(ms), peak
            print(json.dumps({name: {"median_ms": median(ms), "peak_bytes": peak}}), flush=True)
        e = doc["entry_ms"]
        doc["flop_maps_chol"] = 8.0 * H * W * (C * C * KX + C * C + C * C / 2)
        doc["composed_over_fused_maps_chol"] = e["composed_maps_chol"] / e["cine_grappa_gfactor_maps_chol"]
        doc["composed_over_fused_per_coil_chol"] = e["composed_per_coil_chol"] / e["cine_grappa_gfactor_per_coil_chol"]
        doc["measured_g_map_over_analytic"] = (e["pseudo_replica_lattice"] + e["pseudo_replica_full"]) / e["grappa_noise_maps_with_calibration"]
        print(json.dumps({k: doc[k] for k in ("composed_over_fused_maps_chol", "composed_over_fused_per_coil_chol", "measured_g_map_over_analytic",
                                              "fused_vs_composed_max_rel_g", "g_maps")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit to stamp the result with (default: git rev-parse HEAD)")
    ap.add_argument("--gaps", action="store_true", help="measure the path for unevenly spaced rows (accel=None)")
    ap.add_argument("--gfactor", action="store_true", help="measure the analytic noise maps (cine_grappa_gfactor, cine_grappa_image_weights)")
    args = ap.parse_args()
    if args.gaps:
        return gaps_main(args)
    if args.gfactor:
        return gfactor_main(args)
    from cine_hip import grappa as G, ops, synth
    from cine_hip._lib import lib
    from cine_hip.pipeline import SlicePipeline
    from pipeline_rate import _stamp
    dev = torch.device("cuda:0")
    ex = synth.make_cine_slice(T, C, H, W, accel=4, seed=0, noise_std=0.01)
    mask = G.lattice_mask(T, H, R).to(dev)
    commit, csrc = _stamp(args.commit)
    solve_on_device = device_solve_works(dev)
    ns, nr, base, hx = KY * KX * C, (R - 1) * C, (KY // 2 - 1) * R, KX // 2
    doc = {"shape": [1, T, C, H, W], "accel": R, "kernel": [KY, KX], "lam": LAM, "calib": f"tgrappa, calib_rows={CALIB_ROWS}",
           "mask": "interleaved lattice of step 4, no ACS lines", "device": torch.cuda.get_device_name(dev),
           "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "steps": STEPS, "commit": commit, "csrc_sha256": csrc, "ns": ns,
           "n_aug": ns + nr, "composed_solve": "torch.linalg.solve in complex128 on the " + ("device" if solve_on_device else "host")}
    with torch.no_grad():
        mk = ops.apply_mask(ex["kspace"].to(dev), mask)
        rows = mask.view(T, H) != 0
        off_host = torch.from_numpy(G.plan_lattice(mask, R)[0]).to(dev)
        m_of_row = (torch.arange(H, device=dev)[None, :] - off_host[:, None].long()) % R                      # (t, h): 0 on the lattice
        target = [(m_of_row == m) & ~rows for m in range(1, R)]
        n_targets = int(sum(int(tm.sum()) for tm in target))

        # ---- the entry points alone
        off, status = G.lattice_offsets(mask, R)
        cal = G.calibration_data(mk, mask, "tgrappa", None, CALIB_ROWS)
        weights, info = G.grappa_weights(cal[0], R, (KY, KX), LAM)
        hc = cal.shape[2]
        gram = torch.empty((ns + nr, ns + nr), device=dev, dtype=torch.complex128)
        nb_g, nb_w = lib().cine_grappa_gram_ws_bytes(C, hc, W, R, KY, KX), lib().cine_grappa_weights_ws_bytes(C, R, KY, KX)
        ws = torch.empty(max(nb_g, nb_w), device=dev, dtype=torch.uint8)
        st = ops._stream
        out = torch.empty_like(mk)
        parts = {
            "cine_grappa_offsets": lambda: lib().cine_grappa_offsets(mask.data_ptr(), off.data_ptr(), status.data_ptr(), T, H, R, st()),
            "cine_grappa_gram": lambda: lib().cine_grappa_gram(cal.data_ptr(), gram.data_ptr(), ws.data_ptr(), nb_g, C, hc, W, R, KY, KX, st()),
            "cine_grappa_weights": lambda: lib().cine_grappa_weights(gram.data_ptr(), weights.data_ptr(), info.data_ptr(), ws.data_ptr(), nb_w, C,
                                                                     R, KY, KX, LAM, st()),
            "cine_grappa_apply": lambda: G.grappa_apply(mk[0], weights, mask.view(T, H), off[0], R, (KY, KX), out=out[0]),
            "cine_grappa_apply_in_place": lambda: G.grappa_apply(out[0], weights, mask.view(T, H), off[0], R, (KY, KX), out=out[0]),
        }
        lib().cine_grappa_gram(cal.data_ptr(), gram.data_ptr(), ws.data_ptr(), nb_g, C, hc, W, R, KY, KX, st())
        doc["entry_us"] = {k: median(measure(fn, dev)[0]) * 1e3 for k, fn in parts.items()}
        flops = 8.0 * n_targets * W * ns * C
        moved = 8 * W * C * (int(rows.sum()) + n_targets) + weights.numel() * 4
        us = doc["entry_us"]["cine_grappa_apply_in_place"]
        doc["apply"] = {"target_rows": n_targets, "flop": flops, "bytes": moved, "flop_per_byte": flops / moved, "tflops": flops / us * 1e-6,
                        "gb_per_s": moved / us * 1e-3, "weights_info": info.cpu().tolist()}
        print(json.dumps({"entry_us": doc["entry_us"], "apply": doc["apply"]}), flush=True)

        # ---- the whole call against the composed torch path
        def fused():
            return G.grappa(mk, mask, R, kernel=(KY, KX), lam=LAM, calib="tgrappa", calib_rows=CALIB_ROWS, output="kspace", check=False)

        def composed():
            k = torch.view_as_complex(mk[0])                                                                  # (t, c, h, w)
            cnt = rows.sum(0).clamp(min=1).to(torch.float32)
            avg = (k * rows[:, None, :, None]).sum(0) / cnt[None, :, None]
            lo = H // 2 - CALIB_ROWS // 2
            cb = avg[:, lo:lo + CALIB_ROWS].to(torch.complex128)
            span = (KY - 1) * R + 1
            my, mx = CALIB_ROWS - span + 1, W - KX + 1
            cols = [cb[:, j * R:j * R + my, dx:dx + mx] for j in range(KY) for dx in range(KX)]
            cols += [cb[:, base + m:base + m + my, hx:hx + mx] for m in range(1, R)]
            P = torch.stack(cols, 0).reshape(-1, my * mx).transpose(0, 1)
            Gm = P.conj().transpose(0, 1) @ P
            A = Gm[:ns, :ns] + LAM * Gm[:ns, :ns].diagonal().real.sum() / ns * torch.eye(ns, dtype=torch.complex128, device=dev)
            Wc = torch.linalg.solve(A, Gm[:ns, ns:]) if solve_on_device else torch.linalg.solve(A.cpu(), Gm[:ns, ns:].cpu()).to(dev)
            Wc = Wc.to(torch.complex64).reshape(KY, KX, C, R - 1, C)                                          # (j, dx, k, m - 1, q)
            x = torch.cat((k.real, k.imag), 1)                                                                # (t, 2c, h, w)
            filled = x
            for m in range(1, R):
                wq = Wc[:, :, :, m - 1].permute(3, 2, 0, 1)                                                   # (q, k, j, dx)
                wt = torch.cat((torch.cat((wq.real, -wq.imag), 1), torch.cat((wq.imag, wq.real), 1)), 0).contiguous()
                top = m + base
                y = F.conv2d(F.pad(x, (hx, hx, top, (KY - 1) * R - top)), wt, dilation=(R, 1))
                filled = torch.where(target[m - 1][:, None, :, None], y, filled)
            return torch.stack((filled[:, :C], filled[:, C:]), -1)[None]

        kf, kc = fused(), composed()
        doc["fused_vs_composed_max_abs_over_peak"] = float((kf - kc).abs().max() / kc.abs().max())
        del kf, kc
        for variant, fn in (("fused", fused), ("composed", composed), ("fused_again", fused), ("composed_again", composed)):
            G.release_workspaces()
            torch.cuda.empty_cache()
            ms, peak = measure(fn, dev)
            doc[variant] = {"median_ms": median(ms), "ms": ms, "peak_bytes": peak}
            print(json.dumps({variant: doc[variant]}), flush=True)
        doc["composed_over_fused"] = doc["composed"]["median_ms"] / doc["fused"]["median_ms"]
        doc["peak_fused_over_composed"] = doc["fused"]["peak_bytes"] / doc["composed"]["peak_bytes"]

        # the application alone, composed: the convolutions and the scatter with the weights given
        wts_c = torch.view_as_complex(weights).reshape(R - 1, KY, KX, C, C)
        xin = torch.cat((torch.view_as_complex(mk[0]).real, torch.view_as_complex(mk[0]).imag), 1)

        def conv_apply():
            filled = xin
            for m in range(1, R):
                wq = wts_c[m - 1].permute(3, 2, 0, 1)
                wt = torch.cat((torch.cat((wq.real, -wq.imag), 1), torch.cat((wq.imag, wq.real), 1)), 0).contiguous()
                top = m + base
                y = F.conv2d(F.pad(xin, (hx, hx, top, (KY - 1) * R - top)), wt, dilation=(R, 1))
                filled = torch.where(target[m - 1][:, None, :, None], y, filled)
            return filled
        doc["entry_us"]["composed_conv2d_apply"] = median(measure(conv_apply, dev)[0]) * 1e3
        doc["conv2d_apply_over_cine_grappa_apply"] = doc["entry_us"]["composed_conv2d_apply"] / doc["entry_us"]["cine_grappa_apply"]
        print(json.dumps({k: doc[k] for k in ("composed_over_fused", "peak_fused_over_composed", "conv2d_apply_over_cine_grappa_apply",
                                              "fused_vs_composed_max_abs_over_peak")}), flush=True)

        model = G.Grappa(accel=R, kernel=(KY, KX), lam=LAM, calib="tgrappa", calib_rows=CALIB_ROWS).eval()
        with SlicePipeline(model, slots=SLOTS) as pipe:
            pipe.submit(mk, mask, tag="build")
            list(pipe.drain())
            rates = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for j in range(SLICES):
                    pipe.submit(mk, mask, tag=j)
                    for _ in pipe.results():
                        pass
                list(pipe.drain())
                torch.cuda.synchronize()
                rates.append(SLICES / (time.perf_counter() - t0))
        doc["pipeline"] = {"model": f"Grappa(accel={R})", "slots": SLOTS, "slices": SLICES, "slices_per_s": median(rates), "runs": rates}
        print(json.dumps({"pipeline": doc["pipeline"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
