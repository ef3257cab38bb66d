#!/usr/bin/env python3
"""Digest of every data-consistency path of the model families: what a refactor of the dispatch must leave bit for bit.

    python tools/dc_paths_digest.py --out profiles/dc_paths_digest.json [--runs 2]
    python tools/dc_paths_digest.py --compare PARENT.json BRANCH.json

Cases: the nine families of tests/test_general_mask_models.py (same tiny models and shapes), VarNet with its own sensitivity network,
XPDNet(primal_only=False) and XPDNet_RNN with the dual buffer; each with {a row mask, a mask that varies along w with
ops.GENERAL_MASK_FUSED on, the same mask with it off}.  Per case: the sha256 of the inference output (eval, no_grad), the delta of every
counter cine_diag_counter knows over that forward, and -- where the family trains through the HIP path -- the sha256 of the training
output and of every parameter gradient (in --out the gradients of a case are folded into one digest of their digests).  Every family runs in a child process of its own under a time limit; the first child that
fails ends the run.  ``--runs 2`` repeats everything and lists the entries whose two digests differ under "nondeterministic"; the
tensors behind the digests go to OUT.tensors/ (beside --out, not for git) so that --compare can measure such an entry as a relative
error instead.  --compare: every entry that is deterministic in PARENT must be identical in BRANCH; exit status 1 otherwise."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deep-cine-cardiac-mri_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ACS = (9, 6)
XKW = dict(num_cascades=2, sens_chans=4, sens_pools=2, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[1, 1], first_conv_n_filters=8,
           n_primal=2, dynamic_type="XF", weight_sharing=False)
A, B = (5, 3, 20, 18), (4, 3, 24, 20)            # (t, c, h, w)
# family -> (constructor, takes sens_maps, shape, bar of the existing gradient test of that family for a non-deterministic entry)
FAMILIES = {
    "varnet_XF": (lambda m: m.VarNet(2, 4, 2, 4, 2, "XF"), True, A, 1e-3),
    "varnet_2D": (lambda m: m.VarNet(2, 4, 2, 4, 2, "2D"), True, A, 1e-3),
    "varnet_3D": (lambda m: m.VarNet(2, 4, 2, 4, 2, "3D"), True, A, 1e-3),
    "varnet_XF_sensnet": (lambda m: m.VarNet(2, 4, 2, 4, 2, "XF"), False, B, 1e-3),
    "cinenet_XF": (lambda m: m.CineNet(2, 3, 4, 2, "XF"), True, A, 1e-3),
    "cinenet_3D": (lambda m: m.CineNet(2, 2, 4, 2, "3D"), True, A, 1e-3),
    "xpdnet": (lambda m: m.XPDNet(primal_only=True, **XKW), False, B, 2e-3),
    "xpdnet_dual": (lambda m: m.XPDNet(primal_only=False, **XKW), False, B, 2e-3),
    "varnet_rnn": (lambda m: m.VarNet_RNN(2, 4, 2, 6), False, B, 2e-3),
    "cinenet_rnn": (lambda m: m.CineNet_RNN(2, 3, 6), True, B, 2e-3),
    "xpdnet_rnn": (lambda m: m.XPDNet_RNN(2, 4, 2, 6, True, 2, 1), False, B, 2e-3),
    "xpdnet_rnn_dual": (lambda m: m.XPDNet_RNN(2, 4, 2, 6, False, 2, 1), False, B, 2e-3),
}
MODES = ("row", "general_fused", "general_literal")
CHILD_LIMIT_S = 240


def sha(x) -> str:
    return hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def counters(reset: int = 1):
    from cine_hip._lib import lib
    out, i = [], 0
    while True:
        v = lib().cine_diag_counter(i, reset)
        if v == -1:
            return out
        out.append(int(v))
        i += 1


def run_family(family: str, tensor_path: str) -> dict:
    import torch
    import reconstruction.models as M
    from cine_hip import ops, synth
    make, takes_sens, (t, c, h, w), _ = FAMILIES[family]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(6)
    general = (torch.rand(1, t, 1, h, w, 1, generator=g) < 0.4).to(torch.uint8)
    general[:, :, :, 9:15, w // 2 - 4:w // 2 + 4] = 1
    row = general[:, :, :, :, w // 2:w // 2 + 1, :].contiguous()
    sens = torch.randn(1, 1, c, h, w, 2, generator=g)
    sens = (sens / sens.pow(2).sum(dim=(2, 5), keepdim=True).sqrt()).to(dev)
    kfull = torch.randn(1, t, c, h, w, 2, generator=g)
    target = (torch.randn(1, t, h, w, generator=g).abs() + 0.1).to(dev)
    net = make(M)
    synth.fill_parameters_(net, 17, keep=("lambda",))
    net = net.to(dev)
    entries, tensors = {}, {}

    def call(mk, mask):
        with ops.branches(1):
            return net(mk, mask, sens) if takes_sens else net(mk, mask, acs=ACS)

    for mode in MODES:
        mask = row if mode == "row" else general
        ops.GENERAL_MASK_FUSED = mode != "general_literal"
        mk, mask_d = (kfull * mask).to(dev), mask.to(dev)
        key = f"{family}/{mode}"
        net.eval()
        with torch.no_grad():
            call(mk, mask_d)                               # caches (packed weights, side streams) outside the counted forward
        torch.cuda.synchronize()
        counters()
        with torch.no_grad():
            out = call(mk, mask_d)
        torch.cuda.synchronize()
        entries[key + "/counters"] = counters()
        entries[key + "/infer"] = sha(out); tensors[key + "/infer"] = out.cpu()
        net.train(); net.zero_grad(set_to_none=True)
        try:
            with torch.enable_grad():
                out = call(mk, mask_d)
                ((out - target) ** 2).mean().backward()
        except NotImplementedError as e:
            entries[key + "/train"] = f"not on the HIP path: {e}"
            continue
        torch.cuda.synchronize()
        entries[key + "/train"] = sha(out); tensors[key + "/train"] = out.detach().cpu()
        for name, p in net.named_parameters():
            entries[f"{key}/grad/{name}"] = "none" if p.grad is None else sha(p.grad)
            if p.grad is not None:
                tensors[f"{key}/grad/{name}"] = p.grad.cpu()
    ops.GENERAL_MASK_FUSED = True
    torch.save(tensors, tensor_path)
    return entries


def one_run(tensor_dir: str, run: int) -> dict:
    entries = {}
    for family in FAMILIES:
        path = os.path.join(tensor_dir, f"{family}.run{run}.pt")
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--family", family, "--tensors", path],
                           stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:         # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.exit(f"dc_paths_digest: {family} ended with status {r.returncode}; stopping here\n{r.stdout[-2000:]}")
        entries.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"run {run}: {family} done", flush=True)
    return entries


def condense(entries: dict) -> dict:
    """The form that is committed: the digests of a case's parameter gradients folded into one, the sha256 of their "name digest" lines
    (several hundred lines per case otherwise); the digest of each single gradient stays in OUT.tensors/entries.json."""
    out, grads = {}, {}
    for key, v in entries.items():
        case, sep, name = key.partition("/grad/")
        if sep:
            grads.setdefault(case, []).append(f"{name} {v}")
        else:
            out[key] = v
    for case, lines in grads.items():
        out[case + "/grads"] = f"{len(lines)} gradients, sha256 " + hashlib.sha256("\n".join(sorted(lines)).encode()).hexdigest()
    return out


def compare(parent_path: str, branch_path: str) -> int:
    import torch
    parent, branch = json.load(open(parent_path)), json.load(open(branch_path))
    loose = set(parent["nondeterministic"]) | set(branch["nondeterministic"])
    bad, cache = [], {}

    def tensor(path, key):
        f = os.path.join(path + ".tensors", key.split("/")[0] + ".run0.pt")
        if f not in cache:
            cache[f] = torch.load(f)
        return cache[f][key].double()

    def check(key, want, got):
        if key not in loose or key.endswith("/counters"):
            if got != want:
                bad.append((key, want, got))
            return
        a, b = tensor(parent_path, key), tensor(branch_path, key)
        e = float((a - b).norm() / a.norm().clamp_min(1e-30))
        bar = FAMILIES[key.split("/")[0]][3] if "/grad/" in key else 2e-5       # (outputs: the tighter forward bar of those tests)
        print(f"non-deterministic {key}: |branch - parent| / |parent| = {e:.3e} (bar {bar:.0e})")
        if not e < bar:
            bad.append((key, e, bar))

    for key, want in parent["entries"].items():
        prefix = key[:-1] + "/" if key.endswith("/grads") else None         # case/grads -> case/grad/
        if prefix and any(k.startswith(prefix) for k in loose):             # gradient by gradient, from the entries beside the tensors
            full = [json.load(open(os.path.join(q + ".tensors", "entries.json"))) for q in (parent_path, branch_path)]
            for k in (k for k in full[0] if k.startswith(prefix)):
                check(k, full[0][k], full[1].get(k))
        else:
            check(key, want, branch["entries"].get(key))
    extra = sorted(set(branch["entries"]) - set(parent["entries"]))
    print(f"{len(parent['entries'])} entries, {len(loose)} non-deterministic, {len(bad)} differ, {len(extra)} only in the branch")
    for item in bad:
        print("DIFFERS", *item)
    return 1 if bad or extra else 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--family", default=None, help="(child) one family, its entries as one JSON line")
    ap.add_argument("--tensors", default=None, help="(child) where the tensors behind the digests go")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "BRANCH"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.family:
        print(json.dumps(run_family(a.family, a.tensors)))
        return 0
    if not a.out:
        ap.error("--out is needed")
    tensor_dir = a.out + ".tensors"
    os.makedirs(tensor_dir, exist_ok=True)
    runs = [one_run(tensor_dir, r) for r in range(a.runs)]
    loose = sorted(k for k in runs[0] if any(r[k] != runs[0][k] for r in runs[1:]))
    with open(os.path.join(tensor_dir, "entries.json"), "w") as f:
        json.dump(runs[0], f, indent=1, sort_keys=True)
    short = condense(runs[0])
    with open(a.out, "w") as f:         # one entry per line
        f.write(json.dumps({"runs": a.runs, "digests": len(runs[0]), "nondeterministic": loose})[:-1] + ', "entries": {\n')
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(short[k])}" for k in sorted(short)) + "\n}}\n")
    print(f"{len(runs[0])} entries, {len(loose)} non-deterministic over {a.runs} run(s) -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
