#!/usr/bin/env python3
"""HIP-event time of `Flow.log_prob` of masked autoregressive affine flows in one launch (K22) against the same flow with
NFA_K22=0 -- layer by layer: a `weight * mask` product cache, the MADE's GEMMs, K2b and a permutation per layer, which is
what a user had before.

    python tools/maf_time.py [--out profiles/maf_time.json] [--tree PATH]

Shapes (features, hidden, layers, blocks per layer; reverse permutations between the layers as the factory puts them):
(8, 128, 5, 2), (43, 128, 10, 2), (64, 128, 16, 2), (16, 128, 8, 2) with BatchNorm between the layers (eval mode: every MAF
layer a run of one, every BatchNorm one K17 launch), (21, 128, 8, 2) with a 16-feature context; 1 024, 16 384 and 262 144
rows each.  Every shape runs in a fresh child process; per row count the two paths alternate (one launch, layer by layer,
twice each), and every figure is the median (with min / max = the spread) of `--reps` single calls between event pairs and
of trains of calls between one pair (`timed`, as tools/nonlin_time.py).  `max_abs_difference`: the two paths' log_prob on the
timed rows, beside the largest |log_prob| there.  `--tree`: another checkout of the package (the parent commit's) whose log_prob is timed on the same rows with
this build's library, to confirm that NFA_K22=0 is that path."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
DEVICE_ERROR = re.compile(r"HIP error|hipError|HSA_STATUS|illegal memory access|device-side assert|Memory access fault", re.I)
SHAPES = {
    "d8_l5": dict(features=8, hidden_features=128, num_layers=5, num_blocks=2),
    "d43_l10": dict(features=43, hidden_features=128, num_layers=10, num_blocks=2),
    "d64_l16": dict(features=64, hidden_features=128, num_layers=16, num_blocks=2),
    "d16_l8_batch_norm": dict(features=16, hidden_features=128, num_layers=8, num_blocks=2, batch_norm=True),
    "d21_l8_context16": dict(features=21, hidden_features=128, num_layers=8, num_blocks=2, context_features=16),
}
ROWS = (1024, 16384, 262144)


def build(cfg):
    import torch
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.transforms import (BatchNorm, CompositeTransform, MaskedAffineAutoregressiveTransform,
                                       ReversePermutation)
    torch.manual_seed(0)
    d, layers = cfg["features"], []
    for _ in range(cfg["num_layers"]):
        layers.append(ReversePermutation(d))
        layers.append(MaskedAffineAutoregressiveTransform(features=d, hidden_features=cfg["hidden_features"],
                                                          context_features=cfg.get("context_features"),
                                                          num_blocks=cfg["num_blocks"]))
        if cfg.get("batch_norm"):
            layers.append(BatchNorm(d))
    flow = Flow(CompositeTransform(layers), StandardNormal([d]))
    with torch.no_grad():   # off the near-identity initialisation, as tests/maf_cases.py
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.mul_(2.0)
            elif "linear_layers.1" in name:
                p.mul_(100.0)
    flow = flow.to(DEV)
    if cfg.get("batch_norm"):   # running statistics of a trained flow's size (they start at mean 0, variance 0)
        with torch.no_grad():
            flow.train()
            for i in range(50):
                flow.log_prob(1.2 * torch.randn(4096, d, device=DEV, generator=torch.Generator(DEV).manual_seed(100 + i)))
    return flow.eval()


def child(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    else:
        sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    from nonlin_time import timed
    from nflows_amd import ops
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform as MAF
    cfg = SHAPES[args.case]
    flow = build(cfg)
    has_switch = hasattr(MAF, "fuse_conditioner")
    for rows in ROWS:
        g = torch.Generator(DEV).manual_seed(rows)
        x = 1.2 * torch.randn(rows, cfg["features"], device=DEV, generator=g)
        ce = cfg.get("context_features")
        ctx = None if ce is None else torch.randn(rows, ce, device=DEV, generator=g)

        def call():
            with torch.no_grad():
                return flow.log_prob(x, context=ctx)
        entry = {"shape": args.case, "rows": rows, **cfg}
        if not has_switch:   # another tree without K22: its only path
            entry["layer_by_layer"] = [timed(call, args.reps)]
            print("RESULT " + json.dumps(entry), flush=True)
            continue
        results = {"one_launch": [], "layer_by_layer": []}
        values = {}
        for _ in range(2):   # the two paths alternate
            for name, on in (("one_launch", True), ("layer_by_layer", False)):
                MAF.fuse_conditioner = on
                values[name] = call()
                if on:
                    entry["kernel"] = ops.last_layer_kernel()
                results[name].append(timed(call, args.reps))
        MAF.fuse_conditioner = True
        entry.update(results)
        entry["max_abs_difference"] = float((values["one_launch"] - values["layer_by_layer"]).abs().max())
        entry["max_abs_log_prob"] = float(values["layer_by_layer"].abs().max())
        for label, key in (("speedup", "median_us"), ("speedup_back_to_back", "back_to_back_median_us")):
            one = statistics.median(r[key] for r in results["one_launch"])
            many = statistics.median(r[key] for r in results["layer_by_layer"])
            entry[label] = many / one
        entry["one_launch_not_slower"] = bool(
            min(r["median_us"] for r in results["one_launch"]) <= max(r["max_us"] for r in results["layer_by_layer"])
            and min(r["back_to_back_median_us"] for r in results["one_launch"])
            <= max(r["back_to_back_max_us"] for r in results["layer_by_layer"]))
        print("RESULT " + json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=None, help="time log_prob of the package in this other checkout (no switch needed)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--case", default=None, help="internal: one shape in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from nonlin_time import smi
    result = {"clocks_power_before": smi(), "tree": args.tree, "cases": []}
    for name in args.shapes.split(","):   # every shape in a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)]
        if args.tree:
            cmd += ["--tree", args.tree]
        stderr = ""
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            stderr = run.stderr
            entries = [json.loads(ln[7:]) for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            failed = run.returncode
        except subprocess.TimeoutExpired:
            entries, failed = [], "timeout"
        for entry in entries:
            print(json.dumps(entry), flush=True)
        result["cases"] += entries
        if failed:
            result["cases"].append({"shape": name, "child_exit": failed,
                                    "child_stderr": stderr.strip().splitlines()[-1][:200] if stderr.strip() else ""})
            print(json.dumps(result["cases"][-1]), flush=True)
            # a device fault reaches Python as a RuntimeError, exit status 1 like any other: go on only after an exit of 1
            # whose output names no HIP / HSA error, and start nothing more on the device otherwise
            if failed != 1 or DEVICE_ERROR.search(stderr):
                break
    result["clocks_power_after"] = smi()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    if any("child_exit" in c for c in result["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
