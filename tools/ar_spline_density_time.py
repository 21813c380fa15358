#!/usr/bin/env python3
"""HIP-event time of `Flow.log_prob` and `flow._transform` of autoregressive rational-quadratic spline flows in one launch
(K29, NFA_K29=2) against the same flow with NFA_K29=0 -- the parent commit's path: a `weight * mask` product cache, the MADE's
hidden GEMMs, then K13 (8 bins) or the final GEMM + K1 (10 bins), a permutation per layer and the base density's kernel
(DESIGN.md section 4, K29).

    python tools/ar_spline_density_time.py [--out profiles/ar_spline_density_time.json] [--shapes d8_l5,...] [--reps 10]

Flows (features, layers; hidden 128, two residual blocks per layer, reverse permutations between the layers): (8, 5),
(21, 10), (43, 10), (64, 16); 8 and 10 bins; with and without a 16-feature context; 1 024, 16 384 and 262 144 rows each.
Every flow runs in a fresh child process; per row count and call the two paths alternate (one launch, layer by layer, twice
each), and every figure is the median (with min / max = the spread) of `--reps` single calls between event pairs and of
trains of calls between one pair (`timed`, as tools/nonlin_time.py).  `max_abs_difference`: the two paths' results on the
timed rows, beside the largest magnitude there.  `floor_us`: the bytes the algorithm must move -- the rows in, the context in,
the log-density (and z for `_transform`) out, every masked weight once -- at 6.3 TB/s, the device's measured copy rate."""
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
FLOWS = {"d8_l5": (8, 5), "d21_l10": (21, 10), "d43_l10": (43, 10), "d64_l16": (64, 16)}
SHAPES = {"%s_k%d%s" % (name, bins, "_c16" if ce else ""): dict(features=d, num_layers=layers, num_bins=bins,
                                                                 context_features=ce, hidden_features=128, num_blocks=2)
          for name, (d, layers) in FLOWS.items() for bins in (8, 10) for ce in (None, 16)}
ROWS = (1024, 16384, 262144)
COPY_RATE = 6.3e12   # bytes per second


def build(cfg):
    import torch
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.transforms import (CompositeTransform, MaskedPiecewiseRationalQuadraticAutoregressiveTransform,
                                       ReversePermutation)
    torch.manual_seed(0)
    d, layers = cfg["features"], []
    for _ in range(cfg["num_layers"]):
        layers.append(ReversePermutation(d))
        layers.append(MaskedPiecewiseRationalQuadraticAutoregressiveTransform(
            features=d, hidden_features=cfg["hidden_features"], context_features=cfg["context_features"],
            num_bins=cfg["num_bins"], tails="linear", tail_bound=3.0, num_blocks=cfg["num_blocks"]))
    flow = Flow(CompositeTransform(layers), StandardNormal([d]))
    with torch.no_grad():   # off the near-identity initialisation, as tests/ar_spline_sample_cases.py
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.mul_(3.0)
            elif "linear_layers.1" in name:
                p.mul_(100.0)
    return flow.to(DEV).eval()


def algorithmic_bytes(flow, rows, features, ce, writes_z):
    weights = sum(p.numel() * 4 for p in flow.parameters())
    return rows * 4 * (features + (ce or 0) + 1 + (features if writes_z else 0)) + weights


def child(args):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    from nonlin_time import timed
    from nflows_amd import ops
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform as AR
    cfg = SHAPES[args.case]
    flow = build(cfg)
    for rows in ROWS:
        g = torch.Generator(DEV).manual_seed(rows)
        x = 1.5 * torch.randn(rows, cfg["features"], device=DEV, generator=g)
        ce = cfg["context_features"]
        ctx = None if ce is None else torch.randn(rows, ce, device=DEV, generator=g)

        def log_prob():
            with torch.no_grad():
                return flow.log_prob(x, context=ctx)

        def transform():
            with torch.no_grad():
                return flow._transform(x, context=ctx)[1]
        for what, call in (("log_prob", log_prob), ("transform", transform)):
            entry = {"shape": args.case, "call": what, "rows": rows, **cfg}
            results = {"one_launch": [], "layer_by_layer": []}
            values = {}
            for _ in range(2):   # the two paths alternate
                for name, mode in (("one_launch", 2), ("layer_by_layer", 0)):
                    AR.fuse_conditioner = mode
                    values[name] = call()
                    if mode:
                        entry["kernel"] = ops.last_layer_kernel()
                    results[name].append(timed(call, args.reps, warmup=5, train=5))
            AR.fuse_conditioner = 1
            entry.update(results)
            entry["max_abs_difference"] = float((values["one_launch"] - values["layer_by_layer"]).abs().max())
            entry["max_abs_value"] = float(values["layer_by_layer"].abs().max())
            for label, key in (("speedup", "median_us"), ("speedup_back_to_back", "back_to_back_median_us")):
                one = statistics.median(r[key] for r in results["one_launch"])
                many = statistics.median(r[key] for r in results["layer_by_layer"])
                entry[label] = many / one
            # slower beyond the spread the runs themselves show: the one launch's best median above the other path's worst call
            entry["one_launch_not_slower"] = bool(
                min(r["median_us"] for r in results["one_launch"]) <= max(r["max_us"] for r in results["layer_by_layer"])
                and min(r["back_to_back_median_us"] for r in results["one_launch"])
                <= max(r["back_to_back_max_us"] for r in results["layer_by_layer"]))
            nbytes = algorithmic_bytes(flow, rows, cfg["features"], ce, what == "transform")
            entry["algorithmic_bytes"] = nbytes
            entry["floor_us"] = nbytes / COPY_RATE * 1e6
            print("RESULT " + json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--case", default=None, help="internal: one flow in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from nonlin_time import smi
    result = {"clocks_power_before": smi(), "cases": []}
    for name in args.shapes.split(","):   # every flow in a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)]
        stderr = ""
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            stderr = run.stderr
            entries = [json.loads(ln[7:]) for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            failed = run.returncode
        except subprocess.TimeoutExpired:
            entries, failed = [], "timeout"
        for entry in entries:
            print(json.dumps({k: entry[k] for k in ("shape", "call", "rows", "speedup", "speedup_back_to_back",
                                                    "one_launch_not_slower", "max_abs_difference")}), flush=True)
        result["cases"] += entries
        if failed:
            result["cases"].append({"shape": name, "child_exit": failed,
                                    "child_stderr": stderr.strip().splitlines()[-1][:200] if stderr.strip() else ""})
            print(json.dumps(result["cases"][-1]), flush=True)
            # a device fault reaches Python as a RuntimeError, exit status 1 like any other: go on only after an exit of 1
            # whose output names no HIP / HSA error, and start nothing more on the device otherwise
            if failed != 1 or DEVICE_ERROR.search(stderr):
                break
        if args.out:   # (kept up to date flow by flow: a run cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)
    result["clocks_power_after"] = smi()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    if any("child_exit" in c for c in result["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
