#!/usr/bin/env python3
"""HIP-event time of `nn.nde.MixtureOfGaussiansMADE.log_prob(x, context)` under torch.no_grad() -- what
`distributions.MADEMoG.log_prob` and every Flow with a MADEMoG base evaluate -- in one launch (K31, NFA_K31) against the same
module with the switch off: the MADE's stock ops and one K20 "mog" launch, which is what a user had before (DESIGN.md
section 4, K31).

    python tools/mog_density_time.py [--out profiles/mog_density_time.json]

Shapes: hidden 128, two blocks, a 16-feature context; see SHAPES.  Every shape runs in a fresh child process; per row count
the two paths alternate (kernel, parts, twice each).  The counts adapt as in tools/maf_sample_time.py (`adaptive_timed`):
figures are medians with min / max = the spread.  The kernel is timed at every size, whatever the class's size rule says
(`dispatch_takes_kernel` records what the rule does there): the rule is read off these figures."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def _shape(features, components, ce=16, residual=True):
    return dict(features=features, context_features=ce, num_mixture_components=components, hidden_features=128, num_blocks=2,
                use_residual_blocks=residual)


SHAPES = {}
for _k in (5, 10):
    SHAPES.update({"d%d_c16_k%d" % (_d, _k): _shape(_d, _k) for _d in (8, 21, 43, 64)})
SHAPES["d21_c16_k5_ff"] = _shape(21, 5, residual=False)
SHAPES["d21_k10_no_context"] = _shape(21, 10, ce=None)


def build(cfg):
    import torch
    from nflows_amd.nn.nde import MixtureOfGaussiansMADE
    torch.manual_seed(0)
    made = MixtureOfGaussiansMADE(custom_initialization=True, **cfg)
    with torch.no_grad():   # off the near-zero initialisation (times do not depend on the values)
        for name, p in made.named_parameters():
            if "linear_layers.1" in name:
                p.mul_(100.0)
    return made.to(DEV).eval()


def child(args):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    from maf_sample_time import adaptive_timed
    from nflows_amd import ops
    from nflows_amd.nn.nde import MixtureOfGaussiansMADE as M
    cfg = SHAPES[args.case]
    made = build(cfg)
    rule, floor = tuple(M._DENSITY_KERNEL_LOSES), M._DENSITY_KERNEL_MIN_ROWS
    M._DENSITY_KERNEL_LOSES, M._DENSITY_KERNEL_MIN_ROWS = (), 1   # time the kernel itself at every size
    D, K, ce = cfg["features"], cfg["num_mixture_components"], cfg["context_features"]
    for rows in args.rows:
        g = torch.Generator(DEV).manual_seed(rows)
        x = torch.randn(rows, D, device=DEV, generator=g)
        ctx = None if ce is None else torch.randn(rows, ce, device=DEV, generator=g)

        def call():
            with torch.no_grad():
                return made.log_prob(x, context=ctx)
        entry = {"shape": args.case, "rows": rows, **cfg,
                 "dispatch_takes_kernel": rows >= floor and not any(D > f and K > k and rows < r for f, k, r in rule)}
        results = {"kernel": [], "parts": []}
        values = {}
        for _ in range(2):   # the two paths alternate
            for name, on in (("kernel", True), ("parts", False)):
                M._use_density_kernel = on
                values[name] = call()
                if on:
                    entry["kernel_label"] = ops.last_layer_kernel()
                results[name].append(adaptive_timed(call, args.budget))
        M._use_density_kernel = True
        entry.update(results)
        entry["finite"] = bool(torch.isfinite(values["kernel"]).all() and torch.isfinite(values["parts"]).all())
        entry["max_difference"] = float((values["kernel"] - values["parts"]).abs().max())
        for label, key in (("speedup", "median_us"), ("speedup_back_to_back", "back_to_back_median_us")):
            one = statistics.median(r[key] for r in results["kernel"])
            many = statistics.median(r[key] for r in results["parts"])
            entry[label] = many / one
        entry["kernel_not_slower"] = bool(
            min(r["median_us"] for r in results["kernel"]) <= max(r["max_us"] for r in results["parts"])
            and min(r["back_to_back_median_us"] for r in results["kernel"])
            <= max(r["back_to_back_max_us"] for r in results["parts"]))
        print("RESULT " + json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget", type=float, default=2.0, help="seconds of measurement per path, row count and alternation")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1024,16384,65536,262144")
    ap.add_argument("--case", default=None, help="internal: one shape in a child process")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    args.rows = [int(r) for r in args.rows.split(",")]
    if args.case:
        return child(args)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from maf_sample_time import DEVICE_ERROR
    from nonlin_time import smi
    result = {"clocks_power_before": smi(), "cases": []}
    for name in args.shapes.split(","):   # every shape in a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--budget", str(args.budget),
               "--rows", ",".join(str(r) for r in args.rows)]
        stderr = ""
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            stderr = run.stderr
            entries = [json.loads(ln[7:]) for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            failed = run.returncode
        except subprocess.TimeoutExpired:
            entries, failed = [], "timeout"
        for entry in entries:
            print(json.dumps({k: entry[k] for k in ("shape", "rows", "speedup", "speedup_back_to_back", "kernel_not_slower")}),
                  flush=True)
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
