#!/usr/bin/env python3
"""HIP-event time of `nn.nde.MixtureOfGaussiansMADE.sample(1, context)` -- what `distributions.MADEMoG.sample` and every
Flow with a MADEMoG base run -- on one persistent kernel (K30, NFA_K30) against the same module with the switch off: the
reference's host loop of D whole MADE passes with a Categorical draw, two gathers and a randn per feature, which is what a
user had before.

    python tools/mog_sample_time.py [--out profiles/mog_sample_time.json]

Shapes: hidden 128, two residual blocks; see SHAPES.  Every shape runs in a fresh child process; per row count the two
paths alternate (kernel, host loop, twice each).  The counts adapt as in tools/maf_sample_time.py (`adaptive_timed`):
figures are medians with min / max = the spread.  The kernel is timed at every size, whatever the class's size rule says
(`dispatch_takes_kernel` records what the rule does there): the rule is read off these figures."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def _shape(features, ce, components):
    return dict(features=features, context_features=ce, num_mixture_components=components, hidden_features=128, num_blocks=2)


SHAPES = {}
for _k in (5, 10):
    SHAPES.update({
        "d8_c8_k%d" % _k: _shape(8, 8, _k),
        "d21_c16_k%d" % _k: _shape(21, 16, _k),
        "d43_c16_k%d" % _k: _shape(43, 16, _k),
        "d64_c32_k%d" % _k: _shape(64, 32, _k),
    })


def build(cfg):
    import torch
    from nflows_amd.nn.nde import MixtureOfGaussiansMADE
    torch.manual_seed(0)
    made = MixtureOfGaussiansMADE(custom_initialization=False, **cfg)
    with torch.no_grad():   # off the near-zero initialisation (times do not depend on the values)
        for name, p in made.named_parameters():
            if "final_layer" in name:
                p.mul_(3.0)
            elif "linear_layers.1" in name:
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
    rule = tuple(M._SAMPLE_KERNEL_LOSES)
    M._SAMPLE_KERNEL_LOSES = ()   # time the kernel itself at every size
    t0 = time.perf_counter()
    schedule, _ = made._sample_kernel_plan()
    static = {"pack_ms": (time.perf_counter() - t0) * 1e3}
    if schedule is not None:
        state = ops.made_state_bytes(cfg["features"], cfg["hidden_features"], schedule[2][0], len(ops.made_context_layers(made)))
        static.update(blocks=int(schedule[1].numel()) - 2, max_block_bytes=schedule[2][7] * 4, state_bytes=state,
                      lds_bytes=state + 2 * schedule[2][7] * 4)
    for rows in args.rows:
        ctx = torch.randn(rows, cfg["context_features"], device=DEV, generator=torch.Generator(DEV).manual_seed(rows))

        def call():
            return made.sample(1, context=ctx)
        entry = {"shape": args.case, "rows": rows, **cfg, **static,
                 "dispatch_takes_kernel": not any(cfg["features"] <= f and rows > r for f, r in rule)}
        results = {"kernel": [], "host_loop": []}
        values = {}
        for _ in range(2):   # the two paths alternate
            for name, on in (("kernel", True), ("host_loop", False)):
                M._use_sample_kernel = on
                if on:
                    real, seen = ops.made_mog_sample, []

                    def labelled(*a, **kw):
                        r = real(*a, **kw)
                        seen.append(ops.last_layer_kernel() if r is not None else None)
                        return r
                    ops.made_mog_sample = labelled
                    try:
                        values[name] = call()
                    finally:
                        ops.made_mog_sample = real
                    entry["kernel_label"], entry["kernel_launches"] = (seen[0] if seen else None), len(seen)
                else:
                    values[name] = call()
                results[name].append(adaptive_timed(call, args.budget))
        M._use_sample_kernel = True
        entry.update(results)
        entry["finite"] = bool(torch.isfinite(values["kernel"]).all() and torch.isfinite(values["host_loop"]).all())
        # (the two paths draw differently: the distributions agree, not the samples -- first two moments per feature)
        entry["max_mean_difference"] = float((values["kernel"].mean(dim=(0, 1)) - values["host_loop"].mean(dim=(0, 1))).abs().max())
        entry["max_std_ratio"] = float((values["kernel"].std(dim=(0, 1)) / values["host_loop"].std(dim=(0, 1))).max())
        for label, key in (("speedup", "median_us"), ("speedup_back_to_back", "back_to_back_median_us")):
            one = statistics.median(r[key] for r in results["kernel"])
            many = statistics.median(r[key] for r in results["host_loop"])
            entry[label] = many / one
        entry["kernel_not_slower"] = bool(
            min(r["median_us"] for r in results["kernel"]) <= max(r["max_us"] for r in results["host_loop"])
            and min(r["back_to_back_median_us"] for r in results["kernel"])
            <= max(r["back_to_back_max_us"] for r in results["host_loop"]))
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
