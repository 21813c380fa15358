#!/usr/bin/env python3
"""HIP-event time of sampling from conditional autoregressive spline flows -- `flow._transform.inverse` on normal noise with
a context, what `Flow.sample(n, context=...)` runs -- with one persistent kernel per layer (K28, NFA_K28) against the same
flow with the switch off: the column-wise host loop, per feature and layer the MADE's hidden GEMMs, an addmm, a one-column
K1 launch and a rank-1 update, which is what a user had before.

    python tools/ar_spline_sample_time.py [--out profiles/ar_spline_sample_time.json] [--tree PATH --tree-shapes A,B]

Shapes: hidden 128, two residual blocks, reversing permutations, linear tails; see SHAPES.  Every shape runs in a fresh
child process; per row count the two paths alternate (kernel, host loop, twice each).  The counts adapt as in
tools/maf_sample_time.py (`adaptive_timed`): figures are medians with min / max = the spread.  `--tree`: another checkout
of the package (the parent commit's) timed afterwards on the same rows of `--tree-shapes` with this build's library
(`parent_tree_host_loop` in the result), to confirm that NFA_K28=0 is that path."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"


def _shape(layers, features, ce, bins):
    return dict(num_layers=layers, features=features, context_features=ce, num_bins=bins, hidden_features=128, num_blocks=2)


SHAPES = {}
for _bins in (8, 10):
    SHAPES.update({
        "l5_d8_c8_k%d" % _bins: _shape(5, 8, 8, _bins),
        "l8_d21_c16_k%d" % _bins: _shape(8, 21, 16, _bins),
        "l10_d43_c16_k%d" % _bins: _shape(10, 43, 16, _bins),
        "l16_d64_c32_k%d" % _bins: _shape(16, 64, 32, _bins),
    })
SHAPES["l5_d6_k5"] = _shape(5, 6, None, 5)   # unconditional: K12 answers unsupported (continuation blocks), and 5 bins
SHAPES["l8_d16_c16_k8"] = _shape(8, 16, 16, 8)   # between the 8- and the 21-feature shapes: where the size rule ends


def build(cfg):
    import torch
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.transforms import (CompositeTransform, MaskedPiecewiseRationalQuadraticAutoregressiveTransform,
                                       ReversePermutation)
    torch.manual_seed(0)
    layers = []
    for _ in range(cfg["num_layers"]):
        layers.append(ReversePermutation(cfg["features"]))
        layers.append(MaskedPiecewiseRationalQuadraticAutoregressiveTransform(
            features=cfg["features"], hidden_features=cfg["hidden_features"], context_features=cfg["context_features"],
            num_bins=cfg["num_bins"], tails="linear", tail_bound=3.0, num_blocks=cfg["num_blocks"]))
    flow = Flow(CompositeTransform(layers), StandardNormal([cfg["features"]]))
    with torch.no_grad():   # off the near-identity initialisation (times do not depend on the values)
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.mul_(3.0)
            elif "linear_layers.1" in name:
                p.mul_(100.0)
    return flow.to(DEV).eval()


def child(args):
    if not args.in_tree:
        args.tree = None
    if args.tree:
        os.environ.setdefault("NFLOWS_AMD_LIB", os.path.join(os.path.dirname(HERE), "nflows_amd", "libnflows_amd.so"))
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    from maf_sample_time import adaptive_timed
    from nflows_amd import ops
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform as AR
    cfg = SHAPES[args.case]
    flow = build(cfg)
    has_switch = hasattr(AR, "fuse_sequential_inverse_ctx")
    row_limit = getattr(AR, "_SEQUENTIAL_CTX_ROW_LIMIT", None)
    if has_switch:   # time the kernel itself at every size: the dispatch's size rule is read off these figures
        AR._SEQUENTIAL_CTX_ROW_LIMIT = None
    layers = [t for t in flow._transform._transforms if isinstance(t, AR)]
    static = {}
    if has_switch:
        net = layers[0].autoregressive_net
        steps = min(cfg["features"], layers[0]._sequential_steps())
        t0 = time.perf_counter()
        plans = [t._sequential_ctx_plan(t.autoregressive_net, steps) for t in layers]
        static["pack_ms_per_layer"] = (time.perf_counter() - t0) * 1e3 / len(layers)
        schedule = plans[0][0]
        if schedule is not None:
            state = ops.made_state_bytes(steps, cfg["hidden_features"], schedule[2][0], len(ops.made_context_layers(net)))
            static.update(sequential_steps=steps, blocks=int(schedule[1].numel()) - 2, max_block_bytes=schedule[2][7] * 4,
                          state_bytes=state, lds_bytes=state + 2 * schedule[2][7] * 4)
    for rows in args.rows:
        g = torch.Generator(DEV).manual_seed(rows)
        z = torch.randn(rows, cfg["features"], device=DEV, generator=g)
        ce = cfg["context_features"]
        ctx = None if ce is None else torch.randn(rows, ce, device=DEV, generator=g)

        def call():
            with torch.no_grad():
                return flow._transform.inverse(z, context=ctx)
        entry = {"shape": args.case, "rows": rows, **cfg, **static}
        if has_switch:
            entry["dispatch_takes_kernel"] = row_limit is None or not (cfg["features"] <= row_limit[0] and rows > row_limit[1])
        if not has_switch:   # another tree without K28: its only path
            entry["host_loop"] = [adaptive_timed(call, args.budget)]
            print("RESULT " + json.dumps(entry), flush=True)
            continue
        results = {"kernel": [], "host_loop": []}
        values = {}
        for _ in range(2):   # the two paths alternate
            for name, on in (("kernel", True), ("host_loop", False)):
                AR.fuse_sequential_inverse_ctx = on
                if on:   # (the label right behind K28's launch: the tail's kernel follows it)
                    real, seen = ops.made_rqs_inverse_ctx, []

                    def labelled(*a, **kw):
                        r = real(*a, **kw)
                        seen.append(ops.last_layer_kernel() if r is not None else None)
                        return r
                    ops.made_rqs_inverse_ctx = labelled
                    try:
                        values[name] = call()
                    finally:
                        ops.made_rqs_inverse_ctx = real
                    entry["kernel_label"], entry["kernel_launches"] = (seen[0] if seen else None), len(seen)
                else:
                    values[name] = call()
                results[name].append(adaptive_timed(call, args.budget))
        AR.fuse_sequential_inverse_ctx = True
        entry.update(results)
        entry["finite"] = bool(torch.isfinite(values["kernel"][0]).all() and torch.isfinite(values["host_loop"][0]).all())
        entry["max_abs_difference"] = float((values["kernel"][0] - values["host_loop"][0]).abs().max())
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
    ap.add_argument("--tree", default=None, help="time the package in this other checkout as well (no switch needed)")
    ap.add_argument("--tree-shapes", default="l5_d8_c8_k8,l8_d21_c16_k10")
    ap.add_argument("--in-tree", action="store_true", help="internal: the child imports the package from --tree")
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
    result = {"clocks_power_before": smi(), "tree": args.tree, "cases": [], "parent_tree_host_loop": []}
    jobs = [(name, False) for name in args.shapes.split(",")]
    if args.tree:
        jobs += [(name, True) for name in args.tree_shapes.split(",")]
    for name, in_tree in jobs:   # every shape in a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--budget", str(args.budget),
               "--rows", ",".join(str(r) for r in args.rows)]
        if in_tree:
            cmd += ["--tree", args.tree, "--in-tree"]
        stderr = ""
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            stderr = run.stderr
            entries = [json.loads(ln[7:]) for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            failed = run.returncode
        except subprocess.TimeoutExpired:
            entries, failed = [], "timeout"
        for entry in entries:
            print(json.dumps({k: entry[k] for k in ("shape", "rows", "speedup", "speedup_back_to_back", "kernel_not_slower")
                              if k in entry} if not in_tree else
                             {"parent_tree": entry["shape"], "rows": entry["rows"],
                              "median_us": entry["host_loop"][0]["median_us"]}), flush=True)
        result["parent_tree_host_loop" if in_tree else "cases"] += entries
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
