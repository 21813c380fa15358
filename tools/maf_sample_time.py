#!/usr/bin/env python3
"""HIP-event time of sampling from masked autoregressive affine flows -- `flow._transform.inverse` on normal noise, what
`Flow.sample` runs -- with one persistent kernel per layer (K23, NFA_K23) against the same flow with the switch off: the
column-wise host loop, per feature and layer the MADE's hidden GEMMs, an addmm, K2b and a rank-1 update, which is what a
user had before.

    python tools/maf_sample_time.py [--out profiles/maf_sample_time.json] [--tree PATH] [--instances FILE]
    python tools/maf_sample_time.py --compile-instances FILE     # no device: registers / scratch of the kernel instances

Shapes and row counts are tools/maf_time.py's (K22's table), the final layers scaled by 0.5 and the blocks' second Linears by 5 so that normal noise overflows less
often (`finite` says whether it did; times do not depend on the values).  Every shape runs in a fresh child process; per row count the two paths alternate (kernel, host loop, twice each).
A call of the host loop takes up to seconds, so the counts adapt: after two warm-up calls, `reps` single calls between
event pairs and `reps` trains of three calls between one pair, `reps` chosen so that a path's measurement stays within
`--budget` seconds (at least 2).  Figures are medians with min / max = the spread.  `pack_ms_per_layer`: host time of the
first call's packing (schedule and context weights) per layer.  `--tree`: another checkout of the package (the parent
commit's) timed on the same rows with this build's library, to confirm that NFA_K23=0 is that path."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
DEVICE_ERROR = re.compile(r"HIP error|hipError|HSA_STATUS|illegal memory access|device-side assert|Memory access fault", re.I)


def adaptive_timed(fn, budget, max_reps=20, train=3):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    reps = int(max(2, min(max_reps, budget / max(one * (1 + train), 1e-6))))
    single, trains = [], []
    for n, sink in ((1, single), (train, trains)):
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            sink.append(e0.elapsed_time(e1) * 1e3 / n)
    return {"median_us": statistics.median(single), "min_us": min(single), "max_us": max(single),
            "back_to_back_median_us": statistics.median(trains), "back_to_back_min_us": min(trains),
            "back_to_back_max_us": max(trains), "reps": reps, "calls_per_train": train}


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    import maf_time
    from nflows_amd import ops
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform as MAF
    cfg = maf_time.SHAPES[args.case]
    flow = maf_time.build(cfg)
    with torch.no_grad():   # (maf_time scales the final layers by 2 and the blocks' second Linears by 100 for the density pass;
        for name, p in flow.named_parameters():   # normal noise through sixteen such layers overflows: 0.5 and 5 here)
            if "final_layer" in name:
                p.mul_(0.25)
            elif "linear_layers.1" in name:
                p.mul_(0.05)
    has_switch = hasattr(MAF, "fuse_sequential_inverse")
    row_limit = getattr(MAF, "_INVERSE_KERNEL_ROW_LIMIT", None)
    if row_limit is not None:   # time the kernel itself at every size: the dispatch's size rule is read off these figures
        MAF._INVERSE_KERNEL_ROW_LIMIT = (0, 0)
    layers = [t for t in flow._transform._transforms if isinstance(t, MAF)]
    static = {}
    if has_switch:
        t0 = time.perf_counter()
        plans = [t._inverse_kernel_plan(t._inverse_kernel_net()) for t in layers]
        static["pack_ms_per_layer"] = (time.perf_counter() - t0) * 1e3 / len(layers)
        schedule = plans[0][0]
        if schedule is not None:
            vectors = len(ops.made_context_layers(layers[0].autoregressive_net))
            state = ops.made_state_bytes(cfg["features"], cfg["hidden_features"], schedule[2][0], vectors)
            static.update(blocks=int(schedule[1].numel()) - 2, max_block_bytes=schedule[2][7] * 4, state_bytes=state,
                          lds_bytes=state + 2 * schedule[2][7] * 4, schedule_bytes=int(schedule[0].numel()) * 4)
    for rows in args.rows:
        g = torch.Generator(DEV).manual_seed(rows)
        z = torch.randn(rows, cfg["features"], device=DEV, generator=g)
        ce = cfg.get("context_features")
        ctx = None if ce is None else torch.randn(rows, ce, device=DEV, generator=g)

        def call():
            with torch.no_grad():
                return flow._transform.inverse(z, context=ctx)
        entry = {"shape": args.case, "rows": rows, **cfg, **static}
        if row_limit is not None:
            entry["dispatch_takes_kernel"] = not (cfg["features"] <= row_limit[0] and rows > row_limit[1])
        if not has_switch:   # another tree without K23: its only path
            entry["host_loop"] = [adaptive_timed(call, args.budget)]
            print("RESULT " + json.dumps(entry), flush=True)
            continue
        results = {"kernel": [], "host_loop": []}
        values = {}
        for _ in range(2):   # the two paths alternate
            for name, on in (("kernel", True), ("host_loop", False)):
                MAF.fuse_sequential_inverse = on
                values[name] = call()
                if on:
                    entry["kernel_label"] = ops.last_layer_kernel()
                results[name].append(adaptive_timed(call, args.budget))
        MAF.fuse_sequential_inverse = True
        entry.update(results)
        entry["finite"] = bool(torch.isfinite(values["kernel"][0]).all() and torch.isfinite(values["host_loop"][0]).all())
        entry["max_abs_difference"] = float((values["kernel"][0] - values["host_loop"][0]).abs().max())
        entry["max_abs_sample"] = float(values["host_loop"][0].abs().max())
        for label, key in (("speedup", "median_us"), ("speedup_back_to_back", "back_to_back_median_us")):
            one = statistics.median(r[key] for r in results["kernel"])
            many = statistics.median(r[key] for r in results["host_loop"])
            entry[label] = many / one
        entry["kernel_not_slower"] = bool(
            min(r["median_us"] for r in results["kernel"]) <= max(r["max_us"] for r in results["host_loop"])
            and min(r["back_to_back_median_us"] for r in results["kernel"])
            <= max(r["back_to_back_max_us"] for r in results["host_loop"]))
        print("RESULT " + json.dumps(entry), flush=True)


def compile_instances(path):
    """VGPRs / AGPRs / SGPRs / scratch of every instance of csrc/made_inverse.hip, from the compiler's own remarks."""
    src = os.path.join(os.path.dirname(HERE), "nflows_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt", "-I" + os.path.join(os.path.dirname(HERE), "include"),
           "-I" + src, "--cuda-device-only", "-c", os.path.join(src, "made_inverse.hip"), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    found, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
            found[name] = {}
        m = re.search(r"(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            found[name][m.group(1)] = int(m.group(2))
    with open(path, "w") as fh:
        json.dump(found, fh, indent=1)
    print(json.dumps(found, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget", type=float, default=4.0, help="seconds of measurement per path, row count and alternation")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=None, help="time the package in this other checkout (no switch needed)")
    ap.add_argument("--instances", default=None, help="a file of --compile-instances to carry along in --out")
    ap.add_argument("--compile-instances", default=None)
    ap.add_argument("--rows", default="1024,16384,262144")
    ap.add_argument("--case", default=None, help="internal: one shape in a child process")
    sys.path.insert(0, HERE)
    import maf_time
    ap.add_argument("--shapes", default=",".join(maf_time.SHAPES))
    args = ap.parse_args()
    args.rows = [int(r) for r in args.rows.split(",")]
    if args.compile_instances:
        return compile_instances(args.compile_instances)
    if args.case:
        return child(args)
    sys.path.insert(0, os.path.dirname(HERE))
    from nonlin_time import smi
    result = {"clocks_power_before": smi(), "tree": args.tree, "cases": []}
    if args.instances:
        with open(args.instances) as fh:
            result["instances"] = json.load(fh)
    for name in args.shapes.split(","):   # every shape in a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--budget", str(args.budget),
               "--rows", ",".join(str(r) for r in args.rows)]
        if args.tree:
            cmd += ["--tree", args.tree]
        stderr = ""
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
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
