#!/usr/bin/env python3
"""HIP-event time of affine coupling layers (RealNVP) whose ResidualNet conditioner is 192 or 256 units wide: K37 (one launch
per layer, csrc/affine_resnet_wide_kernel.hpp) against the same modules with `fuse_wide_conditioner = False` (NFA_K37=0) -- the
parent commit's path: the conditioner's stock GEMMs and elementwise launches, then K2.

    python tools/wide_affine_time.py [--out profiles/wide_affine_time.json] [--shapes h256_d64,...] [--reps 5]

Per shape (hidden width 192 / 256; 16 / 64 features; two residual blocks): `flow._transform` of ONE layer and `Flow.log_prob`
of a SimpleRealNVP-style stack of 6 layers on flipping masks, at 1 024, 16 384, 65 536 and 262 144 rows.  Every shape runs in
a fresh child process; per row count and call the two paths alternate (twice each), each run with its own warm-up, and every
figure is the median (with min / max = the spread) of `--reps` single calls between event pairs and of trains of calls
between one pair (`timed`, tools/nonlin_time.py).
`k37_slower_session_beats_old_faster`: the size rule's question -- K37's slower session against the old path's faster one,
single calls and trains."""
import argparse
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
DEVICE_ERROR = re.compile(r"HIP error|hipError|HSA_STATUS|illegal memory access|device-side assert|Memory access fault", re.I)
SHAPES = {"h%d_d%d" % (h, d): dict(hidden_features=h, features=d, num_blocks_per_layer=2) for h in (192, 256) for d in (16, 64)}
ROWS = (1024, 16384, 65536, 262144)
LAYERS = 6


def build(cfg, num_layers):
    import torch
    from nflows_amd import configs
    flow = configs.simple_realnvp_flow(num_layers=num_layers, seed=0, **cfg)
    with torch.no_grad():   # (off the near-identity initialisation, as tests/test_gpu_wide_affine.py)
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.mul_(4.0)
            elif "linear_layers.1" in name:
                p.mul_(30.0)
    return flow.to(DEV).eval()


def child(args):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import torch
    from nonlin_time import timed
    from nflows_amd import ops
    from nflows_amd.transforms import AffineCouplingTransform as Affine
    cfg = SHAPES[args.case]
    Affine.fuse_wide_min_rows = 0   # the kernel itself, whatever the size rule
    flows = {1: build(cfg, 1), LAYERS: build(cfg, LAYERS)}
    for rows in ROWS:
        g = torch.Generator(DEV).manual_seed(rows)
        x = 1.2 * torch.randn(rows, cfg["features"], device=DEV, generator=g)

        def transform():
            with torch.no_grad():
                return flows[1]._transform(x)[1]

        def log_prob():
            with torch.no_grad():
                return flows[LAYERS].log_prob(x)
        for what, layers, call in (("transform", 1, transform), ("log_prob", LAYERS, log_prob)):
            entry = {"shape": args.case, "call": what, "rows": rows, "num_layers": layers, **cfg}
            results, values = {"k37": [], "old_path": []}, {}
            for _ in range(2):   # the two paths alternate
                for name, on in (("k37", True), ("old_path", False)):
                    Affine.fuse_wide_conditioner = on
                    values[name] = call()
                    if on:
                        entry["kernel"] = ops.last_layer_kernel()
                    results[name].append(timed(call, args.reps, warmup=3, train=3))
            Affine.fuse_wide_conditioner = True
            entry.update(results)
            entry["max_abs_difference"] = float((values["k37"] - values["old_path"]).abs().max())
            entry["max_abs_value"] = float(values["old_path"].abs().max())
            for label, key in (("speedup", "median_us"), ("speedup_back_to_back", "back_to_back_median_us")):
                # K37's slower session against the old path's faster one
                entry[label] = min(r[key] for r in results["old_path"]) / max(r[key] for r in results["k37"])
            entry["k37_slower_session_beats_old_faster"] = bool(entry["speedup"] > 1.0 and entry["speedup_back_to_back"] > 1.0)
            print("RESULT " + json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--case", default=None, help="internal: one shape in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from nonlin_time import smi
    result = {"clocks_power_before": smi(), "cases": []}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)
    for name in args.shapes.split(","):   # every shape in a fresh process
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
                                                    "k37_slower_session_beats_old_faster", "max_abs_difference")}), flush=True)
        result["cases"] += entries
        if failed:
            result["cases"].append({"shape": name, "child_exit": failed,
                                    "child_stderr": stderr.strip().splitlines()[-1][:200] if stderr.strip() else ""})
            print(json.dumps(result["cases"][-1]), flush=True)
            # a device fault, a signal and a time limit end the run: go on only after an exit of 1 whose output names no
            # HIP / HSA error, and start nothing more on the device otherwise
            if failed != 1 or DEVICE_ERROR.search(stderr):
                save()
                break
        save()   # (kept up to date shape by shape: a run cut short leaves what it measured)
    result["clocks_power_after"] = smi()
    save()
    if any("child_exit" in c for c in result["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
