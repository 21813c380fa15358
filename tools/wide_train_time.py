#!/usr/bin/env python3
"""HIP-event time of a training step of 32-layer spline flows whose ResidualNet conditioners are 192 or 256 units wide: K33
(csrc/resnet_train_wide.hip through autograd.ResidualNetWide) against the same modules with `fuse_wide_training = False`
(NFA_K33=0) -- the parent commit's path: the eager conditioner modules under autograd.

    python tools/wide_train_time.py [--out profiles/wide_train_time.json] [--shapes h256_d64_k8,...] [--reps 5]

Per shape (hidden width 192 / 256; 16 / 64 features; 8 / 10 bins; two residual blocks) and row count (1 024, 16 384,
65 536, 262 144) the step is zero_grad + `-flow.log_prob(x).mean()` + backward.  Every shape runs in a fresh child process;
per row count the two paths alternate (twice each, a session each time), and every figure is the median (with min / max =
the spread) of `--reps` single steps between event pairs.  `k33_faster_beyond_spread`: K33's slower session is faster than
the old path's faster one.  `max_abs_gradient_difference`: the two paths' gradients on the timed rows, beside the largest
magnitude there.  `mfma_share`: the multiply-adds of the conditioners' GEMMs forward and backward (input and weight
gradients: 3 x the forward count, unpadded) x 6 products x 2 over K33's step time, against the 2.5 PFLOP/s of the dense
16-bit matrix pipe -- a whole-step rate, not a kernel's.  `--graph`: one captured `GraphedTrainStep` with Adam per path."""
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
SHAPES = {"h%d_d%d_k%d" % (h, d, k): dict(hidden_features=h, features=d, num_bins=k, num_blocks=2)
          for h in (192, 256) for d in (16, 64) for k in (8, 10)}
ROWS = (1024, 16384, 65536, 262144)
LAYERS = 32
PEAK = 2.5e15


def build(cfg):
    import torch
    from nflows_amd import configs
    flow = configs.rq_nsf_flow(num_layers=LAYERS, tail_bound=3.0, seed=0, **cfg)
    with torch.no_grad():   # off the near-identity initialisation, as __graft_entry__.smoke
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.mul_(4.0)
            elif "linear_layers.1" in name:
                p.mul_(30.0)
    return flow.to(DEV).train()


def layer_macs(cfg):
    d, h, k = cfg["features"], cfg["hidden_features"], cfg["num_bins"]
    dt = (d + 1) // 2
    return (d - dt) * h + 2 * cfg["num_blocks"] * h * h + h * dt * (3 * k - 1)


def single_steps(step, reps, warmup=2):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times), "reps": reps}


def child(args):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch
    from nflows_amd.graphs import GraphedTrainStep
    from nflows_amd.nn.nets.resnet import ResidualNet
    cfg = SHAPES[args.case]
    ResidualNet.fuse_wide_training_min_rows = 0   # the kernels themselves, whatever the size rule
    flow = build(cfg)
    params = list(flow.parameters())
    for rows in ((args.graph_rows,) if args.graph else ROWS):
        x = 1.5 * torch.randn(rows, cfg["features"], device=DEV, generator=torch.Generator(DEV).manual_seed(rows))
        entry = {"shape": args.case, "rows": rows, "num_layers": LAYERS, "graph": bool(args.graph), **cfg}
        results, grads = {"k33": [], "old_path": []}, {}
        for _ in range(1 if args.graph else 2):   # the two paths alternate
            for name, on in (("k33", True), ("old_path", False)):
                ResidualNet.fuse_wide_training = on
                if args.graph:
                    model = build(cfg)
                    opt = torch.optim.Adam(model.parameters(), lr=1e-5, capturable=True)
                    graphed = GraphedTrainStep(model, opt, x)

                    def step():
                        graphed(x)
                else:
                    def step():
                        for p in params:
                            p.grad = None
                        (-flow.log_prob(x).mean()).backward()
                results[name].append(single_steps(step, args.reps))
                if not args.graph:
                    grads[name] = torch.cat([p.grad.reshape(-1) for p in params])
        ResidualNet.fuse_wide_training = True
        entry.update(results)
        if grads:
            entry["max_abs_gradient_difference"] = float((grads["k33"] - grads["old_path"]).abs().max())
            entry["max_abs_gradient"] = float(grads["old_path"].abs().max())
        new = statistics.median(r["median_us"] for r in results["k33"])
        entry["speedup"] = statistics.median(r["median_us"] for r in results["old_path"]) / new
        entry["k33_faster_beyond_spread"] = bool(max(r["median_us"] for r in results["k33"])
                                                 < min(r["median_us"] for r in results["old_path"]))
        entry["mfma_share"] = rows * LAYERS * 3 * layer_macs(cfg) * 12 / (new * 1e-6) / PEAK
        print("RESULT " + json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--graph", action="store_true", help="one captured GraphedTrainStep with Adam per path and shape")
    ap.add_argument("--graph-rows", type=int, default=16384)
    ap.add_argument("--case", default=None, help="internal: one shape in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    result = {"cases": []}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)
    for name in args.shapes.split(","):   # every shape in a fresh process
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps),
               "--graph-rows", str(args.graph_rows)] + (["--graph"] if args.graph else [])
        stderr = ""
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            stderr = run.stderr
            entries = [json.loads(ln[7:]) for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            failed = run.returncode
        except subprocess.TimeoutExpired:
            entries, failed = [], "timeout"
        for entry in entries:
            print(json.dumps({k: entry.get(k) for k in ("shape", "rows", "graph", "speedup", "k33_faster_beyond_spread",
                                                        "mfma_share", "max_abs_gradient_difference")}), flush=True)
        result["cases"] += entries
        if failed:
            result["cases"].append({"shape": name, "child_exit": failed,
                                    "child_stderr": stderr.strip().splitlines()[-1][:200] if stderr.strip() else ""})
            print(json.dumps(result["cases"][-1]), flush=True)
            # a device fault reaches Python as a RuntimeError, exit status 1 like any other: go on only after an exit of 1
            # whose output names no HIP / HSA error, and start nothing more on the device otherwise
            if failed != 1 or DEVICE_ERROR.search(stderr):
                save()
                break
        save()   # (kept up to date shape by shape: a run cut short leaves what it measured)
    save()
    if any("child_exit" in c for c in result["cases"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
