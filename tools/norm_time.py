#!/usr/bin/env python3
"""HIP-event time of K17 (BatchNorm / ActNorm) against the same class on its generic path -- the reference's sequence by
stock torch ops on the same device, which is what a user had before.  `class_takes`: the path the class
chooses by itself for the case (its dispatch rule); K17 is timed everywhere, forced where the rule says otherwise.

    python tools/norm_time.py [--out profiles/norm_time.json]

Cases: BatchNorm eval forward, eval inverse, training forward, training forward + backward (gradients with respect to the
inputs and both parameters, incoming gradients prepared outside the timed region) and ActNorm forward, at 16 384 and
262 144 rows x D = 16, 64, 128, 784.  Every case runs in a fresh child process, small sizes first.  Per case and path:
warm-up, then the median (and the min / max = the spread) of `--reps` single calls between event pairs, and of trains of
calls between one pair (see `timed`).  `traffic_floor_us`: the bytes the operation must move (eval forward / inverse and
ActNorm 2 B D 4, training forward 3 B D 4, training forward + backward 8 B D 4: x twice and y forward, g twice, x twice
and grad_x backward) at K1's measured 5.1 TB/s."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nflows_amd.transforms import ActNorm, BatchNorm  # noqa: E402

DEV = "cuda:0"
OPS = ("bn_eval_forward", "bn_eval_inverse", "bn_train_forward", "bn_train_forward_backward", "an_forward")
PASSES = {"bn_eval_forward": 2, "bn_eval_inverse": 2, "bn_train_forward": 3, "bn_train_forward_backward": 8, "an_forward": 2}


def timed(fn, reps, warmup=10, train=10):
    """`single`: one call between an event pair on an idle device, `reps` times -- the host's enqueue path is INSIDE the
    interval, so for a short kernel this is a latency as a caller sees it.  `back_to_back`: `train` calls between ONE event
    pair, per call, `reps` times -- the queue stays full, so this approaches the device time when the device is the slower
    side."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
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


def smi():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "Power" in ln][:4]
    except (OSError, subprocess.SubprocessError):
        return []


def class_takes(t, x):
    """The path the class chooses by itself for this call (its dispatch rule, transforms/normalization.py)."""
    import copy
    d = copy.copy(t)
    d._use_kernel = True
    return "k17" if d._kernel_serves(x) else "generic"


def make_call(op, batch, features, use_kernel):
    torch.manual_seed(features)
    x = torch.randn(batch, features, device=DEV) * 1.5 + 0.5
    if op == "an_forward":
        t = ActNorm(features)
        with torch.no_grad():
            t.log_scale.normal_(0.0, 0.3)
            t.shift.normal_()
            t.initialized.fill_(True)
    else:
        t = BatchNorm(features)
        with torch.no_grad():
            t.unconstrained_weight.add_(0.3 * torch.randn(features))
            t.bias.normal_()
            t.running_mean.normal_()
            t.running_var.uniform_(0.5, 2.0)
    t = t.to(DEV)
    t._use_kernel = use_kernel          # "always": K17 whatever the dispatch rule says; False: the generic path
    t.train(op.startswith("bn_train"))
    if op == "bn_train_forward_backward":
        x.requires_grad_(True)
        make_call.class_takes = class_takes(t, x)
        gy, gl = torch.randn(batch, features, device=DEV), torch.randn(batch, device=DEV)

        def call():
            x.grad = None
            for p in t.parameters():
                p.grad = None
            y, lad = t(x)
            torch.autograd.backward((y, lad), (gy, gl))
        return call
    with torch.no_grad():
        make_call.class_takes = class_takes(t, x)
    fn = t.inverse if op == "bn_eval_inverse" else t

    def call():
        with torch.no_grad():
            fn(x)
    return call


def child(args):
    op, batch, features = args.case.split(",")
    batch, features = int(batch), int(features)
    floor_us = PASSES[op] * batch * features * 4 / 5.1e12 * 1e6
    case = {"op": op, "batch": batch, "features": features, "traffic_floor_us": floor_us}
    case["k17"] = timed(make_call(op, batch, features, "always"), args.reps)
    case["class_takes"] = make_call.class_takes
    case["fraction_of_floor"] = floor_us / case["k17"]["back_to_back_median_us"]
    print("RESULT " + json.dumps(case), flush=True)
    case["generic"] = timed(make_call(op, batch, features, False), args.reps)
    case["speedup"] = case["generic"]["median_us"] / case["k17"]["median_us"]
    case["speedup_back_to_back"] = case["generic"]["back_to_back_median_us"] / case["k17"]["back_to_back_median_us"]
    # the relative condition: the kernel path is not slower than the generic one beyond the spread the runs themselves show
    case["k17_not_slower"] = bool(case["k17"]["median_us"] <= case["generic"]["max_us"]
                                  and case["k17"]["back_to_back_median_us"] <= case["generic"]["back_to_back_max_us"])
    # ... and the path the class takes by itself: K17 where that holds, the generic path (the yardstick itself) elsewhere
    case["class_not_slower"] = bool(case["k17_not_slower"] or case["class_takes"] == "generic")
    print("RESULT " + json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: one case in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    result = {"clocks_power_before": smi(), "cases": []}
    cases = ["%s,%d,%d" % (op, b, d) for b in (16384, 262144) for d in (16, 64, 128, 784) for op in OPS]
    for name in cases:   # small sizes first, every case in a fresh process
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=120)
            lines = [ln[7:] for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            entry = json.loads(lines[-1]) if lines else {"case": name}
            if run.returncode != 0:
                entry["child_exit"] = run.returncode
                entry["child_stderr"] = run.stderr.strip().splitlines()[-1][:200] if run.stderr.strip() else ""
        except subprocess.TimeoutExpired:
            entry = {"case": name, "child_exit": "timeout"}
        print(json.dumps(entry), flush=True)
        result["cases"].append(entry)
        if entry.get("child_exit") not in (None, 1):   # anything but a Python error: start nothing more on the device
            break
    result["clocks_power_after"] = smi()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
