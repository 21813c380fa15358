#!/usr/bin/env python3
"""HIP-event time of K18 (the elementwise nonlinearity transforms) against the same class on its generic path -- the
reference's sequence by stock torch ops on the same device, which is what a user had before.  The
generic path evaluates float32 inputs in float64 (the stock float32 functions miss the parity rule); `stock_f32` is the same
sequence in plain float32, recorded beside it so that nobody takes the float64 passes for the price of stock ops.
`class_takes`: the path the class chooses by itself for the case (its dispatch rule); K18 is timed everywhere, forced where
the rule says otherwise.

    python tools/nonlin_time.py [--out profiles/nonlin_time.json]

Cases: Sigmoid forward, Logit forward, Tanh forward and Sigmoid forward + backward (learnable temperature; gradients with
respect to the inputs and the temperature, incoming gradients prepared outside the timed region) at 16 384 x 64,
262 144 x 64, 262 144 x 784 and 256 x 3 x 32 x 32.  Every case runs in a fresh child process, small sizes first.  Per case
and path: warm-up, then the median (and the min / max = the spread) of `--reps` single calls between event pairs, and of
trains of calls between one pair (see `timed`).  `traffic_floor_us`: the bytes the operation must move (forward 2 B N 4;
forward + backward 5 B N 4: x and y forward, x, g and grad_x backward) at K1's measured 5.1 TB/s."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nflows_amd.transforms import Logit, Sigmoid, Tanh  # noqa: E402

DEV = "cuda:0"
OPS = ("sigmoid_forward", "logit_forward", "tanh_forward", "sigmoid_forward_backward")
PASSES = {"sigmoid_forward": 2, "logit_forward": 2, "tanh_forward": 2, "sigmoid_forward_backward": 5}
DEVICE_ERROR = re.compile(r"HIP error|hipError|HSA_STATUS|illegal memory access|device-side assert|Memory access fault", re.I)
SHAPES = ((16384, 64), (262144, 64), (262144, 784), (256, 3, 32, 32))


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


def make_call(op, shape, use_kernel, wide=True):
    torch.manual_seed(len(shape))
    x = torch.randn(*shape, device=DEV) * 1.5
    if op == "logit_forward":
        x = torch.rand(*shape, device=DEV) * 0.98 + 0.01
        t = Logit()
        core = t._transform
    elif op == "tanh_forward":
        t = core = Tanh()
    else:
        t = core = Sigmoid(temperature=1.5, learn_temperature=(op == "sigmoid_forward_backward"))
    t = t.to(DEV)
    core._use_kernel = True
    if op == "sigmoid_forward_backward":
        x.requires_grad_(True)
    with torch.set_grad_enabled(op == "sigmoid_forward_backward"):
        make_call.class_takes = "k18" if core._kernel_serves(x) else "generic"
    core._use_kernel = use_kernel       # "always": K18 whatever the dispatch rule says; False: the generic path
    core._generic_wide = wide           # False: the generic path's sequence in plain float32 (misses the parity rule)
    if op == "sigmoid_forward_backward":
        gy, gl = torch.randn(*shape, device=DEV), torch.randn(shape[0], device=DEV)

        def call():
            x.grad = None
            core.temperature.grad = None
            y, lad = t(x)
            torch.autograd.backward((y, lad), (gy, gl))
        return call

    def call():
        with torch.no_grad():
            t(x)
    return call


def child(args):
    op, dims = args.case.split(",", 1)
    shape = tuple(int(d) for d in dims.split("x"))
    elements = 1
    for d in shape:
        elements *= d
    floor_us = PASSES[op] * elements * 4 / 5.1e12 * 1e6
    case = {"op": op, "shape": list(shape), "traffic_floor_us": floor_us}
    case["k18"] = timed(make_call(op, shape, "always"), args.reps)
    case["class_takes"] = make_call.class_takes
    case["fraction_of_floor"] = floor_us / case["k18"]["back_to_back_median_us"]
    print("RESULT " + json.dumps(case), flush=True)
    case["generic"] = timed(make_call(op, shape, False), args.reps)
    case["speedup"] = case["generic"]["median_us"] / case["k18"]["median_us"]
    case["speedup_back_to_back"] = case["generic"]["back_to_back_median_us"] / case["k18"]["back_to_back_median_us"]
    # the relative condition: the kernel path is not slower than the generic one beyond the spread the runs themselves show
    case["k18_not_slower"] = bool(case["k18"]["median_us"] <= case["generic"]["max_us"]
                                  and case["k18"]["back_to_back_median_us"] <= case["generic"]["back_to_back_max_us"])
    case["class_not_slower"] = bool(case["k18_not_slower"] or case["class_takes"] == "generic")
    print("RESULT " + json.dumps(case), flush=True)
    # the second yardstick: the same sequence by the stock float32 functions -- what stock ops cost a user who does not ask for
    # the parity rule (the class's generic path runs float64, which this project made slower itself)
    case["stock_f32"] = timed(make_call(op, shape, False, wide=False), args.reps)
    case["speedup_over_stock_f32"] = case["stock_f32"]["median_us"] / case["k18"]["median_us"]
    case["speedup_over_stock_f32_back_to_back"] = case["stock_f32"]["back_to_back_median_us"] / case["k18"]["back_to_back_median_us"]
    case["k18_not_slower_than_stock_f32"] = bool(case["k18"]["median_us"] <= case["stock_f32"]["max_us"]
                                                 and case["k18"]["back_to_back_median_us"] <= case["stock_f32"]["back_to_back_max_us"])
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
    order = sorted(SHAPES, key=lambda s: torch.Size(s).numel())
    cases = ["%s,%s" % (op, "x".join(str(d) for d in shape)) for shape in order for op in OPS]
    for name in cases:   # small sizes first, every case in a fresh process
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=150)
            lines = [ln[7:] for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            entry = json.loads(lines[-1]) if lines else {"case": name}
            if run.returncode != 0:
                entry["child_exit"] = run.returncode
                entry["child_stderr"] = run.stderr.strip().splitlines()[-1][:200] if run.stderr.strip() else ""
        except subprocess.TimeoutExpired:
            entry = {"case": name, "child_exit": "timeout"}
        print(json.dumps(entry), flush=True)
        result["cases"].append(entry)
        # a device fault reaches Python as a RuntimeError, exit status 1 like any other: go on only after an exit of 1 whose
        # last line names no HIP / HSA error, and start nothing more on the device otherwise
        if entry.get("child_exit") is not None and (entry["child_exit"] != 1 or DEVICE_ERROR.search(run.stderr)):
            break
    result["clocks_power_after"] = smi()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
