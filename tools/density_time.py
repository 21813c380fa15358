#!/usr/bin/env python3
"""HIP-event time of K20 (the learned base densities) against the same class on its generic path -- the reference's sequence
by stock torch ops on the same device, which is what a user had before.

    python tools/density_time.py [--out profiles/density_time.json]

Cases, forward (no grad) and forward + backward (gradients with respect to every operand, the incoming gradient prepared
outside the timed region):
  diag_shared   DiagonalNormal             262 144 x 64
  diag_row      ConditionalDiagonalNormal  262 144 x 64, the [B, 128] parameters given as the context (identity encoder)
  mog           MixtureOfGaussiansMADE.log_prob behind a given final-layer output, 262 144 x 8 x 10 and 16 384 x 64 x 5
Every case runs in a fresh child process.  Per case and path: warm-up, then the median (and the min / max = the spread) of
`--reps` single calls between event pairs, and of trains of calls between one pair (`timed`, as tools/nonlin_time.py).
`traffic_floor_us`: the bytes the operation must move at K1's measured 5.1 TB/s -- forward: the operands once and B results;
forward + backward: the operands twice and every gradient once."""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nonlin_time import smi, timed  # noqa: E402

from nflows_amd.distributions import ConditionalDiagonalNormal, DiagonalNormal  # noqa: E402
from nflows_amd.nn.nde import MixtureOfGaussiansMADE  # noqa: E402

DEV = "cuda:0"
DEVICE_ERROR = re.compile(r"HIP error|hipError|HSA_STATUS|illegal memory access|device-side assert|Memory access fault", re.I)
CASES = (("mog", (16384, 64, 5)), ("diag_shared", (262144, 64)), ("diag_row", (262144, 64)), ("mog", (262144, 8, 10)))


def floor_bytes(kind, shape, backward):
    B = shape[0]
    if kind == "mog":
        operands = B * shape[1] * (1 + 3 * shape[2])
        grads = operands
    else:
        n = shape[1]
        operands = B * n + (2 * n if kind == "diag_shared" else 2 * B * n)
        grads = operands
    return 4 * ((2 * operands + grads + B) if backward else (operands + B))


def make_call(kind, shape, use_kernel, backward):
    torch.manual_seed(len(shape))
    B = shape[0]
    x = torch.randn(B, shape[1], device=DEV) * 1.5
    g = torch.randn(B, device=DEV)
    if kind == "mog":
        D, K = shape[1], shape[2]
        made = MixtureOfGaussiansMADE(features=D, hidden_features=8, num_mixture_components=K).to(DEV)
        made._use_kernel = use_kernel
        outputs = torch.randn(B, D * K * 3, device=DEV)
        made.forward = lambda inputs, context=None: outputs
        leaves = (x, outputs)
        fn = lambda: made.log_prob(x)                                   # noqa: E731
    elif kind == "diag_shared":
        d = DiagonalNormal([shape[1]]).to(DEV)
        d._use_kernel = use_kernel
        d.mean_.data.normal_()
        d.log_std_.data.normal_(std=0.5)
        leaves = (x, d.mean_, d.log_std_)
        fn = lambda: d.log_prob(x)                                      # noqa: E731
    else:
        d = ConditionalDiagonalNormal([shape[1]]).to(DEV)
        d._use_kernel = use_kernel
        params = torch.randn(B, 2 * shape[1], device=DEV) * 0.5
        leaves = (x, params)
        fn = lambda: d.log_prob(x, context=params)                      # noqa: E731
    if not backward:
        def call():
            with torch.no_grad():
                fn()
        return call
    for t in leaves:
        t.requires_grad_(True)

    def call():
        for t in leaves:
            t.grad = None
        fn().backward(g)
    return call


def child(args):
    kind, dims, what = args.case.split(",")
    shape = tuple(int(d) for d in dims.split("x"))
    backward = what == "forward_backward"
    floor_us = floor_bytes(kind, shape, backward) / 5.1e12 * 1e6
    case = {"op": kind, "shape": list(shape), "pass": what, "traffic_floor_us": floor_us}
    case["k20"] = timed(make_call(kind, shape, True, backward), args.reps)
    case["fraction_of_floor"] = floor_us / case["k20"]["back_to_back_median_us"]
    print("RESULT " + json.dumps(case), flush=True)
    case["generic"] = timed(make_call(kind, shape, False, backward), args.reps)
    case["speedup"] = case["generic"]["median_us"] / case["k20"]["median_us"]
    case["speedup_back_to_back"] = case["generic"]["back_to_back_median_us"] / case["k20"]["back_to_back_median_us"]
    case["k20_not_slower"] = bool(case["k20"]["median_us"] <= case["generic"]["max_us"]
                                  and case["k20"]["back_to_back_median_us"] <= case["generic"]["back_to_back_max_us"])
    print("RESULT " + json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: one case in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    result = {"clocks_power_before": smi(), "cases": []}
    names = ["%s,%s,%s" % (kind, "x".join(str(d) for d in shape), what) for kind, shape in CASES
             for what in ("forward", "forward_backward")]
    for name in names:   # every case in a fresh process
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
        # a device fault reaches Python as a RuntimeError, exit status 1 like any other: go on only after an exit of 1 whose
        # output names no HIP / HSA error, and start nothing more on the device otherwise
        if entry.get("child_exit") is not None and (entry["child_exit"] != 1 or DEVICE_ERROR.search(run.stderr)):
            break
    result["clocks_power_after"] = smi()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
