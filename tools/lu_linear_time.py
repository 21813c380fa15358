#!/usr/bin/env python3
"""HIP-event time of K16 (the LU linear layer) against the same layer by stock torch ops on the same device -- the
reference's own sequence: F.linear twice forward, two solve_triangular back.

    python tools/lu_linear_time.py [--out profiles/lu_linear_time.json]

Every case runs in a fresh child process, small sizes first.  Per case: warm-up, then the median (and the min / max = the
spread) of `--reps` single calls between event pairs, and of trains of 20 calls between one pair (see `timed`).
Also: log_prob of a 4-layer NSF-style flow (features 16, hidden 32) with and without LULinear between the permutation
and the coupling -- what interleaving the layer costs while couplings run one per launch."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nflows_amd.transforms import LULinear  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warmup=10, train=20):
    """`single`: one call between an event pair on an idle device, `reps` times -- the host's enqueue path (argument
    checks, ctypes / about a dozen torch dispatches for the stock sequence) is INSIDE the interval, so for a short kernel
    this is a latency as a caller sees it, not the kernel.  `back_to_back`: `train` calls between ONE event pair, per
    call, `reps` times -- the queue stays full, so this approaches the device time when the device is the slower side."""
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


def flow(with_lu, features=16, hidden=32, layers=4):
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms import CompositeTransform, PiecewiseRationalQuadraticCouplingTransform, RandomPermutation
    from nflows_amd.utils.torchutils import create_alternating_binary_mask
    torch.manual_seed(0)
    ts = []
    for i in range(layers):
        ts.append(RandomPermutation(features))
        if with_lu:
            ts.append(LULinear(features))
        ts.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=create_alternating_binary_mask(features, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=hidden, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=3.0))
    return Flow(CompositeTransform(ts), StandardNormal([features])).to(DEV).eval()


def child(args):
    """One case in this process: K16 first, then the stock sequence (a library failure there costs this cell only)."""
    if args.case == "flow":
        x = torch.randn(16384, 16, device=DEV)
        out = {"batch": 16384, "features": 16, "layers": 4}
        for with_lu in (False, True):
            f = flow(with_lu)
            with torch.no_grad():
                out["with_lu" if with_lu else "without_lu"] = timed(lambda: f.log_prob(x), args.reps)
        print("RESULT " + json.dumps(out), flush=True)
        return
    batch, features, direction = args.case.split(",")
    batch, features, inverse = int(batch), int(features), direction == "inverse"
    torch.manual_seed(features)
    t = LULinear(features, identity_init=False).to(DEV)
    x = torch.randn(batch, features, device=DEV)
    floor_us = 2 * batch * features * 4 / 5.1e12 * 1e6   # the layer's traffic at K1's measured 4.9 - 5.3 TB/s
    case = {"batch": batch, "features": features, "direction": direction, "traffic_floor_us": floor_us}
    with torch.no_grad():
        case["k16"] = timed(lambda: (t.inverse if inverse else t)(x), args.reps)
        case["fraction_of_floor"] = floor_us / case["k16"]["back_to_back_median_us"]
        print("RESULT " + json.dumps(case), flush=True)
        try:
            case["torch_ops"] = timed(lambda: t._generic(x, inverse), args.reps)
            case["speedup"] = case["torch_ops"]["median_us"] / case["k16"]["median_us"]
            case["speedup_back_to_back"] = case["torch_ops"]["back_to_back_median_us"] / case["k16"]["back_to_back_median_us"]
        except RuntimeError as e:
            case["torch_ops"] = {"error": str(e).splitlines()[0][:200]}
    print("RESULT " + json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: one case in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    result = {"clocks_power_before": smi(), "cases": [], "flow": {},
              "stock_inverse": "two solve_triangular, at most 65 536 right-hand sides per library call "
                               "(nflows_amd/transforms/lu.py: solve_rows)"}
    cases = ["%d,%d,%s" % (b, d, k) for b in (16384, 262144) for d in (64, 128) for k in ("forward", "inverse")] + ["flow"]
    for name in cases:   # small sizes first, every case in a fresh process
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)],
                                 capture_output=True, text=True, timeout=280)
            lines = [ln[7:] for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            entry = json.loads(lines[-1]) if lines else {"case": name}
            if run.returncode != 0:
                entry["child_exit"] = run.returncode
                entry["child_stderr"] = run.stderr.strip().splitlines()[-1][:200] if run.stderr.strip() else ""
        except subprocess.TimeoutExpired:
            entry = {"case": name, "child_exit": "timeout"}
        print(json.dumps(entry), flush=True)
        if name == "flow":
            result["flow"] = entry
        else:
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
