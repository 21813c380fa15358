#!/usr/bin/env python3
"""HIP-event time of K19 (the 1x1 convolution on NCHW) against the two ways to get the same result without it, on the
same device:
  (a) `stock`    the reference's sequence by stock torch ops: index_select on the channels, permute, reshape, F.linear
                 twice forward / two solve_triangular back, reshape and permute back;
  (b) `composed` index_select + permute + K16 (ops.lu_linear) + permute: what a user could compose before K19.

    python tools/conv1x1_time.py [--out profiles/conv1x1_time.json]

Every case runs in a fresh child process under its own time limit, small sizes first; a child that ends on anything but a
Python error ends the run.  Per case: warm-up, then the median (and the min / max = the spread) of `--reps` single calls
between event pairs, and of trains of 20 calls between one pair (`timed` of tools/lu_linear_time.py).  The floor is the
tensor read once and written once, 2 B C HW 4 bytes, at K1's measured 5.1 TB/s."""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lu_linear_time import DEV, smi, timed  # noqa: E402
from nflows_amd import ops  # noqa: E402
from nflows_amd.transforms import OneByOneConvolution  # noqa: E402

IMAGES = 4096
CASES = ((12, 16, 16), (48, 8, 8), (128, 8, 8))   # (C, H, W)


def stock(t, x, inverse):
    """(a): the reference's forward / inverse, every step a stock device op."""
    b, c, h, w = x.shape
    perm = t.permutation._permutation
    if not inverse:
        x = x.index_select(1, perm)
    rows, lad = t._generic(x.permute(0, 2, 3, 1).reshape(b * h * w, c), inverse)
    out = rows.reshape(b, h, w, c).permute(0, 3, 1, 2)
    if inverse:
        out = out.index_select(1, t.permutation._inverse_permutation)
    return out.contiguous(), lad.reshape(b, h * w).sum(1)


def composed(t, x, inverse):
    """(b): the layout changes by stock ops around K16."""
    b, c, h, w = x.shape
    perm = t.permutation._permutation
    p = (t.lower_entries, t.upper_entries, t.unconstrained_upper_diag, t.bias)
    if not inverse:
        x = x.index_select(1, perm)
    rows, lad = ops.lu_linear(x.permute(0, 2, 3, 1).reshape(b * h * w, c), *p, eps=t.eps, inverse=inverse)
    out = rows.reshape(b, h, w, c).permute(0, 3, 1, 2)
    if inverse:
        out = out.index_select(1, t.permutation._inverse_permutation)
    return out.contiguous(), lad.reshape(b, h * w).sum(1)


def child(args):
    """One case in this process: K19 first, then the two alternatives (a library failure there costs that cell only)."""
    c, h, w, direction = args.case.split(",")
    c, h, w, inverse = int(c), int(h), int(w), direction == "inverse"
    torch.manual_seed(c)
    t = OneByOneConvolution(c, identity_init=False).to(DEV)
    x = torch.randn(IMAGES, c, h, w, device=DEV)
    floor_us = 2 * IMAGES * c * h * w * 4 / 5.1e12 * 1e6
    case = {"images": IMAGES, "channels": c, "height": h, "width": w, "direction": direction, "traffic_floor_us": floor_us}
    with torch.no_grad():
        got, _ = (t.inverse if inverse else t)(x)
        want, _ = composed(t, x, inverse)
        case["equals_composed_bit_for_bit"] = bool(torch.equal(got, want))
        del got, want
        case["k19"] = timed(lambda: (t.inverse if inverse else t)(x), args.reps)
        case["fraction_of_floor"] = floor_us / case["k19"]["back_to_back_median_us"]
        print("RESULT " + json.dumps(case), flush=True)
        for name, fn in (("composed", composed), ("stock", stock)):
            try:
                case[name] = timed(lambda: fn(t, x, inverse), args.reps)
                case["speedup_vs_" + name] = case[name]["median_us"] / case["k19"]["median_us"]
                case["speedup_vs_%s_back_to_back" % name] = \
                    case[name]["back_to_back_median_us"] / case["k19"]["back_to_back_median_us"]
            except RuntimeError as e:
                case[name] = {"error": str(e).splitlines()[0][:200]}
            print("RESULT " + json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: one case in a child process")
    args = ap.parse_args()
    if args.case:
        return child(args)
    result = {"clocks_power_before": smi(), "cases": [],
              "stock_inverse": "two solve_triangular, at most 65 536 right-hand sides per library call "
                               "(nflows_amd/transforms/lu.py: solve_rows)"}
    names = ["%d,%d,%d,%s" % (c, h, w, k) for c, h, w in CASES for k in ("forward", "inverse")]
    for name in names:   # small sizes first, every case in a fresh process under its own time limit
        try:
            run = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--case", name,
                                  "--reps", str(args.reps)], capture_output=True, text=True, timeout=200)
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
    return 0 if all("child_exit" not in e for e in result["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
