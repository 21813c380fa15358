#!/usr/bin/env python3
"""HIP-event time of K24 (SVDLinear / QRLinear on the Householder kernel) against two yardsticks that are not the code
under test, on the same device: the class's own generic path (the reference's op sequence on stock device ops:
`_use_kernel = False`) and the cached-matrix product (`F.linear` with `weight()` / `weight_inverse()` formed beforehand:
what a user could do instead when num_householder is close to features).  DESIGN.md section 4, K24.

    python tools/householder_time.py [--out profiles/householder_time.json]

Every case (class, features, num_householder, rows) runs in a fresh child process, small sizes first, and times forward,
inverse and forward + backward.  Per timing: warm-up, then the median (and the min / max = the spread) of `--reps`
single calls between event pairs, and of trains of calls between one pair (`timed` of tools/lu_linear_time.py)."""
import argparse
import json
import os
import subprocess
import sys

import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lu_linear_time import smi, timed  # noqa: E402
from nflows_amd.transforms import QRLinear, SVDLinear  # noqa: E402

DEV = "cuda:0"


def make(cls, features, count, kernel):
    torch.manual_seed(features * 131 + count)
    t = (SVDLinear(features, count, identity_init=False) if cls == "svd" else QRLinear(features, count))
    with torch.no_grad():
        for n, p in t.named_parameters():
            if n.endswith("q_vectors") or n == "bias":
                p.normal_()
    for m in t.modules():
        m._use_kernel = kernel
    if kernel and cls == "qr":
        t._kernel_pays = lambda inputs, inverse: True   # the kernel itself is timed, not the class's dispatch rule
    return t.to(DEV)


def child(args):
    cls, features, count, rows = args.case.split(",")
    features, count, rows = int(features), int(count), int(rows)
    x = torch.randn(rows, features, device=DEV)
    r = torch.randn(rows, features, device=DEV)
    reps, train = (args.reps, 20) if rows * count <= 16384 * 128 else (max(5, args.reps // 3), 5)
    case = {"class": cls, "features": features, "num_householder": count, "rows": rows,
            "traffic_floor_us": 2 * rows * features * 4 / 5.1e12 * 1e6}
    for path in ("k24", "generic"):
        t = make(cls, features, count, path == "k24")

        def train_step():
            t.zero_grad(set_to_none=True)
            xin = x.detach().requires_grad_(True)
            y, lad = t(xin)
            ((y * r).sum() + lad.sum()).backward()

        out = {}
        try:
            with torch.no_grad():
                out["forward"] = timed(lambda: t(x), reps, train=train)
                out["inverse"] = timed(lambda: t.inverse(x), reps, train=train)
            out["forward_backward"] = timed(train_step, reps, train=train)
        except RuntimeError as e:
            out["error"] = str(e).splitlines()[0][:200]
        case[path] = out
        print("RESULT " + json.dumps(case), flush=True)
    t = make(cls, features, count, True)
    with torch.no_grad():
        w, wi, b = t.weight(), t.weight_inverse(), t.bias
        case["cached_matrix"] = {"forward": timed(lambda: F.linear(x, w, b), reps, train=train),
                                 "inverse": timed(lambda: F.linear(x - b, wi), reps, train=train)}
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
    cases = ["%s,%d,%d,%d" % (cls, d, k, rows) for rows in (16384, 262144) for d in (16, 64, 128)
             for k in sorted({2, 10, d}) for cls in ("svd", "qr")]
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
        result["cases"].append(entry)
        if entry.get("child_exit") not in (None, 1):   # anything but a Python error: start nothing more on the device
            break
        if args.out:   # (kept current: a later case's trouble loses nothing)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)
    result["clocks_power_after"] = smi()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
