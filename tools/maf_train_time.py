#!/usr/bin/env python3
"""HIP-event time of one training step of masked autoregressive affine flows with K25 (MADE.forward under autograd on
K14 / K10, masks folded by the packer) against the same flow with the switch off -- the eager masked Linears, which is
the path before K25 and therefore the baseline.

    python tools/maf_train_time.py [--out profiles/maf_train_time.json]

One process.  Flows: the context-free shapes of profiles/maf_time.json -- 5 / 10 / 16 layers on 8 / 43 / 64 features,
hidden width 128, 2 blocks, reverse permutations -- at 1 024, 16 384 and 262 144 rows.  Per flow and row count, after a
warm-up of both paths:
  * `step`: zero_grad + `-flow.log_prob(x).mean()` + backward(), eagerly enqueued;
  * `graphed_step`: one replay of a `GraphedTrainStep` (the same plus Adam, capturable) per path;
each timed as `--windows` windows of back-to-back calls between ONE event pair, every window at least `--window` seconds
long, the two paths alternating window by window.  Every figure is per call: the median of the windows with their min / max
(the spread of repeats).  `k25_not_slower`: K25's median is not above the switched-off median by more than `spread_us`, the larger of the two
paths' max - min over their windows.
Separately the element's backward kernel alone (nfa_affine_autoregressive_backward_f32, both directions) beside the time
its 28 / 32 bytes per element would take at `--hbm-gbs` (the HBM figure the share is stated against)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
DEV = "cuda:0"
SHAPES = {
    "d8_l5": dict(features=8, hidden_features=128, num_layers=5, num_blocks=2),
    "d43_l10": dict(features=43, hidden_features=128, num_layers=10, num_blocks=2),
    "d64_l16": dict(features=64, hidden_features=128, num_layers=16, num_blocks=2),
}
ROWS = (1024, 16384, 262144)


def window(fn, seconds, calls):
    """`calls` back-to-back calls between one event pair, doubled until the window lasts `seconds`: (us per call, calls)"""
    import torch
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms * 1e3 / calls, calls
        calls = max(calls + 1, int(calls * min(8.0, 1.2 * seconds * 1e3 / max(ms, 1e-3))))


def alternate(paths, seconds, windows, switch):
    """paths: {name: (switch value, fn)}; returns {name: {median_us, min_us, max_us, windows, calls_per_window}}"""
    import torch
    calls = {name: 1 for name in paths}
    for name, (on, fn) in paths.items():   # warm-up of every path
        switch(on)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in paths}
    for _ in range(windows):
        for name, (on, fn) in paths.items():
            switch(on)
            us, calls[name] = window(fn, seconds, calls[name])
            times[name].append(us)
    return {name: {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "windows": len(t),
                   "calls_per_window": calls[name]} for name, t in times.items()}


def verdict(entry):
    entry["speedup"] = entry["k25_off"]["median_us"] / entry["k25_on"]["median_us"]
    spread = max(entry[k]["max_us"] - entry[k]["min_us"] for k in ("k25_on", "k25_off"))
    entry["spread_us"] = spread
    entry["k25_not_slower"] = bool(entry["k25_on"]["median_us"] <= entry["k25_off"]["median_us"] + spread)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS))
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth the element kernel's floor is stated against")
    args = ap.parse_args()
    import copy
    import torch
    from maf_time import build
    from nonlin_time import smi
    from nflows_amd import ops
    from nflows_amd.graphs import GraphedTrainStep
    from nflows_amd.transforms.made import MADE

    def switch(on):
        MADE.fuse_training = on

    result = {"clocks_power_before": smi(), "window_seconds": args.window, "cases": [], "element_backward": []}
    rows_list = [int(r) for r in args.rows.split(",")]
    for name in args.shapes.split(","):
        cfg = SHAPES[name]
        flow = build(cfg).train()
        for rows in rows_list:
            x = 1.2 * torch.randn(rows, cfg["features"], device=DEV, generator=torch.Generator(DEV).manual_seed(rows))

            def step():
                flow.zero_grad(set_to_none=True)
                loss = -flow.log_prob(x).mean()
                loss.backward()
                return loss

            entry = {"what": "step", "shape": name, "rows": rows, **cfg}
            switch(True)
            on = step().item()
            switch(False)
            entry["loss_k25_on"], entry["loss_k25_off"] = on, step().item()
            entry.update(alternate({"k25_on": (True, step), "k25_off": (False, step)}, args.window, args.windows, switch))
            result["cases"].append(verdict(entry))
            print(json.dumps(entry), flush=True)
            # one captured step with Adam per path (the switch is read at capture time)
            graphed = {}
            for label, on in (("k25_on", True), ("k25_off", False)):
                switch(on)
                twin = copy.deepcopy(flow)
                opt = torch.optim.Adam(twin.parameters(), lr=1e-4, capturable=True)
                graphed[label] = (on, (lambda s: (lambda: s(x)))(GraphedTrainStep(twin, opt, x, warmup=2)))
            entry = {"what": "graphed_step", "shape": name, "rows": rows, **cfg}
            entry.update(alternate(graphed, args.window, args.windows, switch))
            result["cases"].append(verdict(entry))
            print(json.dumps(entry), flush=True)
            del graphed
            switch(True)
        del flow
        torch.cuda.empty_cache()
    # the element's backward kernel alone
    for rows, features in ((1024, 8), (16384, 43), (262144, 64)):
        g = torch.Generator(DEV).manual_seed(features)
        x = torch.randn(rows, features, device=DEV, generator=g)
        p = torch.randn(rows, 2 * features, device=DEV, generator=g)
        g_y, g_l = torch.randn(rows, features, device=DEV, generator=g), torch.randn(rows, device=DEV, generator=g)
        for inverse, per_element in ((False, 28), (True, 32)):
            out = ops.affine_autoregressive(x, p, inverse=inverse)[0]

            def call():
                ops.affine_autoregressive_backward(None if inverse else x, p, out if inverse else None, g_y, g_l, inverse)
            t = alternate({"kernel": (True, call)}, args.window, args.windows, switch)["kernel"]
            floor_us = rows * features * per_element / (args.hbm_gbs * 1e9) * 1e6
            entry = {"rows": rows, "features": features, "inverse": inverse, "bytes_per_element": per_element, **t,
                     "floor_us_at_hbm_gbs": floor_us, "hbm_gbs": args.hbm_gbs, "share_of_floor": floor_us / t["median_us"],
                     "note": "back-to-back calls through the Python wrapper: at small sizes the host's enqueue path, not the kernel"}
            result["element_backward"].append(entry)
            print(json.dumps(entry), flush=True)
    result["clocks_power_after"] = smi()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
