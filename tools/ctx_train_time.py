#!/usr/bin/env python3
"""HIP-event time of one training step of CONDITIONAL flows with K27 (conditioners with a context on K14 / K10:
autograd.ResidualNetHiddenCtx / MadeNetCtx) against the same flow with the switch off -- the eager conditioner modules,
which is the path before K27 and therefore the baseline.

    python tools/ctx_train_time.py [--out profiles/ctx_train_time.json]

One process; the method, the windows and the verdict are tools/maf_train_time.py's.  Flows: conditional RQ-NSF coupling
(8 layers on 16 features with a 16-feature context; 16 layers on 32 features with a 32-feature context; hidden 128, 2
blocks, 8 bins, linear tails) and conditional MAF (8 layers on 21 features with a 16-feature context; 5 layers on 8
features with an 8-feature context; hidden 128, 2 blocks) at 1 024, 16 384 and 262 144 rows.  Per flow and row count:
  * `step`: zero_grad + `-flow.log_prob(x, context=c).mean()` + backward(), eagerly enqueued;
  * `graphed_step`: one replay of a `GraphedTrainStep` with a context (the same plus Adam, capturable) per path;
the two paths alternating window by window.  `k27_not_slower`: K27's median is not above the switched-off median by more
than the larger of the two paths' max - min.
Separately the forward and the backward kernel alone per mode against their context-free twins at 65 536 rows (32 identity
columns, 2 blocks, with the final Linear of 368 outputs): the difference is what the plane reads and the gate cost."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
DEV = "cuda:0"
SHAPES = {
    "nsf_d16_c16_l8": dict(kind="nsf", features=16, context=16, num_layers=8),
    "nsf_d32_c32_l16": dict(kind="nsf", features=32, context=32, num_layers=16),
    "maf_d21_c16_l8": dict(kind="maf", features=21, context=16, num_layers=8),
    "maf_d8_c8_l5": dict(kind="maf", features=8, context=8, num_layers=5),
}
ROWS = (1024, 16384, 262144)


def build(cfg):
    import torch
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms import (CompositeTransform, MaskedAffineAutoregressiveTransform,
                                       PiecewiseRationalQuadraticCouplingTransform, ReversePermutation)
    from nflows_amd.utils import create_alternating_binary_mask
    torch.manual_seed(0)
    D, C = cfg["features"], cfg["context"]
    layers = []
    for i in range(cfg["num_layers"]):
        layers.append(ReversePermutation(D))
        if cfg["kind"] == "nsf":
            layers.append(PiecewiseRationalQuadraticCouplingTransform(
                create_alternating_binary_mask(D, even=(i % 2 == 0)),
                lambda i_, o_: ResidualNet(i_, o_, hidden_features=128, context_features=C, num_blocks=2),
                num_bins=8, tails="linear", tail_bound=3.0))
        else:
            layers.append(MaskedAffineAutoregressiveTransform(features=D, hidden_features=128, context_features=C, num_blocks=2))
    return Flow(CompositeTransform(layers), StandardNormal([D])).to(DEV)


def verdict(entry):
    entry["speedup"] = entry["k27_off"]["median_us"] / entry["k27_on"]["median_us"]
    spread = max(entry[k]["max_us"] - entry[k]["min_us"] for k in ("k27_on", "k27_off"))
    entry["spread_us"] = spread
    entry["k27_not_slower"] = bool(entry["k27_on"]["median_us"] <= entry["k27_off"]["median_us"] + spread)
    return entry


def kernels_alone(args, result, alternate):
    import torch
    from nflows_amd import ops
    B, di, nb, out = 65536, 32, 2, 368
    g = torch.Generator(DEV).manual_seed(1)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g)      # noqa: E731
    blocks = [(r(128, 128) / 11, r(128) / 11, r(128, 128) / 16, r(128) / 16) for _ in range(nb)]
    fw, fb, bw, fbias = ops.pack_resnet_hidden_train(r(128, di) / 6, r(128) / 6, blocks, (r(out, 128) / 11, r(out) / 11))
    x, gp = r(B, di), r(B, out)
    planes, initial = [r(B, 128) for _ in range(nb)], torch.relu(r(B, 128))
    modes = {"none": None, "glu": ops.TRAIN_CTX_GLU, "add": ops.TRAIN_CTX_ADD}
    state = {}

    def forward(mode):
        if mode is None:
            state[mode] = ops.resnet_hidden_forward(x, fw, fb, nb, fbias, out) + (None,)
        else:
            state[mode] = ops.resnet_hidden_forward_ctx(mode, x, planes, fw, fb, nb, fbias, out,
                                                        initial_plane=initial if mode == ops.TRAIN_CTX_ADD else None)

    def backward(mode):
        saved, pre = state[mode][1], state[mode][3]
        if mode is None:
            ops.resnet_backward(gp, bw, saved, di)
        else:
            ops.resnet_backward_ctx(mode, gp, bw, saved, di, planes, pre, from_params=True)

    for what, fn in (("forward", forward), ("backward", backward)):
        for m in modes.values():
            forward(m)
        t = alternate(dict((name, (True, (lambda mode: (lambda: fn(mode)))(m))) for name, m in modes.items()),
                      args.window, args.windows, lambda on: None)
        entry = {"what": what + "_kernel", "rows": B, "num_identity": di, "num_blocks": nb, "out_features": out, **t,
                 "note": "through the Python wrapper (allocations included), back-to-back calls"}
        for name in ("glu", "add"):
            entry[name + "_over_none"] = t[name]["median_us"] / t["none"]["median_us"]
        result["kernels"].append(entry)
        print(json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS))
    args = ap.parse_args()
    import copy
    import torch
    from maf_train_time import alternate
    from nonlin_time import smi
    from nflows_amd import ops
    from nflows_amd.graphs import GraphedTrainStep

    def switch(on):
        ops.CTX_TRAINING = on

    result = {"clocks_power_before": smi(), "window_seconds": args.window, "cases": [], "kernels": []}
    kernels_alone(args, result, alternate)
    rows_list = [int(r) for r in args.rows.split(",")]
    for name in args.shapes.split(","):
        cfg = SHAPES[name]
        flow = build(cfg).train()
        for rows in rows_list:
            gen = torch.Generator(DEV).manual_seed(rows)
            x = 1.2 * torch.randn(rows, cfg["features"], device=DEV, generator=gen)
            c = torch.randn(rows, cfg["context"], device=DEV, generator=gen)

            def step():
                flow.zero_grad(set_to_none=True)
                loss = -flow.log_prob(x, context=c).mean()
                loss.backward()
                return loss

            entry = {"what": "step", "shape": name, "rows": rows, **cfg}
            switch(True)
            on = step().item()
            switch(False)
            entry["loss_k27_on"], entry["loss_k27_off"] = on, step().item()
            entry.update(alternate({"k27_on": (True, step), "k27_off": (False, step)}, args.window, args.windows, switch))
            result["cases"].append(verdict(entry))
            print(json.dumps(entry), flush=True)
            graphed = {}
            for label, on in (("k27_on", True), ("k27_off", False)):     # (the switch is read at capture time)
                switch(on)
                twin = copy.deepcopy(flow)
                opt = torch.optim.Adam(twin.parameters(), lr=1e-4, capturable=True)
                graphed[label] = (on, (lambda s: (lambda: s(x, c)))(GraphedTrainStep(twin, opt, x, warmup=2, example_context=c)))
            entry = {"what": "graphed_step", "shape": name, "rows": rows, **cfg}
            entry.update(alternate(graphed, args.window, args.windows, switch))
            result["cases"].append(verdict(entry))
            print(json.dumps(entry), flush=True)
            del graphed
            switch(True)
        del flow
        torch.cuda.empty_cache()
    result["clocks_power_after"] = smi()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
