#!/usr/bin/env python3
"""HIP-event time of float64 spline coupling layers with K26 (the whole layer in one launch on the f64 matrix
instruction) against the same layer with the switch off -- stock float64 GEMMs and K5d, the path before K26 and therefore
the baseline.

    python tools/f64_layer_time.py [--out profiles/f64_layer_time.json]

One process.  After a warm-up of both paths every case is timed as `--windows` windows of back-to-back calls between ONE
event pair, every window at least `--window` seconds long, the two paths alternating window by window; every figure is
per call: the median of the windows with their min / max.  `k26_not_slower`: K26's median is not above the switched-off
median by more than `spread_us`, the larger of the two paths' max - min over their windows.
Cases: one layer (32 / 32 features, H 128, 2 blocks, 8 bins) at 1 024 / 4 096 / 8 192 / 16 384 / 65 536 / 262 144 rows,
forward and inverse; `log_prob` of the 32-layer flow at 8 192 / 16 384 / 65 536 rows; one narrow layer (H 32, D 8) at the
same row counts.  K26 itself is timed at every size (the gate's size rule is lifted for the run); `gate_takes_k26` says
which of the two paths the rule gives that case.
`mfma_share`: the MFMA flop K26 issues (padded tiles included) per second over the float64 matrix rate that
tools/bin/f64_mfma_probe measures on this device with a register-resident loop (no figure when the probe is missing)."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
DEV = "cuda:0"


def measured_f64_rate():
    """TFLOP/s of the probe, the better of one and two waves per SIMD; None without the probe"""
    probe = os.path.join(HERE, "bin", "f64_mfma_probe")
    if not os.path.exists(probe):
        return None
    best = None
    for waves in ("1", "2"):
        out = subprocess.run([probe, waves], check=True, capture_output=True, text=True, timeout=120).stdout
        rate = json.loads(out.strip().splitlines()[-1])["f64_mfma_tflops"]
        best = rate if best is None else max(best, rate)
    return best


def mfma_flop(layer, rows):
    from nflows_amd import ops
    net = layer.transform_net
    lay = ops.resnet_f64_layout(layer.num_identity_features, net.hidden_features, len(net.blocks),
                                layer.num_transform_features, layer._transform_dim_multiplier())
    per_wave = (lay["ks0"] * lay["NT"] + 2 * len(net.blocks) * lay["ksh"] * lay["NT"]
                + lay["ksh"] * ((lay["chunks"] - 1) * lay["NTF"] + lay["NTL"]))
    waves = 4 * ((rows + ops.F64_LAYER_ROWS - 1) // ops.F64_LAYER_ROWS)
    return 2048.0 * per_wave * waves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rows", default="1024,4096,8192,16384,65536,262144")
    ap.add_argument("--flow-rows", default="8192,16384,65536")
    args = ap.parse_args()
    import torch
    from maf_train_time import alternate
    from nflows_amd import configs
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ

    min_rows = RQ.fuse_float64_min_rows
    RQ.fuse_float64_min_rows = 0   # (K26 itself is timed at every size; `gate_takes_k26` says what the size rule does there)

    def switch(on):
        RQ.fuse_float64 = on

    def steep(flow):
        with torch.no_grad():
            for name, p in flow.named_parameters():
                if "final_layer" in name:
                    p.mul_(4.0)
                elif "linear_layers.1" in name:
                    p.mul_(30.0)
        return flow.double().to(DEV).eval()

    def verdict(entry, flop=None):
        on, off = entry["k26_on"], entry["k26_off"]
        entry["ms_k26"], entry["ms_off"] = on["median_us"] / 1e3, off["median_us"] / 1e3
        entry["speedup"] = off["median_us"] / on["median_us"]
        entry["spread_us"] = max(entry[k]["max_us"] - entry[k]["min_us"] for k in ("k26_on", "k26_off"))
        entry["k26_not_slower"] = bool(on["median_us"] <= off["median_us"] + entry["spread_us"])
        entry["gate_takes_k26"] = bool(entry["hidden_features"] <= 32 or entry["rows"] >= min_rows)
        if flop is not None:
            entry["mfma_tflops"] = flop / (on["median_us"] * 1e-6) / 1e12
            entry["mfma_share"] = entry["mfma_tflops"] / rate if rate else None
        print(json.dumps(entry), flush=True)
        return entry

    rate = measured_f64_rate()
    result = {"f64_mfma_tflops_measured": rate, "window_seconds": args.window, "fuse_float64_min_rows": min_rows, "cases": []}
    for what, D, H in (("layer", 64, 128), ("narrow layer", 8, 32)):
        flow = steep(configs.rq_nsf_flow(1, D, 8, H, 2, 3.0, seed=0))
        layer = [t for t in flow._transform._transforms if isinstance(t, RQ)][0]
        for rows in [int(r) for r in args.rows.split(",")]:
            x = torch.randn(rows, D, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(rows))
            for inverse in (False, True):
                fn = layer.inverse if inverse else layer.forward

                def call():
                    with torch.no_grad():
                        fn(x)
                entry = {"what": what, "rows": rows, "features": D, "hidden_features": H, "inverse": inverse}
                entry.update(alternate({"k26_on": (True, call), "k26_off": (False, call)}, args.window, args.windows, switch))
                result["cases"].append(verdict(entry, mfma_flop(layer, rows)))
    flow = steep(configs.rq_nsf_flow(32, 64, 8, 128, 2, 3.0, seed=0))
    layers = [t for t in flow._transform._transforms if isinstance(t, RQ)]
    for rows in [int(r) for r in args.flow_rows.split(",")]:
        x = torch.randn(rows, 64, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(rows))

        def call():
            with torch.no_grad():
                flow.log_prob(x)
        entry = {"what": "log_prob, 32 layers", "rows": rows, "features": 64, "hidden_features": 128}
        entry.update(alternate({"k26_on": (True, call), "k26_off": (False, call)}, args.window, args.windows, switch))
        result["cases"].append(verdict(entry, sum(mfma_flop(t, rows) for t in layers)))
    switch(True)
    RQ.fuse_float64_min_rows = min_rows
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
