#!/usr/bin/env python3
"""Golden vectors of the normalisation transforms and the two flow factories: the REAL reference (bayesiains/nflows,
imported read-only as make_golden.py does) run on the CPU in float32 and float64.  Run in the build container only:

    python tests/golden/make_golden_norm.py

Writes, next to this script, data only:
  norm_bn_d{D}_{part}.npz   BatchNorm with perturbed `unconstrained_weight` / `bias`, D in 2, 5, 64, 100, 128; part =
                      small (parameters, log-determinants, running buffers after one and after three training batches,
                      parameter gradients), train (training forward of batch 1), eval, inv (eval forward / inverse from the
                      buffers after three batches), gtrain, geval, ginv (input gradients of sum(y * r) + sum(logabsdet))
  norm_an_d{D}_{part}.npz   ActNorm initialised by its first training batch: small, fwd, inv, gfwd, ginv
  norm_flow_{maf,realnvp}.npz  MaskedAutoregressiveFlow(8, 32, 3, 2) and SimpleRealNVP(16, 32, 4, 2), batch_norm_between_layers=True
Every file is kept below 1 MiB (one [rows, D] result and its float64 difference each; the row counts of make_golden_lu.py);
inputs are regenerated from their seeds (`norm_inputs`: numpy's RandomState stream is frozen) -- columns with offsets up
to +-3 and spreads 0.2 .. 5, so that a wrong mean or a biased variance cannot hide -- and every float64 result is stored
as the float32 result plus a float32 difference (`*_d`).
"""
import copy
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "_refshim"))
sys.path.insert(0, REF)

import torch  # noqa: E402

from nflows.flows.autoregressive import MaskedAutoregressiveFlow  # noqa: E402
from nflows.flows.realnvp import SimpleRealNVP  # noqa: E402
from nflows.transforms.normalization import ActNorm, BatchNorm  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

ROWS = {2: 4096, 5: 4096, 64: 1280, 100: 800, 128: 640}


def norm_inputs(features, batch, rows=None):
    """Batch number `batch` (0, 1, 2) for D = features and the weights r of the gradient's loss; the tests regenerate them."""
    rng = np.random.RandomState(5000 * features + batch)
    rows = ROWS[features] if rows is None else rows
    offset = rng.uniform(-3.0, 3.0, size=features)
    spread = np.exp(rng.uniform(np.log(0.2), np.log(5.0), size=features))
    x = (offset + spread * rng.randn(rows, features)).astype(np.float32)
    r = rng.randn(rows, features).astype(np.float32)
    return x, r


def pair(out, name, v32, v64):
    v32 = v32.detach().numpy()
    out[name] = v32
    out[name + "_d"] = (v64.detach().numpy() - v32.astype(np.float64)).astype(np.float32)


def both(fn, t32, t64, x32):
    """fn(layer, inputs) on the float32 layer and on the float64 one (same float32 inputs, widened)."""
    return fn(t32, x32), fn(t64, x32.double())


def grads(out, prefix, layers, source, r, call, names):
    got = []
    for layer, dt in zip(layers, (torch.float32, torch.float64)):
        layer.zero_grad()
        xin = source.detach().clone().to(dt).requires_grad_(True)
        y, lad = call(layer, xin)
        ((y * r.to(dt)).sum() + lad.sum()).backward()
        got.append([xin.grad] + [getattr(layer, n).grad.clone() for n in names])
    for n, g32, g64 in zip(("inputs",) + tuple(names), *got):
        pair(out, prefix + n, g32, g64)


def bn_case(features):
    out = {}
    torch.manual_seed(features * 11 + 3)
    t = BatchNorm(features)
    with torch.no_grad():
        t.unconstrained_weight.add_(0.5 * torch.randn(features))
        t.bias.normal_()
    t64 = copy.deepcopy(t).double()
    layers = (t, t64)
    names = ("unconstrained_weight", "bias")
    for n in names:
        out[n] = getattr(t, n).detach().numpy().copy()
    batches = [torch.from_numpy(norm_inputs(features, b)[0]) for b in range(3)]
    r = torch.from_numpy(norm_inputs(features, 0)[1])
    x = batches[0]
    # gradients in training mode first: on copies, so that the running buffers below see exactly three batches
    grads(out, "gtrain_", (copy.deepcopy(t).train(), copy.deepcopy(t64).train()), x, r, lambda m, v: m(v), names)
    t.train(), t64.train()
    with torch.no_grad():
        for b, xb in enumerate(batches):
            (y, lad), (y64, lad64) = both(lambda m, v: m(v), t, t64, xb)
            if b == 0:
                pair(out, "train_y", y, y64)
                pair(out, "train_lad", lad[:1], lad64[:1])
            if b in (0, 2):
                tag = "after%d_" % (b + 1)
                pair(out, tag + "running_mean", t.running_mean.clone(), t64.running_mean.clone())
                pair(out, tag + "running_var", t.running_var.clone(), t64.running_var.clone())
        t.eval(), t64.eval()
        (ye, lade), (ye64, lade64) = both(lambda m, v: m(v), t, t64, x)
        pair(out, "eval_y", ye, ye64)
        pair(out, "eval_lad", lade[:1], lade64[:1])
        (xi, ladi), (xi64, ladi64) = both(lambda m, v: m.inverse(v), t, t64, ye)   # at the float32 eval output
        pair(out, "inv_x", xi, xi64)
        pair(out, "inv_lad", ladi[:1], ladi64[:1])
    grads(out, "geval_", layers, x, r, lambda m, v: m(v), names)
    grads(out, "ginv_", layers, ye, r, lambda m, v: m.inverse(v), names)
    return out


def an_case(features):
    out = {}
    t = ActNorm(features)
    t64 = copy.deepcopy(t).double()
    layers = (t, t64)
    names = ("log_scale", "shift")
    xn, rn = norm_inputs(features, 0)
    x, r = torch.from_numpy(xn), torch.from_numpy(rn)
    t.train(), t64.train()
    with torch.no_grad():
        (y, lad), (y64, lad64) = both(lambda m, v: m(v), t, t64, x)     # initialises both
        assert bool(t.initialized) and bool(t64.initialized)
        for n in names:
            pair(out, n, getattr(t, n).data.clone(), getattr(t64, n).data.clone())
        pair(out, "fwd_y", y, y64)
        pair(out, "fwd_lad", lad[:1], lad64[:1])
        (xi, ladi), (xi64, ladi64) = both(lambda m, v: m.inverse(v), t, t64, y)
        pair(out, "inv_x", xi, xi64)
        pair(out, "inv_lad", ladi[:1], ladi64[:1])
    grads(out, "gfwd_", layers, x, r, lambda m, v: m(v), names)
    grads(out, "ginv_", layers, y, r, lambda m, v: m.inverse(v), names)
    return out


BN_PARTS = (("train_y", "train"), ("eval_y", "eval"), ("inv_x", "inv"), ("gtrain_inputs", "gtrain"),
            ("geval_inputs", "geval"), ("ginv_inputs", "ginv"))
AN_PARTS = (("fwd_y", "fwd"), ("inv_x", "inv"), ("gfwd_inputs", "gfwd"), ("ginv_inputs", "ginv"))


def part_of(key, parts):
    for stem, part in parts:
        if key in (stem, stem + "_d"):
            return part
    return "small"


def save(path, arrays):
    np.savez(path, **arrays)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


FLOWS = {
    "maf": (lambda: MaskedAutoregressiveFlow(features=8, hidden_features=32, num_layers=3, num_blocks_per_layer=2,
                                             batch_norm_between_layers=True), 8, 21),
    "realnvp": (lambda: SimpleRealNVP(features=16, hidden_features=32, num_layers=4, num_blocks_per_layer=2,
                                      batch_norm_between_layers=True), 16, 22),
}


def perturb(flow):
    """Away from the initial state (identity BatchNorm, near-identity couplings); the tests apply nothing: they load."""
    with torch.no_grad():
        for name, p in flow.named_parameters():
            if name.endswith("unconstrained_weight"):
                p.add_(0.5 * torch.randn_like(p))
            elif name.endswith("bias") and name.split(".")[-2].isdigit() and p.dim() == 1 and "net" not in name:
                p.normal_()
            elif "final_layer" in name:
                p.add_(0.05 * torch.randn_like(p))   # (larger: the MAF's inverse divides by scales near zero)


def flow_case(out, key, rows=512):
    make, features, seed = FLOWS[key]
    torch.manual_seed(seed)
    flow = make()
    for k, v in flow.state_dict().items():
        out["%s/init/%s" % (key, k)] = v.numpy().copy()
    torch.manual_seed(seed + 100)
    perturb(flow)
    flow64 = copy.deepcopy(flow).double()
    xa, xb, x = (torch.from_numpy(norm_inputs(features, 10 + i, rows)[0]) for i in range(3))
    for k, v in flow.state_dict().items():
        out["%s/start/%s" % (key, k)] = v.numpy().copy()
    flow.train(), flow64.train()
    with torch.no_grad():
        pair(out, key + "/train_log_prob", flow.log_prob(xa), flow64.log_prob(xa.double()))
        flow.log_prob(xb), flow64.log_prob(xb.double())
        flow.eval(), flow64.eval()
        state64 = flow64.state_dict()
        for k, v in flow.state_dict().items():
            out["%s/state/%s" % (key, k)] = v.numpy().copy()
            if "running_" in k:     # what the two training passes left: float32 + the float64 flow's, for the parity rule
                pair(out, "%s/buffers/%s" % (key, k), v.clone(), state64[k].clone())
        pair(out, key + "/log_prob", flow.log_prob(x), flow64.log_prob(x.double()))
        z, lad = flow._transform(x)
        z64, lad64 = flow64._transform(x.double())
        pair(out, key + "/z", z, z64)
        pair(out, key + "/lad", lad, lad64)
        xs, ladi = flow._transform.inverse(z)      # noise -> data, from the float32 z stored above
        xs64, ladi64 = flow64._transform.inverse(z.double())
        pair(out, key + "/x_from_z", xs, xs64)
        pair(out, key + "/ladi", ladi, ladi64)


def main():
    for features in sorted(ROWS):
        for stem, case, parts in (("bn", bn_case, BN_PARTS), ("an", an_case, AN_PARTS)):
            out = case(features)
            for part in ("small",) + tuple(p for _, p in parts):
                save(os.path.join(HERE, "norm_%s_d%d_%s.npz" % (stem, features, part)),
                     {k: v for k, v in out.items() if part_of(k, parts) == part})
    for key in sorted(FLOWS):
        out = {}
        flow_case(out, key)
        save(os.path.join(HERE, "norm_flow_%s.npz" % key), out)


if __name__ == "__main__":
    main()
