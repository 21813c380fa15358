#!/usr/bin/env python3
"""Golden vectors of the LU linear layer: the REAL reference (bayesiains/nflows, imported read-only as
make_golden.py does) run on the CPU in float32 and float64.  Run in the build container only:

    python tests/golden/make_golden_lu.py

Writes, next to this script, data only:
  lu_linear_d{D}_{kind}_{part}.npz  D in 2, 5, 64, 100, 128; kind = "rand" (identity_init=False) or "trained" (identity
                      init perturbed the way a trained layer looks); part = params (parameters, log-determinants, parameter
                      gradients), fwd, inv (outputs of the two directions), gradf, gradi (input gradients of the two)
  lu_flow.npz         one small NSF-style flow [RandomPermutation, LULinear, RQ coupling] x 4
Every file is kept below 1 MiB (at most three [rows, D] float32 arrays each), so: the split above, the row counts below --
4 096 rows at D <= 5, 1 280 / 800 / 640 at D = 64 / 100 / 128 --, inputs regenerated from their seeds
(numpy's RandomState stream is frozen) and every float64 result stored as the float32 result plus a float32 difference
(`*_d`: float64 = float32 + difference, good to ~1e-14 -- the errors compared are 1e-8 and above).
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

from nflows.distributions.normal import StandardNormal  # noqa: E402
from nflows.flows.base import Flow  # noqa: E402
from nflows.nn.nets import ResidualNet  # noqa: E402
from nflows.transforms.base import CompositeTransform  # noqa: E402
from nflows.transforms.coupling import PiecewiseRationalQuadraticCouplingTransform  # noqa: E402
from nflows.transforms.lu import LULinear  # noqa: E402
from nflows.transforms.permutations import RandomPermutation  # noqa: E402
from nflows.utils.torchutils import create_alternating_binary_mask  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

ROWS = {2: 4096, 5: 4096, 64: 1280, 100: 800, 128: 640}
PARAMS = ("lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")


def lu_inputs(features, kind):
    """Inputs and the fixed weights r of the gradient's loss; the tests regenerate them from the same seeds."""
    rng = np.random.RandomState(1000 * features + (1 if kind == "rand" else 2))
    x = rng.randn(ROWS[features], features).astype(np.float32)
    r = rng.randn(ROWS[features], features).astype(np.float32)
    return x, r


def make_layer(features, kind):
    torch.manual_seed(features * 7 + (0 if kind == "rand" else 1))
    t = LULinear(features, identity_init=(kind != "rand"))
    if kind == "trained":
        with torch.no_grad():
            s = 0.9 / np.sqrt(features)
            t.lower_entries.uniform_(-s, s)
            t.upper_entries.uniform_(-s, s)
            t.unconstrained_upper_diag.add_(0.5 * torch.randn(features))
            t.bias.normal_()
    return t


def pair(out, name, v32, v64):
    v32 = v32.detach().numpy()
    out[name] = v32
    out[name + "_d"] = (v64.detach().numpy() - v32.astype(np.float64)).astype(np.float32)


def lu_case(out, features, kind):
    t = make_layer(features, kind)
    t64 = copy.deepcopy(t).double()
    pre = "%s/" % kind
    for n in PARAMS:
        out[pre + n] = getattr(t, n).detach().numpy().copy()
    xn, rn = lu_inputs(features, kind)
    x, r = torch.from_numpy(xn), torch.from_numpy(rn)
    with torch.no_grad():
        y, lad = t(x)
        y64, lad64 = t64(x.double())
        pair(out, pre + "y", y, y64)
        pair(out, pre + "lad", lad[:1], lad64[:1])
        xi, ladi = t.inverse(y)               # the inverse's input: the float32 forward output stored above
        xi64, ladi64 = t64.inverse(y.double())
        pair(out, pre + "xi", xi, xi64)
        pair(out, pre + "ladi", ladi[:1], ladi64[:1])
        out[pre + "cond"] = np.float64(torch.linalg.cond(t64.weight()).item())
        te = copy.deepcopy(t).eval()
        te.use_cache(True)
        yc, ladc = te(x)
        xic, ladic = te.inverse(y)
        out[pre + "y_cached"], out[pre + "lad_cached"] = yc.numpy(), ladc[:1].numpy()
        out[pre + "xi_cached"], out[pre + "ladi_cached"] = xic.numpy(), ladic[:1].numpy()
    for direction, source in (("grad_", x), ("gradinv_", y)):   # forward: loss of (y, lad) at x; inverse: of (x, ladi) at y
        grads = []
        for layer, dt in ((t, torch.float32), (t64, torch.float64)):
            layer.zero_grad()
            xin = source.detach().clone().to(dt).requires_grad_(True)
            yy, ll = layer(xin) if direction == "grad_" else layer.inverse(xin)
            ((yy * r.to(dt)).sum() + ll.sum()).backward()
            grads.append([xin.grad] + [getattr(layer, n).grad.clone() for n in PARAMS])
        for n, g32, g64 in zip(("inputs",) + PARAMS, *grads):
            pair(out, pre + direction + n, g32, g64)


def part_of(key):
    name = key.split("/", 1)[1]
    for stem, part in (("grad_inputs", "gradf"), ("gradinv_inputs", "gradi"), ("y", "fwd"), ("xi", "inv")):
        if name in (stem, stem + "_d", stem + "_cached"):
            return part
    return "params"


def make_flow(features=16, hidden=32, layers=4):
    torch.manual_seed(4)
    ts = []
    for i in range(layers):
        ts.append(RandomPermutation(features))
        ts.append(LULinear(features, identity_init=True))
        ts.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=create_alternating_binary_mask(features, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=hidden, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=3.0))
    flow = Flow(CompositeTransform(ts), StandardNormal([features]))
    with torch.no_grad():
        for name, p in flow.named_parameters():   # default init gives near-identity splines and identity LU layers
            if "final_layer" in name:
                p.mul_(4.0)
            elif "linear_layers.1" in name:
                p.mul_(30.0)
            elif name.endswith("lower_entries") or name.endswith("upper_entries"):
                p.uniform_(-0.9 / np.sqrt(features), 0.9 / np.sqrt(features))
            elif name.endswith("unconstrained_upper_diag"):
                p.add_(0.5 * torch.randn(features))
            elif name.endswith("bias") and p.shape == (features,) and "transform_net" not in name:
                p.normal_()
    return flow


def flow_case(out, rows=512):
    flow = make_flow().eval()
    flow64 = copy.deepcopy(flow).double()
    for k, v in flow.state_dict().items():
        out["state/" + k] = v.numpy().copy()
    x = torch.from_numpy(np.random.RandomState(77).randn(rows, 16).astype(np.float32))
    out["x"] = x.numpy()
    with torch.no_grad():
        pair(out, "log_prob", flow.log_prob(x), flow64.log_prob(x.double()))
        z, lad = flow._transform(x)
        z64, lad64 = flow64._transform(x.double())
        pair(out, "z", z, z64)
        pair(out, "lad", lad, lad64)
        xs, ladi = flow._transform.inverse(z)      # the sample side: noise -> data, from the float32 z stored above
        xs64, ladi64 = flow64._transform.inverse(z.double())
        pair(out, "x_from_z", xs, xs64)
        pair(out, "ladi", ladi, ladi64)


def main():
    for features in sorted(ROWS):
        for kind in ("rand", "trained"):
            out = {}
            lu_case(out, features, kind)
            for part in ("params", "fwd", "inv", "gradf", "gradi"):
                path = os.path.join(HERE, "lu_linear_d%d_%s_%s.npz" % (features, kind, part))
                np.savez(path, **{k: v for k, v in out.items() if part_of(k) == part})
                print(path, os.path.getsize(path))
                assert os.path.getsize(path) < 1 << 20
    out = {}
    flow_case(out)
    path = os.path.join(HERE, "lu_flow.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
