#!/usr/bin/env python3
"""Golden vectors of the image transforms -- OneByOneConvolution, SqueezeTransform and a Glow-style step built from
them: the REAL reference (bayesiains/nflows, imported read-only as make_golden_lu.py does) run on the CPU in float32 and
float64.  Run in the build container only:

    python tests/golden/make_golden_conv.py

Writes, next to this script, data only:
  conv1x1_c{C}_{kind}_{part}.npz  the shapes of SHAPES; kind = "rand" (identity_init=False) or "trained" (identity init
                      perturbed as in make_golden_lu.py); part = out (parameters, the permutation, log-determinants,
                      parameter gradients, outputs of the two directions) or grad (input gradients of the two)
  squeeze.npz         SqueezeTransform: forward of (2, 3, 4, 6) factor 2 and (3, 2, 9, 6) factor 3 and their inverses.
                      The reference's inverse refuses every channel count that is not a multiple of 4, whatever the
                      factor, so the inverse of the factor-3 output (18 channels) is recorded as "raises"; a factor-3
                      inverse that the reference does serve, on 36 channels, is stored beside it.
  conv_flow.npz       [SqueezeTransform(2), (ActNorm(12), OneByOneConvolution(12), RQ coupling with an alternating
                      channel mask and a ConvResidualNet) x 2] on [16, 3, 8, 8]
Every file is kept below 1 MiB, inputs are regenerated from their seeds (numpy's RandomState stream is frozen) and every
float64 result is stored as the float32 result plus a float32 difference (`*_d`: float64 = float32 + difference).
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

from nflows.nn.nets import ConvResidualNet  # noqa: E402
from nflows.transforms.base import CompositeTransform  # noqa: E402
from nflows.transforms.conv import OneByOneConvolution  # noqa: E402
from nflows.transforms.coupling import PiecewiseRationalQuadraticCouplingTransform  # noqa: E402
from nflows.transforms.normalization import ActNorm  # noqa: E402
from nflows.transforms.reshape import SqueezeTransform  # noqa: E402
from nflows.utils.torchutils import create_alternating_binary_mask  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

SHAPES = ((2, 37, 5, 3), (3, 10, 28, 28), (12, 9, 16, 16), (48, 21, 4, 4), (100, 3, 7, 9), (128, 5, 8, 8))   # (C, B, H, W)
PARAMS = ("lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")


def conv_inputs(shape, kind):
    """Inputs and the fixed weights r of the gradient's loss; the tests regenerate them from the same seeds."""
    c, b, h, w = shape
    rng = np.random.RandomState(1000 * c + (1 if kind == "rand" else 2))
    x = rng.randn(b, c, h, w).astype(np.float32)
    r = rng.randn(b, c, h, w).astype(np.float32)
    return x, r


def layer_seed(channels, kind):
    return channels * 7 + (0 if kind == "rand" else 1)


def make_layer(channels, kind):
    torch.manual_seed(layer_seed(channels, kind))
    t = OneByOneConvolution(channels, identity_init=(kind != "rand"))   # (the permutation is drawn here, after the parameters)
    if kind == "trained":
        with torch.no_grad():
            s = 0.9 / np.sqrt(channels)
            t.lower_entries.uniform_(-s, s)
            t.upper_entries.uniform_(-s, s)
            t.unconstrained_upper_diag.add_(0.5 * torch.randn(channels))
            t.bias.normal_()
    return t


def pair(out, name, v32, v64):
    v32 = v32.detach().numpy()
    out[name] = v32
    out[name + "_d"] = (v64.detach().numpy() - v32.astype(np.float64)).astype(np.float32)


def conv_case(out, shape, kind):
    t = make_layer(shape[0], kind)
    t64 = copy.deepcopy(t).double()
    pre = "%s/" % kind
    for n in PARAMS:
        out[pre + n] = getattr(t, n).detach().numpy().copy()
    out[pre + "permutation._permutation"] = t.permutation._permutation.numpy().copy()
    xn, rn = conv_inputs(shape, kind)
    x, r = torch.from_numpy(xn), torch.from_numpy(rn)
    with torch.no_grad():
        y, lad = t(x)
        y64, lad64 = t64(x.double())
        pair(out, pre + "y", y, y64)
        pair(out, pre + "lad", lad, lad64)
        xi, ladi = t.inverse(y)               # the inverse's input: the float32 forward output stored above
        xi64, ladi64 = t64.inverse(y.double())
        pair(out, pre + "xi", xi, xi64)
        pair(out, pre + "ladi", ladi, ladi64)
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
    return "grad" if name in ("grad_inputs", "grad_inputs_d", "gradinv_inputs", "gradinv_inputs_d") else "out"


def squeeze_case(out):
    for name, shape, factor in (("f2", (2, 3, 4, 6), 2), ("f3", (3, 2, 9, 6), 3)):
        t = SqueezeTransform(factor)
        x = torch.from_numpy(np.random.RandomState(10 + factor).randn(*shape).astype(np.float32))
        y, lad = t(x)
        out[name + "/x"], out[name + "/y"], out[name + "/lad"] = x.numpy(), y.numpy(), lad.numpy()
        try:
            back, ladi = t.inverse(y)
            out[name + "/inverse_of_y"], out[name + "/ladi"] = back.numpy(), ladi.numpy()
            out[name + "/inverse_raises"] = np.array("")
        except ValueError as e:
            out[name + "/inverse_raises"] = np.array(str(e))
    t = SqueezeTransform(3)
    v = torch.from_numpy(np.random.RandomState(20).randn(2, 36, 3, 2).astype(np.float32))
    back, ladi = t.inverse(v)
    out["f3/v"], out["f3/inverse_of_v"], out["f3/ladi_v"] = v.numpy(), back.numpy(), ladi.numpy()


def make_flow(channels=12, hidden=8, steps=2):
    torch.manual_seed(5)
    ts = [SqueezeTransform(2)]
    for i in range(steps):
        ts.append(ActNorm(channels))
        ts.append(OneByOneConvolution(channels))
        ts.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=create_alternating_binary_mask(channels, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ConvResidualNet(i_, o_, hidden_channels=hidden, num_blocks=1),
            num_bins=4, tails="linear", tail_bound=3.0))
    flow = CompositeTransform(ts)
    with torch.no_grad():
        for name, p in flow.named_parameters():   # default init gives near-identity splines and identity 1x1 convolutions
            if "final_layer" in name:
                p.mul_(4.0)
            elif "conv_layers.1" in name:
                p.mul_(30.0)
            elif name.endswith("lower_entries") or name.endswith("upper_entries"):
                p.uniform_(-0.9 / np.sqrt(channels), 0.9 / np.sqrt(channels))
            elif name.endswith("unconstrained_upper_diag"):
                p.add_(0.5 * torch.randn(channels))
            elif name.endswith("log_scale"):
                p.copy_(0.2 * torch.randn(channels))
            elif (name.endswith("bias") or name.endswith("shift")) and p.shape == (channels,) and "transform_net" not in name:
                p.normal_()
        for m in flow.modules():
            if isinstance(m, ActNorm):
                m.initialized.data = torch.tensor(True, dtype=torch.bool)
    return flow


def flow_case(out):
    flow = make_flow().eval()
    flow64 = copy.deepcopy(flow).double()
    for k, v in flow.state_dict().items():
        out["state/" + k] = v.numpy().copy()
    x = torch.from_numpy(np.random.RandomState(78).randn(16, 3, 8, 8).astype(np.float32))
    out["x"] = x.numpy()
    with torch.no_grad():
        z, lad = flow(x)
        z64, lad64 = flow64(x.double())
        pair(out, "z", z, z64)
        pair(out, "lad", lad, lad64)
        xs, ladi = flow.inverse(z)      # noise -> data, from the float32 z stored above
        xs64, ladi64 = flow64.inverse(z.double())
        pair(out, "x_from_z", xs, xs64)
        pair(out, "ladi", ladi, ladi64)


def save(name, out):
    path = os.path.join(HERE, name)
    np.savez(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def main():
    for shape in SHAPES:
        for kind in ("rand", "trained"):
            out = {}
            conv_case(out, shape, kind)
            for part in ("out", "grad"):
                save("conv1x1_c%d_%s_%s.npz" % (shape[0], kind, part), {k: v for k, v in out.items() if part_of(k) == part})
    out = {}
    squeeze_case(out)
    save("squeeze.npz", out)
    out = {}
    flow_case(out)
    save("conv_flow.npz", out)


if __name__ == "__main__":
    main()
