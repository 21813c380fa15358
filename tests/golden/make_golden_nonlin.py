#!/usr/bin/env python3
"""Golden vectors of the elementwise nonlinearity transforms: the REAL reference (bayesiains/nflows, imported read-only as
make_golden_norm.py does; its checkout is named by the environment variable NFLOWS_REFERENCE) run on the CPU in float32
and float64.  Run in the build container only:

    NFLOWS_REFERENCE=<checkout of bayesiains/nflows> python tests/golden/make_golden_nonlin.py

Writes, next to this script, data only:
  nonlin_{kind}_n{N}_{part}.npz   kind in exp, tanh, logtanh (cut point 1), leaky (slope 0.1), sigmoid, sigmoid_t
                      (temperature 2.5, learnable), cauchy; [rows, N] in 4093 x 1, 4093 x 5, 1021 x 67, 381 x 256, 23 x 4100
                      and the image 37 x 3 x 5 x 7 (N written 3x5x7); part = fwd (y, lad of the forward pass), inv (x, lad of
                      the inverse pass at the reference's own float32 forward outputs), and at N = 5, 67, 4100 grad / gradi
                      (gradients of sum(y * r) + sum(logabsdet) of the forward / the inverse pass with respect to the
                      inputs, for sigmoid_t also to `temperature`)
  nonlin_flow.npz     data in (0, 1) -> Logit -> two rational-quadratic couplings with a permutation between them ->
                      StandardNormal: the state_dict, 512 rows' log_prob
Every file is kept below 1 MiB; inputs are regenerated from their seeds (`nonlin_inputs`: numpy's RandomState stream is
frozen) -- N(0, 1.5^2) clipped to +-4, where every float32 result of the reference is finite, which is asserted for
everything written -- and every float64 result is stored as the float32 result plus a float32 difference (`*_d`).

One float64 result is not the reference's own: LeakyReLU's logabsdet.  The reference forms it from a float32 mask
(`.type(torch.Tensor)`) and a float32 `log_negative_slope` attribute that `.double()` does not reach, so its "float64" run
returns the float32 number again and the yardstick would be zero.  The float64 logabsdet written here is the quantity
itself, (number of negative elements of the row) x log(slope) in float64 (`leaky_logabsdet64`).
"""
import copy
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "_refshim"))
sys.path.insert(0, os.environ["NFLOWS_REFERENCE"])

import torch  # noqa: E402

from nflows.distributions.normal import StandardNormal  # noqa: E402
from nflows.flows.base import Flow  # noqa: E402
from nflows.nn.nets import ResidualNet  # noqa: E402
from nflows.transforms import nonlinearities as ref  # noqa: E402
from nflows.transforms.base import CompositeTransform  # noqa: E402
from nflows.transforms.coupling import PiecewiseRationalQuadraticCouplingTransform  # noqa: E402
from nflows.transforms.permutations import ReversePermutation  # noqa: E402
from nflows.utils import torchutils  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

KINDS = ("exp", "tanh", "logtanh", "leaky", "sigmoid", "sigmoid_t", "cauchy")
SHAPES = ((4093, 1), (4093, 5), (1021, 67), (381, 256), (23, 4100), (37, 3, 5, 7))
GRAD_N = (5, 67, 4100)


def make(kind):
    if kind == "exp":
        return ref.Exp()
    if kind == "tanh":
        return ref.Tanh()
    if kind == "logtanh":
        return ref.LogTanh(cut_point=1)
    if kind == "leaky":
        return ref.LeakyReLU(negative_slope=0.1)
    if kind == "sigmoid":
        return ref.Sigmoid()
    if kind == "sigmoid_t":
        return ref.Sigmoid(temperature=2.5, learn_temperature=True)
    return ref.CauchyCDF()


def leaky_logabsdet64(t, inputs, inverse):
    count = (inputs.double() < 0).double().reshape(inputs.shape[0], -1).sum(1)
    return count * ((-1.0 if inverse else 1.0) * float(np.log(t.negative_slope)))


def tag(shape):
    return "x".join(str(s) for s in shape[1:])


def nonlin_inputs(kind, shape):
    """Forward inputs and the weights r of the gradient's loss; the tests regenerate them."""
    rng = np.random.RandomState(7000 + 100 * KINDS.index(kind) + int(np.prod(shape[1:])) % 97)
    x = np.clip(1.5 * rng.randn(*shape), -4.0, 4.0).astype(np.float32)
    r = rng.randn(*shape).astype(np.float32)
    return x, r


def pair(out, name, v32, v64):
    v32 = v32.detach().numpy()
    v64 = v64.detach().numpy()
    assert np.isfinite(v32).all() and np.isfinite(v64).all(), name
    out[name] = v32
    out[name + "_d"] = (v64 - v32.astype(np.float64)).astype(np.float32)


def save(path, arrays):
    np.savez(path, **arrays)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def grads(out, layers, source, r, inverse):
    got = []
    for layer, dt in zip(layers, (torch.float32, torch.float64)):
        layer.zero_grad()
        xin = source.detach().clone().to(dt).requires_grad_(True)
        y, lad = layer.inverse(xin) if inverse else layer(xin)
        ((y * r.to(dt)).sum() + lad.sum()).backward()
        g = {"inputs": xin.grad}
        if isinstance(getattr(layer, "temperature", None), torch.nn.Parameter):
            g["temperature"] = layer.temperature.grad.clone()
        got.append(g)
    for n in got[0]:
        pair(out, n, got[0][n], got[1][n])


def case(kind, shape):
    t = make(kind)
    t64 = copy.deepcopy(t).double()
    xn, rn = nonlin_inputs(kind, shape)
    x, r = torch.from_numpy(xn), torch.from_numpy(rn)
    stem = os.path.join(HERE, "nonlin_%s_n%s_" % (kind, tag(shape)))
    with torch.no_grad():
        fwd = {}
        (y, lad), (y64, lad64) = t(x), t64(x.double())
        assert lad.shape == (shape[0],)
        if kind == "leaky":
            lad64 = leaky_logabsdet64(t, x, False)
        pair(fwd, "y", y, y64)
        pair(fwd, "lad", lad, lad64)
        save(stem + "fwd.npz", fwd)
        inv = {}
        (xi, ladi), (xi64, ladi64) = t.inverse(y), t64.inverse(y.double())   # at the float32 forward output
        if kind == "leaky":
            ladi64 = leaky_logabsdet64(t, y, True)
        pair(inv, "x", xi, xi64)
        pair(inv, "lad", ladi, ladi64)
        save(stem + "inv.npz", inv)
    if len(shape) == 2 and shape[1] in GRAD_N:
        for part, inverse, source in (("grad", False, x), ("gradi", True, y)):
            out = {}
            grads(out, (t, t64), source, r, inverse)
            save(stem + part + ".npz", out)


def flow_case():
    D, H, K = 6, 32, 8
    torch.manual_seed(31)
    layers = [ref.Logit()]
    for i in range(2):
        layers.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=torchutils.create_alternating_binary_mask(D, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=H, num_blocks=2),
            num_bins=K, tails="linear", tail_bound=4.0))
        if i == 0:
            layers.append(ReversePermutation(D))
    flow = Flow(CompositeTransform(layers), StandardNormal([D]))
    with torch.no_grad():   # away from the near-identity initial splines
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.add_(0.5 * torch.randn_like(p))
    flow.eval()
    flow64 = copy.deepcopy(flow).double()
    out = {}
    for k, v in flow.state_dict().items():
        out["state/" + k] = v.numpy().copy()
    rng = np.random.RandomState(7999)
    x = torch.from_numpy(rng.uniform(0.01, 0.99, size=(512, D)).astype(np.float32))
    with torch.no_grad():
        pair(out, "log_prob", flow.log_prob(x), flow64.log_prob(x.double()))
    save(os.path.join(HERE, "nonlin_flow.npz"), out)


def main():
    for kind in KINDS:
        for shape in SHAPES:
            case(kind, shape)
    flow_case()


if __name__ == "__main__":
    main()
