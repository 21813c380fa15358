#!/usr/bin/env python3
"""Golden vectors of the learned base densities: the REAL reference (bayesiains/nflows, imported read-only as
make_golden_nonlin.py does; its checkout is named by the environment variable NFLOWS_REFERENCE) run on the CPU in float32
and float64.  Run in the build container only:

    NFLOWS_REFERENCE=<checkout of bayesiains/nflows> python tests/golden/make_golden_density.py

Writes, next to this script, data only:
  density_diag_{shared,row}_{B}x{N}.npz   DiagonalNormal (shared [1, N] parameters) / ConditionalDiagonalNormal behind the
                      identity encoder (the [B, 2 N] parameters are the context) at 517 x 1, 517 x 5, 129 x 67, 37 x 3 x 5 x 7
                      and 9 x 4100: log_prob, and the gradients of sum(log_prob * r) with respect to the inputs and the
                      parameters (shared: means, log_stds; row: the [B, 2 N] tensor).  DiagonalNormal broadcasts its [1, N]
                      parameters against the inputs, which serves one-dimensional shapes only: the image case runs it on the
                      flattened [37, 105] view, the same numbers.
  density_mog_{plain,wide}_{B}x{D}x{K}.npz   MixtureOfGaussiansMADE.log_prob (nn/nde/made.py:328-353; its `forward` replaced
                      by the given [B, D * K * 3] tensor, everything behind it the reference's own lines) at 517 x 1 x 1,
                      517 x 5 x 5, 129 x 67 x 3, 33 x 7 x 64, 5 x 2100 x 2 and "wide" at 129 x 5 x 5 (logits of +-30,
                      unconstrained stds down to -30, x 50 standard deviations from every mean): log_prob, and the gradients
                      of sum(log_prob * r) with respect to the inputs and that tensor
  density_mademog.npz MADEMoG(7 features, context 3, 5 components): the state_dict, 64 rows' log_prob
  density_flow.npz    two rational-quadratic couplings with a context -> ConditionalDiagonalNormal with a Linear encoder:
                      the state_dict, 512 rows' log_prob
Every file is kept below 1 MiB; the operands are regenerated from their seeds (tests/density_cases.py: numpy's RandomState
stream is frozen), every float32 and float64 result of the reference is finite, which is asserted for everything written,
and every float64 result is stored as the float32 result plus a float32 difference (`*_d`).
"""
import copy
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "_refshim"))
sys.path.insert(0, os.environ["NFLOWS_REFERENCE"])

import torch  # noqa: E402

from nflows.distributions import ConditionalDiagonalNormal, DiagonalNormal, MADEMoG  # noqa: E402
from nflows.flows.base import Flow  # noqa: E402
from nflows.nn.nde import MixtureOfGaussiansMADE  # noqa: E402
from nflows.nn.nets import ResidualNet  # noqa: E402
from nflows.transforms.base import CompositeTransform  # noqa: E402
from nflows.transforms.coupling import PiecewiseRationalQuadraticCouplingTransform  # noqa: E402
from nflows.transforms.permutations import ReversePermutation  # noqa: E402
from nflows.utils.torchutils import create_alternating_binary_mask  # noqa: E402

import density_cases as C  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")


def pair(out, name, v32, v64):
    v32 = v32.detach().numpy()
    v64 = v64.detach().numpy()
    assert np.isfinite(v32).all() and np.isfinite(v64).all(), name
    out[name] = v32
    out[name + "_d"] = (v64 - v32.astype(np.float64)).astype(np.float32)


def save(name, arrays):
    path = os.path.join(HERE, "density_%s.npz" % name)
    np.savez(path, **arrays)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def both(run, operands, r):
    """run(dtype, *operands as leaf tensors of that dtype) -> log_prob; log_prob and the gradients of sum(log_prob * r)."""
    got = []
    for dt in (torch.float32, torch.float64):
        leaves = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in operands]
        lp = run(dt, *leaves)
        assert lp.shape == (len(r),)
        (lp * torch.from_numpy(r).to(dt)).sum().backward()
        got.append([lp] + [t.grad for t in leaves])
    return got


def diag_case(mode, shape):
    n = int(np.prod(shape[1:]))
    if mode == "shared":
        x, r, means, log_stds = C.diag_inputs(mode, shape)

        def run(dt, xt, mt, lt):
            d = DiagonalNormal([n]).to(dt)
            del d.mean_, d.log_std_
            d.mean_, d.log_std_ = mt, lt
            return d.log_prob(xt.reshape(shape[0], n))
        names, operands = ("g_x", "g_means", "g_log_stds"), (x, means, log_stds)
    else:
        x, r, params = C.diag_inputs(mode, shape)

        def run(dt, xt, pt):
            return ConditionalDiagonalNormal(list(shape[1:])).to(dt).log_prob(xt, context=pt)
        names, operands = ("g_x", "g_params"), (x, params)
    got32, got64 = both(run, operands, r)
    out = {}
    for name, a, b in zip(("log_prob",) + names, got32, got64):
        pair(out, name, a, b)
    save("diag_%s_%s" % (mode, C.tag(shape)), out)


def mog_case(kind, shape):
    B, D, K = shape
    x, r, outputs = C.mog_inputs(kind, shape)

    def run(dt, xt, ot):
        made = MixtureOfGaussiansMADE(features=D, hidden_features=8, num_mixture_components=K, epsilon=C.EPSILON).to(dt)
        made.forward = types.MethodType(lambda self, inputs, context=None: ot, made)
        return made.log_prob(xt)
    got32, got64 = both(run, (x, outputs), r)
    out = {}
    for name, a, b in zip(("log_prob", "g_x", "g_outputs"), got32, got64):
        pair(out, name, a, b)
    save("mog_%s_%s" % (kind, C.tag(shape)), out)


def state(module):
    return {"state/" + k: v.numpy().copy() for k, v in module.state_dict().items()}


def mademog_case():
    torch.manual_seed(41)
    d = MADEMoG(**C.MADEMOG)
    with torch.no_grad():   # away from the near-zero initial blocks and a bland output layer
        for name, p in d.named_parameters():
            if "final_layer" in name or "linear_layers.1" in name:
                p.add_(0.5 * torch.randn_like(p))
    d.eval()
    d64 = copy.deepcopy(d).double()
    out = state(d)
    x, ctx = (torch.from_numpy(a) for a in C.module_inputs("mademog"))
    with torch.no_grad():
        pair(out, "log_prob", d.log_prob(x, context=ctx), d64.log_prob(x.double(), context=ctx.double()))
    save("mademog", out)


def flow_case():
    nf = types.SimpleNamespace(PiecewiseRationalQuadraticCouplingTransform=PiecewiseRationalQuadraticCouplingTransform,
                               create_alternating_binary_mask=create_alternating_binary_mask, ResidualNet=ResidualNet,
                               ReversePermutation=ReversePermutation, Flow=Flow, CompositeTransform=CompositeTransform,
                               ConditionalDiagonalNormal=ConditionalDiagonalNormal)
    torch.manual_seed(43)
    flow = C.conditional_flow(nf)
    with torch.no_grad():   # away from the near-identity initial splines
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.add_(0.5 * torch.randn_like(p))
    flow.eval()
    flow64 = copy.deepcopy(flow).double()
    out = state(flow)
    x, ctx = (torch.from_numpy(a) for a in C.module_inputs("flow"))
    with torch.no_grad():
        pair(out, "log_prob", flow.log_prob(x, context=ctx), flow64.log_prob(x.double(), context=ctx.double()))
    save("flow", out)


def main():
    for mode in C.DIAG_MODES:
        for shape in C.DIAG_SHAPES:
            diag_case(mode, shape)
    for kind, shape in C.MOG_CASES:
        mog_case(kind, shape)
    mademog_case()
    flow_case()


if __name__ == "__main__":
    main()
