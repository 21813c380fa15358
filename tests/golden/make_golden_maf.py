#!/usr/bin/env python3
"""Golden vectors of the masked autoregressive affine flows (K22): the REAL reference (bayesiains/nflows, imported
read-only as make_golden.py does) run on the CPU in float32 and float64.  Run in the build container only:

    python tests/golden/make_golden_maf.py

Writes flows_maf.npz next to this script, data only: for every case of tests/maf_cases.py the 256 input rows `x`, the
`context` where the case has one, `z`, `lad`, `log_prob` in float32 and `z64`, `lad64`, `log_prob64` in float64, and the
names and checksums of the reference's state_dict (weights, masks, degrees, permutations: configs.masked_affine_flow
rebuilds them from the seed, nothing of them is stored).  The flows are built like the reference's MaskedAutoregressiveFlow
factory builds its own -- per layer the permutation, then the layer -- from the reference's classes directly, because the
factory has no context argument and always permutes; the weights are then moved off the near-identity initialisation
(maf_cases.SHARPEN), as the RealNVP fixtures' are.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "_refshim"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

from nflows.distributions.normal import StandardNormal  # noqa: E402
from nflows.flows.base import Flow  # noqa: E402
from nflows.transforms.autoregressive import MaskedAffineAutoregressiveTransform  # noqa: E402
from nflows.transforms.base import CompositeTransform  # noqa: E402
from nflows.transforms.permutations import RandomPermutation, ReversePermutation  # noqa: E402

import maf_cases  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")


def reference_flow(features, hidden_features, num_layers, num_blocks, use_residual_blocks, seed, random_mask=False,
                   permutation=None, context_features=None):
    torch.manual_seed(seed)
    layers = []
    for _ in range(num_layers):
        if permutation is not None:
            layers.append({"reverse": ReversePermutation, "random": RandomPermutation}[permutation](features))
        layers.append(MaskedAffineAutoregressiveTransform(
            features=features, hidden_features=hidden_features, context_features=context_features,
            num_blocks=num_blocks, use_residual_blocks=use_residual_blocks, random_mask=random_mask))
    flow = Flow(CompositeTransform(layers), StandardNormal([features]))
    with torch.no_grad():
        for name, p in flow.named_parameters():
            if "final_layer" in name:
                p.mul_(maf_cases.SHARPEN["scale_final"])
            elif "linear_layers.1" in name:
                p.mul_(maf_cases.SHARPEN["scale_linear1"])
    return flow.eval()


def main():
    out = {}
    for name, cfg in maf_cases.CASES.items():
        flow = reference_flow(**cfg)
        x, context = maf_cases.fixture_inputs(name)
        with torch.no_grad():
            lp = flow.log_prob(x, context=context)
            z, lad = flow._transform(x, context=context)
            names, sums = maf_cases.checksums(flow.state_dict())
            f64 = flow.double()
            c64 = None if context is None else context.double()
            lp64 = f64.log_prob(x.double(), context=c64)
            z64, lad64 = f64._transform(x.double(), context=c64)
        vectors = dict(x=x, z=z, lad=lad, log_prob=lp, z64=z64, lad64=lad64, log_prob64=lp64)
        if context is not None:
            vectors["context"] = context
        for k, v in vectors.items():
            assert torch.isfinite(v).all(), (name, k)   # (no test may skip an element)
            out[name + "/" + k] = v.numpy()
        out[name + "/param_names"] = np.array(names).astype(str)
        out[name + "/param_checksums"] = sums
        scale = torch.nn.functional.softplus(torch.zeros(1)).item()
        print("   %s: |lad| mean %.2f (softplus(0) = %.2f), |z| max %.1f, |z - x| mean %.2f, reference fp32 vs fp64: z %.2e "
              "lad %.2e" % (name, float(lad64.abs().mean()), scale, float(z64.abs().max()),
                            float((z64 - x.double()).abs().mean()), float((z.double() - z64).abs().max()),
                            float((lad.double() - lad64).abs().max())))
    out["cases"] = np.array(list(maf_cases.CASES)).astype(str)
    path = os.path.join(HERE, "flows_maf.npz")
    np.savez_compressed(path, **out)
    print("flows_maf: %d cases, %d bytes" % (len(maf_cases.CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
