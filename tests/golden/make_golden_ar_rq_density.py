#!/usr/bin/env python3
"""Golden vectors of the density pass of autoregressive rational-quadratic spline flows (K29): the REAL reference
(bayesiains/nflows, imported read-only as make_golden_ar_rq_ctx.py does) run on the CPU in float32 and float64.  Run in the
build container only:

    python tests/golden/make_golden_ar_rq_density.py

Writes flows_ar_rq_density.npz next to this script, data only: for every flow of tests/ar_spline_density_cases.FIXTURE 256
rows `x`, the `context` where the flow has one, the reference's `z`, `lad` (flow._transform) and `log_prob` in float32 and
`z64`, `lad64`, `log_prob64` after `.double()`, and the names and checksums of the reference's state_dict (weights, masks,
degrees, permutations: ar_spline_density_cases.build rebuilds them from the seed, nothing of them is stored).  The flows
are stacks of the reference's MaskedPiecewiseRationalQuadraticAutoregressiveTransform with linear tails, per layer the
permutation, then the layer; the weights are then moved off the near-identity initialisation (ar_spline_sample_cases.SCALES).
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402

from nflows.distributions.normal import StandardNormal  # noqa: E402
from nflows.flows.base import Flow  # noqa: E402
from nflows.transforms.autoregressive import MaskedPiecewiseRationalQuadraticAutoregressiveTransform  # noqa: E402
from nflows.transforms.base import CompositeTransform  # noqa: E402
from nflows.transforms.permutations import RandomPermutation, ReversePermutation  # noqa: E402

import ar_spline_density_cases as C  # noqa: E402
import ar_spline_sample_cases as S  # noqa: E402
import maf_cases  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")


def reference_flow(features, hidden_features, context_features, num_bins, num_layers, permutation, seed, **kw):
    torch.manual_seed(seed)
    layers = []
    for _ in range(num_layers):
        if permutation is not None:
            layers.append({"reverse": ReversePermutation, "random": RandomPermutation}[permutation](features))
        layers.append(MaskedPiecewiseRationalQuadraticAutoregressiveTransform(
            features=features, hidden_features=hidden_features, context_features=context_features, num_bins=num_bins,
            tails="linear", tail_bound=C.TAIL_BOUND, **kw))
    flow = Flow(CompositeTransform(layers), StandardNormal([features]))
    return S.sharpen(flow).eval()


def main():
    out = {}
    for name, cfg in C.FIXTURE.items():
        flow = reference_flow(**cfg)
        x, context = C.inputs(name, rows=C.FIXTURE_ROWS)
        with torch.no_grad():
            z, lad = flow._transform(x, context=context)
            lp = flow.log_prob(x, context=context)
            names, sums = maf_cases.checksums(flow.state_dict())
            f64 = flow.double()
            c64 = None if context is None else context.double()
            z64, lad64 = f64._transform(x.double(), context=c64)
            lp64 = f64.log_prob(x.double(), context=c64)
        vectors = dict(x=x, z=z, lad=lad, log_prob=lp, z64=z64, lad64=lad64, log_prob64=lp64)
        if context is not None:
            vectors["context"] = context
        for k, v in vectors.items():
            assert torch.isfinite(v).all(), (name, k)   # (no test may skip an element)
            out[name + "/" + k] = v.numpy()
        out[name + "/param_names"] = np.array(names).astype(str)
        out[name + "/param_checksums"] = sums
        print("   %s: |lad| mean %.2f, |z - x| mean %.2f max %.2f, reference fp32 vs fp64: z %.2e lad %.2e log_prob %.2e"
              % (name, float(lad64.abs().mean()), float((z64 - x.double()).abs().mean()),
                 float((z64 - x.double()).abs().max()), float((z.double() - z64).abs().max()),
                 float((lad.double() - lad64).abs().max()), float((lp.double() - lp64).abs().max())))
    out["cases"] = np.array(list(C.FIXTURE)).astype(str)
    path = os.path.join(HERE, "flows_ar_rq_density.npz")
    np.savez_compressed(path, **out)
    print("flows_ar_rq_density: %d cases, %d bytes" % (len(C.FIXTURE), os.path.getsize(path)))


if __name__ == "__main__":
    main()
