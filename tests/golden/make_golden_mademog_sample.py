#!/usr/bin/env python3
"""Golden vectors of the mixture-of-Gaussians MADE's sampler: the REAL reference (bayesiains/nflows, imported read-only as
make_golden_density.py does; its checkout is named by the environment variable NFLOWS_REFERENCE) run on the CPU.  Run in
the build container only:

    NFLOWS_REFERENCE=<checkout of bayesiains/nflows> python tests/golden/make_golden_mademog_sample.py

Writes mademog_sample.npz next to this script, data only: the reference's `MixtureOfGaussiansMADE.sample(1, context)`
(nn/nde/made.py:355-388) for 7 features, a context of 3, 5 components, 64 rows, weights scaled as in
tests/mog_sample_cases.py, with what the reference drew recorded on the way --
  state/*     the state_dict
  context     [64, 3]
  components  int64 [64, 7]: what `Categorical.sample` returned, step by step
  eps         [64, 7]: the `torch.randn` draws
  samples     float32 [64, 7]: what `sample` returned
  samples64   float64 [64, 7]: the same trajectory (same components, same draws) through the float64 copy of the module
  u           float32 [64, 7]: for every element the MIDDLE of the chosen component's interval of the float64 CDF of its step
              (on the float64 trajectory) -- a uniform that makes K30's selection rule choose what the reference drew.
The seed is the first from 4100 on for which every such interval is at least 2e-4 wide."""
import copy
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "_refshim"))
sys.path.insert(0, os.environ["NFLOWS_REFERENCE"])

import torch  # noqa: E402
from torch import distributions  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from nflows.nn.nde import MixtureOfGaussiansMADE  # noqa: E402

import mog_sample_cases as C  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

FEATURES, CONTEXT, COMPONENTS, HIDDEN, ROWS = 7, 3, 5, 32, 64
MIN_INTERVAL = 2e-4


def run(seed):
    torch.manual_seed(seed)
    made = MixtureOfGaussiansMADE(features=FEATURES, hidden_features=HIDDEN, context_features=CONTEXT, num_blocks=2,
                                  num_mixture_components=COMPONENTS, epsilon=C.EPSILON, custom_initialization=False)
    C.sharpen(made).eval()
    context = torch.randn(ROWS, CONTEXT)
    drawn_components, drawn_normals = [], []
    sample_was, randn_was = distributions.Categorical.sample, torch.randn

    def sample(self, sample_shape=torch.Size()):
        c = sample_was(self, sample_shape)
        drawn_components.append(c.reshape(-1).clone())
        return c

    def randn(*args, **kwargs):
        z = randn_was(*args, **kwargs)
        drawn_normals.append(z.clone())
        return z

    distributions.Categorical.sample, torch.randn = sample, randn
    try:
        samples = made.sample(1, context=context)
    finally:
        distributions.Categorical.sample, torch.randn = sample_was, randn_was
    assert len(drawn_components) == len(drawn_normals) == FEATURES
    components, eps = torch.stack(drawn_components, dim=1), torch.stack(drawn_normals, dim=1)
    samples = samples.reshape(ROWS, FEATURES)

    # the same trajectory in float64, and the chosen components' intervals of its CDFs
    made64 = copy.deepcopy(made).double()
    x = torch.zeros(ROWS, FEATURES, dtype=torch.float64)
    u = torch.zeros(ROWS, FEATURES, dtype=torch.float64)
    narrowest = float("inf")
    with torch.no_grad():
        for t in range(FEATURES):
            out = made64(x, context.double()).reshape(ROWS, FEATURES, COMPONENTS, 3)[:, t]
            c = components[:, t:t + 1]
            logits = out[..., 0]
            e = torch.exp(logits - logits.max(dim=-1, keepdim=True).values)
            run_sum = torch.cumsum(e, dim=-1)
            upper = (run_sum / run_sum[:, -1:]).gather(1, c)[:, 0]
            lower = upper - (e / run_sum[:, -1:]).gather(1, c)[:, 0]
            narrowest = min(narrowest, float((upper - lower).min()))
            u[:, t] = 0.5 * (lower + upper)
            std = F.softplus(out[..., 2].gather(1, c)[:, 0]) + made64.epsilon
            x[:, t] = out[..., 1].gather(1, c)[:, 0] + eps[:, t].double() * std
    return made, context, components, eps, samples, x, u.float(), narrowest


def main():
    seed = 4100
    while True:
        made, context, components, eps, samples, samples64, u, narrowest = run(seed)
        if narrowest >= MIN_INTERVAL:
            break
        print("seed %d: an interval of %.3g, next" % (seed, narrowest))
        seed += 1
    out = {"state/" + k: v.numpy().copy() for k, v in made.state_dict().items()}
    out.update(context=context.numpy(), components=components.numpy(), eps=eps.numpy(), samples=samples.numpy(),
               samples64=samples64.numpy(), u=u.numpy(), seed=np.int64(seed))
    for k, v in out.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    path = os.path.join(HERE, "mademog_sample.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "seed", seed, "narrowest interval", narrowest)
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
