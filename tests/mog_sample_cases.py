"""The sampler of the mixture-of-Gaussians MADE (K30, csrc/made_inverse.hip): a restatement of
`nn.nde.MixtureOfGaussiansMADE.sample` that takes its randomness as inputs, the table of cases of the GPU and host tests,
and inputs built so that every decision is well-conditioned.

The restatement (`restated`) is the reference's loop (nn/nde/made.py:355-388) -- D passes of the whole masked network on
the samples so far -- with the Categorical draw replaced by K30's SELECTION RULE on a given uniform `u[row, t]`:
    m = max_k l_k, e_k = exp(l_k - m), S = e_0 + .. + e_{K-1} in index order;
    c = the smallest index whose running sum e_0 + .. + e_c exceeds u * S, K - 1 if none does;
    x_t = mean_c + eps[row, t] * (softplus(ustd_c) + epsilon).
In float64 it is the truth, in float32 on the CPU the yardstick (`maf_inverse_cases.assert_parity`).

Inputs with a margin (`conditioned_inputs`): the float64 trajectory is run, every u[row, t] within MARGIN of an interior
boundary of its step's float64 CDF is redrawn from a fixed stream, and so on until none is -- then an fp32 evaluation of the
logits (relative error ~1e-6) chooses the same component everywhere, no row needs excluding, every row is compared.
tests/test_mog_sample_host.py checks that the construction terminates for every case."""
import copy
import functools

import numpy as np
import torch
from torch.nn import functional as F

from maf_inverse_cases import assert_parity, error_figures  # noqa: F401  (the GPU and host files take them from here)

MARGIN = 1e-4
SCALES = dict(scale_final=3.0, scale_linear1=100.0)   # off the near-zero initialisation: the components differ
EPSILON = 1e-2

# name -> (features, components, hidden, blocks kind, context features, rows).  The smallest shapes that reach each path:
# K = 1 (no choice), K <= 8 (one pass of logit rows), K > 8 (two, the second partial at 10 and full at 16); H = 256 takes the
# pipelined dot product; B = 1 and 17 leave a ragged sixteen-sample group, 130 is more than one group per wave slot.  The
# parity rule compares error statistics with the fp32 yardstick's, which mean nothing over a handful of elements (at 1 x 2
# one element a last bit off beside a yardstick that happened to round both exactly is a "5 x" mean): the single row goes
# with the widest case and the two-feature cases get the rows, so every case compares at least 17 elements
CASES = {
    "d2_k1_h16_res_c1_b130": (2, 1, 16, "residual", 1, 130),
    "d7_k5_h32_res_c8_b17": (7, 5, 32, "residual", 8, 17),
    "d17_k16_h128_res_c8_b1": (17, 16, 128, "residual", 8, 1),
    "d7_k2_h16_ff_c1_b17": (7, 2, 16, "feedforward", 1, 17),
    "d17_k5_h32_ffrand_c8_b130": (17, 5, 32, "feedforward_random", 8, 130),
    "d2_k16_h128_ff_c8_b17": (2, 16, 128, "feedforward", 8, 17),
    "d7_k10_h256_ff_c8_b17": (7, 10, 256, "feedforward", 8, 17),
    "d7_k5_h128_res_c1_b130": (7, 5, 128, "residual", 1, 130),
}
CONTINUATION_CASE = "d7_k5_h128_res_c1_b130"   # its steps are cut at half the plan's block size
GROUP_CASE = "d7_k5_h128_res_c1_b130"          # 128 / 6 = 21 units per Linear and step: groups of eight apply


def sharpen(module):
    with torch.no_grad():
        for pname, p in module.named_parameters():
            if "final_layer" in pname:
                p.mul_(SCALES["scale_final"])
            elif "linear_layers.1" in pname:
                p.mul_(SCALES["scale_linear1"])
    return module


def build(name, made_class=None):
    """The module of a case on the CPU in float32, eval mode; `made_class`: MixtureOfGaussiansMADE of another package."""
    if made_class is None:
        from nflows_amd.nn.nde import MixtureOfGaussiansMADE as made_class
    D, K, H, kind, ce, _ = CASES[name]
    torch.manual_seed(3000 + sorted(CASES).index(name))
    made = made_class(features=D, hidden_features=H, context_features=ce, num_blocks=2, num_mixture_components=K,
                      use_residual_blocks=kind == "residual", random_mask=kind == "feedforward_random", epsilon=EPSILON,
                      custom_initialization=False)
    return sharpen(made).eval()


def select(logits, u):
    """THE SELECTION RULE on [B, K] logits and [B] uniforms: (components int64 [B], interior CDF boundaries [B, K - 1])."""
    m = logits.max(dim=-1, keepdim=True).values
    e = torch.exp(logits - m)
    run = torch.cumsum(e, dim=-1)                      # (index order)
    total = run[:, -1]
    exceeds = run > (u * total)[:, None]               # monotone: e_k >= 0
    K = logits.shape[1]
    c = (~exceeds).sum(dim=-1).clamp(max=K - 1)        # the first index that exceeds, K - 1 if none does
    return c, run[:, :-1] / total[:, None]


def restated(made, context, u, eps, components=None):
    """(samples [B, D], components [B, D], distance of every u to the nearest interior CDF boundary [B, D]) in the dtype of
    `made`'s weights.  `components`: take these instead of choosing (the replay of a recorded trajectory)."""
    dtype = made.final_layer.weight.dtype
    context, u, eps = context.to(dtype), u.to(dtype), eps.to(dtype)
    B, D, K = context.shape[0], made.features, made.num_mixture_components
    x = torch.zeros(B, D, dtype=dtype)
    chosen = torch.zeros(B, D, dtype=torch.int64)
    gap = torch.full((B, D), float("inf"), dtype=dtype)
    with torch.no_grad():
        for t in range(D):
            out = made.forward(x, context).reshape(B, D, K, 3)[:, t]
            c, bounds = select(out[..., 0], u[:, t])
            if components is not None:
                c = components[:, t].to(torch.int64)
            if K > 1:
                gap[:, t] = (bounds - u[:, t, None]).abs().min(dim=-1).values
            mean = out[..., 1].gather(1, c[:, None])[:, 0]
            std = F.softplus(out[..., 2].gather(1, c[:, None])[:, 0]) + made.epsilon
            x[:, t] = mean + eps[:, t] * std
            chosen[:, t] = c
    return x, chosen, gap


def conditioned_inputs(made64, context, rows, seed, max_rounds=64):
    """(u, eps) float32 [rows, D] with every u at least MARGIN from the interior boundaries of its step's float64 CDF and
    below 1 - MARGIN, and the number of rounds the construction took."""
    g = torch.Generator().manual_seed(seed)
    D = made64.features
    u = torch.rand(rows, D, generator=g) * (1.0 - 2 * MARGIN)
    eps = torch.randn(rows, D, generator=g)
    for rounds in range(1, max_rounds + 1):
        _, _, gap = restated(made64, context, u, eps)
        near = gap < MARGIN
        if not near.any():
            return u, eps, rounds
        fresh = torch.rand(int(near.sum()), generator=g) * (1.0 - 2 * MARGIN)
        u = u.clone()
        u[near] = fresh
    raise AssertionError("no well-conditioned uniforms after %d rounds" % max_rounds)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's module, inputs and both restatements, computed once: dict(made, context, u, eps, x32, x64, components)."""
    made = build(name)
    D, K, H, kind, ce, rows = CASES[name]
    context = torch.randn(rows, ce, generator=torch.Generator().manual_seed(77 + rows))
    made64 = copy.deepcopy(made).double()
    u, eps, rounds = conditioned_inputs(made64, context, rows, seed=500 + D + K)
    x64, c64, gap = restated(made64, context, u, eps)
    x32, c32, _ = restated(made, context, u, eps)
    assert float(gap.min()) >= MARGIN and torch.equal(c32, c64), name
    return dict(made=made, context=context, u=u, eps=eps, rounds=rounds, x32=x32.numpy(), x64=x64.numpy(),
                components=c64.numpy())
