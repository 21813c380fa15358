"""Cases of K31 (csrc/made_mog.hip: MixtureOfGaussiansMADE.log_prob in one launch), shared by tests/test_gpu_mog_density.py
and tests/test_mog_density_host.py: seeded modules, their inputs, and per case the float64 truth and the fp32 yardstick
(the module itself on the CPU: the reference's sequence), computed once."""
import copy
import functools

import torch

from nflows_amd.nn.nde import MixtureOfGaussiansMADE

# name: (features, components, context features, hidden width, blocks, residual, random mask, rows)
CASES = {
    "d1_k1_b1": (1, 1, None, 128, 1, True, False, 128),            # the log-softmax is exactly 0
    "d5_k5_c3": (5, 5, 3, 128, 2, True, False, 256),               # odd: a dead lane-half; T = 1
    "d32_k6_c17_b3": (32, 6, 17, 128, 3, True, False, 256),        # T = 2; two context k-steps; two initial k-steps
    "d33_k10_ragged": (33, 10, None, 128, 2, True, False, 130),    # four initial k-steps; no context; a ragged batch
    "d64_k11_c64_b1": (64, 11, 64, 128, 1, True, False, 256),      # T = 3
    "d8_k16_c3": (8, 16, 3, 128, 2, True, False, 256),
    "d7_k5_c3_ff": (7, 5, 3, 128, 2, False, False, 256),           # the raw initial layer in front of feed-forward blocks
    "d7_k10_ff_random": (7, 10, None, 128, 2, False, True, 256),
    "d6_k5_c3_h20": (6, 5, 3, 20, 2, True, False, 256),            # zero padding, no multiple of 16
    "d6_k10_c3_h64_ff": (6, 10, 3, 64, 2, False, False, 256),
    "d5_k5_c3_wide": (5, 5, 3, 128, 2, True, False, 256),          # logits to +-30, unconstrained stds down to -30
    "d4_k17_c3_old_path": (4, 17, 3, 128, 2, True, False, 256),    # above what K31 serves
}
EPSILON = 1e-2


def build(name):
    D, K, C, H, blocks, residual, random_mask, _ = CASES[name]
    torch.manual_seed(sorted(CASES).index(name) + 31)
    made = MixtureOfGaussiansMADE(features=D, hidden_features=H, context_features=C, num_blocks=blocks,
                                  num_mixture_components=K, use_residual_blocks=residual, random_mask=random_mask,
                                  epsilon=EPSILON, custom_initialization=True)
    with torch.no_grad():
        for pname, p in made.named_parameters():
            if "linear_layers.1" in pname:     # (initialised to 1e-3: the residual blocks would do nothing)
                p.mul_(300.0)
        if name.endswith("wide"):
            rows = made.final_layer.weight.view(D, K, 3, H)
            rows[:, :, 0] *= 35.0
            rows[:, :, 2] *= 45.0
            made.final_layer.bias.view(D, K, 3)[:, :, 2] -= 5.0
    return made.eval()


def inputs(name, rows=None):
    D, _, C, _, _, _, _, n = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 77)
    n = n if rows is None else rows
    x = 1.5 * torch.randn(n, D, generator=g)
    return x, None if C is None else torch.randn(n, C, generator=g)


@functools.lru_cache(maxsize=None)
def reference(name, rows=None):
    """(module, x, context, yardstick fp32 [B], truth fp64 [B]) -- shared: leave unchanged"""
    made = build(name)
    x, ctx = inputs(name, rows)
    with torch.no_grad():
        ref32 = made.log_prob(x, context=ctx).numpy()
        truth = copy.deepcopy(made).double().log_prob(x.double(), context=None if ctx is None else ctx.double()).numpy()
    return made, x, ctx, ref32, truth
