"""The masked autoregressive affine flows of tests/golden/flows_maf.npz (K22, csrc/affine_made.hip) and a restatement of
their density pass in stock torch ops.

The fixture holds six flows built with the REAL reference's classes (tests/golden/make_golden_maf.py), 256 rows each:
x, the context where there is one, and z / lad / log_prob in fp32 and fp64.  Weights are not stored: `build` rebuilds every
flow from its seed with configs.masked_affine_flow, and the stored per-tensor checksums (parameters, masks, degrees,
permutations) say whether that worked.

`restated` is the reference's forward pass written out op for op -- MADE.forward (made.py:274-283) with its masked Linears
(:71-72), residual (:187-202) and feed-forward blocks (:115-123), the affine map (autoregressive.py:96-128), the
composite's running total (transforms/base.py:45-52) and the standard-normal base (distributions/normal.py:27-33).
tests/test_maf_host.py holds it bit for bit to the fixture in fp32 and fp64 on the CPU; the GPU tests use it as the
yardstick for batches larger than the fixture (fp32 on the CPU, fp64 by stock ops on the device)."""
import os

import numpy as np
import torch
from torch.nn import functional as F

# name -> arguments of configs.masked_affine_flow; the smallest shapes at which the kernel can go wrong
CASES = {
    # two initial k-steps, one half-empty final tile
    "d8_h32_reverse": dict(features=8, hidden_features=32, num_layers=3, num_blocks=2, use_residual_blocks=True,
                           permutation="reverse", seed=410),
    # four initial k-steps, a partial third final tile
    "d36_random_perm": dict(features=36, hidden_features=128, num_layers=4, num_blocks=2, use_residual_blocks=True,
                            permutation="random", seed=411),
    # a pad column the density must skip; random masks need feed-forward blocks
    "d63_random_masks": dict(features=63, hidden_features=128, num_layers=3, num_blocks=1, use_residual_blocks=False,
                             random_mask=True, seed=412),
    # a pad of two, an odd number of layers
    "d6_l5": dict(features=6, hidden_features=128, num_layers=5, num_blocks=2, use_residual_blocks=True, seed=413),
    # context, residual blocks
    "d21_ctx5": dict(features=21, hidden_features=64, num_layers=3, num_blocks=2, use_residual_blocks=True,
                     context_features=5, seed=414),
    # context, feed-forward blocks
    "d16_ctx64_ff": dict(features=16, hidden_features=128, num_layers=2, num_blocks=2, use_residual_blocks=False,
                         context_features=64, seed=415),
}
SHARPEN = dict(scale_final=2.0, scale_linear1=100.0)
ROWS = 256


def fixture_inputs(name):
    """(x, context or None) of a case: 1.2 * randn rows, randn context rows, from the case's seed."""
    cfg = CASES[name]
    g = torch.Generator().manual_seed(9000 + cfg["seed"])
    x = 1.2 * torch.randn(ROWS, cfg["features"], generator=g)
    ce = cfg.get("context_features")
    return x, (None if ce is None else torch.randn(ROWS, ce, generator=g))


def checksums(state_dict):
    """Per tensor: sum, sum of magnitudes and a position-weighted sum (a permuted mask or permutation changes it)."""
    names, sums = [], []
    for k, v in state_dict.items():
        v = v.double().reshape(-1)
        weights = 1.0 + (torch.arange(v.numel(), dtype=torch.float64) % 97.0)
        names.append(k)
        sums.append([float(v.sum()), float(v.abs().sum()), float((v * weights).sum())])
    return names, np.array(sums, dtype=np.float64)


def load(golden_dir):
    return np.load(os.path.join(golden_dir, "flows_maf.npz"))


def build(name, golden=None):
    """The case's flow on the CPU in eval mode, rebuilt from its seed; with `golden` its state_dict is held to the
    fixture's names and checksums."""
    from nflows_amd import configs
    flow = configs.masked_affine_flow(**CASES[name], **SHARPEN).eval()
    if golden is not None:
        names, sums = checksums(flow.state_dict())
        assert [str(n) for n in golden[name + "/param_names"]] == names, "state_dict keys differ from the reference's"
        want = golden[name + "/param_checksums"]
        assert np.all(np.abs(sums - want) <= 1e-9 * (1 + np.abs(want))), name
    return flow


# ---- the restatement ---------------------------------------------------------------------------------------------------

def _masked(lin, h):
    return F.linear(h, lin.weight * lin.mask, lin.bias)


def made_forward(net, x, context=None):
    """MADE.forward of the reference (ReLU, no batch norm, no dropout)."""
    h = _masked(net.initial_layer, x)
    if context is not None:
        h = h + F.relu(F.linear(context, net.context_layer.weight, net.context_layer.bias))
    if not net.use_residual_blocks:
        h = F.relu(h)
    for block in net.blocks:
        if net.use_residual_blocks:
            t = _masked(block.linear_layers[0], F.relu(h))
            if context is not None:
                t = t + F.linear(context, block.context_layer.weight, block.context_layer.bias)
            h = h + _masked(block.linear_layers[1], F.relu(t))
        else:
            h = F.relu(_masked(block.linear, h))
    return _masked(net.final_layer, h)


def affine_layer_forward(layer, x, context=None):
    params = made_forward(layer.autoregressive_net, x, context).view(-1, layer.features, 2)
    scale = F.softplus(params[..., 0]) + 1e-3
    return scale * x + params[..., 1], torch.sum(torch.log(scale), dim=[1])


def restated(flow, x, context=None):
    """(z, lad, log_prob) of the flow's density pass in the dtype of `x`; `flow` is used for its tensors only."""
    h, total = x, x.new_zeros(x.shape[0])
    for t in flow._transform._transforms:
        if type(t).__name__.endswith("Permutation"):
            h, lad = torch.index_select(h, 1, t._permutation), h.new_zeros(h.shape[0])
        else:
            h, lad = affine_layer_forward(t, h, context)
        total += lad
    log_z = torch.tensor(0.5 * h.shape[1] * np.log(2 * np.pi), dtype=torch.float64)
    return h, total, (-0.5 * torch.sum(h ** 2, dim=[1]) - log_z) + total


def restated_pair(flow_cpu, x, context=None, fp64_device=None):
    """{z32, lad32, lp32, z64, lad64, lp64} as numpy arrays: fp32 on the CPU (the yardstick), fp64 on the CPU or, with
    `fp64_device`, by the same stock ops on that device (the truth)."""
    import copy
    out = {}
    with torch.no_grad():
        for k, v in zip(("z", "lad", "lp"), restated(flow_cpu.float(), x.float(), None if context is None else context.float())):
            out[k + "32"] = v.numpy()
        f64 = copy.deepcopy(flow_cpu).double()
        x64, c64 = x.double(), None if context is None else context.double()
        if fp64_device is not None:
            f64, x64, c64 = f64.to(fp64_device), x64.to(fp64_device), None if c64 is None else c64.to(fp64_device)
        for k, v in zip(("z", "lad", "lp"), restated(f64, x64, c64)):
            out[k + "64"] = v.cpu().numpy()
    return out
