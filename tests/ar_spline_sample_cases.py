"""Sampling from conditional autoregressive spline layers (K28, csrc/made_inverse.hip `made_inverse_kernel<KT, 16, true>`):
the case table, builders, a restatement of the layer's inverse in stock torch ops, and a free-running fp32 CPU stand-in that
walks the packed schedule the way the kernel walks it.

`layer_inverse` is AutoregressiveTransform.inverse (autoregressive.py:43-52) written out for
MaskedPiecewiseRationalQuadraticAutoregressiveTransform (autoregressive.py:404-495): D passes of the whole MADE
(`maf_cases.made_forward`) on the outputs so far, each followed by the spline inverse over all features (the oracle's
torch restatement, oracle.eager.rqs_unconstrained).  `restated_inverse` runs a flow's layers backwards with it.
tests/test_ar_spline_sample_host.py holds it to the fixture of the real reference (tests/golden/flows_ar_rq_ctx.npz,
tests/golden/make_golden_ar_rq_ctx.py) and runs every case of the GPU file with the stand-in in the kernel's place: no case
may ask what correct fp32 arithmetic cannot give.

The stand-in (`stand_in_layer`): `maf_inverse_cases.walk_schedule`'s logic over a batch in fp32 (numpy) -- per block the
units in table order: dot product, bias, context term, residual add, ReLU --, on a step's last block feature t's output
rows, then the C oracle's float32 inverse spline (oracle.capi.rqs_elementwise), its own x_t fed back; the tail features
from the final hidden vector; the log-derivatives summed in float64 and rounded once, as the kernel sums them."""
import copy
import os

import numpy as np
import torch
from torch.nn import functional as F

import maf_cases
from maf_inverse_cases import assert_parity, error_figures  # noqa: F401  (the GPU and host files take them from here)

TAIL_BOUND = 3.0
SCALES = dict(scale_final=3.0, scale_linear1=100.0)   # off the near-identity initialisation: bins are not flat
ROWS = 1024                                           # rows of a GPU case (the host file runs the stand-in on the same rows)
FIXTURE_ROWS = 64
MANY_ROWS = 16 * 1024 + 5                             # more sixteen-sample groups than are resident at once, a ragged last one

# name -> arguments of `build`.  The first three are the flows of tests/golden/flows_ar_rq_ctx.npz.
FIXTURE = {
    "d8_h32_c5_k10": dict(features=8, hidden_features=32, context_features=5, num_bins=10, num_layers=3, num_blocks=2,
                          use_residual_blocks=True, permutation="reverse", seed=510),
    "d21_h64_c16_k8": dict(features=21, hidden_features=64, context_features=16, num_bins=8, num_layers=2, num_blocks=2,
                           use_residual_blocks=True, permutation="random", seed=511),
    # no context, 5 bins; one step block does not fit the LDS twice beside the state: continuation blocks
    "d6_h128_k5": dict(features=6, hidden_features=128, context_features=None, num_bins=5, num_layers=3, num_blocks=2,
                       use_residual_blocks=True, permutation="reverse", seed=512),
}


def _one(features, hidden, bins, seed, ce=None, **kw):
    return dict(features=features, hidden_features=hidden, context_features=ce, num_bins=bins, num_layers=1,
                permutation=None, seed=seed, **kw)


CASES = dict(FIXTURE)
CASES.update({
    # one conditional case per bin count in {2, 3, 5, 16}: the ends of the dispatch's range and two odd counts between
    "k2_ctx": _one(7, 32, 2, 620, ce=3),
    "k3_ctx": _one(7, 32, 3, 521, ce=3),
    "k5_ctx": _one(9, 48, 5, 522, ce=4),
    "k16_ctx": _one(7, 32, 16, 523, ce=3),
    # shape edges
    "d2": _one(2, 16, 8, 530, ce=2),
    "d3_h4": _one(3, 4, 6, 531, ce=2),
    "h50": _one(9, 50, 8, 532, ce=3),                                        # padded columns (50 -> 64)
    "d65_h128": _one(65, 128, 4, 533, ce=6),                                 # the feature vector crosses a chunk row
    "ff_random_masks": _one(9, 48, 7, 534, ce=5, use_residual_blocks=False, random_mask=True),
    "d64_h48_tail": _one(64, 48, 8, 535, ce=4),                              # H < D - 1: T = 48 steps, K13's tail
    "one_block": _one(8, 32, 9, 536, ce=3, num_blocks=1),
    "three_blocks": _one(8, 32, 12, 537, ce=3, num_blocks=3),
    "d6_h128_c8": _one(6, 128, 8, 538, ce=8),                                # continuation blocks with a context
    "d10_h32": _one(10, 32, 6, 639, ce=3),                                   # non-contiguous input, NaN, round trip
    "d17_h64_batches": _one(17, 64, 11, 540, ce=4),                          # the batch edges' 16 389 rows (17 features: beyond the size rule)
})

# |error| against float64 on the rows the GPU file uses, as tests/test_ar_spline_sample_host.py::
# test_the_stand_in_passes_every_gpu_case printed them when the seeds were chosen (k2_ctx and d10_h32 took a second seed: with
# the first the stand-in's logabsdet was at 2.8 x and 2.6 x the yardstick's 99.9 % quantile):
# name -> for x and for logabsdet ((mean, q99.9, max) as (stand-in, fp32 restatement), elements above 4 x the yardstick's maximum)
STAND_IN_FIGURES = {
    "d8_h32_c5_k10": (((1.1e-06, 1e-06), (5.2e-05, 0.00011), (0.00085, 0.00037), 0), ((4.3e-05, 5.1e-05), (0.0042, 0.0042), (0.0076, 0.011), 0)),
    "d21_h64_c16_k8": (((4.4e-07, 5.6e-07), (1.4e-05, 2.3e-05), (6.7e-05, 0.00013), 0), ((2.2e-05, 2.7e-05), (0.00025, 0.0004), (0.00043, 0.0012), 0)),
    "d6_h128_k5": (((7.2e-07, 9e-07), (4.4e-05, 5.5e-05), (9.9e-05, 0.0002), 0), ((9.5e-06, 1.2e-05), (0.00052, 0.0006), (0.00063, 0.00088), 0)),
    "k2_ctx": (((1.9e-07, 1.9e-07), (3.6e-06, 3.5e-06), (8.4e-06, 1e-05), 0), ((1.1e-06, 1.1e-06), (3.8e-05, 3.3e-05), (0.00026, 0.00026), 0)),
    "k3_ctx": (((2.6e-07, 2.8e-07), (4e-06, 4.7e-06), (1.3e-05, 1.3e-05), 0), ((3e-06, 3.5e-06), (0.00036, 0.0007), (0.00072, 0.00078), 0)),
    "k5_ctx": (((2.4e-07, 2.9e-07), (5.2e-06, 6.4e-06), (1.1e-05, 1.8e-05), 0), ((3.4e-06, 3.9e-06), (7.9e-05, 0.0001), (8.8e-05, 0.00017), 0)),
    "k16_ctx": (((2.6e-07, 3.3e-07), (8.8e-06, 9.4e-06), (2.5e-05, 0.0001), 0), ((1.3e-05, 1.5e-05), (0.00034, 0.00061), (0.0012, 0.0018), 0)),
    "d2": (((2.3e-07, 2.3e-07), (8.3e-06, 1.2e-05), (1.4e-05, 1.6e-05), 0), ((2.3e-06, 2.2e-06), (5.4e-05, 0.00011), (0.0002, 0.00013), 0)),
    "d3_h4": (((2.4e-07, 2.7e-07), (6.9e-06, 9.7e-06), (9.6e-06, 1.5e-05), 0), ((7.2e-06, 8e-06), (0.00016, 0.00012), (0.00042, 0.00043), 0)),
    "h50": (((2.5e-07, 3e-07), (5.9e-06, 8.7e-06), (4.2e-05, 3.9e-05), 0), ((6.7e-06, 7.6e-06), (0.00019, 0.00013), (0.00022, 0.00023), 0)),
    "d65_h128": (((3e-07, 3.3e-07), (6.9e-06, 8e-06), (0.00012, 0.00012), 0), ((1.3e-05, 1.6e-05), (0.0002, 0.0004), (0.00034, 0.00046), 0)),
    "ff_random_masks": (((1.7e-07, 2.2e-07), (1e-06, 1.4e-06), (1.2e-06, 2e-06), 0), ((1.1e-06, 1.3e-06), (5.9e-06, 6.3e-06), (7.2e-06, 6.6e-06), 0)),
    "d64_h48_tail": (((2.7e-07, 3.5e-07), (8e-06, 1.1e-05), (0.00016, 8.4e-05), 0), ((2.4e-05, 3e-05), (0.00044, 0.00059), (0.00084, 0.00065), 0)),
    "one_block": (((2.2e-07, 3.2e-07), (5.7e-06, 7.2e-06), (2.7e-05, 2.4e-05), 0), ((6.2e-06, 8e-06), (0.00013, 0.00021), (0.00028, 0.00028), 0)),
    "three_blocks": (((2.6e-07, 3.3e-07), (6.8e-06, 1.1e-05), (3.4e-05, 7e-05), 0), ((8.5e-06, 1.1e-05), (0.00012, 0.00047), (0.00018, 0.0005), 0)),
    "d6_h128_c8": (((2.8e-07, 3.3e-07), (8e-06, 6.5e-06), (3.2e-05, 3.2e-05), 0), ((6.7e-06, 6.7e-06), (0.00018, 0.00018), (0.00042, 0.00021), 0)),
    "d10_h32": (((2.5e-07, 2.9e-07), (7.4e-06, 6.8e-06), (1.5e-05, 2.7e-05), 0), ((4.7e-06, 5.1e-06), (0.00014, 0.00013), (0.00016, 0.00026), 0)),
    "d17_h64_batches": (((2.6e-07, 3.4e-07), (7.1e-06, 9.6e-06), (0.00025, 0.00038), 0), ((1.3e-05, 1.5e-05), (0.00048, 0.00047), (0.0015, 0.0025), 0)),
}


def build(name, golden=None, cases=None):
    """The case's flow on the CPU in eval mode, rebuilt from its seed: per layer the permutation, then the layer (the
    order of tests/golden/make_golden_ar_rq_ctx.py); with `golden` its state_dict is held to the fixture's checksums."""
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.transforms import (CompositeTransform, MaskedPiecewiseRationalQuadraticAutoregressiveTransform,
                                       RandomPermutation, ReversePermutation)
    cfg = dict((cases or CASES)[name])
    torch.manual_seed(cfg.pop("seed"))
    permutation, num_layers, features = cfg.pop("permutation"), cfg.pop("num_layers"), cfg["features"]
    layers = []
    for _ in range(num_layers):
        if permutation is not None:
            layers.append({"reverse": ReversePermutation, "random": RandomPermutation}[permutation](features))
        layers.append(MaskedPiecewiseRationalQuadraticAutoregressiveTransform(tails="linear", tail_bound=TAIL_BOUND, **cfg))
    flow = Flow(CompositeTransform(layers), StandardNormal([features])).eval()
    sharpen(flow)
    if golden is not None:
        names, sums = maf_cases.checksums(flow.state_dict())
        assert [str(n) for n in golden[name + "/param_names"]] == names, "state_dict keys differ from the reference's"
        want = golden[name + "/param_checksums"]
        assert np.all(np.abs(sums - want) <= 1e-9 * (1 + np.abs(want))), name
    return flow


def sharpen(module):
    with torch.no_grad():
        for pname, p in module.named_parameters():
            if "final_layer" in pname:
                p.mul_(SCALES["scale_final"])
            elif "linear_layers.1" in pname:
                p.mul_(SCALES["scale_linear1"])
    return module


def load(golden_dir):
    return np.load(os.path.join(golden_dir, "flows_ar_rq_ctx.npz"))


def rows_of(name):
    return MANY_ROWS if name == "d17_h64_batches" else ROWS


def inputs(name, rows=None, cases=None):
    """(z, context or None): 1.5 * randn rows -- about one element in twenty in the linear tails --, randn context rows."""
    cfg = (cases or CASES)[name]
    rows = rows_of(name) if rows is None else rows
    g = torch.Generator().manual_seed(7000 + cfg["seed"])
    z = 1.5 * torch.randn(rows, cfg["features"], generator=g)
    ce = cfg.get("context_features")
    return z, (None if ce is None else torch.randn(rows, ce, generator=g))


# ---- the restatement -------------------------------------------------------------------------------------------------------

def layer_inverse(layer, z, context=None, per_element=False):
    from oracle import eager
    net, K = layer.autoregressive_net, layer.num_bins
    x, lad = torch.zeros_like(z), None
    for _ in range(z.shape[1]):
        params = maf_cases.made_forward(net, x, context).view(z.shape[0], z.shape[1], 3 * K - 1)
        x, lad = eager.rqs_unconstrained(z, params[..., :K], params[..., K:2 * K], params[..., 2 * K:], inverse=True,
                                         tail_bound=layer.tail_bound)
    return x, (lad if per_element else torch.sum(lad, dim=[1]))


def layer_forward(layer, x, context=None):
    from oracle import eager
    net, K = layer.autoregressive_net, layer.num_bins
    params = maf_cases.made_forward(net, x, context).view(x.shape[0], x.shape[1], 3 * K - 1)
    z, lad = eager.rqs_unconstrained(x, params[..., :K], params[..., K:2 * K], params[..., 2 * K:], inverse=False,
                                     tail_bound=layer.tail_bound)
    return z, torch.sum(lad, dim=[1])


def restated_inverse(flow, z, context=None):
    """(x, logabsdet) of flow._transform.inverse in the dtype of `z`; `flow` is used for its tensors only."""
    h, total = z, z.new_zeros(z.shape[0])
    for t in reversed(list(flow._transform._transforms)):
        if type(t).__name__.endswith("Permutation"):
            h = torch.index_select(h, 1, torch.argsort(t._permutation))
        else:
            h, lad = layer_inverse(t, h, context)
            total = total + lad
    return h, total


def inverse_pair(flow_cpu, z, context=None, fp64_device=None, fp32_device=None):
    """{x32, lad32, x64, lad64} as numpy arrays: the restatement in fp32 (the yardstick) and in fp64 (the truth), on the CPU
    or by the same stock ops on the devices given.  `z` is an fp32 tensor: both invert the same numbers."""
    out = {}
    with torch.no_grad():
        for tag, dtype, dev in (("32", torch.float32, fp32_device), ("64", torch.float64, fp64_device)):
            f = copy.deepcopy(flow_cpu).to(dtype)
            zz, cc = z.to(dtype), None if context is None else context.to(dtype)
            if dev is not None:
                f, zz, cc = f.to(dev), zz.to(dev), None if cc is None else cc.to(dev)
            x, lad = restated_inverse(f, zz, cc)
            out["x" + tag], out["lad" + tag] = x.cpu().numpy(), lad.cpu().numpy()
    return out


def one_layer_flow(layer):
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.transforms import CompositeTransform
    features = layer.autoregressive_net.initial_layer.weight.shape[1]
    return Flow(CompositeTransform([copy.deepcopy(layer)]), StandardNormal([features]))


# ---- the plan of a layer, as the class makes it ------------------------------------------------------------------------------

def sequential_steps(net):
    return int(max(int(d.max()) for d in [net.initial_layer.degrees] + [b.degrees for b in net.blocks]))


def plan(layer, block_cap=None):
    """(schedule, packed context or None, T, cap): `MaskedPiecewiseRationalQuadraticAutoregressiveTransform.
    _sequential_ctx_plan`'s arithmetic on a CPU layer; `block_cap` replaces the LDS's own."""
    from nflows_amd import ops
    net = layer.autoregressive_net
    D = net.initial_layer.weight.shape[1]
    T = min(D, sequential_steps(net))
    H = net.initial_layer.weight.shape[0]
    cap = ops.made_block_cap(T, H, len(ops._made_linears(net)), len(ops.made_context_layers(net)))
    if block_cap is not None:
        cap = block_cap
    schedule = ops.pack_made_schedule(net, T, 3 * layer.num_bins - 1, block_cap=cap, context=True) if cap > 0 else None
    return schedule, ops.pack_made_context(net), T, cap


# ---- the free-running fp32 stand-in --------------------------------------------------------------------------------------------

def _inverse_spline32(z, params, K):
    from oracle import capi
    spec = capi.make_spec(K, tails="linear", tail_bound=TAIL_BOUND)
    p = np.ascontiguousarray(params, dtype=np.float32)
    y, lad, _ = capi.rqs_elementwise(np.ascontiguousarray(z, dtype=np.float32), p[..., :K], p[..., K:2 * K], p[..., 2 * K:],
                                     spec, inverse=True)
    return y, lad


def stand_in_layer(layer, z, context=None, block_cap=None):
    """(x, logabsdet, continuation blocks) of one layer from its packed schedule, everything in fp32 but the row sum."""
    from nflows_amd import ops
    schedule, packed_context, T, _ = plan(layer, block_cap)
    assert schedule is not None
    net, K = layer.autoregressive_net, layer.num_bins
    P = 3 * K - 1
    z = np.ascontiguousarray(z.numpy(), dtype=np.float32)
    B, D = z.shape
    terms = None
    if packed_context is not None:
        with torch.no_grad():
            terms = ops.made_context_terms(context.float(), packed_context).numpy()
    blocks_f, block_at, layout = schedule
    blocks_f, block_at = blocks_f.numpy(), block_at.numpy()
    n, _, final_src, stream_vec, num_vectors, Hp, Xp, _ = layout[:8]
    xs = np.zeros((B, Xp), dtype=np.float32)
    vecs = np.zeros((num_vectors, B, Hp), dtype=np.float32)
    x = np.zeros((B, D), dtype=np.float32)
    lad = np.zeros(B, dtype=np.float64)
    t, continuation = 0, 0
    for b in range(block_at.size - 2):
        blk = blocks_f[int(block_at[b]) * 256:int(block_at[b + 1]) * 256]
        units, rows, out_rows, out_bias, continued = (int(v) for v in blk[:5].view(np.int32))
        for u in range(units):
            e = blk[16 + 8 * u:24 + 8 * u]
            j, kp, src, dst, add_stream, set_stream, ctx_v = (int(v) for v in e[1:].view(np.int32))
            w = blk[rows:rows + kp]
            rows += kp
            v = (xs[:, :kp] if src < 0 else vecs[src][:, :kp]) @ w + e[0]
            if ctx_v:
                v = v + terms[:, ctx_v - 1, j]
            if add_stream:
                v = vecs[stream_vec][:, j] + v
            if set_stream:
                vecs[stream_vec][:, j] = v
            if dst >= 0:
                vecs[dst][:, j] = np.where(v < 0, np.float32(0), v)
        assert rows == out_rows
        if continued:
            continuation += 1
            continue
        if out_bias == 0:
            break
        params = vecs[final_src] @ blk[out_rows:out_bias].reshape(P, Hp).T + blk[out_bias:out_bias + P]
        y, l = _inverse_spline32(z[:, t], params, K)
        xs[:, t] = x[:, t] = y
        lad += l.astype(np.float64)
        t += 1
    assert t == T
    if T < D:   # the features beyond the largest hidden degree, from the final hidden vector
        with torch.no_grad():
            final = net.final_layer
            w = (final.weight * final.mask).float().numpy().reshape(D, P, -1)[T:]
            bias = final.bias.float().numpy().reshape(D, P)[T:]
        H = w.shape[2]
        params = np.einsum("bh,dph->bdp", vecs[final_src][:, :H], w).astype(np.float32) + bias
        y, l = _inverse_spline32(z[:, T:], params, K)
        x[:, T:] = y
        lad += l.astype(np.float64).sum(axis=1)
    return x, lad.astype(np.float32), continuation


def stand_in(flow, z, context=None):
    h, total = z, np.zeros(z.shape[0], dtype=np.float32)
    for t in reversed(list(flow._transform._transforms)):
        if type(t).__name__.endswith("Permutation"):
            h = torch.index_select(h, 1, torch.argsort(t._permutation))
        else:
            x, lad, _ = stand_in_layer(t, h, context)
            h, total = torch.from_numpy(x), total + lad
    return h.numpy(), total
