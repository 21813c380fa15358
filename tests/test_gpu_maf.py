"""The density pass of masked autoregressive affine layers in one launch (K22, csrc/affine_made.hip).

`MaskedAffineAutoregressiveTransform.forward` was a `weight * mask` product per masked layer, the MADE's GEMMs, K2b and a
permutation, layer by layer.  With the masks multiplied into the weights at pack time a MADE is K11's conditioner with
d_i = d_t = features, so K11's kernel body runs such layers in its autoregressive mode, context terms included.  Here:
  * every case of tests/golden/flows_maf.npz (tests/maf_cases.py: built by the real reference, 256 rows) is ONE run of
    K22 and meets the golden rule -- mean / q999 at 2 x the reference-fp32's own error against float64, max at 4 x --,
    agrees with the layer-by-layer path to 2e-4, and a ragged batch gives the full batch's rows;
  * more 128-row blocks than the device has CUs against the restatement (the persistent loop and the table double buffer
    wrap), same rule;
  * a single layer and the factory's flow with batch norm between the layers: every MAF layer a run of one;
  * the inverse, sampling and differentiated passes do not change by a bit with the switch;
  * the packed weights follow an optimizer step, a write through `.data` and a load_state_dict with other masks;
  * layers outside the kernel's family plan no run and give the switch-off path's results.
"""
import copy

import numpy as np
import pytest
import torch

import maf_cases
from helpers import assert_error_ratio
from test_gpu_flows import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional


def switch(value):
    """Context manager: MaskedAffineAutoregressiveTransform.fuse_conditioner = value."""
    import contextlib
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform as MAF

    @contextlib.contextmanager
    def scope():
        saved = MAF.fuse_conditioner
        MAF.fuse_conditioner = value
        try:
            yield
        finally:
            MAF.fuse_conditioner = saved
    return scope()


def kernel_label(cfg):
    return "affine_mlp_kernel<autoregressive=1, init_ks=%d, resnet=%d, context=%d>" % (
        4 if cfg["features"] > 32 else 2, int(cfg["use_residual_blocks"]), int("context_features" in cfg))


def count_k22(fn):
    """Number of K22 launches `fn` makes under no-grad, and what it returns."""
    from nflows_amd import ops
    whole, n = ops.affine_flow_made, [0]

    def counted(*args, **kw):
        n[0] += 1
        return whole(*args, **kw)
    ops.affine_flow_made = counted
    try:
        with torch.no_grad():
            result = fn()
    finally:
        ops.affine_flow_made = whole
    return n[0], result


@pytest.mark.parametrize("case", list(maf_cases.CASES))
def test_fixture_flow_is_one_run_of_k22(golden_dir, case):
    import nflows_amd
    from nflows_amd import ops
    g = maf_cases.load(golden_dir)
    cfg = maf_cases.CASES[case]
    flow = copy.deepcopy(maf_cases.build(case, g)).to(DEV)
    x = torch.from_numpy(g[case + "/x"]).to(DEV)
    ctx = torch.from_numpy(g[case + "/context"]).to(DEV) if "context_features" in cfg else None
    layers = list(flow._transform._transforms)
    with torch.no_grad():
        units, after = flow._transform._collect_run(layers, 0, x, ctx, inverse=False)
        assert len(units) == cfg["num_layers"] and after == len(layers), "the flow is not one run of K22"
        assert flow._transform._collect_run(layers[::-1], 0, x, ctx, inverse=True)[0] == []
        launches, lp = count_k22(lambda: flow.log_prob(x, context=ctx))
        assert launches == 1 and ops.last_layer_kernel() == kernel_label(cfg), ops.last_layer_kernel()
        launches, (z, lad) = count_k22(lambda: flow._transform(x, context=ctx))
        assert launches == 1 and ops.last_layer_kernel() == kernel_label(cfg), ops.last_layer_kernel()
        lp_ragged = flow.log_prob(x[:200], context=None if ctx is None else ctx[:200])
        z_ragged, lad_ragged = flow._transform(x[:200], context=None if ctx is None else ctx[:200])
        with switch(False):
            launches, (z2, lad2) = count_k22(lambda: flow._transform(x, context=ctx))
            assert launches == 0
            lp2 = flow.log_prob(x, context=ctx)
    nflows_amd.check_status()
    d = cfg["features"]
    figures = {k: float((a - b).abs().max()) for k, a, b in (("z", z, z2), ("lad", lad, lad2), ("log_prob", lp, lp2))}
    print(case, "against the layer-by-layer path:", figures)
    check(z, g[case + "/z"], g[case + "/z64"], case + " z", 3e-6)
    check(lad, g[case + "/lad"], g[case + "/lad64"], case + " lad", 3e-6 * d)
    check(lp, g[case + "/log_prob"], g[case + "/log_prob64"], case + " log_prob", 3e-6 * d)
    assert all(v < 2e-4 for v in figures.values()), figures
    assert torch.equal(lp_ragged, lp[:200]) and torch.equal(z_ragged, z[:200]) and torch.equal(lad_ragged, lad[:200])


def test_more_row_blocks_than_compute_units():
    """8 features, 5 layers, more 128-row blocks than CUs plus a ragged tail: every workgroup walks several row blocks, the
    table double buffer ends a row block on its second half and wraps.  Against the restatement under the golden rule."""
    import nflows_amd
    from nflows_amd import configs, ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 128 * (2 * cus + 3) + 37
    flow_cpu = configs.masked_affine_flow(features=8, hidden_features=128, num_layers=5, num_blocks=2, permutation="random",
                                          seed=21, **maf_cases.SHARPEN).eval()
    x = 1.2 * torch.randn(rows, 8, generator=torch.Generator().manual_seed(22))
    o = maf_cases.restated_pair(flow_cpu, x, fp64_device=DEV)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    with torch.no_grad():
        launches, (z, lad) = count_k22(lambda: flow._transform(x.to(DEV)))
        assert launches == 1 and "autoregressive=1" in ops.last_layer_kernel()
        lp = flow.log_prob(x.to(DEV))
    nflows_amd.check_status()
    for what, got, k, width in (("z", z, "z", 1), ("lad", lad, "lad", 8), ("log_prob", lp, "lp", 8)):
        scale = 1 + np.abs(o[k + "64"]).max()
        f = assert_error_ratio(got.cpu().numpy(), o[k + "32"], o[k + "64"], "many blocks " + what, factor=2.0, max_factor=4.0,
                               max_floor=3e-6 * scale * width)
        print("many blocks", what, f)


def test_single_layers_are_runs_of_one():
    """A layer called on its own, and the factory's flow with batch norm between the layers in eval mode: every MAF layer
    runs K22 as a run of one, every BatchNorm stays one K17 launch."""
    from nflows_amd import ops
    from nflows_amd.flows import MaskedAutoregressiveFlow
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform as MAF
    from test_gpu_normalization import launches
    torch.manual_seed(5)
    layer = MAF(features=10, hidden_features=48, num_blocks=2).to(DEV).eval()
    x = 1.2 * torch.randn(300, 10, device=DEV)
    n, (z, lad) = count_k22(lambda: layer(x))
    assert n == 1 and "autoregressive=1" in ops.last_layer_kernel()
    with switch(False):
        n, (z2, lad2) = count_k22(lambda: layer(x))
    assert n == 0 and float((z - z2).abs().max()) < 2e-4 and float((lad - lad2).abs().max()) < 2e-4

    torch.manual_seed(6)
    flow = MaskedAutoregressiveFlow(features=8, hidden_features=32, num_layers=6, num_blocks_per_layer=2,
                                    batch_norm_between_layers=True).to(DEV)
    with torch.no_grad():
        flow.train()
        flow.log_prob(1.2 * torch.randn(512, 8, device=DEV))   # (running statistics off their initial values)
    flow.eval()
    xs = 1.2 * torch.randn(512, 8, device=DEV)
    layers = list(flow._transform._transforms)
    with torch.no_grad():
        for i, t in enumerate(layers):
            if isinstance(t, MAF):   # [permutation, layer], then the BatchNorm ends the run
                units, after = flow._transform._collect_run(layers, i - 1, xs, None, inverse=False)
                assert len(units) == 1 and units[0][0] is t and units[0][1] is layers[i - 1] and after == i + 1
    n, (z, lad) = count_k22(lambda: flow._transform(xs))
    assert n == 6
    calls = launches(lambda: flow._transform(xs))
    assert calls.count("norm_map") == 6 and "norm_stats" not in calls, calls
    # every layer's plan is kept: a second call builds none (six runs of one in one composite)
    tables, built = ops.flow_layer_tables, [0]

    def counted(*args, **kw):
        built[0] += 1
        return tables(*args, **kw)
    ops.flow_layer_tables = counted
    try:
        count_k22(lambda: flow._transform(xs))
    finally:
        ops.flow_layer_tables = tables
    assert built[0] == 0
    with switch(False):
        n, (z2, lad2) = count_k22(lambda: flow._transform(xs))
        calls = launches(lambda: flow._transform(xs))
    assert n == 0 and calls.count("norm_map") == 6, calls
    # (a BatchNorm on running statistics of one batch stretches the columns: 2e-4 is the fixtures' bound at |z| <= 12, and
    #  both paths round in fp32 at the magnitude they meet, so the bound grows with it)
    grow = max(1.0, float(z2.abs().max()) / 12.0)
    assert float((z - z2).abs().max()) < 2e-4 * grow and float((lad - lad2).abs().max()) < 2e-4 * grow


def test_inverse_sampling_and_gradients_do_not_change_by_a_bit(golden_dir):
    case = "d8_h32_reverse"
    flow = copy.deepcopy(maf_cases.build(case)).to(DEV)
    x, _ = maf_cases.fixture_inputs(case)
    x = x.to(DEV)

    def passes():
        out = {}
        with torch.no_grad():
            torch.manual_seed(3)
            out["sample"] = flow.sample(64)
            out["inv_x"], out["inv_lad"] = flow._transform.inverse(x)
        flow.zero_grad()
        xin = x.clone().requires_grad_(True)
        lp = flow.log_prob(xin)
        lp.sum().backward()
        out["log_prob"], out["grad_x"] = lp.detach(), xin.grad
        for name, p in flow.named_parameters():
            out["grad " + name] = p.grad.clone()
        return out

    n, on = count_k22(lambda: torch.enable_grad()(passes)())
    assert n == 0, "K22 serves the no-grad density pass only"
    with switch(False):
        off = passes()
    assert on.keys() == off.keys()
    for k in on:
        assert torch.equal(on[k], off[k]), k


def test_packed_weights_follow_the_parameters_and_the_masks():
    """After an optimizer step, after a write through `.data`, and after a load_state_dict with other random masks the next
    log_prob is a freshly built copy's, bit for bit."""
    from nflows_amd import configs
    kw = dict(features=12, hidden_features=64, num_layers=2, num_blocks=2, use_residual_blocks=False, random_mask=True,
              **maf_cases.SHARPEN)
    flow = configs.masked_affine_flow(seed=31, **kw).to(DEV).eval()
    x = 1.2 * torch.randn(256, 12, device=DEV, generator=torch.Generator(DEV).manual_seed(1))

    def fresh():
        with torch.no_grad():
            return copy.deepcopy(flow).log_prob(x)

    with torch.no_grad():
        first = flow.log_prob(x)
    assert torch.equal(first, fresh())
    opt = torch.optim.SGD(flow.parameters(), lr=1e-2)
    (-flow.log_prob(x).mean()).backward()
    opt.step()
    with torch.no_grad():
        stepped = flow.log_prob(x)
    assert torch.equal(stepped, fresh()) and not torch.equal(stepped, first)
    with torch.no_grad():
        for p in flow._transform._transforms[0].autoregressive_net.final_layer.parameters():
            p.data.mul_(2)
        doubled = flow.log_prob(x)
    assert torch.equal(doubled, fresh()) and not torch.equal(doubled, stepped)
    other = configs.masked_affine_flow(seed=32, **kw)
    masks = [k for k in other.state_dict() if k.endswith(".mask")]
    assert any(not torch.equal(other.state_dict()[k], flow.state_dict()[k].cpu()) for k in masks)
    flow.load_state_dict(other.state_dict())
    n, loaded = count_k22(lambda: flow.log_prob(x))
    assert n == 1
    with torch.no_grad():
        assert torch.equal(loaded, other.to(DEV).eval().log_prob(x)) and not torch.equal(loaded, doubled)


@pytest.mark.parametrize("why, kw, ce", [
    ("elu", dict(activation=F.elu), None),
    ("batch norm within layers", dict(use_batch_norm=True), None),
    ("active dropout", dict(dropout_probability=0.5), None),
    ("hidden 256", dict(hidden_features=256), None),
    ("65 features", dict(features=65), None),
    ("65-feature context", dict(context_features=65), 65),
])
def test_layers_outside_the_family_take_the_layer_by_layer_path(why, kw, ce):
    from nflows_amd.transforms import CompositeTransform, MaskedAffineAutoregressiveTransform as MAF, ReversePermutation
    torch.manual_seed(9)
    args = dict(features=12, hidden_features=64, num_blocks=2)
    args.update(kw)
    d = args["features"]
    stack = CompositeTransform([t for _ in range(2) for t in (ReversePermutation(d), MAF(**args))]).to(DEV)
    stack.train() if why == "active dropout" else stack.eval()
    x = 1.2 * torch.randn(256, d, device=DEV)
    ctx = None if ce is None else torch.randn(256, ce, device=DEV)
    with torch.no_grad():
        assert stack._collect_run(list(stack._transforms), 0, x, ctx, inverse=False)[0] == []

    def run():
        torch.manual_seed(4)   # (the dropout masks)
        return stack(x, ctx)
    n, (z, lad) = count_k22(run)
    assert n == 0
    with switch(False):
        n, (z2, lad2) = count_k22(run)
    assert torch.isfinite(z).all() and torch.isfinite(lad).all()
    assert torch.equal(z, z2) and torch.equal(lad, lad2)
    if why == "active dropout":   # in eval mode the dropout is inactive and the layers form a run
        stack.eval()
        with torch.no_grad():
            assert len(stack._collect_run(list(stack._transforms), 0, x, ctx, inverse=False)[0]) == 2
