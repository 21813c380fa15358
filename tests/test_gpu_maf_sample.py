"""Sampling from masked autoregressive affine layers in one persistent kernel per layer (K23, csrc/made_inverse.hip).

`MaskedAffineAutoregressiveTransform.inverse` was a host loop over the features: the MADE's hidden GEMMs, an addmm, K2b and
a rank-1 update per feature.  K23 is K12's step loop with the affine element: every feature a step, the context terms as
per-sample constants in LDS, wide steps cut into continuation blocks.  Here, under the project's parity rule (against the
float64 restatement on the device: mean and 99.9 % quantile of the error at most 2 x the fp32 restatement's, at most three
elements above 4 x its maximum, everything finite -- tests/maf_inverse_cases.py):
  * the six fixture flows (tests/maf_cases.py), whole and layer by layer, one launch per layer and none of K2b;
  * `Flow.sample`, with and without a context, and the factory's flow;
  * batch and shape edges, a NaN row, the round trip, stale packed weights, the layers that fall back.
Inputs are the density pass of small x (the sharpened fixture flows push normal noise to 1e52), or normal noise through
the milder `SAMPLING` weights."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import maf_cases
import maf_inverse_cases as inv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional
LABEL = "made_inverse_kernel<element=affine"


def MAF():
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform
    return MaskedAffineAutoregressiveTransform


@contextlib.contextmanager
def switch(value):
    saved = MAF().fuse_sequential_inverse
    MAF().fuse_sequential_inverse = value
    try:
        yield
    finally:
        MAF().fuse_sequential_inverse = saved


def count(fn):
    """(launches of K23's wrapper, calls of ops.affine_autoregressive, result of `fn` under no-grad), as test_gpu_maf.count_k22
    counts."""
    from nflows_amd import ops
    kernel, k2b, n = ops.made_affine_inverse, ops.affine_autoregressive, [0, 0]

    def counted_kernel(*args, **kw):
        n[0] += 1
        return kernel(*args, **kw)

    def counted_k2b(*args, **kw):
        n[1] += 1
        return k2b(*args, **kw)
    ops.made_affine_inverse, ops.affine_autoregressive = counted_kernel, counted_k2b
    try:
        with torch.no_grad():
            result = fn()
    finally:
        ops.made_affine_inverse, ops.affine_autoregressive = kernel, k2b
    return n[0], n[1], result


def another_label():
    """`ops.last_layer_kernel()` keeps the last layer kernel's name and the host loop launches none: a K22 density pass of a
    small layer puts another name there, so that a test can tell whether the call that follows launched K23."""
    from nflows_amd import ops
    torch.manual_seed(1)
    with torch.no_grad():
        MAF()(features=4, hidden_features=16).to(DEV).eval()(torch.randn(128, 4, device=DEV))
    assert ops.last_layer_kernel().startswith("affine_mlp_kernel"), ops.last_layer_kernel()


def one_layer_flow(layer):
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.transforms import CompositeTransform
    return Flow(CompositeTransform([copy.deepcopy(layer)]), StandardNormal([layer.features]))


def check_against_restatement(flow_cpu, z, context, got_x, got_lad, what):
    o = inv.inverse_pair(flow_cpu, z, context, fp64_device=DEV)
    inv.assert_parity(got_x.cpu().numpy(), o["x32"], o["x64"], what + " x")
    inv.assert_parity(got_lad.cpu().numpy(), o["lad32"], o["lad64"], what + " logabsdet")
    return o


@pytest.mark.parametrize("case", list(maf_cases.CASES))
def test_fixture_flow_inverse_is_one_launch_per_layer(golden_dir, case):
    import nflows_amd
    from nflows_amd import ops
    cfg = maf_cases.CASES[case]
    flow_cpu = maf_cases.build(case, maf_cases.load(golden_dir))
    z, context = inv.fixture_z(flow_cpu, case, rows=1024, seed=77)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    zd, cd = z.to(DEV), None if context is None else context.to(DEV)
    launches, k2b, (x, lad) = count(lambda: flow._transform.inverse(zd, context=cd))
    label = ops.last_layer_kernel()
    assert launches == cfg["num_layers"] and k2b == 0, (launches, k2b)
    assert label.startswith(LABEL) and ("context=1" in label) == ("context_features" in cfg), label
    assert ("group=1" in label) == (cfg["hidden_features"] >= 5 * (cfg["features"] - 1)), label
    if case == "d6_l5":
        assert "continuation_blocks=0" not in label, label   # a step of 60 KB does not fit twice beside 44 KB of state
    nflows_amd.check_status()
    o = check_against_restatement(flow_cpu, z, context, x, lad, case)
    assert np.abs(o["x64"]).max() <= 5.1
    # the last layer alone
    layer = flow._transform._transforms[-1]
    launches, k2b, (x1, lad1) = count(lambda: layer.inverse(zd, context=cd))
    assert launches == 1 and k2b == 0 and ops.last_layer_kernel() == label
    check_against_restatement(one_layer_flow(flow_cpu._transform._transforms[-1]), z, context, x1, lad1, case + " last layer")
    another_label()
    with switch(False):
        launches, k2b, (x0, lad0) = count(lambda: layer.inverse(zd, context=cd))
    assert launches == 0 and k2b >= 1 and not ops.last_layer_kernel().startswith(LABEL)


@pytest.mark.parametrize("case", list(maf_cases.CASES))
def test_sampling_agrees_with_the_host_loop(case):
    """Flow.sample with normal noise through the milder weights: the kernel's samples against the switch-off path's, both
    measured against the float64 restatement of the inverse on the same noise."""
    cfg = maf_cases.CASES[case]
    flow_cpu = inv.build_for_sampling(case)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    ce = cfg.get("context_features")
    context = None if ce is None else torch.randn(4, ce, generator=torch.Generator().manual_seed(5)).to(DEV)
    num = 64 if ce is None else 8

    def draw():
        torch.manual_seed(3)
        return flow.sample(num, context=context)
    launches, k2b, on = count(draw)
    assert launches == cfg["num_layers"] and k2b == 0
    with switch(False):
        launches, k2b, off = count(draw)
        assert launches == 0 and k2b > 0
        with torch.no_grad():
            torch.manual_seed(3)
            noise = flow._noise(num, context, False).reshape(-1, cfg["features"])
            rows_ctx = None if ce is None else torch.repeat_interleave(context, num, dim=0)
            assert torch.equal(flow._transform.inverse(noise, context=rows_ctx)[0], off.reshape(-1, cfg["features"]))
    with torch.no_grad():
        f64 = copy.deepcopy(flow_cpu).double().to(DEV)
        truth = inv.restated_inverse(f64, noise.double(), None if ce is None else rows_ctx.double())[0]
    assert float(truth.abs().max()) <= 1.2e3
    inv.assert_parity(on.reshape(-1, cfg["features"]).cpu().numpy(), off.reshape(-1, cfg["features"]).cpu().numpy(),
                      truth.cpu().numpy(), case + " sample")


def test_the_factory_flow_samples_through_the_kernel():
    from nflows_amd import ops
    from nflows_amd.flows import MaskedAutoregressiveFlow
    torch.manual_seed(6)
    flow = MaskedAutoregressiveFlow(features=8, hidden_features=32, num_layers=3, num_blocks_per_layer=2).to(DEV).eval()
    launches, k2b, samples = count(lambda: flow.sample(100))
    assert launches == 3 and k2b == 0 and ops.last_layer_kernel().startswith(LABEL)
    assert samples.shape == (100, 8) and torch.isfinite(samples).all()
    launches, k2b, (s, lp) = count(lambda: flow.sample_and_log_prob(50))
    assert launches == 3 and k2b == 0
    with torch.no_grad():
        assert float((flow.log_prob(s) - lp).abs().max()) < 1e-3


def _layer(features, hidden, seed, ce=None, **kw):
    """One layer off its near-identity initialisation (as configs.masked_affine_flow moves it, milder)."""
    torch.manual_seed(seed)
    layer = MAF()(features=features, hidden_features=hidden, context_features=ce, **kw).eval()
    with torch.no_grad():
        for name, p in layer.named_parameters():
            if "final_layer" in name:
                p.mul_(0.5)
            elif "linear_layers.1" in name:
                p.mul_(100.0)
    return layer


def _layer_check(layer_cpu, rows, what, seed=11, ce=None, make_input=None):
    """The layer's inverse on the density pass of small x against the restatement; returns (layer on the device, z, ctx)."""
    from nflows_amd import ops
    d = layer_cpu.features
    g = torch.Generator().manual_seed(seed)
    x = 1.2 * torch.randn(rows, d, generator=g)
    context = None if ce is None else torch.randn(rows, ce, generator=g)
    flow_cpu = one_layer_flow(layer_cpu)
    with torch.no_grad():
        z = maf_cases.restated(copy.deepcopy(flow_cpu).double(), x.double(),
                               None if ce is None else context.double())[0].float()
    layer = copy.deepcopy(layer_cpu).to(DEV)
    zd = z.to(DEV) if make_input is None else make_input(z.to(DEV))
    cd = None if ce is None else context.to(DEV)
    launches, k2b, (got_x, got_lad) = count(lambda: layer.inverse(zd, context=cd))
    assert launches == 1 and k2b == 0 and ops.last_layer_kernel().startswith(LABEL), (what, ops.last_layer_kernel())
    assert got_x.shape == (rows, d) and got_lad.shape == (rows,)
    check_against_restatement(flow_cpu, z, context, got_x, got_lad, what)
    return layer, zd, cd


@pytest.fixture(scope="module")
def many_groups():
    """16 * 1024 + 5 rows -- more sixteen-sample groups than are resident at once, a ragged last one -- under the rule;
    (layer, z, x, logabsdet), computed once."""
    layer, z, _ = _layer_check(_layer(8, 32, seed=20), 16 * 1024 + 5, "rows=16389")
    with torch.no_grad():
        x, lad = layer.inverse(z)
    return layer, z, x, lad


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 16 * 1024 + 5])
def test_batch_edges(many_groups, rows):
    """Sixteen samples per workgroup: a lone row, one short of a group, a full group, one more.  Samples do not meet, so a
    short batch gives the long batch's rows bit for bit -- at both ends of it, where the ragged group is."""
    layer, z, x, lad = many_groups
    for part in (slice(0, rows), slice(z.shape[0] - rows, z.shape[0])):
        launches, k2b, (px, plad) = count(lambda: layer.inverse(z[part]))
        assert launches == 1 and k2b == 0 and px.shape == (rows, 8)
        assert torch.equal(px, x[part]) and torch.equal(plad, lad[part])


@pytest.mark.parametrize("features, hidden, kw", [
    (2, 16, {}), (3, 16, {}), (17, 32, {}), (63, 64, {}), (64, 64, {}),
    (8, 20, {}),                                             # padded columns
    (8, 256, {}),                                            # dot_rows_64
    (9, 48, dict(use_residual_blocks=False, random_mask=True)),
    (12, 32, dict(num_blocks=0)),
    (5, 24, dict(use_residual_blocks=False, num_blocks=3, ce=7)),
    (7, 32, dict(ce=3)),
])
def test_shape_edges(features, hidden, kw):
    kw = dict(kw)
    ce = kw.pop("ce", None)
    _layer_check(_layer(features, hidden, seed=features + hidden, ce=ce, **kw), 1024, "D=%d H=%d %s" % (features, hidden, kw),
                 ce=ce)


def test_a_non_contiguous_input():
    def strided(z):
        wide = torch.zeros(z.shape[0], 2 * z.shape[1], device=z.device)
        wide[:, ::2] = z
        view = wide[:, ::2]
        assert not view.is_contiguous()
        return view
    _layer_check(_layer(10, 32, seed=30), 1024, "non-contiguous", make_input=strided)


def test_a_nan_stays_in_its_row_and_behind_its_column():
    layer, z, _ = _layer_check(_layer(12, 32, seed=40), 1024, "nan: the clean call")
    r, j = 37, 5
    with torch.no_grad():
        clean_x, clean_lad = layer.inverse(z)
        dirty = z.clone()
        dirty[r, j] = float("nan")
        x, lad = layer.inverse(dirty)
    others = [i for i in range(z.shape[0]) if i != r]
    assert torch.equal(x[others], clean_x[others]) and torch.equal(lad[others], clean_lad[others])
    assert torch.equal(x[r, :j], clean_x[r, :j]) and bool(torch.isnan(x[r, j]))


def test_round_trip():
    """forward(inverse(z)) against z: the kernel's inverse under the rule, the host loop's as the yardstick."""
    layer, z, _ = _layer_check(_layer(16, 64, seed=50), 1024, "round trip: inverse")
    with torch.no_grad():
        back_on = layer(layer.inverse(z)[0])[0]
        with switch(False):
            back_off = layer(layer.inverse(z)[0])[0]
    inv.assert_parity(back_on.cpu().numpy(), back_off.cpu().numpy(), z.double().cpu().numpy(), "round trip")


def test_packed_schedule_follows_the_parameters_and_the_masks():
    kw = dict(use_residual_blocks=False, random_mask=True)
    layer = _layer(12, 48, seed=60, **kw).to(DEV)
    z = torch.randn(64, 12, device=DEV, generator=torch.Generator(DEV).manual_seed(1))

    def now():
        n, _, out = count(lambda: layer.inverse(z))
        assert n == 1
        return out

    def fresh():
        n, _, out = count(lambda: copy.deepcopy(layer).inverse(z))
        assert n == 1
        return out

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    first = now()
    assert same(first, fresh())
    with torch.no_grad():
        for p in layer.autoregressive_net.final_layer.parameters():
            p.mul_(2)
    doubled = now()
    assert same(doubled, fresh()) and not same(doubled, first)
    with torch.no_grad():
        for p in layer.autoregressive_net.final_layer.parameters():
            p.data.mul_(0.5)
    halved = now()
    assert same(halved, fresh()) and same(halved, first)
    other = _layer(12, 48, seed=61, **kw)
    masks = [k for k in other.state_dict() if k.endswith(".mask")]
    assert any(not torch.equal(other.state_dict()[k], layer.state_dict()[k].cpu()) for k in masks)
    layer.load_state_dict(other.state_dict())
    loaded = now()
    assert same(loaded, count(lambda: other.to(DEV).inverse(z))[2]) and not same(loaded, halved)


@pytest.mark.parametrize("features, hidden, kw", [
    (6, 128, {}),                                            # 26 units per Linear and step, continuation blocks
    (8, 256, {}),                                            # dot_rows_64
    (7, 20, dict(use_residual_blocks=False, random_mask=True, ce=3)),
    (63, 64, dict(ce=4)),                                    # one or two units per Linear and step
])
def test_groups_of_units_give_the_same_bits(monkeypatch, features, hidden, kw):
    """NFA_K23_GROUP: up to eight units of a Linear per pass of the dot products, or one by one -- every dot product keeps
    its summation order."""
    from nflows_amd import ops
    kw = dict(kw)
    ce = kw.pop("ce", None)
    layer = _layer(features, hidden, seed=70 + features, ce=ce, **kw).to(DEV)
    g = torch.Generator(DEV).manual_seed(2)
    z = torch.randn(300, features, device=DEV, generator=g)
    context = None if ce is None else torch.randn(300, ce, device=DEV, generator=g)
    results = {}
    for value in ("1", "0"):
        monkeypatch.setenv("NFA_K23_GROUP", value)
        launches, _, results[value] = count(lambda: layer.inverse(z, context=context))
        assert launches == 1 and ops.last_layer_kernel().endswith("group=%s>" % value), ops.last_layer_kernel()
    assert torch.isfinite(results["1"][0]).all()
    assert torch.equal(results["1"][0], results["0"][0]) and torch.equal(results["1"][1], results["0"][1])


def _fallback_cases():
    class Mine(MAF()):
        def _elementwise_inverse(self, inputs, params):
            return super()._elementwise_inverse(inputs, params)
    plain = dict(features=6, hidden_features=32)
    return {
        "grad enabled": (MAF(), plain, True, None),
        "a subclass's _elementwise_inverse": (Mine, plain, False, None),
        "tanh": (MAF(), dict(plain, activation=torch.tanh), False, None),
        "batch norm inside": (MAF(), dict(plain, use_batch_norm=True), False, None),
        "hidden 512": (MAF(), dict(features=6, hidden_features=512), False, None),
        "NFA_K23=0": (MAF(), plain, False, False),
        "few features, many rows": (MAF(), dict(features=4, hidden_features=16), False, None),
    }


@pytest.mark.parametrize("why", ["grad enabled", "a subclass's _elementwise_inverse", "tanh", "batch norm inside",
                                 "hidden 512", "NFA_K23=0", "few features, many rows"])
def test_layers_outside_the_family_take_the_host_loop(why):
    from nflows_amd import ops
    cls, kw, grad, flag = _fallback_cases()[why]
    torch.manual_seed(9)
    layer = cls(**kw).to(DEV).eval()
    z = torch.randn(65537 if why == "few features, many rows" else 48, kw["features"], device=DEV)

    def run():
        with torch.set_grad_enabled(grad):
            x, lad = layer.inverse(z)
        return x.detach(), lad.detach()
    another_label()
    with switch(MAF().fuse_sequential_inverse if flag is None else flag):
        launches, _, (x, lad) = count(run)
        label = ops.last_layer_kernel()
    # (hidden 512 reaches the planner, which finds no room for the state: no launch is attempted)
    assert launches == 0 and not (label or "").startswith(LABEL), (why, launches, label)
    with switch(False):
        _, _, (x0, lad0) = count(run)
    assert torch.isfinite(x).all() and torch.equal(x, x0) and torch.equal(lad, lad0)
