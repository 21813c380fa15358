"""K34 on the device (csrc/made_rqs_wide_kernel.hpp, ops.rqs_flow_made_wide): the density pass of autoregressive
rational-quadratic spline layers whose MADE is 129 .. 256 units wide, one launch per layer.  Truth: the forward pass restated
in stock torch ops (tests/ar_spline_density_cases.py) in float64 on the device; yardstick: the same in float32 on the CPU.
The project's parity rule (`assert_parity`): mean and 99.9 % quantile of the error against the truth at most 2 x the
yardstick's, at most three elements above 4 x its maximum.

Measured on the MI355X: mean error 0.6 - 1.0 x the yardstick's; all six cases pass (DESIGN.md section 4 "K34" has the figures,
and those of the single-accumulator form that missed the rule on `two_layers_log_prob`)."""
import pytest
import torch

from ar_spline_density_cases import restated_pair
from maf_inverse_cases import assert_parity
from nflows_amd import ops
from nflows_amd.distributions import StandardNormal
from nflows_amd.flows import Flow
from nflows_amd.transforms import CompositeTransform, ReversePermutation
from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform as ARSpline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 34
CUS = "cus"   # rows = 64 x (CU count + 1): the persistent loop's second pass

# name: (features, hidden, blocks, form of the blocks, bins, rows, layers)
CASES = {
    "hp160_idle_waves_odd_d_one_tile": (3, 129, 1, "residual", 2, 64, 1),
    "rows_padded_two_tiles_odd_d": (7, 192, 2, "residual", 10, 100, 1),
    "full_width_8_bins": (64, 256, 2, "residual", 8, 128, 1),
    "feed_forward_three_tiles": (64, 256, 1, "feed_forward", 16, 64, 1),
    "second_pass_random_masks": (6, 160, 2, "feed_forward_random_mask", 6, CUS, 1),
    "two_layers_log_prob": (16, 256, 2, "residual", 10, 128, 2),
}
_built = {}


@pytest.fixture(autouse=True)
def the_kernel_itself_whatever_the_size_rule(monkeypatch):
    monkeypatch.setattr(ARSpline, "fuse_wide_min_rows", 0)


def make_layer(features, hidden, blocks=1, form="residual", bins=10, **kw):
    kw.setdefault("tails", "linear")
    return ARSpline(features, hidden, num_bins=bins, tail_bound=3.0 if kw["tails"] else 1.0, num_blocks=blocks,
                    use_residual_blocks=form == "residual", random_mask=form.endswith("random_mask"), **kw)


def build(name):
    """(flow on the device, inputs on the device, `restated_pair`'s yardstick and truth), once per case"""
    if name not in _built:
        features, hidden, blocks, form, bins, rows, layers = CASES[name]
        rows = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) if rows == CUS else rows
        torch.manual_seed(SEED)
        transforms = []
        for _ in range(layers):
            transforms += ([ReversePermutation(features)] if layers > 1 else []) + [make_layer(features, hidden, blocks,
                                                                                              form, bins)]
        flow = Flow(CompositeTransform(transforms), StandardNormal([features])).eval()
        with torch.no_grad():
            for pname, p in flow.named_parameters():   # (the default init leaves the blocks and the splines near identity)
                if "final_layer" in pname:
                    p.mul_(8.0 if bins == 16 else 4.0)
                elif "linear_layers.1" in pname or ".linear." in pname:   # each block's last Linear
                    p.mul_(30.0)
        x = 1.5 * torch.randn(rows, features, generator=torch.Generator().manual_seed(SEED + 1))
        ref = restated_pair(flow, x, None, fp64_device=DEV)
        _built[name] = (flow.to(DEV), x.to(DEV), ref)
    return _built[name]


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_truth(name, monkeypatch):
    if CASES[name][4] == 8:
        monkeypatch.setattr(ARSpline, "fuse_conditioner", 2)   # K29's mode rule for 8 bins
    flow, x, ref = build(name)
    with torch.no_grad():
        z, lad = flow._transform(x)
        assert ops.last_layer_kernel().startswith("k34::"), ops.last_layer_kernel()   # (fails without K34)
        lp = flow.log_prob(x)
    assert ops.last_layer_kernel().startswith("k34::"), ops.last_layer_kernel()
    ops.check_status()
    assert_parity(z.cpu().numpy(), ref["z32"], ref["z64"], name + " z")
    assert_parity(lad.cpu().numpy(), ref["lad32"], ref["lad64"], name + " logabsdet")
    assert_parity(lp.cpu().numpy(), ref["lp32"], ref["lp64"], name + " log_prob")


def test_autoregressive_property_bit_for_bit():
    flow, x, _ = build("rows_padded_two_tiles_odd_d")
    other = x.clone()
    other[:, -1] = torch.randn(x.shape[0], device=DEV)
    with torch.no_grad():
        z, _ = flow._transform(x)
        z_other, _ = flow._transform(other)
    assert ops.last_layer_kernel().startswith("k34::")
    # (masked-out weights are exact zeros in all three pieces: the features in front do not see the last one at all)
    assert torch.equal(z[:, :-1], z_other[:, :-1]) and not torch.equal(z[:, -1], z_other[:, -1])


def test_second_pass_rows_equal_the_rows_alone_bit_for_bit():
    flow, x, _ = build("second_pass_random_masks")
    with torch.no_grad():
        z, lad = flow._transform(x)
        z_tail, lad_tail = flow._transform(x[-64:].clone())
    assert ops.last_layer_kernel().startswith("k34::")
    assert torch.equal(z[-64:], z_tail) and torch.equal(lad[-64:], lad_tail)


@pytest.mark.parametrize("how", ["width_128", "width_257", "features_65", "context", "tails_none", "bins_17", "elu", "grad",
                                 "switch_off", "bins_8_mode_1"])
def test_other_layers_keep_their_path(how, monkeypatch):
    torch.manual_seed(3)
    features = 65 if how == "features_65" else 8
    layer = make_layer(features, {"width_128": 128, "width_257": 257}.get(how, 256),
                       bins={"bins_17": 17, "bins_8_mode_1": 8}.get(how, 10),
                       context_features=3 if how == "context" else None,
                       activation=torch.nn.functional.elu if how == "elu" else torch.nn.functional.relu,
                       tails=None if how == "tails_none" else "linear").to(DEV).eval()
    x = torch.rand(128, features, device=DEV) if how == "tails_none" else torch.randn(128, features, device=DEV)
    ctx = torch.randn(128, 3, device=DEV) if how == "context" else None
    served, _, _ = build("hp160_idle_waves_odd_d_one_tile")
    with torch.no_grad():
        served._transform(torch.zeros(64, 3, device=DEV))   # leaves a k34:: label behind
    assert ops.last_layer_kernel().startswith("k34::")
    if how == "switch_off":
        monkeypatch.setattr(ARSpline, "fuse_wide_conditioner", False)
    if how == "bins_8_mode_1":
        monkeypatch.setattr(ARSpline, "fuse_conditioner", 1)
    with torch.set_grad_enabled(how == "grad"):
        y, lad = layer(x, ctx)
    assert torch.isfinite(y).all() and torch.isfinite(lad).all()
    assert not ops.last_layer_kernel().startswith("k34::"), ops.last_layer_kernel()
