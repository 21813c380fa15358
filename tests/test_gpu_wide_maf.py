"""K36 on the device (csrc/affine_made_wide_kernel.hpp, ops.affine_flow_made_wide): the density pass of masked
autoregressive affine layers whose MADE is 129 .. 256 units wide, with and without a context, one launch per layer.  Truth:
the forward pass restated in stock torch ops (tests/maf_cases.py) in float64 on the device; yardstick: the same in float32 on
the CPU.  The project's parity rule (`assert_parity`): mean and 99.9 % quantile of the error against the truth at most 2 x
the yardstick's, at most three elements above 4 x its maximum."""
import pytest
import torch

import maf_cases
from maf_inverse_cases import assert_parity
from nflows_amd import configs, ops
from nflows_amd.transforms import MaskedAffineAutoregressiveTransform as MAF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 36
CUS = "cus"   # rows = 64 x (CU count + 1): the persistent loop's second pass

# name: (features, hidden, blocks, form of the blocks, context features, rows, layers)
CASES = {
    "hp160_idle_waves_odd_d_one_tile": (3, 129, 1, "residual", None, 64, 1),
    "rows_padded": (7, 192, 2, "residual", None, 100, 1),
    "second_tile_one_feature_second_pass_random_masks": (17, 160, 2, "feed_forward_random_mask", None, CUS, 1),
    "four_final_tiles_four_initial_ksteps": (64, 256, 2, "residual", None, 128, 1),
    "one_padded_context_kstep": (8, 256, 2, "residual", 3, 128, 1),
    "lds_maximum": (64, 256, 1, "residual", 64, 64, 1),
    "feed_forward_initial_context_only": (12, 192, 2, "feed_forward", 5, 128, 1),
    "two_layers_reverse_permutation": (16, 256, 2, "residual", 16, 128, 2),
}
_built = {}


@pytest.fixture(autouse=True)
def the_kernel_itself_whatever_the_size_rule(monkeypatch):
    monkeypatch.setattr(MAF, "fuse_wide_min_rows", 0)


def build(name):
    """(flow on the device, inputs and context on the device, `restated_pair`'s yardstick and truth), once per case"""
    if name not in _built:
        features, hidden, blocks, form, ce, rows, layers = CASES[name]
        rows = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) if rows == CUS else rows
        flow = configs.masked_affine_flow(features, hidden, layers, num_blocks=blocks, use_residual_blocks=form == "residual",
                                          random_mask=form.endswith("random_mask"),
                                          permutation="reverse" if layers > 1 else None, context_features=ce, seed=SEED,
                                          **maf_cases.SHARPEN).eval()
        g = torch.Generator().manual_seed(SEED + 1)
        x = 1.2 * torch.randn(rows, features, generator=g)
        ctx = None if ce is None else torch.randn(rows, ce, generator=g)
        ref = maf_cases.restated_pair(flow, x, ctx, fp64_device=DEV)
        _built[name] = (flow.to(DEV), x.to(DEV), None if ctx is None else ctx.to(DEV), ref)
    return _built[name]


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_truth(name):
    flow, x, ctx, ref = build(name)
    with torch.no_grad():
        z, lad = flow._transform(x, ctx)
        assert ops.last_layer_kernel().startswith("k36::"), ops.last_layer_kernel()   # (fails without K36)
        lp = flow.log_prob(x, ctx)
    assert ops.last_layer_kernel().startswith("k36::"), ops.last_layer_kernel()
    ops.check_status()
    assert_parity(z.cpu().numpy(), ref["z32"], ref["z64"], name + " z")
    assert_parity(lad.cpu().numpy(), ref["lad32"], ref["lad64"], name + " logabsdet")
    assert_parity(lp.cpu().numpy(), ref["lp32"], ref["lp64"], name + " log_prob")


def test_autoregressive_property_bit_for_bit():
    flow, x, _, _ = build("rows_padded")
    other = x.clone()
    other[:, -1] = torch.randn(x.shape[0], device=DEV)
    with torch.no_grad():
        z, _ = flow._transform(x)
        z_other, _ = flow._transform(other)
    assert ops.last_layer_kernel().startswith("k36::")
    # (masked-out weights are exact zeros in all three pieces: the features in front do not see the last one at all)
    assert torch.equal(z[:, :-1], z_other[:, :-1]) and not torch.equal(z[:, -1], z_other[:, -1])


def test_second_pass_rows_equal_the_rows_alone_bit_for_bit():
    flow, x, _, _ = build("second_tile_one_feature_second_pass_random_masks")
    with torch.no_grad():
        z, lad = flow._transform(x)
        z_tail, lad_tail = flow._transform(x[-64:].clone())
    assert ops.last_layer_kernel().startswith("k36::")
    assert torch.equal(z[-64:], z_tail) and torch.equal(lad[-64:], lad_tail)


@pytest.mark.parametrize("how", ["width_128", "width_257", "features_65", "context_65", "elu", "grad", "switch_off"])
def test_other_layers_keep_their_path(how, monkeypatch):
    torch.manual_seed(3)
    features = 65 if how == "features_65" else 8
    ce = 65 if how == "context_65" else None
    layer = MAF(features, {"width_128": 128, "width_257": 257}.get(how, 256), context_features=ce,
                activation=torch.nn.functional.elu if how == "elu" else torch.nn.functional.relu).to(DEV).eval()
    x = torch.randn(128, features, device=DEV)
    ctx = torch.randn(128, ce, device=DEV) if ce else None
    # (the old path's last kernel, K2b, leaves no label: a 128-wide layer's K22 launch puts another one in K36's place)
    with torch.no_grad():
        MAF(3, 128).to(DEV).eval()(torch.zeros(128, 3, device=DEV))
    assert ops.last_layer_kernel().startswith("affine_mlp_kernel"), ops.last_layer_kernel()
    if how == "switch_off":
        monkeypatch.setattr(MAF, "fuse_wide_conditioner", False)
    with torch.set_grad_enabled(how == "grad"):
        y, lad = layer(x, ctx)
    assert torch.isfinite(y).all() and torch.isfinite(lad).all()
    assert not ops.last_layer_kernel().startswith("k36::"), ops.last_layer_kernel()
