"""K37 on the device (csrc/affine_resnet_wide_kernel.hpp, ops.affine_coupling_wide): affine and additive coupling layers whose
conditioner is 129 .. 256 units wide, in one launch.  Truth: oracle/eager.py's stock-torch expressions on a float64 copy of
the modules on the CPU (the general scale activation, which it does not cover, restated below); yardstick: the same in
float32.  The project's parity rule (tests/test_gpu_wide_layer.py) with no element exempt: mean and 99.9 % quantile of the
error against the truth at most 2 x the yardstick's, the maximum at most 4 x."""
import copy

import numpy as np
import pytest
import torch

from maf_inverse_cases import error_figures
from nflows_amd import ops
from nflows_amd.flows.base import Flow
from nflows_amd.distributions import StandardNormal
from nflows_amd.nn.nets import MLP, ResidualNet
from nflows_amd.transforms import AdditiveCouplingTransform, AffineCouplingTransform, CompositeTransform
from oracle import eager

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUS = "cus"   # rows = 64 x (CU count + 1): the persistent loop's second pass
GENERAL = AffineCouplingTransform.GENERAL_SCALE_ACTIVATION

# name: (identity features, transformed features, conditioner (width, blocks) or MLP hidden sizes, rows, layers, kind)
CASES = {
    "hp160_idle_waves_three_of_a_tile": (3, 3, (129, 1), 64, 1, "affine"),
    "rows_padded_to_128": (8, 8, (192, 2), 100, 1, "affine"),
    "four_final_tiles_lds_limit": (64, 64, (256, 2), 128, 1, "affine"),
    "uneven_split_second_pass": (1, 5, (160, 1), CUS, 1, "affine"),
    "additive": (8, 8, (256, 2), 128, 1, "additive"),
    "additive_two_tiles": (30, 34, (192, 1), 64, 1, "additive"),
    "general_scale_activation": (8, 8, (256, 2), 128, 1, "general"),
    "mlp_sizes_padded_to_one_hp": (5, 5, [192, 256], 64, 1, "affine"),
    "two_layers_alternating_masks": (8, 8, (256, 2), 128, 2, "affine"),
}
BOTH = ("rows_padded_to_128", "four_final_tiles_lds_limit", "additive")
DIRECTIONS = [(n, inv) for n in CASES for inv in ((False, True) if n in BOTH else (False,))]
_built = {}


@pytest.fixture(autouse=True)
def the_kernel_itself_whatever_the_size_rule(monkeypatch):
    monkeypatch.setattr(AffineCouplingTransform, "fuse_wide_min_rows", 0)


def conditioner(shape, **kw):
    if isinstance(shape, list):
        return lambda i, o: MLP([i], [o], shape)
    return lambda i, o: ResidualNet(i, o, hidden_features=shape[0], num_blocks=shape[1], **kw)


def truth_transform(flow, x, inverse):
    """eager.flow_transform, with coupling.py:225 / :234-252 restated for the general scale activation"""
    layer = flow._transform._transforms[0]
    if layer.scale_activation is not GENERAL:
        return eager.flow_transform(flow, x, inverse=inverse)
    params = layer.transform_net(x[:, layer.identity_features], None)
    dt = layer.num_transform_features
    shift, scale = params[:, :dt], (torch.nn.functional.softplus(params[:, dt:]) + 1e-3).clamp(0, 3)
    out, xt, lad = x.clone(), x[:, layer.transform_features], torch.log(scale).sum(dim=1)
    out[:, layer.transform_features] = (xt - shift) / scale if inverse else xt * scale + shift
    return out, -lad if inverse else lad


def build(name):
    """(flow on the device, inputs, {inverse: (yardstick outputs, logabsdet, truth outputs, logabsdet)}), once per case"""
    if name not in _built:
        di, dt, shape, rows, layers, kind = CASES[name]
        rows = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) if rows == CUS else rows
        torch.manual_seed(37)
        mask = torch.ones(di + dt)
        mask[torch.arange(0, di + dt, 2)[:di]] = -1   # (di <= dt in every case: the identity features on even columns)
        cls, kw = (AdditiveCouplingTransform, {}) if kind == "additive" else (
            AffineCouplingTransform, dict(scale_activation=GENERAL) if kind == "general" else {})
        flow = Flow(CompositeTransform([cls((-1) ** k * mask, conditioner(shape), **kw) for k in range(layers)]),
                    StandardNormal([di + dt])).eval()
        with torch.no_grad():
            for pname, p in flow.named_parameters():   # (the default init leaves the blocks and the scales near identity)
                if "final_layer" in pname or "_output_layer" in pname:
                    p.mul_(4.0)
                elif "linear_layers.1" in pname:
                    p.mul_(30.0)
        x = 1.5 * torch.randn(rows, di + dt, generator=torch.Generator().manual_seed(38))
        ref = {}
        with torch.no_grad():
            f64 = copy.deepcopy(flow).double()
            for inverse in (False, True):
                y32, l32 = truth_transform(flow, x, inverse)
                y64, l64 = truth_transform(f64, x.double(), inverse)
                ref[inverse] = tuple(t.numpy() for t in (y32, l32, y64, l64))
            if kind != "general":
                ref["log_prob"] = (eager.flow_log_prob(flow, x).numpy(), eager.flow_log_prob(f64, x.double()).numpy())
        _built[name] = (copy.deepcopy(flow).to(DEV), x.to(DEV), ref)
    return _built[name]


def assert_parity(got, ref32, truth, what):
    got = got.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(ref32).all() and np.isfinite(truth).all(), what
    f = error_figures(got, ref32, truth)
    print(what, f)
    assert f["mean"][0] <= 2.0 * f["mean"][1] and f["q999"][0] <= 2.0 * f["q999"][1] and f["above_4x_max"] == 0, (what, f)


@pytest.mark.parametrize("name,inverse", DIRECTIONS)
def test_parity_with_the_truth(name, inverse):
    flow, x, ref = build(name)
    with torch.no_grad():
        y, lad = flow._transform.inverse(x) if inverse else flow._transform(x)
    assert ops.last_layer_kernel().startswith("k37::"), ops.last_layer_kernel()   # (fails without K37)
    ops.check_status()
    y32, l32, y64, l64 = ref[inverse]
    assert_parity(y, y32, y64, name + " outputs")
    if CASES[name][5] == "additive":
        assert torch.equal(lad, torch.zeros_like(lad))   # exactly zero
    else:
        assert_parity(lad, l32, l64, name + " logabsdet")


def test_log_prob_of_two_layers():
    flow, x, ref = build("two_layers_alternating_masks")
    with torch.no_grad():
        lp = flow.log_prob(x)
    assert ops.last_layer_kernel().startswith("k37::")
    assert_parity(lp, *ref["log_prob"], "two layers log_prob")


def test_second_pass_rows_equal_the_rows_alone_bit_for_bit():
    flow, x, _ = build("uneven_split_second_pass")
    with torch.no_grad():
        y, lad = flow._transform(x)
        y_tail, lad_tail = flow._transform(x[-64:].clone())
    assert ops.last_layer_kernel().startswith("k37::")
    assert torch.equal(y[-64:], y_tail) and torch.equal(lad[-64:], lad_tail)


def test_a_wide_layer_is_one_launch():
    """The conditioner module is never called (no stock GEMM, no K2 behind it), no per-layer launcher reports to the launch
    hook, and the layer kernel that ran is K37."""
    flow, x, _ = build("rows_padded_to_128")
    layer, seen = flow._transform._transforms[0], []

    class Hook:
        begin = staticmethod(lambda name: name)
        end = staticmethod(lambda token, nbytes: seen.append(token))
    handle = layer.transform_net.register_forward_pre_hook(lambda *a: seen.append("conditioner"))
    ops.set_launch_hook(Hook)
    try:
        with torch.no_grad():
            layer(x)
            layer.inverse(x)
    finally:
        ops.set_launch_hook(None)
        handle.remove()
    assert seen == [] and ops.last_layer_kernel().startswith("k37::"), (seen, ops.last_layer_kernel())


@pytest.mark.parametrize("how", ["width_128", "width_257", "context", "elu", "grad", "batch_norm", "custom_scale",
                                 "unconditional_transform", "image", "switch_off"])
def test_other_layers_keep_their_path(how, monkeypatch):
    from nflows_amd.transforms import ReversePermutation
    torch.manual_seed(3)
    kw = dict(context_features=3) if how == "context" else dict(activation=torch.nn.functional.elu) if how == "elu" else \
        dict(use_batch_norm=True) if how == "batch_norm" else {}
    net = conditioner(({"width_128": 128, "width_257": 257}.get(how, 256), 1), **kw)
    if how == "image":
        layer = AffineCouplingTransform(torch.tensor([1, -1, 1, -1]), _Conv)
        x = torch.randn(8, 4, 2, 2, device=DEV)
    else:
        layer = AffineCouplingTransform(
            torch.tensor([1, -1] * 4), net,
            unconditional_transform=(lambda features: ReversePermutation(features)) if how == "unconditional_transform" else None,
            **(dict(scale_activation=lambda u: torch.exp(u)) if how == "custom_scale" else {}))
        x = torch.randn(128, 8, device=DEV)
    layer = layer.to(DEV).eval()
    ctx = torch.randn(128, 3, device=DEV) if how == "context" else None
    served, _, _ = build("hp160_idle_waves_three_of_a_tile")
    with torch.no_grad():
        served._transform(torch.zeros(64, 6, device=DEV))   # leaves a k37:: label behind
        assert ops.last_layer_kernel().startswith("k37::")
        # (the old path's last kernel, K2, leaves no label: a run of two 128-wide layers, K11's, puts another one in K37's place)
        CompositeTransform([AffineCouplingTransform(torch.tensor([s, -s] * 4), conditioner((128, 1))) for s in (1, -1)]).to(
            DEV).eval()(torch.zeros(128, 8, device=DEV))
    assert ops.last_layer_kernel().startswith("affine_mlp_kernel"), ops.last_layer_kernel()
    if how == "switch_off":
        monkeypatch.setattr(AffineCouplingTransform, "fuse_wide_conditioner", False)
    with torch.set_grad_enabled(how == "grad"):
        y, lad = layer(x, ctx)
    assert torch.isfinite(y).all() and torch.isfinite(lad).all()
    assert not ops.last_layer_kernel().startswith("k37::"), ops.last_layer_kernel()


class _Conv(torch.nn.Module):
    """a 256-channel conditioner for 4-D inputs: (identity channels, context) -> parameter channels"""

    def __init__(self, i, o):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Conv2d(i, 256, 1), torch.nn.ReLU(), torch.nn.Conv2d(256, o, 1))

    def forward(self, inputs, context=None):
        return self.net(inputs)
