"""K32 on the device (csrc/rqs_resnet_wide_kernel.hpp, ops.rqs_coupling_resnet_wide): spline coupling layers whose ResidualNet
conditioner is 129 .. 256 units wide, in one launch.  Truth: oracle/eager.py's stock-torch expressions on a float64 copy of
the modules on the CPU; yardstick: the same in float32.  The project's parity rule (tests/test_gpu_steep.py) with no element
exempt: mean and 99.9 % quantile of the error against the truth at most 2 x the yardstick's, the maximum at most 4 x.
Per element on logits known bit for bit, every instance, knots / +-B / +-1e30 / outside-box inputs: tests/test_gpu_wide_exact.py."""
import copy

import numpy as np
import pytest
import torch

from maf_inverse_cases import error_figures
from nflows_amd import configs, ops
from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQCoupling
from oracle import eager

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUS = "cus"   # rows = 64 x (CU count + 1): the persistent loop's second pass

# name: (features, hidden, blocks, bins, rows, layers, factor on the final Linear's parameters)
CASES = {
    "pad_hp160_idle_waves": (6, 129, 1, 2, 64, 1, 4.0),
    "rows_padded_to_128": (16, 192, 2, 8, 100, 1, 4.0),
    "headline_full_width": (64, 256, 2, 8, 128, 1, 4.0),
    "three_final_tiles": (64, 256, 3, 16, 128, 1, 8.0),
    "geometry_and_lds_limit": (128, 256, 1, 10, 64, 1, 4.0),
    "second_pass": (6, 160, 1, 4, CUS, 1, 4.0),
    "two_layers_folded_tables": (16, 256, 2, 8, 128, 2, 4.0),
}
DIRECTIONS = [(n, inv) for n in CASES for inv in ((False, True) if n in ("rows_padded_to_128", "headline_full_width",
                                                                          "three_final_tiles") else (False,))]
_built = {}


@pytest.fixture(autouse=True)
def the_kernel_itself_whatever_the_size_rule(monkeypatch):
    monkeypatch.setattr(RQCoupling, "fuse_wide_min_rows", 0)


def build(name):
    """(flow on the device, inputs, {inverse: (yardstick outputs, logabsdet, truth outputs, logabsdet)}), once per case"""
    if name not in _built:
        features, hidden, blocks, bins, rows, layers, final = CASES[name]
        rows = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) if rows == CUS else rows
        flow = configs.rq_nsf_flow(num_layers=layers, features=features, num_bins=bins, hidden_features=hidden,
                                   num_blocks=blocks, tail_bound=3.0, seed=11).eval()
        with torch.no_grad():
            for pname, p in flow.named_parameters():   # (the default init leaves the blocks and the splines near identity)
                if "final_layer" in pname:
                    p.mul_(final)
                elif "linear_layers.1" in pname:
                    p.mul_(30.0)
        x = 1.5 * torch.randn(rows, features, generator=torch.Generator().manual_seed(12))
        ref = {}
        with torch.no_grad():
            f64 = copy.deepcopy(flow).double()
            for inverse in (False, True):
                y32, l32 = eager.flow_transform(flow, x, inverse=inverse)
                y64, l64 = eager.flow_transform(f64, x.double(), inverse=inverse)
                ref[inverse] = tuple(t.numpy() for t in (y32, l32, y64, l64))
            ref["log_prob"] = (eager.flow_log_prob(flow, x).numpy(), eager.flow_log_prob(f64, x.double()).numpy())
        _built[name] = (copy.deepcopy(flow).to(DEV), x.to(DEV), ref)
    return _built[name]


def assert_parity(got, ref32, truth, what):
    got = got.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(ref32).all(), what
    f = error_figures(got, ref32, truth)
    print(what, f)
    assert f["mean"][0] <= 2.0 * f["mean"][1] and f["q999"][0] <= 2.0 * f["q999"][1] and f["above_4x_max"] == 0, (what, f)


@pytest.mark.parametrize("name,inverse", DIRECTIONS)
def test_parity_with_the_truth(name, inverse):
    flow, x, ref = build(name)
    with torch.no_grad():
        y, lad = flow._transform.inverse(x) if inverse else flow._transform(x)
    assert ops.last_layer_kernel().startswith("k32::"), ops.last_layer_kernel()   # (fails without K32)
    ops.check_status()
    y32, l32, y64, l64 = ref[inverse]
    assert_parity(y, y32, y64, name + " outputs")
    assert_parity(lad, l32, l64, name + " logabsdet")


def test_second_pass_rows_equal_the_rows_alone_bit_for_bit():
    flow, x, _ = build("second_pass")
    with torch.no_grad():
        y, lad = flow._transform(x)
        y_tail, lad_tail = flow._transform(x[-64:].clone())
    assert torch.equal(y[-64:], y_tail) and torch.equal(lad[-64:], lad_tail)


def test_log_prob_of_two_layers():
    flow, x, ref = build("two_layers_folded_tables")
    with torch.no_grad():
        lp = flow.log_prob(x)
    assert ops.last_layer_kernel().startswith("k32::")
    assert_parity(lp, *ref["log_prob"], "two layers log_prob")


def test_size_rule_keeps_unmeasured_sizes_on_the_old_path(monkeypatch):
    monkeypatch.undo()   # the class's own rule
    flow, x, _ = build("two_layers_folded_tables")
    with torch.no_grad():
        flow._transform(x.repeat(8, 1))
        assert ops.last_layer_kernel().startswith("k32::")          # 1 024 rows
        flow._transform(x)
        assert not ops.last_layer_kernel().startswith("k32::")      # 128 rows


@pytest.mark.parametrize("how", ["width_128", "width_257", "context", "tails_none", "bins_17", "elu", "grad", "switch_off"])
def test_other_layers_keep_their_path(how, monkeypatch):
    from nflows_amd.nn.nets.resnet import ResidualNet
    from nflows_amd.utils.torchutils import create_alternating_binary_mask
    torch.manual_seed(3)
    hidden = {"width_128": 128, "width_257": 257}.get(how, 256)
    layer = RQCoupling(create_alternating_binary_mask(8), lambda i, o: ResidualNet(
        i, o, hidden_features=hidden, num_blocks=1, context_features=3 if how == "context" else None,
        activation=torch.nn.functional.elu if how == "elu" else torch.nn.functional.relu),
        num_bins=17 if how == "bins_17" else 8, tails=None if how == "tails_none" else "linear",
        tail_bound=1.0 if how == "tails_none" else 3.0).to(DEV).eval()
    x = torch.rand(128, 8, device=DEV) if how == "tails_none" else torch.randn(128, 8, device=DEV)
    ctx = torch.randn(128, 3, device=DEV) if how == "context" else None
    served, _, _ = build("pad_hp160_idle_waves")
    with torch.no_grad():
        served._transform(torch.zeros(64, 6, device=DEV))   # leaves a k32:: label behind
        assert ops.last_layer_kernel().startswith("k32::")
        RQCoupling(create_alternating_binary_mask(8), lambda i, o: ResidualNet(i, o, hidden_features=64, num_blocks=1),
                   num_bins=8, tails="linear", tail_bound=3.0).to(DEV).eval()(x)
    assert not ops.last_layer_kernel().startswith("k32::")                              # ... and K8 replaces it
    if how == "switch_off":
        monkeypatch.setattr(RQCoupling, "fuse_wide_conditioner", False)
    with torch.set_grad_enabled(how == "grad"):
        y, lad = layer(x, ctx)
    assert torch.isfinite(y).all() and not ops.last_layer_kernel().startswith("k32::"), ops.last_layer_kernel()
