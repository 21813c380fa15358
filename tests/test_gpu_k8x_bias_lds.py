"""K8x's bias area: a layer's biases and the next layer's table reach LDS as LDS-DMA pieces requested a layer ahead
(rqs_resnet_f16x3_kernel.hpp: bias_area_piece), so the kernel carries state from layer to layer and from one row block of a
workgroup to the next -- the hidden biases of the NEXT layer (of layer 0 again behind the last one), the raw table, the
final layer's biases.  A bias read before it has landed, or a piece left from another layer, row block or launch, is an
O(bias) error: every case here is held against the layer-by-layer path (`RQ.fuse_conditioner = False`: no whole-layer
kernel at all) under the 2 x rule of tests/test_gpu_headline_parity.compare, the truth being the float64 port on the device.
  * carried state across row blocks: 131 072 rows whose second half repeats the first -- on a grid of 512 workgroups row
    block q + 512 is the second pass of the workgroup that ran block q: the halves must agree bit for bit;
  * the geometries that lay the area out differently: no blocks (the final layer follows the initial GEMM at once), one,
    two; d_i > 32 (the four-k-step initial layer); 10 bins (the general final layer: 32 bias rows per feature);
  * launch order: a stale area from another launch must not be read;
  * the fall-back: 20 bins with two blocks at D = 64, where the area would take the launch from two workgroups per CU to one,
    runs the entry that reads the hidden biases from global memory -- the kernel's name says which entry ran
    (`bias=lds` / `bias=global`), and every other case here asserts `bias=lds`.
"""
import copy

import pytest
import torch

from helpers import LAD_TOL, OUT_TOL
from test_gpu_headline_parity import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def f16x3(monkeypatch):
    import nflows_amd
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ
    monkeypatch.setattr(RQ, "conditioner_engine", "f16x3")
    monkeypatch.setattr(RQ, "fuse_conditioner", True)
    try:   # (the device status word is sticky)
        nflows_amd.check_status()
    except (AssertionError, IndexError, ValueError, RuntimeError):
        pass
    return RQ


def _flow(num_layers, features=64, num_bins=8, num_blocks=2, seed=0):
    """configs.rq_nsf_flow as it is initialised, like the whole-flow cases of tests/test_gpu_k8x.py: every Linear's bias is
    drawn from U(+-1 / sqrt(fan_in)), so a bias of another layer is an error of 0.1 in a pre-activation, and the splines are
    well conditioned in both directions -- compare()'s plain rule bounds the MAXIMUM by 2 x the reference's own, which a
    steep spline's heavy-tailed inverse error does not meet in any fp32 evaluation (see compare's `max_count`)."""
    from nflows_amd import configs
    return configs.rq_nsf_flow(num_layers=num_layers, features=features, num_bins=num_bins, hidden_features=128,
                               num_blocks=num_blocks, seed=seed).eval()


def _ran_k8x(bias="lds"):
    from nflows_amd import ops
    label = ops.last_layer_kernel()
    assert "k8x::" in label and "bias=%s>" % bias in label, label


def _truth(flow_cpu, x, inverse):
    from oracle import eager
    f64 = copy.deepcopy(flow_cpu).double().to(DEV)
    with torch.no_grad():
        y, lad = eager.flow_transform(f64, x.double().to(DEV), inverse=inverse)
        lp = None if inverse else eager.standard_normal_log_prob(y) + lad
    return y.cpu().numpy(), lad.cpu().numpy(), None if lp is None else lp.cpu().numpy()


def _run(RQ, flow, xd, inverse, fused, bias="lds"):
    """(y, logabsdet, log_prob) of the fused or the layer-by-layer path"""
    import nflows_amd
    RQ.fuse_conditioner = fused
    with torch.no_grad():
        if inverse:
            y, lad = flow._transform.inverse(xd)
            lp = None
        else:
            y, lad = flow._transform(xd)
            if fused:
                _ran_k8x(bias)
            lp = flow.log_prob(xd)
        if fused:
            _ran_k8x(bias)
    nflows_amd.check_status()
    return y, lad, lp


def _against_layer_by_layer(config, RQ, flow_cpu, x, inverse, rows=None, bias="lds"):
    """the whole-layer kernel on x against the layer-by-layer path on x[:rows]; returns the kernel's results and its name"""
    from nflows_amd import ops
    flow = copy.deepcopy(flow_cpu).to(DEV).eval()
    xd = x.to(DEV)
    y, lad, lp = _run(RQ, flow, xd, inverse, True, bias)
    assert ops.last_redo_blocks() == 0
    label = ops.last_layer_kernel()
    rows = x.shape[0] if rows is None else rows
    y1, lad1, lp1 = _run(RQ, flow, xd[:rows], inverse, False)
    RQ.fuse_conditioner = True
    t_y, t_lad, t_lp = _truth(flow_cpu, x[:rows], inverse)
    compare(config, "x" if inverse else "z", y[:rows].cpu().numpy(), y1.cpu().numpy(), t_y, OUT_TOL)
    compare(config, "logabsdet", lad[:rows].cpu().numpy(), lad1.cpu().numpy(), t_lad, LAD_TOL)
    if not inverse:
        compare(config, "log_prob", lp[:rows].cpu().numpy(), lp1.cpu().numpy(), t_lp, LAD_TOL)
    return y, lad, lp, label


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_state_carried_across_the_row_blocks_of_a_workgroup(f16x3, inverse):
    B, half = 131072, 65536
    blocks = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    if blocks > half // 128:
        pytest.skip("%d workgroups: row block q + 512 is not the second pass of the workgroup that ran block q" % blocks)
    flow_cpu = _flow(3)
    x = torch.randn(half, 64, generator=torch.Generator().manual_seed(31 + inverse))
    x = torch.cat([x, x])
    y, lad, lp, _ = _against_layer_by_layer("k8x_bias_lds_rowblocks_" + ("inverse" if inverse else "forward"), f16x3, flow_cpu, x,
                                         inverse, rows=half)
    assert torch.equal(y[:half], y[half:]) and torch.equal(lad[:half], lad[half:])
    if not inverse:
        assert torch.equal(lp[:half], lp[half:])


@pytest.mark.parametrize("case,kw", [("no_blocks", dict(num_blocks=0)), ("one_block", dict(num_blocks=1)),
                                     ("two_blocks", dict(num_blocks=2)), ("d100_init_ks4", dict(features=100)),
                                     ("ten_bins", dict(num_bins=10)), ("twenty_bins_global_bias", dict(num_bins=20))])
def test_geometries_of_the_bias_area(f16x3, case, kw):
    """256 rows: two workgroups, one row block each, two layers"""
    bias = "global" if case == "twenty_bins_global_bias" else "lds"
    flow_cpu = _flow(2, seed=7, **kw)
    features = kw.get("features", 64)
    x = torch.randn(256, features, generator=torch.Generator().manual_seed(5))
    for inverse in (False, True):
        label = _against_layer_by_layer("k8x_bias_lds_" + case + ("_inverse" if inverse else ""), f16x3, flow_cpu, x, inverse,
                                        bias=bias)[3]
        assert ("inverse=1" in label) == inverse, label
        assert ("init_ks=4" in label) == (case == "d100_init_ks4"), label
        assert ("K=10," in label) == (case == "ten_bins") and ("K=20," in label) == (bias == "global"), label


def test_launch_order_leaves_no_stale_area(f16x3):
    """five layers, two layers, five layers again on one stream: the first and the third results are the same bits"""
    five = copy.deepcopy(_flow(5, seed=11)).to(DEV).eval()
    two = copy.deepcopy(_flow(2, seed=12)).to(DEV).eval()
    import nflows_amd
    from nflows_amd import ops
    x = torch.randn(2048, 64, generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        z1, lad1 = five._transform(x)
        _ran_k8x()
        assert ops.last_redo_blocks() == 0   # (a redone block would hold the exact kernel's bits both times)
        two._transform(x)
        _ran_k8x()
        z3, lad3 = five._transform(x)
        _ran_k8x()
        assert ops.last_redo_blocks() == 0
    nflows_amd.check_status()
    assert torch.isfinite(z1).all() and torch.equal(z1, z3) and torch.equal(lad1, lad3)
