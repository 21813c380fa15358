"""K8x at bench.py's full batch: every workgroup walks several row blocks (quad loop of rqs_resnet_f16x3_kernel.hpp), so the
state carried from one row block to the next -- the running log-determinant, the status words, the table of the next
layer, the redo flag -- is exercised where the other K8x tests (at most 65 536 rows: one or two row blocks per workgroup)
do not reach.  Same rules as tests/test_gpu_k8x.py: the 2 x rule against the float64 oracle, K8's bits on redone blocks.
"""
import copy

import pytest
import torch

from helpers import LAD_TOL, OUT_TOL
from test_gpu_headline_parity import compare, oracle_eval

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def f16x3(monkeypatch):
    import nflows_amd
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ
    monkeypatch.setattr(RQ, "conditioner_engine", "f16x3")
    try:   # (the device status word is sticky)
        nflows_amd.check_status()
    except (AssertionError, IndexError, ValueError, RuntimeError):
        pass
    return RQ


def _ran_k8x(inverse):
    from nflows_amd import ops
    label = ops.last_layer_kernel()
    assert "k8x::rqs_resnet_f16x3_kernel" in label, label
    assert ("inverse=1" in label) == inverse, label


def _grid():
    # the launch: two workgroups per CU at D = 64 (rqs_resnet_f16x3.hip), row block q runs on workgroup q % grid
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def _flow():
    from nflows_amd import configs
    return configs.rq_nsf_flow(num_layers=32, features=64, num_bins=8, hidden_features=128, seed=0).eval()


def test_log_prob_at_the_bench_batch(f16x3):
    """262 144 rows (bench.py's batch: four row blocks per workgroup on a 256-CU part): log_prob against the oracle on
    rows of the second and of the last row block each workgroup runs."""
    import nflows_amd
    from nflows_amd import ops
    B = 262144
    grid = _grid()
    passes = B // 128 // grid
    assert passes >= 2, "fewer than two row blocks per workgroup: %d workgroups" % grid
    flow_cpu = _flow()
    x = torch.randn(B, 64, generator=torch.Generator().manual_seed(4321))
    flow = copy.deepcopy(flow_cpu).to(DEV).eval()
    with torch.no_grad():
        lp = flow.log_prob(x.to(DEV))
        _ran_k8x(False)
        assert ops.last_redo_blocks() == 0
    nflows_amd.check_status()
    # 4 096 rows from the second pass over the grid, 4 096 from the last
    rows = torch.cat([torch.arange(4096) + grid * 128, torch.arange(4096) + (passes - 1) * grid * 128])
    o = oracle_eval(flow_cpu, x[rows], need=("lp",))
    compare("k8x_rowblocks_262144", "log_prob", lp[rows.to(DEV)].cpu().numpy(), o["lp32"], o["lp64"], LAD_TOL)


def test_inverse_at_half_the_bench_batch(f16x3):
    """131 072 rows through the inverse (two row blocks per workgroup): inverse(forward(x)) against the reference's own
    fp32 round trip on rows of the second row block of each workgroup, z against the oracle there."""
    import nflows_amd
    from nflows_amd import ops
    from oracle import eager
    B = 131072
    grid = _grid()
    flow_cpu = _flow()
    x = torch.randn(B, 64, generator=torch.Generator().manual_seed(8765))
    flow = copy.deepcopy(flow_cpu).to(DEV).eval()
    xd = x.to(DEV)
    with torch.no_grad():
        z, _ = flow._transform(xd)
        _ran_k8x(False)
        xr, _ = flow._transform.inverse(z)
        _ran_k8x(True)
        assert ops.last_redo_blocks() == 0
    nflows_amd.check_status()
    rows = torch.arange(4096) + (B // 128 // grid - 1) * grid * 128
    o = oracle_eval(flow_cpu, x[rows], need=("z",))
    compare("k8x_rowblocks_inverse", "z", z[rows.to(DEV)].cpu().numpy(), o["z32"], o["z64"], OUT_TOL)
    with torch.no_grad():
        xr_ref, _ = eager.flow_transform(flow_cpu, torch.from_numpy(o["z32"]), inverse=True)
    err = (xr[rows.to(DEV)].cpu() - x[rows]).abs()
    ref = (xr_ref - x[rows]).abs()
    assert float(err.mean()) <= 2.0 * float(ref.mean())


def test_redo_in_later_row_blocks_of_one_workgroup(f16x3):
    """A row that leaves the f16 range in the 2nd and in the 4th row block workgroup 0 runs (an infinite input, a NaN: a
    merely large row is no test -- outside the spline's box every feature is the identity and the poisoned logits are
    never used): exactly those two blocks are redone by K8 (its bits there), every other row keeps the clean run's bits."""
    import nflows_amd
    from nflows_amd import ops
    B = 262144
    grid = _grid()
    assert B // 128 // grid >= 4, "fewer than four row blocks per workgroup: %d workgroups" % grid
    flow_cpu = _flow()
    x = torch.randn(B, 64, generator=torch.Generator().manual_seed(2468))
    q2, q4 = grid, 3 * grid             # workgroup 0's second and fourth row blocks
    xb = x.clone()
    xb[q2 * 128 + 5, 3] = float("inf")
    xb[q4 * 128 + 77, 10] = float("nan")
    flow = copy.deepcopy(flow_cpu).to(DEV).eval()
    with torch.no_grad():
        z0, lad0 = flow._transform(x.to(DEV))
        _ran_k8x(False)
        assert ops.last_redo_blocks() == 0
        z, lad = flow._transform(xb.to(DEV))
        _ran_k8x(False)
        flags = ops._last_redo.clone()
        assert ops.last_redo_blocks() == 2
        f16x3.conditioner_engine = "bf16x3"
        z8, lad8 = flow._transform(xb.to(DEV))
        assert "rqs_resnet_kernel<" in ops.last_layer_kernel()
    try:
        nflows_amd.check_status()
    except AssertionError:   # (non-finite inputs set the reference's own flags)
        pass
    assert flags[q2] != 0 and flags[q4] != 0
    redo = (flags != 0).repeat_interleave(128)
    assert torch.equal(torch.nan_to_num(z[redo], nan=7.0), torch.nan_to_num(z8[redo], nan=7.0))
    assert torch.equal(torch.nan_to_num(lad[redo], nan=7.0), torch.nan_to_num(lad8[redo], nan=7.0))
    keep = ~redo
    assert torch.equal(z[keep], z0[keep]) and torch.equal(lad[keep], lad0[keep])
