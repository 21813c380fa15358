"""K8x after the round-10 VALU cuts: the activations' last piece made as bf8 directly (f16x3_gemm.hpp: split3_scaled's
v_cvt_scalef32_pk_bf8_f32 in place of an f16 piece whose high byte was picked out afterwards) and the softplus correction
without its reciprocal (rqs_fused8.hpp).  Engine f16x3, D = 64, 8 bins, 2 layers x 2 blocks, both directions:
  * 128 rows run the narrow form; 256 and 384 rows are forced wide (384: an odd number of row blocks, the upper half of the
    second workgroup recomputes the lower one's rows and stores nothing);
  * outputs and log-determinants against the layer-by-layer path under the 2 x rule, the truth being the float64 port
    (tests/test_gpu_k8x_bias_lds.py: _against_layer_by_layer -> tests/test_gpu_headline_parity.compare);
  * the two forms agree bit for bit (tests/test_gpu_k8x_wide.py: _same_bits);
  * one input of 1e6: at the pieces' scale it leaves the f16 range, hi = inf, and the NaN that d = t - lo then is goes
    through the bf8 conversion as a NaN byte -- its row block is flagged, redone by the exact kernel (K8) and holds K8's bits;
    the other block is not flagged and holds what it holds without the large input.
"""
import copy

import pytest
import torch

from test_gpu_k8x_bias_lds import _against_layer_by_layer, _flow, f16x3   # noqa: F401  (f16x3: the fixture)
from test_gpu_k8x_wide import NARROW, WIDE, _assert_form, _same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = {128: NARROW, 256: WIDE, 384: WIDE}


@pytest.fixture(scope="module")
def flow_cpu():
    return _flow(2, seed=21)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("rows", [128, 256, 384])
def test_against_the_float64_path(f16x3, monkeypatch, flow_cpu, rows, inverse):
    from nflows_amd import ops
    monkeypatch.setattr(ops, "K8X_FORM", FORMS[rows])
    x = torch.randn(rows, 64, generator=torch.Generator().manual_seed(rows + 7 * inverse))
    config = "k8x_valu_diet_%d_%s" % (rows, "inverse" if inverse else "forward")
    label = _against_layer_by_layer(config, f16x3, flow_cpu, x, inverse)[3]
    assert ("waves=8, bias=" in label) == (FORMS[rows] == WIDE) and ("inverse=1" in label) == inverse, label


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("rows", [128, 256, 384])
def test_the_two_forms_are_bit_identical(f16x3, monkeypatch, flow_cpu, rows, inverse):
    x = torch.randn(rows, 64, generator=torch.Generator().manual_seed(100 + rows + inverse))
    _same_bits(monkeypatch, flow_cpu, x, inverse)


@pytest.mark.parametrize("form", [NARROW, WIDE], ids=["narrow", "wide"])
def test_one_large_input_flags_its_row_block_alone(f16x3, monkeypatch, flow_cpu, form):
    import nflows_amd
    from nflows_amd import ops
    monkeypatch.setattr(ops, "K8X_FORM", form)
    flow = copy.deepcopy(flow_cpu).to(DEV).eval()
    x = torch.randn(256, 64, generator=torch.Generator().manual_seed(55))
    clean = x.to(DEV)
    # (an identity feature of the first layer, whichever column the layer's permutation takes it from: it enters the
    #  first GEMM's pieces.  A column both layers transform would be passed through untouched, outside the box.)
    layers = flow_cpu._transform._transforms
    column = int(layers[0]._permutation[layers[1].identity_features[0]])
    x[128 + 9, column] = 1e6
    xd = x.to(DEV)
    with torch.no_grad():
        z, lad = flow._transform(xd)
        _assert_form(form)
        flags = ops._last_redo.clone()
        z0, lad0 = flow._transform(clean)
        assert ops.last_redo_blocks() == 0
        f16x3.conditioner_engine = "bf16x3"
        z8, lad8 = flow._transform(xd)
        assert "rqs_resnet_kernel<" in ops.last_layer_kernel()
    try:
        nflows_amd.check_status()
    except (AssertionError, IndexError, ValueError, RuntimeError):   # (the large value may set the reference's own flags)
        pass
    assert flags.tolist() == [0, 1], flags.tolist()
    # the flagged block: the exact kernel's bits; the other one: untouched by its neighbour's redo
    assert torch.equal(z[128:].view(torch.int32), z8[128:].view(torch.int32))
    assert torch.equal(lad[128:].view(torch.int32), lad8[128:].view(torch.int32))
    assert torch.isfinite(z[:128]).all() and torch.isfinite(lad[:128]).all()
    assert torch.equal(z[:128], z0[:128]) and torch.equal(lad[:128], lad0[:128])
