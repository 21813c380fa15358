"""K8x's wide form: one eight-wave workgroup per CU on one weight ring (rqs_resnet_f16x3_kernel.hpp, WAVES = 8) instead of two
four-wave workgroups with a ring each.  Every wave runs the narrow form's program on its 32 rows -- same fragments, same
order --, so the two forms must agree BIT FOR BIT: every case runs the forced-narrow and the forced-wide form
(`ops.K8X_FORM`) on the same inputs and asserts `torch.equal` on z (or x), logabsdet and log_prob, and that the kernel's
name says which form ran (`waves=8, ` in front of `bias=`).  "Both forms wrong alike" is excluded by one case held against
the layer-by-layer path under the 2 x rule, as in tests/test_gpu_k8x_bias_lds.py.
  * carried state: 131 072 rows -- a wide workgroup makes two passes on up to 511 CUs (ring, bias area and tables go on);
  * tails: 128 rows (a lone lower half: the upper half recomputes it and stores nothing), 384 (a pair and an odd block),
    256 (one workgroup, no tail);
  * geometries: no, one, two residual blocks; D = 100 (`init_ks=4`), whose eight row tiles do not fit the LDS beside the
    ring: the launcher takes the narrow form even when the wide one is asked for;
  * redo granularity: the flag is per 128 rows, not per workgroup;
  * the launcher's own choice.
"""
import copy

import pytest
import torch

from test_gpu_k8x_bias_lds import _against_layer_by_layer, _flow, f16x3   # noqa: F401  (f16x3: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NARROW, WIDE = 1, 2


def _label():
    from nflows_amd import ops
    return ops.last_layer_kernel()


def _assert_form(form):
    label = _label()
    assert "k8x::rqs_resnet_f16x3_kernel" in label and label.endswith("bias=lds>"), label
    assert ("waves=8, bias=" in label) == (form == WIDE), (form, label)


def _forced(monkeypatch, form, flow, xd, inverse, expect=None):
    """(y, logabsdet, log_prob) of the whole-layer kernel in the form asked for; `expect`: the form that must have run"""
    import nflows_amd
    from nflows_amd import ops
    monkeypatch.setattr(ops, "K8X_FORM", form)
    expect = form if expect is None else expect
    with torch.no_grad():
        if inverse:
            y, lad = flow._transform.inverse(xd)
            lp = None
        else:
            y, lad = flow._transform(xd)
            _assert_form(expect)
            lp = flow.log_prob(xd)
        _assert_form(expect)
    nflows_amd.check_status()
    return y, lad, lp


def _same_bits(monkeypatch, flow_cpu, x, inverse, expect_wide=WIDE):
    from nflows_amd import ops
    flow = copy.deepcopy(flow_cpu).to(DEV).eval()
    xd = x.to(DEV)
    yn, ladn, lpn = _forced(monkeypatch, NARROW, flow, xd, inverse)
    assert ops.last_redo_blocks() == 0   # (a redone block would hold the exact kernel's bits both times)
    yw, ladw, lpw = _forced(monkeypatch, WIDE, flow, xd, inverse, expect=expect_wide)
    assert ops.last_redo_blocks() == 0
    assert torch.isfinite(yn).all() and torch.isfinite(ladn).all()
    assert torch.equal(yn, yw) and torch.equal(ladn, ladw)
    if not inverse:
        assert torch.equal(lpn, lpw)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_state_carried_across_the_passes_of_a_wide_workgroup(f16x3, monkeypatch, inverse):
    B = 131072
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus >= B // 256:
        pytest.skip("%d CUs: no wide workgroup makes a second pass over %d rows" % (cus, B))
    x = torch.randn(B, 64, generator=torch.Generator().manual_seed(41 + inverse))
    _same_bits(monkeypatch, _flow(3), x, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("rows", [128, 384, 256])
def test_tails(f16x3, monkeypatch, rows, inverse):
    x = torch.randn(rows, 64, generator=torch.Generator().manual_seed(rows + inverse))
    _same_bits(monkeypatch, _flow(2, seed=3), x, inverse)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_odd_tail_against_layer_by_layer(f16x3, monkeypatch, inverse):
    """384 rows in the wide form (a pair and an odd block) against the path without any whole-layer kernel"""
    from nflows_amd import ops
    monkeypatch.setattr(ops, "K8X_FORM", WIDE)
    x = torch.randn(384, 64, generator=torch.Generator().manual_seed(17 + inverse))
    label = _against_layer_by_layer("k8x_wide_odd_tail" + ("_inverse" if inverse else ""), f16x3, _flow(3), x, inverse)[3]
    assert "waves=8, bias=lds>" in label and ("inverse=1" in label) == inverse, label


@pytest.mark.parametrize("num_blocks", [0, 1, 2])
def test_geometries(f16x3, monkeypatch, num_blocks):
    """384 rows, two layers: the stages of a layer are 2 + 16 blocks + 48, pairs of them never straddle a layer"""
    flow_cpu = _flow(2, seed=7, num_blocks=num_blocks)
    x = torch.randn(384, 64, generator=torch.Generator().manual_seed(5))
    for inverse in (False, True):
        _same_bits(monkeypatch, flow_cpu, x, inverse)
        assert ("inverse=1" in _label()) == inverse


def test_d100_takes_the_narrow_form(f16x3, monkeypatch):
    """D = 100: eight [100][33] row tiles beside the 72 KB ring are past the launch's LDS -- the narrow form runs, asked or not"""
    flow_cpu = _flow(2, seed=7, features=100)
    x = torch.randn(384, 100, generator=torch.Generator().manual_seed(5))
    for inverse in (False, True):
        _same_bits(monkeypatch, flow_cpu, x, inverse, expect_wide=NARROW)
        assert "init_ks=4" in _label()


def test_redo_is_per_128_rows(f16x3, monkeypatch):
    """512 rows, one value of 1e30 in a row of block 1 (the upper half of workgroup 0): block 1 alone is flagged and redone by
    the exact kernel; blocks 0, 2 and 3 hold the narrow form's bits, and so do the final results."""
    import nflows_amd
    from nflows_amd import ops
    flow = copy.deepcopy(_flow(2, seed=3)).to(DEV).eval()
    x = torch.randn(512, 64, generator=torch.Generator().manual_seed(77))
    x[128 + 5, 3] = 1e30
    xd = x.to(DEV)
    got = {}
    for form in (NARROW, WIDE):
        monkeypatch.setattr(ops, "K8X_FORM", form)
        with torch.no_grad():
            z, lad = flow._transform(xd)
        _assert_form(form)
        got[form] = (z, lad, ops._last_redo.clone())
        try:
            nflows_amd.check_status()
        except (AssertionError, IndexError, ValueError, RuntimeError):   # (the huge value may set the reference's own flags)
            pass
    for form in (NARROW, WIDE):
        assert got[form][2].tolist() == [0, 1, 0, 0], (form, got[form][2].tolist())
    (zn, ladn, _), (zw, ladw, _) = got[NARROW], got[WIDE]
    keep = torch.ones(512, dtype=torch.bool, device=DEV)
    keep[128:256] = False
    assert torch.isfinite(zn[keep]).all() and torch.isfinite(ladn[keep]).all()
    assert torch.equal(zn[keep], zw[keep]) and torch.equal(ladn[keep], ladw[keep])
    # (block 1: the exact kernel's results both times; bit patterns, whatever the huge value made of its row)
    assert torch.equal(zn.view(torch.int32), zw.view(torch.int32))
    assert torch.equal(ladn.view(torch.int32), ladw.view(torch.int32))


def test_launcher_choice(f16x3, monkeypatch):
    """auto: the wide form from two 128-row blocks per CU (csrc/rqs_resnet_f16x3_kernel.hpp: kWideBlocksPerCu), where it exists"""
    from nflows_amd import ops
    monkeypatch.setattr(ops, "K8X_FORM", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    flow = copy.deepcopy(_flow(2, seed=3)).to(DEV).eval()
    with torch.no_grad():
        for rows in (32768, 131072):
            flow._transform(torch.randn(rows, 64, device=DEV))
            assert ("waves=8, " in _label()) == (rows // 128 >= 2 * cus), (rows, cus, _label())
        ten = copy.deepcopy(_flow(2, seed=3, num_bins=10)).to(DEV).eval()
        ten._transform(torch.randn(131072, 64, device=DEV))
        assert "K=10," in _label() and "waves=8" not in _label(), _label()
        wide = copy.deepcopy(_flow(2, seed=3, features=128)).to(DEV).eval()
        wide._transform(torch.randn(131072, 128, device=DEV))
        assert "k8x::" in _label() and "waves=8" not in _label(), _label()
