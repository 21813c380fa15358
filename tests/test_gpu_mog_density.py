"""K31 on the device (csrc/made_mog.hip, ops.made_mog_log_prob, nn.nde.MixtureOfGaussiansMADE.log_prob): every case of
tests/mog_density_cases.py against the float64 truth under the project's parity rule with the module in float32 on the CPU
as the yardstick, the rows' independence and determinism bit for bit, the `logabsdet` term, the launches, and the gate."""
import copy

import numpy as np
import pytest
import torch

import mog_density_cases as C
from density_cases import module_inputs, truth
from maf_inverse_cases import assert_parity
from nflows_amd import ops
from nflows_amd.distributions import MADEMoG
from nflows_amd.nn.nde import MixtureOfGaussiansMADE
from test_density_host import mademog_from_fixture
from test_gpu_nonlinearities import launches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOOK = "made_mog_log_prob"


def on_device(name, rows=None):
    made, x, ctx, ref32, truth64 = C.reference(name, rows)
    return copy.deepcopy(made).to(DEV), x.to(DEV), None if ctx is None else ctx.to(DEV), ref32, truth64


@pytest.mark.parametrize("name", list(C.CASES))
def test_parity_with_the_truth(name, monkeypatch):
    monkeypatch.setattr(MixtureOfGaussiansMADE, "_DENSITY_KERNEL_LOSES", ())   # the kernel itself, whatever the size rule
    made, x, ctx, ref32, truth64 = on_device(name)
    K, served = made.num_mixture_components, made.num_mixture_components <= 16
    with torch.no_grad():
        calls = launches(lambda: made.log_prob(x, context=ctx))
        got = made.log_prob(x, context=ctx)
    assert calls == ([HOOK] if served else ["mog"]), calls
    if served:
        residual = int(ops._made_residual(made))
        assert ops.last_layer_kernel() == "made_mog_kernel<K=%d, resnet=%d, context=%d>" % (K, residual, int(ctx is not None))
    assert got.shape == (x.shape[0],) and got.dtype == torch.float32
    assert_parity(got.cpu().numpy(), ref32, truth64, name)


def test_rows_are_independent_and_repeatable_bit_for_bit():
    """128 x (CU count + 1) rows: one workgroup makes a second pass of the persistent loop."""
    name = "d5_k5_c3"
    rows = 128 * (torch.cuda.get_device_properties(0).multi_processor_count + 1)
    made, x, ctx, ref32, truth64 = on_device(name, rows)
    with torch.no_grad():
        whole = made.log_prob(x, context=ctx)
        again = made.log_prob(x, context=ctx)
        head = made.log_prob(x[:128], context=ctx[:128])
    assert ops.last_layer_kernel().startswith("made_mog_kernel")
    assert torch.equal(whole, again) and torch.equal(whole[:128], head)
    assert_parity(whole.cpu().numpy(), ref32, truth64, name + " large batch")


@pytest.mark.parametrize("name", ["d5_k5_c3", "d33_k10_ragged"])
def test_logabsdet_joins_the_float64_sum(name):
    made, x, ctx, ref32, truth64 = on_device(name)
    add = 37.0 * torch.randn(x.shape[0], generator=torch.Generator().manual_seed(3))
    got = made._density_kernel(x, ctx, logabsdet=add.to(DEV))
    assert got is not None
    assert_parity(got.cpu().numpy(), (torch.from_numpy(ref32) + add).numpy(), truth64 + add.double().numpy(), name + " + add")


def test_switches_give_todays_launches(monkeypatch):
    torch.manual_seed(5)
    dist = MADEMoG(features=6, hidden_features=32, context_features=3, num_blocks=2, num_mixture_components=5).to(DEV).eval()
    x, ctx = torch.randn(256, 6, device=DEV), torch.randn(256, 3, device=DEV)
    with torch.no_grad():
        served = launches(lambda: dist.log_prob(x, context=ctx))
        kernel = dist.log_prob(x, context=ctx)
        monkeypatch.setattr(MixtureOfGaussiansMADE, "_use_density_kernel", False)
        before = launches(lambda: dist.log_prob(x, context=ctx))
        parts = dist.log_prob(x, context=ctx)
        monkeypatch.setattr(MixtureOfGaussiansMADE, "_use_kernel", False)
        monkeypatch.setattr(MixtureOfGaussiansMADE, "_use_density_kernel", True)
        generic = launches(lambda: dist.log_prob(x, context=ctx))
    assert served == [HOOK] and before == ["mog"] and generic == []
    assert float((kernel - parts).abs().max()) <= 1e-4 * (1.0 + float(parts.abs().max()))


@pytest.mark.parametrize("how", ["input_requires_grad", "double", "batch_norm", "dropout_in_training"])
def test_gate_keeps_the_old_path(how, monkeypatch):
    kw = dict(features=6, hidden_features=32, context_features=3, num_blocks=2, num_mixture_components=5)
    torch.manual_seed(6)
    made = MixtureOfGaussiansMADE(use_batch_norm=how == "batch_norm", dropout_probability=0.5 if how.startswith("dropout") else 0.0,
                                  **kw).to(DEV).eval()
    x, ctx = torch.randn(256, 6, device=DEV), torch.randn(256, 3, device=DEV)
    if how == "double":
        made, x, ctx = made.double(), x.double(), ctx.double()
    if how == "dropout_in_training":
        made.train()
    if how == "input_requires_grad":
        x.requires_grad_(True)
        calls, got = launches(lambda: made.log_prob(x, context=ctx)), made.log_prob(x, context=ctx)
        assert got.grad_fn is not None
    else:
        with torch.no_grad():
            calls = launches(lambda: made.log_prob(x, context=ctx))
            torch.manual_seed(1)
            got = made.log_prob(x, context=ctx)
    assert HOOK not in calls, calls
    monkeypatch.setattr(MixtureOfGaussiansMADE, "_use_density_kernel", False)
    with torch.no_grad():
        torch.manual_seed(1)     # (the dropout masks)
        want = made.log_prob(x, context=ctx)
    assert torch.equal(got.detach(), want)


def test_real_reference_fixture():
    """The reference's own MADEMoG vectors (tests/golden/density_mademog.npz), through the kernel's op: the class keeps
    the fixture's 64 rows, fewer than a block, on the old path."""
    d, g = mademog_from_fixture()
    made = d._made.to(DEV)
    x, ctx = (torch.from_numpy(a).to(DEV) for a in module_inputs("mademog"))
    with torch.no_grad():
        assert HOOK not in launches(lambda: made.log_prob(x, context=ctx))
        got = made._density_kernel(x, ctx)
    assert_parity(got.cpu().numpy(), g["log_prob"], truth(g, "log_prob"), "reference fixture")
