"""The learned base densities without a GPU: every name the reference's `distributions` and `nn.nde` export exists, state_dict
keys and buffer persistence equal the reference's (tests/golden/density_mademog.npz, density_flow.npz), the reference's error
messages are raised, the generic path on CPU tensors meets the fixtures in float32 and float64, and the library exports
K20's entry points at ABI 19."""
import numpy as np
import pytest
import torch

from density_cases import (DIAG_MODES, DIAG_SHAPES, EPSILON, MADEMOG, MOG_CASES, conditional_flow, diag_inputs, golden,
                           module_inputs, mog_inputs, tag, truth)
from helpers import LAD_TOL, OUT_TOL
from test_gpu_headline_parity import compare


def test_every_exported_name_imports():
    from nflows_amd import autograd, distributions, nn, ops
    for name in ("Distribution", "NoMeanException", "StandardNormal", "ConditionalDiagonalNormal", "DiagonalNormal", "MADEMoG",
                 "ConditionalIndependentBernoulli", "MG1Uniform", "LotkaVolterraOscillating"):
        assert hasattr(distributions, name), name
    from nflows_amd.distributions.uniform import BoxUniform  # noqa: F401
    assert hasattr(nn.nde, "MADE") and hasattr(nn.nde, "MixtureOfGaussiansMADE")
    assert callable(ops.diag_normal_log_prob) and callable(ops.mog_log_prob)
    assert hasattr(autograd, "DiagNormalLogProb") and hasattr(autograd, "MoGLogProb")


def test_the_density_made_does_not_import_matplotlib():
    import subprocess
    import sys
    code = "import sys; import nflows_amd.nn.nde, nflows_amd.distributions; sys.exit(1 if 'matplotlib' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


def _nf():
    import types
    from nflows_amd import distributions as D, flows, transforms as T
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.utils import torchutils
    return types.SimpleNamespace(PiecewiseRationalQuadraticCouplingTransform=T.PiecewiseRationalQuadraticCouplingTransform,
                                 create_alternating_binary_mask=torchutils.create_alternating_binary_mask,
                                 ResidualNet=ResidualNet, ReversePermutation=T.ReversePermutation, Flow=flows.Flow,
                                 CompositeTransform=T.CompositeTransform, ConditionalDiagonalNormal=D.ConditionalDiagonalNormal)


def _state(g):
    return {k[len("state/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("state/")}


def mademog_from_fixture():
    from nflows_amd.distributions import MADEMoG
    g = golden("mademog")
    d = MADEMoG(**MADEMOG)
    assert list(d.state_dict().keys()) == list(_state(g).keys())
    d.load_state_dict(_state(g), strict=True)
    return d.eval(), g


def flow_from_fixture():
    g = golden("flow")
    flow = conditional_flow(_nf())
    assert list(flow.state_dict().keys()) == list(_state(g).keys())
    flow.load_state_dict(_state(g), strict=True)
    return flow.eval(), g


def test_state_dict_keys_and_buffers_equal_the_references():
    from nflows_amd.distributions import ConditionalDiagonalNormal, DiagonalNormal
    d, _ = mademog_from_fixture()
    assert "_made.final_layer.mask" in d.state_dict() and "_made.blocks.0.context_layer.weight" in d.state_dict()
    flow_from_fixture()
    n = DiagonalNormal([5])
    assert list(n.state_dict().keys()) == ["mean_", "log_std_"] and tuple(n.mean_.shape) == (1, 5)
    assert n._log_z.dtype == torch.float64 and "_log_z" in dict(n.named_buffers())       # non-persistent, as the reference's
    c = ConditionalDiagonalNormal([5], context_encoder=torch.nn.Linear(3, 10))
    assert list(c.state_dict().keys()) == ["_context_encoder.weight", "_context_encoder.bias"]
    assert float(c._log_z) == pytest.approx(2.5 * np.log(2 * np.pi), rel=1e-15)
    assert n.mean() is n.mean_
    with pytest.raises(NotImplementedError):
        n.sample(3)


def test_the_references_error_messages():
    from nflows_amd.distributions import ConditionalDiagonalNormal, ConditionalIndependentBernoulli, DiagonalNormal, MADEMoG
    from nflows_amd.nn.nde import MADE, MixtureOfGaussiansMADE
    from nflows_amd.nn.nde.made import MaskedResidualBlock
    x = torch.randn(4, 3)
    c = ConditionalDiagonalNormal([3])
    with pytest.raises(RuntimeError, match="The context encoder must return a tensor whose last dimension is even."):
        c.log_prob(x, context=torch.randn(4, 5))
    bad = ConditionalDiagonalNormal([3], context_encoder=lambda ctx: ctx[:2])
    with pytest.raises(RuntimeError, match="The batch dimension of the parameters is inconsistent with the input."):
        bad.log_prob(x, context=torch.randn(4, 6))
    with pytest.raises(ValueError, match="Context can't be None."):
        c.log_prob(x)
    with pytest.raises(ValueError, match="Number of input items must be equal to number of context items."):
        c.log_prob(x, context=torch.randn(5, 6))
    for dist, ctx in ((c, torch.randn(4, 6)), (DiagonalNormal([3]), None), (ConditionalIndependentBernoulli([3]), torch.randn(4, 3))):
        with pytest.raises(ValueError, match=r"Expected input of shape torch.Size\(\[3\]\), got torch.Size\(\[2\]\)"):
            dist.log_prob(torch.randn(4, 2), context=ctx)
    b = ConditionalIndependentBernoulli([3])
    with pytest.raises(ValueError, match="Context can't be None."):
        b.log_prob(x)
    for build in (lambda: MADE(4, 8, random_mask=True), lambda: MixtureOfGaussiansMADE(4, 8, random_mask=True),
                  lambda: MADEMoG(4, 8, None, random_mask=True)):
        with pytest.raises(ValueError, match="Residual blocks can't be used with random masks."):
            build()
    with pytest.raises(ValueError, match="Masked residual block can't be used with random masks."):
        MaskedResidualBlock(torch.arange(1, 5), 4, random_mask=True)
    MADE(4, 8, use_residual_blocks=False, random_mask=True)      # feed-forward blocks take random masks


def _leaf(a, dt):
    return torch.from_numpy(a).to(dt).requires_grad_(True)


def assert_float64(got, g, name, what, rel=1e-12):
    """A float64 result against the fixture's float64, which is held as float32 + a float32 difference: 2^-24 of the largest
    difference is the fixture's own resolution."""
    want = truth(g, name)
    err = float(np.abs(got - want).max())
    assert err <= rel * (1 + float(np.abs(want).max())) + 2.0 ** -24 * float(np.abs(g[name + "_d"]).max()), (what, err)


def _hold(config, names, got32, got64, g, tols):
    for name, a32, a64, tol in zip(names, got32, got64, tols):
        compare(config, name, a32.detach().numpy(), g[name], truth(g, name), tol)
        assert_float64(a64.detach().numpy(), g, name, (config, name))


@pytest.mark.parametrize("shape", DIAG_SHAPES, ids=tag)
@pytest.mark.parametrize("mode", DIAG_MODES)
def test_generic_diag_on_cpu_tensors_meets_the_fixtures(mode, shape):
    from nflows_amd.distributions import ConditionalDiagonalNormal, DiagonalNormal
    g = golden("diag_%s_%s" % (mode, tag(shape)))
    got = []
    for dt in (torch.float32, torch.float64):
        if mode == "shared":
            x, r, means, log_stds = diag_inputs(mode, shape)
            d = DiagonalNormal(list(shape[1:])).to(dt)
            d.mean_.data, d.log_std_.data = torch.from_numpy(means).to(dt), torch.from_numpy(log_stds).to(dt)
            xt = _leaf(x, dt)
            lp = d.log_prob(xt)
            (lp * torch.from_numpy(r).to(dt)).sum().backward()
            got.append((lp, xt.grad, d.mean_.grad, d.log_std_.grad))
            names = ("log_prob", "g_x", "g_means", "g_log_stds")
        else:
            x, r, params = diag_inputs(mode, shape)
            xt, pt = _leaf(x, dt), _leaf(params, dt)
            lp = ConditionalDiagonalNormal(list(shape[1:])).to(dt).log_prob(xt, context=pt)
            (lp * torch.from_numpy(r).to(dt)).sum().backward()
            got.append((lp, xt.grad, pt.grad))
            names = ("log_prob", "g_x", "g_params")
    _hold("generic diag %s %s" % (mode, tag(shape)), names, got[0], got[1], g, (LAD_TOL,) + (OUT_TOL,) * 3)


@pytest.mark.parametrize("kind,shape", MOG_CASES, ids=lambda v: v if isinstance(v, str) else tag(v))
def test_generic_mog_on_cpu_tensors_meets_the_fixtures(kind, shape):
    from nflows_amd.nn.nde.made import mog_log_prob_generic
    g = golden("mog_%s_%s" % (kind, tag(shape)))
    x, r, outputs = mog_inputs(kind, shape)
    got = []
    for dt in (torch.float32, torch.float64):
        xt, ot = _leaf(x, dt), _leaf(outputs, dt)
        lp = mog_log_prob_generic(xt, ot, shape[2], EPSILON)
        (lp * torch.from_numpy(r).to(dt)).sum().backward()
        got.append((lp, xt.grad, ot.grad))
    _hold("generic mog %s %s" % (kind, tag(shape)), ("log_prob", "g_x", "g_outputs"), got[0], got[1], g, (LAD_TOL, OUT_TOL, OUT_TOL))


def test_module_fixtures_on_the_cpu():
    d, g = mademog_from_fixture()
    x, ctx = (torch.from_numpy(a) for a in module_inputs("mademog"))
    with torch.no_grad():
        lp = d.log_prob(x, context=ctx)
        lp64 = d.double().log_prob(x.double(), context=ctx.double())
    _hold("generic MADEMoG", ("log_prob",), (lp,), (lp64,), g, (LAD_TOL,))
    # (the conditional flow's couplings have no CPU path: its fixture is held on the GPU, tests/test_gpu_density.py)


def test_sampling_on_the_cpu_follows_the_references_random_stream():
    """MixtureOfGaussiansMADE.sample: per feature one Categorical draw, then one randn(rows) (made.py:378-386)."""
    import torch.nn.functional as F
    d, _ = mademog_from_fixture()
    made = d._made
    ctx = torch.from_numpy(module_inputs("mademog")[1][:5])
    torch.manual_seed(3)
    got = d.sample(4, context=ctx)
    assert got.shape == (5, 4, 7) and torch.isfinite(got).all()
    torch.manual_seed(3)
    rows = ctx.repeat_interleave(4, dim=0)
    want = torch.zeros(20, 7)
    with torch.no_grad():
        for f in range(7):
            o = made.forward(want, rows).reshape(20, 7, 5, 3)
            comp = torch.distributions.Categorical(logits=torch.log_softmax(o[:, f, :, 0], dim=-1)).sample((1,)).reshape(-1, 1)
            stds = F.softplus(o[:, f, :, 2]) + made.epsilon
            want[:, f] = o[:, f, :, 1].gather(1, comp).reshape(-1) + torch.randn(20) * stds.gather(1, comp).reshape(-1)
    assert torch.equal(got, want.reshape(5, 4, 7))


def test_the_stock_op_distributions():
    from nflows_amd.distributions import ConditionalIndependentBernoulli, LotkaVolterraOscillating, MG1Uniform
    from nflows_amd.distributions.uniform import BoxUniform
    torch.manual_seed(0)
    b = ConditionalIndependentBernoulli([2, 3])
    logits = torch.randn(5, 6)
    s = b.sample(4, context=logits)
    assert s.shape == (5, 4, 2, 3) and set(s.unique().tolist()) <= {0.0, 1.0}
    x = (torch.rand(5, 2, 3) < 0.5).float()
    want = -(torch.nn.functional.binary_cross_entropy_with_logits(logits.reshape(5, 2, 3), x, reduction="none")).sum((1, 2))
    assert torch.allclose(b.log_prob(x, context=logits), want, atol=1e-5)
    assert torch.equal(b.mean(logits), torch.sigmoid(logits).reshape(5, 2, 3))
    box = BoxUniform(torch.zeros(3), torch.ones(3) * 2)
    assert box.log_prob(torch.ones(4, 3)).shape == (4,)
    m = MG1Uniform(low=torch.zeros(3), high=torch.tensor([10.0, 10.0, 1.0 / 3.0]))
    p = m.sample((100,))
    assert p.shape == (100, 3) and torch.all(p[:, 1] >= p[:, 0]) and torch.isfinite(m.log_prob(p)).all()
    lv = LotkaVolterraOscillating()
    p = lv.sample((50,))
    assert p.shape == (50, 4) and torch.all(p >= -5) and torch.all(p < 2) and torch.isfinite(lv.log_prob(p)).all()


def test_library_exports_k20_at_abi_19():
    from nflows_amd import _native as N
    import os
    lib = N.load()
    for name in ("nfa_diag_normal_log_prob_f32", "nfa_diag_normal_backward_f32", "nfa_mog_log_prob_f32", "nfa_mog_backward_f32",
                 "nfa_diag_normal_workspace_bytes", "nfa_mog_workspace_bytes"):
        assert hasattr(lib, name) and name in N.EXPORTS, name
    assert lib.nfa_abi_version() == N.ABI_VERSION == 19
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nflows_amd.h")) as f:
        assert "#define NFA_ABI_VERSION 19 " in f.read()
    # the workspace follows the plan: none in the rows regime or with one piece a row, [batch][pieces] float64 otherwise
    assert lib.nfa_diag_normal_workspace_bytes(517, 5) == 0 and lib.nfa_mog_workspace_bytes(2000, 2100) == 0
    assert lib.nfa_diag_normal_workspace_bytes(9, 4100) == 9 * 4 * 8 == lib.nfa_mog_workspace_bytes(9, 4100)
    # argument errors come back without touching a device
    assert lib.nfa_mog_log_prob_f32(None, None, None, None, None, 4, 3, 65, 0.01, None) == N.ERR_UNSUPPORTED
    assert lib.nfa_mog_log_prob_f32(None, None, None, None, None, 4, 3, 0, 0.01, None) == N.ERR_INVALID_ARGUMENT
    assert lib.nfa_diag_normal_log_prob_f32(None, None, None, None, None, None, 4, 8, 4, 0.0, None) == N.ERR_INVALID_ARGUMENT
    assert lib.nfa_diag_normal_log_prob_f32(None, None, None, None, None, None, 0, 8, 0, 0.0, None) == N.OK
    assert lib.nfa_mog_backward_f32(None, None, None, None, None, 0, 3, 5, 0.01, None) == N.OK
