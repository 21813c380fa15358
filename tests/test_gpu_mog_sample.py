"""K30 on the device (csrc/made_inverse.hip `made_inverse_kernel<element=mog>`, ops.made_mog_sample,
nn.nde.MixtureOfGaussiansMADE.sample): every case of tests/mog_sample_cases.py against the float64 truth and the fp32
yardstick with the components compared exactly, the real reference's fixture through the class, the selection rule on
inputs where it can be read off, and the class's own behaviour -- determinism under the seed, shapes, the switch."""
import copy

import numpy as np
import pytest
import torch

import mog_sample_cases as C
from nflows_amd import ops
from nflows_amd.distributions import MADEMoG
from nflows_amd.nn.nde import MixtureOfGaussiansMADE
from test_mog_sample_host import load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(made_dev, context, u, eps, block_cap="plan", want_components=True):
    D, H, K = made_dev.features, made_dev.hidden_features, made_dev.num_mixture_components
    if block_cap == "plan":
        block_cap = ops.made_mog_block_cap(D, H, len(ops._made_linears(made_dev)), len(ops.made_context_layers(made_dev)))
    schedule = ops.pack_mog_schedule(made_dev, block_cap=block_cap)
    assert schedule is not None
    terms = ops.made_mog_context_terms(context.to(DEV), ops.pack_made_context(made_dev))
    got = ops.made_mog_sample(u.to(DEV), eps.to(DEV), schedule, H, K, made_dev.epsilon, terms, want_components=want_components)
    assert got is not None
    return got, schedule


@pytest.mark.parametrize("name", list(C.CASES))
def test_parity_with_the_truth(name):
    r = C.reference(name)
    made = copy.deepcopy(r["made"]).to(DEV)
    (x, c), _ = _run(made, r["context"], r["u"], r["eps"])
    assert c.dtype == torch.int32 and np.array_equal(c.cpu().numpy(), r["components"]), "components differ from the truth's"
    C.assert_parity(x.cpu().numpy(), r["x32"], r["x64"], name)
    assert "element=mog, K=%d, context=1" % made.num_mixture_components in ops.last_layer_kernel()
    # without the diagnostic output: the same samples
    x_plain, _ = _run(made, r["context"], r["u"], r["eps"], want_components=False)
    assert torch.equal(x_plain, x)


def test_continuation_blocks_give_the_same_bits():
    """The plan's block cap against half of it: more continuation blocks, the same bits."""
    name = C.CONTINUATION_CASE
    r = C.reference(name)
    made = copy.deepcopy(r["made"]).to(DEV)
    D, H = made.features, made.hidden_features
    cap = ops.made_mog_block_cap(D, H, len(ops._made_linears(made)), len(ops.made_context_layers(made)))
    (x, c), plain = _run(made, r["context"], r["u"], r["eps"], block_cap=cap)
    at_cap = ops.last_layer_kernel()
    (x2, c2), cut = _run(made, r["context"], r["u"], r["eps"], block_cap=cap // 2 // 256 * 256)
    extra = cut[1].numel() - 2 - (D + 1)
    assert cut[1].numel() > plain[1].numel() and extra > 0 and cut[2][7] <= cap // 2
    assert "continuation_blocks=%d," % extra in ops.last_layer_kernel() and ops.last_layer_kernel() != at_cap
    assert torch.equal(x, x2) and torch.equal(c, c2)


def test_groups_of_eight_give_the_same_bits(monkeypatch):
    name = C.GROUP_CASE
    r = C.reference(name)
    made = copy.deepcopy(r["made"]).to(DEV)
    got = {}
    for group in ("0", "1"):
        monkeypatch.setenv("NFA_K23_GROUP", group)
        (got[group], _), _ = _run(made, r["context"], r["u"], r["eps"])
        assert "group=%s" % group in ops.last_layer_kernel()
    assert torch.equal(got["0"], got["1"])
    C.assert_parity(got["1"].cpu().numpy(), r["x32"], r["x64"], name + " grouped")


def test_fixture_through_the_class(golden_dir):
    """The real reference's trajectory: its components, its normal draws, and u in the middle of the chosen components'
    intervals, injected into the class's kernel path."""
    made, f = load_fixture(golden_dir)
    made = made.to(DEV)
    x = made._sample_kernel(f["context"].to(DEV), draws=(f["u"].to(DEV), f["eps"].to(DEV)))
    assert x is not None
    x64, _, _ = C.restated(copy.deepcopy(made).cpu().double(), f["context"], f["u"], f["eps"], components=f["components"])
    assert float(((x64 - f["samples64"]).abs() / (1.0 + f["samples64"].abs())).max()) <= 1e-12
    C.assert_parity(x.cpu().numpy(), f["samples"].numpy(), f["samples64"].numpy(), "fixture")
    # the components: through the op, on the same plan
    schedule, packed = made._sample_kernel_plan()
    terms = ops.made_mog_context_terms(f["context"].to(DEV), packed)
    x_op, c = ops.made_mog_sample(f["u"].to(DEV), f["eps"].to(DEV), schedule, 32, 5, made.epsilon, terms, want_components=True)
    assert torch.equal(x_op, x) and torch.equal(c.cpu().long(), f["components"])


def _flat_made(K, logit_bias, D=2):
    """Zero weights everywhere; the logits are `logit_bias`, the means the component's index, the stds softplus(0) + eps."""
    made = MixtureOfGaussiansMADE(features=D, hidden_features=16, context_features=1, num_blocks=2,
                                  num_mixture_components=K, epsilon=C.EPSILON, custom_initialization=False)
    with torch.no_grad():
        for p in made.parameters():
            p.zero_()
        bias = made.final_layer.bias.view(D, K, 3)
        bias[:, :, 0] = torch.as_tensor(logit_bias, dtype=torch.float32)
        bias[:, :, 1] = torch.arange(K, dtype=torch.float32)
    return made.eval().to(DEV)


def test_selection_rule_exactly():
    """Equal logits, K = 4: e_k = 1, S = 4, the running sums 1, 2, 3, 4, and u S exact for the u used.  The rule -- the
    smallest c whose running sum EXCEEDS u S -- gives c = k at u = k / 4 and c = k - 1 just below it; eps = 0: x == c."""
    made = _flat_made(4, [0.0] * 4)
    edges = np.array([0.0, 0.25, 0.5, 0.75], dtype=np.float32)
    below = np.nextafter(edges[1:], np.float32(0.0), dtype=np.float32)
    u = np.concatenate((edges, below))
    want = np.array([0, 1, 2, 3, 0, 1, 2])
    uu = torch.from_numpy(np.stack((u, u[::-1].copy()), axis=1))
    (x, c), _ = _run(made, torch.zeros(len(u), 1), uu, torch.zeros(len(u), 2))
    assert np.array_equal(c.cpu().numpy(), np.stack((want, want[::-1]), axis=1))
    assert torch.equal(x.cpu(), c.cpu().float())
    # the largest float below 1 with uneven logits: a valid component (by the rule: the last one), a finite x
    uneven = _flat_made(5, [3.0, -2.0, 0.5, 1.0, -30.0])
    top = torch.full((3, 2), float(np.nextafter(np.float32(1.0), np.float32(0.0))))
    (x, c), _ = _run(uneven, torch.zeros(3, 1), top, torch.ones(3, 2))
    assert torch.isfinite(x).all() and int(c.min()) >= 0 and int(c.max()) <= 4
    x64, c64, _ = C.restated(copy.deepcopy(uneven).cpu().double(), torch.zeros(3, 1), top, torch.ones(3, 2))
    assert torch.equal(c.cpu().long(), c64)


def _class_made(name="d7_k5_h32_res_c8_b17"):
    return copy.deepcopy(C.reference(name)["made"]).to(DEV)


def test_class_is_deterministic_under_the_seed_and_equals_the_op():
    made = _class_made()
    context = C.reference("d7_k5_h32_res_c8_b17")["context"][:5].to(DEV)
    torch.manual_seed(123)
    a = made.sample(3, context=context)
    label = ops.last_layer_kernel()
    torch.manual_seed(123)
    b = made.sample(3, context=context)
    assert a.shape == (5, 3, 7) and torch.equal(a, b) and "element=mog" in label
    # the same two draws, in the documented order, through the op
    torch.manual_seed(123)
    u = torch.rand(15, 7, device=DEV)
    z = torch.randn(15, 7, device=DEV)
    rep = context.repeat_interleave(3, dim=0)
    (x, _), _ = _run(made, rep, u, z)
    assert torch.equal(a, x.reshape(5, 3, 7))


def test_sample_and_log_prob_of_the_distribution():
    torch.manual_seed(9)
    dist = MADEMoG(features=4, hidden_features=32, context_features=3, num_blocks=2, num_mixture_components=5).to(DEV).eval()
    context = torch.randn(6, 3, device=DEV)
    with torch.no_grad():
        samples, log_prob = dist.sample_and_log_prob(8, context=context)
        assert "element=mog, K=5" in ops.last_layer_kernel()
        assert samples.shape == (6, 8, 4) and log_prob.shape == (6, 8)
        assert torch.isfinite(samples).all() and torch.isfinite(log_prob).all()
        again = dist.log_prob(samples.reshape(48, 4), context=context.repeat_interleave(8, dim=0)).reshape(6, 8)
    assert torch.allclose(log_prob, again, rtol=1e-6, atol=1e-6)


def test_component_frequencies():
    """Zero weights, logit biases (0, log 3): mixture weights (0.25, 0.75) for every feature, means 0 and 1, eps-sized
    stds.  4 096 samples x 2 features: the share of component 0 lies within 0.035 of 0.25 -- 5 standard deviations of the
    binomial at n = 4 096 (sqrt(0.1875 / 4096) = 0.0068) -- and the run is deterministic under the seed."""
    made = _flat_made(2, [0.0, float(np.log(3.0))])
    with torch.no_grad():
        made.final_layer.bias.view(2, 2, 3)[:, :, 2] = -20.0      # std = softplus(-20) + 0.01: the components stay apart
    torch.manual_seed(2024)
    x = made.sample(4096, context=torch.zeros(1, 1, device=DEV))
    assert x.shape == (1, 4096, 2) and "element=mog" in ops.last_layer_kernel()
    first = (x[0] < 0.5).float().mean(dim=0).cpu().numpy()
    print("share of component 0 per feature:", first)
    assert np.all(np.abs(first - 0.25) <= 0.035)


def test_switch_gives_the_host_loop(monkeypatch):
    made = _class_made()
    context = C.reference("d7_k5_h32_res_c8_b17")["context"][:4].to(DEV)
    torch.manual_seed(1)
    made.sample(2, context=context)
    assert "element=mog" in ops.last_layer_kernel()
    before = ops.last_layer_kernel()
    monkeypatch.setattr(ops, "made_mog_sample", lambda *a, **k: pytest.fail("the kernel path with the switch off"))
    monkeypatch.setattr(MixtureOfGaussiansMADE, "_use_sample_kernel", False)
    torch.manual_seed(1)
    x = made.sample(2, context=context)
    assert x.shape == (4, 2, 7) and torch.isfinite(x).all() and x.is_cuda
    assert ops.last_layer_kernel() == before
