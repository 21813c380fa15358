"""Host side of K32's exact-logit suite and K33's bit-for-bit suite (tests/wide_exact_cases.py; no GPU).

  * Every conditioner those suites use is built and passes exact_logits' exactness checks (operand bits, the 2^24 q budget
    of every output, the bf16 piece count of every product), forward and backward.
  * Stock torch on the CPU in float32 AND float64 -- forward, and autograd for every gradient -- equals exact_forward /
    exact_backward as numbers: this is what validates the host code the device suites take as the truth.
  * Folded scale (widths 129, 160, 192): every stored width / height entry of the final layer comes back from the packer's
    own expression, (w.double() * (1.0 / math.sqrt(H))).float(), as its dyadic target.
  * Caps: for every K32 case the ORACLE'S OWN fp32 result passes the check function the kernel's result goes through
    (rows_ok >= 0.95, bulk 0.995, the 99.9 % element share are conditions on the inputs: the reference alone must stay
    inside them), and the reference's 99.9 % quantile covers its own maximum at the rule's factor of 4
    (wide_exact_cases.reference_tail_covered: a condition on the inputs as well)."""
import math

import numpy as np
import pytest
import torch

import exact_logits as X
import wide_exact_cases as W


@pytest.mark.parametrize("name", [c[0] for c in W.K32_CASES])
def test_k32_case_conditioner_and_caps(name):
    _, hidden, D, K, more = W.K32_BY_NAME[name]
    case = W.k32_case(name)     # (builds the conditioner and runs the exactness checks)
    assert case["D"] == D and len(case["ti"]) == D // 2
    net = case["flow"]._transform._transforms[-1].transform_net
    assert net.hidden_features == hidden and len(net.blocks) == more.get("num_blocks", 2)
    P = X.params_per_feature(K, "linear")
    if case["fold"]:
        w = net.final_layer.weight.detach().view(-1, P, hidden)[:, :2 * K]
        b = net.final_layer.bias.detach().view(-1, P)[:, :2 * K]
        for stored in (w, b):
            packed = (stored.double() * (1.0 / math.sqrt(hidden))).float().double().numpy()     # the pack's expression
            assert np.array_equal(packed, X.pack_scaled(stored.numpy(), hidden))
            # a dyadic target with few bits: k / 64 (weights), k / 16 and the regimes' 1.5, +-90 (biases)
            assert np.array_equal(packed * 64, np.round(packed * 64)) and np.abs(packed).max() <= 96
            assert int(X.significant_bits(packed).max()) <= 10
    # stock torch on the conditioner, float32 and float64, against the exact logits (the final layer K32 holds)
    for direction, inverse in (("fwd", False), ("inv", True)):
        full, _, raw, _, _ = case[direction]
        ident = torch.from_numpy(full[:, case["ii"]])
        for dtype in (torch.float32, torch.float64):
            with torch.no_grad():
                got = net.to(dtype)(ident.to(dtype)).double().numpy().reshape(raw.shape)
            net.float()
            if case["fold"]:    # (stock torch holds the unscaled rows: the derivative logits are the comparable ones)
                got, want = got[..., 2 * K:], raw[..., 2 * K:]
            else:
                want = raw
            assert np.array_equal(got, want), (name, direction, dtype)
    W.check_k32(name, case, K, W.oracle_result(case))
    covered, figures = W.reference_tail_covered(case)
    assert covered, "%s: the reference's own third-worst row sits beneath a cliff of its error tail: %r" % (name, figures)


@pytest.mark.parametrize("name", [c[0] for c in W.K32_CASES if not c[4].get("variant") == "two_layer"])
def test_k32_scaled_final_layer_in_torch(name):
    """the final layer K32 holds (`scaled_final`), applied by stock torch to the exact hidden values: the scaled logits"""
    net, ident, K, fold = W.k32_conditioner(name)
    f = X.exact_forward(net, ident, final=X.scaled_final(net, K, "linear") if fold else None)
    wf, bf = X.scaled_final(net, K, "linear") if fold else (net.final_layer.weight.detach().double().numpy(),
                                                            net.final_layer.bias.detach().double().numpy())
    for dtype in (torch.float32, torch.float64):
        got = torch.nn.functional.linear(torch.from_numpy(f["hidden"]).to(dtype), torch.from_numpy(wf).to(dtype),
                                         torch.from_numpy(bf).to(dtype))
        assert np.array_equal(got.double().numpy(), f["params"]), (name, dtype)


@pytest.mark.parametrize("shape", W.K33_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_k33_shape_exact_values_are_stock_torch(shape):
    di, H, nb, out, rows, recipe = shape
    rows = 64 * 3 if rows == W.CUS else rows        # (the device test's row count depends on the CU count)
    net, x, g, forward, backward = W.k33_problem(di, H, nb, out, rows, recipe)
    want = {k: forward[k] for k in ("hidden", "saved", "params")}
    want.update({k: backward[k] for k in ("g_hidden", "grads", "g_x")})
    for dtype in (torch.float32, torch.float64):
        W.assert_equal_as_numbers(W.torch_chain(net, x, g, dtype, with_final=bool(out)), want, "%s %s" % (shape, dtype))
    if recipe == "long":    # the recipe's point: factors with all three bf16 pieces in use, forward and backward
        assert 20 <= int(X.significant_bits(net.initial_layer.weight.detach().double().numpy()).max()) <= 22
        assert 20 <= int(X.significant_bits(forward["hidden"]).max()) <= 22
        assert int(X.significant_bits(backward["g_x"]).max()) >= 17


@pytest.mark.parametrize("H", W.CLASS_WIDTHS)
def test_class_path_parameter_gradients_are_stock_torch(H):
    net, x, g, forward, backward = W.class_problem(H)
    assert set(backward["param_grads"]) == set(dict(net.named_parameters()))
    for dtype in (torch.float32, torch.float64):
        got = W.torch_chain(net, x, g, dtype)
        W.assert_equal_as_numbers(got["param_grads"], backward["param_grads"], "H=%d %s" % (H, dtype))
        W.assert_equal_as_numbers(got["g_x"], backward["g_x"], "H=%d %s g_x" % (H, dtype))


@pytest.mark.parametrize("H", [129, 160, 192, 256])
def test_folded_scale_round_trip(H):
    """over v = k / 8, |k| <= 64: the pool of targets the packer's expression returns exactly is ample at every width, and
    at 256 (a power-of-two scale) it is all of them"""
    v = np.arange(-64, 65) / 8.0
    stored, ok = X.fold_store(v, H)
    torch_way = (torch.from_numpy(stored).float().double() * (1.0 / math.sqrt(H))).float().double().numpy()
    assert np.array_equal(torch_way == v, ok)
    assert ok.sum() >= 96 and (H != 256 or ok.all()), int(ok.sum())
    assert np.array_equal(torch_way[ok], v[ok])
