"""CPU-only checks of K31's host side: the final rows of `ops.pack_made_mog_conditioner` unpacked by the inverse of its
order, and the decisions of `MixtureOfGaussiansMADE`'s gate that need no device."""
import pytest
import torch

import mog_density_cases as C
from nflows_amd import _native as N
from nflows_amd import ops
from nflows_amd.nn.nde import MixtureOfGaussiansMADE


@pytest.mark.parametrize("name", ["d5_k5_c3", "d64_k11_c64_b1", "d6_k10_c3_h64_ff"])
def test_final_rows_unpack_to_the_masked_final_layer(name):
    made = C.build(name)
    D, K, ce, H, blocks, residual = C.CASES[name][:6]
    weights, biases, epsilon = ops.pack_made_mog_conditioner(made)
    T, pairs = ops.made_mog_tiles(K), (D + 1) // 2
    tiles, linears, cks = pairs * T, blocks * (2 if residual else 1), (ce + 15) // 16
    assert epsilon == C.EPSILON and T == (3 * K + 15) // 16
    assert weights.shape == ((4 if D > 32 else 2) + 8 * linears + cks * (1 + (blocks if residual else 0)) + 2 * tiles, 768 * 8)
    assert biases.numel() == 128 * (2 + linears) + 32 * tiles
    # (tile, hs, piece, k4, hf, i, j): the three bf16 pieces summed, rows (tile, i), columns (hs, k4, hf, j)
    w = weights[-2 * tiles:].view(tiles, 2, 3, 4, 2, 32, 8).double().sum(dim=2).permute(0, 4, 1, 2, 3, 5).reshape(tiles * 32, 128)
    b = biases[-32 * tiles:].double().view(tiles, 2, 4, 4).permute(0, 2, 1, 3).reshape(-1)      # accumulator order undone
    order_r = ops._k8_row_order_32(2 * pairs, T)
    rows = torch.zeros(2 * pairs * 16 * T, 128, dtype=torch.float64)
    bias = torch.zeros(2 * pairs * 16 * T, dtype=torch.float64)
    rows[order_r] = w.new_zeros(w.shape).index_copy_(1, ops._k8_column_order(), w)
    bias[order_r] = b
    rows, bias = rows.view(2 * pairs, 16 * T, 128), bias.view(2 * pairs, 16 * T)
    final = made.final_layer
    want = (final.weight.detach() * final.mask).double().view(D, 3 * K, H)
    # three bf16 pieces keep 24 bits of a weight; the bias is fp32 as it is
    assert (rows[:D, :3 * K, :H] - want).abs().le(2.0 ** -23 * want.abs()).all()
    assert torch.equal(bias[:D, :3 * K], final.bias.detach().double().view(D, 3 * K))
    assert not rows[:D, 3 * K:].any() and not rows[D:].any() and not rows[:, :, H:].any()
    assert not bias[:D, 3 * K:].any() and not bias[D:].any()


def test_gate_decisions_without_a_device(monkeypatch):
    assert "nfa_made_mog_log_prob_f32" in N.EXPORTS
    kw = dict(features=6, hidden_features=32, context_features=3, num_blocks=2)
    assert MixtureOfGaussiansMADE(num_mixture_components=16, **kw)._density_kernel_net()
    assert MixtureOfGaussiansMADE(num_mixture_components=5, use_residual_blocks=False, random_mask=True, **kw)._density_kernel_net()
    out = [MixtureOfGaussiansMADE(num_mixture_components=17, **kw),
           MixtureOfGaussiansMADE(use_batch_norm=True, **kw),
           MixtureOfGaussiansMADE(activation=torch.tanh, **kw),
           MixtureOfGaussiansMADE(dropout_probability=0.5, **kw).train(),
           MixtureOfGaussiansMADE(**kw).double(),
           MixtureOfGaussiansMADE(**dict(kw, hidden_features=129)),
           MixtureOfGaussiansMADE(**dict(kw, features=65)),
           MixtureOfGaussiansMADE(**dict(kw, context_features=65))]
    assert not any(m._density_kernel_net() for m in out)
    assert MixtureOfGaussiansMADE(dropout_probability=0.5, **kw).eval()._density_kernel_net()
    # the call's side, on a CPU module: never K31 (and the op must not be reached)
    made = MixtureOfGaussiansMADE(**kw).eval()
    x, ctx = torch.randn(128, 6), torch.randn(128, 3)
    monkeypatch.setattr(ops, "made_mog_log_prob", lambda *a, **k: pytest.fail("the kernel path on the CPU"))
    assert not made._density_kernel_serves(x, ctx)
    with torch.no_grad():
        assert made.log_prob(x, context=ctx).shape == (128,)
    # what the gate reads of a call, with the device tests stubbed out: tensors that claim to be on the module's device
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with torch.no_grad():
        assert made._density_kernel_serves(x, ctx)
        assert not made._density_kernel_serves(x[:127], ctx[:127])          # fewer rows than one block
        assert not made._density_kernel_serves(x, None) and not made._density_kernel_serves(x, ctx[:, :2])
        assert not made._density_kernel_serves(x.double(), ctx)
        for switch in ("_use_density_kernel", "_use_kernel"):
            monkeypatch.setattr(MixtureOfGaussiansMADE, switch, False)
            assert not made._density_kernel_serves(x, ctx)
            monkeypatch.setattr(MixtureOfGaussiansMADE, switch, True)
        # the size rule (features >, components >, rows <): 64 features with 10 components below 16 384 rows
        big = MixtureOfGaussiansMADE(**dict(kw, features=44, num_mixture_components=6)).eval()
        x44 = torch.randn(16384, 44)
        assert big._density_kernel_serves(x44, x44[:, :3]) and not big._density_kernel_serves(x44[:16383], x44[:16383, :3])
        for edge in (dict(features=43, num_mixture_components=6), dict(features=44, num_mixture_components=5)):
            at = MixtureOfGaussiansMADE(**dict(kw, **edge)).eval()
            assert at._density_kernel_serves(x44[:128, :edge["features"]], x44[:128, :3])
    assert not made._density_kernel_serves(x, ctx)                              # parameters that require a gradient
    assert not made._density_kernel_serves(x.clone().requires_grad_(True), ctx)
