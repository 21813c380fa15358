"""K25's host side on the CPU: the packed streams of a MADE's masked weights, the gate of `MADE._fusable`, and the
wiring of autograd.MadeNet with the kernels replaced by tensor-operation emulations of their contracts (as
tests/test_host_logic.py::test_training_function_wiring_with_emulated_kernels does for ResidualNetHidden)."""
import contextlib
import copy

import pytest
import torch

import maf_cases
import maf_train_cases as cases


def _decode_kmajor(stages, order_k):
    """[8, 6144] split-bf16 stages -> the [128, 128] matrix whose three pieces they hold (sum of the pieces)"""
    p = stages.view(8, 4, 3, 2, 32, 8).float().sum(dim=2)          # (ks, tile, hf, i, j)
    m = p.permute(1, 3, 0, 2, 4).reshape(128, 128)                  # rows 32 tile + i, columns (ks, hf, j)
    out = torch.empty_like(m)
    out[:, order_k] = m
    return out


def _decode_tilemajor(stages, tiles, order_k):
    m = stages.view(tiles, 2, 3, 4, 2, 32, 8).float().sum(dim=2).permute(0, 4, 1, 2, 3, 5).reshape(tiles * 32, 128)
    out = torch.empty_like(m)
    out[:, order_k] = m
    return out


@pytest.mark.parametrize("features,blocks,hidden", [(8, 2, 32), (36, 2, 128), (64, 1, 128), (4, 1, 4)])
def test_streams_of_the_masked_products_decode_to_the_masked_weights(features, blocks, hidden):
    """`pack_resnet_hidden_train_reference` of `mask * weight` (what the masked packer launch has to equal bit for bit)
    holds the masked weights: every stage group decodes to mask * W within the three pieces' precision, and a
    masked-out position contributes zero pieces."""
    from nflows_amd import ops
    net = cases.made(features, hidden, blocks, multiplier=2, seed=features)
    with torch.no_grad():
        for b in net.blocks:
            b.linear_layers[1].weight.mul_(maf_cases.SHARPEN["scale_linear1"])

    def product(lin):
        return (lin.mask * lin.weight).detach()

    block_params = [(product(b.linear_layers[0]), b.linear_layers[0].bias, product(b.linear_layers[1]), b.linear_layers[1].bias)
                    for b in net.blocks]
    fwd, bias, bwd, fbias = ops.pack_resnet_hidden_train_reference(
        product(net.initial_layer), net.initial_layer.bias, block_params, (product(net.final_layer), net.final_layer.bias))
    order_k = ops._k8_column_order()
    init_ks = 4 if features > 32 else 2
    H, out = hidden, 2 * features

    def check(decoded, lin, transposed=False):
        want, mask = product(lin), lin.mask
        if transposed:
            want, mask = want.t(), mask.t()
        r, c = want.shape
        assert torch.allclose(decoded[:r, :c], want, rtol=0, atol=1e-7 * float(want.abs().max()) + 1e-9)
        assert not decoded[:r, :c][mask == 0].any(), "a masked-out weight left a non-zero piece"
        assert (mask == 0).any() and not decoded[r:].any() and not decoded[:, c:].any()

    at = init_ks
    for b in net.blocks:
        for lin in b.linear_layers:
            check(_decode_kmajor(fwd[at:at + 8], order_k), lin)
            at += 8
    ft = (out + 31) // 32
    check(_decode_tilemajor(fwd[at:], ft, order_k), net.final_layer)
    at = 0
    for b in reversed(net.blocks):
        for lin in (b.linear_layers[1], b.linear_layers[0]):
            check(_decode_kmajor(bwd[at:at + 8], order_k), lin, transposed=True)
            at += 8
    tiles = (features + 31) // 32
    check(_decode_tilemajor(bwd[at:at + 2 * tiles], tiles, order_k), net.initial_layer, transposed=True)
    # the initial layer, k-major over the input features in natural order: k = 16 ks + 8 hf + j
    first = fwd[:init_ks].view(init_ks, 4, 3, 2, 32, 8).float().sum(dim=2).permute(1, 3, 0, 2, 4).reshape(128, 16 * init_ks)
    assert torch.allclose(first[:H, :features], product(net.initial_layer), rtol=0, atol=1e-8)
    assert not first[:H, :features][net.initial_layer.mask == 0].any() and not first[H:].any()
    assert not first[:, features:].any()


def test_gate_accepts_the_fused_shapes_and_refuses_everything_else():
    for features, hidden, blocks, rows in cases.ACCEPTED:
        net = cases.made(features, hidden, blocks)
        assert net._fusable(rows, features), (features, hidden, blocks, rows)
        net.fuse_training = False
        assert not net._fusable(rows, features)
    for name, (net, rows, context, scope) in cases.refused().items():
        features = net.initial_layer.in_features
        with (torch.autocast("cpu", dtype=torch.bfloat16) if scope == "autocast" else contextlib.nullcontext()):
            assert not net._fusable(rows, features, context), name
        # ... and the CPU tensors of this test never take the fused path, whatever the net
        x = torch.randn(rows, features, requires_grad=True)
        assert not net._fused_training(x, context), name
        assert net(x, context).shape == (rows, net.final_layer.out_features)
    # the refusals are the named property's doing: the same nets without it are accepted
    assert cases.made()._fusable(256, 8) and not cases.made()._fusable(256, 9)
    dropped = cases.made(dropout_probability=0.2)
    assert not dropped._fusable(256, 8) and dropped.eval()._fusable(256, 8)
    assert not cases.made(use_batch_norm=True)._fusable(256, 8)
    assert not cases.made(activation=torch.tanh)._fusable(256, 8)


def test_switch_reads_the_environment():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("0", "False"), (None, "True")):
        env = {k: v for k, v in os.environ.items() if k != "NFA_K25"}
        if value is not None:
            env["NFA_K25"] = value
        got = subprocess.check_output([sys.executable, "-c", "from nflows_amd.transforms.made import MADE; print(MADE.fuse_training)"],
                                      env=env, cwd=root).decode().strip()
        assert got == want, (value, got)


def test_made_function_wiring_with_emulated_kernels(monkeypatch):
    """autograd.MadeNet with the packer, K14's two kernels and K10 replaced by float64 tensor operations that do what
    include/nflows_amd.h says each does: output and every gradient equal autograd through the eager masked Linears --
    the order of the gradients, the masks on the weight gradients (exact zeros), hidden widths below 128, feature counts
    and output widths that are no multiples of four, frozen parameters."""
    from nflows_amd import autograd as AG
    from nflows_amd import ops
    book = {}

    def pad2(w, rows, cols):
        out = w.new_zeros(rows, cols)
        out[:w.shape[0], :w.shape[1]] = w
        return out

    def pad1(b, n):
        return torch.cat((b, b.new_zeros(n - b.shape[0])))

    def pack(w_in, b_in, blocks, final, masks):   # nfa_pack_made_train_f32: mask * weight, padded to the kernels' sizes
        assert len(masks) == 2 + 2 * len(blocks)
        di, out4 = (w_in.shape[1] + 3) // 4 * 4, (final[0].shape[0] + 3) // 4 * 4
        key = float(len(book))
        ms = list(masks)
        book[key] = dict(w_in=pad2((w_in * ms[0]).detach(), 128, di), b_in=pad1(b_in.detach(), 128),
                         blocks=[(pad2((w0 * ms[1 + 2 * k]).detach(), 128, 128), pad1(b0.detach(), 128),
                                  pad2((w1 * ms[2 + 2 * k]).detach(), 128, 128), pad1(b1.detach(), 128))
                                 for k, (w0, b0, w1, b1) in enumerate(blocks)],
                         final=(pad2((final[0] * ms[-1]).detach(), out4, 128), pad1(final[1].detach(), out4)))
        tag = torch.tensor([key], dtype=torch.float64)
        return tag, tag, tag, tag

    def forward(x, fwd_w, fwd_b, num_blocks, final_bias=None, out_features=0):
        assert x.shape[1] % 4 == 0 and x.shape[0] % 128 == 0 and out_features % 4 == 0 and final_bias is not None
        w = book[fwd_w.item()]
        h = x @ w["w_in"].t() + w["b_in"]
        saved = []
        for w0, b0, w1, b1 in w["blocks"]:
            t = torch.relu(h)
            u = torch.relu(t @ w0.t() + b0)
            saved += [t, u]
            h = h + u @ w1.t() + b1
        params = h @ w["final"][0].t() + w["final"][1]
        assert params.shape[1] == out_features
        return h, (torch.stack(saved) if saved else x.new_zeros(0, x.shape[0], 128)), params

    def backward_from_params(grad_params, bwd_w, saved, num_identity):   # nfa_resnet_backward_f32
        w = book[bwd_w.item()]
        assert grad_params.shape[1] % 4 == 0
        gh = g_hidden = grad_params @ w["final"][0]
        nb = saved.shape[0] // 2
        grads = [None] * (2 * nb)
        for k in reversed(range(nb)):
            w0, b0, w1, b1 = w["blocks"][k]
            ga = (gh @ w1) * (saved[2 * k + 1] > 0)
            gh = gh + (ga @ w0) * (saved[2 * k] > 0)
            grads[2 * k + 1], grads[2 * k] = ga, gh
        gx = gh @ w["w_in"]
        assert gx.shape[1] == num_identity and num_identity % 4 == 0
        return gx, (torch.stack(grads) if grads else grad_params.new_zeros(0, grad_params.shape[0], 128)), g_hidden

    monkeypatch.setattr(ops, "pack_made_train", pack)
    monkeypatch.setattr(ops, "resnet_hidden_forward", forward)
    monkeypatch.setattr(ops, "resnet_backward", backward_from_params)
    monkeypatch.setattr(ops, "linear_wgrad", lambda x, gy, need_bias=True: (gy.t() @ x, gy.sum(0) if need_bias else None))
    monkeypatch.setattr(ops, "linear_wgrad_batched", lambda problems, need_bias=True: [
        (gy.t() @ x, gy.sum(0) if need_bias else None) for x, gy in problems])
    seen_masked_out = 0
    for features, hidden, blocks, mult, frozen in ((8, 32, 2, 2, ()), (36, 128, 3, 2, ()), (63, 128, 1, 2, ()), (2, 4, 2, 2, ()),
                                                   (7, 52, 2, 3, ()), (12, 128, 0, 23, ()),
                                                   (8, 64, 1, 2, ("initial_layer.weight", "blocks.0.linear_layers.1.bias",
                                                                  "final_layer.weight"))):
        net = cases.made(features, hidden, blocks, multiplier=mult, seed=features).double()
        with torch.no_grad():
            for b in net.blocks:
                b.linear_layers[1].weight.mul_(50.0)
        for name, p in net.named_parameters():
            p.requires_grad_(name not in frozen)
        x = torch.randn(256, features, dtype=torch.float64, requires_grad=True)
        weight = torch.randn(256, features * mult, dtype=torch.float64)
        ref_net, ref_x = copy.deepcopy(net), x.detach().clone().requires_grad_(True)
        want = maf_cases.made_forward(ref_net, ref_x)
        (want * weight).sum().backward()
        masks, params = [net.initial_layer.mask], [net.initial_layer.weight, net.initial_layer.bias]
        for b in net.blocks:
            for lin in b.linear_layers:
                masks.append(lin.mask)
                params += [lin.weight, lin.bias]
        masks.append(net.final_layer.mask)
        result = AG.MadeNet.apply(x, tuple(masks), *params, net.final_layer.weight, net.final_layer.bias)
        assert result.shape == weight.shape and torch.allclose(result, want, rtol=1e-10, atol=1e-12)
        (result * weight).sum().backward()
        assert torch.allclose(x.grad, ref_x.grad, rtol=1e-10, atol=1e-12)
        for (name, p), (_, q) in zip(net.named_parameters(), ref_net.named_parameters()):
            if name in frozen:
                assert p.grad is None, name
                continue
            assert p.grad.shape == p.shape and torch.allclose(p.grad, q.grad, rtol=1e-10, atol=1e-12), name
            if name.endswith("weight"):
                mask = dict(net.named_buffers())[name[:-len("weight")] + "mask"]
                assert not p.grad[mask == 0].any(), name   # (exact zeros)
                seen_masked_out += int((mask == 0).sum())
    assert seen_masked_out > 10000


def test_gradient_fixture_rebuilds_and_its_fp32_side_meets_the_rule(golden_dir):
    """tests/golden/maf_grads*.npz: the drop-in flows rebuilt from their seeds carry the reference's weights (checksums),
    every gradient is there in both precisions, and the reference's own fp32 gradients pass `close_to_truth` against its
    float64 ones (by construction: the rule the GPU test applies to the kernels)."""
    from helpers import close_to_truth
    table = cases.load_grads(golden_dir)
    assert [str(c) for c in table["cases"]] == list(cases.GRAD_CASES)
    for name in cases.GRAD_CASES:
        flow = cases.build_grad_flow(name, table)
        wanted = {"x"} | {n for n, _ in flow.named_parameters()}
        assert wanted == {k.split("/g32/")[1] for k in table if k.startswith(name + "/g32/")}
        for k in wanted:
            g32, g64 = table["%s/g32/%s" % (name, k)], table["%s/g64/%s" % (name, k)]
            assert g32.dtype == "float32" and g64.dtype == "float64" and g32.shape == g64.shape
            close_to_truth(torch.from_numpy(g32), g32, g64, "%s %s" % (name, k))
        x, _ = maf_cases.fixture_inputs(name)
        assert tuple(table[name + "/g64/x"].shape) == tuple(x.shape)
