"""K25 on the device: MAF layers under autograd on HIP kernels -- the masked packer launch
(nfa_pack_made_train_f32), the backward kernel of the affine autoregressive element
(nfa_affine_autoregressive_backward_f32), one layer and whole flows through autograd.MadeNet (K14 + K10) against
float64, the fallbacks, training and graph capture.  Run with `-m gpu`.

Rules.  Gradients of whole flows against the REAL reference's autograd (tests/golden/maf_grads*.npz):
helpers.close_to_truth -- at most 4 x the reference-fp32's own error against its float64 + 2e-5 of the scale.  One
layer against a float64 restatement: at most 4 x the switched-off (eager) path's own error + 1e-6 of the scale, the rule
of test_gpu_grads.py::test_fused_conditioner_training_kernels."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import maf_cases
import maf_train_cases as cases
from helpers import close_to_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def k25(enabled):
    from nflows_amd.transforms.made import MADE
    saved = MADE.fuse_training
    MADE.fuse_training = enabled
    try:
        yield
    finally:
        MADE.fuse_training = saved


@pytest.fixture
def k14_calls(monkeypatch):
    """the list grows by one per `ops.resnet_hidden_forward` call (K14's forward kernel)"""
    from nflows_amd import ops
    calls = []
    real = ops.resnet_hidden_forward
    monkeypatch.setattr(ops, "resnet_hidden_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def sharpened(net):
    """the blocks' second Linears moved off their +-1e-3 initialisation and the output layer scaled (maf_cases.SHARPEN)"""
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "final_layer" in name:
                p.mul_(maf_cases.SHARPEN["scale_final"])
            elif "linear_layers.1" in name:
                p.mul_(maf_cases.SHARPEN["scale_linear1"])
    return net


def assert_within_eager(names, got, eager, truth):
    for name, a, b, t in zip(names, got, eager, truth):
        assert a.shape == t.shape, name
        scale = 1.0 + t.abs().max().item()
        e_a, e_b = (a.double() - t).abs().max().item(), (b.double() - t).abs().max().item()
        print("%-44s fused %.3e eager %.3e scale %.2e" % (name, e_a, e_b, scale))
        assert e_a <= 4 * e_b + 1e-6 * scale, "%s: fused %.3e, eager %.3e, scale %.2e" % (name, e_a, e_b, scale)


# ---- 1. the packer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("features,blocks,hidden", [(8, 2, 32), (36, 2, 128), (63, 1, 128), (2, 1, 4)])
def test_masked_packer_launch_matches_the_tensor_reference_on_the_products(features, blocks, hidden):
    """nfa_pack_made_train_f32 writes the bytes of `pack_resnet_hidden_train_reference` called on the products
    `mask * weight` (zero-padded to the kernels' multiples of four where the MADE's sizes are odd), with the final
    Linear and without it; the unmasked entry's hidden-only call on the products agrees with the same prefix."""
    from nflows_amd import ops
    net = sharpened(cases.made(features, hidden, blocks, multiplier=2, seed=features)).to(DEV)
    lins = [net.initial_layer] + [l for b in net.blocks for l in b.linear_layers] + [net.final_layer]
    prod = [(l.mask * l.weight).detach() for l in lins]
    di, out = (features + 3) // 4 * 4, (2 * features + 3) // 4 * 4
    block_params = [(b.linear_layers[0].weight, b.linear_layers[0].bias, b.linear_layers[1].weight, b.linear_layers[1].bias)
                    for b in net.blocks]
    prod_blocks = [(prod[1 + 2 * k], b.linear_layers[0].bias, prod[2 + 2 * k], b.linear_layers[1].bias)
                   for k, b in enumerate(net.blocks)]
    w_in = torch.nn.functional.pad(prod[0], (0, di - features))
    w_f = torch.nn.functional.pad(prod[-1], (0, 0, 0, out - 2 * features))
    b_f = torch.nn.functional.pad(net.final_layer.bias.detach(), (0, out - 2 * features))
    got = ops.pack_made_train(net.initial_layer.weight, net.initial_layer.bias, block_params,
                              (net.final_layer.weight, net.final_layer.bias), [l.mask for l in lins])
    ref = ops.pack_resnet_hidden_train_reference(w_in, net.initial_layer.bias, prod_blocks, (w_f, b_f))
    for q in (0, 2):
        assert got[q].shape == ref[q].shape and torch.equal(got[q].view(torch.int16), ref[q].view(torch.int16)), q
    assert torch.equal(got[1], ref[1]) and torch.equal(got[3], ref[3])
    assert (prod[-1] == 0).any() and got[0].view(torch.int16).ne(0).any()
    # the masked launch without the final Linear (out_features = 0, 1 + 2 nb masks, no W_f^T stages behind W_in^T's)
    ref_h = ops.pack_resnet_hidden_train_reference(w_in, net.initial_layer.bias, prod_blocks, None)
    masked_h = ops.pack_made_train(net.initial_layer.weight, net.initial_layer.bias, block_params, None,
                                   [l.mask for l in lins[:-1]])
    for q in (0, 2):
        assert masked_h[q].shape == ref_h[q].shape and torch.equal(masked_h[q].view(torch.int16), ref_h[q].view(torch.int16)), q
    assert torch.equal(masked_h[1], ref_h[1]) and masked_h[3] is None and ref_h[3] is None
    with pytest.raises(ValueError):   # (one mask per weight: the final Linear's is one too many here)
        ops.pack_made_train(net.initial_layer.weight, net.initial_layer.bias, block_params, None, [l.mask for l in lins])
    # ... and the unmasked entry on the products (the hidden-only form) is the same prefix
    hid = ops.pack_resnet_hidden_train(w_in, net.initial_layer.bias, prod_blocks, None)
    n_h = ref_h[0].shape[0]
    assert torch.equal(hid[0].view(torch.int16), ref_h[0].view(torch.int16)) and torch.equal(hid[2].view(torch.int16), ref_h[2].view(torch.int16))
    assert torch.equal(got[0][:n_h].view(torch.int16), ref_h[0].view(torch.int16)) and hid[3] is None
    # no masks at all through the new entry: the bytes of the existing one
    plain = ops.pack_made_train(w_in, net.initial_layer.bias, prod_blocks, (w_f, b_f), [None] * len(lins))
    old = ops.pack_resnet_hidden_train(w_in, net.initial_layer.bias, prod_blocks, (w_f, b_f))
    for q in (0, 2):
        assert torch.equal(plain[q].view(torch.int16), old[q].view(torch.int16)) and torch.equal(plain[q].view(torch.int16), ref[q].view(torch.int16))
    assert torch.equal(plain[1], old[1]) and torch.equal(plain[3], old[3])


# ---- 2. the element's backward kernel --------------------------------------------------------------------------------------

@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("B,D", [(1, 1), (3, 5), (128, 7), (257, 64)])
def test_affine_autoregressive_backward_kernel(B, D, inverse, monkeypatch):
    """Both directions, each incoming gradient missing in turn, against float64 autograd of the layer under the CPU
    test's rule (per element: 4 x the float32 evaluation's error + 2e-5 (1 + max |truth|)); repeated launches are
    bit-identical.  1 x 1 and 3 x 5 run the scalar tail only, 128 x 7 has float4 groups that straddle rows."""
    from nflows_amd import ops
    g = torch.Generator().manual_seed(100 * B + D)
    x = 1.5 * torch.randn(B, D, generator=g)
    params = torch.randn(B, D, 2, generator=g) * torch.tensor([3.0, 1.0])
    if B * D > 8:
        params[0, :4, 0] = torch.tensor([25.0, 20.5, -30.0, 30.0])[:min(4, D)]     # (both sides of the u > 20 branch)
    w_y, w_l = torch.randn(B, D, generator=g), torch.randn(B, generator=g)
    xd, pd = x.to(DEV), params.reshape(B, 2 * D).to(DEV)
    with torch.no_grad():
        out, _ = ops.affine_autoregressive(xd, pd, inverse=inverse)
    for use_y, use_l in ((True, True), (False, True), (True, False)):
        g_y = w_y if use_y else torch.zeros(B, D)
        g_l = w_l if use_l else torch.zeros(B)
        spread = g_l[:, None].expand(B, D)
        truth = cases.affine_element_truth(x, params[..., 0], params[..., 1], g_y, spread, inverse)
        ref32 = cases.affine_element_truth(x, params[..., 0], params[..., 1], g_y, spread, inverse, dtype=torch.float32)
        args = (None if inverse else xd, pd, out if inverse else None, g_y.to(DEV) if use_y else None,
                g_l.to(DEV) if use_l else None, inverse)
        g_x, g_p = ops.affine_autoregressive_backward(*args)
        assert g_x.shape == (B, D) and g_p.shape == (B, 2 * D)
        again = ops.affine_autoregressive_backward(*args)
        assert torch.equal(g_x, again[0]) and torch.equal(g_p, again[1])
        g_p = g_p.view(B, D, 2).cpu()
        what = "%dx%d %s y=%d l=%d " % (B, D, "inverse" if inverse else "forward", use_y, use_l)
        for name, got, r, t in (("g_x", g_x.cpu(), ref32[0], truth[0]), ("g_u", g_p[..., 0], ref32[1], truth[1]),
                                ("g_shift", g_p[..., 1], ref32[2], truth[2])):
            assert torch.isfinite(got).all(), what + name
            cases.within_truth_rule(got.numpy(), r.numpy(), t.numpy(), what + name)
    # the Function every caller of ops.affine_autoregressive gets under autograd runs this kernel
    xg, pg = xd.clone().requires_grad_(True), pd.clone().requires_grad_(True)
    y, lad = ops.affine_autoregressive(xg, pg, inverse=inverse)
    ((y * w_y.to(DEV)).sum() + (lad * w_l.to(DEV)).sum()).backward()
    want = ops.affine_autoregressive_backward(None if inverse else xd, pd, out if inverse else None, w_y.to(DEV), w_l.to(DEV), inverse)
    assert torch.equal(xg.grad, want[0]) and torch.equal(pg.grad, want[1])
    # an output the loss does not use reaches the kernel as a null gradient, not as a tensor of zeros
    seen = []
    real = ops.affine_autoregressive_backward
    monkeypatch.setattr(ops, "affine_autoregressive_backward", lambda *a: (seen.append((a[3] is None, a[4] is None)), real(*a))[1])
    for use_y in (True, False):
        xg, pg = xd.clone().requires_grad_(True), pd.clone().requires_grad_(True)
        y, lad = ops.affine_autoregressive(xg, pg, inverse=inverse)
        ((y * w_y.to(DEV)).sum() if use_y else (lad * w_l.to(DEV)).sum()).backward()
        want = real(None if inverse else xd, pd, out if inverse else None, w_y.to(DEV) if use_y else None,
                    None if use_y else w_l.to(DEV), inverse)
        assert torch.equal(xg.grad, want[0]) and torch.equal(pg.grad, want[1])
    assert seen == [(False, True), (True, False)]


def test_affine_autoregressive_backward_kernel_takes_unaligned_buffers():
    """views that start 4 bytes into an allocation take the scalar path: the same bits as the aligned launch"""
    from nflows_amd import ops
    B, D = 130, 12
    g = torch.Generator().manual_seed(7)
    x, p = torch.randn(B, D, generator=g).to(DEV), torch.randn(B, 2 * D, generator=g).to(DEV)
    g_y, g_l = torch.randn(B, D, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)
    want = ops.affine_autoregressive_backward(x, p, None, g_y, g_l, False)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        buf[1:].copy_(t.reshape(-1))
        return buf[1:].view(t.shape)

    xs = shifted(x)
    assert xs.data_ptr() % 16 == 4 and xs.is_contiguous()
    got = ops.affine_autoregressive_backward(xs, shifted(p), None, shifted(g_y), g_l, False)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 3. one layer ----------------------------------------------------------------------------------------------------------

def layer_truth(layer, x, w_y, w_l):
    layer64 = copy.deepcopy(layer).double()
    x64 = x.detach().double().requires_grad_(True)
    y, lad = maf_cases.affine_layer_forward(layer64, x64)
    ((y * w_y.double()).sum() + (lad * w_l.double()).sum()).backward()
    return [y.detach(), lad.detach(), x64.grad] + [p.grad for p in layer64.parameters()]


@pytest.mark.parametrize("features,hidden,blocks,rows", cases.ACCEPTED)
def test_one_layer_against_float64(features, hidden, blocks, rows, k14_calls):
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform
    torch.manual_seed(1000 * features + hidden + blocks)
    layer = sharpened(MaskedAffineAutoregressiveTransform(features=features, hidden_features=hidden, num_blocks=blocks)).to(DEV)
    x = 1.2 * torch.randn(rows, features, device=DEV)
    w_y, w_l = torch.randn(rows, features, device=DEV), torch.randn(rows, device=DEV)

    def run(fused):
        with k25(fused):
            layer.zero_grad(set_to_none=True)
            xin = x.clone().requires_grad_(True)
            y, lad = layer(xin)
            ((y * w_y).sum() + (lad * w_l).sum()).backward()
        return [y.detach().clone(), lad.detach().clone(), xin.grad.clone()] + [p.grad.clone() for p in layer.parameters()]

    got = run(True)
    assert len(k14_calls) == 1, "one K14 forward launch per layer with the switch on"
    again = run(True)
    assert len(k14_calls) == 2
    eager = run(False)
    assert len(k14_calls) == 2, "none with it off"
    names = ["outputs", "logabsdet", "grad_inputs"] + [n for n, _ in layer.named_parameters()]
    assert_within_eager(names, got, eager, layer_truth(layer, x, w_y, w_l))
    for name, a, b in zip(names, got, again):
        assert torch.equal(a, b), name + ": a second identical call gave other bits"
    masks = {n[:-len("mask")]: m for n, m in layer.named_buffers() if n.endswith("mask")}
    masked_out = 0
    for (name, _), grad in zip(layer.named_parameters(), got[3:]):
        if name.endswith("weight"):
            mask = masks[name[:-len("weight")]]
            assert not grad[mask == 0].any(), name + ": a masked-out weight has a gradient"
            masked_out += int((mask == 0).sum())
    assert masked_out > 0


# ---- 4. whole flows against the real reference -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def G(golden_dir):
    return cases.load_grads(golden_dir)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", list(cases.GRAD_CASES))
def test_flow_gradients_match_reference_autograd(G, name, fused, k14_calls):
    flow = cases.build_grad_flow(name, G).to(DEV)
    x, _ = maf_cases.fixture_inputs(name)
    with k25(fused):
        loss, grads = cases.flow_gradients(flow, x.to(DEV))
    layers = cases.grad_case_config(name)["num_layers"]
    assert len(k14_calls) == (layers if fused else 0)
    close_to_truth(loss, G[name + "/loss32"], G[name + "/loss64"], name + " loss")
    assert set(grads) == set(k.split("/g64/")[1] for k in G if k.startswith(name + "/g64/"))
    for k, got in grads.items():
        close_to_truth(got, G["%s/g32/%s" % (name, k)], G["%s/g64/%s" % (name, k)], "%s %s" % (name, k))


# ---- 5. fallbacks ------------------------------------------------------------------------------------------------------------

def test_refused_nets_train_through_the_eager_path(k14_calls):
    for name, (net, rows, context, scope) in cases.refused().items():
        net = net.to(DEV)
        features = net.initial_layer.in_features
        x = torch.randn(rows, features, device=DEV, requires_grad=True)
        context = None if context is None else context.to(DEV)
        with (torch.autocast("cuda", dtype=torch.bfloat16) if scope == "autocast" else contextlib.nullcontext()):
            out = net(x, context)
            out.float().square().sum().backward()
        assert len(k14_calls) == 0, name
        assert x.grad is not None and torch.isfinite(x.grad).all(), name
        for pname, p in net.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (name, pname)
    # the same net without any of it takes K14
    net = cases.made().to(DEV)
    net(torch.randn(256, 8, device=DEV)).sum().backward()
    assert len(k14_calls) == 1


def test_autoregressive_spline_layer_trains_through_k14(k14_calls):
    """Every transform built on MADE gets the fused conditioner: the rational-quadratic autoregressive layer (its
    default, constrained spline on [0, 1]: 3 K + 1 logits per feature) at 256 rows, against its own switched-off path and
    a float64 copy of that path (rule 3)."""
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform
    torch.manual_seed(12)
    layer = sharpened(MaskedPiecewiseRationalQuadraticAutoregressiveTransform(features=12, hidden_features=32, num_bins=8)).to(DEV)
    x = 0.05 + 0.9 * torch.rand(256, 12, device=DEV)
    w_y, w_l = torch.randn(256, 12, device=DEV), torch.randn(256, device=DEV)

    from nflows_amd.transforms import splines

    def restated(module, xin):
        """the switched-off path in tensor operations: the eager masked Linears, then the functional per element
        (float64: K5d; a MADE has no `hidden_features`, so the logits are not divided, autoregressive.py:464-466)"""
        K = module.num_bins
        assert module.tails is None
        p = maf_cases.made_forward(module.autoregressive_net, xin).view(xin.shape[0], xin.shape[1], 3 * K + 1)
        y, lad = splines.rational_quadratic_spline(
            xin, p[..., :K], p[..., K:2 * K], p[..., 2 * K:], inverse=False,
            min_bin_width=module.min_bin_width, min_bin_height=module.min_bin_height, min_derivative=module.min_derivative)
        return y, lad.sum(dim=1)

    def run(module, xin, fused, forward=None):
        with k25(fused):
            module.zero_grad(set_to_none=True)
            xin = xin.clone().requires_grad_(True)
            y, lad = module(xin) if forward is None else forward(module, xin)
            ((y * w_y.to(xin.dtype)).sum() + (lad * w_l.to(xin.dtype)).sum()).backward()
        return [y.detach().clone(), lad.detach().clone(), xin.grad.clone()] + [p.grad.clone() for p in module.parameters()]

    got = run(layer, x, True)
    assert len(k14_calls) == 1
    eager = run(layer, x, False)
    assert len(k14_calls) == 1
    truth = run(copy.deepcopy(layer).double(), x.double(), False, forward=restated)
    names = ["outputs", "logabsdet", "grad_inputs"] + [n for n, _ in layer.named_parameters()]
    assert_within_eager(names, got, eager, truth)


# ---- 6. training and capture -------------------------------------------------------------------------------------------------

def _two_moons(n, generator):
    t = np.pi * torch.rand(n, generator=generator)
    upper = torch.rand(n, generator=generator) < 0.5
    x = torch.where(upper, torch.cos(t), 1 - torch.cos(t))
    y = torch.where(upper, torch.sin(t), 0.5 - torch.sin(t))
    return torch.stack((x, y), dim=1) + 0.1 * torch.randn(n, 2, generator=generator)


@pytest.mark.parametrize("which", ["moons", "d8_l5"])
def test_flows_lower_their_loss(which, k14_calls):
    from nflows_amd import configs
    g = torch.Generator().manual_seed(4)
    if which == "moons":
        flow, data = configs.moons_maf_flow(), _two_moons(512, g)
    else:
        flow = configs.masked_affine_flow(features=8, hidden_features=64, num_layers=5, permutation="reverse", seed=3)
        data = torch.randn(512, 8, generator=g) * torch.linspace(0.3, 1.5, 8) + 0.7
    flow, data = flow.to(DEV).train(), data.to(DEV)
    layers = sum(1 for t in flow._transform._transforms if hasattr(t, "autoregressive_net"))
    opt = torch.optim.Adam(flow.parameters(), lr=5e-3)
    losses = []
    for _ in range(15):
        opt.zero_grad()
        loss = -flow.log_prob(data).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert len(k14_calls) == 15 * layers
    assert np.isfinite(losses).all() and losses[-1] < losses[0] - 0.05, losses


def test_graphed_training_step_follows_the_eager_steps(k14_calls):
    import nflows_amd
    from nflows_amd import configs
    from nflows_amd.graphs import GraphedTrainStep
    flow_a = configs.masked_affine_flow(features=8, hidden_features=64, num_layers=5, permutation="reverse", seed=5).to(DEV).train()
    flow_b = copy.deepcopy(flow_a)
    g = torch.Generator().manual_seed(6)
    batches = [(torch.randn(512, 8, generator=g) * 0.8 + 0.2).to(DEV) for _ in range(6)]
    warm = 2
    opt_a = torch.optim.Adam(flow_a.parameters(), lr=1e-3, capturable=True)
    eager_losses = []
    for i, xb in enumerate([batches[0]] * warm + batches):   # (the graphed step warms up on batches[0])
        opt_a.zero_grad(set_to_none=True)
        loss = -flow_a.log_prob(xb).mean()
        loss.backward()
        opt_a.step()
        if i >= warm:
            eager_losses.append(loss.item())
    assert len(k14_calls) == 5 * (warm + len(batches))
    opt_b = torch.optim.Adam(flow_b.parameters(), lr=1e-3, capturable=True)
    step = GraphedTrainStep(flow_b, opt_b, batches[0], warmup=warm)
    graphed_losses = [step(xb).item() for xb in batches]
    nflows_amd.check_status()
    np.testing.assert_allclose(graphed_losses, eager_losses, rtol=2e-5, atol=2e-5)
    assert graphed_losses[-1] < graphed_losses[0]
