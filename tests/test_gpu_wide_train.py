"""K33 on the device (csrc/resnet_train_wide.hip, autograd.ResidualNetWide): training ResidualNet conditioners of 129 .. 256
hidden units.  Truth: the same chain of torch.nn.functional.linear in float64 on the CPU; yardstick: in float32.  The
project's parity rule (tests/test_gpu_wide_layer.py) with no element exempt: mean and 99.9 % quantile of the error against
the truth at most 2 x the yardstick's, no element above 4 x its maximum, everything finite, pad columns exactly zero.
Bit for bit on dyadic data (chunk edges 256 / 257, d_i = 33, the class path's parameter gradients): tests/test_gpu_wide_train_exact.py."""
import copy

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from maf_inverse_cases import error_figures
from nflows_amd import configs, ops
from nflows_amd.nn.nets.resnet import ResidualNet
from oracle import eager

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUS = "cus"   # rows = 64 x (CU count + 1): the persistent loop's second pass
WIDE = "ResidualNetWideBackward"


def assert_parity(got, ref32, truth, what):
    got, ref32, truth = (t.detach().cpu().numpy() for t in (got, ref32, truth))
    assert np.isfinite(got).all() and np.isfinite(ref32).all(), what
    f = error_figures(got, ref32, truth)
    print(what, f)
    assert f["mean"][0] <= 2.0 * f["mean"][1] and f["q999"][0] <= 2.0 * f["q999"][1] and f["above_4x_max"] == 0, (what, f)


# (features in, width, blocks, out, rows)
@pytest.mark.parametrize("di,H,nb,out,rows", [(3, 129, 1, 20, 64), (8, 192, 2, 184, 128), (32, 256, 2, 736, 128),
                                              (64, 256, 3, 1472, 64), (16, 256, 0, 0, 64), (6, 160, 1, 44, CUS)])
def test_kernels_against_the_truth(di, H, nb, out, rows):
    second_pass = rows == CUS
    rows = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) if second_pass else rows
    torch.manual_seed(21)
    net = ResidualNet(di, out or 4, hidden_features=H, num_blocks=nb)
    with torch.no_grad():
        for name, p in net.named_parameters():   # (the default init leaves the blocks near the identity)
            if "final_layer" in name:
                p.mul_(4.0)
            elif "linear_layers.1" in name:
                p.mul_(30.0)
    Hp, dp = (H + 31) // 32 * 32, (di + 3) // 4 * 4
    x = 1.5 * torch.randn(rows, di)
    g = torch.randn(rows, out) if out else F.pad(torch.randn(rows, H), (0, Hp - H))
    dev = copy.deepcopy(net).to(DEV)
    blocks = [(b.linear_layers[0].weight, b.linear_layers[0].bias, b.linear_layers[1].weight, b.linear_layers[1].bias)
              for b in dev.blocks]
    final = (dev.final_layer.weight, dev.final_layer.bias) if out else None
    fwd_w, bias, bwd_w = ops.pack_resnet_wide_train(dev.initial_layer.weight, dev.initial_layer.bias, blocks, final)

    def run(xs, gs):
        hidden, saved, params = ops.resnet_wide_forward(F.pad(xs, (0, dp - di)).to(DEV), fwd_w, bias, H, nb, out)
        gx, grads, g_hidden = ops.resnet_wide_backward(gs.to(DEV), bwd_w, saved, dp, H, from_params=bool(out))
        return hidden, saved, params, gx, grads, g_hidden

    hidden, saved, params, gx, grads, g_hidden = run(x, g)
    masks = [(saved[j, :, :H] > 0).cpu() for j in range(2 * nb)]   # the backward chain's masks are the forward kernel's

    def chain(net, x, g):
        """every array both kernels write, in the dtype of `net`"""
        h = F.linear(x, net.initial_layer.weight, net.initial_layer.bias)
        saved = []
        for b in net.blocks:
            s0 = F.relu(h)
            s1 = F.relu(F.linear(s0, b.linear_layers[0].weight, b.linear_layers[0].bias))
            h = h + F.linear(s1, b.linear_layers[1].weight, b.linear_layers[1].bias)
            saved += [s0, s1]
        params = F.linear(h, net.final_layer.weight, net.final_layer.bias) if out else None
        g_h = F.linear(g, net.final_layer.weight.t()) if out else g[:, :H]
        g_hidden, grads = g_h, [None] * (2 * nb)
        for k in reversed(range(nb)):
            w0, w1 = (l.weight for l in net.blocks[k].linear_layers)
            grads[2 * k + 1] = F.linear(g_h, w1.t()) * masks[2 * k + 1]
            g_h = g_h + F.linear(grads[2 * k + 1], w0.t()) * masks[2 * k]
            grads[2 * k] = g_h
        return h, saved, params, F.linear(g_h, net.initial_layer.weight.t()), grads, g_hidden

    with torch.no_grad():
        ref = chain(net, x, g)
        truth = chain(copy.deepcopy(net).double(), x.double(), g.double())
    got = (hidden, list(saved), params, gx, list(grads), g_hidden)
    for what, a, r, t in zip(("hidden", "saved", "params", "grad_inputs", "grads", "grad_hidden"), got, ref, truth):
        if a is None:
            assert r is None
            continue
        for j, (aj, rj, tj) in enumerate(zip(*[v if isinstance(v, list) else [v] for v in (a, r, t)])):
            width = rj.shape[1]   # the net's own columns; what lies behind them is padding
            assert not aj[:, width:].any(), "%s[%d]: pad columns" % (what, j)
            assert_parity(aj[:, :width], rj, tj, "%s[%d]" % (what, j))
    if second_pass:   # the last 64 rows, run alone, bit for bit
        alone = run(x[-64:], g[-64:])
        for what, a, b in zip(("hidden", "saved", "params", "grad_inputs", "grads", "grad_hidden"), got, alone):
            a, b = (torch.stack(v) if isinstance(v, list) else v for v in (a, b))
            assert torch.equal(a[..., -64:, :], b), what


def test_training_step_through_the_class(monkeypatch):
    monkeypatch.setattr(ResidualNet, "fuse_wide_training_min_rows", 64)   # the kernel itself, whatever the size rule
    flow = configs.rq_nsf_flow(num_layers=2, features=16, hidden_features=192, num_blocks=1, num_bins=8, tail_bound=3.0,
                               seed=26)
    x = torch.randn(64, 16, generator=torch.Generator().manual_seed(4))
    f64, dev = copy.deepcopy(flow).double(), copy.deepcopy(flow).to(DEV)
    net = next(m for m in dev.modules() if isinstance(m, ResidualNet))
    out = net(torch.randn(64, net.initial_layer.in_features, device=DEV))
    assert type(out.grad_fn).__name__ == WIDE, out.grad_fn   # (fails without K33)
    # the truth's pre-activations h_k, a_k stay clear of zero: no ReLU may flip under rounding (the seeds were chosen so)
    pre = []

    def note(net, args):   # (one block: h_0 and a_0)
        h = F.linear(args[0].detach(), net.initial_layer.weight, net.initial_layer.bias)
        first = net.blocks[0].linear_layers[0]
        pre.extend([h.abs().min().item(), F.linear(F.relu(h), first.weight, first.bias).abs().min().item()])
    hooks = [n.register_forward_pre_hook(note) for n in f64.modules() if isinstance(n, ResidualNet)]
    (-eager.flow_log_prob(f64, x.double()).mean()).backward()
    for h in hooks:
        h.remove()
    assert len(pre) == 4 and min(pre) > 1e-5, pre
    (-eager.flow_log_prob(flow, x).mean()).backward()
    (-dev.log_prob(x.to(DEV)).mean()).backward()
    for (name, p), p32, p64 in zip(dev.named_parameters(), flow.parameters(), f64.parameters()):
        assert_parity(p.grad, p32.grad, p64.grad, name)


@pytest.mark.parametrize("how", ["width_128", "width_257", "context", "elu", "rows_96", "switch_off", "no_grad"])
def test_other_nets_keep_their_path(how, monkeypatch):
    monkeypatch.setattr(ResidualNet, "fuse_wide_training_min_rows", 0)
    if how == "switch_off":
        monkeypatch.setattr(ResidualNet, "fuse_wide_training", False)
    torch.manual_seed(5)
    net = ResidualNet(8, 12, hidden_features={"width_128": 128, "width_257": 257}.get(how, 192), num_blocks=1,
                      context_features=3 if how == "context" else None,
                      activation=F.elu if how == "elu" else F.relu).to(DEV)
    rows = 96 if how == "rows_96" else 128
    ctx = torch.randn(rows, 3, device=DEV) if how == "context" else None
    with torch.set_grad_enabled(how != "no_grad"):
        out = net(torch.randn(rows, 8, device=DEV), ctx)
    assert torch.isfinite(out).all() and type(out.grad_fn).__name__ != WIDE, out.grad_fn
