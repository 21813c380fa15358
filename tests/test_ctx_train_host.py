"""K27's host side on the CPU: the table of tests/ctx_train_cases.py against its own yardsticks, the emulated split-bf16
scheme and two mutants; the wiring of autograd.ResidualNetHiddenCtx / MadeNetCtx with the kernels replaced by
tensor-operation emulations of their contracts (include/nflows_amd.h); the gates; GraphedTrainStep's argument checks."""
import copy

import numpy as np
import pytest
import torch

import ctx_train_cases as cc
from test_train_kernels_host import emulated_linear

NAMES = [c.name for c in cc.CASES]


# ------------------------------------------------------------------------------------------------------------- the table
def test_the_table_covers_what_it_says():
    glu = [c for c in cc.CASES if c.mode == "glu"]
    add = [c for c in cc.CASES if c.mode == "add"]
    assert set(cc.di_of(c) for c in glu) >= {4, 8, 32, 36, 64} and any((c.d + c.C) % 4 for c in glu)
    assert set(c.nb for c in glu) == {1, 2, 3} and set(c.nb for c in add) == {0, 1, 2, 3}
    assert set(c.H for c in glu) == {128, 64, 4} and {0, 24, 40} <= set(c.out for c in cc.CASES)
    assert sorted((c.made, c.H, c.C) for c in add if c.made) == [(21, 64, 5), (63, 128, 16)]
    assert all(c.B <= 256 for c in cc.CASES) and sorted(cc.CAPS) == sorted(NAMES)
    sat = cc.prepared("glu_saturated_hidden")
    values = set(np.unique(sat["planes"][0].numpy()).tolist())
    assert values == {88.80000305175781, -88.80000305175781, 104.0, -104.0, 30000.0, -30000.0}
    # the gate's gradient is pinned to exactly zero where float32 cannot tell s from 0 or 1 -- and only there
    closed = cc.gate_is_exactly_closed(np.array([-104.0, -88.8, -17.0, 0.0, 17.0, 17.5, 88.8, 104.0, 30000.0, -30000.0]))
    assert closed.tolist() == [True, False, False, False, False, True, True, True, True, True]
    for k in range(2):
        t, A = sat["truth"]["plane_grads%d" % k]
        c = sat["planes"][k].numpy()
        assert not t[np.abs(c) >= 104.0].any() and not A[np.abs(c) >= 104.0].any() and not t[c > 88.0].any()
        assert A[(c < -88.0) & (c > -100.0)].all()


@pytest.mark.parametrize("name", NAMES)
def test_yardsticks_and_the_emulated_scheme_hold_the_stored_caps(name):
    """Both yardsticks at half their caps (the caps ARE 2 x their maximum, rounded up); the MADE cases' seeds are the first
    at which the split-bf16 scheme emulated on the CPU (six products per k-step of 16, one rounding of the accumulator
    each) stays within them."""
    p = cc.prepared(name)
    caps = cc.CAPS[name]
    assert caps == cc.caps_from(*cc.yardsticks(p)), "%s: the stored caps are not the yardsticks' (python tests/ctx_train_cases.py)" % name
    for stats in cc.yardsticks(p):
        half = dict((k, tuple(v / cc.PARITY * 1.006 for v in c)) for k, c in caps.items())   # (1.006: the two-digit rounding)
        assert not cc.misses(stats, half), (name, cc.misses(stats, half))
    if not p["case"].made:      # (the emulation is the MADE cases' seed rule, ctx_train_cases.py; elsewhere it decides nothing)
        return
    emu = cc.stats_of(cc.chain(p["case"], p["e"], p["xp"], p["gp"], p["masks"], p["planes"], p["initial"], p["pre"],
                               emulated_linear(), cc.sigmoid_ref), p["truth"], name)
    cc.assert_within_caps(name + " emulated", emu, caps)


@pytest.mark.parametrize("name,mutant,arrays", [
    ("glu_nb2_out24", "gate_c", ("hidden",)),                 # gated with the logit instead of its sigmoid
    ("glu_nb2_out24", "pair_g", ("grads3", "grads1")),        # the second Linear handed g instead of g sigmoid(c)
    ("glu_w32_out40", "gate_c", ("hidden",)),
    ("glu_w32_out40", "pair_g", ("grads1",)),
])
def test_mutants_miss(name, mutant, arrays):
    """Recorded (mean ratio / its cap): gate_c `hidden` 1.5e4 = 1.8e6 x (glu_nb2_out24), 1.1e5 = 1.3e6 x (glu_w32_out40);
    pair_g `grads3` 2.7e5 = 2.2e6 x, `grads1` 6.9e4 = 2.3e6 x (glu_nb2_out24), `grads1` 2.2e5 = 2.0e6 x (glu_w32_out40)."""
    p = cc.prepared(name)
    stats = cc.yardsticks(p, mutant)[0]
    missed = set(m[0] for m in cc.misses(stats, cc.CAPS[name]))
    assert set(arrays) <= missed, (name, mutant, sorted(missed))
    for k in arrays:     # ... and by a wide margin (recorded: the mean ratio of the mutant over its cap)
        factor = stats[k][0] / cc.CAPS[name][k][0]
        print("%s %s %s: mean ratio %.3g = %.3g x its cap" % (name, mutant, k, stats[k][0], factor))
        assert factor > 1000.0


# ------------------------------------------------------------------------------------------------------------ the wiring
def emulate_kernels(monkeypatch):
    """ops.* of the K27 path as float64 tensor operations of their contracts; returns the list of calls"""
    from nflows_amd import ops
    book, calls = {}, []

    def pad2(w, rows, cols):
        out = w.new_zeros(rows, cols)
        out[:w.shape[0], :w.shape[1]] = w
        return out

    def pad1(b, n):
        return torch.cat((b, b.new_zeros(n - b.shape[0])))

    def pack(w_in, b_in, blocks, final=None, masks=None):
        m = masks if masks is not None else [None] * (2 + 2 * len(blocks))
        w = lambda t, k: t.detach() if m[k] is None else t.detach() * m[k]      # noqa: E731
        di = (w_in.shape[1] + 3) // 4 * 4
        key = float(len(book))
        fin = None
        if final is not None:
            rows = (final[0].shape[0] + 3) // 4 * 4 if masks is not None else final[0].shape[0]
            fin = (pad2(w(final[0], -1), rows, 128), pad1(final[1].detach(), rows))
        book[key] = dict(w_in=pad2(w(w_in, 0), 128, di), b_in=pad1(b_in.detach(), 128),
                         blocks=[(pad2(w(w0, 1 + 2 * k), 128, 128), pad1(b0.detach(), 128), pad2(w(w1, 2 + 2 * k), 128, 128),
                                  pad1(b1.detach(), 128)) for k, (w0, b0, w1, b1) in enumerate(blocks)], final=fin)
        tag = torch.tensor([key], dtype=torch.float64)
        return tag, tag, tag, (tag if final is not None else None)

    def forward(mode, x, planes, fwd_w, fwd_b, num_blocks, final_bias=None, out_features=0, initial_plane=None):
        assert x.shape[1] % 4 == 0 and x.shape[0] % 128 == 0 and len(planes) == num_blocks
        assert all(p.shape == (x.shape[0], 128) for p in planes)
        calls.append(("forward", mode))
        w = book[fwd_w.item()]
        h = x @ w["w_in"].t() + w["b_in"]
        if mode == ops.TRAIN_CTX_ADD:
            h = h + initial_plane
        else:
            assert initial_plane is None
        saved, pre = [], []
        for k, (w0, b0, w1, b1) in enumerate(w["blocks"]):
            t = torch.relu(h)
            a = t @ w0.t() + b0
            u = torch.relu(a + planes[k] if mode == ops.TRAIN_CTX_ADD else a)
            saved += [t, u]
            y = u @ w1.t() + b1
            pre.append(y)
            h = h + (y * torch.sigmoid(planes[k]) if mode == ops.TRAIN_CTX_GLU else y)
        params = None
        if final_bias is not None:
            params = h @ w["final"][0].t() + w["final"][1]
            assert params.shape[1] == out_features
        empty = x.new_zeros(0, x.shape[0], 128)
        return (h, torch.stack(saved) if saved else empty, params,
                (torch.stack(pre) if pre else empty) if mode == ops.TRAIN_CTX_GLU else None)

    def backward(mode, grad, bwd_w, saved, num_identity, planes=(), pre=None, from_params=False):
        calls.append(("backward", mode, from_params))
        w = book[bwd_w.item()]
        nb = saved.shape[0] // 2
        gh = g_hidden = grad @ w["final"][0] if from_params else grad
        assert gh.shape[1] == 128
        grads, pgs, gts = [None] * (2 * nb), [None] * nb, [None] * nb
        for k in reversed(range(nb)):
            w0, b0, w1, b1 = w["blocks"][k]
            gt = gh
            if mode == ops.TRAIN_CTX_GLU:
                s = torch.sigmoid(planes[k])
                pgs[k], gts[k] = gh * pre[k] * s * (1 - s), gh * s
                gt = gts[k]
            ga = (gt @ w1) * (saved[2 * k + 1] > 0)
            gh = gh + (ga @ w0) * (saved[2 * k] > 0)
            grads[2 * k + 1], grads[2 * k] = ga, gh
        gx = gh @ w["w_in"]
        assert gx.shape[1] == num_identity
        glu = mode == ops.TRAIN_CTX_GLU and nb
        return (gx, torch.stack(grads) if grads else grad.new_zeros(0, grad.shape[0], 128), g_hidden,
                torch.stack(pgs) if glu else None, torch.stack(gts) if glu else None)

    monkeypatch.setattr(ops, "pack_resnet_hidden_train", pack)
    monkeypatch.setattr(ops, "pack_made_train", lambda w_in, b_in, blocks, final, masks: pack(w_in, b_in, blocks, final, masks))
    monkeypatch.setattr(ops, "resnet_hidden_forward_ctx", forward)
    monkeypatch.setattr(ops, "resnet_backward_ctx", backward)
    monkeypatch.setattr(ops, "linear_wgrad", lambda x, gy, need_bias=True: (gy.t() @ x, gy.sum(0) if need_bias else None))
    monkeypatch.setattr(ops, "linear_wgrad_batched", lambda problems, need_bias=True: [
        (gy.t() @ x, gy.sum(0) if need_bias else None) for x, gy in problems])
    return calls


def check_against_eager(net, emb, x, raw, run, weight):
    """gradients of `run(net, x, emb(raw))` weighted by `weight` on the fused routing (the net's `_fused_training` forced
    open) against autograd through the eager modules of a copy"""
    ref_net, ref_emb = copy.deepcopy(net), copy.deepcopy(emb)
    ref_x, ref_raw = x.detach().clone().requires_grad_(True), raw.detach().clone().requires_grad_(True)
    (run(ref_net, ref_x, ref_emb(ref_raw)) * weight).sum().backward()
    net._fused_training = lambda inputs, context=None: True
    result = run(net, x, emb(raw))
    assert result.shape == weight.shape
    (result * weight).sum().backward()
    pairs = [("inputs", x.grad, ref_x.grad), ("raw context", raw.grad, ref_raw.grad)]
    pairs += [("embedding " + n, p.grad, q.grad) for (n, p), (_, q) in zip(emb.named_parameters(), ref_emb.named_parameters())]
    pairs += [(n, p.grad, q.grad) for (n, p), (_, q) in zip(net.named_parameters(), ref_net.named_parameters())]
    for name, got, want in pairs:
        if want is None:
            assert got is None, name
        else:
            assert got is not None and got.shape == want.shape and torch.allclose(got, want, rtol=1e-9, atol=1e-11), name


def test_function_wiring_with_emulated_kernels(monkeypatch):
    from nflows_amd import ops
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms.made import MADE
    calls = emulate_kernels(monkeypatch)
    torch.manual_seed(0)
    # ResidualNet / GLU: (features, context, hidden, blocks, out, through forward or hidden); 3 + 2 and 21 + 8: odd sums
    for d, C, H, nb, out, whole in ((8, 4, 128, 2, 40, True), (3, 2, 128, 1, 24, True), (21, 8, 52, 2, 40, True),
                                    (12, 5, 64, 3, 16, False), (6, 3, 20, 1, 8, False)):
        net = ResidualNet(d, out, H, context_features=C, num_blocks=nb).double()
        emb = torch.nn.Linear(7, C).double()
        with torch.no_grad():
            for b in net.blocks:
                b.linear_layers[1].weight.mul_(50.0)
        x = torch.randn(256, d, dtype=torch.float64, requires_grad=True)
        raw = torch.randn(256, 7, dtype=torch.float64, requires_grad=True)
        weight = torch.randn(256, out if whole else H, dtype=torch.float64)
        before = len(calls)
        check_against_eager(net, emb, x, raw, (lambda n, a, c: n(a, c)) if whole else (lambda n, a, c: n.hidden(a, c)), weight)
        assert calls[before:] == [("forward", ops.TRAIN_CTX_GLU), ("backward", ops.TRAIN_CTX_GLU, whole)], calls[before:]
    # MADE / ADD: odd feature counts and output widths, narrow H, no block
    for D, C, H, nb, mult in ((8, 3, 128, 2, 2), (21, 5, 64, 2, 2), (5, 16, 32, 1, 3), (7, 2, 128, 0, 1), (63, 16, 128, 3, 2)):
        net = MADE(D, H, context_features=C, num_blocks=nb, output_multiplier=mult).double()
        emb = torch.nn.Linear(7, C).double()
        with torch.no_grad():
            for b in net.blocks:
                b.linear_layers[1].weight.mul_(50.0)
        x = torch.randn(128, D, dtype=torch.float64, requires_grad=True)
        raw = torch.randn(128, 7, dtype=torch.float64, requires_grad=True)
        before = len(calls)
        check_against_eager(net, emb, x, raw, lambda n, a, c: n(a, c), torch.randn(128, D * mult, dtype=torch.float64))
        assert calls[before:] == [("forward", ops.TRAIN_CTX_ADD), ("backward", ops.TRAIN_CTX_ADD, True)], calls[before:]


# -------------------------------------------------------------------------------------------------------------- the gates
def test_gates(monkeypatch):
    from nflows_amd import ops
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms.made import MADE
    x = lambda d: torch.randn(256, d)      # noqa: E731
    for d, C in ((48, 16), (45, 16), (3, 1)):            # d + C = 64, 61 (pads to 64), 4
        assert ResidualNet(d, 8, 32, context_features=C)._fusable_with_context(x(d), x(C)), (d, C)
    net = ResidualNet(49, 8, 32, context_features=16)
    assert not net._fusable_with_context(x(49), x(16))                                   # d + C = 65
    net = ResidualNet(8, 8, 32, context_features=4)
    assert net._fusable_with_context(x(8), x(4))
    assert not net._fusable_with_context(x(8), x(4).double())
    assert not net._fusable_with_context(x(8), x(5)) and not net._fusable_with_context(x(8), torch.randn(128, 4))
    del net.blocks[1].context_layer
    assert not net._fusable_with_context(x(8), x(4))                                     # a block without its context_layer
    net = ResidualNet(8, 8, 32, context_features=4)
    net.blocks[0].context_layer = torch.nn.Linear(4, 32, bias=False)
    assert not net._fusable_with_context(x(8), x(4))
    net = ResidualNet(8, 8, 32, context_features=4)
    monkeypatch.setattr(ops, "CTX_TRAINING", False)                                      # NFA_K27=0
    assert not net._fusable_with_context(x(8), x(4))
    made = MADE(8, 32, context_features=3)
    assert not made._fusable_with_context(256, 8, x(3))
    monkeypatch.setattr(ops, "CTX_TRAINING", True)
    assert made._fusable_with_context(256, 8, x(3)) and MADE(21, 64, context_features=5)._fusable_with_context(256, 21, x(5))
    assert not made._fusable_with_context(256, 8, x(3).double()) and not made._fusable_with_context(200, 8, torch.randn(200, 3))
    assert not made._fusable(256, 8, x(3)) and not made._fusable(256, 8)     # K25's own gate: as before, with or without
    assert not MADE(8, 32)._fusable_with_context(256, 8, x(3))               # no context layers at all
    assert not MADE(8, 32, context_features=3, use_residual_blocks=False)._fusable_with_context(256, 8, x(3))
    made.fuse_training = False
    assert not made._fusable_with_context(256, 8, x(3))
    # on the CPU nothing takes the fused path, and a net built with a context but called without one goes where it went
    net = ResidualNet(8, 8, 32, context_features=4)
    a = torch.randn(256, 8, requires_grad=True)
    assert not net._fused_training(a, x(4)) and not net._fused_training(torch.randn(256, 12, requires_grad=True), None)
    assert not MADE(8, 32, context_features=3)._fused_training(a, x(3)) and not MADE(8, 32, context_features=3)._fused_training(a)
    net.fuse_training = False
    assert net(a, x(4)).shape == (256, 8)


def test_fuse_training_false_and_missing_context_refuse_on_a_pretend_device(monkeypatch):
    """the device part of the ResidualNet gate with `is_cuda` out of the way: what is left is the gate's own logic"""
    from nflows_amd import ops
    from nflows_amd.nn.nets import ResidualNet

    class OnDevice(torch.Tensor):
        is_cuda = True

    a = torch.randn(256, 8, requires_grad=True).as_subclass(OnDevice)
    c = torch.randn(256, 4)
    net = ResidualNet(8, 8, 32, context_features=4)
    assert net._fused_training(a, c)
    assert not net._fused_training(torch.randn(256, 12, requires_grad=True).as_subclass(OnDevice), None)   # built with a context, called without
    net.fuse_training = False
    assert not net._fused_training(a, c)
    net.fuse_training = True
    monkeypatch.setattr(ops, "CTX_TRAINING", False)
    assert not net._fused_training(a, c)


def test_switch_reads_the_environment():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("0", "False"), (None, "True")):
        env = dict(os.environ, PYTHONPATH=root)
        env.pop("NFA_K27", None)
        if value is not None:
            env["NFA_K27"] = value
        out = subprocess.run([sys.executable, "-c", "from nflows_amd import ops; print(ops.CTX_TRAINING)"], env=env,
                             capture_output=True, text=True, check=True).stdout.strip()
        assert out == want


def test_graphed_train_step_argument_checks():
    from nflows_amd.graphs import GraphedTrainStep
    with pytest.raises(NotImplementedError):
        GraphedTrainStep(None, None, torch.randn(4, 2))
    with pytest.raises(NotImplementedError):
        GraphedTrainStep(None, None, torch.randn(4, 2), example_context=torch.randn(4, 3))
    step = GraphedTrainStep.__new__(GraphedTrainStep)
    step._static_in, step._static_ctx = torch.zeros(4, 2), torch.zeros(4, 3)
    for args in ((torch.zeros(4, 2),), (torch.zeros(4, 2), torch.zeros(4, 5)), (torch.zeros(4, 2), torch.zeros(4, 3).double()),
                 (torch.zeros(5, 2), torch.zeros(4, 3))):
        with pytest.raises(ValueError):
            step(*args)
    step._static_ctx = None
    with pytest.raises(ValueError):
        step(torch.zeros(4, 2), torch.zeros(4, 3))
