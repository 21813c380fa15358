"""K27 on the device: the conditioner training kernels with a context (nfa_resnet_hidden_forward_ctx_f32,
nfa_resnet_backward_ctx_f32) through the table of tests/ctx_train_cases.py -- every array against float64 element by
element, caps from the two CPU yardsticks, elements without an allowance exact --, saturated and NaN logits, later passes
of the persistent loops, and the class level: conditional flows whose gradients (parameters, embedding net, raw context)
are held to 2 x the eager fp32 path's error against the float64 flow, determinism, and one captured training step.
Run with `-m gpu`; -s prints every figure."""
import copy

import numpy as np
import pytest
import torch

import ctx_train_cases as cc
import maf_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(t):
    return (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def on_device(case, net, x, g, planes, initial, from_hidden=False):
    """packer, forward kernel, backward kernel: {array: device tensor} of everything they write.  from_hidden: a case with
    a final Linear enters the backward pass with d loss / d hidden = g W_f formed by a library GEMM (the other entry)."""
    from nflows_amd import ops
    nb, di = case.nb, cc.di_of(case)
    out = (2 * case.made + 3) // 4 * 4 if case.made else case.out
    mode = ops.TRAIN_CTX_GLU if case.mode == "glu" else ops.TRAIN_CTX_ADD
    blocks = [tuple(dev(t) for t in b) for b in net["blocks"]]
    final = None if net["final"] is None else tuple(dev(t) for t in net["final"])
    if net["masks"] is not None:
        fw, fb, bw, fbias = ops.pack_made_train(dev(net["w_in"]), dev(net["b_in"]), blocks, final, [dev(m) for m in net["masks"]])
    else:
        w_in = torch.nn.functional.pad(net["w_in"], (0, di - net["w_in"].shape[1]))
        fw, fb, bw, fbias = ops.pack_resnet_hidden_train(dev(w_in), dev(net["b_in"]), blocks, final)
    xd, gd = dev(cc.padded(host(x), di)), dev(cc.padded(host(g), out or 128))
    pd = [dev(p) for p in planes]
    hidden, saved, params, pre = ops.resnet_hidden_forward_ctx(mode, xd, pd, fw, fb, nb, fbias, out,
                                                               initial_plane=None if initial is None else dev(initial))
    arrays = {"hidden": hidden}
    if final is not None:
        arrays["params"] = params
    if final is not None and not from_hidden:
        gx, grads, arrays["grad_hidden"], pg, gt = ops.resnet_backward_ctx(mode, gd, bw, saved, di, pd, pre, from_params=True)
    else:
        gx, grads, _, pg, gt = ops.resnet_backward_ctx(mode, gd, bw, saved, di, pd, pre)
    arrays["grad_inputs"] = gx
    for j in range(2 * nb):
        arrays["saved%d" % j], arrays["grads%d" % j] = saved[j], grads[j]
    if case.mode == "glu":
        for k in range(nb):
            arrays["pre%d" % k], arrays["plane_grads%d" % k], arrays["gated_grads%d" % k] = pre[k], pg[k], gt[k]
    else:
        assert pre is None and pg is None and gt is None
    torch.cuda.synchronize()
    return arrays


def truth_for(p, arrays, x=None, g=None, planes=None, initial=None):
    """float64 truth and allowance, the backward pass through the masks and the pre{k} the forward KERNEL produced"""
    case, e = p["case"], p["e"]
    if x is None:
        fwd = dict((k, v) for k, v in p["truth"].items() if k in cc.forward_arrays(case))
        g, planes = p["gp"], p["planes"]
    else:
        fwd = cc.forward_truth(case, e, x, planes, initial)[0]
    masks = [host(arrays["saved%d" % j]) > 0.0 for j in range(2 * case.nb)]
    pre = [host(arrays["pre%d" % k]) for k in range(case.nb)] if case.mode == "glu" else None
    truth = dict(fwd)
    truth.update(cc.backward_truth(case, e, g, masks, planes, pre))
    return truth


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_table(name):
    p = cc.prepared(name)
    case = p["case"]
    arrays = on_device(case, p["net"], p["x"], p["g"], p["planes"], p["initial"])
    truth = truth_for(p, arrays)
    assert sorted(truth) == sorted(arrays)
    got = dict((k, host(v)) for k, v in arrays.items())
    if case.kind == "saturated":
        assert not any(np.isnan(v).any() for v in got.values()), "a saturated gate produced a NaN"
        for k in range(case.nb):
            closed = cc.gate_is_exactly_closed(p["planes"][k])
            assert closed.any() and not got["plane_grads%d" % k][closed].any()
    if case.H < 128:       # the padded units: exactly zero in everything 128 wide
        for k, v in got.items():
            if v.shape[1] == 128:
                assert not v[:, case.H:].any(), "%s: %s is not zero past the net's width" % (name, k)
    cc.assert_within_caps(name, cc.stats_of(got, truth, name), cc.CAPS[name], verbose=True)


@pytest.mark.parametrize("name", ["glu_nb2_out24", "add_nb2_out24", "add_nb0_out40"])
def test_backward_entry_from_the_hidden_gradient(name):
    """A net WITH a final Linear entering the backward pass through the other entry: d loss / d hidden from a library GEMM.
    Same table rule; the incoming gradient is an input here, so the caps are this run's own yardsticks'."""
    p = cc.prepared(name)
    case = p["case"]._replace(out=0, name=name + "_from_hidden")
    net = dict(p["net"], final=None)
    g_hidden = torch.from_numpy(p["gp"]) @ p["net"]["final"][0]
    e = dict(p["e"], W_f=None, b_f=None)
    arrays = on_device(case, net, p["x"], g_hidden, p["planes"], p["initial"])
    gp = cc.padded(host(g_hidden), 128)
    fwd, masks64 = cc.forward_truth(case, e, p["xp"], p["planes"], p["initial"])
    pre64 = [fwd["pre%d" % k][0].astype(np.float32) for k in range(case.nb)] if case.mode == "glu" else None
    own = dict(fwd)
    own.update(cc.backward_truth(case, e, gp, masks64, p["planes"], pre64))
    caps = cc.caps_from(*(cc.stats_of(cc.chain(case, e, p["xp"], gp, masks64, p["planes"], p["initial"], pre64,
                                               cc._linear_with_plane(lin), sig), own, case.name)
                          for lin, sig in ((cc.linear_ref, cc.sigmoid_ref), (cc.linear_seq, cc.sigmoid_seq))))
    q = dict(p, case=case, e=e)
    truth = truth_for(q, arrays, p["xp"], gp, p["planes"], p["initial"])
    cc.assert_within_caps(case.name, cc.stats_of(dict((k, host(v)) for k, v in arrays.items()), truth, case.name), caps, verbose=True)


def test_a_row_of_nan_logits_stays_in_its_row():
    p = cc.prepared("glu_nb2_hidden")
    planes = [t.clone() for t in p["planes"]]
    planes[0][5, :] = float("nan")
    clean = on_device(p["case"], p["net"], p["x"], p["g"], p["planes"], None)
    dirty = on_device(p["case"], p["net"], p["x"], p["g"], planes, None)
    hidden = host(dirty["hidden"])
    assert np.isnan(hidden[5]).all()
    keep = np.arange(hidden.shape[0]) != 5
    assert not np.isnan(hidden[keep]).any() and np.array_equal(hidden[keep], host(clean["hidden"])[keep])


@pytest.mark.parametrize("name", ["glu_nb2_out24", "add_nb2_out24"])
def test_later_passes_are_bit_equal_to_first_passes(name):
    """128 (2 CU + 1) rows on the grid's 2 CU workgroups: one workgroup walks a second row block, the weight ring carrying
    on from the slot the first left.  Its rows, and the first pass's, are bit-equal to launches on those rows alone."""
    CU = torch.cuda.get_device_properties(0).multi_processor_count
    first, B = 256 * CU, 128 * (2 * CU + 1)
    case = cc.BY_NAME[name]._replace(B=B, name=name + "_later_pass")
    net = cc.net_of(case)
    x, g, planes, initial = cc.data_of(case)
    whole = on_device(case, net, x, g, planes, initial)
    for lo, hi in ((first - 128, first), (first, B)):
        part = on_device(case._replace(B=hi - lo), net, x[lo:hi], g[lo:hi], [q[lo:hi].contiguous() for q in planes],
                         None if initial is None else initial[lo:hi].contiguous())
        for k in sorted(whole):
            assert torch.equal(whole[k][lo:hi], part[k]), "%s: %s of rows %d .. %d differs from a launch on those rows alone" % (
                name, k, lo, hi)


# ------------------------------------------------------------------------------------------------------------ class level
def spline_flow():
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms import (CompositeTransform, PiecewiseRationalQuadraticCouplingTransform,
                                       RandomPermutation)
    from nflows_amd.utils import create_alternating_binary_mask
    torch.manual_seed(27)
    D, C = 6, 5
    layers = []
    for i in range(3):
        layers.append(RandomPermutation(D))
        layers.append(PiecewiseRationalQuadraticCouplingTransform(
            create_alternating_binary_mask(D, even=(i % 2 == 0)),
            lambda i_, o_: ResidualNet(i_, o_, hidden_features=32, context_features=C, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=3.0))
    return Flow(CompositeTransform(layers), StandardNormal([D]), embedding_net=torch.nn.Linear(7, C)), D, 7


def maf_flow():
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.transforms import (CompositeTransform, MaskedAffineAutoregressiveTransform, RandomPermutation)
    torch.manual_seed(28)
    D, C = 5, 3
    layers = []
    for _ in range(3):
        layers.append(RandomPermutation(D))
        layers.append(MaskedAffineAutoregressiveTransform(features=D, hidden_features=32, context_features=C, num_blocks=2))
    return Flow(CompositeTransform(layers), StandardNormal([D])), D, C


def sharpen(flow):
    """the blocks' second Linears are initialised at 1e-3: scaled up so that every path carries signal"""
    with torch.no_grad():
        for name, p in flow.named_parameters():
            if "linear_layers.1" in name:
                p.mul_(60.0)
    return flow


class eager_conditioners:
    """every conditioner's eager modules (the float64 truth)"""

    def __enter__(self):
        from nflows_amd.nn.nets.resnet import _Net
        from nflows_amd.transforms.made import MADE
        self.saved = (_Net.fuse_training, MADE.fuse_training)
        _Net.fuse_training = MADE.fuse_training = False

    def __exit__(self, *exc):
        from nflows_amd.nn.nets.resnet import _Net
        from nflows_amd.transforms.made import MADE
        _Net.fuse_training, MADE.fuse_training = self.saved


def loss_and_grads(flow, x, raw, log_prob=None):
    """(log_prob values, {name: gradient}) of -log_prob(x, context=raw).mean(), the raw context's gradient as 'raw'"""
    flow.zero_grad(set_to_none=True)
    raw = raw.detach().clone().requires_grad_(True)
    lp = flow.log_prob(x, context=raw) if log_prob is None else log_prob(flow, x, raw)
    (-lp.mean()).backward()
    grads = dict((n, p.grad.detach().clone()) for n, p in flow.named_parameters())
    assert all(g is not None for g in grads.values())
    grads["raw"] = raw.grad.detach().clone()
    return lp.detach(), grads


def rel_err(got, truth):
    truth = truth.double()
    return float((got.double() - truth).norm() / truth.norm().clamp_min(1e-300))


def count_calls(monkeypatch):
    from nflows_amd import ops
    calls = []
    real = ops.resnet_hidden_forward_ctx

    def counted(*args, **kwargs):
        calls.append(args[0])
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, "resnet_hidden_forward_ctx", counted)
    return calls


@pytest.mark.parametrize("make", [spline_flow, maf_flow])
def test_conditional_flow_gradients_against_float64(make, monkeypatch):
    """-log_prob(x, context=raw).mean().backward() on the fused path: log_prob, every parameter's gradient and the raw
    context's within PARITY x the eager fp32 path's relative error against the same flow in float64 -- and the call DID
    reach the new entry point (this fails on a tree without K27), twice bit for bit."""
    from nflows_amd import ops
    flow, D, C_raw = make()
    flow = sharpen(flow).to(DEV)
    gen = torch.Generator().manual_seed(5)
    x, raw = torch.randn(256, D, generator=gen).to(DEV), torch.randn(256, C_raw, generator=gen).to(DEV)
    flow64 = copy.deepcopy(flow).double()
    # (the affine autoregressive layer has no float64 kernel: the MAF's truth is its restatement in tensor operations)
    restated = (lambda f, a, c: maf_cases.restated(f, a, f._embedding_net(c))[2]) if make is maf_flow else None
    with eager_conditioners():
        lp64, truth = loss_and_grads(flow64, x.double(), raw.double(), restated)
    calls = count_calls(monkeypatch)
    lp, fused = loss_and_grads(flow, x, raw)
    assert len(calls) == 3, "the conditioners with a context did not reach nfa_resnet_hidden_forward_ctx_f32 (%d calls)" % len(calls)
    lp2, again = loss_and_grads(flow, x, raw)
    assert torch.equal(lp, lp2) and all(torch.equal(fused[k], again[k]) for k in fused), "the fused path is not deterministic"
    monkeypatch.setattr(ops, "CTX_TRAINING", False)        # NFA_K27=0: the eager modules
    before = len(calls)
    lp_e, eager = loss_and_grads(flow, x, raw)
    assert len(calls) == before
    bad = []
    for k, got, ref, tr in [("log_prob", lp, lp_e, lp64)] + [(k, fused[k], eager[k], truth[k]) for k in sorted(truth)]:
        ef, ee = rel_err(got, tr), rel_err(ref, tr)
        print("%-60s fused %.3g  eager %.3g" % (k, ef, ee))
        if not ef <= cc.PARITY * ee:
            bad.append("%s: fused %.3g > %g x eager %.3g" % (k, ef, cc.PARITY, ee))
    assert not bad, "; ".join(bad)


def test_graphed_train_step_with_a_context(monkeypatch):
    """three replays of one captured step (Adam, capturable) on fresh inputs and contexts = three eager steps from the same
    start, the parameters within PARITY x the error the eager-module steps have against float64 steps"""
    from nflows_amd.graphs import GraphedTrainStep
    from nflows_amd import ops
    flow, D, C_raw = spline_flow()
    flow = sharpen(flow).to(DEV)
    gen = torch.Generator().manual_seed(6)
    xs = [torch.randn(256, D, generator=gen).to(DEV) for _ in range(4)]
    cs = [torch.randn(256, C_raw, generator=gen).to(DEV) for _ in range(4)]

    def steps(f, dtype, graphed):
        f = copy.deepcopy(f).to(dtype)
        opt = torch.optim.Adam(f.parameters(), lr=1e-3, capturable=True)
        if graphed:
            # (the warm-up's real steps run on a throw-away copy of the start: the captured step begins where the others do)
            start = copy.deepcopy(f.state_dict())
            step = GraphedTrainStep(f, opt, xs[3], example_context=cs[3], warmup=1)
            f.load_state_dict(start)
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
            for x, c in zip(xs[:3], cs[:3]):
                step(x, c)
        else:
            for x, c in zip(xs[:3], cs[:3]):
                opt.zero_grad(set_to_none=True)
                (-f.log_prob(x.to(dtype), context=c.to(dtype)).mean()).backward()
                opt.step()
        torch.cuda.synchronize()
        return dict((n, p.detach().clone()) for n, p in f.named_parameters())

    with eager_conditioners():
        truth = steps(flow, torch.float64, False)
    calls = count_calls(monkeypatch)
    graphed = steps(flow, torch.float32, True)
    assert calls, "the captured step did not reach nfa_resnet_hidden_forward_ctx_f32"
    fused = steps(flow, torch.float32, False)
    monkeypatch.setattr(ops, "CTX_TRAINING", False)
    eager = steps(flow, torch.float32, False)
    bad = []
    for k in sorted(truth):
        eg, ef, ee = rel_err(graphed[k], truth[k]), rel_err(fused[k], truth[k]), rel_err(eager[k], truth[k])
        print("%-60s replayed %.3g  fused %.3g  eager %.3g" % (k, eg, ef, ee))
        if not (eg <= cc.PARITY * ee and ef <= cc.PARITY * ee):
            bad.append("%s: replayed %.3g / fused %.3g > %g x eager %.3g" % (k, eg, ef, cc.PARITY, ee))
    assert not bad, "; ".join(bad)
