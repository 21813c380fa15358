"""K14 (nfa_pack_resnet_hidden_train_f32 / nfa_pack_made_train_f32, nfa_resnet_hidden_forward_f32,
nfa_resnet_hidden_backward_f32, nfa_resnet_backward_f32) and K10 (nfa_linear_wgrad_f32 / _batched_f32) under the
per-element rule of tests/train_kernel_cases.py: every array the kernels write against float64, element by element, under
an allowance built from that element's own conditioning -- the mean, the 99.9 % quantile and the maximum of the ratio per
case and array under caps taken from two CPU yardsticks; elements without an allowance exactly zero.  Beyond the table:
LATER PASSES of K14's persistent loops (more row blocks than workgroups: the weight ring carries on from the slot the
previous row block left), K10's slice lengths (read from the device), and the pairing of saved / grads planes in the
autograd wiring.  Run with `-m gpu`; -s prints every figure.

What the table found on its first run (tests/train_kernel_cases.py CHANGED): the forward kernel summed
a block's second Linear into the residual stream's accumulator -- `hidden` and saved{2k} of later blocks at up to 2.7 x their
caps in all 24 cases with a block and in six second-pass shapes; fixed in resnet_train.hip, and these tests pin it --; and two
honest properties of the arithmetic in elements of one or a few terms, for which the MADE cases were re-seeded and the
one-column case made exact."""
import numpy as np
import pytest
import torch

import train_kernel_cases as tk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(t):
    return (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- K14
def k14_on_device(case, net, x, g):
    """The packer, the forward kernel and the backward kernel of a case on (x, g): {array: device tensor} of everything
    they write, saved / grads as planes.  `saved` goes to the backward kernel exactly as the forward call returned it."""
    from nflows_amd import ops
    nb, di, out = case.nb, case.di, case.out
    blocks = [tuple(dev(t) for t in b) for b in net["blocks"]]
    final = None if net["final"] is None else tuple(dev(t) for t in net["final"])
    if net["masks"] is not None:
        fw, fb, bw, fbias = ops.pack_made_train(dev(net["w_in"]), dev(net["b_in"]), blocks, final, [dev(m) for m in net["masks"]])
    else:
        fw, fb, bw, fbias = ops.pack_resnet_hidden_train(dev(net["w_in"]), dev(net["b_in"]), blocks, final)
    xd, gd = dev(tk.padded(host(x), di)), dev(tk.padded(host(g), out or 128))
    hidden, saved, params = ops.resnet_hidden_forward(xd, fw, fb, nb, fbias, out)
    arrays = {"hidden": hidden}
    if final is not None:
        arrays["params"] = params
        gx, grads, arrays["grad_hidden"] = ops.resnet_backward(gd, bw, saved, di)
    else:
        assert params is None
        gx, grads = ops.resnet_hidden_backward(gd, bw, saved, di)
    arrays["grad_inputs"] = gx
    for j in range(2 * nb):
        arrays["saved%d" % j], arrays["grads%d" % j] = saved[j], grads[j]
    torch.cuda.synchronize()
    return arrays


def k14_truth_for(e, xp, gp, arrays, nb, forward=None):
    """float64 truth and allowance of every array, the backward pass through the masks the forward KERNEL produced"""
    fwd = forward if forward is not None else tk.k14_forward_truth(e, xp)[0]
    masks = [host(arrays["saved%d" % j]) > 0.0 for j in range(2 * nb)]
    truth = dict(fwd)
    truth.update(tk.k14_backward_truth(e, gp, masks))
    return truth


@pytest.mark.parametrize("name", [c.name for c in tk.K14_CASES])
def test_k14_table(name):
    p = tk.k14_prepared(name)
    case = p["case"]
    arrays = k14_on_device(case, p["net"], p["x"], p["g"])
    forward = dict((k, v) for k, v in p["truth"].items() if k in tk.forward_arrays(case.nb, bool(case.out)))
    truth = k14_truth_for(p["e"], p["xp"], p["gp"], arrays, case.nb, forward)
    assert sorted(truth) == sorted(arrays)
    stats = tk.stats_of(dict((k, host(v)) for k, v in arrays.items()), truth, name)
    tk.assert_within_caps(name, stats, tk.CAPS[name], verbose=True)


# Shapes (d_i, blocks, out or 0) of the later-pass tests.  Stages per row block: forward init_ks + 16 nb + 2 ceil(out / 32),
# backward 16 nb + 2 ceil(d_i / 32) (+ ceil(out / 16) with the final Linear: it starts at `final_first` and wraps through
# stage 0).  The stream is started once per workgroup, so a second row block begins at ring slot (stages mod 3).
PASS_SHAPES = [(32, 1, 0), (32, 0, 32), (16, 3, 0), (64, 2, 40), (36, 1, 368), (32, 2, 0), (32, 1, 24)]


def stream_stages(di, nb, out):
    fwd = (4 if di > 32 else 2) + 16 * nb + 2 * ((out + 31) // 32)
    bwd = 16 * nb + 2 * ((di + 31) // 32) + (out + 15) // 16
    return fwd, bwd


def test_the_later_pass_shapes_start_in_every_ring_slot():
    residues = {"forward": set(), "backward": set(), "backward_final": set()}
    for di, nb, out in PASS_SHAPES:
        fwd, bwd = stream_stages(di, nb, out)
        residues["forward"].add(fwd % 3)
        residues["backward_final" if out else "backward"].add(bwd % 3)
    assert all(r == {0, 1, 2} for r in residues.values()), residues


def later_pass_run(di, nb, out):
    """128 (2 CU + 5) rows on the grid's 2 CU workgroups: five workgroups walk a second row block"""
    CU = torch.cuda.get_device_properties(0).multi_processor_count
    first, B_big = 256 * CU, 128 * (2 * CU + 5)
    assert B_big // 128 > 2 * CU                    # more row blocks than the grid min(B / 128, 2 CU) has workgroups
    name = "later_pass_di%d_nb%d_out%d" % (di, nb, out)
    case = tk.K14Case(name, B_big, di, nb, 128, out, "plain", 0, 14500 + di + 7 * nb + out)
    net = tk.k14_net(case)
    x, g = tk.k14_data(case)
    return case, net, x, g, first, k14_on_device(case, net, x, g)


@pytest.mark.parametrize("di,nb,out", PASS_SHAPES)
def test_k14_later_passes_are_bit_equal_to_first_passes(di, nb, out):
    """Rows of the first pass and rows of the second are bit-equal to launches on those rows alone (one pass each: a
    row's arithmetic depends on the row and the weights only) -- all six arrays."""
    case, net, x, g, first, whole = later_pass_run(di, nb, out)
    for lo, hi in ((0, first), (first, case.B)):
        part = k14_on_device(case._replace(B=hi - lo), net, x[lo:hi], g[lo:hi])
        for k in sorted(whole):
            assert torch.equal(whole[k][lo:hi], part[k]), "%s: %s of rows %d .. %d differs from a launch on those rows alone" % (
                case.name, k, lo, hi)


@pytest.mark.parametrize("di,nb,out", PASS_SHAPES)
def test_k14_later_pass_rows_against_float64(di, nb, out):
    """The second pass's 640 rows under the table rule, caps from the two yardsticks on these rows: a later pass is held
    to float64 and not only to itself."""
    case, net, x, g, first, whole = later_pass_run(di, nb, out)
    e = tk.effective(net, di, out)
    xp, gp = tk.padded(host(x[first:]), di), tk.padded(host(g[first:]), out or 128)
    own, masks64 = tk.k14_forward_truth(e, xp)
    own = dict(own)
    own.update(tk.k14_backward_truth(e, gp, masks64))
    caps = tk.caps_from(*(tk.stats_of(tk.k14_chain(e, xp, gp, masks64, lin), own, case.name) for lin in (tk.linear_ref, tk.linear_seq)))
    tail = dict((k, v[first:]) for k, v in whole.items())
    truth = k14_truth_for(e, xp, gp, tail, nb)
    tk.assert_within_caps(case.name, tk.stats_of(dict((k, host(v)) for k, v in tail.items()), truth, case.name), caps, verbose=True)


# ---------------------------------------------------------------------------------------------------------------- K10
def k10_on_device(problems, need_bias, batched):
    from nflows_amd import ops
    on = [(dev(x), dev(gy)) for x, gy in problems]
    got = ops.linear_wgrad_batched(on, need_bias=need_bias) if batched else [ops.linear_wgrad(x, gy, need_bias=need_bias) for x, gy in on]
    assert got is not None and all(g is not None for g in got)
    torch.cuda.synchronize()
    out = {"gw": np.stack([host(gw) for gw, _ in got])}
    if need_bias:
        out["gb"] = np.stack([host(gb) for _, gb in got])
    else:
        assert all(gb is None for _, gb in got)
    return out


@pytest.mark.parametrize("name", [c.name for c in tk.K10_CASES])
def test_k10_table(name):
    """every case through nfa_linear_wgrad_f32 (problem by problem) and through nfa_linear_wgrad_batched_f32 (one launch)"""
    p = tk.k10_prepared(name)
    case = p["case"]
    for batched in (False, True):
        got = k10_on_device(p["problems"], case.need_bias, batched)
        what = name + (" batched" if batched else " single")
        tk.assert_within_caps(what, tk.stats_of(got, p["truth"], what), tk.CAPS[name], verbose=True)


def k10_plan(count, B, I, O):
    """(ksplit, rows per stage) of a launch: ksplit from the workspace size, bytes / (count (O I + O) 4); a stage has 16 rows
    where four or more 128 x 128 result blocks share the launch, 32 otherwise (linear_wgrad.hip: wgrad_rows)"""
    from nflows_amd import _native as N
    ksplit = N.load().nfa_linear_wgrad_batched_workspace_bytes(count, B, I, O) // (count * (O * I + O) * 4)
    blocks = -(-O // 128) * -(-I // (32 if I <= 32 else 128))
    return int(ksplit), 16 if I > 32 and blocks * count >= 4 else 32


# (count, I, O, stages per slice -- 2.5: uneven slices of two and three stages).  Three stages wrap the ring exactly once.
SLICES = [(1, 36, 8, 1), (1, 36, 8, 2), (1, 36, 8, 3), (1, 36, 8, 4), (1, 36, 8, 7), (1, 36, 8, 2.5), (1, 32, 8, 3), (4, 128, 128, 3)]


@pytest.mark.parametrize("count,I,O,per_slice", SLICES)
def test_k10_slice_lengths(count, I, O, per_slice):
    """Batches chosen at run time so that every batch slice of the partial kernel holds the wanted number of stages; the
    slice lengths asserted from the plan the library reports, then the table rule with caps from this case's own yardsticks."""
    ksplit1, rows = k10_plan(count, 1 << 20, I, O)      # (a batch with more stages than slices: the chip's share per problem)
    B = int(rows * ksplit1 * per_slice)
    ksplit, _ = k10_plan(count, B, I, O)
    stages = B // rows
    lengths = sorted(set(stages * (k + 1) // ksplit - stages * k // ksplit for k in range(ksplit)))
    assert ksplit == ksplit1 and lengths == ([2, 3] if per_slice == 2.5 else [per_slice]), (ksplit, ksplit1, lengths)
    name = "slices_%dx_i%d_o%d_%s_stages" % (count, I, O, per_slice)
    problems = tk.k10_data(tk.K10Case(name, B, I, O, count, "relu_x", True, 10500 + int(10 * per_slice)))
    truth, caps = tk.k10_runtime_caps(problems, True, name)
    got = k10_on_device(problems, True, batched=count > 1)
    print("%s: B = %d, %d slices of %s stages of %d rows" % (name, B, ksplit, lengths, rows))
    tk.assert_within_caps(name, tk.stats_of(got, truth, name), caps, verbose=True)


# ------------------------------------------------------------------------------------------------------ autograd wiring
def _linears(net):
    return [net.initial_layer] + [l for b in net.blocks for l in b.linear_layers] + [net.final_layer]


@pytest.mark.parametrize("kind,di,nb,H,out", [("resnet", 32, 2, 128, 40), ("resnet", 32, 3, 128, 736), ("made", 21, 2, 64, 42)])
def test_autograd_wiring_pairs_the_planes(kind, di, nb, H, out, monkeypatch):
    """A ResidualNet / a K25 MADE through its fused training path at 256 rows: every parameter gradient under the K10 rule,
    the truth being the float64 product of the arrays the kernels themselves produce in a manual call of the same ops
    (deterministic kernels: the arrays autograd used) -- a saved plane paired with the wrong grads plane shows per element.
    Masked-out weights get exactly zero."""
    from nflows_amd import ops
    B = 256
    torch.manual_seed(di + nb + out)
    if kind == "made":
        from nflows_amd.transforms.made import MADE
        net = MADE(di, H, num_blocks=nb, output_multiplier=2).to(DEV)
        monkeypatch.setattr(MADE, "fuse_training", True)
    else:
        from nflows_amd.nn.nets import ResidualNet
        net = ResidualNet(di, out, H, num_blocks=nb).to(DEV)
        monkeypatch.setattr(ResidualNet, "fuse_training", True)
    with torch.no_grad():
        for b in net.blocks:
            b.linear_layers[1].weight.mul_(60.0)
            b.linear_layers[1].bias.mul_(60.0)
    calls = []
    real = ops.resnet_hidden_forward
    monkeypatch.setattr(ops, "resnet_hidden_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = torch.randn(B, di, device=DEV)
    w = torch.randn(B, out, device=DEV)
    (net(x) * w).sum().backward()
    assert len(calls) == 1, "the net did not take its fused training path"
    lins = _linears(net)
    masks = [getattr(l, "mask", None) for l in lins]
    # the same ops by hand
    di4, out4 = (di + 3) // 4 * 4, (out + 3) // 4 * 4
    with torch.no_grad():
        blocks = [(b.linear_layers[0].weight, b.linear_layers[0].bias, b.linear_layers[1].weight, b.linear_layers[1].bias) for b in net.blocks]
        final = (net.final_layer.weight, net.final_layer.bias)
        if kind == "made":
            fw, fb, bw, fbias = ops.pack_made_train(net.initial_layer.weight, net.initial_layer.bias, blocks, final, masks)
        else:
            fw, fb, bw, fbias = ops.pack_resnet_hidden_train(net.initial_layer.weight, net.initial_layer.bias, blocks, final)
        xp = torch.nn.functional.pad(x, (0, di4 - di)).contiguous()
        gp = torch.nn.functional.pad(w, (0, out4 - out)).contiguous()
        hidden, saved, _ = real(xp, fw, fb, nb, fbias, out4)
        _, grads, g_hidden = ops.resnet_backward(gp, bw, saved, di4)
    pairs = [(xp, grads[0] if nb else g_hidden)]
    for k in range(nb):
        pairs += [(saved[2 * k], grads[2 * k + 1]), (saved[2 * k + 1], grads[2 * k + 2] if k + 1 < nb else g_hidden)]
    pairs.append((hidden, gp))
    for q, (lin, (inp, g_o)) in enumerate(zip(lins, pairs)):
        rows, cols = lin.weight.shape
        what = "%s %d blocks out %d, Linear %d" % (kind, nb, out, q)
        # autograd through mask * weight gives the gradient times the mask, exactly; the net's own extent of the padded arrays
        m = np.ones((rows, cols)) if masks[q] is None else host(masks[q]).astype(np.float64)
        assert masks[q] is None or (m == 0).any()
        cut = lambda a: {"gw": a["gw"][:, :rows, :cols] * m, "gb": a["gb"][:, :rows]}      # noqa: E731
        full = tk.k10_truth([(inp, g_o)])
        truth = dict((k, (cut(dict((n, v[0]) for n, v in full.items()))[k], cut(dict((n, v[1]) for n, v in full.items()))[k])) for k in full)
        caps = tk.caps_from(*(tk.stats_of(cut(tk.k10_apply([(inp, g_o)], wgrad)), truth, what) for wgrad in (tk.wgrad_ref, tk.wgrad_seq)))
        got = {"gw": host(lin.weight.grad)[None], "gb": host(lin.bias.grad)[None]}
        tk.assert_within_caps(what, tk.stats_of(got, truth, what), caps, verbose=True)
