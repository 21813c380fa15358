"""The density pass of autoregressive rational-quadratic spline layers in one launch (K29, csrc/made_rqs.hip).

`MaskedPiecewiseRationalQuadraticAutoregressiveTransform.forward` ran the MADE's hidden layers as stock device ops and then
K13 (8 bins) or a GEMM + K1 (any other bin count), and a stack of such layers was never a run.  K29 is the MADE and the spline
in one layer kernel, runs of layers with their permutations and the base density in one launch.  Here, under the project's
parity rule (tests/maf_inverse_cases.assert_parity: against the float64 restatement on the device, mean and 99.9 % quantile
of the error at most 2 x the fp32 CPU restatement's, at most three elements above 4 x its maximum, everything finite) unless
"bit for bit" is stated; tests/test_ar_spline_density_host.py runs every case with an fp32 stand-in first."""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch

import ar_spline_density_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional
LABEL = "made_rqs_kernel<K="


def AR():
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform
    return MaskedPiecewiseRationalQuadraticAutoregressiveTransform


@contextlib.contextmanager
def switch(value):
    saved = AR().__dict__.get("fuse_conditioner")
    AR().fuse_conditioner = value
    try:
        yield
    finally:
        AR().fuse_conditioner = saved


def mode_of(name):
    return 2 if C.CASES[name]["num_bins"] == 8 else 1


LABELS = []   # `ops.last_layer_kernel()` right behind every served K29 launch of the last `count`


def count(fn):
    """(launches of K29's wrapper that were served, result of `fn` under no-grad)"""
    from nflows_amd import ops
    kernel, n = ops.rqs_flow_made, [0]
    del LABELS[:]

    def counted(*args, **kw):
        r = kernel(*args, **kw)
        n[0] += r is not None
        if r is not None:
            LABELS.append(ops.last_layer_kernel())
        return r
    ops.rqs_flow_made = counted
    try:
        with torch.no_grad():
            result = fn()
    finally:
        ops.rqs_flow_made = kernel
    return n[0], result


def another_label():
    """`ops.last_layer_kernel()` keeps the last layer kernel's name: a K22 layer puts another name there, so that a test
    can tell whether the call that follows launched K29."""
    from nflows_amd import ops
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform
    torch.manual_seed(1)
    with torch.no_grad():
        MaskedAffineAutoregressiveTransform(features=6, hidden_features=16).to(DEV).eval()(torch.randn(32, 6, device=DEV))
    assert ops.last_layer_kernel() and not ops.last_layer_kernel().startswith(LABEL), ops.last_layer_kernel()


def _dev(t):
    return None if t is None else t.to(DEV)


def _status():
    from nflows_amd import ops
    w = ops._status_word(torch.device(DEV))
    s = int(w.item())
    w.zero_()
    return s


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(flow on the CPU, x, context, the restatement's vectors): computed once per case, shared, never written to."""
    flow_cpu = C.build(name)
    x, context = C.inputs(name)
    return flow_cpu, x, context, C.restated_pair(flow_cpu, x, context, fp64_device=DEV)


def served(name, fn, launches=1):
    """`fn()` under the case's mode: `launches` served K29 launches, every one under K29's label with the case's fields."""
    cfg = C.CASES[name]
    another_label()
    with switch(mode_of(name)):
        n, result = count(fn)
    assert n == launches and len(LABELS) == launches, (name, n, LABELS)
    for label in LABELS:
        assert label.startswith(LABEL) and label.endswith(">"), label
        fields = dict(f.strip().split("=") for f in label[len("made_rqs_kernel<"):-1].split(","))
        assert int(fields["K"]) == cfg["num_bins"] and int(fields["context"]) == int(cfg["context_features"] is not None)
        assert int(fields["resnet"]) == int(cfg.get("use_residual_blocks", True)), label
    return result


@pytest.mark.parametrize("name", list(C.CASES))
def test_parity_label_and_one_launch_per_run(name):
    """flow._transform(x) and flow.log_prob(x) are ONE launch each -- every layer, its permutation and (log_prob) the base
    density --, under K29's label, with a clean status word, within the rule on z, logabsdet and log_prob."""
    import nflows_amd
    flow_cpu, x, context, o = prepared(name)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    xd, cd = _dev(x), _dev(context)
    z, lad = served(name, lambda: flow._transform(xd, context=cd))
    lp = served(name, lambda: flow.log_prob(xd, context=cd), launches=1)
    nflows_amd.check_status()
    assert z.shape == x.shape and lad.shape == (x.shape[0],) and lp.shape == (x.shape[0],)
    C.assert_parity(z.cpu().numpy(), o["z32"], o["z64"], name + " z")
    C.assert_parity(lad.cpu().numpy(), o["lad32"], o["lad64"], name + " logabsdet")
    C.assert_parity(lp.cpu().numpy(), o["lp32"], o["lp64"], name + " log_prob")
    if C.CASES[name]["num_layers"] == 1 and not C.CASES[name].get("lu"):
        layer = C.spline_layers(flow)[0]
        z1, lad1 = served(name, lambda: layer(xd, context=cd))   # the layer on its own: a run of one
        assert torch.equal(z1, z) and torch.equal(lad1, lad)


def test_a_run_behind_another_transform_accumulates():
    """lu_in_front: the LULinear's log-determinant is in the running total the run adds to (covered by the parity above);
    here the two parts are separated: total == LULinear's own + the run's own, to fp32 rounding of the sum."""
    flow_cpu, x, context, o = prepared("lu_in_front")
    flow = copy.deepcopy(flow_cpu).to(DEV)
    xd = _dev(x)
    z, lad = served("lu_in_front", lambda: flow._transform(xd))
    layers = list(flow._transform._transforms)
    from nflows_amd.transforms import CompositeTransform
    with torch.no_grad():
        h, lad_lu = layers[0](xd)
    z_run, lad_run = served("lu_in_front", lambda: CompositeTransform(layers[1:])(h))
    assert torch.equal(z_run, z)
    want = lad_lu.double() + lad_run.double()
    assert (lad.double() - want).abs().max().item() <= 2.0 ** -22 * want.abs().max().item()


@pytest.mark.parametrize("name", list(C.FIXTURE))
def test_the_real_reference_fixture(golden_dir, name):
    g = C.load(golden_dir)
    flow = C.build(name, g).to(DEV)
    x = torch.from_numpy(g[name + "/x"]).to(DEV)
    context = torch.from_numpy(g[name + "/context"]).to(DEV) if name + "/context" in g.files else None
    z, lad = served(name, lambda: flow._transform(x, context=context))
    lp = served(name, lambda: flow.log_prob(x, context=context))
    C.assert_parity(z.cpu().numpy(), g[name + "/z"], g[name + "/z64"], name + " fixture z")
    C.assert_parity(lad.cpu().numpy(), g[name + "/lad"], g[name + "/lad64"], name + " fixture logabsdet")
    C.assert_parity(lp.cpu().numpy(), g[name + "/log_prob"], g[name + "/log_prob64"], name + " fixture log_prob")


def test_batch_edges_bit_for_bit():
    """1, 127, 128, 129 and 256 rows, and enough 128-row blocks for a second pass of the persistent loop that ends on a
    ragged block: rows evaluated alone equal, bit for bit, the same rows inside the larger batch; two calls give equal bits."""
    name = "d8_batches"
    flow = copy.deepcopy(prepared(name)[0]).to(DEV)
    layer = C.spline_layers(flow)[0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    many = cus * 128 + 128 + 5
    x, _ = C.inputs(name, rows=many)
    xd = _dev(x)
    z, lad = served(name, lambda: layer(xd))
    z2, lad2 = served(name, lambda: layer(xd))
    assert torch.equal(z, z2) and torch.equal(lad, lad2)
    lp = served(name, lambda: flow.log_prob(xd))
    o = C.restated_pair(prepared(name)[0], x[-261:], None, fp64_device=DEV)   # the second pass and the ragged block
    C.assert_parity(z[-261:].cpu().numpy(), o["z32"], o["z64"], "last rows z")
    C.assert_parity(lad[-261:].cpu().numpy(), o["lad32"], o["lad64"], "last rows logabsdet")
    for rows in (1, 127, 128, 129, 256):
        for start in (0, many - rows):
            part = xd[start:start + rows].clone()
            zp, lp_ = served(name, lambda: layer(part))
            assert torch.equal(zp, z[start:start + rows]) and torch.equal(lp_, lad[start:start + rows]), (rows, start)
            assert torch.equal(served(name, lambda: flow.log_prob(part)), lp[start:start + rows]), (rows, start)


def test_inputs_outside_the_box_on_the_knots_and_strided():
    name = "d8_batches"
    flow_cpu = prepared(name)[0]
    flow = copy.deepcopy(flow_cpu).to(DEV)
    layer = C.spline_layers(flow)[0]
    x, _ = C.inputs(name, rows=512)
    x = x.clamp(-2.9, 2.9)
    # columns 2 and 5 beyond +-tail_bound (exactly on the bound is inside), rows 7 and 300 wholly outside
    x[:, 2] = torch.where(torch.arange(512) % 2 == 0, torch.tensor(3.0000002), torch.tensor(-57.25))
    x[:, 5] = torch.tensor(3.0e30)
    x[7] = torch.linspace(3.5, 9.0, 8)
    x[300] = -torch.linspace(3.5, 9.0, 8)
    xd = _dev(x)
    z, lad = served(name, lambda: layer(xd))
    assert torch.equal(z[:, 2].view(torch.int32), xd[:, 2].view(torch.int32))
    assert torch.equal(z[:, 5].view(torch.int32), xd[:, 5].view(torch.int32))
    assert torch.equal(z[7], xd[7]) and torch.equal(z[300], xd[300])
    assert lad[7].item() == 0.0 and lad[300].item() == 0.0
    # exactly 0 from an outside column, whatever value it holds: feature j's term depends on columns <= j only, so the rows
    # cut off behind column k (every later column at 1e3, outside) sum the terms of columns <= k in the kernel's fixed
    # order.  Column k itself is outside in these rows (k = 2: 3.0000002 or -57.25, k = 5: 3e30), so that sum must equal,
    # bit for bit, the sum of the rows cut off behind column k - 1, where column k holds 1e3 instead.
    def cut(k):
        rows = xd.clone()
        rows[:, k + 1:] = 1.0e3
        z_cut, lad_cut = served(name, lambda: layer(rows))
        assert torch.equal(z_cut[:, k + 1:], rows[:, k + 1:])
        return rows, lad_cut
    for k in (2, 5):
        assert torch.equal(cut(k)[1], cut(k - 1)[1]), k
    assert torch.equal(cut(5)[1], cut(4)[1]) and not torch.equal(cut(4)[1], cut(3)[1])   # (an inside column does add)
    # ... and what the inside columns add is right: columns 0 and 1 alone inside, under the rule
    only, lad_only = cut(1)
    o = C.restated_pair(flow_cpu, only.cpu(), None, fp64_device=DEV)
    C.assert_parity(lad_only.cpu().numpy(), o["lad32"], o["lad64"], "two inside columns logabsdet")
    # inputs on every knot of feature 3: the knots of the fp64 restatement's spline for each row, rounded to fp32
    from oracle import eager   # noqa: F401  (the restatement's spline)
    net64 = copy.deepcopy(flow_cpu).double()._transform._transforms[0].autoregressive_net
    base, _ = C.inputs(name, rows=11 * 32)
    with torch.no_grad():
        import maf_cases
        K = 10
        params = maf_cases.made_forward(net64, base.double()).view(-1, 8, 3 * K - 1)[:, 3, :K]
        widths = 1e-3 + (1 - 1e-3 * K) * torch.softmax(params, dim=-1)
        knots = torch.cat((torch.zeros(len(base), 1, dtype=torch.float64), torch.cumsum(widths, -1)), dim=-1) * 6.0 - 3.0
        knots[:, -1] = 3.0
        base[:, 3] = knots[torch.arange(len(base)), torch.arange(len(base)) % 11].float()   # (feature 3 reads features 0 .. 2 only)
    zk, ladk = served(name, lambda: layer(_dev(base)))
    o = C.restated_pair(flow_cpu, base, None, fp64_device=DEV)
    C.assert_parity(zk.cpu().numpy(), o["z32"], o["z64"], "knots z")
    C.assert_parity(ladk.cpu().numpy(), o["lad32"], o["lad64"], "knots logabsdet")
    # a non-contiguous view gives the bits of its contiguous copy
    wide = torch.randn(300, 16, device=DEV) * 1.5
    view = wide[:, ::2]
    assert not view.is_contiguous()
    a, b = served(name, lambda: layer(view)), served(name, lambda: layer(view.contiguous()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ["d63_h128_k12_ff", "d8_h32_c5_k5_reverse", "d33"])
def test_folded_base_density(name):
    """log_prob (z never written) == logabsdet of the z-writing call + StandardNormal.log_prob(z), to fp32 rounding of that
    sum; with 63 features the pad column does not enter."""
    flow_cpu, x, context, _ = prepared(name)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    xd, cd = _dev(x), _dev(context)
    z, lad = served(name, lambda: flow._transform(xd, context=cd))
    lp = served(name, lambda: flow.log_prob(xd, context=cd))
    D = x.shape[1]
    base = -0.5 * (z.double() ** 2).sum(1) - 0.5 * D * np.log(2 * np.pi)
    want = base + lad.double()
    # the kernel sums z^2 in fp32 (D terms), rounds the base density and adds: a few ulps of the largest intermediate
    scale = torch.maximum(torch.maximum(base.abs(), lad.double().abs()), want.abs())
    assert ((lp.double() - want).abs() <= (D + 4) * 2.0 ** -24 * scale).all(), float((lp.double() - want).abs().max())


@pytest.mark.parametrize("K,D", [(5, 7), (10, 8), (11, 5), (12, 6), (16, 64), (8, 9)])
def test_exact_logits(K, D):
    """Zero weights, the final biases distinct dyadic logits per feature (and a divisor of 8 that is exact): every sample's
    output equals the C oracle's float32 spline on those exact logits under the exact-logit rule -- a wrong row order, a
    wrong pad row or a wrong tile of a pair shows exactly, not statistically."""
    import ar_spline_cases as A
    import exact_logits as X
    P = 3 * K - 1
    rng = np.random.RandomState(100 * K + D)
    torch.manual_seed(K)
    layer = AR()(features=D, hidden_features=64, num_bins=K, tails="linear", tail_bound=A.TAIL_BOUND).eval()
    logits = rng.randint(-24, 25, (D, P)) / 4.0
    assert len({tuple(r) for r in logits}) == D
    with torch.no_grad():
        for p in layer.parameters():
            p.zero_()
        layer.autoregressive_net.final_layer.bias.copy_(torch.from_numpy(logits.reshape(-1)))
    layer.autoregressive_net.hidden_features = 64   # sqrt(64) = 8: the width / height divisor is a power of two
    raw = np.ascontiguousarray(np.broadcast_to(logits[None], (A.EXACT_ROWS, D, P)))
    xt = X.spline_inputs(raw, K, "linear", False, seed=K + D, hidden=64, outside_rows=A.EXACT_OUTSIDE_ROWS)
    o = X.reference_order(xt, raw, K, "linear", False, hidden=64)
    layer = layer.to(DEV)
    _status()
    with switch(2):
        n, (z, lad) = count(lambda: layer(torch.from_numpy(xt).to(DEV)))
    assert n == 1 and LABELS[0].startswith(LABEL + "%d," % K)
    A.assert_exact_rule(z.cpu().numpy(), lad.cpu().numpy(), xt, o, False, _status(), "exact K29 k%d d%d" % (K, D))


def test_weight_changes_are_served_with_the_new_bits():
    """An in-place parameter change, a write through `.data`, a load_state_dict with other masks: each is served on the
    next call with the bits of a fresh copy of the module, which differ from the bits before."""
    name = "d8_batches"
    flow = copy.deepcopy(prepared(name)[0]).to(DEV)
    layer = C.spline_layers(flow)[0]
    x = _dev(C.inputs(name, rows=300)[0])
    before = served(name, lambda: layer(x))

    def fresh():
        return served(name, lambda: copy.deepcopy(layer)(x))
    net = layer.autoregressive_net
    with torch.no_grad():
        net.blocks[0].linear_layers[1].weight.mul_(1.5)
    a = served(name, lambda: layer(x))
    assert torch.equal(a[0], fresh()[0]) and torch.equal(a[1], fresh()[1]) and not torch.equal(a[0], before[0])
    net.final_layer.bias.data[5] += 0.75
    b = served(name, lambda: layer(x))
    assert torch.equal(b[0], fresh()[0]) and torch.equal(b[1], fresh()[1]) and not torch.equal(b[0], a[0])
    torch.manual_seed(5)
    other = AR()(features=8, hidden_features=32, num_bins=10, tails="linear", tail_bound=C.TAIL_BOUND, random_mask=True,
                 use_residual_blocks=False, num_blocks=2)
    plain = AR()(features=8, hidden_features=32, num_bins=10, tails="linear", tail_bound=C.TAIL_BOUND,
                 use_residual_blocks=False, num_blocks=2).to(DEV).eval()
    C.S.sharpen(other)
    with switch(1):
        _, first = count(lambda: plain(x))
    plain.load_state_dict(other.state_dict())
    with switch(1):
        n, c = count(lambda: plain(x))
        _, want = count(lambda: copy.deepcopy(other).to(DEV).eval()(x))
    assert n == 1 and torch.equal(c[0], want[0]) and torch.equal(c[1], want[1]) and not torch.equal(c[0], first[0])


def _declined(make, call=None, mode=1):
    """(result, label) of a call that K29 must not serve, and the same call with the switch at 0: equal bits."""
    from nflows_amd import ops
    layer = make()
    another_label()
    with switch(mode):
        n, got = count(lambda: call(layer))
        label = ops.last_layer_kernel()
    assert n == 0 and not LABELS and not label.startswith(LABEL), label
    with switch(0):
        _, want = count(lambda: call(layer))
    for g, w in zip(got, want):
        assert torch.equal(g.detach(), w.detach())


def test_declined_calls_keep_todays_path():
    torch.manual_seed(3)
    x = torch.randn(200, 6, device=DEV) * 1.5

    def make(**kw):
        args = dict(features=6, hidden_features=32, num_bins=10, tails="linear", tail_bound=3.0)
        args.update(kw)
        return lambda: C.S.sharpen(AR()(**args)).to(DEV).eval()
    plain = lambda layer: layer(x)   # noqa: E731
    _declined(make(activation=torch.tanh), plain)
    _declined(make(use_batch_norm=True), plain)
    unit = torch.rand(200, 6, device=DEV)
    _declined(make(tails=None, tail_bound=1.0), lambda layer: layer(unit))
    _declined(make(num_bins=17), plain)
    wide = torch.randn(130, 65, device=DEV)
    _declined(make(features=65), lambda layer: layer(wide))
    _declined(make(hidden_features=132), plain)
    _declined(make(num_bins=8), plain, mode=1)                                 # 8 bins in default mode

    class Mine(AR()):
        def _elementwise_forward(self, inputs, params):
            return super()._elementwise_forward(inputs, params)
    _declined(lambda: C.S.sharpen(Mine(6, 32, tails="linear", tail_bound=3.0)).to(DEV).eval(), plain)
    # grad enabled: the differentiable path, the label is not K29's, the bits are those of the same call with the switch at 0
    from nflows_amd import ops
    layer = make()()
    another_label()
    with switch(1):
        z, lad = layer(x)
        label = ops.last_layer_kernel()
    assert not label.startswith(LABEL) and lad.requires_grad
    with switch(0):
        z0, lad0 = layer(x)
    assert torch.equal(z.detach(), z0.detach()) and torch.equal(lad.detach(), lad0.detach())


def test_declined_shapes_and_dropout_raise_or_fall_back_as_before():
    """A context of the wrong width, a 3-D input, a float64 layer: what the call did with the switch at 0 (an exception of
    the same type, or the same bits) it does with the switch at 1; active dropout keeps the stock path."""
    from nflows_amd import ops
    torch.manual_seed(4)
    layer = C.S.sharpen(AR()(6, 32, context_features=3, num_bins=10, tails="linear", tail_bound=3.0)).to(DEV).eval()
    x = torch.randn(64, 6, device=DEV)

    def outcome(fn):
        try:
            with torch.no_grad():
                return ("ok", fn())
        except Exception as e:   # noqa: BLE001
            return (type(e).__name__, None)
    double = C.S.sharpen(AR()(6, 32, num_bins=10, tails="linear", tail_bound=3.0)).to(DEV).eval().double()
    for fn in (lambda: layer(x, context=torch.randn(64, 5, device=DEV)),
               lambda: double(x.double()),
               lambda: layer(torch.randn(4, 16, 6, device=DEV), context=torch.randn(4, 16, 3, device=DEV))):
        another_label()
        with switch(1):
            n, a = count(lambda: outcome(fn))
            assert n == 0 and not ops.last_layer_kernel().startswith(LABEL)
        with switch(0):
            b = outcome(fn)
        assert a[0] == b[0]
        if a[0] == "ok":
            assert all(torch.equal(p, q) for p, q in zip(a[1], b[1]))
    # (active dropout draws a new mask on every call: two calls cannot be compared bit for bit, with any switch -- the check
    #  is that K29's wrapper was not asked and that its label does not appear)
    dropped = AR()(6, 32, num_bins=10, tails="linear", tail_bound=3.0, dropout_probability=0.5).to(DEV).train()
    another_label()
    with switch(1):
        n, _ = count(lambda: dropped(x))
    assert n == 0 and not ops.last_layer_kernel().startswith(LABEL)


@pytest.mark.parametrize("name", list(C.CASES))
def test_inverse_is_untouched(name):
    flow_cpu, x, context, _ = prepared(name)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    z, cd = _dev(x[:130]), _dev(None if context is None else context[:130])
    with torch.no_grad():
        with switch(0):
            a = flow._transform.inverse(z, context=cd)
        with switch(2):
            n, b = count(lambda: flow._transform.inverse(z, context=cd))
    assert n == 0 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_capture_replays_the_eager_bits():
    name = "d8_h32_c5_k5_reverse"
    flow_cpu, x, context, _ = prepared(name)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    xd, cd = _dev(x[:300]).clone(), _dev(context[:300]).clone()
    eager_lp = served(name, lambda: flow.log_prob(xd, context=cd))
    eager_z, eager_lad = served(name, lambda: flow._transform(xd, context=cd))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with switch(1), torch.no_grad():
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            flow.log_prob(xd, context=cd)   # (warm-up on the side stream)
        torch.cuda.current_stream().wait_stream(stream)
        with torch.cuda.graph(graph):
            lp = flow.log_prob(xd, context=cd)
            z, lad = flow._transform(xd, context=cd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lp, eager_lp) and torch.equal(z, eager_z) and torch.equal(lad, eager_lad)
