"""Sampling from conditional autoregressive spline layers in one persistent kernel per layer (K28, csrc/made_inverse.hip).

`MaskedPiecewiseRationalQuadraticAutoregressiveTransform.inverse` kept the column-wise host loop wherever K12 does not
serve -- a context, bin counts other than 8 and 10, a step block that does not fit the LDS twice.  K28 is the RQ element in
K23's loop.  Here, under the project's parity rule (tests/maf_inverse_cases.assert_parity: against the float64 restatement
on the device, mean and 99.9 % quantile of the error at most 2 x the fp32 restatement's, at most three elements above 4 x
its maximum, everything finite) unless "bit for bit" is stated; tests/test_ar_spline_sample_host.py runs every case with
an fp32 stand-in first."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import ar_spline_sample_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = torch.nn.functional
LABEL = "made_inverse_kernel<element=rqs"


def AR():
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform
    return MaskedPiecewiseRationalQuadraticAutoregressiveTransform


@contextlib.contextmanager
def switch(value):
    saved = AR().__dict__.get("fuse_sequential_inverse_ctx")
    AR().fuse_sequential_inverse_ctx = value
    try:
        yield
    finally:
        AR().fuse_sequential_inverse_ctx = saved


LABELS = []   # `ops.last_layer_kernel()` right behind every K28 launch of the last `count` (the tail's kernel follows it)


def count(fn):
    """(launches of K28's wrapper that were served, result of `fn` under no-grad)"""
    from nflows_amd import ops
    kernel, n = ops.made_rqs_inverse_ctx, [0]
    del LABELS[:]

    def counted(*args, **kw):
        r = kernel(*args, **kw)
        n[0] += r is not None
        if r is not None:
            LABELS.append(ops.last_layer_kernel())
        return r
    ops.made_rqs_inverse_ctx = counted
    try:
        with torch.no_grad():
            result = fn()
    finally:
        ops.made_rqs_inverse_ctx = kernel
    return n[0], result


def another_label():
    """`ops.last_layer_kernel()` keeps the last layer kernel's name: a layer K12 serves (and its tail) puts another name
    there, so that a test can tell whether the call that follows launched K28."""
    from nflows_amd import ops
    torch.manual_seed(1)
    with torch.no_grad():
        AR()(features=20, hidden_features=30, num_bins=10, tails="linear", tail_bound=3.0).to(DEV).eval().inverse(
            torch.randn(32, 20, device=DEV))
    assert ops.last_layer_kernel() and not ops.last_layer_kernel().startswith(LABEL), ops.last_layer_kernel()


def check_against_restatement(flow_cpu, z, context, got_x, got_lad, what):
    o = S.inverse_pair(flow_cpu, z, context, fp64_device=DEV)
    S.assert_parity(got_x.cpu().numpy(), o["x32"], o["x64"], what + " x")
    S.assert_parity(got_lad.cpu().numpy(), o["lad32"], o["lad64"], what + " logabsdet")
    return o


def _dev(t):
    return None if t is None else t.to(DEV)


def _label_fields(label):
    assert label.startswith(LABEL) and label.endswith(">"), label
    return dict(f.strip().split("=") for f in label[len("made_inverse_kernel<"):-1].split(","))


def run_case(name, make_input=None):
    """The case's flow through `flow._transform.inverse` on the device: one K28 launch per layer, the label, a clean
    status word, parity.  Returns (flow on the device, z, context, x, logabsdet, label fields)."""
    import nflows_amd
    from nflows_amd import ops
    cfg = S.CASES[name]
    flow_cpu = S.build(name)
    z, context = S.inputs(name)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    zd, cd = _dev(z), _dev(context)
    if make_input is not None:
        zd = make_input(zd)
    launches, (x, lad) = count(lambda: flow._transform.inverse(zd, context=cd))
    assert launches == cfg["num_layers"] and len(set(LABELS)) == 1, (name, launches, LABELS, ops.last_layer_kernel())
    label = LABELS[0]
    fields = _label_fields(label)
    assert fields["element"] == "rqs" and int(fields["K"]) == cfg["num_bins"], label
    assert int(fields["context"]) == int(cfg["context_features"] is not None), label
    nflows_amd.check_status()
    assert x.shape == z.shape and lad.shape == (z.shape[0],)
    check_against_restatement(flow_cpu, z, context, x, lad, name)
    return flow, zd, cd, x, lad, fields


@pytest.mark.parametrize("name", list(S.FIXTURE) + ["k2_ctx", "k3_ctx", "k5_ctx", "k16_ctx"])
def test_flow_inverse_is_one_launch_per_layer(name):
    from nflows_amd import ops
    flow, zd, cd, x, lad, fields = run_case(name)
    assert (int(fields["continuation_blocks"]) != 0) == (name == "d6_h128_k5"), fields
    cfg = S.CASES[name]
    assert int(fields["group"]) == int(cfg["hidden_features"] >= 5 * (cfg["features"] - 1)), fields
    another_label()
    with switch(False):
        launches, (x0, lad0) = count(lambda: flow._transform.inverse(zd, context=cd))
    assert launches == 0 and not LABELS and not ops.last_layer_kernel().startswith(LABEL)
    assert torch.isfinite(x0).all() and torch.isfinite(lad0).all()


@pytest.mark.parametrize("name", list(S.FIXTURE))
def test_the_real_reference_fixture(golden_dir, name):
    g = S.load(golden_dir)
    flow = S.build(name, g).to(DEV)
    z = torch.from_numpy(g[name + "/z"]).to(DEV)
    context = torch.from_numpy(g[name + "/context"]).to(DEV) if name + "/context" in g.files else None
    launches, (x, lad) = count(lambda: flow._transform.inverse(z, context=context))
    assert launches == S.FIXTURE[name]["num_layers"]
    S.assert_parity(x.cpu().numpy(), g[name + "/x"], g[name + "/x64"], name + " fixture x")
    S.assert_parity(lad.cpu().numpy(), g[name + "/lad"], g[name + "/lad64"], name + " fixture logabsdet")


@pytest.mark.parametrize("name", ["d8_h32_c5_k10", "d6_h128_k5"])
def test_sampling_agrees_with_the_host_loop(name):
    """Flow.sample draws the same noise with the switch on and off; both are held against the float64 restatement of the
    inverse on that noise."""
    cfg = S.CASES[name]
    flow_cpu = S.build(name)
    flow = copy.deepcopy(flow_cpu).to(DEV)
    ce, D = cfg["context_features"], cfg["features"]
    context = None if ce is None else torch.randn(8, ce, generator=torch.Generator().manual_seed(5)).to(DEV)
    num = 1024 if ce is None else 128

    def draw():
        torch.manual_seed(3)
        return flow.sample(num, context=context)
    launches, on = count(draw)
    assert launches == cfg["num_layers"]
    with switch(False):
        launches, off = count(draw)
        assert launches == 0
    with torch.no_grad():
        torch.manual_seed(3)
        noise = flow._noise(num, context, False).reshape(-1, D)
        rows_ctx = None if ce is None else torch.repeat_interleave(context, num, dim=0)
        f64 = copy.deepcopy(flow_cpu).double().to(DEV)
        truth = S.restated_inverse(f64, noise.double(), None if ce is None else rows_ctx.double())[0]
    S.assert_parity(on.reshape(-1, D).cpu().numpy(), off.reshape(-1, D).cpu().numpy(), truth.cpu().numpy(), name + " sample")


def _ops_call(layer, z, context=None, block_cap=None, fn="made_rqs_inverse_ctx"):
    """K28 (or K12) at the ops level on a device layer: (x, lad, hidden, T)"""
    from nflows_amd import ops
    net, K = layer.autoregressive_net, layer.num_bins
    H, D = net.initial_layer.weight.shape
    T = min(D, S.sequential_steps(net))
    spec = ops.make_rqs_spec(K, "linear", tail_bound=layer.tail_bound)
    with torch.no_grad():
        if fn == "made_rqs_inverse":
            r = ops.made_rqs_inverse(z, ops.pack_made_schedule(net, T, 3 * K - 1), H, T, spec)
        else:
            cap = ops.made_block_cap(T, H, len(ops._made_linears(net)), len(ops.made_context_layers(net)))
            schedule = ops.pack_made_schedule(net, T, 3 * K - 1, block_cap=cap if block_cap is None else block_cap, context=True)
            packed = ops.pack_made_context(net)
            terms = None if packed is None else ops.made_context_terms(context, packed)
            r = ops.made_rqs_inverse_ctx(z, schedule, H, T, spec, terms)
    assert r is not None
    return r[0], r[1], r[2], T


def test_tied_to_k12_bit_for_bit():
    """A shape K12 serves, through both ops functions on the same inputs: the same features and hidden vector; the
    logabsdet differs by the rounding of K12's sequential fp32 sum, at most (T - 1) 2^-24 sum_t |l_t| per row."""
    from nflows_amd import ops
    torch.manual_seed(20)
    layer_cpu = S.sharpen(AR()(features=20, hidden_features=30, num_bins=10, tails="linear", tail_bound=3.0).eval())
    layer = copy.deepcopy(layer_cpu).to(DEV)
    z = 1.5 * torch.randn(1024, 20, generator=torch.Generator().manual_seed(21))
    x12, lad12, h12, T = _ops_call(layer, z.to(DEV), fn="made_rqs_inverse")
    assert ops.last_layer_kernel().startswith("made_rqs_inverse_kernel<K=10")
    x28, lad28, h28, _ = _ops_call(layer, z.to(DEV))
    assert ops.last_layer_kernel().startswith(LABEL) and T == 19
    assert torch.equal(x12[:, :T], x28[:, :T]) and torch.equal(h12, h28)
    with torch.no_grad():
        l64 = S.layer_inverse(copy.deepcopy(layer_cpu).double().to(DEV), z.double().to(DEV), per_element=True)[1][:, :T]
    bound = (T - 1) * 2.0 ** -24 * l64.abs().sum(dim=1)
    assert bool(((lad12.double() - lad28.double()).abs() <= bound).all()), float(((lad12 - lad28).abs().double() - bound).max())


def test_context_wiring():
    torch.manual_seed(30)
    cond_cpu = S.sharpen(AR()(features=9, hidden_features=48, context_features=4, num_bins=5, tails="linear",
                              tail_bound=3.0).eval())
    twin_cpu = AR()(features=9, hidden_features=48, num_bins=5, tails="linear", tail_bound=3.0).eval()
    state = {k: v for k, v in cond_cpu.state_dict().items() if "context_layer" not in k}
    twin_cpu.load_state_dict(state)
    zeroed = copy.deepcopy(cond_cpu)
    with torch.no_grad():
        for k, p in zeroed.named_parameters():
            if "context_layer" in k:
                p.zero_()
    g = torch.Generator().manual_seed(31)
    z, context = (1.5 * torch.randn(1024, 9, generator=g)).to(DEV), torch.randn(1024, 4, generator=g).to(DEV)
    x0, lad0, h0, T = _ops_call(zeroed.to(DEV), z, context)
    x1, lad1, h1, _ = _ops_call(twin_cpu.to(DEV), z)
    assert torch.equal(x0[:, :T], x1[:, :T]) and torch.equal(h0, h1) and torch.equal(lad0, lad1)
    # a real context: equal z under two contexts differ, equal z under equal contexts agree bit for bit
    z2, c2 = z.clone(), context.clone()
    z2[1], z2[2], z2[3] = z2[0], z2[0], z2[0]
    c2[2] = c2[0]
    x, lad, h, _ = _ops_call(copy.deepcopy(cond_cpu).to(DEV), z2, c2)
    assert torch.equal(x[0, :T], x[2, :T]) and torch.equal(h[0], h[2]) and torch.equal(lad[0], lad[2])
    assert not torch.equal(x[0, :T], x[1, :T]) and not torch.equal(h[0], h[1]) and not torch.equal(x[1, :T], x[3, :T])


def test_continuation_blocks_give_the_same_bits():
    from nflows_amd import ops
    flow, zd, cd, x, lad, fields = run_case("d6_h128_c8")
    assert int(fields["continuation_blocks"]) != 0, fields
    layer = flow._transform._transforms[-1]
    net = layer.autoregressive_net
    cap = ops.made_block_cap(5, 128, 5, 3)
    own = _ops_call(layer, zd, cd)
    own_blocks = int(_label_fields(ops.last_layer_kernel())["continuation_blocks"])
    half = _ops_call(layer, zd, cd, block_cap=cap // 2 // 256 * 256)
    half_blocks = int(_label_fields(ops.last_layer_kernel())["continuation_blocks"])
    assert 0 < own_blocks < half_blocks
    assert all(torch.equal(a, b) for a, b in zip((own[0][:, :5], own[1], own[2]), (half[0][:, :5], half[1], half[2])))
    assert torch.equal(own[0][:, :5], x[:, :5])


@pytest.mark.parametrize("name", ["d6_h128_c8", "d21_h64_c16_k8"])
def test_groups_of_units_give_the_same_bits(monkeypatch, name):
    from nflows_amd import ops
    flow = S.build(name).to(DEV)
    z, context = S.inputs(name, 300)
    results = {}
    for value in ("1", "0"):
        monkeypatch.setenv("NFA_K23_GROUP", value)
        launches, results[value] = count(lambda: flow._transform.inverse(_dev(z), context=_dev(context)))
        assert launches == S.CASES[name]["num_layers"] and all(l.endswith("group=%s>" % value) for l in LABELS), LABELS
    assert torch.isfinite(results["1"][0]).all()
    assert torch.equal(results["1"][0], results["0"][0]) and torch.equal(results["1"][1], results["0"][1])


@pytest.fixture(scope="module")
def many_groups():
    """16 * 1024 + 5 rows under the rule; (layer, z, context, x, K28's own (x, logabsdet, hidden, T)), computed once."""
    flow, zd, cd, x, lad, _ = run_case("d17_h64_batches")
    assert zd.shape[0] == S.MANY_ROWS
    layer = flow._transform._transforms[-1]
    return layer, zd, cd, x, _ops_call(layer, zd, cd)


@pytest.mark.parametrize("rows", [1, 15, 16, 17, S.MANY_ROWS])
def test_batch_edges(many_groups, rows):
    """Sixteen samples per workgroup: a lone row, one short of a group, a full group, one more.  Samples do not meet, so a
    short batch gives the long batch's rows bit for bit -- at both ends of it, where the ragged group is: the kernel's
    T = 16 columns, its logabsdet and its hidden vector.  (The last column is the untouched tail code's: a library GEMM
    whose summation order may follow the batch size.)"""
    layer, z, context, x, (kx, klad, khidden, T) = many_groups
    assert T == 16 and torch.equal(kx[:, :T], x[:, :T])
    for part in (slice(0, rows), slice(z.shape[0] - rows, z.shape[0])):
        launches, (px, plad) = count(lambda: layer.inverse(z[part], context=context[part]))
        assert launches == 1 and px.shape == (rows, 17) and plad.shape == (rows,)
        assert torch.equal(px[:, :T], x[part][:, :T]) and torch.isfinite(px).all() and torch.isfinite(plad).all()
        ox, olad, ohidden, _ = _ops_call(layer, z[part], context[part])
        assert torch.equal(ox[:, :T], kx[part][:, :T]) and torch.equal(olad, klad[part]) and torch.equal(ohidden, khidden[part])


@pytest.mark.parametrize("name", ["d2", "d3_h4", "h50", "d65_h128", "ff_random_masks", "d64_h48_tail", "one_block",
                                  "three_blocks"])
def test_shape_edges(name):
    flow, zd, cd, x, lad, fields = run_case(name)
    if name == "d64_h48_tail":   # K28 fills T = 48 columns, the untouched tail code the rest
        assert flow._transform._transforms[-1]._sequential_steps() == 48


def test_a_non_contiguous_input():
    def strided(z):
        wide = torch.zeros(z.shape[0], 2 * z.shape[1], device=z.device)
        wide[:, ::2] = z
        view = wide[:, ::2]
        assert not view.is_contiguous()
        return view
    run_case("d10_h32", make_input=strided)


def test_a_nan_stays_in_its_row_and_behind_its_column():
    import nflows_amd
    flow, z, context, clean_x, clean_lad, _ = run_case("d10_h32")
    layer = flow._transform._transforms[-1]
    r, j = 37, 4
    with torch.no_grad():
        dirty = z.clone()
        dirty[r, j] = float("nan")
        launches, (x, lad) = count(lambda: layer.inverse(dirty, context=context))
    assert launches == 1
    try:   # (a NaN may raise the sticky negative-discriminant bit: read and clear it, the next test starts clean)
        nflows_amd.check_status()
    except AssertionError:
        pass
    others = [i for i in range(z.shape[0]) if i != r]
    assert torch.equal(x[others], clean_x[others]) and torch.equal(lad[others], clean_lad[others])
    assert torch.equal(x[r, :j], clean_x[r, :j]) and bool(torch.isnan(x[r, j]))


def test_round_trip():
    """forward(inverse(z)) against z: no worse than 2 x the host loop's plus 1e-5."""
    flow, z, context, x, _, _ = run_case("d10_h32")
    layer = flow._transform._transforms[-1]
    with torch.no_grad():
        back_on = layer(x, context=context)[0]
        with switch(False):
            launches, (x_off, _) = count(lambda: layer.inverse(z, context=context))
            assert launches == 0
        back_off = layer(x_off, context=context)[0]
    assert float((back_on - z).abs().max()) <= 2.0 * float((back_off - z).abs().max()) + 1e-5


def test_packed_plan_follows_the_parameters_and_the_masks():
    kw = dict(features=12, hidden_features=48, num_bins=6, tails="linear", tail_bound=3.0, use_residual_blocks=False,
              random_mask=True)

    def build(seed):
        torch.manual_seed(seed)
        return S.sharpen(AR()(**kw).eval())
    layer = build(60).to(DEV)
    z = torch.randn(64, 12, device=DEV, generator=torch.Generator(DEV).manual_seed(1))

    def now(t=None):
        n, out = count(lambda: (layer if t is None else t).inverse(z))
        assert n == 1
        return out

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    first = now()
    assert same(first, now(copy.deepcopy(layer)))
    with torch.no_grad():
        for p in layer.autoregressive_net.final_layer.parameters():
            p.mul_(2)
    doubled = now()
    assert same(doubled, now(copy.deepcopy(layer))) and not same(doubled, first)
    with torch.no_grad():
        for p in layer.autoregressive_net.final_layer.parameters():
            p.data.mul_(0.5)
    halved = now()
    assert same(halved, now(copy.deepcopy(layer))) and same(halved, first)
    other = build(61)
    masks = [k for k in other.state_dict() if k.endswith(".mask")]
    assert any(not torch.equal(other.state_dict()[k], layer.state_dict()[k].cpu()) for k in masks)
    layer.load_state_dict(other.state_dict())
    loaded = now()
    assert same(loaded, now(other.to(DEV))) and not same(loaded, halved)


def _fallback_cases():
    class Mine(AR()):
        def _elementwise_inverse(self, inputs, params):
            return super()._elementwise_inverse(inputs, params)
    plain = dict(features=6, hidden_features=32, num_bins=5, tails="linear", tail_bound=3.0)
    # name -> (class, constructor arguments, grad enabled, input shape or None, dtype, context width or None, train mode)
    return {
        "grad enabled": (AR(), plain, True, None, torch.float32, None, False),
        "tanh": (AR(), dict(plain, activation=torch.tanh), False, None, torch.float32, None, False),
        "batch norm inside": (AR(), dict(plain, use_batch_norm=True), False, None, torch.float32, None, False),
        "active dropout": (AR(), dict(plain, dropout_probability=0.2), False, None, torch.float32, None, True),
        "tails=None": (AR(), dict(plain, tails=None, tail_bound=1.0), False, None, torch.float32, None, False),
        "17 bins": (AR(), dict(plain, num_bins=17), False, None, torch.float32, None, False),
        "a subclass's _elementwise_inverse": (Mine, plain, False, None, torch.float32, None, False),
        "a 3-D input": (AR(), plain, False, (48, 2, 3), torch.float32, None, False),
        "a float64 layer": (AR(), plain, False, None, torch.float64, None, False),
        "a context of the wrong width": (AR(), dict(plain, context_features=4), False, None, torch.float32, 3, False),
        "few features, many rows": (AR(), plain, False, (AR()._SEQUENTIAL_CTX_ROW_LIMIT[1] + 1, 6), torch.float32, None, False),
    }


@pytest.mark.parametrize("why", ["grad enabled", "tanh", "batch norm inside", "active dropout", "tails=None", "17 bins",
                                 "a subclass's _elementwise_inverse", "a 3-D input", "a float64 layer",
                                 "a context of the wrong width", "few features, many rows"])
def test_layers_outside_the_family_take_the_host_loop(why):
    """Zero K28 launches, and what the layer did before: the result (or the exception) of the switch-off path."""
    from nflows_amd import ops
    cls, kw, grad, shape, dtype, context_width, train = _fallback_cases()[why]
    torch.manual_seed(9)
    layer = cls(**kw).to(DEV).to(dtype)
    layer.train(train)
    g = torch.Generator().manual_seed(10)
    z = torch.rand(*(shape or (48, kw["features"])), generator=g).to(dtype).to(DEV)   # (inside [0, 1]: tails=None has no outside)
    context = None if context_width is None else torch.randn(48, context_width, generator=g).to(DEV)

    def run():
        torch.manual_seed(11)   # (an active dropout draws the same masks in both runs)
        with torch.set_grad_enabled(grad):
            try:
                x, lad = layer.inverse(z, context=context)
            except Exception as e:   # noqa: BLE001  (the host loop's own refusal of such a call, whatever it is)
                return type(e).__name__, None
        return x.detach(), lad.detach()
    another_label()
    launches, got = count(run)
    assert launches == 0 and not LABELS and not (ops.last_layer_kernel() or "").startswith(LABEL), (why, launches)
    with switch(False):
        _, want = count(run)
    if want[1] is None:
        assert got == want, (why, got, want)
    else:
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), why
