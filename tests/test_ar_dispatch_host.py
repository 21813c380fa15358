"""CPU-only dispatch tables of the masked autoregressive layers and of the run planner above them: which launcher a call
takes -- K23 for `MaskedAffineAutoregressiveTransform.inverse`, K22 / K29 for a layer's `forward` as a run of one, the one
`ops.*_flow_*` wrapper for a composite of [Permutation, layer] x 3 -- and where a call is refused and runs layer by layer.
As tests/test_ar_spline_sample_host.py::test_which_layers_take_which_kernel does it for K28: recorders in the launchers'
place, `_OnDevice` standing in for a device tensor (the gates read nothing else of the device)."""
import pytest
import torch

from nflows_amd import configs, ops
from nflows_amd.nn.nets import MLP
from nflows_amd.transforms import (AffineCouplingTransform, CompositeTransform, MaskedAffineAutoregressiveTransform as MAF,
                                   MaskedPiecewiseRationalQuadraticAutoregressiveTransform as ARQ, RandomPermutation)
from nflows_amd.transforms.autoregressive import AutoregressiveTransform
from nflows_amd.utils.torchutils import create_alternating_binary_mask

F = torch.nn.functional
ROWS = 4


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers `is_cuda` as a device tensor would."""
    is_cuda = property(lambda self: True)


def _dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_OnDevice)


def _maf(features=8, hidden=32, ce=None, cls=MAF, **kw):
    torch.manual_seed(1)
    return cls(features=features, hidden_features=hidden, context_features=ce, **kw).eval()


def _arq(features=8, hidden=32, bins=5, ce=None, cls=ARQ, **kw):
    torch.manual_seed(1)
    kw.setdefault("tails", "linear")
    return cls(features=features, hidden_features=hidden, num_bins=bins, context_features=ce, tail_bound=3.0, **kw).eval()


@pytest.fixture
def switches(monkeypatch):
    """The class-level switches at their defaults, whatever the environment says."""
    monkeypatch.setattr(MAF, "fuse_conditioner", True)
    monkeypatch.setattr(MAF, "fuse_sequential_inverse", True)
    monkeypatch.setattr(ARQ, "fuse_conditioner", 1)
    monkeypatch.setattr(ARQ, "fuse_output_layer", True)
    monkeypatch.setattr(AffineCouplingTransform, "fuse_conditioner", True)
    return monkeypatch


# ---- K23: MaskedAffineAutoregressiveTransform.inverse --------------------------------------------------------------------------------

def _inverse_taken(monkeypatch, layer, rows=ROWS, context=None, inputs=None, grad=False):
    """"k23" / "host": what `inverse` calls, the launcher and the column-wise loop stubbed."""
    calls = []

    def k23(inputs, schedule, hidden_features, context_terms=None):
        net = layer.autoregressive_net
        assert hidden_features == net.initial_layer.weight.shape[0] and schedule[1].numel() - 2 >= layer.features + 1
        assert (context_terms is None) == (not hasattr(net, "context_layer"))
        calls.append("k23")
        return "k23"
    monkeypatch.setattr(ops, "made_affine_inverse", k23)
    monkeypatch.setattr(AutoregressiveTransform, "inverse", lambda self, inputs, context=None: calls.append("host") or "host")
    z = _dev(rows, layer.features) if inputs is None else inputs
    with torch.set_grad_enabled(grad):
        got = layer.inverse(z, context)
    assert calls == [got], (got, calls)
    return got


def test_which_inverse_calls_take_k23(switches):
    mp = switches
    assert _inverse_taken(mp, _maf()) == "k23"
    assert _inverse_taken(mp, _maf(7, 32, use_residual_blocks=False, random_mask=True)) == "k23"
    assert _inverse_taken(mp, _maf(ce=5), context=_dev(ROWS, 5)) == "k23"
    assert _inverse_taken(mp, _maf(2)) == "k23"
    # each refusal of `_inverse_kernel_net`
    assert _inverse_taken(mp, _maf(activation=torch.tanh)) == "host"
    assert _inverse_taken(mp, _maf(use_batch_norm=True)) == "host"
    assert _inverse_taken(mp, _maf(dropout_probability=0.3).train()) == "host"
    assert _inverse_taken(mp, _maf(dropout_probability=0.3)) == "k23"            # eval: the dropout is off
    assert _inverse_taken(mp, _maf(num_blocks=6)) == "host"                      # 13 Linears
    assert _inverse_taken(mp, _maf(num_blocks=5)) == "k23"                       # 11
    assert _inverse_taken(mp, _maf(1)) == "host"                                 # one feature
    swapped = _maf()
    assert _inverse_taken(mp, swapped) == "k23"
    swapped.autoregressive_net.blocks[1].activation = torch.tanh                 # read per call
    assert _inverse_taken(mp, swapped) == "host"
    swapped.autoregressive_net.blocks[1].activation = torch.relu
    assert _inverse_taken(mp, swapped) == "k23"
    # the context
    assert _inverse_taken(mp, _maf(ce=5), context=_dev(ROWS, 4)) == "host"       # of the wrong width
    assert _inverse_taken(mp, _maf(ce=5)) == "host"                              # missing
    assert _inverse_taken(mp, _maf(), context=_dev(ROWS, 3)) == "host"           # unwanted
    assert _inverse_taken(mp, _maf(ce=5), context=_dev(ROWS + 1, 5)) == "host"   # of another number of rows
    assert _inverse_taken(mp, _maf(ce=5), context=torch.zeros(ROWS, 5)) == "host"                  # not on the device
    assert _inverse_taken(mp, _maf(ce=5), context=_dev(ROWS, 5, dtype=torch.float64)) == "host"
    # the inputs
    assert _inverse_taken(mp, _maf(), inputs=torch.zeros(ROWS, 8)) == "host"
    assert _inverse_taken(mp, _maf(), inputs=_dev(ROWS, 8, dtype=torch.float64)) == "host"
    assert _inverse_taken(mp, _maf(), inputs=_dev(ROWS, 9)) == "host"
    assert _inverse_taken(mp, _maf(), inputs=_dev(0, 8)) == "host"
    assert _inverse_taken(mp, _maf(), inputs=_dev(ROWS, 2, 4)) == "host"
    # a state that does not fit the LDS: there is no schedule
    wide = _maf(8, 512)
    assert ops.made_block_cap(8, 512, 6, 0) <= 0 and _inverse_taken(mp, wide) == "host"
    assert wide._inverse_kernel_net() is wide.autoregressive_net and wide._inverse_kernel_plan(wide.autoregressive_net) == (None, None)
    # the size rule: many rows of few features keep the host loop
    few, many = MAF._INVERSE_KERNEL_ROW_LIMIT
    assert _inverse_taken(mp, _maf(few), rows=many) == "k23"
    assert _inverse_taken(mp, _maf(few), rows=many + 1) == "host"
    assert _inverse_taken(mp, _maf(few + 1), rows=many + 1) == "k23"
    # grad mode, the switch on the class and on the instance
    assert _inverse_taken(mp, _maf(), grad=True) == "host"
    off = _maf()
    off.fuse_sequential_inverse = False
    assert _inverse_taken(mp, off) == "host"
    mp.setattr(MAF, "fuse_sequential_inverse", False)
    assert _inverse_taken(mp, _maf()) == "host"


def _subclass_overriding(base, hook):
    def override(self, *args, **kw):
        return getattr(base, hook)(self, *args, **kw)
    return type("Mine", (base,), {hook: override})


@pytest.mark.parametrize("hook", MAF._INVERSE_HOOKS)
def test_an_overridden_inverse_hook_keeps_the_host_loop(switches, hook):
    assert MAF._INVERSE_HOOKS == ("inverse", "_elementwise_inverse", "_inverse_column", "_output_dim_multiplier")
    assert _inverse_taken(switches, _maf(cls=_subclass_overriding(MAF, hook))) == "host"
    assigned = _maf()
    setattr(assigned, hook, lambda *args, **kw: getattr(MAF, hook)(assigned, *args, **kw))
    assert _inverse_taken(switches, assigned) == "host"
    # a hook of the density pass alone does not concern the inverse
    assert _inverse_taken(switches, _maf(cls=_subclass_overriding(MAF, "_elementwise_forward"))) == "k23"


def test_the_k23_plan_follows_the_weights_key():
    layer = _maf(ce=3)
    net = layer.autoregressive_net
    first = layer._inverse_kernel_plan(net)
    assert layer._inverse_kernel_plan(net) is first and first[0] is not None and first[1] is not None
    with torch.no_grad():
        net.final_layer.weight.mul_(2)
    second = layer._inverse_kernel_plan(net)
    assert second is not first and not torch.equal(second[0][0], first[0][0])


# ---- K22 / K29: a layer's forward as a run of one ---------------------------------------------------------------------------------------

def _record_flow_launchers(monkeypatch, calls):
    """The three run wrappers record (kind, num_layers, the plan's weights) and hand the rows on unchanged."""
    def k22(inputs, weights, biases, tables, features, hidden_linears, context=None, accumulate_into=None, num_layers=1,
            standard_normal_log_prob=False, pad=None, residual_blocks=True):
        assert pad == ((features + 3) // 4 * 4, 0.0) and tables.shape[0] >= num_layers
        calls.append(("k22", num_layers, weights))
        return inputs, "log_prob" if standard_normal_log_prob else accumulate_into

    def k29(inputs, weights, biases, tables, features, hidden_linears, spec, context=None, accumulate_into=None, num_layers=1,
            standard_normal_log_prob=False, pad=None, residual_blocks=True):
        assert pad == ((features + 3) // 4 * 4, 0.0) and spec.num_bins >= 2
        calls.append(("k29", num_layers, weights))
        return inputs, "log_prob" if standard_normal_log_prob else accumulate_into

    def k11(inputs, weights, biases, tables, num_transform, num_identity, hidden_linears, scale_activation, inverse=False,
            accumulate_into=None, num_layers=1, standard_normal_log_prob=False, pad=None, residual_blocks=False):
        assert pad == ((num_transform + num_identity + 3) // 4 * 4, 0.0) and not inverse
        calls.append(("k11", num_layers, weights))
        return inputs, "log_prob" if standard_normal_log_prob else accumulate_into
    monkeypatch.setattr(ops, "affine_flow_made", k22)
    monkeypatch.setattr(ops, "rqs_flow_made", k29)
    monkeypatch.setattr(ops, "affine_flow_mlp", k11)


def _record_layer_by_layer(monkeypatch, calls):
    """What the layer-by-layer path of the two classes ends in: the base class's MADE pass + elementwise kernel, or (8 bins)
    K13 on the hidden vector."""
    def host(self, inputs, context=None):
        calls.append(("host", self))
        return inputs, torch.zeros(inputs.shape[0])

    def k13(inputs, hidden, packed, spec, first_column=0, inverse=False, out=None):
        calls.append(("host", "k13"))
        return inputs, torch.zeros(inputs.shape[0])
    monkeypatch.setattr(AutoregressiveTransform, "forward", host)
    monkeypatch.setattr(ops, "made_output_spline", k13)


def _forward_taken(monkeypatch, layer, rows=ROWS, context=None, inputs=None, grad=False):
    """"k22" / "k29" / "host": what `forward` calls for this layer."""
    calls = []
    _record_flow_launchers(monkeypatch, calls)
    _record_layer_by_layer(monkeypatch, calls)
    features = layer.autoregressive_net.initial_layer.weight.shape[1]
    x = _dev(rows, features) if inputs is None else inputs
    with torch.set_grad_enabled(grad):
        layer.forward(x, context)
    assert len(calls) == 1 and (calls[0][0] == "host" or calls[0][1] == 1), calls
    return calls[0][0]


def _forward_table(mp, make, kind, cls, hooks_of_the_inverse):
    """The decisions the two classes share."""
    assert _forward_taken(mp, make()) == kind
    assert _forward_taken(mp, make(7, 32, use_residual_blocks=False, random_mask=True, num_blocks=3)) == kind
    assert _forward_taken(mp, make(ce=5), context=_dev(ROWS, 5)) == kind
    assert _forward_taken(mp, make(1)) == kind and _forward_taken(mp, make(64, 128)) == kind
    assert _forward_taken(mp, make(num_blocks=6)) == kind                       # (no limit on the Linears: K23 / K28 have one)
    # the conditioner
    assert _forward_taken(mp, make(activation=torch.tanh)) == "host"
    assert _forward_taken(mp, make(use_batch_norm=True)) == "host"
    assert _forward_taken(mp, make(dropout_probability=0.3).train()) == "host"
    assert _forward_taken(mp, make(dropout_probability=0.3)) == kind            # eval: the dropout is off
    assert _forward_taken(mp, make(8, 132)) == "host" and _forward_taken(mp, make(65, 32)) == "host"
    assert _forward_taken(mp, make(ce=65), context=_dev(ROWS, 65)) == "host"
    swapped = make()
    swapped.autoregressive_net.activation = torch.tanh                          # read per call
    assert _forward_taken(mp, swapped) == "host"
    swapped.autoregressive_net.activation = F.relu
    assert _forward_taken(mp, swapped) == kind
    # the context
    assert _forward_taken(mp, make(ce=5), context=_dev(ROWS, 4)) == "host"      # of the wrong width
    assert _forward_taken(mp, make(ce=5)) == "host"                             # missing
    assert _forward_taken(mp, make(), context=_dev(ROWS, 3)) == "host"          # unwanted
    assert _forward_taken(mp, make(ce=5), context=torch.zeros(ROWS, 5)) == "host"
    assert _forward_taken(mp, make(ce=5), context=_dev(ROWS, 5, dtype=torch.float64)) == "host"
    assert _forward_taken(mp, make(ce=5), context=_dev(ROWS, 5, 1)) == "host"
    # the inputs
    assert _forward_taken(mp, make(), inputs=torch.zeros(ROWS, 8)) == "host"
    assert _forward_taken(mp, make(), inputs=_dev(ROWS, 8, dtype=torch.float64)) == "host"
    assert _forward_taken(mp, make(), inputs=_dev(ROWS, 9)) == "host"
    assert _forward_taken(mp, make(), inputs=_dev(0, 8)) == "host"
    assert _forward_taken(mp, make(), inputs=_dev(ROWS, 2, 4)) == "host"
    # a user's functions, by subclass and by assignment; the inverse's hooks do not concern the density pass
    for hook in cls._HOOKS:
        assert _forward_taken(mp, make(cls=_subclass_overriding(cls, hook))) == "host", hook
        assigned = make()
        setattr(assigned, hook, lambda *args, _h=hook, _l=assigned, **kw: getattr(cls, _h)(_l, *args, **kw))
        assert _forward_taken(mp, assigned) == "host", hook
    for hook in hooks_of_the_inverse:
        assert _forward_taken(mp, make(cls=_subclass_overriding(cls, hook))) == kind, hook
    # grad mode, the switch on the instance and on the class
    assert _forward_taken(mp, make(), grad=True) == "host"
    off = make()
    off.fuse_conditioner = False
    assert _forward_taken(mp, off) == "host"
    mp.setattr(cls, "fuse_conditioner", False)
    assert _forward_taken(mp, make()) == "host"


def test_which_forward_calls_take_k22(switches):
    mp = switches
    assert MAF._HOOKS == ("forward", "_elementwise_forward", "_elementwise_inverse", "_output_dim_multiplier")
    # where the two classes differ today: K22 reads neither the weights' dtype nor the context's rows
    assert _forward_taken(mp, _maf().double()) == "k22"
    assert _forward_taken(mp, _maf(ce=5), context=_dev(ROWS + 1, 5)) == "k22"
    _forward_table(mp, _maf, "k22", MAF, ("inverse", "_inverse_column"))


def test_which_forward_calls_take_k29(switches):
    mp = switches
    assert ARQ._HOOKS == ("forward", "_elementwise", "_elementwise_forward", "_output_dim_multiplier")
    # where the two classes differ today: K29 refuses float64 weights and a context of another number of rows
    assert _forward_taken(mp, _arq().double()) == "host"
    assert _forward_taken(mp, _arq(ce=5), context=_dev(ROWS + 1, 5)) == "host"
    # bins, tails and the switch's modes: 8 bins keep hidden GEMMs + K13 unless the mode is 2
    for bins in (2, 3, 9, 10, 16):
        assert _forward_taken(mp, _arq(bins=bins)) == "k29", bins
    assert _forward_taken(mp, _arq(bins=17)) == "host" and _forward_taken(mp, _arq(bins=8)) == "host"
    assert _forward_taken(mp, _arq(tails=None)) == "host"
    mp.setattr(ARQ, "fuse_conditioner", 2)
    assert _forward_taken(mp, _arq(bins=8)) == "k29" and _forward_taken(mp, _arq(bins=10)) == "k29"
    mp.setattr(ARQ, "fuse_conditioner", 1)
    _forward_table(mp, _arq, "k29", ARQ, ("inverse", "_elementwise_inverse", "_inverse_column"))


def test_a_run_of_one_keeps_its_plan(switches):
    """A layer called on its own packs once: the second call is handed the same blobs."""
    for layer in (_maf(), _arq()):
        calls = []
        _record_flow_launchers(switches, calls)
        with torch.no_grad():
            layer.forward(_dev(ROWS, 8))
            layer.forward(_dev(ROWS + 3, 8))
            assert len(calls) == 2 and calls[0][2] is calls[1][2] and len(layer.__dict__["_run_plans"]) == 1
            layer.autoregressive_net.final_layer.bias.add_(1.0)
            layer.forward(_dev(ROWS, 8))
        assert calls[2][2] is not calls[0][2]


def test_the_k13_pack_is_kept_per_first_feature(switches):
    layer = _arq(bins=8)
    packs, real = [], ops.pack_made_output
    switches.setattr(ops, "pack_made_output", lambda net, mult, first=0: packs.append(first) or real(net, mult, first))
    switches.setattr(ops, "made_output_spline", lambda inputs, hidden, packed, spec, **kw: packed)
    x, h = _dev(ROWS, 8), _dev(ROWS, 32)
    with torch.no_grad():
        a = layer._output_layer_kernel(x, h, 0, inverse=False)
        b = layer._output_layer_kernel(x, h, 5, inverse=True)
        assert layer._output_layer_kernel(x, h, 0, inverse=False) is a and layer._output_layer_kernel(x, h, 5, inverse=True) is b
        assert packs == [0, 5]
        layer.autoregressive_net.final_layer.weight.mul_(2)
        assert layer._output_layer_kernel(x, h, 0, inverse=False) is not a and packs == [0, 5, 0]


# ---- composites of [Permutation, layer] x 3 ------------------------------------------------------------------------------------------------

def _k11(features=8, hidden=32, depth=2, activation=F.relu, **kw):
    return AffineCouplingTransform(create_alternating_binary_mask(features, even=True),
                                   lambda a, b: MLP([a], [b], [hidden] * depth, activation=activation))


def _composite(make, middle=None):
    """[Permutation, layer] x 3; `middle`: keyword arguments of the second layer's own."""
    torch.manual_seed(2)
    layers = []
    for i in range(3):
        layers += [RandomPermutation(8), make(**(middle if middle and i == 1 else {}))]
    return CompositeTransform(layers).eval()


def _runs(comp, x):
    """[(first layer's index, layers in the run)] as `forward` would find them, None for a layer taken on its own."""
    layers, found, i = list(comp._transforms), [], 0
    with torch.no_grad():
        while i < len(layers):
            units, after = comp._collect_run(layers, i, x, None, inverse=False)
            found.append((i, len(units)) if units else None)
            i = after if units else i + 1
    return found


KINDS = {"k22": (_maf, MAF), "k29": (_arq, ARQ), "k11": (_k11, AffineCouplingTransform)}


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_composite_is_one_run_with_one_plan(switches, kind):
    make, cls = KINDS[kind]
    comp = _composite(make)
    calls = []
    _record_flow_launchers(switches, calls)
    _record_layer_by_layer(switches, calls)
    x = _dev(ROWS, 8)
    assert _runs(comp, x) == [(0, 3)]
    with torch.no_grad():
        out, total = comp.forward(x)
        comp.forward(_dev(ROWS + 1, 8))
        assert out is x and total.shape == (ROWS,)
        assert [c[:2] for c in calls] == [(kind, 3)] * 2 and calls[0][2] is calls[1][2]
        assert len(comp.__dict__["_run_plans"]) == 1
        units, _ = comp._collect_run(list(comp._transforms), 0, x, None, inverse=False)
        plan = comp._run_plan(units, False, 0)
        assert len(plan) == 5 and plan[0] is calls[0][2] and plan[3] is None and plan[4] is None
        assert comp._run_plan(units, False, 0) is plan and len(comp.__dict__["_run_plans"]) == 1
        # the inverse: K22 / K29 serve the density pass only, K11 both directions under a plan of its own
        reverse = comp._collect_run(list(comp._transforms)[::-1], 0, x, None, inverse=True)[0]
        assert len(reverse) == (3 if kind == "k11" else 0)
        if kind == "k11":
            assert comp._run_plan(reverse, True, 0) is not plan and len(comp.__dict__["_run_plans"]) == 2
        # a weight changed in place: packed again
        list(comp._transforms[3]._conditioner().parameters())[-1].add_(1.0)
        comp.forward(x)
    assert calls[2][:2] == (kind, 3) and calls[2][2] is not calls[0][2]
    # the log-density of a standard normal base: the same run, the second of the launcher's results
    with torch.no_grad():
        assert comp.standard_normal_log_prob(x) == "log_prob"
    assert calls[3][:2] == (kind, 3)


@pytest.mark.parametrize("kind", list(KINDS))
def test_where_a_broken_run_splits(switches, kind):
    make, cls = KINDS[kind]
    x = _dev(ROWS, 8)
    alone = 1 if kind != "k11" else None    # (an autoregressive layer is a run of one; a coupling layer on its own is none)
    split = [(0, 1), None, None, (4, 1)] if alone else [None] * 6
    # tanh in the middle layer
    assert _runs(_composite(make), x) == [(0, 3)]
    assert _runs(_composite(make, middle=dict(activation=torch.tanh)), x) == split
    # the switch set on the middle layer's instance
    comp = _composite(make)
    comp._transforms[3].fuse_conditioner = False
    assert _runs(comp, x) == split
    # ... and on the last layer's: the run ends in front of it
    comp = _composite(make)
    comp._transforms[5].fuse_conditioner = False
    assert _runs(comp, x) == [(0, 2), None, None]
    del comp._transforms[5].fuse_conditioner
    assert _runs(comp, x) == [(0, 3)]
    # another signature in the middle (the conditioner's depth): three runs of one, or none
    comp = _composite(make, middle=dict(depth=3) if kind == "k11" else dict(num_blocks=1))
    assert _runs(comp, x) == ([(0, 1), (2, 1), (4, 1)] if alone else [None] * 6)
    if kind == "k11":
        return
    # what `forward` then launches: the wrapper for each run of one, the middle layer on the layer-by-layer path
    comp = _composite(make)
    comp._transforms[3].fuse_conditioner = False
    calls = []
    _record_flow_launchers(switches, calls)
    _record_layer_by_layer(switches, calls)
    switches.setattr(ops, "permute_cols", lambda inputs, index: inputs)    # (the permutation in front of the middle layer)
    with torch.no_grad():
        comp.forward(x)
    assert [c[:2] for c in calls] == [(kind, 1), ("host", comp._transforms[3]), (kind, 1)]
    assert len(comp.__dict__["_run_plans"]) == 2


def test_a_run_of_spline_coupling_layers_goes_through_the_cascade(switches):
    """The K8 family under the same planner: one launch of the engine's launcher with the run's plan."""
    flow = configs.rq_nsf_flow(num_layers=3, features=8, num_bins=8, hidden_features=32, seed=0).eval()
    comp = flow._transform
    calls = []

    def launcher(name):
        def launch(inputs, *args, num_layers=1, **kw):
            calls.append((name, num_layers))
            return inputs, None
        return launch
    for name in ("rqs_coupling_resnet", "rqs_coupling_resnet_f16", "rqs_coupling_resnet_f16x3"):
        switches.setattr(ops, name, launcher(name))
    x = torch.zeros(ROWS, 8)
    assert _runs(comp, x) == [(0, 3)]
    with torch.no_grad():
        comp.forward(x)
        comp.forward(x)
    assert len(calls) == 2 and calls[0] == calls[1] and calls[0][1] == 3 and len(comp.__dict__["_run_plans"]) == 1
