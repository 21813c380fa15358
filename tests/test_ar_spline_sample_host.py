"""CPU-only checks of K28's host side (csrc/made_inverse.hip `nfa_made_rqs_inverse_ctx_f32`, the plan and the gate of
`MaskedPiecewiseRationalQuadraticAutoregressiveTransform._sequential_kernel`): the restatement of the inverse against the
real reference's fixture, the packed step blocks walked the way the kernel walks them, every case of the GPU file run with
the fp32 stand-in under the GPU file's rule, the entry point's argument contract, and which kernel a layer takes."""
import ctypes

import numpy as np
import pytest
import torch

import ar_spline_sample_cases as S
import maf_inverse_cases as inv
from nflows_amd import _native as N
from nflows_amd import ops

F = torch.nn.functional


# ---- the restatement against the real reference ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.FIXTURE))
def test_restated_inverse_reproduces_the_reference(golden_dir, name):
    g = S.load(golden_dir)
    flow = S.build(name, g)
    z = torch.from_numpy(g[name + "/z"])
    context = torch.from_numpy(g[name + "/context"]) if name + "/context" in g.files else None
    assert z.shape == (S.FIXTURE_ROWS, S.FIXTURE[name]["features"])
    assert torch.equal(z, S.inputs(name, rows=S.FIXTURE_ROWS)[0])
    o = S.inverse_pair(flow, z, context)
    for got, want in ((o["x64"], g[name + "/x64"]), (o["lad64"], g[name + "/lad64"])):
        assert np.abs(got - want).max() <= 1e-12 * (1 + np.abs(want).max()), name
    S.assert_parity(o["x32"], g[name + "/x"], g[name + "/x64"], name + " restated fp32 x")
    S.assert_parity(o["lad32"], g[name + "/lad"], g[name + "/lad64"], name + " restated fp32 lad")


# ---- the packed schedule, walked ------------------------------------------------------------------------------------------------

def _context_terms(net, context):
    packed = ops.pack_made_context(net)
    if packed is None:
        return None
    with torch.no_grad():
        return ops.made_context_terms(context[None], packed)[0].double()


CUT_BY_THE_LDS = {"d6_h128_k5", "d6_h128_c8"}   # one block per step does not fit twice beside the state


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_k28_schedule_reproduces_the_masked_network(name):
    """The last layer's schedule (P = 3 K - 1, T = the largest hidden degree) walked like the kernel in float64: every
    sequential feature's logits and the final hidden vector equal the masked network's -- with one block per step, with
    the plan's own cap, and with half of it."""
    layer = S.build(name)._transform._transforms[-1]
    net, K = layer.autoregressive_net, layer.num_bins
    P, (H, D) = 3 * K - 1, net.initial_layer.weight.shape
    ce = S.CASES[name].get("context_features")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(D, dtype=torch.float64, generator=g)
    context = None if ce is None else torch.randn(ce, generator=g)
    terms = _context_terms(net, context)
    _, _, T, cap = S.plan(layer)
    assert T == min(D, S.sequential_steps(net)) and 1 <= T <= D and cap > 0
    with torch.no_grad():
        c64 = None if ce is None else context.double()[None]
        net64 = net.double()
        want = net64(x[None], c64)[0].view(D, P)[:T]
        # (the hidden vector once every unit is final: of the features < T alone)
        xT = x.clone()
        xT[T:] = 0.0
        hidden_want = net64.hidden(xT[None], c64)[0]
        net.float()
    whole = ops.pack_made_schedule(net, T, P, context=True)
    assert whole[1].numel() == T + 3
    params, continuation, final_vec = inv.walk_schedule(whole, x, terms)
    assert params.shape == (T, P) and continuation == [0] * T
    assert (params - want).abs().max().item() < 1e-5 * (1 + want.abs().max().item())
    assert (final_vec[:H] - hidden_want).abs().max().item() < 1e-5 * (1 + hidden_want.abs().max().item())
    counts = {}
    for c in (cap, cap // 2 // 256 * 256):
        cut = ops.pack_made_schedule(net, T, P, block_cap=c, context=True)
        assert cut is not None and cut[2][7] <= c and cut[2][:7] == whole[2][:7] and cut[2][8:] == whole[2][8:]
        p2, c2, f2 = inv.walk_schedule(cut, x, terms, block_cap=c)
        assert torch.equal(p2, params) and torch.equal(f2, final_vec), c    # the same numbers in the same order
        assert cut[1].numel() - 2 >= T + 1 + sum(c2)
        counts[c] = c2
    # continuation blocks exactly where a whole step is more than the cap
    assert (max(counts[cap]) > 0) == (whole[2][7] > cap) == (name in CUT_BY_THE_LDS), (name, counts[cap], whole[2][7], cap)
    if name in CUT_BY_THE_LDS:
        assert sum(counts[cap // 2 // 256 * 256]) > sum(counts[cap])
    # a cap below one unit's row, or below a feature's output rows, has no schedule
    assert ops.pack_made_schedule(net, T, P, block_cap=0, context=True) is None
    assert ops.pack_made_schedule(net, T, P, block_cap=256, context=True) is None or P * whole[2][5] + P + 16 <= 256


def test_lds_budget_of_the_continuation_shape():
    """D = 6, H = 128, two residual blocks: T = 5, 44 KB of state, a step of 26 units per Linear -- K12's one block per
    step does not fit twice, K28's plan cuts it."""
    layer = S.build("d6_h128_k5")._transform._transforms[-1]
    schedule, packed_context, T, cap = S.plan(layer)
    assert T == 5 and packed_context is None
    whole = ops.pack_made_schedule(layer.autoregressive_net, T, 14)
    assert ops.made_state_bytes(T, 128, 5) + 2 * 4 * whole[2][7] > ops.MADE_LDS_BYTES
    assert schedule[2][7] <= cap and schedule[1].numel() - 2 > T + 1
    assert ops.made_state_bytes(T, 128, 5) + 2 * 4 * schedule[2][7] <= ops.MADE_LDS_BYTES


# ---- every case of the GPU file with the stand-in in the kernel's place -------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.CASES))
def test_the_stand_in_passes_every_gpu_case(name):
    flow = S.build(name)
    z, context = S.inputs(name)
    assert z.shape[0] == S.rows_of(name)
    o = S.inverse_pair(flow, z, context)
    x, lad = S.stand_in(flow, z, context)
    fx = S.assert_parity(x, o["x32"], o["x64"], name + " stand-in x")
    fl = S.assert_parity(lad, o["lad32"], o["lad64"], name + " stand-in lad")
    print("FIGURES", repr(name), tuple(float("%.2e" % v) for f in (fx, fl) for v in
                                       (f["mean"][0], f["mean"][1], f["q999"][0], f["q999"][1], f["max"][0], f["max"][1],
                                        f["above_4x_max"])))


@pytest.mark.parametrize("name", list(S.FIXTURE))
def test_the_stand_in_passes_the_reference_fixture(golden_dir, name):
    """What tests/test_gpu_ar_spline_sample.py::test_the_real_reference_fixture asks of the kernel, asked of the stand-in."""
    g = S.load(golden_dir)
    flow = S.build(name, g)
    context = torch.from_numpy(g[name + "/context"]) if name + "/context" in g.files else None
    x, lad = S.stand_in(flow, torch.from_numpy(g[name + "/z"]), context)
    S.assert_parity(x, g[name + "/x"], g[name + "/x64"], name + " stand-in on the fixture x")
    S.assert_parity(lad, g[name + "/lad"], g[name + "/lad64"], name + " stand-in on the fixture lad")


def test_the_stand_in_follows_the_block_cap_bit_for_bit():
    layer = S.build("d6_h128_c8")._transform._transforms[-1]
    z, context = S.inputs("d6_h128_c8", 64)
    cap = S.plan(layer)[3]
    a, b = S.stand_in_layer(layer, z, context), S.stand_in_layer(layer, z, context, block_cap=cap // 2 // 256 * 256)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and 0 < a[2] < b[2]


# ---- the entry point without a device -----------------------------------------------------------------------------------------------

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer for buffers that are checked but never read


def _layout(n=5, Hp=32, Xp=16, max_block=1024, residual=1):
    layout = [n, residual, n - 1, n - 1 if residual else -1, n, Hp, Xp, max_block]
    for l in range(n):
        layout += [Xp if l == 0 else Hp, l - 1, l, 0, 0]
    return layout


def _call(lib, layout=None, bufs=None, **kw):
    p = dict(batch=64, D=8, H=32, C=0, T=7, nblocks=8, ctx=None, K=8, tails="linear", status=None)
    p.update(kw)
    layout = _layout() if layout is None else layout
    arr = (ctypes.c_int32 * len(layout))(*layout)
    spec = ops.make_rqs_spec(p["K"], p["tails"], tail_bound=3.0)
    return lib.nfa_made_rqs_inverse_ctx_f32(bufs, p["ctx"], p["C"], bufs, bufs, p["nblocks"], arr, len(layout), bufs, bufs,
                                            bufs, p["status"], p["batch"], p["D"], p["H"], p["T"], ctypes.byref(spec), None)


def test_rqs_inverse_ctx_entry_point_contract():
    lib = N.load()
    assert lib.nfa_abi_version() == 19 and N.ABI_VERSION == 19
    assert "nfa_made_rqs_inverse_ctx_f32" in N.EXPORTS
    assert _call(lib, batch=0) == N.OK
    assert _call(lib, batch=0, C=3) == N.OK
    for K in range(2, 17):
        assert _call(lib, batch=0, K=K) == N.OK, K
    # null pointers
    assert _call(lib) == N.ERR_INVALID_ARGUMENT
    assert _call(lib, bufs=DUMMY, C=2, ctx=None) == N.ERR_INVALID_ARGUMENT   # context vectors without their buffer
    # bad sizes and layouts, batch 0 does not hide them; fewer blocks than steps + 1
    for kw in (dict(batch=-1), dict(D=0), dict(H=0), dict(C=-1), dict(C=6), dict(nblocks=7), dict(T=9), dict(T=-1),
               dict(H=33), dict(D=40, T=17, nblocks=18)):
        assert _call(lib, **kw) == N.ERR_INVALID_ARGUMENT, kw
        if "batch" not in kw:
            assert _call(lib, batch=0, **kw) == N.ERR_INVALID_ARGUMENT, kw
    for layout in (_layout(n=0), _layout(n=13), _layout()[:-1], _layout(Hp=40), _layout(Xp=8), _layout(max_block=1000),
                   _layout(max_block=0), _layout()[:2] + [7] + _layout()[3:], _layout()[:3] + [9] + _layout()[4:]):
        assert _call(lib, layout=layout, batch=0) == N.ERR_INVALID_ARGUMENT, layout
    # outside the family: 17 bins, 1 bin, tails=None
    assert _call(lib, batch=0, K=17) == N.ERR_UNSUPPORTED
    assert _call(lib, batch=0, K=1) == N.ERR_UNSUPPORTED
    assert _call(lib, batch=0, tails=None) == N.ERR_UNSUPPORTED
    # more than the LDS holds: two blocks of 80 KB; the state of hidden 512 with five Linears; context vectors on top
    assert _call(lib, layout=_layout(max_block=20480), batch=0) == N.ERR_UNSUPPORTED
    assert _call(lib, layout=_layout(Hp=512), H=512, batch=0) == N.ERR_UNSUPPORTED
    fits = _layout(Hp=256, max_block=4096)
    assert _call(lib, layout=fits, H=256, batch=0) == N.OK
    assert _call(lib, layout=fits, H=256, batch=0, C=5) == N.ERR_UNSUPPORTED
    # a grid beyond 2^31 - 1 workgroups
    assert _call(lib, bufs=DUMMY, batch=16 * 2 ** 31 + 1) == N.ERR_UNSUPPORTED


# ---- which kernel a layer takes ---------------------------------------------------------------------------------------------------------

class _OnDevice(torch.Tensor):
    """A CPU tensor that answers `is_cuda` as a device tensor would: the gate reads nothing else of the device."""
    is_cuda = property(lambda self: True)


def _AR():
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform
    return MaskedPiecewiseRationalQuadraticAutoregressiveTransform


def _taken(monkeypatch, layer, rows=32, context_width=None, inputs=None, grad=False):
    """"k12" / "k28" / "host": what `_sequential_kernel` calls for this layer, the two ops functions stubbed (K12's stub
    answers None where its one block per step does not fit the LDS twice, as the entry point does)."""
    calls = []

    def k12(inputs, schedule, hidden_features, sequential_steps, spec, out=None):
        layout = schedule[2]
        if ops.made_state_bytes(sequential_steps, hidden_features, layout[0]) + 8 * layout[7] > ops.MADE_LDS_BYTES:
            return None
        calls.append("k12")
        return "k12"

    def k28(inputs, schedule, hidden_features, sequential_steps, spec, context_terms=None, out=None):
        assert schedule[1].numel() - 2 >= sequential_steps + 1 and spec.num_bins == layer.num_bins
        assert (context_terms is None) == (not hasattr(layer.autoregressive_net, "context_layer"))
        calls.append("k28")
        return "k28"
    monkeypatch.setattr(ops, "made_rqs_inverse", k12)
    monkeypatch.setattr(ops, "made_rqs_inverse_ctx", k28)
    net = layer.autoregressive_net
    D = net.initial_layer.weight.shape[1]
    z = torch.randn(rows, D).as_subclass(_OnDevice) if inputs is None else inputs
    context = None if context_width is None else torch.randn(rows, context_width).as_subclass(_OnDevice)
    with torch.set_grad_enabled(grad):
        got = layer._sequential_kernel(z, context, min(D, layer._sequential_steps()))
    assert (got is None and not calls) or calls == [got], (got, calls)
    return got or "host"


def _layer(features=8, hidden=32, bins=8, ce=None, cls=None, **kw):
    torch.manual_seed(1)
    kw.setdefault("tails", "linear")
    return (cls or _AR())(features=features, hidden_features=hidden, num_bins=bins, context_features=ce, tail_bound=3.0,
                          **kw).eval()


def test_which_layers_take_which_kernel(monkeypatch):
    AR = _AR()
    # what K12 serves keeps K12
    assert _taken(monkeypatch, _layer(20, 30, 10)) == "k12"
    assert _taken(monkeypatch, _layer(12, 48, 8, use_residual_blocks=False, random_mask=True)) == "k12"
    # a context, other bin counts, a step that does not fit twice: K28
    assert _taken(monkeypatch, _layer(8, 32, 10, ce=5), context_width=5) == "k28"
    assert _taken(monkeypatch, _layer(8, 32, 8, ce=5, use_residual_blocks=False), context_width=5) == "k28"
    for bins in (2, 3, 5, 9, 16):
        assert _taken(monkeypatch, _layer(8, 32, bins)) == "k28", bins
    assert _taken(monkeypatch, _layer(6, 128, 8)) == "k28"          # K12 answers unsupported
    assert _taken(monkeypatch, _layer(6, 128, 5)) == "k28"
    # the host loop
    assert _taken(monkeypatch, _layer(8, 32, 17)) == "host"
    assert _taken(monkeypatch, _layer(8, 32, 8, tails=None)) == "host"
    assert _taken(monkeypatch, _layer(8, 32, 5, activation=torch.tanh)) == "host"
    assert _taken(monkeypatch, _layer(8, 32, 5, use_batch_norm=True)) == "host"
    assert _taken(monkeypatch, _layer(8, 32, 5, dropout_probability=0.3).train()) == "host"
    assert _taken(monkeypatch, _layer(8, 32, 5, dropout_probability=0.3)) == "k28"      # eval: the dropout is off
    assert _taken(monkeypatch, _layer(8, 512, 5)) == "host"                             # the state alone does not fit
    assert _taken(monkeypatch, _layer(8, 32, 5, num_blocks=6)) == "host"                # 13 Linears
    assert _taken(monkeypatch, _layer(8, 32, 5, ce=5), context_width=4) == "host"       # a context of the wrong width
    assert _taken(monkeypatch, _layer(8, 32, 5, ce=5)) == "host"                        # a conditional net without its context
    assert _taken(monkeypatch, _layer(8, 32, 5), context_width=3) == "host"             # a context the net does not take
    assert _taken(monkeypatch, _layer(8, 32, 5), inputs=torch.randn(4, 8)) == "host"    # not on the device
    assert _taken(monkeypatch, _layer(8, 32, 5).double(), inputs=torch.randn(4, 8).double().as_subclass(_OnDevice)) == "host"

    class Mine(AR):
        def _elementwise_inverse(self, inputs, params):
            return super()._elementwise_inverse(inputs, params)
    assert _taken(monkeypatch, _layer(8, 32, 5, cls=Mine)) == "host"
    assert _taken(monkeypatch, _layer(20, 30, 10, cls=Mine)) == "k12"                   # (K12's gate is what it was)
    hooked = _layer(8, 32, 5)
    hooked._inverse_column = lambda column, params: AR._inverse_column(hooked, column, params)
    assert _taken(monkeypatch, hooked) == "host"
    # the size rule: many rows of few features keep the host loop
    few, many = AR._SEQUENTIAL_CTX_ROW_LIMIT
    assert _taken(monkeypatch, _layer(few, 32, 5), rows=many) == "k28"
    assert _taken(monkeypatch, _layer(few, 32, 5), rows=many + 1) == "host"
    assert _taken(monkeypatch, _layer(few + 1, 32, 5), rows=many + 1) == "k28"
    assert _taken(monkeypatch, _layer(20, 30, 10), rows=many + 1) == "k12"              # (K12 has no such rule)
    # the switches: NFA_K28 turns K28 off alone, NFA_K12 both
    monkeypatch.setattr(AR, "fuse_sequential_inverse_ctx", False)
    assert _taken(monkeypatch, _layer(8, 32, 5)) == "host" and _taken(monkeypatch, _layer(20, 30, 10)) == "k12"
    monkeypatch.setattr(AR, "fuse_sequential_inverse_ctx", True)
    monkeypatch.setattr(AR, "fuse_sequential_inverse", False)
    assert _taken(monkeypatch, _layer(8, 32, 5)) == "host" and _taken(monkeypatch, _layer(20, 30, 10)) == "host"


def test_the_plan_follows_the_weights_key(monkeypatch):
    layer = _layer(8, 32, 5, ce=3)
    net = layer.autoregressive_net
    first = layer._sequential_ctx_plan(net, 7)
    assert layer._sequential_ctx_plan(net, 7) is first
    with torch.no_grad():
        net.final_layer.weight.mul_(2)
    second = layer._sequential_ctx_plan(net, 7)
    assert second is not first and not torch.equal(second[0][0], first[0][0])
    assert layer._sequential_ctx_plan(net, 6) is not second
