"""CPU-only checks of K29's host side (csrc/made_rqs.hip, ops.pack_made_rqs_conditioner): the fixture
tests/golden/flows_ar_rq_density.npz with its seed builder and its restatement (tests/ar_spline_density_cases.py), the packed
stream walked in numpy against the float64 logits of the MADE, the argument contract of `nfa_rqs_flow_made_f32` through
the C ABI with null pointers, and the decisions of the gate that need no device."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import ar_spline_density_cases as C
import maf_cases
from nflows_amd import _native as N
from nflows_amd import ops

NORMAL, SKIP, RESIDUAL = N.FLAG_STANDARD_NORMAL_LOG_PROB, N.FLAG_SKIP_OUTPUTS, N.FLAG_RESIDUAL_BLOCKS
_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer for buffers that are checked but never read


@pytest.mark.parametrize("name", list(C.FIXTURE))
def test_builder_and_restatement_reproduce_the_fixture(golden_dir, name):
    """`build` rebuilds the reference's state_dict from the seed (names and checksums of every parameter, mask, degree vector
    and permutation), and the restatement of the density pass reproduces the reference's vectors bit for bit in fp32 and in
    fp64 -- no element skipped."""
    g = C.load(golden_dir)
    assert [str(n) for n in g["cases"]] == list(C.FIXTURE)
    flow = C.build(name, g)
    x, context = C.inputs(name, rows=C.FIXTURE_ROWS)
    assert np.array_equal(x.numpy(), g[name + "/x"]) and x.shape[0] == 256
    assert (context is None) == (name + "/context" not in g.files)
    if context is not None:
        assert np.array_equal(context.numpy(), g[name + "/context"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # (as the fixture was made: a threaded fp32 GEMM sums a 21-wide row in another order)
    try:
        o = C.restated_pair(flow, x, context)
    finally:
        torch.set_num_threads(threads)
    for mine, theirs in (("z", "z"), ("lad", "lad"), ("lp", "log_prob")):
        for tag, suffix, dtype in (("32", "", np.float32), ("64", "64", np.float64)):
            want = g[name + "/" + theirs + suffix]
            assert want.dtype == dtype and np.isfinite(want).all()
            assert np.array_equal(o[mine + tag], want), (name, theirs, tag, float(np.abs(o[mine + tag] - want).max()))


def test_the_fixture_is_small_and_covers_what_it_should(golden_dir):
    import os
    assert os.path.getsize(os.path.join(golden_dir, "flows_ar_rq_density.npz")) < 600 * 1024
    cfgs = list(C.FIXTURE.values())
    assert {ops.made_rqs_tiles(c["num_bins"]) for c in cfgs} == {1, 2, 3} and all(c["num_bins"] != 8 for c in cfgs)
    assert any(c["context_features"] for c in cfgs) and any(c["permutation"] == "random" for c in cfgs)
    assert any(c["features"] % 4 == 3 for c in cfgs)   # a pad column


@pytest.mark.parametrize("name", list(C.CASES))
def test_packed_stream_reproduces_the_logits(name):
    """A numpy walk over the stages of `pack_made_rqs_conditioner`: the final layer's bf16 pieces recombined and its row and
    column orders undone, applied to the float64 hidden vector, give the float64 logits of `made_forward` -- the width and
    height logits after the divisor where the net has one -- within what three bf16 pieces leave of a weight; padded rows
    and features are exactly zero; the head of the stream is `pack_made_conditioner`'s, bit for bit."""
    cfg = C.CASES[name]
    flow = C.build(name)
    K, P, D = cfg["num_bins"], 3 * cfg["num_bins"] - 1, cfg["features"]
    x, context = C.inputs(name, rows=64)
    for index, layer in enumerate(C.spline_layers(flow)):
        net = layer.autoregressive_net
        if index == 1:
            net.hidden_features = cfg["hidden_features"]   # the reference's divisor, where a net exposes the attribute
        weights, biases = ops.pack_made_rqs_conditioner(net, K)
        H = net.initial_layer.weight.shape[0]
        residual = bool(net.use_residual_blocks)
        hidden_linears = len(net.blocks) * (2 if residual else 1)
        cks = (cfg["context_features"] + 15) // 16 if cfg["context_features"] else 0
        T = ops.made_rqs_tiles(K)
        tiles = (D + 1) // 2 * T
        head = (4 if D > 32 else 2) + 8 * hidden_linears + cks * (1 + (len(net.blocks) if residual else 0))
        assert weights.dtype == torch.bfloat16 and weights.shape == (head + 2 * tiles, 768 * 8)
        assert biases.numel() == 128 * (1 + hidden_linears + (1 if cks else 0)) + 32 * tiles
        # the head: K22's stream of the same net (its own final layer has other rows: compare the stages in front of it)
        affine_like = ops.pack_mlp_conditioner(net, D, row_order=torch.full((32,), -1, dtype=torch.int64),
                                               context=ops._context_linears(net) if cks else None)
        assert torch.equal(weights[:head].view(torch.int16), affine_like[0][:head].view(torch.int16))
        assert torch.equal(biases[:-32 * tiles], affine_like[1][:-32])
        W, b, pad_w, pad_b = C.unpack_final_logit_rows(weights, biases, net, K)
        assert not pad_w.any() and not pad_b.any()
        assert not W[:, :, H:].any()                       # hidden units beyond the net's own
        with torch.no_grad():
            net64 = copy.deepcopy(net).double()
            x64, c64 = x.double(), None if context is None else context.double()
            h = C.hidden_vector(net64, x64, c64)
            want = maf_cases.made_forward(net64, x64, c64).view(-1, D, P).clone()
            if hasattr(net, "hidden_features"):
                want[..., :2 * K] /= np.sqrt(net.hidden_features)
            got = torch.einsum("bh,dph->bdp", h, W[:, :, :H]) + b
            # three bf16 pieces keep 24 bits of a weight: every term of the dot product is off by at most 2^-24 of itself
            # (the pieces round to nearest: half an ulp of the 8-bit third piece below 2^-16 of the weight), plus the one
            # fp32 rounding of the scaled weight and bias where a divisor is folded in
            masked = (net64.final_layer.weight * net64.final_layer.mask).view(D, P, H).abs()
            bound = 2.0 ** -23 * (torch.einsum("bh,dph->bdp", h.abs(), masked) + net64.final_layer.bias.view(D, P).abs())
            assert (got - want).abs().le(bound + 1e-300).all(), (name, index, float((got - want).abs().max()))
        net.__dict__.pop("hidden_features", None)
        if index == 1:
            break


def call(lib, spec, **kw):
    p = dict(batch=128, row=8, D=8, hidden=128, blocks=2, layers=2, ce=0, flags=RESIDUAL, bufs=None)
    p.update(kw)
    b = p["bufs"]
    return lib.nfa_rqs_flow_made_f32(b, b, p["ce"], b, b, b, p["layers"], b, b, b, p["batch"], p["row"], p["D"],
                                     p["hidden"], p["blocks"], ctypes.byref(spec) if spec is not None else None,
                                     p["flags"], None)


def test_entry_point_contract():
    lib = N.load()
    assert "nfa_rqs_flow_made_f32" in N.EXPORTS and lib.nfa_abi_version() == 19 and N.ABI_VERSION == 19
    spec = ops.make_rqs_spec(10, "linear", tail_bound=3.0)
    assert call(lib, spec, batch=0) == N.OK
    assert call(lib, spec, batch=0, flags=RESIDUAL | NORMAL | SKIP | (2 << N.FLAG_PAD_COLUMNS_SHIFT)) == N.OK
    for kw in [dict(batch=-128), dict(D=0), dict(row=4, D=8), dict(layers=0), dict(blocks=-1), dict(ce=-1),
               dict(flags=RESIDUAL, blocks=3), dict(flags=1 << 20), dict(flags=SKIP), dict(flags=NORMAL | N.FLAG_INVERSE)]:
        assert call(lib, spec, **kw) == N.ERR_INVALID_ARGUMENT, kw
    assert call(lib, None) == N.ERR_INVALID_ARGUMENT
    for kw in [dict(D=65, row=68), dict(row=10, D=8), dict(hidden=64), dict(hidden=132), dict(batch=100), dict(ce=65),
               dict(flags=RESIDUAL | N.FLAG_INVERSE), dict(blocks=66), dict(layers=4097)]:
        assert call(lib, spec, **kw) == N.ERR_UNSUPPORTED, kw
    for bins, tails in ((1, "linear"), (17, "linear"), (20, "linear"), (10, None)):
        assert call(lib, ops.make_rqs_spec(bins, tails, tail_bound=3.0)) == N.ERR_UNSUPPORTED, (bins, tails)
    for bins in range(2, 17):   # every instance is there: an in-family shape with null buffers gets past the dispatch's checks
        s = ops.make_rqs_spec(bins, "linear", tail_bound=3.0)
        assert call(lib, s) == N.ERR_INVALID_ARGUMENT and call(lib, s, batch=0) == N.OK, bins
    p = DUMMY
    assert lib.nfa_rqs_flow_made_f32(p, None, 5, p, p, p, 2, p, p, p, 128, 8, 8, 128, 2, ctypes.byref(spec), RESIDUAL,
                                     None) == N.ERR_INVALID_ARGUMENT


def test_gate_decisions_without_a_device():
    """What the planner reads off a layer, on the CPU: kind, signature, geometry, the switch's three modes and the
    eligibility rules that do not need a device tensor."""
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform as AR
    from nflows_amd.transforms.base import _switch_state
    F = torch.nn.functional
    assert AR.fuse_conditioner in _switch_state() and AR._forward_only_run
    saved = AR.fuse_conditioner

    def layer(**kw):
        args = dict(features=6, hidden_features=32, num_bins=10, tails="linear", tail_bound=3.0)
        args.update(kw)
        return AR(**args).eval()
    try:
        AR.fuse_conditioner = 1
        with torch.no_grad():
            plain = layer()
            assert plain._run_kind(None) == "k29" and plain._fused_geometry() == (8, 6, 6, 0.0) and plain.features == 6
            assert plain._run_signature() == ("k29", 6, (4, True), 0, (10, 3.0, 1e-3, 1e-3, 1e-3, 0.0))
            assert plain._conditioner() is plain.autoregressive_net and not plain._user_hooks
            assert plain.unconditional_transform is None
            assert layer(use_residual_blocks=False, num_blocks=3)._conditioner_shape() == (3, False)
            for kw in (dict(activation=torch.tanh), dict(use_batch_norm=True), dict(hidden_features=132), dict(features=65),
                       dict(tails=None), dict(num_bins=17), dict(num_bins=8), dict(context_features=65)):
                assert layer(**kw)._run_kind(None) is None, kw
            for bins in (2, 5, 6, 7, 9, 11, 12, 16):
                assert layer(num_bins=bins)._run_kind(None) == "k29", bins
            assert layer().double()._run_kind(None) is None
            dropped = layer(dropout_probability=0.5)
            assert dropped.eval()._run_kind(None) == "k29" and dropped.train()._run_kind(None) is None
            assert layer(context_features=3)._run_kind(None) is None       # a context net without a context
            assert plain._run_kind(torch.zeros(4, 3)) is None              # a context without a context net
            plain.autoregressive_net.activation = torch.tanh               # read per call
            assert plain._run_kind(None) is None
            plain.autoregressive_net.activation = F.relu
            assert plain._run_kind(None) == "k29"

            class Mine(AR):
                def _elementwise_forward(self, inputs, params):
                    return super()._elementwise_forward(inputs, params)
            assert Mine(6, 32, tails="linear")._user_hooks
            patched = layer()
            patched._elementwise = patched._elementwise
            assert patched._user_hooks
            # the switch: 8 bins in mode 2 only, nothing in mode 0
            eight = layer(num_bins=8)
            AR.fuse_conditioner = 2
            assert eight._run_kind(None) == "k29" and plain._run_kind(None) == "k29"
            AR.fuse_conditioner = 0
            assert eight._run_kind(None) is None and plain._run_kind(None) is None
            AR.fuse_conditioner = 1
            # the divisor is part of the signature and of the pack's key
            plain.autoregressive_net.hidden_features = 64
            assert plain._run_signature()[-1][-1] == 8.0
        assert plain._run_kind(None) is None   # grad mode
    finally:
        AR.fuse_conditioner = saved


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_stand_in_passes_every_gpu_case(name):
    """What tests/test_gpu_ar_spline_density.py asks of the kernel on a case's rows, asked of a free-running fp32 stand-in
    first: no case may ask what correct fp32 arithmetic on the packed weights cannot give."""
    flow = C.build(name)
    x, context = C.inputs(name)
    o = C.restated_pair(flow, x, context)
    z, lad, lp = C.stand_in(flow, x, context)
    figures = [C.assert_parity(z, o["z32"], o["z64"], name + " stand-in z"),
               C.assert_parity(lad, o["lad32"], o["lad64"], name + " stand-in logabsdet"),
               C.assert_parity(lp, o["lp32"], o["lp64"], name + " stand-in log_prob")]
    print("FIGURES", repr(name), tuple(float("%.2e" % v) for f in figures for v in
                                       (f["mean"][0], f["mean"][1], f["q999"][0], f["q999"][1], f["above_4x_max"])))
