"""CPU-only checks of K22's host side (csrc/affine_made.hip, ops.pack_made_conditioner): the argument contract of
`nfa_affine_flow_made_f32` -- none of these paths reaches the device, so the library answers them through the C ABI with
null pointers, as tests/test_whole_layer_abi.py asks of the other whole-layer entry points --, the packed blob of a MADE,
and the fixture tests/golden/flows_maf.npz with its seed builder and its restatement (tests/maf_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import maf_cases
from nflows_amd import _native as N
from nflows_amd import ops

NORMAL, SKIP = N.FLAG_STANDARD_NORMAL_LOG_PROB, N.FLAG_SKIP_OUTPUTS
RESIDUAL = N.FLAG_RESIDUAL_BLOCKS
UNKNOWN_FLAG = 1 << 20

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer for buffers that are checked but never read


def pad(n):
    return n << N.FLAG_PAD_COLUMNS_SHIFT


def call(lib, **kw):
    p = dict(batch=128, row=8, D=8, hidden=128, blocks=2, layers=2, ce=0, flags=RESIDUAL, bufs=None)
    p.update(kw)
    b = p["bufs"]
    return lib.nfa_affine_flow_made_f32(b, b, p["ce"], b, b, b, p["layers"], b, b, b, p["batch"], p["row"], p["D"],
                                        p["hidden"], p["blocks"], p["flags"], None)


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_made_entry_point_contract(lib):
    assert "nfa_affine_flow_made_f32" in N.EXPORTS
    # batch 0 is a no-op, whatever the density flags say
    assert call(lib, batch=0) == N.OK
    assert call(lib, batch=0, flags=RESIDUAL | NORMAL | SKIP | pad(2)) == N.OK
    assert call(lib, batch=0, flags=0, blocks=3) == N.OK
    # invalid arguments
    bad = [dict(batch=-128), dict(D=0), dict(D=-4), dict(row=4, D=8), dict(layers=0), dict(blocks=-1), dict(ce=-1),
           dict(flags=RESIDUAL, blocks=3), dict(flags=UNKNOWN_FLAG), dict(flags=N.FLAG_LOGITS_LOG2E),
           dict(flags=1 << N.FLAG_ACTIVATION_SHIFT), dict(flags=SKIP), dict(flags=pad(1)), dict(flags=NORMAL | N.FLAG_INVERSE),
           dict(flags=NORMAL | pad(7), row=4, D=4, bufs=DUMMY)]   # no density column left
    for kw in bad:
        assert call(lib, **kw) == N.ERR_INVALID_ARGUMENT, kw
    # an argument error wins over a family limit, and batch 0 does not hide it
    for kw in [dict(flags=UNKNOWN_FLAG, hidden=64), dict(D=0, batch=100), dict(layers=0, batch=0), dict(flags=SKIP, batch=0),
               dict(ce=-1, D=65, row=68), dict(flags=N.FLAG_INVERSE | UNKNOWN_FLAG)]:
        assert call(lib, **kw) == N.ERR_INVALID_ARGUMENT, kw
    # family limits, checked before batch 0 returns (except for the ragged batch itself)
    limits = [dict(D=65, row=68), dict(row=10, D=8), dict(row=10, D=10), dict(hidden=64), dict(hidden=256), dict(batch=100),
              dict(batch=130), dict(ce=65), dict(flags=RESIDUAL | N.FLAG_INVERSE), dict(flags=N.FLAG_INVERSE),
              dict(blocks=66), dict(layers=4097)]
    for kw in limits:
        assert call(lib, **kw) == N.ERR_UNSUPPORTED, kw
        if "batch" not in kw:
            assert call(lib, batch=0, **kw) == N.ERR_UNSUPPORTED, kw
    # an in-family shape with null buffers
    shapes = [dict(), dict(row=64, D=64, blocks=0), dict(row=64, D=63, layers=32), dict(row=8, D=6), dict(flags=0, blocks=3),
              dict(flags=RESIDUAL | NORMAL | SKIP | pad(2), row=8, D=6), dict(flags=RESIDUAL | N.FLAG_ACCUMULATE_LOGABSDET),
              dict(ce=5), dict(ce=64, flags=0)]
    for kw in shapes:
        assert call(lib, **kw) == N.ERR_INVALID_ARGUMENT, kw
        assert call(lib, batch=0, **kw) == N.OK, kw
    # a context with columns needs its buffer, whatever else is given
    p = DUMMY
    assert lib.nfa_affine_flow_made_f32(p, None, 5, p, p, p, 2, p, p, p, 128, 8, 8, 128, 2, RESIDUAL, None) == \
        N.ERR_INVALID_ARGUMENT


def test_coupling_entry_point_keeps_its_answers(lib):
    """K11's entry point still declines what only K22 serves."""
    def k11(**kw):
        p = dict(D=8, dt=4, di=4, scale=N.SCALE_DEFAULT)
        p.update(kw)
        return lib.nfa_affine_flow_mlp_f32(None, None, None, None, 2, None, None, None, 128, p["D"], p["dt"], p["di"], 128, 2,
                                           p["scale"], 0, None)
    assert k11(dt=8, di=4) == N.ERR_INVALID_ARGUMENT
    assert k11(dt=8, di=8) == N.ERR_INVALID_ARGUMENT
    assert k11(scale=N.SCALE_SOFTPLUS) == N.ERR_UNSUPPORTED


class _Plain(torch.nn.Module):
    """A conditioner with no masks that `ops.pack_mlp_conditioner` takes: a ResidualNet's attributes (initial_layer,
    blocks[*].linear_layers, final_layer) or an MLP's (_input_layer, _hidden_layers, _output_layer)."""


def _linear(weight, bias):
    lin = torch.nn.Linear(weight.shape[1], weight.shape[0])
    with torch.no_grad():
        lin.weight.copy_(weight)
        lin.bias.copy_(bias)
    return lin


@pytest.mark.parametrize("name", [n for n, c in maf_cases.CASES.items() if "context_features" not in c])
def test_made_blob_is_the_plain_conditioners_blob(name):
    """The packed MADE equals, bit for bit, `pack_mlp_conditioner` of a net without masks that carries `weight * mask`,
    its final rows reordered from the reference's interleaved [scale, shift] pairs to K11's [shift block | scale block]."""
    cfg = maf_cases.CASES[name]
    net = maf_cases.build(name)._transform._transforms[-1].autoregressive_net
    d = cfg["features"]

    def masked(lin):
        return (lin.weight * lin.mask).detach(), lin.bias.detach()
    wf, bf = masked(net.final_layer)
    rows = torch.cat((torch.arange(d) * 2 + 1, torch.arange(d) * 2))   # shifts, then unconstrained scales
    plain = _Plain()
    if cfg["use_residual_blocks"]:
        plain.initial_layer = _linear(*masked(net.initial_layer))
        plain.blocks = torch.nn.ModuleList()
        for block in net.blocks:
            b = _Plain()
            b.linear_layers = torch.nn.ModuleList([_linear(*masked(lin)) for lin in block.linear_layers])
            plain.blocks.append(b)
        plain.final_layer = _linear(wf[rows], bf[rows])
    else:
        plain._input_layer = _linear(*masked(net.initial_layer))
        plain._hidden_layers = torch.nn.ModuleList([_linear(*masked(block.linear)) for block in net.blocks])
        plain._output_layer = _linear(wf[rows], bf[rows])
    got_w, got_b = ops.pack_made_conditioner(net)
    want_w, want_b = ops.pack_mlp_conditioner(plain, d)
    assert got_w.dtype == want_w.dtype and got_w.shape == want_w.shape
    assert torch.equal(got_w.view(torch.int16), want_w.view(torch.int16)) and torch.equal(got_b, want_b)
    final_tiles = (d + 15) // 16
    hidden = len(net.blocks) * (2 if cfg["use_residual_blocks"] else 1)
    assert got_w.shape[0] == (4 if d > 32 else 2) + 8 * hidden + 2 * final_tiles
    assert got_b.numel() == 128 + 128 * hidden + 32 * final_tiles


@pytest.mark.parametrize("name", [n for n, c in maf_cases.CASES.items() if "context_features" in c])
def test_context_stages_join_the_stream_where_they_are_consumed(name):
    """With a context the blob is the unconditional blob with the context stages spliced in -- in front of the initial
    layer's, and behind the first Linear's of every residual block -- and the biases take the context biases."""
    cfg = maf_cases.CASES[name]
    net = maf_cases.build(name)._transform._transforms[-1].autoregressive_net
    d, ce, residual = cfg["features"], cfg["context_features"], cfg["use_residual_blocks"]
    got_w, got_b = ops.pack_made_conditioner(net)
    bare_w, bare_b = ops.pack_mlp_conditioner(net, d, row_order=ops._made_row_order(d))
    init_ks, cks = (4 if d > 32 else 2), (ce + 15) // 16
    keep = list(range(cks, cks + init_ks))
    at = cks + init_ks
    for i in range(len(net.blocks) * (2 if residual else 1)):
        keep += list(range(at, at + 8))
        at += 8 + (cks if residual and i % 2 == 0 else 0)
    keep += list(range(at, got_w.shape[0]))
    assert torch.equal(got_w[keep].view(torch.int16), bare_w.view(torch.int16))
    assert got_w.shape[0] == bare_w.shape[0] + cks * (1 + (len(net.blocks) if residual else 0))
    assert got_b.numel() == bare_b.numel() + 128
    assert torch.equal(got_b[:128], bare_b[:128]) and torch.equal(got_b[-32:], bare_b[-32:])
    # the context layer's first stage holds its columns in the input layer's order: piece sum of lane 0 = row 0
    w = got_w[0].float().view(4, 3, 64, 8)
    want = torch.zeros(8)
    want[:min(8, ce)] = net.context_layer.weight[0, :8].detach()
    assert torch.allclose(w[0, :, 0, :].sum(0), want, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("name", list(maf_cases.CASES))
def test_builder_and_restatement_reproduce_the_fixture(golden_dir, name):
    """configs.masked_affine_flow rebuilds the reference's state_dict from the seed (names and checksums of every
    parameter, mask, degree vector and permutation), and the restatement of the density pass reproduces the reference's
    vectors bit for bit in fp32 and in fp64 -- no element skipped."""
    g = maf_cases.load(golden_dir)
    assert [str(n) for n in g["cases"]] == list(maf_cases.CASES)
    flow = maf_cases.build(name, g)
    x, context = maf_cases.fixture_inputs(name)
    assert np.array_equal(x.numpy(), g[name + "/x"]) and x.shape[0] == maf_cases.ROWS
    assert (context is None) == (name + "/context" not in g.files)
    if context is not None:
        assert np.array_equal(context.numpy(), g[name + "/context"])
    o = maf_cases.restated_pair(flow, x, context)
    for mine, theirs in (("z", "z"), ("lad", "lad"), ("lp", "log_prob")):
        for tag, suffix, dtype in (("32", "", np.float32), ("64", "64", np.float64)):
            want = g[name + "/" + theirs + suffix]
            assert want.dtype == dtype and np.isfinite(want).all()
            assert np.array_equal(o[mine + tag], want), (name, theirs, tag)


def test_run_planner_protocol_without_a_device():
    """What the planner reads off a layer, on the CPU: kind, signature, geometry, and the eligibility rules that do not
    need a device tensor."""
    from nflows_amd.transforms import MaskedAffineAutoregressiveTransform as MAF
    from nflows_amd.transforms.base import _switch_state
    F = torch.nn.functional
    assert MAF.fuse_conditioner in _switch_state()
    with torch.no_grad():
        plain = MAF(features=6, hidden_features=32).eval()
        assert plain._run_kind(None) == "k22" and plain._fused_geometry() == (8, 6, 6, 0.0)
        assert plain._run_signature() == ("k22", 6, (4, True), 0) and plain._conditioner() is plain.autoregressive_net
        assert not plain._user_hooks and plain.unconditional_transform is None
        assert MAF(6, 32, use_residual_blocks=False, num_blocks=3).eval()._conditioner_shape() == (3, False)
        for kw in (dict(activation=F.elu), dict(use_batch_norm=True), dict(hidden_features=256), dict(features=65)):
            args = dict(features=6, hidden_features=32)
            args.update(kw)
            assert MAF(**args).eval()._run_kind(None) is None, kw
        dropped = MAF(6, 32, dropout_probability=0.5)
        assert dropped.eval()._run_kind(None) == "k22" and dropped.train()._run_kind(None) is None
        assert MAF(6, 32, context_features=3).eval()._run_kind(None) is None   # a context net without a context
        assert plain._run_kind(torch.zeros(4, 3)) is None                      # a context without a context net

        class Mine(MAF):
            def _elementwise_forward(self, inputs, params):
                return super()._elementwise_forward(inputs, params)
        assert Mine(6, 32)._user_hooks
        saved = MAF.fuse_conditioner
        try:
            MAF.fuse_conditioner = False
            assert plain._run_kind(None) is None
        finally:
            MAF.fuse_conditioner = saved
    assert plain._run_kind(None) is None   # grad mode
