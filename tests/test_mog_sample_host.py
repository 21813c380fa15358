"""CPU-only checks of K30's host side (csrc/made_inverse.hip `nfa_made_mog_sample_f32`, ops.pack_mog_schedule,
nn.nde.MixtureOfGaussiansMADE.sample): the restatement of the sampler against the real reference's fixture, the packed
step blocks walked in float64 the way the kernel walks them, the entry point's argument contract, and which path a module
takes."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import mog_sample_cases as C
from nflows_amd import _native as N
from nflows_amd import ops
from nflows_amd.nn.nde import MixtureOfGaussiansMADE
from nflows_amd.nn.nde import made as made_module


def load_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "mademog_sample.npz"))
    made = MixtureOfGaussiansMADE(features=7, hidden_features=32, context_features=3, num_blocks=2,
                                  num_mixture_components=5, epsilon=C.EPSILON, custom_initialization=False)
    made.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")})
    return made.eval(), {k: torch.from_numpy(g[k]) for k in ("context", "u", "eps", "components", "samples", "samples64")}


def test_restatement_reproduces_the_reference_fixture(golden_dir):
    """The fixture's components and draws are the real reference's; its u lie in the middle of the chosen components'
    float64 CDF intervals.  The restatement with the selection rule chooses the same components, its float64 samples are the
    fixture's float64 trajectory, and its fp32 samples stand to the reference's fp32 samples under the project's parity rule."""
    made, f = load_fixture(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "mademog_sample.npz")) < 200 * 1024
    x64, c64, gap = C.restated(copy.deepcopy(made).double(), f["context"], f["u"], f["eps"])
    assert torch.equal(c64, f["components"]) and float(gap.min()) >= C.MARGIN
    want = f["samples64"]
    assert float(((x64 - want).abs() / (1.0 + want.abs())).max()) <= 1e-12
    x32, c32, _ = C.restated(made, f["context"], f["u"], f["eps"])
    assert torch.equal(c32, f["components"])
    C.assert_parity(x32.numpy(), f["samples"].numpy(), want.numpy(), "restated fp32 against the reference's samples")


@pytest.mark.parametrize("name", list(C.CASES))
def test_conditioned_inputs_terminate(name):
    r = C.reference(name)
    D, K, H, kind, ce, rows = C.CASES[name]
    assert r["rounds"] <= 16 and r["u"].shape == (rows, D) and float(r["u"].min()) >= 0.0 and float(r["u"].max()) < 1.0
    assert r["components"].min() >= 0 and r["components"].max() <= K - 1
    if K >= 5 and rows > 1:
        assert len(np.unique(r["components"])) >= 3, "the weights leave the components apart"


# ---- the packed schedule, walked in float64 -----------------------------------------------------------------------------------

def walk(schedule, x, terms, K, block_cap=None):
    """[D, K, 3] float64: what K30's loop forms from the step blocks for one sample `x` ([D] float64) -- per block the units
    in table order (dot product, bias, context term, residual add; stored rectified unless the raw bit says otherwise), on
    a step's last block the 3K output rows on the hidden vector as it stands, then "feature t found".  Asserts the format:
    the rows' order [K logits][K x (mean, ustd)] is undone here, so a packer with another order fails the comparison."""
    blocks_f, block_at, layout = schedule
    n, is_res, final_src, stream_vec, num_vectors, Hp, Xp, max_block = layout[:8]
    nblocks = block_at.numel() - 2
    assert blocks_f.numel() == int(block_at[-1]) * 256 and max_block % 256 == 0
    xs, vecs = torch.zeros(Xp, dtype=torch.float64), torch.zeros(num_vectors, Hp, dtype=torch.float64)
    out, t, raw_units, layers_seen, continuation = [], 0, 0, [], 0
    for b in range(nblocks):
        blk = blocks_f[int(block_at[b]) * 256:int(block_at[b + 1]) * 256]
        assert 256 <= blk.numel() <= max_block and (block_cap is None or blk.numel() <= block_cap)
        hdr = blk[:16].view(torch.int32)
        units, rows, out_rows, out_bias, continued = (int(v) for v in hdr[:5])
        assert rows == 16 + 8 * units and continued in (0, 1) and not hdr[5:].any()
        for i in range(units):
            e = blk[16 + 8 * i:24 + 8 * i]
            j, kp, src, dst, add_stream, stream_word, ctx_v = (int(v) for v in e[1:].view(torch.int32))
            set_stream, raw = stream_word & 1, stream_word & 2
            assert stream_word in (0, 1, 2) and 0 <= j < Hp and kp in (Xp, Hp)
            # the raw-store bit: exactly the initial layer's units in front of feed-forward blocks
            assert bool(raw) == (not is_res and src < 0), "raw-store bit"
            # context vector 1 (the initial term) on the initial layer only; residual blocks' on their first Linear
            assert (ctx_v == 1) == (src < 0) and (ctx_v == 0 or is_res or src < 0)
            raw_units += bool(raw)
            layers_seen.append(src)
            w = blk[rows:rows + kp].double()
            rows += kp
            v = float(w @ (xs[:kp] if src < 0 else vecs[src, :kp])) + float(e[0])
            if ctx_v:
                v = v + float(terms[ctx_v - 1, j])
            if add_stream:
                v = float(vecs[stream_vec, j]) + v
            if set_stream:
                vecs[stream_vec, j] = v
            if dst >= 0:
                vecs[dst, j] = v if raw else max(v, 0.0)
        assert rows == out_rows
        if continued:
            assert units >= 1 and out_bias == 0, "a continuation block carries units only"
            continuation += 1
            continue
        assert layers_seen == sorted(layers_seen), "the units of a step run in layer order across its blocks"
        layers_seen = []
        if out_bias == 0:
            assert b == nblocks - 1
            break
        assert out_bias == out_rows + 3 * K * Hp and out_bias + 3 * K <= blk.numel()
        p = blk[out_rows:out_bias].double().view(3 * K, Hp) @ vecs[final_src] + blk[out_bias:out_bias + 3 * K].double()
        out.append(torch.cat((p[:K, None], p[K:].view(K, 2)), dim=1))     # [K logits][K x (mean, ustd)] -> [K, 3]
        xs[t] = x[t]
        t += 1
    return torch.stack(out), raw_units, continuation


def _walk_case(name, cap):
    r = C.reference(name)
    made = r["made"]
    D, K, H, kind, ce, rows = C.CASES[name]
    schedule = ops.pack_mog_schedule(made, block_cap=cap)
    assert schedule is not None
    packed = ops.pack_made_context(made)
    made64 = copy.deepcopy(made).double()
    total_raw = continuation = 0
    for row in range(min(rows, 2)):
        ctx = r["context"][row:row + 1]
        terms = ops.made_mog_context_terms(ctx, packed)[0].double()
        # the initial context term is context_layer(ctx) as it is: not rectified
        want0 = made.context_layer(ctx)[0].detach()
        assert torch.allclose(terms[0, :H].float(), want0, rtol=1e-5, atol=1e-6) and bool((terms[0, :H] < 0).any())
        terms64 = torch.addmm(packed[1].double(), ctx.double(), packed[0].double().t()).view(packed[2], packed[3])
        x = torch.from_numpy(r["x64"][row])
        got, raw_units, continuation = walk(schedule, x, terms64, K, cap)
        with torch.no_grad():
            want = made64(x[None], ctx.double()).view(D, K, 3)
        assert float(((got - want).abs() / (1.0 + want.abs())).max()) <= 1e-5, name
        total_raw += raw_units
    assert (total_raw > 0) == (kind != "residual")
    return schedule, continuation


@pytest.mark.parametrize("name", list(C.CASES))
def test_packed_schedule_walks_to_the_masked_network(name):
    D, K, H, kind, ce, rows = C.CASES[name]
    made = C.reference(name)["made"]
    cap = ops.made_mog_block_cap(D, H, len(ops._made_linears(made)), len(ops.made_context_layers(made)))
    schedule, _ = _walk_case(name, cap)
    assert schedule[2][1] == int(kind == "residual")


def test_half_the_block_cap_gives_continuation_blocks():
    name = C.CONTINUATION_CASE
    plain = ops.pack_mog_schedule(C.reference(name)["made"])
    cap = plain[2][7] // 2 // 256 * 256
    schedule, continuation = _walk_case(name, cap)
    assert continuation > 0 and schedule[1].numel() > plain[1].numel() and schedule[2][7] <= cap
    # where a feature's output rows do not fit a block there is no schedule
    assert ops.pack_mog_schedule(C.reference(name)["made"], block_cap=1024) is None


# ---- the entry point without a device --------------------------------------------------------------------------------------

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer for buffers that are checked but never read


def _layout(n=5, Hp=32, Xp=16, max_block=1024, residual=1):
    layout = [n, residual, n - 1, n - 1 if residual else -1, n, Hp, Xp, max_block]
    for l in range(n):
        layout += [Xp if l == 0 else Hp, l - 1, l, 0, 0]
    return layout


def _call(lib, layout=None, bufs=None, **kw):
    p = dict(batch=64, D=8, H=32, C=0, nblocks=9, ctx=None, K=5, u=bufs, z=bufs, out=bufs)
    p.update(kw)
    layout = _layout() if layout is None else layout
    arr = (ctypes.c_int32 * len(layout))(*layout)
    return lib.nfa_made_mog_sample_f32(p["u"], p["z"], p["ctx"], p["C"], bufs, bufs, p["nblocks"], arr, len(layout), p["out"],
                                       None, p["batch"], p["D"], p["H"], p["K"], 1e-2, None)


def test_mog_sample_entry_point_contract():
    lib = N.load()
    assert "nfa_made_mog_sample_f32" in N.EXPORTS and N.ABI_VERSION == 19 and lib.nfa_abi_version() == 19
    assert _call(lib, batch=0) == N.OK
    assert _call(lib, batch=0, C=3, K=16) == N.OK and _call(lib, batch=0, K=1) == N.OK
    # null pointers
    assert _call(lib) == N.ERR_INVALID_ARGUMENT
    for missing in ("u", "z", "out"):
        assert _call(lib, bufs=DUMMY, **{missing: None}) == N.ERR_INVALID_ARGUMENT, missing
    assert _call(lib, bufs=DUMMY, C=2, ctx=None) == N.ERR_INVALID_ARGUMENT   # context vectors without their buffer
    assert lib.nfa_made_mog_sample_f32(None, None, None, 0, None, None, 9, None, 33, None, None, 0, 8, 32, 5, 1e-2, None) == \
        N.ERR_INVALID_ARGUMENT
    # bad counts, batch 0 does not hide them
    for kw in (dict(batch=-1), dict(D=0), dict(H=0), dict(C=-1), dict(C=6), dict(nblocks=8), dict(D=17), dict(H=33), dict(K=0),
               dict(K=-3)):
        assert _call(lib, **kw) == N.ERR_INVALID_ARGUMENT, kw
        if "batch" not in kw:
            assert _call(lib, batch=0, **kw) == N.ERR_INVALID_ARGUMENT, kw
    for layout in (_layout(n=0), _layout(n=13), _layout()[:-1], _layout(Hp=40), _layout(max_block=1000)):
        assert _call(lib, layout=layout, batch=0) == N.ERR_INVALID_ARGUMENT, layout
    # outside the family: more than sixteen components; more than the LDS holds
    assert _call(lib, K=17, batch=0) == N.ERR_UNSUPPORTED and _call(lib, K=17) == N.ERR_UNSUPPORTED
    assert _call(lib, layout=_layout(max_block=20480), batch=0) == N.ERR_UNSUPPORTED
    assert _call(lib, layout=_layout(Hp=512), H=512, batch=0) == N.ERR_UNSUPPORTED


# ---- which path a module takes ------------------------------------------------------------------------------------------------

class _OnDevice:
    """A float32 context that says it is on a HIP device (the gate reads attributes only)."""

    def __init__(self, t):
        self.t = t
        self.is_cuda, self.dtype, self.shape, self.device = True, t.dtype, t.shape, t.device

    def dim(self):
        return self.t.dim()


def _gate(made, context, monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _OnDevice)))
    return made._sample_kernel_serves(context)


def _made(**kw):
    args = dict(features=4, hidden_features=16, context_features=3, num_blocks=2, num_mixture_components=5)
    args.update(kw)
    return MixtureOfGaussiansMADE(**args).eval()


def test_which_path_a_module_takes(monkeypatch):
    ctx = torch.randn(6, 3)
    assert not _made()._sample_kernel_serves(ctx), "CPU: the host loop"
    on = _OnDevice(ctx)
    assert _gate(_made(), on, monkeypatch)
    assert _gate(_made(use_residual_blocks=False, random_mask=True), on, monkeypatch)
    assert not _gate(_made().double(), on, monkeypatch) and not _gate(_made(), _OnDevice(ctx.double()), monkeypatch)
    assert not _gate(_made(use_batch_norm=True), on, monkeypatch)
    dropout = _made(dropout_probability=0.3)
    assert _gate(dropout, on, monkeypatch) and not _gate(dropout.train(), on, monkeypatch)
    assert not _gate(_made(num_mixture_components=17), on, monkeypatch) and _gate(_made(num_mixture_components=16), on, monkeypatch)
    assert not _gate(_made(activation=torch.tanh), on, monkeypatch)
    # the size rule (features <=, rows >) = (16, 65 536): profiles/mog_sample_time.json
    assert MixtureOfGaussiansMADE._SAMPLE_KERNEL_LOSES == ((16, 65536),)
    many, most = _OnDevice(ctx), _OnDevice(ctx)
    many.shape, most.shape = torch.Size((65536, 3)), torch.Size((65537, 3))
    assert _gate(_made(), many, monkeypatch) and not _gate(_made(), most, monkeypatch)
    assert not _gate(_made(features=16), most, monkeypatch) and _gate(_made(features=17), most, monkeypatch)
    off = _made()
    monkeypatch.setattr(MixtureOfGaussiansMADE, "_use_sample_kernel", False)
    assert not _gate(off, on, monkeypatch)


def test_switch_reads_the_environment():
    import subprocess
    import sys
    code = "from nflows_amd.nn.nde import MixtureOfGaussiansMADE as M; print(int(M._use_sample_kernel))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("0", "0"), ("1", "1")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NFA_K30=value), cwd=root,
                             capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_cpu_sample_is_the_host_loop_with_the_reference_stream(monkeypatch):
    """On the CPU nothing of the kernel path runs (the op raises if it is reached) and the random stream is the loop's."""
    monkeypatch.setattr(ops, "made_mog_sample", lambda *a, **k: pytest.fail("the kernel path on the CPU"))
    made = _made()
    ctx = torch.randn(5, 3)
    torch.manual_seed(5)
    a = made.sample(3, context=ctx)
    torch.manual_seed(5)
    b = made.sample(3, context=ctx)
    assert a.shape == (5, 3, 4) and torch.equal(a, b)


def test_kernel_path_draws_rand_then_randn_once_each(monkeypatch):
    """With the op stubbed out: one `torch.rand(B, D)`, then one `torch.randn(B, D)`, on the context's device, and the
    op's result reshaped to [N, num_samples, D]."""
    made = _made()
    ctx = torch.randn(5, 3)
    calls, seen = [], {}
    rand_was, randn_was = torch.rand, torch.randn

    def rand(*a, **k):
        calls.append(("rand", tuple(a[0]) if len(a) == 1 else a, k.get("device")))
        return rand_was(*a, **k)

    def randn(*a, **k):
        calls.append(("randn", tuple(a[0]) if len(a) == 1 else a, k.get("device")))
        return randn_was(*a, **k)

    def op(uniforms, normals, schedule, hidden_features, num_components, epsilon, context_terms=None, want_components=False):
        seen.update(u=uniforms, z=normals, terms=context_terms, args=(hidden_features, num_components, epsilon))
        return uniforms + 2.0 * normals

    monkeypatch.setattr(made_module.torch, "rand", rand)
    monkeypatch.setattr(made_module.torch, "randn", randn)
    monkeypatch.setattr(ops, "made_mog_sample", op)
    monkeypatch.setattr(MixtureOfGaussiansMADE, "_sample_kernel_serves", lambda self, context: True)
    torch.manual_seed(11)
    out = made.sample(3, context=ctx)
    assert calls == [("rand", (15, 4), ctx.device), ("randn", (15, 4), ctx.device)]
    torch.manual_seed(11)
    u = rand_was(15, 4)
    z = randn_was(15, 4)
    assert torch.equal(seen["u"], u) and torch.equal(seen["z"], z) and seen["args"] == (16, 5, made.epsilon)
    assert out.shape == (5, 3, 4) and torch.equal(out, (u + 2.0 * z).reshape(5, 3, 4))
    # the context terms: the repeated rows through the raw initial Linear and the residual blocks' Linears
    rep = ctx.repeat_interleave(3, dim=0)
    assert seen["terms"].shape == (15, 3, 16)
    assert torch.allclose(seen["terms"][:, 0], made.context_layer(rep), atol=1e-6)
    assert torch.allclose(seen["terms"][:, 2], made.blocks[1].context_layer(rep), atol=1e-6)
    # the plan is cached until a weight changes
    plan = made._sample_kernel_plan()
    assert made._sample_kernel_plan() is plan
    with torch.no_grad():
        made.final_layer.weight.mul_(2.0)
    again = made._sample_kernel_plan()
    assert again is not plan and not torch.equal(again[0][0], plan[0][0])
    with torch.no_grad():
        made.initial_layer.mask.zero_()
    assert made._sample_kernel_plan() is not again
