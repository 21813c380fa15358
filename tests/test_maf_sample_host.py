"""CPU-only checks of K23's host side (csrc/made_inverse.hip `nfa_made_affine_inverse_f32`, ops.pack_made_schedule with a
block cap and context vectors): the restatement of the inverse against the real reference's fixture, the packed step
blocks walked the way the kernel walks them, the entry point's argument contract, and the packer's unchanged output for
K12's call."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import maf_cases
import maf_inverse_cases as inv
from nflows_amd import _native as N
from nflows_amd import ops


@pytest.mark.parametrize("name", list(maf_cases.CASES))
def test_restated_inverse_reproduces_the_reference_pairs(golden_dir, name):
    """The fixture's pairs (x, z64, lad64) are the real reference's.  Inverting z64 rounded to fp32 with the restatement in
    float64 gives x and -lad back; what is left is the rounding of z, which the restatement's own fp32 error on the same
    rows bounds: mean within 2 x, maximum within 4 x."""
    g = maf_cases.load(golden_dir)
    flow = maf_cases.build(name, g)
    z = torch.from_numpy(g[name + "/z64"]).float()
    context = torch.from_numpy(g[name + "/context"]) if name + "/context" in g.files else None
    o = inv.inverse_pair(flow, z, context)
    for got, own32, want, what in ((o["x64"], o["x32"], g[name + "/x"].astype(np.float64), "x"),
                                   (o["lad64"], o["lad32"], -g[name + "/lad64"], "lad")):
        assert np.isfinite(got).all() and np.isfinite(own32).all()
        left, own = np.abs(got - want), np.abs(own32.astype(np.float64) - got)
        print(name, what, "restatement fp64 vs the fixture: mean %.3e max %.3e; its fp32 vs its fp64: mean %.3e q999 %.3e "
              "max %.3e" % (left.mean(), left.max(), own.mean(), np.quantile(own, 0.999), own.max()))
        assert left.mean() <= 2.0 * own.mean() and left.max() <= 4.0 * own.max(), (name, what)
    assert np.abs(o["x64"]).max() <= 5.1   # the inputs of the GPU tests stay small


def _net(features, hidden, blocks, residual, random_mask, ce, seed):
    from nflows_amd.transforms import made
    torch.manual_seed(seed)
    net = made.MADE(features=features, hidden_features=hidden, context_features=ce, num_blocks=blocks, output_multiplier=2,
                    use_residual_blocks=residual, random_mask=random_mask)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
    return net


def _context_terms(net, context):
    packed = ops.pack_made_context(net)
    if packed is None:
        return None
    with torch.no_grad():
        return ops.made_context_terms(context[None], packed)[0].double()


WALKS = [
    # residual, random masks, features, hidden, blocks, context features
    (True, False, 6, 32, 2, None),
    (True, False, 3, 40, 2, 5),       # wide steps: continuation blocks; padded columns (40 -> 48)
    (False, False, 5, 24, 3, 4),      # feed-forward blocks ignore the context beyond the initial layer
    (False, True, 9, 16, 2, None),    # random masks: degrees missing in some layer, steps with no units
    (False, True, 7, 20, 1, 3),
    (True, False, 2, 16, 1, 2),       # D = 2: every hidden unit has degree 1
    (True, False, 4, 16, 0, 3),       # no blocks
    (False, False, 17, 8, 2, None),   # fewer hidden units than degrees
]


@pytest.mark.parametrize("residual, random_mask, features, hidden, blocks, ce", WALKS)
def test_affine_schedule_reproduces_the_masked_network(residual, random_mask, features, hidden, blocks, ce):
    """The affine schedule (P = 2, T = D) walked like the kernel in float64: every feature's two parameters equal the
    masked network's on the features before it, context included -- with one block per step, and with every block cap
    down to the smallest that still packs, among them caps that cut a step into two and into three blocks."""
    net = _net(features, hidden, blocks, residual, random_mask, ce, seed=features * 7 + hidden)
    x = torch.randn(features, dtype=torch.float64)
    context = None if ce is None else torch.randn(ce)
    terms = _context_terms(net, context)
    with torch.no_grad():
        want = net.double()(x[None], None if ce is None else context.double()[None])[0].view(features, 2)
        net = net.float()
        whole = ops.pack_made_schedule(net, features, 2, context=True)
    assert whole[1].numel() == features + 3
    params, continuation, final_vec = inv.walk_schedule(whole, x, terms)
    assert params.shape == (features, 2) and continuation == [0] * features
    assert (params - want).abs().max().item() < 1e-5 * (1 + want.abs().max().item())
    with torch.no_grad():
        hidden_want = net.double().hidden(x[None], None if ce is None else context.double()[None])[0]
        net = net.float()
    assert (final_vec[:hidden] - hidden_want).abs().max().item() < 1e-5 * (1 + hidden_want.abs().max().item())
    seen = set()
    for cap in range(whole[2][7], 0, -256):
        cut = ops.pack_made_schedule(net, features, 2, block_cap=cap, context=True)
        if cut is None:
            break
        assert cut[2][7] <= cap and cut[2][:7] == whole[2][:7] and cut[2][8:] == whole[2][8:]
        p2, c2, f2 = inv.walk_schedule(cut, x, terms, block_cap=cap)
        assert torch.equal(p2, params) and torch.equal(f2, final_vec), cap    # the same numbers in the same order
        assert cut[1].numel() - 2 == features + 1 + sum(c2)
        seen.add(max(c2))
    assert seen, "no cap was tried"
    if hidden * (1 + blocks) >= 8 * max(1, features - 1):   # (steps wide enough to be cut twice at the 1 KB grain)
        assert 0 in seen and max(seen) >= 2, seen
    # a cap below one unit's row, or below the output rows, has no schedule
    assert ops.pack_made_schedule(net, features, 2, block_cap=0, context=True) is None


def test_steps_are_cut_into_two_and_three_blocks():
    """The shape of the wide-step case above, looked at directly: D = 3, H = 40, five Linears -- 20 units per Linear
    and step."""
    net = _net(3, 40, 2, True, False, 5, seed=1)
    whole = ops.pack_made_schedule(net, 3, 2, context=True)
    counts = {}
    for cap in range(whole[2][7], 0, -256):
        cut = ops.pack_made_schedule(net, 3, 2, block_cap=cap, context=True)
        if cut is None:
            break
        counts[cap] = inv.walk_schedule(cut, torch.zeros(3, dtype=torch.float64), torch.zeros(3, 48, dtype=torch.float64), cap)[1]
    assert any(max(c) == 1 for c in counts.values()) and any(max(c) == 2 for c in counts.values()), counts


def test_lds_budget_of_the_fixture_shapes():
    """The arithmetic of the issue: d6_l5 (D = 6, H = 128, five Linears) has 44 KB of state and one step of about 60 KB, so
    two whole steps do not fit and the step is cut; hidden 512 with two residual blocks has no room at all."""
    assert ops.made_state_bytes(6, 128, 5) == (16 + 5 * 32) * 4 * 16 * 4 == 45056
    cap = ops.made_block_cap(6, 128, 5)
    assert cap * 4 == (ops.MADE_LDS_BYTES - 45056) // 2 // 1024 * 1024
    net = maf_cases.build("d6_l5")._transform._transforms[-1].autoregressive_net
    whole = ops.pack_made_schedule(net, 6, 2, context=True)
    assert whole[2][7] * 4 > 56 * 1024 and 2 * whole[2][7] * 4 + 45056 > ops.MADE_LDS_BYTES
    cut = ops.pack_made_schedule(net, 6, 2, block_cap=cap, context=True)
    assert cut is not None and cut[2][7] <= cap and cut[1].numel() - 2 > 7
    assert ops.made_block_cap(8, 512, 5) <= 0
    assert ops.made_block_cap(21, 64, 5, 3) > 0


def test_context_vectors_are_named_in_the_spare_word():
    net = _net(4, 16, 2, True, False, 3, seed=2)
    blocks_f, block_at, layout = ops.pack_made_schedule(net, 4, 2, context=True)

    def named(schedule):
        blocks_f, block_at, _ = schedule
        found = {}
        for b in range(block_at.numel() - 2):
            blk = blocks_f[int(block_at[b]) * 256:int(block_at[b + 1]) * 256]
            for u in range(int(blk[:1].view(torch.int32))):
                e = blk[16 + 8 * u:24 + 8 * u].view(torch.int32)
                found.setdefault(int(e[3]), set()).add(int(e[7]))   # source vector -> context vector
        return found
    assert named(ops.pack_made_schedule(net, 4, 2, context=True)) == {-1: {1}, 0: {2}, 1: {0}, 2: {3}, 3: {0}}
    plain = _net(4, 16, 2, True, False, None, seed=2)
    assert named(ops.pack_made_schedule(plain, 4, 2, context=True)) == {v: {0} for v in range(-1, 4)}
    assert ops.pack_made_context(plain) is None
    w, b, vectors, Hp = ops.pack_made_context(net)
    assert (vectors, Hp) == (3, 16) and w.shape == (48, 3) and b.shape == (48,)


# ---- the entry point without a device ---------------------------------------------------------------------------------------

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer for buffers that are checked but never read


def _layout(n=5, Hp=32, Xp=16, max_block=1024, residual=1):
    layout = [n, residual, n - 1, n - 1 if residual else -1, n, Hp, Xp, max_block]
    for l in range(n):
        layout += [Xp if l == 0 else Hp, l - 1, l, 0, 0]
    return layout


def _call(lib, layout=None, bufs=None, **kw):
    p = dict(batch=64, D=8, H=32, C=0, nblocks=9, ctx=None)
    p.update(kw)
    layout = _layout() if layout is None else layout
    arr = (ctypes.c_int32 * len(layout))(*layout)
    return lib.nfa_made_affine_inverse_f32(bufs, p["ctx"], p["C"], bufs, bufs, p["nblocks"], arr, len(layout), bufs, bufs,
                                           p["batch"], p["D"], p["H"], None)


def test_affine_inverse_entry_point_contract():
    lib = N.load()
    assert "nfa_made_affine_inverse_f32" in N.EXPORTS
    assert _call(lib, batch=0) == N.OK
    assert _call(lib, batch=0, C=3) == N.OK
    # null pointers
    assert _call(lib) == N.ERR_INVALID_ARGUMENT
    assert _call(lib, bufs=DUMMY, C=2, ctx=None) == N.ERR_INVALID_ARGUMENT   # context vectors without their buffer
    assert lib.nfa_made_affine_inverse_f32(None, None, 0, None, None, 9, None, 33, None, None, 0, 8, 32, None) == \
        N.ERR_INVALID_ARGUMENT
    # bad sizes and layouts, batch 0 does not hide them
    for kw in (dict(batch=-1), dict(D=0), dict(H=0), dict(C=-1), dict(C=6), dict(nblocks=8), dict(D=17), dict(H=33)):
        assert _call(lib, **kw) == N.ERR_INVALID_ARGUMENT, kw
        if "batch" not in kw:
            assert _call(lib, batch=0, **kw) == N.ERR_INVALID_ARGUMENT, kw
    for layout in (_layout(n=0), _layout(n=13), _layout()[:-1], _layout(Hp=40), _layout(Xp=8), _layout(max_block=1000),
                   _layout(max_block=0), _layout()[:2] + [7] + _layout()[3:], _layout()[:3] + [9] + _layout()[4:]):
        assert _call(lib, layout=layout, batch=0) == N.ERR_INVALID_ARGUMENT, layout
    # more than the LDS holds: two blocks of 80 KB; the state of hidden 512 with five Linears; context vectors on top
    assert _call(lib, layout=_layout(max_block=20480), batch=0) == N.ERR_UNSUPPORTED
    assert _call(lib, layout=_layout(Hp=512), H=512, batch=0) == N.ERR_UNSUPPORTED
    fits = _layout(Hp=256, max_block=4096)
    assert _call(lib, layout=fits, H=256, batch=0) == N.OK
    assert _call(lib, layout=fits, H=256, batch=0, C=5) == N.ERR_UNSUPPORTED
    # K12's entry point answers as before
    spec = ops.make_rqs_spec(8, "linear", tail_bound=3.0)
    arr = (ctypes.c_int32 * 33)(*_layout())
    rqs = lib.nfa_made_rqs_inverse_f32
    assert rqs(None, None, None, arr, 33, None, None, None, None, 0, 8, 32, 8, ctypes.byref(spec), None) == N.OK
    assert rqs(None, None, None, arr, 33, None, None, None, None, 64, 8, 32, 8, ctypes.byref(spec), None) == \
        N.ERR_INVALID_ARGUMENT
    arr = (ctypes.c_int32 * 33)(*_layout(max_block=20480))
    assert rqs(None, None, None, arr, 33, None, None, None, None, 0, 8, 32, 8, ctypes.byref(spec), None) == N.ERR_UNSUPPORTED


# ---- K12's call of the packer -------------------------------------------------------------------------------------------------

def _exact_net(residual):
    """A MADE whose parameters are small dyadic numbers (no random draw, no library function: the same bits everywhere)."""
    from nflows_amd.transforms import made
    net = made.MADE(features=7, hidden_features=20, num_blocks=2, output_multiplier=5, use_residual_blocks=residual)
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            k = torch.arange(p.numel(), dtype=torch.float64)
            p.copy_((((k * 37 + 11 * i) % 101 - 50) / 64).view(p.shape))
    return net


def _digest(schedule):
    blocks_f, block_at, layout = schedule
    h = hashlib.sha256()
    h.update(blocks_f.cpu().numpy().tobytes())
    h.update(block_at.cpu().numpy().tobytes())
    h.update(np.asarray(layout, dtype=np.int64).tobytes())
    return h.hexdigest()


PARENT_DIGESTS = {True: "f63e309566e40f26d033d0e5a83a9bcdb83df1249df7e6b88b54b42395e6dfea", False: "123c03ecf4f7d1e20d9821440e21435793e35c8afb92e054ad981d9a8276f42e"}


@pytest.mark.parametrize("residual", [True, False])
def test_todays_call_of_the_packer_is_unchanged(residual):
    """`pack_made_schedule(net, T, P)` returns what it returned before the keywords existed (the digests were taken from
    that version), and the slice-wise packer behind the keywords builds the same bytes when nothing is asked of it."""
    net = _exact_net(residual)
    old = ops.pack_made_schedule(net, 6, 5)
    assert old[0].dtype == torch.float32 and old[1].dtype == torch.int32 and old[1].numel() == 9
    assert _digest(old) == PARENT_DIGESTS[residual]
    new = ops._pack_made_blocks(net, 6, 5, None, False)
    assert torch.equal(old[0].view(torch.int32), new[0].view(torch.int32)) and torch.equal(old[1], new[1]) and old[2] == new[2]
    assert _digest(ops.pack_made_schedule(net, 6, 5, block_cap=old[2][7])) == PARENT_DIGESTS[residual]
