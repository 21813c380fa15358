"""K1-backward (`nfa_rqs_coupling_backward_f32`, nflows_amd/csrc/rqs_bwd.hip) on the GPU.

The arithmetic: the case table and the rules of tests/k1_backward_cases.py, which tests/test_k1_backward_host.py applies to
the host build of `rqs_backward` -- every case laid out as `RqsElementwise` (one spline per sample, the generic kernel) and
as a coupling layer of 16 features (alternating mask and K = 8: the pipelined kernel), bit-equal per spline, and held to
the float64 gradient per row.

The launch code, shown from outside that each path ran (R, C and the LDS image come from the host build of the planner,
tests/launch_plan_shim.py; the grids from the device's CU count as the launcher computes them): pipelined against
generic, tile tails, later passes of both persistent loops, the chunked path and a halved R, misaligned stores, every
element written, absent upstream gradients, permutations.  The yardstick of a launch test is the D = 1 layout of the same
splines, the one the table holds to float64: a layout is correct when it is bit-equal to it.  Indices are valid and
sizes are ones the planner accepts.  Run with -s for the per-case figures.  Needs an MI355X: `-m gpu`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cdf_shared_cases
import k1_backward_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c.name for c in kc.CASES]
D_LAYER, DT_LAYER = 16, kc.ROW_SPLINES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    import nflows_amd
    from nflows_amd import ops as o
    assert os.path.exists(nflows_amd.native_library_path())
    return o


def take_status(ops):
    """The device status word (read and cleared)."""
    w = ops._status_word(torch.device(DEV))
    bits = int(w.item())
    w.zero_()
    return bits


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def plan(D, dt, P, batch):
    """The tile K1-backward takes: {ok, R, C, lds} from the host build of the planner."""
    out = (ctypes.c_int64 * 8)()
    cdf_shared_cases.shim().k1_backward(D, dt, P, batch, out)
    return dict(ok=int(out[0]), R=int(out[1]), C=int(out[2]), lds=int(out[3]))


def pipelined(D, dt, P, R, batch):
    return bool(cdf_shared_cases.shim().aligned(dt, D, P, R, batch))


def grid_limit(pl, pipeline):
    """Workgroups of the persistent grid when there are more tiles than that: 3 x CUs (pipelined), min(6, LDS) x CUs."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * (3 if pipeline else max(1, min(6, (160 * 1024) // (pl["lds"] + 256))))


def params_per_spline(spec):
    from nflows_amd import _native as N
    return 3 * spec.num_bins + (-1 if spec.tails == N.TAILS_LINEAR else 1)


def backward(ops, x, params, tidx, gout, glad, spec, inverse, perm=None, scat=None, gin=None, gparams=None):
    """The kernel's entry point as nflows_amd/autograd.py calls it, on buffers of the caller's choosing (contiguous
    [B, D] / [B, dt P] tensors or views).  Returns (grad_inputs, grad_params)."""
    from nflows_amd import _native as N
    B, D = x.shape
    assert x.is_contiguous() and params.is_contiguous() and gout.is_contiguous() and gout.shape == x.shape
    assert params.shape == (B, tidx.numel() * params_per_spline(spec)) and (glad is None or glad.shape == (B,))
    assert int(tidx.min()) >= 0 and int(tidx.max()) < D
    for p in (perm, scat):
        assert p is None or sorted(p.tolist()) == list(range(D))
    gin = torch.empty_like(x) if gin is None else gin
    gparams = torch.empty_like(params) if gparams is None else gparams
    assert gin.is_contiguous() and gin.shape == x.shape and gparams.is_contiguous() and gparams.shape == params.shape
    with torch.cuda.device(x.device):
        rc = N.load().nfa_rqs_coupling_backward_f32(
            N.ptr(x), N.ptr(params), N.ptr(tidx), N.ptr(perm), N.ptr(scat), N.ptr(gout), N.ptr(glad), N.ptr(gin), N.ptr(gparams),
            N.ptr(ops._status_word(x.device)), B, D, tidx.numel(), ctypes.byref(spec), N.FLAG_INVERSE if inverse else 0,
            N.stream_handle(x.device))
    N.check(rc)
    return gin, gparams


def by_splines(ops, x, params, tidx, gout, glad, spec, inverse, perm=None, scat=None):
    """What a layer's backward has to return, from the D = 1 layout: every spline of the layer as a sample of its own
    through the same entry point (the layout test_table holds to float64), put together on the host side of the
    kernel's index arithmetic: out[:, scat[c]] = f(in[:, perm[c]]), identity columns copied."""
    B, D = x.shape
    dt, P = tidx.numel(), params_per_spline(spec)
    src = torch.arange(D, device=x.device) if perm is None else perm
    dst = torch.arange(D, device=x.device) if scat is None else scat
    xs = x[:, src[tidx]].reshape(-1, 1).contiguous()
    gy = gout[:, dst[tidx]].reshape(-1, 1).contiguous()
    gl = None if glad is None else glad.repeat_interleave(dt).contiguous()
    col0 = torch.zeros(1, dtype=torch.int64, device=x.device)
    gx, gp = backward(ops, xs, params.reshape(B * dt, P).contiguous(), col0, gy, gl, spec, inverse)
    gin = torch.empty_like(x)
    gin[:, src] = gout[:, dst]            # pass-through columns (the transformed ones are overwritten next)
    gin[:, src[tidx]] = gx.view(B, dt)
    return gin, gp.view(B, dt * P)


def layer_tensors(p, tidx, D, rng):
    """The splines of a prepared case as rows of a layer: (x [B, D], params [B, dt P], gout [B, D], glad [B]); identity
    columns are N(0, 1).  The case's wl is constant over the splines of a row (k1_backward_cases.weights)."""
    dt = len(tidx)
    n = (p["x"].size // dt) * dt
    B = n // dt
    x, gout = rng.randn(B, D).astype(np.float32), rng.randn(B, D).astype(np.float32)
    x[:, tidx], gout[:, tidx] = p["x"][:n].reshape(B, dt), p["wy"][:n].reshape(B, dt)
    params = kc.packed(p["uw"], p["uh"], p["ud"])[:n].reshape(B, -1)
    wl = p["wl"][:n].reshape(B, dt)
    assert (wl == wl[:, :1]).all()
    return x, params, gout, np.ascontiguousarray(wl[:, 0])


ALTERNATING = list(range(1, D_LAYER, 2))
RANDOM_MASK = sorted(np.random.RandomState(16).permutation(D_LAYER)[:DT_LAYER].tolist())


# ----------------------------------------------------------------------------------------------------- the table
def elementwise_gradients(ops, case, p):
    """[gx [n], gparams [n, P]] through autograd on `ops.rqs_elementwise` (RqsElementwise: features = 1)."""
    x, uw, uh, ud = (dev(p[k]).requires_grad_(True) for k in ("x", "uw", "uh", "ud"))
    y, lad = ops.rqs_elementwise(x, uw, uh, ud, kc.product_spec(case), case.inverse)
    loss = (y * dev(p["wy"])).sum() if case.loss == "y" else (lad * dev(p["wl"])).sum() if case.loss == "lad" else \
        (y * dev(p["wy"])).sum() + (lad * dev(p["wl"])).sum()
    loss.backward()
    return [x.grad, torch.cat([uw.grad, uh.grad, ud.grad], dim=1)]


def layer_gradients(ops, case, p, tidx):
    """The same splines as a coupling layer of D_LAYER features through autograd on `ops.rqs_coupling`: [gx [n],
    gparams [n, P]] per spline, and (grad_inputs, grad_outputs) for the identity columns."""
    x, params, gout, wl = layer_tensors(p, tidx, D_LAYER, np.random.RandomState(case.seed + 7))
    x, params = dev(x).requires_grad_(True), dev(params).requires_grad_(True)
    y, lad = ops.rqs_coupling(x, params, dev(np.array(tidx, dtype=np.int64)), kc.product_spec(case), inverse=case.inverse)
    loss = (y * dev(gout)).sum() if case.loss == "y" else (lad * dev(wl)).sum() if case.loss == "lad" else \
        (y * dev(gout)).sum() + (lad * dev(wl)).sum()
    loss.backward()
    return [x.grad[:, tidx].reshape(-1), params.grad.reshape(p["x"].size, -1)], (x.grad, gout)


@pytest.mark.parametrize("name", NAMES)
def test_table(ops, name):
    """Every case through the kernel in two or three layouts: D = 1 (generic kernel), D = 16 with the alternating mask
    (K = 8: pipelined; other K: generic) and, for K = 8, D = 16 with a random mask (generic).  Per spline the layouts
    agree bit for bit -- they run the same `rqs_backward` and the build has no floating-point contraction -- and the
    D = 1 layout is held to the rule at the cap of the case's group; the layer's identity columns carry the upstream
    gradient bit for bit.  A loss on y alone or on lad alone (the `_loss_` cases) reaches the kernel through autograd
    with one upstream gradient absent or zero."""
    case, p = kc.BY_NAME[name], kc.prepared(name)
    P = params_per_spline(kc.product_spec(case))
    B = kc.ROWS // DT_LAYER
    pl = plan(D_LAYER, DT_LAYER, P, B)
    if case.K == 8:     # (the launcher's other condition for the pipelined kernel; all buffers come from the allocator)
        assert pl["C"] == 0 and pl["R"] == 32 and pipelined(D_LAYER, DT_LAYER, P, pl["R"], B)
    got = elementwise_gradients(ops, case, p)
    assert take_status(ops) == 0
    share = kc.assert_rows([host(t) for t in got], p, kc.GRAD_CAP[(case.tails, case.inverse)], what=name, verbose=True)
    for tidx in [ALTERNATING] + ([RANDOM_MASK] if case.K == 8 else []):
        layer, (gin, gout) = layer_gradients(ops, case, p, tidx)
        assert take_status(ops) == 0
        differ = [int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum()) for a, b in zip(layer, got)]
        print("%-44s mask %s: %d + %d entries differ from the D = 1 layout; rows outside %.4f %%" % (
            name, "alternating" if tidx is ALTERNATING else "random", differ[0], differ[1], 100.0 * share))
        assert differ == [0, 0], (name, tidx, differ)
        identity = [c for c in range(D_LAYER) if c not in tidx]
        expect = dev(gout)[:, identity] if case.loss != "lad" else torch.zeros(gin.shape[0], len(identity), device=DEV)
        assert bits_equal(gin[:, identity], expect), name


@pytest.mark.parametrize("name", kc.KNOT_CASES)
def test_inputs_on_the_knots(ops, name):
    """The knot fixture (inputs on every knot, its fp32 neighbours, the box ends and one ulp beyond) through the entry
    point directly -- the functional raises on the box's outside inputs before a backward could run --: either-side
    rule at twice the reference's own share, identity and NFA_STATUS_OUTSIDE_DOMAIN outside."""
    pk = kc.prepared_knots(name)
    case = pk["case"]
    col0 = torch.zeros(1, dtype=torch.int64, device=DEV)
    gx, gp = backward(ops, dev(pk["x"]).view(-1, 1), dev(kc.packed(pk["uw"], pk["uh"], pk["ud"])), col0, dev(pk["wy"]).view(-1, 1),
                      dev(pk["wl"]), kc.product_spec(case), case.inverse)
    kc.assert_knot_rows([host(gx).reshape(-1), host(gp)], take_status(ops), pk, kc.KNOT_CAP[name], what=name, verbose=True)


@pytest.mark.parametrize("inverse", [False, True])
def test_derivative_logit_below_minus_88_gives_zero_not_nan(ops, inverse):
    """The inputs of test_k1_backward_host.py's test of the same name (K = 2, unit box, derivative logits at scale 25;
    row 4092 has one of -116.5, where the derivative of softplus was 1 / (1 + NaN)): the non-finite pattern of the
    kernel's gradients is the one of the reference's fp32 autograd, and that entry is zero."""
    case = kc.Case("probe", 2, False, inverse, kc.UNIT, 0.0, 3.0, 25.0, False, None, "both", 0)
    p = kc.probe_inputs(0)
    ref = kc.autograd_gradients(case, *(p[k] for k in ("x", "uw", "uh", "ud", "wy", "wl")), np.float32)
    got = [host(t) for t in elementwise_gradients(ops, case, p)]
    assert take_status(ops) == 0
    n = p["x"].size
    assert np.array_equal(kc.nonfinite_pattern(got, n), kc.nonfinite_pattern(ref, n))
    assert got[1][4092, 4] == 0.0


@pytest.mark.parametrize("K,tails", [(8, True), (2, False)])
def test_extreme_derivative_logits(ops, K, tails):
    """test_k1_backward_host.py's test_nan_pattern_with_extreme_derivative_logits through the kernel: derivative logits
    at -120 .. 120 on both sides of every threshold of softplus and its derivative, with and without the identity
    initialisation, both directions -- the reference's non-finite pattern, and the rule at twice the reference's own
    share on these inputs (at least 0.5 %, five rows of 1024)."""
    values = np.array([-120.0, -104.0, -90.0, -88.0, -87.0, -86.0, -21.0, 21.0, 30.0, 120.0], dtype=np.float32)
    for inverse in (False, True):
        for ident in (False, True):
            case = kc.Case("extreme", K, tails, inverse, None if tails else kc.UNIT, 0.0, 1.5, 1.5, ident, None, "both", 8800 + K)
            x, uw, uh, ud = kc.inputs(case, 1024)
            ud[:] = values[np.random.RandomState(5).randint(0, values.size, size=ud.shape)]
            wy, wl = kc.weights(case, 1024)
            p = kc.truth_for(case, x, uw, uh, ud, wy, wl)
            p.update(x=x, uw=uw, uh=uh, ud=ud, wy=wy, wl=wl, outside=kc.outside_box(case, x))
            got = [host(t) for t in elementwise_gradients(ops, case, p)]
            assert take_status(ops) == 0
            assert np.array_equal(kc.nonfinite_pattern(got, 1024), kc.nonfinite_pattern(p["ref"], 1024)), (inverse, ident)
            rbad, rkeep = kc.rows_outside(p["ref"], p)
            kc.assert_rows(got, p, max(2.0 * rbad[rkeep].mean(), 5e-3), what="extreme K=%d inverse=%d ident=%d" % (K, inverse, ident),
                           verbose=True)


# ---------------------------------------------------------------------------------------------------- launch code
def random_layer(K, tails, D, tidx, B, seed, scale=1.5):
    """A layer of random splines at the table's mild scale: spec, x, params, gout, glad (numpy) -- inputs over the box,
    with tails one in twenty beyond it."""
    case = kc.Case("layer", K, tails, False, None if tails else kc.UNIT, 0.0, scale, scale, False, None, "both", seed)
    dt = len(tidx)
    xs, uw, uh, ud = kc.inputs(case, B * dt)
    rng = np.random.RandomState(seed + 1)
    x = (rng.rand(B, D) if not tails else 3.0 * (2.0 * rng.rand(B, D) - 1.0)).astype(np.float32)
    x[:, tidx] = xs.reshape(B, dt)
    gout, glad = rng.randn(B, D).astype(np.float32), rng.randn(B).astype(np.float32)
    return kc.product_spec(case), x, kc.packed(uw, uh, ud).reshape(B, -1), gout, glad


def shifted(t, floats):
    """A contiguous copy of `t` whose storage starts `floats` floats past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("tails", [True, False])
@pytest.mark.parametrize("inverse", [False, True])
def test_pipelined_against_generic(ops, tails, inverse):
    """K = 8, D = 16, alternating mask, 2 R + 5 rows: with every buffer on a 16-byte boundary the full tiles take the
    pipelined kernel (and the 5 leftover rows the generic one on a grid of 1); with the parameter buffer 4 bytes further
    `aligned16` fails and the generic kernel takes everything.  Same bits, and the bits of the D = 1 layout."""
    tidx = dev(np.array(ALTERNATING, dtype=np.int64))
    P = 23 if tails else 25
    R = plan(D_LAYER, DT_LAYER, P, 1 << 20)["R"]
    B = 2 * R + 5
    assert R == 32 and pipelined(D_LAYER, DT_LAYER, P, R, B)
    spec, x, params, gout, glad = (a if i == 0 else dev(a) for i, a in enumerate(random_layer(8, tails, D_LAYER, ALTERNATING, B, 300)))
    assert all(t.data_ptr() % 16 == 0 for t in (x, params, gout))
    a = backward(ops, x, params, tidx, gout, glad, spec, inverse)
    b = backward(ops, x, shifted(params, 1), tidx, gout, glad, spec, inverse)
    want = by_splines(ops, x, params, tidx, gout, glad, spec, inverse)
    assert take_status(ops) == 0
    for got in (a, b):
        assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])


@pytest.mark.parametrize("shape", ["pipelined", "generic"])
def test_batches_around_a_tile(ops, shape):
    """1, R - 1, R, R + 1 and 2 R + 1 rows: row for row the bits of the D = 1 layout of the same splines, so every batch
    agrees with every slice of every other.  Pipelined shape (D = 16, K = 8): below R rows the tile shrinks to the batch,
    at R + 1 and 2 R + 1 the leftover row goes to the generic kernel.  Generic shape: D = 9, 5 of them transformed, K = 5."""
    if shape == "pipelined":
        K, D, mask = 8, D_LAYER, ALTERNATING
    else:
        K, D, mask = 5, 9, [0, 2, 3, 6, 8]
    P = 3 * K - 1
    R = plan(D, len(mask), P, 1 << 20)["R"]
    assert R == 256 // len(mask)
    tidx = dev(np.array(mask, dtype=np.int64))
    spec, x, params, gout, glad = (a if i == 0 else dev(a) for i, a in enumerate(random_layer(K, True, D, mask, 2 * R + 1, 310)))
    want = by_splines(ops, x, params, tidx, gout, glad, spec, True)
    for B in (1, R - 1, R, R + 1, 2 * R + 1):
        pl = plan(D, len(mask), P, B)
        assert pl["R"] == min(R, B) and pl["C"] == 0 and pipelined(D, len(mask), P, pl["R"], B) == (shape == "pipelined")
        gin, gp = backward(ops, x[:B].contiguous(), params[:B].contiguous(), tidx, gout[:B].contiguous(), glad[:B].contiguous(), spec, True)
        assert bits_equal(gin, want[0][:B]) and bits_equal(gp, want[1][:B]), (shape, B)
    assert take_status(ops) == 0


def assert_repeats(t, block, what):
    """Every repetition of the block inside `t` (and the partial one at the end) equals `block` bit for bit."""
    t, block = t.contiguous().view(torch.int32), block.contiguous().view(torch.int32)
    rows = block.shape[0]
    full = t.shape[0] // rows
    assert torch.equal(t[:full * rows].view((full, rows) + tuple(t.shape[1:])), block.unsqueeze(0).expand((full, rows) + tuple(t.shape[1:]))), what
    assert torch.equal(t[full * rows:], block[:t.shape[0] - full * rows]), what


BLOCK_ROWS = {"pipelined": 227, "generic": 359}     # primes: see test_later_passes_of_the_persistent_loop


@pytest.mark.parametrize("shape", ["pipelined_fwd", "pipelined_inv", "generic"])
def test_later_passes_of_the_persistent_loop(ops, shape):
    """(2 g + 3) R + 7 rows, g the grid the launcher computes: every workgroup takes a second tile, most a third; the
    pipelined kernel's register-carried next tile is then a real one, and the generic kernel's per-tile store offset
    changes from tile to tile (D = 9: R x D = 459 floats is no multiple of 4).  The batch repeats a block whose gradients
    are the bits of the D = 1 layout, and every repetition has to give the block's bits.
    The block's length is chosen so that a workgroup's later tiles hold OTHER data than its earlier ones: a workgroup
    strides by g R rows (96 x CUs pipelined, 306 x CUs generic), and tile t starts at row t R of the batch, i.e. at row
    t R mod block of the block.  The blocks are 227 rows (pipelined, R = 32) and 359 rows (generic, R = 51), both prime:
    k g R is a multiple of the block only if k x 96 x CUs resp. k x 306 x CUs is, which for the k = 1, 2 of this batch
    needs a device of a multiple of 227 resp. 359 CUs; and no two tiles less than a block's worth of tiles apart start
    at the same row of the block (R is coprime to the block).  So a prefetch that re-reads the tile in hand, a register
    of the carried tile that is not renewed, or a tile index off by any number of tiles below 227 resp. 359 gives the
    bits of other splines.  Asserted below for the device at hand."""
    if shape == "generic":
        K, D, mask, inverse = 5, 9, [0, 2, 3, 6, 8], True
    else:
        K, D, mask, inverse = 8, D_LAYER, ALTERNATING, shape == "pipelined_inv"
    P, dt = 3 * K - 1, len(mask)
    pl = plan(D, dt, P, 1 << 20)
    R, pipe = pl["R"], pipelined(D, dt, P, pl["R"], 1 << 20)
    assert pl["C"] == 0 and pipe == (shape != "generic") and (pipe or (R * D) % 4 != 0)
    g = grid_limit(pl, pipe)
    B = (2 * g + 3) * R + 7
    block = BLOCK_ROWS["pipelined" if pipe else "generic"]
    assert (g * R) % block != 0 and (2 * g * R) % block != 0 and R % block != 0 and block % R != 0
    assert B * dt * P * 4 < 64 << 20
    tidx = dev(np.array(mask, dtype=np.int64))
    spec, x, params, gout, glad = (a if i == 0 else dev(a) for i, a in enumerate(random_layer(K, True, D, mask, block, 320)))
    want = by_splines(ops, x, params, tidx, gout, glad, spec, inverse)
    first = backward(ops, x, params, tidx, gout, glad, spec, inverse)
    assert bits_equal(first[0], want[0]) and bits_equal(first[1], want[1])
    # (the check can tell two tiles of the block apart: no two rows of the block have the same gradients)
    assert len(set(map(bytes, host(want[1]).view(np.uint8)))) == block
    reps = -(-B // block)
    big = [t.repeat((reps,) + (1,) * (t.dim() - 1))[:B].contiguous() for t in (x, params, gout, glad)]
    gin = torch.full((B, D), float("nan"), device=DEV)
    gp = torch.full((B, dt * P), float("nan"), device=DEV)
    backward(ops, big[0], big[1], tidx, big[2], big[3], spec, inverse, gin=gin, gparams=gp)
    assert take_status(ops) == 0
    assert_repeats(gin, want[0], "grad_inputs")
    assert_repeats(gp, want[1], "grad_params")


def first_chunked_features():
    """The smallest D (half of them transformed, K = 8, linear tails) whose sample no longer fits the LDS image."""
    for D in range(800, 1200):
        if plan(D, D // 2, 23, 3)["C"] > 0:
            return D
    raise AssertionError("no chunked shape below D = 1200")


@pytest.mark.parametrize("which", ["chunked", "last_that_fits", "halved"])
def test_chunked_path_and_halved_tiles(ops, which):
    """The first D whose d_t x P floats exceed the 64 KiB image (the parameters then stream through LDS in chunks of C
    splines, the last chunk partial), the D one below it (R = 1, the largest image), and K = 40 with 32 of 64 features
    transformed (R halved from 8 to 4 by the image, not by the batch).  Bits of the D = 1 layout, both directions."""
    if which == "halved":
        K, D, B = 40, 64, 17
        pl = plan(D, D // 2, 3 * K - 1, B)
        assert pl["ok"] and pl["C"] == 0 and 1 < pl["R"] < 256 // (D // 2)
    else:
        K, D, B = 8, first_chunked_features() - (which == "last_that_fits"), 3
        pl = plan(D, D // 2, 3 * K - 1, B)
        assert pl["ok"] and pl["R"] == 1 and (pl["C"] > 0) == (which == "chunked")
        if which == "chunked":
            assert 0 < pl["C"] < D // 2 and (D // 2) % pl["C"] != 0
    mask = list(range(0, D - 1, 2))
    assert len(mask) == D // 2
    tidx = dev(np.array(mask, dtype=np.int64))
    spec, x, params, gout, glad = (a if i == 0 else dev(a) for i, a in enumerate(random_layer(K, True, D, mask, B, 330)))
    for inverse in (False, True):
        gin, gp = backward(ops, x, params, tidx, gout, glad, spec, inverse)
        want = by_splines(ops, x, params, tidx, gout, glad, spec, inverse)
        assert bits_equal(gin, want[0]) and bits_equal(gp, want[1]), (which, inverse)
    assert take_status(ops) == 0


def test_misaligned_stores(ops):
    """D = 3, one feature transformed, K = 2 (P = 5, odd): the parameter gradients leave through `tile_store` when the
    gradient buffer is misaligned like the parameter buffer, through the copy loop when it is not (parameters 1, 2, 3
    floats past a 16-byte boundary, gradients on it, and the other way round); grad_inputs written one row into a
    larger buffer (its tile starts 3 floats past the boundary) leaves the rows around it alone."""
    D, mask, K, B = 3, [1], 2, 2 * 256 + 3
    tidx = dev(np.array(mask, dtype=np.int64))
    spec, x, params, gout, glad = (a if i == 0 else dev(a) for i, a in enumerate(random_layer(K, True, D, mask, B, 340)))
    want = by_splines(ops, x, params, tidx, gout, glad, spec, False)
    for off_p in range(4):
        for off_g in range(4):
            gp = shifted(torch.full_like(params, float("nan")), off_g)
            gin, _ = backward(ops, x, shifted(params, off_p), tidx, gout, glad, spec, False, gparams=gp)
            assert bits_equal(gin, want[0]) and bits_equal(gp, want[1]), (off_p, off_g)
    big = torch.full((B + 2, D), -7.0, device=DEV)
    backward(ops, x, params, tidx, gout, glad, spec, False, gin=big[1:B + 1])
    assert bits_equal(big[1:B + 1], want[0]) and bool((big[0] == -7.0).all()) and bool((big[B + 1] == -7.0).all())
    assert take_status(ops) == 0


@pytest.mark.parametrize("shape", ["leftover_rows", "last_chunk", "three_features"])
def test_backward_writes_every_element(ops, shape):
    """Two backward passes through autograd, the allocator's free blocks filled with two different values before each
    (K9's device): every entry of grad_inputs and grad_params has the same bits both times, so none was left unwritten
    -- identity columns, splines in the tails, the leftover rows behind the pipelined kernel's full tiles, the last
    chunk of a chunked sample, a layer of three features."""
    if shape == "leftover_rows":
        K, D, mask, B = 8, D_LAYER, ALTERNATING, 2 * 32 + 5
    elif shape == "last_chunk":
        D = first_chunked_features()
        K, mask, B = 8, list(range(0, D - 1, 2)), 3
    else:
        K, D, mask, B = 5, 3, [0, 2], 300
    spec, x, params, gout, glad = random_layer(K, True, D, mask, B, 350)
    assert (np.abs(x[:, mask]) > 3.0).any()
    runs = []
    for poison in (1e30, -7.0):
        xs, ps = dev(x).requires_grad_(True), dev(params).requires_grad_(True)
        y, lad = ops.rqs_coupling(xs, ps, dev(np.array(mask, dtype=np.int64)), spec, inverse=True)
        loss = (y * dev(gout)).sum() + (lad * dev(glad)).sum()
        junk = [torch.full_like(t, poison) for t in (xs, ps) for _ in range(3)]
        del junk
        loss.backward()
        runs.append((xs.grad, ps.grad))
    assert take_status(ops) == 0
    assert bits_equal(runs[0][0], runs[1][0]) and bits_equal(runs[0][1], runs[1][1]), shape
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())


@pytest.mark.parametrize("shape", ["pipelined", "generic"])
def test_absent_upstream_gradients(ops, shape):
    """grad_logabsdet = NULL is grad_logabsdet = 0 (the kernel's `a.glad ? .. : 0`), in the pipelined kernel's prefetch and
    in the generic kernel; and a loss on logabsdet alone reaches the kernel as grad_outputs = 0."""
    K, D, mask = (8, D_LAYER, ALTERNATING) if shape == "pipelined" else (5, 9, [0, 2, 3, 6, 8])
    tidx = dev(np.array(mask, dtype=np.int64))
    B = 2 * (256 // len(mask)) + 3
    spec, x, params, gout, glad = (a if i == 0 else dev(a) for i, a in enumerate(random_layer(K, True, D, mask, B, 360)))
    for inverse in (False, True):
        none = backward(ops, x, params, tidx, gout, None, spec, inverse)
        zero = backward(ops, x, params, tidx, gout, torch.zeros_like(glad), spec, inverse)
        want = by_splines(ops, x, params, tidx, gout, None, spec, inverse)
        assert bits_equal(none[0], zero[0]) and bits_equal(none[1], zero[1])
        assert bits_equal(none[0], want[0]) and bits_equal(none[1], want[1])
        # a loss on lad alone, through autograd: the identity columns get exactly 0
        xs, ps = x.clone().requires_grad_(True), params.clone().requires_grad_(True)
        _, lad = ops.rqs_coupling(xs, ps, tidx, spec, inverse=inverse)
        (lad * glad).sum().backward()
        want = by_splines(ops, x, params, tidx, torch.zeros_like(gout), glad, spec, inverse)
        assert bits_equal(xs.grad, want[0]) and bits_equal(ps.grad, want[1])
    assert take_status(ops) == 0


@pytest.mark.parametrize("shape", ["pipelined", "generic"])
def test_permutations(ops, shape):
    """`in_perm` and `out_scatter` with pass-through columns: the layer's gradients are those of its splines put where
    the index arithmetic says (`by_splines`), and the pass-through columns of grad_inputs are bit-exact copies of the
    permuted grad_outputs: grad_inputs[:, in_perm[c]] = grad_outputs[:, out_scatter[c]]."""
    K, D, mask = (8, D_LAYER, ALTERNATING) if shape == "pipelined" else (5, 9, [0, 2, 3, 6, 8])
    rng = np.random.RandomState(370)
    tidx = dev(np.array(mask, dtype=np.int64))
    perm, scat = dev(rng.permutation(D).astype(np.int64)), dev(rng.permutation(D).astype(np.int64))
    B = 2 * (256 // len(mask)) + 3
    spec, x, params, gout, glad = (a if i == 0 else dev(a) for i, a in enumerate(random_layer(K, True, D, mask, B, 371)))
    identity = [c for c in range(D) if c not in mask]
    for inverse in (False, True):
        for pm, sc in ((perm, None), (None, scat), (perm, scat)):
            gin, gp = backward(ops, x, params, tidx, gout, glad, spec, inverse, perm=pm, scat=sc)
            want = by_splines(ops, x, params, tidx, gout, glad, spec, inverse, perm=pm, scat=sc)
            assert bits_equal(gin, want[0]) and bits_equal(gp, want[1]), (shape, inverse)
            src = torch.arange(D, device=DEV) if pm is None else pm
            dst = torch.arange(D, device=DEV) if sc is None else sc
            assert bits_equal(gin[:, src[identity]], gout[:, dst[identity]])
    assert take_status(ops) == 0
