"""K6 (`rqs_shared_kernel`, nflows_amd/csrc/rqs_shared.hip) and the four batch-shared CDF classes on the device.

The table, the float64 truth and the rules are tests/cdf_shared_cases.py's; tests/test_cdf_shared_host.py holds the
oracle's own float32 to the same rules on the CPU.  Sections a - h go through the class under `torch.no_grad()`:
  a  the table: outputs per element, the [B] logabsdet as one element's (F = 1) or as a row sum;
  b  one log-derivative per row: every feature of a row but one sits in the linear tails and adds an exact +0, so the
     [B] result is ONE element's log-derivative and a reduction that reads the wrong slot, or a table indexed by the wrong
     feature, shows at the per-element tolerance;
  c  tiling: a row's result does not depend on its tile (batches around R rows, a batch that makes the persistent loop
     take further passes), and two calls agree bit for bit;
  d  alignment: tiles off a 16-byte boundary, and an unaligned input with an aligned output (the scalar store);
  e  the LDS boundary: halved R, R = 1, and `ops.rqs_shared`'s fallback to K5 and a row sum where the tables no longer fit;
  f  inputs on every knot and one ulp beside it, the ends of the box, the first value outside;
  g  InputOutsideDomain from all four classes, and a clean status word afterwards;
  h  the reference's scenarios for all four classes (tests/transforms/nonlinearities_test.py:52-91);
  i  the real reference's vectors and its autograd's gradients (tests/golden/cdf_shared.npz) for all four classes.
Which branch ran is shown from outside the kernel: the plan from the host shim of the launch planner, the grid from
the CU count, the store branch from the tensors' addresses, the fallback from a call counter.

Measured on an MI355X: see DESIGN.md section 4, "K6"."""
import numpy as np
import pytest
import torch

import cdf_shared_cases as C
import k9_cases
from helpers import (LAD_TOL, OUT_TOL, _log_parity, assert_fp32_parity, assert_sibling_truth_parity, assert_trimmed_error_ratio,
                     close_to_truth, conditioning, knot_case_keep, parse_kwargs)
from oracle import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def ops():
    from nflows_amd import ops as o
    return o


def take_status(ops):
    """The status word as a number (read and cleared): 0, 1 outside the domain, 2 negative discriminant."""
    from nflows_amd import InputOutsideDomain
    try:
        ops.check_status()
    except InputOutsideDomain:
        return 1
    except AssertionError:
        return 2
    return 0


def rq_class(shape, K, tails, uw, uh, ud):
    from nflows_amd.transforms import PiecewiseRationalQuadraticCDF
    t = PiecewiseRationalQuadraticCDF(list(shape), num_bins=K, tails=tails, tail_bound=C.TAIL_BOUND if tails else 1.0)
    with torch.no_grad():
        for p, a in ((t.unnormalized_widths, uw), (t.unnormalized_heights, uh), (t.unnormalized_derivatives, ud)):
            assert tuple(p.shape) == a.shape
            p.copy_(torch.from_numpy(a))
    return t.to(DEV).eval()


def call(t, x, inverse):
    with torch.no_grad():
        return t.inverse(x) if inverse else t(x)


@pytest.fixture
def k5_launches(ops, monkeypatch):
    """Counts the launches of K5 (`ops._rqs_elementwise_launch`): what `ops.rqs_shared` falls back to."""
    count = [0]
    launch = ops._rqs_elementwise_launch

    def counted(*args, **kwargs):
        count[0] += 1
        return launch(*args, **kwargs)

    monkeypatch.setattr(ops, "_rqs_elementwise_launch", counted)
    return count


# --------------------------------------------------------------------------------------------------------- a. values
@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_table_values(ops, k5_launches, name):
    """Every case of the table; the engine is the one the shim's plan says (K6, or the fallback for F = 255 at K = 10)."""
    case, p = C.BY_NAME[name], C.prepared(name)
    t = rq_class(case.shape, case.K, case.tails, p["uw"], p["uh"], p["ud"])
    y, lad = call(t, dev(p["x"]), case.inverse)
    status = take_status(ops)
    assert k5_launches[0] == (0 if C.k6_plan(C.features(case.shape), case.K, case.tails).ok else 1)
    fig = C.assert_values(host(y), host(lad), p["x"], p["ref"], p["truth"], p["cond"], case.tails, case.inverse, status, what=name)
    print(name, fig)


# ------------------------------------------------------------------------------------ b. one log-derivative per row
@pytest.mark.parametrize("shape", [(5,), (100,), (255,), (2, 3, 4)])
@pytest.mark.parametrize("inverse", [False, True])
def test_one_log_derivative_per_row(ops, shape, inverse):
    F, K, tb = C.features(shape), 8, C.TAIL_BOUND
    B = 4 * F
    assert C.k6_plan(F, K, "linear").ok
    rng = np.random.RandomState(9800 + F + int(inverse))
    uw, uh, ud = C.logits(shape, K, "linear", 1.5, 9900 + F)
    x = (np.where(rng.rand(B, F) < 0.5, -1.0, 1.0) * tb * (1.0 + rng.rand(B, F) + 1e-3)).astype(np.float32)
    rows, feat = np.arange(B), np.arange(B) % F
    xin = (tb * (2.0 * rng.rand(B) - 1.0)).astype(np.float32)
    x[rows, feat] = xin
    assert (C.in_box(x, "linear").sum(axis=1) == 1).all()
    y, lad = call(rq_class(shape, K, "linear", uw, uh, ud), dev(x.reshape((B,) + shape)), inverse)
    status = take_status(ops)
    assert status in ((0, 2) if inverse else (0,))
    y, lad = host(y).reshape(B, F), host(lad)
    # the features in the tails: the identity bit for bit (and their +0 leaves the sum one element's log-derivative)
    others = np.ones((B, F), dtype=bool)
    others[rows, feat] = False
    assert np.array_equal(y[others].view(np.uint32), x[others].view(np.uint32))
    sel = [a.reshape(F, -1)[feat] for a in (uw, uh, ud)]
    spec = C.oracle_spec(K, "linear")
    ry, rl, _ = capi.rqs_elementwise(xin, *sel, spec, inverse=inverse)
    ty, tl, _ = capi.rqs_elementwise(xin.astype(np.float64), *sel, spec, inverse=inverse)
    cy, cl = conditioning(lambda *a: capi.rqs_elementwise(*a, spec, inverse=inverse)[:2], (xin,) + tuple(sel), (0, 1, 2, 3))
    keep = knot_case_keep(y[rows, feat], ry, lad, rl, status, inverse, str(shape))
    assert_fp32_parity(y[rows, feat][keep], ry[keep], ty[keep], OUT_TOL, "one per row %s y" % (shape,), cond=cy[keep])
    assert_fp32_parity(lad[keep], rl[keep], tl[keep], LAD_TOL, "one per row %s lad" % (shape,), cond=cl[keep])


# ---------------------------------------------------------------------------------------------------------- c. tiling
@pytest.mark.parametrize("F", [3, 100])
@pytest.mark.parametrize("inverse", [False, True])
def test_rows_do_not_depend_on_their_tile(ops, F, inverse):
    """Batches of 1, R - 1, R, R + 1 and 2 R + 1 rows, R = floor(1024 / F) from the shim: every row of the longest call is
    bit-identical to the same row of a call on a slice (the element map is per element, the reduction order
    `lane, lane + 64, ...` then `wave_sum` whatever the tile), and a second call gives the same bits."""
    K = 8
    R = C.k6_plan(F, K, "linear").R
    assert R == 1024 // F
    uw, uh, ud = C.logits((F,), K, "linear", 1.5, 9910 + F)
    t = rq_class((F,), K, "linear", uw, uh, ud)
    x = dev(C.box_inputs(np.random.RandomState(9920 + F), 2 * R + 1, (F,), "linear"))
    y, lad = call(t, x, inverse)
    y2, lad2 = call(t, x, inverse)
    assert same_bits(y, y2) and same_bits(lad, lad2)
    for lo, hi in ((0, 1), (0, R - 1), (0, R), (0, R + 1), (R, 2 * R + 1), (R + 1, 2 * R + 1), (2 * R, 2 * R + 1)):
        ys, ls = call(t, x[lo:hi], inverse)
        assert same_bits(ys, y[lo:hi]) and same_bits(ls, lad[lo:hi]), (F, lo, hi)
    assert take_status(ops) in ((0, 2) if inverse else (0,))


@pytest.mark.parametrize("inverse", [False, True])
def test_persistent_loop_takes_further_passes(ops, inverse):
    """F = 100: 2 x 8 x CUs x R + 7 rows are more tiles than 8 workgroups per CU can take in one pass (the grid, from the
    planner: at most 8 per CU).  The first, middle and last 256 rows are bit-identical to calls on those slices and are
    held to the truth under the rules of the table; no truth is evaluated on the whole batch."""
    F, K, tails = 100, 8, "linear"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = C.k6_plan(F, K, tails).R
    rows = 2 * 8 * cus * R + 7
    tiles, grid = (rows + R - 1) // R, C.k6_grid(cus, F, K, tails, rows)
    assert grid <= 8 * cus < tiles and tiles > 2 * grid, (tiles, grid)
    uw, uh, ud = C.logits((F,), K, tails, 1.5, 9930)
    t = rq_class((F,), K, tails, uw, uh, ud)
    xs = C.box_inputs(np.random.RandomState(9931), 3 * 256, (F,), tails)
    x = torch.empty(rows, F, device=DEV).uniform_(-C.TAIL_BOUND, C.TAIL_BOUND, generator=torch.Generator(device=DEV).manual_seed(9932))
    mid = (rows // 2 // R) * R + 3          # (a slice that starts inside a tile of the long call)
    starts = (0, mid, rows - 256)
    for i, lo in enumerate(starts):
        x[lo:lo + 256] = dev(xs[256 * i:256 * (i + 1)])
    y, lad = call(t, x, inverse)
    assert take_status(ops) in ((0, 2) if inverse else (0,))
    _log_parity({"what": "K6 second pass", "rows": rows, "tiles": tiles, "grid": grid, "cus": cus, "inverse": inverse})
    for i, lo in enumerate(starts):
        ys, ls = call(t, x[lo:lo + 256], inverse)
        status = take_status(ops)
        assert same_bits(ys, y[lo:lo + 256]) and same_bits(ls, lad[lo:lo + 256]), lo
        xi = xs[256 * i:256 * (i + 1)]
        v = C.value_truth(K, tails, inverse, xi, uw, uh, ud)
        C.assert_values(host(ys), host(ls), xi, v["ref"], v["truth"], v["cond"], tails, inverse, status, what="second pass rows %d.." % lo)


# ------------------------------------------------------------------------------------------------------- d. alignment
@pytest.mark.parametrize("inverse", [False, True])
def test_unaligned_tiles_and_the_scalar_store(ops, inverse):
    """F = 3: the second tile of a call starts off a 16-byte boundary in the input AND the output (the vector store with
    an offset window).  F = 5, the input one row into a larger buffer: the input is off a 16-byte boundary, the fresh
    output is on one, so the tile's LDS image is shifted against the output and the kernel stores element by element.
    Both: bit-identical to the same rows in an aligned tensor of their own."""
    K = 8
    uw, uh, ud = C.logits((3,), K, None, 1.5, 9940)
    t = rq_class((3,), K, None, uw, uh, ud)
    R = C.k6_plan(3, K, None).R
    assert (R * 3 * 4) % 16 != 0
    x = dev(C.box_inputs(np.random.RandomState(9941), 3 * R, (3,), None))
    y, lad = call(t, x, inverse)
    for i in range(3):
        xa = x[i * R:(i + 1) * R].clone()
        assert xa.data_ptr() % 16 == 0 and (x[i * R:].data_ptr() % 16 != 0 or i == 0)
        ya, la = call(t, xa, inverse)
        assert same_bits(ya, y[i * R:(i + 1) * R]) and same_bits(la, lad[i * R:(i + 1) * R]), i
    uw, uh, ud = C.logits((5,), K, "linear", 3.0, 9942)
    t = rq_class((5,), K, "linear", uw, uh, ud)
    R = C.k6_plan(5, K, "linear").R
    rows = 2 * R + 3
    buf = torch.zeros(rows + 1, 5, device=DEV)
    buf[1:] = dev(C.box_inputs(np.random.RandomState(9943), rows, (5,), "linear"))
    xv = buf[1:]
    assert buf.data_ptr() % 16 == 0 and xv.is_contiguous() and xv.data_ptr() % 16 == 4
    xa = xv.clone()
    assert xa.data_ptr() % 16 == 0
    yv, lv = call(t, xv, inverse)
    ya, la = call(t, xa, inverse)
    assert yv.data_ptr() % 16 == 0            # (the fresh output: aligned, so `mx != tile_store_offset(y)` in every tile)
    assert same_bits(yv, ya) and same_bits(lv, la)
    assert take_status(ops) in ((0, 2) if inverse else (0,))


# ------------------------------------------------------------------------------- e. the LDS boundary and the fallback
def boundary_inputs():
    b = C.lds_boundary()
    uw, uh, ud = C.logits((b.unsupported,), C.BOUNDARY_K, None, 1.5, 9950)
    x = C.box_inputs(np.random.RandomState(9951), 64, (b.unsupported,), None)
    return b, x, uw, uh, ud


@pytest.mark.parametrize("which", C.Boundary._fields)
@pytest.mark.parametrize("inverse", [False, True])
def test_lds_boundary(ops, k5_launches, which, inverse):
    """K = 10, tails=None, 64 rows at the four feature counts of `cases.lds_boundary` (R halved to 2; R = 1 with rows off
    and on a 16-byte boundary; the first F the kernel refuses): the truth under the rules of the table, and the fallback
    ran exactly where the plan says the kernel refuses."""
    b, x, uw, uh, ud = boundary_inputs()
    F = getattr(b, which)
    x, uw, uh, ud = np.ascontiguousarray(x[:, :F]), uw[:F], uh[:F], ud[:F]
    plan = C.k6_plan(F, C.BOUNDARY_K, None, 64)
    assert (plan.ok, plan.R) == {"halved": (1, 2), "single_unaligned": (1, 1), "single_aligned": (1, 1), "unsupported": (0, 1)}[which]
    y, lad = call(rq_class((F,), C.BOUNDARY_K, None, uw, uh, ud), dev(x), inverse)
    assert k5_launches[0] == (1 if which == "unsupported" else 0)
    v = C.value_truth(C.BOUNDARY_K, None, inverse, x, uw, uh, ud)
    C.assert_values(host(y), host(lad), x, v["ref"], v["truth"], v["cond"], None, inverse, take_status(ops), what="boundary F=%d" % F)


@pytest.mark.parametrize("inverse", [False, True])
def test_continuity_across_the_fallback(ops, inverse):
    """The same 200 features through K6 (F = 248), through the fallback (F = 249) and through K5 called directly on the
    broadcast logits: both slices within twice the per-element allowance of the direct call on 99.9 % of the elements
    (two kernels: their knots may differ in the last bit).  The number of elements whose bits differ is recorded."""
    b, x, uw, uh, ud = boundary_inputs()
    n = 200
    spec = ops.make_rqs_spec(C.BOUNDARY_K, None)
    xd = dev(x[:, :n])
    share = [dev(a[:n]).unsqueeze(0).expand(64, n, a.shape[-1]) for a in (uw, uh, ud)]
    with torch.no_grad():
        direct = host(ops.rqs_elementwise(xd, share[0], share[1], share[2], spec, inverse)[0])
    v = C.value_truth(C.BOUNDARY_K, None, inverse, x[:, :n], uw[:n], uh[:n], ud[:n])
    allow = C.element_allowance(v["ref"][0], v["truth"][0], v["cond"][0], OUT_TOL)
    for F in (b.single_aligned, b.unsupported):
        y, _ = call(rq_class((F,), C.BOUNDARY_K, None, uw[:F], uh[:F], ud[:F]), dev(np.ascontiguousarray(x[:, :F])), inverse)
        got = host(y)[:, :n]
        within = float(np.mean(np.abs(got.astype(np.float64) - direct) <= 2.0 * allow))
        _log_parity({"what": "continuity F=%d vs K5 direct, inverse=%d" % (F, inverse), "elements": got.size,
                     "within_twice_allowance": within, "bit_different": int((got.view(np.uint32) != direct.view(np.uint32)).sum())})
        assert within >= C.SHARE, (F, within)
    assert take_status(ops) == 0


# ----------------------------------------------------------------------------------------------------------- f. edges
@pytest.mark.parametrize("name", C.EDGE_NAMES)
def test_knots_and_box_ends(ops, monkeypatch, name):
    """Inputs on every interior knot of every feature and one ulp to either side, and the ends of the box.  The class
    checks the status word itself where tails=None; here the check is held back and the word read afterwards, so that a
    negative discriminant of the inverse (legitimate on a knot: `knot_case_keep`) does not cost the outputs -- an
    InputOutsideDomain would show as status 1 and fails the test."""
    case, p = C.BY_NAME[name], C.edge_prepared(name)
    monkeypatch.setattr(ops, "_after_spline", lambda *a, **k: None)
    x = p["x"]
    y, lad = call(rq_class(case.shape, case.K, case.tails, p["uw"], p["uh"], p["ud"]), dev(x), case.inverse)
    status = take_status(ops)
    y, lad = host(y), host(lad)
    ry, rl = p["ref"][0], p["ref"][1]
    knot_case_keep(y, ry, y, rl, status, case.inverse, name)       # status, and at most 0.5 % NaN on either side
    fig = C.assert_values(y, lad, x, p["ref"], p["truth"], p["cond"], case.tails, case.inverse, status, what="edges " + name,
                          min_rows=C.EDGE_MIN_ROWS)
    print(name, fig)
    B = x.shape[0]
    ends = y.reshape(B, -1)[3 * (case.K - 1):]
    if case.tails is None:
        # the reference's test_zeros_to_zeros / test_ones_to_ones (nonlinearities_test.py:52-66): within 1e-5
        assert np.abs(ends[0]).max() <= 1e-5 and np.abs(ends[1] - 1.0).max() <= 1e-5
    else:
        # +-tail_bound are inside the box: `assert_values` held them to a truth that evaluates the spline there (how close to
        # +-tail_bound the spline's own end lands is the evaluation's business: the oracle's float32 is 3.9e-5 off at K = 2,
        # scale 3; the derivative there is 1 by construction, so the logabsdet cannot tell the two apart) ...
        # ... their neighbours outside are the identity (`assert_values`) and add nothing to the log-determinant
        assert np.all(lad[-2:] == 0.0)


# --------------------------------------------------------------------------------------------------- g. domain errors
def cdf_classes():
    from nflows_amd import transforms as T
    return {"linear": T.PiecewiseLinearCDF, "quadratic": T.PiecewiseQuadraticCDF, "cubic": T.PiecewiseCubicCDF,
            "rq": T.PiecewiseRationalQuadraticCDF}


@pytest.mark.parametrize("kind", ["linear", "quadratic", "cubic", "rq"])
def test_raises_domain_exception(ops, kind):
    """nonlinearities_test.py:44-50, and the inverse; the status word is clean afterwards: a valid call succeeds."""
    from nflows_amd import InputOutsideDomain
    torch.manual_seed(3)
    t = cdf_classes()[kind]([2, 3, 4]).to(DEV)
    for inverse in (False, True):
        for value in (-1.0, -0.1, 1.1, 2.0):
            with pytest.raises(InputOutsideDomain):
                call(t, torch.full([10, 2, 3, 4], value, device=DEV), inverse)
            assert take_status(ops) == 0
            y, lad = call(t, torch.full([10, 2, 3, 4], 0.5, device=DEV), inverse)
            assert torch.isfinite(y).all() and torch.isfinite(lad).all()


# ---------------------------------------------------------------------------------- h. the reference's scenarios
@pytest.mark.parametrize("kind", ["linear", "quadratic", "cubic", "rq"])
def test_reference_scenarios(ops, kind):
    """nonlinearities_test.py:52-91: zeros to zeros and ones to ones within 1e-5; inverse-then-forward gives the inputs
    back and a zero logabsdet within 1e-3 (transform_test.py's assert_forward_inverse_are_consistent), constrained on
    uniform inputs and with linear tails on 3 x standard normal ones; shape [2, 3, 4], batch 10."""
    torch.manual_seed(11)
    shape, batch = [2, 3, 4], 10
    t = cdf_classes()[kind](shape).to(DEV)
    for value in (0.0, 1.0):
        inputs = torch.full([batch] + shape, value, device=DEV)
        outputs, logabsdet = call(t, inputs, False)
        assert list(outputs.shape) == [batch] + shape and list(logabsdet.shape) == [batch]
        assert float((outputs - inputs).abs().max()) <= 1e-5, (kind, value)
    gen = torch.Generator().manual_seed(12)
    for transform, inputs in ((t, torch.rand(batch, *shape, generator=gen)),
                              (cdf_classes()[kind](shape, tails="linear").to(DEV), 3 * torch.randn(batch, *shape, generator=gen))):
        inputs = inputs.to(DEV)
        mid, lad_inv = call(transform, inputs, True)
        outputs, lad_fwd = call(transform, mid, False)
        for a, s in ((outputs, [batch] + shape), (lad_inv + lad_fwd, [batch])):
            assert list(a.shape) == s and torch.isfinite(a).all()
        assert float((outputs - inputs).abs().max()) <= 1e-3, kind
        assert float((lad_inv + lad_fwd).abs().max()) <= 1e-3, kind
    assert take_status(ops) == 0


# ------------------------------------------------------------- i. the real reference's vectors and gradients
def golden_class(G, name, kind, kw):
    t = cdf_classes()[kind](**kw)
    prefix = name + "/p/"
    t.load_state_dict({k[len(prefix):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(prefix)}, strict=True)
    return t.to(DEV)


def golden_oracle(kind, kw, K, x, params, inverse):
    """Per-element reference-fp32, float64 and conditioning from the C oracle (the fixture holds row sums only)."""
    B = x.shape[0]
    if kind == "rq":
        v = C.value_truth(K, kw["tails"], inverse, x, params["unnormalized_widths"], params["unnormalized_heights"],
                          params["unnormalized_derivatives"], tail_bound=kw["tail_bound"])
        return v["ref"], v["truth"], v["cond"]
    order = {"linear": ("unnormalized_pdf",), "quadratic": ("unnormalized_widths", "unnormalized_heights"),
             "cubic": ("unnormalized_widths", "unnormalized_heights", "unnorm_derivatives_left", "unnorm_derivatives_right")}[kind]
    logits = [np.ascontiguousarray(np.broadcast_to(params[n][None], (B,) + params[n].shape)).reshape(x.size, -1) for n in order]
    spline_kw = dict(tails="linear", tail_bound=kw["tail_bound"]) if kw["tails"] == "linear" else {}
    v = k9_cases.value_truth(kind, K, spline_kw, x.reshape(-1), logits, inverse)
    return v["ref"], v["truth"], v["cond"]


def test_reference_vectors_of_all_four_classes(ops, golden_dir):
    """Values: outputs of the siblings under `assert_sibling_truth_parity` (reference-fp32 and float64 from the fixture;
    the 99.9 % quantile rule on a kind's and direction's four cases together: below 2000 elements that quantile is an
    interpolation towards the maximum), of the rational-quadratic class under `assert_fp32_parity`; the [64] logabsdet
    against the fixture's float64 row sum with the allowance of the table's row-sum rule, per-element terms from the
    oracle."""
    G = C.golden(golden_dir)
    pool = {}
    for name, kind, kw in G["meta"]:
        name, kind, kw = str(name), str(kind), parse_kwargs(kw)
        t = golden_class(G, name, kind, kw)
        K, tails = kw["num_bins"], kw["tails"]
        x = G["x/" + name.split("_", 1)[1]]
        B = x.shape[0]
        params = dict((n, host(p)) for n, p in t.named_parameters())
        for inverse in (False, True):
            pre = name + ("/inv_" if inverse else "/")
            what = pre.rstrip("/")
            y, lad = call(t, dev(x), inverse)
            status = take_status(ops)
            y, lad = host(y), host(lad)
            ref, truth, cond = golden_oracle(kind, kw, K, x, params, inverse)
            y64, lad64 = C.golden64(G, pre + "y"), C.golden64(G, pre + "lad")
            if kind == "rq":
                assert status == 0 and np.array_equal(np.isnan(y), np.isnan(G[pre + "y"]))
                inside = C.in_box(x, tails, kw["tail_bound"])
                assert np.array_equal(y[~inside].view(np.uint32), x[~inside].view(np.uint32))
                assert_fp32_parity(y, G[pre + "y"], y64, OUT_TOL, what + " y", cond=cond[0])
            else:
                # (the logabsdet slot of the rule is per element and the class returns row sums: it is given the oracle's on
                #  both sides, so only the outputs are judged here, and the row sums below)
                rl = ref[1].reshape(-1)
                fig = assert_sibling_truth_parity((y, rl), (G[pre + "y"], rl), (y64, truth[1]), cond, x, status, inverse,
                                                  kw["tail_bound"] if tails == "linear" else None, what=what, ratios=False)
                pool.setdefault((kind, inverse), []).append(fig["y"]["errors"])
            assert not np.isnan(lad).any(), what
            C.assert_row_sums(lad, ref[1].reshape(B, -1), np.asarray(truth[1]).reshape(B, -1), np.asarray(cond[1]).reshape(B, -1),
                              what=what, truth_sum=lad64)
    assert len(pool) == 6
    for key in sorted(pool):
        e_got, e_ref, mag = (np.concatenate(v) for v in zip(*pool[key]))
        assert_trimmed_error_ratio(e_got, e_ref, mag, what="cdf_shared pooled %s inverse=%d y" % key)


def test_reference_gradients_of_all_four_classes(ops, golden_dir):
    """L = sum(Wy y) + sum(Wl logabsdet) in grad mode: dL/dx and dL/dparameter -- sums over the batch through autograd's
    expand of the shared parameters -- against the reference's float64 autograd under `close_to_truth`.
    (What it found: the inverse's width-logit gradients of the rational-quadratic class, through `rqs_backward` of
    rqs_bwd.hip, were 19 - 164 x the bound -- 0.27 on a scale of 14 at [37] on the box -- until `inverse_map_adjoint`;
    every gradient of every class is within it now.  DESIGN.md section 4, "K6".)"""
    G = C.golden(golden_dir)
    for name, kind, kw in G["meta"]:
        name, kind, kw = str(name), str(kind), parse_kwargs(kw)
        t = golden_class(G, name, kind, kw)
        tag = name.split("_", 1)[1]
        Wy, Wl = dev(G["Wy/" + tag]), dev(G["Wl/" + tag])
        for inverse in (False, True):
            pre = name + ("/inv_" if inverse else "/")
            t.zero_grad()
            x = dev(G["x/" + tag]).requires_grad_(True)
            y, lad = t.inverse(x) if inverse else t(x)
            assert y.requires_grad and lad.requires_grad
            ((Wy * y).sum() + (Wl * lad).sum()).backward()
            assert take_status(ops) == 0
            close_to_truth(x.grad, G[pre + "gx"], C.golden64(G, pre + "gx"), pre + "gx")
            for pn, p in t.named_parameters():
                close_to_truth(p.grad, G[pre + "g/" + pn], C.golden64(G, pre + "g/" + pn), pre + "g/" + pn)
