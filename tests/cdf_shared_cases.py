"""Cases, inputs, float64 truth and rules for K6 (nflows_amd/csrc/rqs_shared.hip), the rational-quadratic CDF transform
whose [F, K] logits are shared by the whole batch: `PiecewiseRationalQuadraticCDF`, and every coupling layer built with
apply_unconditional_transform=True.  tests/test_cdf_shared_host.py runs the table with the oracle's float32 result in the
implementation's place (no case may set a rule that a correct fp32 evaluation cannot meet) and reads K6's plans at the
LDS boundary from the host shim of the launch planner; tests/test_gpu_cdf_shared.py runs the table through the class on
the device.  Both import the cases and the rules from here.

Truth: oracle/capi.py's `rqs_elementwise` on float64 copies, the [F, K] logits broadcast over the batch on the host.
Yardstick (the reference's fp32 arithmetic): the same call on the float32 arrays.  Conditioning: `helpers.conditioning`
over x and the three logit arrays (the SHARED arrays are moved, then broadcast: one feature's rows move together, as
they do when an implementation rounds that feature's table differently).

The rules:
  values      per element under `helpers.assert_fp32_parity(..., OUT_TOL, cond=cy)`; inverse: elements that are NaN on
              one side alone are left out, at most 0.5 % of the case (`NAN_CAP`; see `assert_values`); at least 90 % of
              the in-box elements are finite on all sides (`FINITE_SHARE`); linear tails: outside +-tail_bound the output
              is the input bit for bit.
  logabsdet   F = 1: the [B] result is one element's: the same rule with LAD_TOL.  F > 1 (`assert_row_sums`): against the
              float64 sum of the truth with the allowance
                  sum_i A_i + (F - 1) 2^-24 sum_i |truth_i|,   A_i = LAD_TOL (1 + |truth_i|) + 32 cond_i + 2 |ref_i - truth_i|
              -- the per-element allowance of `assert_fp32_parity`, summed, plus the worst-case bound of an fp32 sum of F
              terms in any order (F - 1 additions, each rounding a partial sum that is at most sum |truth_i| ... to first
              order) -- on at least 99.9 % of the rows (`SHARE`).
"""
import atexit
import collections
import functools
import os
import shutil
import tempfile

import numpy as np

from helpers import LAD_TOL, OUT_TOL, _log_parity, assert_fp32_parity, conditioning
from oracle import capi

ROWS = 256
TAIL_BOUND = 3.0
SHARE = 0.999
NAN_CAP = 0.005
FINITE_SHARE = 0.9

Case = collections.namedtuple("Case", "name shape K tails inverse scale seed")

SHAPES = ((1,), (3,), (5,), (32,), (2, 3, 4), (100,), (255,))
BINS = (2, 8, 10, 16)
# F = 255: the tables of K = 10 and 16 do not fit in LDS (the first unsupported F at K = 10 is 249: `lds_boundary`); two
# cases stay in K6 at K = 8, one at K = 2, and the K = 10 case goes through `ops.rqs_shared`'s fallback on purpose
BINS_255 = (8, 10, 2, 8)

# name -> the fields that differ from the pattern of `_table` (a seed on which the ORACLE's float32 misses a rule is a
# bad input choice, not a finding: change it here and say why).  None so far: tests/test_cdf_shared_host.py passes on
# every seed of the pattern.
CHANGED = {}


def _table():
    """Every shape with both tails and both directions; K walks over 2, 8, 10, 16 and the logit scale alternates between
    1.5 and 3, so that every K and both scales meet both tails and both directions somewhere in the table."""
    cases = []
    for si, shape in enumerate(SHAPES):
        for ci, (tails, inverse) in enumerate(((None, False), (None, True), ("linear", False), ("linear", True))):
            K = BINS_255[ci] if shape == (255,) else BINS[(si + ci) % 4]
            scale = 1.5 if (si + ci // 2 + ci) % 2 == 0 else 3.0
            name = "f%s_k%d_%s_%s_s%g" % ("x".join(str(s) for s in shape), K, "inv" if inverse else "fwd",
                                          "tails" if tails else "box", scale)
            c = Case(name, shape, K, tails, inverse, scale, 9600 + 4 * si + ci)
            cases.append(c._replace(**CHANGED.get(name, {})))
    return cases


CASES = _table()
BY_NAME = dict((c.name, c) for c in CASES)


def features(shape):
    return int(np.prod(shape))


def num_derivatives(K, tails):
    return K - 1 if tails == "linear" else K + 1


def spec_kwargs(case):
    return dict(tails="linear", tail_bound=TAIL_BOUND) if case.tails == "linear" else dict(tails=None)


def oracle_spec(K, tails, tail_bound=TAIL_BOUND):
    return capi.make_spec(K, tails="linear", tail_bound=tail_bound) if tails == "linear" else capi.make_spec(K, tails=None)


def logits(shape, K, tails, scale, seed):
    """(uw [*shape, K], uh [*shape, K], ud [*shape, K -+ 1]) in float32: `scale` x standard normal."""
    rng = np.random.RandomState(seed)
    return tuple((scale * rng.randn(*shape, w)).astype(np.float32) for w in (K, K, num_derivatives(K, tails)))


def box_inputs(rng, rows, shape, tails):
    """x [rows, *shape] in float32, uniform over the box -- [0, 1] or [-3, 3], and for linear tails one element in twenty
    outside +-3 (up to +-6), as k9_cases.inputs does."""
    n = rows * features(shape)
    if tails != "linear":
        return rng.rand(n).astype(np.float32).reshape((rows,) + tuple(shape))
    x = TAIL_BOUND * (2.0 * rng.rand(n) - 1.0)
    out = rng.permutation(n)[:n // 20]
    x[out] = np.where(rng.rand(out.size) < 0.5, -1.0, 1.0) * TAIL_BOUND * (1.0 + rng.rand(out.size) + 1e-3)
    return x.astype(np.float32).reshape((rows,) + tuple(shape))


def inputs(case, rows=ROWS):
    """(x, uw, uh, ud) of a case from its seed."""
    lg = logits(case.shape, case.K, case.tails, case.scale, case.seed)
    return (box_inputs(np.random.RandomState(case.seed + 50000), rows, case.shape, case.tails),) + lg


def evaluate(spec, x, uw, uh, ud, inverse):
    """(y, lad per element, status) of the C oracle in the dtype of `x`: x [B, *shape], logits [*shape, w] broadcast."""
    share = [np.broadcast_to(np.asarray(a, dtype=x.dtype)[None], (x.shape[0],) + a.shape) for a in (uw, uh, ud)]
    return capi.rqs_elementwise(x, share[0], share[1], share[2], spec, inverse=inverse)


def value_truth(K, tails, inverse, x, uw, uh, ud, tail_bound=TAIL_BOUND):
    """{"ref": (y, lad, status) float32, "truth": (y, lad) float64, "cond": (cy, cl)}, all per element [B, *shape]."""
    spec = oracle_spec(K, tails, tail_bound)
    ref = evaluate(spec, x, uw, uh, ud, inverse)
    ty, tl, _ = evaluate(spec, x.astype(np.float64), uw, uh, ud, inverse)
    cond = conditioning(lambda *a: evaluate(spec, *a, inverse)[:2], (x, uw, uh, ud), (0, 1, 2, 3))
    return {"ref": ref, "truth": (ty, tl), "cond": tuple(cond)}


@functools.lru_cache(maxsize=None)
def prepared(name):
    """Inputs and truth of a case of the table, computed once per process and left unchanged."""
    case = BY_NAME[name]
    x, uw, uh, ud = inputs(case)
    out = value_truth(case.K, case.tails, case.inverse, x, uw, uh, ud)
    out.update(x=x, uw=uw, uh=uh, ud=ud)
    return out


# ------------------------------------------------------------------------------------------------------------ rules
def in_box(x, tails, tail_bound=TAIL_BOUND):
    if tails != "linear":
        return np.ones(x.shape, dtype=bool)
    tb = np.float32(tail_bound)
    return (x >= -tb) & (x <= tb)


def fp32_row_sum(a):
    """Row sums of [B, F] float32 in fp32, one term after the other."""
    return np.cumsum(np.asarray(a, dtype=np.float32), axis=1, dtype=np.float32)[:, -1]


def element_allowance(ref, truth, cond, tol):
    truth = np.asarray(truth, dtype=np.float64)
    return tol * (1.0 + np.abs(truth)) + 32.0 * np.asarray(cond, dtype=np.float64) + 2.0 * np.abs(np.asarray(ref, dtype=np.float64) - truth)


def assert_row_sums(got_lad, ref_l, truth_l, cond_l, rows=None, what="", share=SHARE, truth_sum=None):
    """The logabsdet rule at F > 1 (module docstring).  `got_lad` [B]; `ref_l`, `truth_l`, `cond_l` per element
    [B, F]; `rows`: the rows to judge (default: all); `truth_sum` [B]: a float64 row sum from elsewhere (the real
    reference's, where the elements are the oracle's) to be held to in the place of the elements' sum.  Returns
    {"share", "worst"}: the share of the judged rows within their allowance and the largest error over allowance."""
    got = np.asarray(got_lad, dtype=np.float64).reshape(-1)
    B = got.shape[0]
    ref_l, truth_l, cond_l = (np.asarray(a).reshape(B, -1) for a in (ref_l, truth_l, cond_l))
    F = truth_l.shape[1]
    rows = np.ones(B, dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
    assert rows.any(), what + ": no row to judge"
    t = truth_l[rows].astype(np.float64)
    allow = element_allowance(ref_l[rows], t, cond_l[rows], LAD_TOL).sum(axis=1) + (F - 1) * 2.0 ** -24 * np.abs(t).sum(axis=1)
    want = t.sum(axis=1) if truth_sum is None else np.asarray(truth_sum, dtype=np.float64).reshape(-1)[rows]
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got[rows] - want) / allow
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    fig = {"what": what + " lad row sums", "rows": int(rows.sum()), "features": F, "share": float(np.mean(ratio <= 1.0)),
           "worst": float(ratio.max())}
    _log_parity(dict(fig, worst_error_over_allowance=fig["worst"]))
    assert fig["share"] >= share, "%s: only %.5f of the rows within their allowance of the float64 row sum (worst %.2f x)" % (
        what, fig["share"], fig["worst"])
    return fig


def assert_values(got_y, got_lad, x, ref, truth, cond, tails, inverse, status=0, tail_bound=TAIL_BOUND, what="",
                  min_rows=FINITE_SHARE):
    """Both rules of the module docstring on one call's results: `got_y` [B, *shape], `got_lad` [B]; `ref`, `truth`,
    `cond` as `value_truth` returns them.  NaN: the implementation shows a NaN per element in its outputs and per ROW in its
    logabsdet, so an element counts as NaN on one side alone if its output is NaN on one side alone, and a row if its
    logabsdet is NaN while the reference-fp32's elements of that row are not, or the other way round; the two counts
    together stay within `NAN_CAP` of the case's elements (inverse; forward: none).  A row with a NaN on either side has
    no sum to be held to and is left out; at least `min_rows` of the rows are judged.  Returns the figures."""
    got_y, got_lad, x = np.asarray(got_y), np.asarray(got_lad).reshape(-1), np.asarray(x)
    ry, rl = ref[0], ref[1]
    ty, tl = truth
    cy, cl = cond
    B = x.shape[0]
    assert got_y.shape == x.shape and got_lad.shape == (B,), (what, got_y.shape, got_lad.shape)
    F = x.size // B
    inside = in_box(x, tails, tail_bound)
    assert np.array_equal(got_y[~inside].view(np.uint32), x[~inside].view(np.uint32)), what + ": tails are not the identity"
    ref_nan = np.isnan(ry) | np.isnan(rl)
    one_sided = np.isnan(got_y) != np.isnan(ry)
    one_sided_rows = np.isnan(got_lad) != ref_nan.reshape(B, -1).any(axis=1)
    left_out = int(one_sided.sum()) + int(one_sided_rows.sum())
    if inverse:
        assert status in (0, 2), (what, status)
        assert left_out <= NAN_CAP * x.size, "%s: %d elements and %d rows NaN on one side only" % (
            what, int(one_sided.sum()), int(one_sided_rows.sum()))
    else:
        assert status == 0, (what, status)
        assert left_out == 0, what + ": NaN pattern differs"
    keep = ~(np.isnan(got_y) | ref_nan) & np.isfinite(ty) & np.isfinite(tl)
    finite = float(keep[inside].mean())
    assert finite >= FINITE_SHARE, "%s: only %.4f of the in-box elements finite on all sides" % (what, finite)
    assert_fp32_parity(got_y[keep], ry[keep], ty[keep], OUT_TOL, what + " y", cond=cy[keep])
    rows = keep.reshape(B, -1).all(axis=1) & ~np.isnan(got_lad)
    figures = {"finite": finite, "nan_on_one_side": left_out / x.size, "rows_judged": float(rows.mean())}
    assert rows.mean() >= min_rows, "%s: only %.4f of the rows have a sum to be held to" % (what, float(rows.mean()))
    if F == 1:
        assert_fp32_parity(got_lad[rows], rl.reshape(-1)[rows], tl.reshape(-1)[rows], LAD_TOL, what + " lad", cond=cl.reshape(-1)[rows])
    else:
        figures["row_sums"] = assert_row_sums(got_lad, rl, tl, cl, rows, what)
    return figures


# --------------------------------------------------------------------------------------------------- edge inputs (f)
def edge_inputs(case, uw, uh):
    """x [3 (K - 1) + 4, *shape] in float32: every feature's own interior knots of the searched axis (`capi.rqs_knots`
    in float32: widths forward, heights inverse), each with its two `nextafter` neighbours, and the ends of the box:
    box cases 0.0, 1.0 and their neighbours inside; tails cases +-tail_bound (inside the box) and their neighbours
    outside (the identity)."""
    spec = oracle_spec(case.K, case.tails)
    knots = capi.rqs_knots(uh if case.inverse else uw, spec, axis=int(case.inverse)).reshape(-1, case.K + 1)
    lo, hi = knots[:, 0], knots[:, -1]
    rows = []
    for j in range(1, case.K):
        k = knots[:, j]
        rows += [np.nextafter(k, lo), k, np.nextafter(k, hi)]
    if case.tails == "linear":
        rows += [lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))]
    else:
        rows += [lo, hi, np.nextafter(lo, hi), np.nextafter(hi, lo)]
    return np.stack(rows).astype(np.float32).reshape((len(rows),) + tuple(case.shape))


EDGE_NAMES = [c.name for c in CASES if features(c.shape) in (5, 24, 100)]
# Every feature of a row sits on a knot, so one NaN logabsdet (the inverse's logarithm of a root one ulp outside [0, 1]:
# the oracle's own float32 has one or two such elements in three of these cases) takes its whole row's sum with it: here
# half of the rows have to be left to judge, not 90 %.  The cap on NaNs on one side alone stays what it is.
EDGE_MIN_ROWS = 0.5


@functools.lru_cache(maxsize=None)
def edge_prepared(name):
    """The case's parameters with `edge_inputs` in the place of its random inputs, and their truth."""
    case = BY_NAME[name]
    _, uw, uh, ud = inputs(case, rows=1)
    x = edge_inputs(case, uw, uh)
    out = value_truth(case.K, case.tails, case.inverse, x, uw, uh, ud)
    out.update(x=x, uw=uw, uh=uh, ud=ud)
    return out


# ----------------------------------------------------------------------------------------- K6's plans, from the shim
_shim = []


def shim():
    """tests/launch_plan_shim.py built once per process (the product's planner, compiled for the host)."""
    if not _shim:
        import launch_plan_shim
        d = tempfile.mkdtemp(prefix="cdf_shared_shim")
        atexit.register(shutil.rmtree, d, True)
        _shim.append(launch_plan_shim.build(d))
    return _shim[0]


Plan = collections.namedtuple("Plan", "ok R lds")


@functools.lru_cache(maxsize=None)
def k6_plan(F, K, tails, batch=1 << 20):
    """The tile `nfa_rqs_shared_f32` plans for a shape: ok (0: NFA_ERR_UNSUPPORTED, the fallback), rows per tile, bytes of LDS."""
    import ctypes
    out = (ctypes.c_int64 * 12)()
    shim().k6(F, K, num_derivatives(K, tails), batch, out)
    return Plan(int(out[0]), int(out[1]), int(out[3]))


def k6_grid(cus, F, K, tails, batch):
    """Workgroups of the launch: `persistent_grid(cus, lds, 8, tiles)`."""
    p = k6_plan(F, K, tails, batch)
    return int(shim().grid_lds(cus, p.lds, 8, (batch + p.R - 1) // p.R))


Boundary = collections.namedtuple("Boundary", "halved single_unaligned single_aligned unsupported")
BOUNDARY_K = 10


@functools.lru_cache(maxsize=None)
def lds_boundary():
    """Feature counts around the end of K6's reach at K = 10, tails=None, read from the shim: the last F whose tile of
    floor(1024 / F) = 4 rows is halved to R = 2 and no further; the last F with R = 1 whose rows are not / are 16-byte
    aligned; the first F with ok = 0."""
    plans = dict((F, k6_plan(F, BOUNDARY_K, None)) for F in range(129, 400))
    unsupported = min(F for F, p in plans.items() if not p.ok)
    single = [F for F, p in plans.items() if F < unsupported and p.R == 1]
    halved = max(F for F, p in plans.items() if p.ok and 1024 // F == 4 and p.R == 2)
    return Boundary(halved, max(F for F in single if F % 4), max(F for F in single if F % 4 == 0), unsupported)


# -------------------------------------------------------------------- the real reference's vectors (cdf_shared.npz)
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "cdf_shared.npz"))


def golden64(G, key):
    """The float64 result stored next to the float32 result `key` (make_golden_cdf_shared.py: v + s * d)."""
    s = dict(zip((str(k) for k in G["scale_keys"]), G["scale_values"]))[key]
    return G[key].astype(np.float64) + s * G[key + "_d"].astype(np.float64)
