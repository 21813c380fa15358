"""Cases, inputs, float64 gradient truth and rules for K1-backward (`nfa_rqs_coupling_backward_f32`,
nflows_amd/csrc/rqs_bwd.hip): the one kernel every rational-quadratic layer trains through.  tests/test_k1_backward_host.py
runs the table through the host build of the kernel's per-spline function `rqs_backward`
(tests/_hostcore/rqs_f32_host.py), tests/test_gpu_k1_backward.py through the kernel; both import the cases and the rules
from here, so a defect in the arithmetic shows on a CPU before a GPU sees it.

A case is `ROWS` independent splines, flat: inputs x [n], logits uw, uh [n, K] and ud [n, K - 1 | K + 1], upstream
gradients wy, wl [n] of the loss  L = <y, wy> + <logabsdet, wl>.
  * Truth: float64 autograd through oracle/eager.py's `rqs_unconstrained` / `rqs_constrained` (the op-for-op port that
    tests/test_oracle_golden.py pins to the real reference); `fd_gradients` cross-checks it against central differences of
    the C oracle (oracle/capi.py) in float64.
  * Yardstick: the same port in float32 on the CPU -- the reference's own fp32 autograd.
  * Conditioning: `helpers.conditioning` of the float64 gradient over all four arguments.
  * Rule (`rows_outside`, one implementation for the caps, the product and the knots; it is `helpers.assert_gradient_rows`'
    rule, the project's gradient rule, and a CPU test holds the two counts equal): a row -- one spline: gx and its P logit gradients --
    passes when every entry is within 2e-5 (1 + |truth|) + 32 cond of the truth.  NaN / inf: the pattern of the
    reference's fp32; a row that is non-finite on one side only is a miss, a row non-finite on both sides in the same
    entries is left out.  Splines in the tails: gx == gy bit for bit and all P gradients exactly +0.  The share of missing
    rows of a case is at most GRAD_CAP of its (tails, direction) group.  There is NO rule on the maximum.

Logit scales are the scales the softmax SEES: with `wh_divisor` the raw width / height logits are the divisor times
larger (the kernel and the port divide them)."""
import collections
import functools
import math

import numpy as np

from helpers import conditioning
from oracle import capi

ROWS = 2048
ROW_SPLINES = 8     # transformed features per row when a case is laid out as a coupling layer
TAIL_BOUND = 3.0
GRAD_TOL = 2e-5
DIVISOR = math.sqrt(128.0)
RECT = (-1.5, 2.5, -4.0, 0.5)       # left, right, bottom, top of the non-square box
UNIT = (0.0, 1.0, 0.0, 1.0)
FD_STEPS = (1e-5, 5e-6)             # (k9_cases.FD_STEPS)
FD_AGREE = 1e-6

Case = collections.namedtuple("Case", "name K tails inverse box divisor scale dscale ident mins loss seed")

# The gradient rule on the REFERENCE's own fp32 autograd (oracle/eager.py in float32) on the table's inputs, pooled per
# (linear tails?, inverse?): (rows outside, rows).  test_k1_backward_host.py recomputes these and holds the constants to
# the result.  The cap of a group is twice that share (the project's standing allowance for a second correct fp32
# evaluation), never below 0.1 %.
REFERENCE_GRAD_OUTSIDE = {
    (True, False): (14, 20480), (True, True): (29, 18432),        # 0.068 % -> cap 0.137 %; 0.157 % -> cap 0.315 %
    (False, False): (7, 20480), (False, True): (55, 22528),       # 0.034 % -> cap 0.1 %;   0.244 % -> cap 0.488 %
}
GRAD_CAP = dict((k, max(2.0 * bad / rows, 1e-3)) for k, (bad, rows) in REFERENCE_GRAD_OUTSIDE.items())

# ADMISSION.  A case, with its seed, is in the table only if the host build of `rqs_backward` leaves at most HALF the cap
# of its group outside (test_k1_backward_host.py asserts it) -- the rule must not ask of the kernel what a correct fp32
# evaluation of these formulas cannot give.  Half the cap is the reference's own pooled share, and the host build misses
# where the reference misses (same formulas: per case their counts differ by a row or two), so a case harder than its
# group's average cannot stay, and every replacement lowers the average: the search (seed + 100, + 200, ... until the
# host build is admitted at the caps of the table as it then stands; repeated until nothing changes) ends with groups of
# like cases.  It took 4 rounds.  (case name in the pattern of `_table`, BEFORE the change: the case's own name states
# its scales after it, e.g. k2_tails_inv_s1.5_d12) -> the fields that differ from the pattern;
# rows outside of 2048, host build / reference's fp32, before -> after:
CHANGED = {
    # Not reachable by a seed (12 / 39 seeds tried): the inverse with K = 2 and derivative logits at scale 25 -- 8 / 26
    # (tails) and 39 / 69 (box) rows; input gradients of several hundred next to the box end, where the reference's fp32
    # is 50 % off -- and the forward saturated cases with derivative logits at scale 12 -- 14 / 17 and 13 / 15; gx in bins
    # of minimum width, whose width is a difference of two knots of size 1.  Derivative scale 12 still puts 5 % of the
    # logits past the z > 20 branch; the K = 2 forward cases and test_nan_pattern_with_extreme_derivative_logits keep 25
    # and more, the inverse saturated cases keep scale 12.
    "k2_tails_inv_s1.5_d25": dict(dscale=12.0),                                     # 8 / 26 -> 3 / 13
    "k2_box_inv_s1.5_d25": dict(dscale=12.0, seed=9126),                            # 39 / 69 -> 5 / 17
    "k8_tails_fwd_raw40_d12_div_saturated": dict(dscale=3.0, seed=13605),           # 14 / 17 -> 1 / 2
    "k8_box_fwd_raw40_d12_div_saturated": dict(dscale=3.0, seed=10821),             # 13 / 15 -> 1 / 2
    # Seeds (rows outside on the host build at the pattern's seed -> at the new one):
    "k8_tails_fwd_s1.5": dict(seed=8200),                                           # 3 -> 1
    "k8_tails_fwd_s3_div": dict(seed=8901),                                         # 4 -> 1
    "k40_tails_fwd_s1.5": dict(seed=9432),                                          # 3 -> 1
    "k8_tails_fwd_s3_div_identity_init": dict(seed=8335),                           # 2 -> 1
    "k8_tails_inv_s1.5": dict(seed=8208),                                           # 4 -> 1
    "k8_tails_inv_s1.5_loss_lad": dict(seed=8208),                                  # 4 -> 1
    "k8_box_fwd_s1.5": dict(seed=8216),                                             # 2 -> 1
    "k8_box_fwd_s1.5_loss_lad": dict(seed=8516),                                    # 3 -> 1
    "k8_box_fwd_s3_div": dict(seed=8517),                                           # 5 -> 1
    "k8_box_fwd_s3_div_rect": dict(seed=8534),                                      # 3 -> 1
    "k8_box_inv_raw40_d12_div_saturated": dict(seed=8229),                          # 7 -> 3
}


def _name(c, tag):
    name = "k%d_%s_%s_" % (c.K, "tails" if c.tails else "box", "inv" if c.inverse else "fwd")
    name += "raw40" if tag == "saturated" else "s%g" % c.scale
    name += ("_d%g" % c.dscale if c.dscale != c.scale else "") + ("_div" if c.divisor else "")
    return name + ("_" + tag if tag else "") + ("_loss_" + c.loss if c.loss != "both" else "")


def _table():
    """Scale 1.5 goes without the divisor, scale 3 through it (without it the REFERENCE's fp32 autograd leaves 2 % of the
    rows outside at scale 3 -- height-logit gradients off by a relative 1e-4 in both evaluations alike --, which no cap of
    a group would admit).  Per tail kind and direction: K = 8 (the compiled instance) at both scales;
    K = 2 with derivative logits at scale 25 (the z > 20 branch of softplus and its derivative); two of the run-time
    bin counts 3, 5, 10, 16 (every one in both directions and with both tail kinds over the table); one saturated case
    (raw width / height logits at scale 40 through the divisor, 3.5 at the softmax: its smallest terms are 1e-4 and
    less, so those bins sit at their minimum; derivative logits at scale 12) -- 24 cases; K = 40 once per tail kind; the
    non-square box, the identity initialisation (softplus beta != 1) and non-default minimums in both directions; and the two degenerate losses (wl = 0: "y", wy = 0: "lad") on
    the first case of every group."""
    rows = []
    for ti, tails in enumerate((True, False)):
        for inverse in (False, True):
            odd = (ti + int(inverse)) % 2 == 1
            rows += [dict(K=8, scale=1.5), dict(K=8, scale=3.0, divisor=DIVISOR), dict(K=2, scale=1.5, dscale=25.0),
                     dict(K=16 if odd else 3, scale=3.0, divisor=DIVISOR), dict(K=5 if odd else 10, scale=1.5),
                     dict(K=8, scale=40.0 / DIVISOR, dscale=12.0, divisor=DIVISOR, tag="saturated"),
                     dict(K=8, scale=1.5, loss="y"), dict(K=8, scale=1.5, loss="lad")]
            for r in rows[-8:]:
                r.update(tails=tails, inverse=inverse)
    rows += [dict(K=40, scale=1.5, tails=True, inverse=False), dict(K=40, scale=1.5, tails=False, inverse=True)]
    for inverse in (False, True):
        rows += [dict(K=8, scale=3.0, divisor=DIVISOR, tails=False, inverse=inverse, box=RECT, tag="rect"),
                 dict(K=5 if inverse else 8, scale=3.0, divisor=DIVISOR, tails=not inverse, inverse=inverse, ident=True,
                      tag="identity_init"),
                 dict(K=8 if inverse else 10, scale=3.0, divisor=DIVISOR, tails=inverse, inverse=inverse,
                      mins=(0.02, 0.02, 0.1), tag="mins")]
    cases = []
    for i, r in enumerate(rows):
        tails, inverse = r["tails"], r["inverse"]
        c = Case("", r["K"], tails, inverse, None if tails else r.get("box", UNIT), r.get("divisor", 0.0), r["scale"],
                 r.get("dscale", r["scale"]), r.get("ident", False), r.get("mins"), r.get("loss", "both"), 8100 + i)
        if c.loss != "both":
            c = c._replace(seed=cases[len(cases) - (6 if c.loss == "y" else 7)].seed)   # the group's first case
        c = c._replace(**CHANGED.get(_name(c, r.get("tag")), {}))     # (CHANGED is keyed by the PATTERN's name)
        cases.append(c._replace(name=_name(c, r.get("tag"))))        # (the name states what the case now is)
    assert len(set(c.name for c in cases)) == len(cases)
    return cases


CASES = _table()
BY_NAME = dict((c.name, c) for c in CASES)
GROUPS = ((True, False), (True, True), (False, False), (False, True))


def functional_kwargs(case):
    """Keyword arguments of the reference's functional (and of oracle/eager.py's port of it)."""
    kw = dict(tail_bound=TAIL_BOUND) if case.tails else dict(zip(("left", "right", "bottom", "top"), case.box))
    if case.ident:
        kw["enable_identity_init"] = True
    if case.mins:
        kw.update(zip(("min_bin_width", "min_bin_height", "min_derivative"), case.mins))
    return kw


def product_spec(case):
    from nflows_amd import ops
    return ops.make_rqs_spec(case.K, "linear" if case.tails else None, wh_divisor=case.divisor, **functional_kwargs(case))


def oracle_spec(case):
    return capi.make_spec(case.K, tails="linear" if case.tails else None, wh_divisor=case.divisor, **functional_kwargs(case))


def num_derivatives(case):
    return case.K - 1 if case.tails else case.K + 1


def input_range(case):
    """Where inputs are inside the spline's domain.  The reference tests `inputs` against left / right in EITHER
    direction (rational_quadratic.py:81) and searches the heights in the inverse: on a non-square box the inverse's
    usable inputs are the overlap of the two intervals."""
    if case.tails:
        return -TAIL_BOUND, TAIL_BOUND
    left, right, bottom, top = case.box
    return (max(left, bottom), min(right, top)) if case.inverse else (left, right)


def inputs(case, rows=ROWS):
    """(x, uw, uh, ud) in float32 from the case's seed: x uniform over `input_range`, with linear tails one element in
    twenty outside +-3 (up to +-6); logits `scale` x N(0, 1) (x the divisor), derivative logits `dscale` x N(0, 1)."""
    rng = np.random.RandomState(case.seed)
    lo, hi = input_range(case)
    x = lo + (hi - lo) * rng.rand(rows)
    if case.tails:
        out = rng.permutation(rows)[:rows // 20]
        x[out] = np.where(rng.rand(out.size) < 0.5, -1.0, 1.0) * TAIL_BOUND * (1.0 + rng.rand(out.size) + 1e-3)
    s = case.scale * (case.divisor if case.divisor else 1.0)
    uw, uh = s * rng.randn(rows, case.K), s * rng.randn(rows, case.K)
    ud = case.dscale * rng.randn(rows, num_derivatives(case))
    return tuple(a.astype(np.float32) for a in (x, uw, uh, ud))


def weights(case, rows=ROWS):
    """Upstream gradients (wy, wl) of outputs and logabsdet, float32; the degenerate losses zero one of them.  wl is
    constant over runs of ROW_SPLINES splines: a coupling layer's logabsdet is one number per row, so the GPU test can
    lay the same splines out as rows of ROW_SPLINES transformed features."""
    wy = np.random.RandomState(case.seed + 50000).randn(rows).astype(np.float32)
    wl = np.repeat(np.random.RandomState(case.seed + 60000).randn(-(-rows // ROW_SPLINES)), ROW_SPLINES)[:rows].astype(np.float32)
    return (wy if case.loss != "lad" else np.zeros_like(wy)), (wl if case.loss != "y" else np.zeros_like(wl))


def packed(uw, uh, ud):
    return np.ascontiguousarray(np.concatenate([uw, uh, ud], axis=1), dtype=np.float32)


def autograd_gradients(case, x, uw, uh, ud, wy, wl, dtype):
    """(gx [n], gparams [n, P]) of L = <y, wy> + <lad, wl> by autograd through oracle/eager.py in `dtype`, as numpy."""
    import torch
    from oracle import eager
    dt = {np.float32: torch.float32, np.float64: torch.float64}[dtype]
    ts = [torch.from_numpy(np.array(a, dtype=dtype)).requires_grad_(True) for a in (x, uw, uh, ud)]
    fn = eager.rqs_unconstrained if case.tails else eager.rqs_constrained
    d = case.divisor if case.divisor else 1.0
    y, lad = fn(ts[0], ts[1] / d, ts[2] / d, ts[3], inverse=case.inverse, **functional_kwargs(case))
    loss = (y * torch.from_numpy(np.asarray(wy)).to(dt)).sum() + (lad * torch.from_numpy(np.asarray(wl)).to(dt)).sum()
    loss.backward()
    return ts[0].grad.numpy(), torch.cat([t.grad for t in ts[1:]], dim=1).numpy()


def outside_box(case, x):
    if not case.tails:
        return np.zeros(x.shape, dtype=bool)
    tb = np.float32(TAIL_BOUND)
    return ~((x >= -tb) & (x <= tb))


def truth_for(case, x, uw, uh, ud, wy, wl):
    """{"truth": [gx, gp] float64, "ref": [gx, gp] the reference's fp32, "cond": [cx, cp]} for the given inputs."""
    truth = autograd_gradients(case, x, uw, uh, ud, wy, wl, np.float64)
    ref = autograd_gradients(case, x, uw, uh, ud, wy, wl, np.float32)
    cond = conditioning(lambda *a: autograd_gradients(case, *a, wy, wl, np.float64), (x, uw, uh, ud), (0, 1, 2, 3))
    return {"truth": list(truth), "ref": list(ref), "cond": list(cond)}


@functools.lru_cache(maxsize=None)
def prepared(name):
    """Inputs, upstream gradients, truth, yardstick and conditioning of a case of the table, once per process."""
    case = BY_NAME[name]
    x, uw, uh, ud = inputs(case)
    wy, wl = weights(case)
    out = truth_for(case, x, uw, uh, ud, wy, wl)
    out.update(x=x, uw=uw, uh=uh, ud=ud, wy=wy, wl=wl, outside=outside_box(case, x))
    return out


def nonfinite_pattern(arrays, n):
    """[n, 1 + P] int8: 0 finite, 1 NaN, 2 +inf, 3 -inf."""
    a = np.concatenate([np.asarray(t).reshape(n, -1) for t in arrays], axis=1)
    return (np.isnan(a) * 1 + (np.isposinf(a)) * 2 + (np.isneginf(a)) * 3).astype(np.int8)


def rows_outside(got, p, extra=None):
    """(bad, keep): per row, is any entry further than 2e-5 (1 + |truth|) + 32 cond (+ `extra`) from the truth, or
    non-finite on one side only; `keep` leaves out the rows that are non-finite in the same entries on both sides."""
    n = p["truth"][0].shape[0]
    pg, pr = nonfinite_pattern(got, n), nonfinite_pattern(p["ref"], n)
    same = (pg == pr).all(axis=1)
    keep = ~(same & (pr != 0).any(axis=1))
    bad = ~same
    for i, (g, t, c) in enumerate(zip(got, p["truth"], p["cond"])):
        allow = GRAD_TOL * (1.0 + np.abs(t)) + 32.0 * c + (0.0 if extra is None else extra[i])
        with np.errstate(invalid="ignore"):
            ok = np.abs(np.asarray(g, dtype=np.float64).reshape(t.shape) - t) <= allow
        bad |= ~ok.reshape(n, -1).all(axis=1)
    return bad, keep


def assert_tails(got, p, what=""):
    """Splines in the tails: gx == gy bit for bit, every logit gradient exactly +0 (the sign bit too)."""
    out = p["outside"]
    if out.any():
        gx, gp = np.asarray(got[0]).reshape(-1), np.asarray(got[1]).reshape(out.size, -1)
        assert np.array_equal(gx[out].view(np.uint32), p["wy"][out].view(np.uint32)), what + ": gx != gy in the tails"
        assert not gp[out].view(np.uint32).any(), what + ": logit gradient in the tails is not +0"


def assert_rows(got, p, cap, what="", verbose=False):
    """The rule of this module on `got` = [gx [n], gparams [n, P]] for a prepared case `p`: the tails exactly, and at most
    `cap` of the kept rows outside by `rows_outside` -- the count the caps themselves are taken with.  Returns the share."""
    assert_tails(got, p, what)
    bad, keep = rows_outside(got, p)
    share = float(bad[keep].mean()) if keep.any() else 0.0
    if verbose:
        print("%-44s gradients: %d of %d rows kept, %d outside (%.4f %%), cap %.2f %%" % (
            what, int(keep.sum()), keep.size, int(bad[keep].sum()), 100.0 * share, 100.0 * cap))
    assert share <= cap, "%s: %.4f %% of the rows outside their allowance (cap %.2f %%)" % (what, 100.0 * share, 100.0 * cap)
    return share


def reference_gradient_shares():
    """The rule on the reference's own fp32 autograd over the table, pooled per group: {(tails, inverse): (bad, rows)}."""
    out = {}
    for c in CASES:
        p = prepared(c.name)
        bad, keep = rows_outside(p["ref"], p)
        b, r = out.get((c.tails, c.inverse), (0, 0))
        out[(c.tails, c.inverse)] = (b + int(bad[keep].sum()), r + int(keep.sum()))
    return out


def probe_inputs(seed, n=4096, K=2, scale=3.0, dscale=25.0):
    """The inputs on which the NaN of `sigmoid_beta` was found (K = 2, unit box; see test_k1_backward_host.py): logits first, then x, then the upstream gradients."""
    rng = np.random.RandomState(seed)
    uw, uh = (scale * rng.randn(n, K)).astype(np.float32), (scale * rng.randn(n, K)).astype(np.float32)
    ud = (dscale * rng.randn(n, K + 1)).astype(np.float32)
    x = rng.rand(n).astype(np.float32)
    return dict(x=x, uw=uw, uh=uh, ud=ud, wy=rng.randn(n).astype(np.float32), wl=rng.randn(n).astype(np.float32))


# ------------------------------------------------------------------------------------------- central differences
def fd_gradients(case, x, uw, uh, ud, wy, wl, h):
    """Central difference quotients of L in float64 through the C oracle (capi.rqs_elementwise): (gx [n], gp [n, P]).
    A logit is moved by `h`, the input by `h` mean bin widths, one column at a time (the splines are independent);
    the raw width / height logits by `h` divisors, so that the softmax sees `h`."""
    spec = oracle_spec(case)
    x = np.asarray(x, dtype=np.float64)
    logits = [np.array(a, dtype=np.float64) for a in (uw, uh, ud)]
    wy, wl = np.asarray(wy, dtype=np.float64), np.asarray(wl, dtype=np.float64)
    lo, hi = (spec.bottom, spec.top) if case.inverse else (spec.left, spec.right)
    hx = h * (hi - lo) / case.K

    def loss(x_, lg):
        y, lad = capi.rqs_elementwise(x_, lg[0], lg[1], lg[2], spec, inverse=case.inverse)[:2]
        return wy * y + wl * lad

    with np.errstate(invalid="ignore"):
        gx = (loss(x + hx, logits) - loss(x - hx, logits)) / (2.0 * hx)
        cols = []
        for a, step in zip(logits, (h * (case.divisor or 1.0), h * (case.divisor or 1.0), h)):
            for j in range(a.shape[1]):
                keep = a[:, j].copy()
                a[:, j] = keep + step
                up = loss(x, logits)
                a[:, j] = keep - step
                cols.append((up - loss(x, logits)) / (2.0 * step))
                a[:, j] = keep
    return gx, np.stack(cols, axis=1)


# ------------------------------------------------------------------------------------------------------ knot cases
KNOT_CASES = ("knots_k8_tails_fwd", "knots_k8_tails_inv", "knots_k5_box_fwd", "knots_k5_box_inv")
KNOT_SPLINES = 48
KNOT_DELTA_ULPS = 8
# The knot rule (`knot_rows_outside`) on the reference's own fp32 autograd at the same inputs: (rows outside, rows);
# recomputed by test_k1_backward_host.py.  Cap: twice that share, never below 0.1 %.  (In the inverse direction a
# gradient next to a knot of a steep bin changes by its own size within `delta`; the reference's fp32 and the
# product's agree with each other there and not with either one-sided truth.)
KNOT_REFERENCE_OUTSIDE = {"knots_k8_tails_fwd": (0, 1296), "knots_k8_tails_inv": (18, 1296),
                          "knots_k5_box_fwd": (2, 864), "knots_k5_box_inv": (22, 864)}
KNOT_CAP = dict((k, max(2.0 * bad / rows, 1e-3)) for k, (bad, rows) in KNOT_REFERENCE_OUTSIDE.items())


def knot_case(name):
    """The spec of a knot case: K = 8 with linear tails, K = 5 on the unit box, logit scale 1.5."""
    K, tails, inverse = int(name[7]), "_tails_" in name, name.endswith("_inv")
    return Case(name, K, tails, inverse, None if tails else UNIT, 0.0, 1.5, 1.5, False, None, "both", 8900 + K + int(inverse))


def _neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def _on_rows(rows, n, fn):
    """`fn` (returning (gx, gp)) on the rows of `rows` only; the others get the identity's gradient (wy, 0) later."""
    gx, gp = fn()
    P = gp.shape[1]
    fx, fp = np.zeros(n, dtype=gx.dtype), np.zeros((n, P), dtype=gp.dtype)
    fx[rows], fp[rows] = gx, gp
    return fx, fp


@functools.lru_cache(maxsize=None)
def prepared_knots(name):
    """Inputs ON the knots.  For each of KNOT_SPLINES logit rows: every interior knot of the searched axis as the float64
    oracle places it, rounded to fp32, with its two fp32 neighbours; the two box ends exactly, one ulp inside and one ulp
    outside.  Each input is one spline (its logit row repeated).  At a knot d lad / d x and the parameter gradients are
    one-sided: the truth is taken at x - delta and at x + delta (delta = KNOT_DELTA_ULPS fp32 ulp of the larger box end:
    the knots of two correct fp32 evaluations lie within 4 of those ulp of each other, helpers.assert_bins_match, so
    float64 sits in a definite bin on either side), clamped to the box, and a row passes against EITHER side.  What
    `delta` costs is read off the truth itself: per entry |truth(x +- delta) - truth(x +- 2 delta)| is added to that
    side's allowance -- inside a bin the gradient is smooth, so to first order the first step of `delta` moves it as
    much as the second.  Inputs outside the box are not compared with a truth: the identity's gradient (tails), or the
    identity's gradient and NFA_STATUS_OUTSIDE_DOMAIN (box), exactly.
    Returns inputs, upstream gradients, `inside`, `ref` (the reference's fp32 at x itself, for the NaN pattern) and
    `sides`: per side {"truth", "cond", "extra"}."""
    case = knot_case(name)
    _, uw, uh, ud = inputs(case, KNOT_SPLINES)
    spec = oracle_spec(case)
    lo, hi = input_range(case)
    knots = capi.rqs_knots((uh if case.inverse else uw).astype(np.float64), spec, axis=1 if case.inverse else 0)
    xs, rows = [], []
    for r in range(KNOT_SPLINES):
        pts = [v for kn in knots[r, 1:-1] for v in _neighbours(kn)] + _neighbours(lo) + _neighbours(hi)
        xs += pts
        rows += [r] * len(pts)
    x = np.array(xs, dtype=np.float32)
    rows = np.array(rows)
    uw, uh, ud = uw[rows], uh[rows], ud[rows]
    n = x.size
    wy, wl = weights(case, n)
    inside = (x >= np.float32(lo)) & (x <= np.float32(hi))
    delta = KNOT_DELTA_ULPS * float(np.spacing(np.float32(max(abs(lo), abs(hi)))))
    sub = lambda *arrays: [a[inside] for a in arrays]     # noqa: E731
    x64 = x.astype(np.float64)
    sides = []
    for sgn in (-1.0, 1.0):
        near, far = (np.clip(x64 + sgn * m * delta, lo, hi) for m in (1.0, 2.0))
        t = truth_for(case, *sub(near, uw, uh, ud, wy, wl))
        f = autograd_gradients(case, *sub(far, uw, uh, ud, wy, wl), np.float64)
        side = {"truth": list(_on_rows(inside, n, lambda: t["truth"])), "cond": list(_on_rows(inside, n, lambda: t["cond"])),
                "extra": list(_on_rows(inside, n, lambda: [np.abs(a - b) for a, b in zip(t["truth"], f)]))}
        side["truth"][0][~inside] = wy[~inside]
        sides.append(side)
    ref = list(_on_rows(inside, n, lambda: autograd_gradients(case, *sub(x, uw, uh, ud, wy, wl), np.float32)))
    ref[0][~inside] = wy[~inside]
    return dict(case=case, x=x, uw=uw, uh=uh, ud=ud, wy=wy, wl=wl, sides=sides, inside=inside, ref=ref, outside=~inside)


def knot_rows_outside(got, pk):
    """(bad, keep) of a knot case: a row is bad when it misses the rule (with the side's extra allowance) against BOTH
    sides, or is non-finite where the reference's fp32 at the same input is finite (or the other way round)."""
    both = None
    for side in pk["sides"]:
        bad, keep = rows_outside(got, dict(truth=side["truth"], cond=side["cond"], ref=pk["ref"]), extra=side["extra"])
        both = bad if both is None else (both & bad)
    return both, keep


def knot_reference_shares():
    out = {}
    for name in KNOT_CASES:
        pk = prepared_knots(name)
        bad, keep = knot_rows_outside(pk["ref"], pk)
        out[name] = (int(bad[keep].sum()), int(keep.sum()))
    return out


def assert_knot_rows(got, status, pk, cap, what="", verbose=False):
    """The knot rule; `status` is the evaluation's status word.  Returns the share of rows outside."""
    from nflows_amd import _native as N
    case = pk["case"]
    assert_tails(got, pk, what)
    allowed = (N.STATUS_NEG_DISCRIMINANT if case.inverse else 0) | (0 if case.tails else N.STATUS_OUTSIDE_DOMAIN)
    assert status & ~allowed == 0, (what, status)
    if not case.tails:
        assert status & N.STATUS_OUTSIDE_DOMAIN, what + ": inputs one ulp outside the box were not reported"
    bad, keep = knot_rows_outside(got, pk)
    share = float(bad[keep].mean())
    if verbose:
        print("%-44s knots: %d of %d rows kept, %d outside (%.4f %%), cap %.2f %%" % (
            what, int(keep.sum()), keep.size, int(bad[keep].sum()), 100.0 * share, 100.0 * cap))
    assert share <= cap, "%s: %.4f %% of the rows outside their allowance (cap %.2f %%)" % (what, 100.0 * share, 100.0 * cap)
    return share
