"""Conditioners whose logits are known EXACTLY on the host (test infrastructure, not a conftest).

A ResidualNet whose weights, biases and inputs are sparse dyadic numbers computes every intermediate exactly in fp32 --
in any summation order and on every operand split of the whole-layer engines (two or three f16 pieces, three bf16
pieces, fp32 FMA chains) -- as long as two conditions hold, which `exact_logits` checks on the actual data:

  * every GEMM operand (input, weight, activation) has at most 22 significant bits (two f16 pieces hold 22);
  * every output of every Linear -- with q the common quantum of its terms (products, bias and, for the residual add,
    the block's input) -- has  sum |terms| + |bias| (+ |residual|) < 2^24 q:  every partial sum, in any order, is then a
    multiple of q below 2^24 q, i.e. representable in fp32.

With hidden_features = 64 the width / height logits are divided by sqrt(64) = 8 (coupling.py:554-556), exactly.  So the
logits every kernel feeds its spline are known bit for bit, and the difference between a kernel's output and a float64
spline on those logits is the kernel's own spline arithmetic, element by element.

The recipe (`dyadic_conditioner`):
  identity inputs k / 4, |k| <= 8 (context features too);
  initial layer: 4 nonzeros per row of +-{1, 2} / 4, bias k / 4;
  residual blocks: 2 nonzeros per row of +-{1, 2} / 4, bias k / 8 (a context layer: 2 nonzeros of +-1 / 4, bias 64, so
  that its GLU gate is exactly 1);
  final layer: 4 nonzeros per row of +-{1 .. 8} / 8, bias k / 2 -- and per transformed feature a logit REGIME through
  the final bias (REGIMES; the rows it fixes get zero weights, so that their value is the bias alone): equal logits, a
  saturated width or height softmax (one logit 90 above the others after the division by 8, one 90 below: numerators
  below 2^-126), derivative logits of -100, -20, 0, 20, 30, 100 (softplus's
  two branches and its overflow guard).

`spline_inputs` places the transformed features of every row on that row's own knots (the oracle's fp32 knots and one
ulp on either side), at +-B and one ulp inside / outside, at +-1e30 and +-0.0, or uniformly inside the box; in the
inverse direction on the height knots; with tails=None on the box's edges and the knots only.
"""
import math

import numpy as np

TAIL_BOUND = 3.0
HIDDEN = 64             # sqrt(64) = 8: the width / height divisor is a power of two
REGIMES = ("random", "equal", "width_saturated", "height_saturated", "d-100", "d-20", "d0", "d20", "d30", "d100")
SAT = 720.0             # a width / height logit 90 above (or below) the others after the division by 8


def params_per_feature(K, tails):
    return 3 * K - 1 if tails == "linear" else 3 * K + 1


def _sparse(rng, rows, cols, nnz, values):
    """[rows, cols] with `nnz` nonzeros per row drawn from +-values"""
    w = np.zeros((rows, cols))
    for i in range(rows):
        j = rng.choice(cols, size=min(nnz, cols), replace=False)
        w[i, j] = rng.choice(values, size=j.size) * rng.choice((-1.0, 1.0), size=j.size)
    return w


def regime_of(feature):
    return REGIMES[feature % len(REGIMES)]


def dyadic_conditioner(net, K, tails, seed=0, regimes=True, zero_initial=False):
    """Overwrites `net` (a ResidualNet [identity (+ context) -> dt * P]) with the recipe above; per transformed feature f
    the regime `regime_of(f)` (regimes=False: every feature "random").  `zero_initial`: the initial layer's weights are
    zero (its output is its bias: the pass-through first layer of the two-layer run).  Returns `net`."""
    import torch
    rng = np.random.RandomState(seed)
    P = params_per_feature(K, tails)
    H = net.hidden_features
    dt = net.final_layer.out_features // P
    quarter = np.array([1.0, 2.0]) / 4
    with torch.no_grad():
        lin = net.initial_layer
        w = _sparse(rng, H, lin.in_features, 4, quarter)
        lin.weight.copy_(torch.from_numpy(0.0 * w if zero_initial else w))
        lin.bias.copy_(torch.from_numpy(rng.randint(-4, 5, H) / 4.0))
        for block in net.blocks:
            for layer in block.linear_layers:
                layer.weight.copy_(torch.from_numpy(_sparse(rng, H, H, 2, quarter)))
                layer.bias.copy_(torch.from_numpy(rng.randint(-4, 5, H) / 8.0))
            if getattr(block, "context_layer", None) is not None:
                cl = block.context_layer
                cl.weight.copy_(torch.from_numpy(_sparse(rng, H, cl.in_features, 2, np.array([0.25]))))
                cl.bias.fill_(64.0)
        w = _sparse(rng, dt * P, H, 4, np.arange(1, 9) / 8.0)
        b = rng.randint(-4, 5, dt * P) / 2.0
        wv, bv = w.reshape(dt, P, H), b.reshape(dt, P)
        for f in range(dt if regimes else 0):
            r = regime_of(f)
            if r == "equal":
                wv[f] = 0.0
                bv[f] = 1.5
            elif r in ("width_saturated", "height_saturated"):
                base = 0 if r == "width_saturated" else K
                j = rng.permutation(K)[:2 if K > 2 else 1]
                wv[f, base + j] = 0.0          # (the saturated logits are their bias alone: +-720 would spend the bits
                bv[f, base + j[0]] = SAT       #  the products of the deeper recipes need)
                bv[f, base + j[1:]] = -SAT
            elif r.startswith("d"):
                wv[f, 2 * K:] = 0.0
                bv[f, 2 * K:] = float(r[1:])
        net.final_layer.weight.copy_(torch.from_numpy(w))
        net.final_layer.bias.copy_(torch.from_numpy(b))
    return net


# ---- exactness ----------------------------------------------------------------------------------------------------

def _log2_quantum(v):
    """log2 of the lowest set bit of every float64 value (+inf for 0)"""
    v = np.asarray(v, dtype=np.float64)
    m, e = np.frexp(np.abs(v))
    i = (m * 2.0 ** 53).astype(np.int64)
    low = i & -i
    lq = np.frexp(low.astype(np.float64))[1] - 1 + e.astype(np.int64) - 53
    return np.where(v == 0, np.inf, lq.astype(np.float64))


def significant_bits(v):
    """significand bits of every float64 value (0 for 0)"""
    v = np.asarray(v, dtype=np.float64)
    m, _ = np.frexp(np.abs(v))
    i = (m * 2.0 ** 53).astype(np.int64)
    odd = i // np.maximum(i & -i, 1)
    return np.where(v == 0, 0, np.frexp(odd.astype(np.float64))[1])


def _check_operand(a, what):
    bits = int(significant_bits(a).max()) if np.size(a) else 0
    assert bits <= 22, "%s: an operand with %d significant bits (at most 22 fit two f16 pieces)" % (what, bits)
    assert np.all(np.isfinite(a)) and float(np.abs(a).max(initial=0.0)) < 4094.0, what   # (K8x: x 16 within f16's range)


def _exact_linear(a, w, b, what, residual=None, chunk=256):
    """a @ w.T + b (+ residual) in float64, after checking the sufficient condition for an exact fp32 result in any
    order: sum |terms| < 2^24 q per output, q the common quantum of the output's nonzero terms"""
    _check_operand(a, what + " input")
    _check_operand(w, what + " weight")
    lq_b = _log2_quantum(b)
    out = a @ w.T + b
    if residual is not None:
        out = out + residual
    # the weights are sparse: per output row its nonzero columns (padded with a zero column, quantum +inf)
    nz = [np.flatnonzero(r) for r in w]
    width = max(1, max(len(j) for j in nz))
    cols = np.zeros((w.shape[0], width), dtype=np.int64)
    lq_w = np.full((w.shape[0], width), np.inf)
    for i, j in enumerate(nz):
        cols[i, :len(j)] = j
        lq_w[i, :len(j)] = _log2_quantum(w[i, j])
    for s in range(0, a.shape[0], chunk):
        aa = a[s:s + chunk]
        total = np.abs(aa) @ np.abs(w).T + np.abs(b)
        # (the quantum of a product of dyadics is the product of their quanta)
        lq = np.minimum((_log2_quantum(aa)[:, cols] + lq_w[None]).min(axis=2), lq_b[None, :])
        if residual is not None:
            rr = residual[s:s + chunk]
            total = total + np.abs(rr)
            lq = np.minimum(lq, _log2_quantum(rr))
        fin = np.isfinite(lq)
        ok = total[fin] < np.exp2(lq[fin] + 24)
        assert ok.all(), "%s: %d outputs outside the exact fp32 budget (sum |terms| >= 2^24 q)" % (what, int((~ok).sum()))
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out), what
    return out


def exact_logits(net, identity, context=None):
    """The conditioner's output for `identity` rows ([rows, identity features], dyadic) -- checked to be exact in fp32
    in any evaluation order -- as float64 [rows, out_features] (raw: the width / height entries NOT divided)."""
    sd = {k: v.detach().double().cpu().numpy() for k, v in net.state_dict().items()}
    a = np.asarray(identity, dtype=np.float64)
    if context is not None:
        a = np.concatenate([a, np.asarray(context, dtype=np.float64)], axis=1)
    h = _exact_linear(a, sd["initial_layer.weight"], sd["initial_layer.bias"], "initial layer")
    for i, block in enumerate(net.blocks):
        p = "blocks.%d." % i
        t = _exact_linear(np.maximum(h, 0.0), sd[p + "linear_layers.0.weight"], sd[p + "linear_layers.0.bias"], p + "0")
        t = np.maximum(t, 0.0)
        if getattr(block, "context_layer", None) is not None:
            gate = np.asarray(context, dtype=np.float64) @ sd[p + "context_layer.weight"].T + sd[p + "context_layer.bias"]
            assert gate.min() >= 40.0, "the GLU gate must be exactly 1 in fp32 (sigmoid of >= 40)"
        h = _exact_linear(t, sd[p + "linear_layers.1.weight"], sd[p + "linear_layers.1.bias"], p + "1", residual=h)
    return _exact_linear(h, sd["final_layer.weight"], sd["final_layer.bias"], "final layer")


def divided(logits, K, tails, hidden=HIDDEN):
    """[rows, dt * P] raw logits -> [rows, dt, P] with the width / height entries divided by sqrt(hidden) (float64; exact
    for hidden = 64), as the kernels hold them; `.astype(np.float32)` is then the fp32 value bit for bit"""
    P = params_per_feature(K, tails)
    v = np.array(logits, dtype=np.float64).reshape(logits.shape[0], -1, P)
    v[..., :2 * K] /= math.sqrt(hidden)
    return v


def identity_rows(rows, features, seed, low=-8, high=8, scale=0.25):
    """dyadic identity / context features k * scale, low <= k <= high"""
    return np.random.RandomState(seed).randint(low, high + 1, (rows, features)) * scale


# ---- the oracle on those logits ----------------------------------------------------------------------------------

def oracle_spec(K, tails, hidden=HIDDEN):
    from oracle import capi
    return capi.make_spec(K, tails=tails, tail_bound=TAIL_BOUND, wh_divisor=math.sqrt(hidden))


def split_logits(params, K, tails):
    """[..., P] -> (widths, heights, derivatives)"""
    return params[..., :K], params[..., K:2 * K], params[..., 2 * K:]


def knots(params, K, tails, hidden=HIDDEN, axis=0):
    """the oracle's fp32 knots [rows, dt, K + 1] of every (row, feature): axis 0 = widths, 1 = heights"""
    from oracle import capi
    uw, uh, _ = split_logits(np.asarray(params, dtype=np.float32), K, tails)
    return capi.rqs_knots(uw if axis == 0 else uh, oracle_spec(K, tails, hidden), axis=axis)


POINT_KINDS = ("knot", "knot_below", "knot_above", "+B", "-B", "+B_in", "-B_in", "+B_out", "-B_out", "+1e30", "-1e30",
               "+0", "-0", "interior", "interior")
POINT_KINDS_BOX = ("knot", "knot_below", "knot_above", "low_edge", "high_edge", "low_edge_in", "high_edge_in", "interior",
                   "interior", "interior", "interior")


def spline_inputs(params, K, tails, inverse, seed, hidden=HIDDEN, outside_rows=(), huge_rows=None):
    """Transformed-feature inputs [rows, dt] (float32) for rows whose logits are `params` [rows, dt, P] (raw): every
    element gets a kind of point (POINT_KINDS: cycled over rows and features, the knot index drawn at random) on the
    knots of its own spline -- the height knots in the inverse direction.  Rows listed in `outside_rows` have every
    element outside the box (their log-determinant is exactly 0).  tails=None: points inside [0, 1] only."""
    rng = np.random.RandomState(seed)
    params = np.asarray(params)
    rows, dt = params.shape[:2]
    kn = knots(params, K, tails, hidden, axis=1 if inverse else 0)
    pick = kn[np.arange(rows)[:, None], np.arange(dt)[None, :], rng.randint(0, K + 1, (rows, dt))]
    f32 = np.float32
    if tails == "linear":
        B = f32(TAIL_BOUND)
        kinds = POINT_KINDS
        table = {"+B": B, "-B": -B, "+B_in": np.nextafter(B, f32(0)), "-B_in": np.nextafter(-B, f32(0)),
                 "+B_out": np.nextafter(B, f32(np.inf)), "-B_out": np.nextafter(-B, f32(-np.inf)),
                 "+1e30": f32(1e30), "-1e30": f32(-1e30), "+0": f32(0.0), "-0": f32(-0.0)}
        lo, hi = -B, B
    else:
        kinds = POINT_KINDS_BOX
        table = {"low_edge": f32(0.0), "high_edge": f32(1.0), "low_edge_in": np.nextafter(f32(0), f32(1)),
                 "high_edge_in": np.nextafter(f32(1), f32(0))}
        lo, hi = f32(0.0), f32(1.0)
    kind = (np.arange(rows)[:, None] * 7 + np.arange(dt)[None, :] * 3 + rng.randint(0, 2, (rows, 1))) % len(kinds)
    x = (lo + (hi - lo) * rng.rand(rows, dt)).astype(np.float32)
    for i, k in enumerate(kinds):
        m = kind == i
        if k == "knot":
            x[m] = pick[m]
        elif k == "knot_below":
            x[m] = np.nextafter(pick[m], f32(-np.inf))
        elif k == "knot_above":
            x[m] = np.nextafter(pick[m], f32(np.inf))
        elif k in table:
            x[m] = table[k]
    if huge_rows is not None:
        m = (np.abs(x) == f32(1e30)) & ~np.asarray(huge_rows)[:, None]
        x[m] = (lo + (hi - lo) * rng.rand(int(m.sum()))).astype(np.float32)
    if tails != "linear":
        x = np.clip(x, f32(0.0), f32(1.0))
    for r in outside_rows:
        assert tails == "linear"
        x[r] = np.where(rng.rand(dt) < 0.5, -1.0, 1.0) * (B + np.float32(0.25) * rng.randint(1, 5, dt))
    return x.astype(np.float32)


def reference_order(x_t, params, K, tails, inverse, hidden=HIDDEN, cond=True):
    """The oracle's fp32 (the reference's rounding sequence) and float64 evaluation of the spline coupling on transformed
    inputs x_t [rows, dt] with raw logits `params` [rows, dt, P]: per element y / logabsdet, per row the logabsdet sum
    (the oracle's coupling: the reference's reduction), the fp32 status word, and with `cond` the per-element conditioning
    scales (helpers.conditioning over inputs and logits) of y and logabsdet."""
    from helpers import conditioning
    from oracle import capi
    rows, dt = x_t.shape
    P = params_per_feature(K, tails)
    spec = oracle_spec(K, tails, hidden)
    tidx = np.arange(dt)
    out = {}
    for tag, dtype in (("32", np.float32), ("64", np.float64)):
        xx = np.ascontiguousarray(x_t, dtype=dtype)
        pp = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(rows, dt * P), dtype=dtype)
        z, lad_row, st = capi.rqs_coupling(xx, pp, tidx, spec, inverse=inverse)
        uw, uh, ud = split_logits(pp.reshape(rows, dt, P), K, tails)
        y, lad, st_e = capi.rqs_elementwise(xx, uw, uh, ud, spec, inverse=inverse)
        assert np.array_equal(np.nan_to_num(z), np.nan_to_num(y)), "oracle: coupling and elementwise disagree"
        out.update({"y" + tag: y, "lad" + tag: lad, "row" + tag: lad_row, "status" + tag: st})
    if cond:
        uw, uh, ud = split_logits(np.asarray(params, dtype=np.float64), K, tails)
        out["cond_y"], out["cond_lad"] = conditioning(
            lambda *a: capi.rqs_elementwise(*a, spec, inverse=inverse)[:2], (x_t.astype(np.float64), uw, uh, ud), (0, 1, 2, 3))
    return out


def standard_normal_log_prob(z, lad):
    """Flow.log_prob with a StandardNormal base in the reference's order (distributions/normal.py:23-33, then + logabsdet),
    in the dtype of z"""
    import torch
    from oracle import eager
    zt = torch.from_numpy(np.ascontiguousarray(z))
    return (eager.standard_normal_log_prob(zt) + torch.from_numpy(np.ascontiguousarray(lad))).numpy()


def assert_row_allowance(got, truth, ref, cond_rows, tol, what, bulk=0.999):
    """Per-row analogue of helpers.assert_fp32_parity's allowance: a row sum (log-determinant, log_prob) is within
        A_r = tol (1 + |truth_r|) + 32 sum_f cond_rf + 2 |ref_r - truth_r|
    of the float64 truth on at least `bulk` of the rows (`cond_rows`: the row's summed per-element conditioning scales,
    reference_order's `cond_lad`).  A row whose spline sits in a minimal-width bin beside a steep one is ill-conditioned
    in ANY fp32 evaluation (the reference's own error reaches 0.5 there); a feature missing from the row's reduction, or
    a wrong element, is off by far more than its allowance.  Returns the worst error / allowance."""
    got, truth, ref, cond_rows = (np.asarray(a, dtype=np.float64) for a in (got, truth, ref, cond_rows))
    fin = np.isfinite(ref) & np.isfinite(truth)
    assert np.isfinite(got[fin]).all(), what + ": non-finite rows"
    allow = tol * (1.0 + np.abs(truth[fin])) + 32.0 * cond_rows[fin] + 2.0 * np.abs(ref[fin] - truth[fin])
    e = np.abs(got[fin] - truth[fin])
    frac = float(np.mean(e <= allow))
    assert frac >= bulk, "%s: only %.4f of the rows within their allowance of the float64 row sum (worst %.1f x)" % (
        what, frac, float((e / allow).max()))
    return float((e / allow).max())


def assert_elements_within_allowance(got, ref, truth, cond, tol, what, worst_factor=8.0):
    """helpers.assert_fp32_parity with the worst element bounded by its OWN allowance instead of a flat factor on the
    reference's worst: identical NaN / inf pattern; >= 99.9 % of the elements within A_i = tol (1 + |t_i|) + 32 cond_i +
    2 |ref_i - t_i| of the float64 truth (and within 2 A_i of the reference); mean and 99.9 % quantile of the error at
    most 2 x the reference's (helpers.assert_error_ratio); every element within `worst_factor` A_i.  For the inverse of
    the FusedSteps engines, whose Newton-refined root puts the worst element of an ill-conditioned bin 4.6 - 6.9 x the
    reference's worst (one element in 10^5) while the means stay within 1.2 x; measured against the allowance on the
    device: 7.7 x at 2 bins, 5.0 x at 24, below 4 x elsewhere."""
    from helpers import assert_error_ratio, bulk_fraction
    got, ref, truth = (np.asarray(a) for a in (got, ref, truth))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN pattern differs"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what + ": inf pattern differs"
    fin = np.isfinite(ref) & np.isfinite(truth)
    g, r, t = (a[fin].astype(np.float64) for a in (got, ref, truth))
    allow = tol * (1.0 + np.abs(t)) + 32.0 * np.asarray(cond, dtype=np.float64)[fin] + 2.0 * np.abs(r - t)
    e = np.abs(g - t)
    assert np.mean(e <= allow) >= 0.999 and np.mean(np.abs(g - r) <= 2 * allow) >= 0.999, what
    assert float((e / allow).max()) <= worst_factor, "%s: worst element %.1f x its allowance" % (what, float((e / allow).max()))
    assert_error_ratio(g, r, t, what, factor=2.0, max_factor=np.inf)
    return bulk_fraction(got, ref, tol)
