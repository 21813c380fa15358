"""Every layer-kernel engine's spline arithmetic against float64, element by element, on logits known EXACTLY.

The conditioners here are the dyadic recipe of tests/exact_logits.py: every intermediate of the conditioner is exact in
fp32 in any order and on every operand split, so the logits each kernel feeds its spline are known bit for bit on the
host -- for every engine and bin count, diagnostic twin or not.  The difference between a kernel's output and the
oracle's spline on those logits is then the kernel's own spline arithmetic: its lane / feature mapping of the logits,
its boundary-derivative slots, its tail tests and its per-row log-determinant reduction.

Inputs: each row's transformed features on that row's knots and one ulp beside them, at +-B and one ulp inside /
outside, at +-1e30 and +-0.0, inside the box (tails=None: the box's edges and knots); a few rows wholly outside the
box.  Logits: every regime of exact_logits.REGIMES (saturated softmaxes, derivative logits in both softplus branches).

`ROWS` distinct rows are repeated to the batch size that selects the engine; every copy must come out bit for bit as
the first (rows are independent and their logits exact).  Per case, forward and inverse of a one-layer flow and its
log_prob (density epilogue):
  * the kernel that ran (ops.last_layer_kernel) and no row block redone by the exact kernel;
  * identity columns and outside-box elements bit-equal to the input; rows wholly outside the box: log-determinant 0;
  * z / x per element: helpers.assert_fp32_parity against the oracle's fp32 (reference order) and float64 evaluation on
    the same logits, with the per-element conditioning allowance (in the inverse, helpers.knot_case_keep decides the
    discriminant cases; the FusedSteps engines' inverse has its worst element bounded by 8 x its own allowance instead of
    4 x the reference's worst: exact_logits.assert_elements_within_allowance);
  * log-determinant and log_prob per row, every case: exact_logits.assert_row_allowance -- each row within its
    allowance built from the per-element conditioning (99.5 % of the rows, helpers.knot_case_keep's share; on the device
    a few rows in 2048 of FusedSteps at 11 bins leave it) -- and helpers.assert_error_ratio against the oracle's
    fp32 and float64 row sums.  The FusedSteps engines (K8h / K8x) at bin counts other than 8 are held to the allowance
    alone in the FORWARD direction: their running fp32 knot sums put the mean per-row error at up to 3.8 x the
    reference's own there (measured: 3.1 x at 10 bins, 3.5 x at 16, 3.8 x at 24 on the device; 2.9 x / 4.4 x at 16 / 32
    on the host, tests/test_rqs_f32_host.py), all of it on rows with a minimal-width bin beside +-B, whose allowance
    covers it (the reference's own error there reaches 0.5); the ratio is reported.

Geometry: D = 64 (32 transformed features, whole groups of four) and D = 62 (31: a padded group); one-layer flows, and
a two-layer run (layer, permutation, layer in ONE launch) whose first layer passes its rows through -- zero initial
weights, every transformed input outside the box -- so that the SECOND layer of a persistent run is under the oracle.
"""
import copy

import numpy as np
import pytest
import torch

import exact_logits as X
from helpers import LAD_TOL, OUT_TOL, assert_error_ratio, assert_fp32_parity, knot_case_keep
from test_gpu_headline_parity import _report
from test_gpu_steep import _nsf_engines, _status, engine_switches  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64
ROWS = 2048                 # distinct rows; the batch repeats them
OUTSIDE_ROWS = (300, 777)   # rows with every transformed feature outside the box (not in the +-1e30 blocks)
HUGE_ROWS = 256             # +-1e30 only in the first 256 rows of every copy: the f16 engines hand such a block (an
                            # eight-wave workgroup: two flags) to the exact kernel (asserted: no other block is redone)
CONTEXT = 8
_cases = {}
_fused_z = {}               # engine -> z of the K = 8 case (FusedSteps agreement: reported)


def _engine(name, K):
    """(switches, batch rows, K8s setting, label pieces) of `name` at K bins"""
    if name == "k8x":
        return dict(path="k8", engine="f16x3"), 16384, True, ("k8x::", "K=%d," % K)
    return _nsf_engines(K)[name]


def _case(K, tails="linear", context=False, hidden=X.HIDDEN, variant=""):
    """flow (CPU) with the dyadic conditioner, its exact logits, inputs and the oracle, per direction.  `variant`: "" (one
    layer, D = 64), "odd" (one layer, D = 62: 31 transformed features, a padded group), "two_layer" (D = 64: a
    pass-through layer, a permutation, the layer under test).  Inputs and results in the coordinates of the layer under
    test (`perm`: its input column j is the flow's column perm[j])."""
    key = (K, tails, context, hidden, variant)
    if key in _cases:
        return _cases[key]
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms import CompositeTransform, Permutation
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ
    D = 62 if variant == "odd" else 64
    C = CONTEXT if context else None

    def make(mask, seed, zero_initial=False):
        layer = RQ(mask, lambda i, o: ResidualNet(i, o, hidden_features=hidden, context_features=C, num_blocks=2), num_bins=K,
                   tails=tails, tail_bound=X.TAIL_BOUND)
        X.dyadic_conditioner(layer.transform_net, K, tails, seed=seed, zero_initial=zero_initial)
        return layer
    mask = torch.ones(D)
    mask[::2] = -1
    perm = np.arange(D)
    if variant == "two_layer":
        first = make(mask, seed=200 + K, zero_initial=True)
        perm = torch.randperm(D, generator=torch.Generator().manual_seed(K)).numpy()
        # the second layer's identity features are the first layer's transformed ones (outside the box: passed through)
        mask2 = torch.from_numpy(np.where(mask.numpy()[perm] > 0, -1.0, 1.0)).float()
        layer = make(mask2, seed=100 + K)
        transform = CompositeTransform([first, Permutation(torch.from_numpy(perm)), layer])
    else:
        layer = make(mask, seed=100 + K)
        transform = CompositeTransform([layer])
    flow = Flow(transform, StandardNormal([D])).eval()
    ti, ii = layer.transform_features.numpy(), layer.identity_features.numpy()
    Pn = X.params_per_feature(K, tails)
    case = {"flow": flow, "ti": ti, "ii": ii, "hidden": hidden, "perm": perm, "D": D}
    ctx = X.identity_rows(ROWS, C, seed=K + 7) if context else None
    case["context"] = None if ctx is None else torch.from_numpy(ctx.astype(np.float32))
    for inverse in (False, True):
        if variant == "two_layer":      # dyadic values in (B, B + 1]
            ident = X.TAIL_BOUND + X.identity_rows(ROWS, len(ii), seed=K + 3 * inverse, low=1, high=4)
        else:
            ident = X.identity_rows(ROWS, len(ii), seed=K + 3 * inverse)
        raw = X.exact_logits(layer.transform_net, ident, ctx).reshape(ROWS, len(ti), Pn)
        xt = X.spline_inputs(raw, K, tails, inverse, seed=K + 11 * inverse, hidden=hidden,
                             outside_rows=OUTSIDE_ROWS if tails == "linear" else (), huge_rows=np.arange(ROWS) < HUGE_ROWS)
        if tails is None and inverse:
            # (tails=None raises the reference's assertion on a discriminant rounded below zero, rational_quadratic.py:142,
            #  which any fp32 evaluation may meet on an input ON a height knot -- the box's edges included: the inverse
            #  keeps interior points, the knots and edges are the forward direction's)
            kn = X.knots(raw, K, tails, hidden, axis=1)
            near = (np.abs(xt[..., None] - kn) <= 4 * np.spacing(np.float32(1))).any(-1)
            xt[near] = np.random.RandomState(K).uniform(0.05, 0.95, int(near.sum())).astype(np.float32)
        full = np.zeros((ROWS, D), np.float32)
        full[:, ii] = ident
        full[:, ti] = xt
        o = X.reference_order(xt, raw, K, tails, inverse, hidden=hidden)
        o["cond_row"] = np.where(np.isfinite(o["cond_lad"]), o["cond_lad"], 0.0).sum(1)
        if not inverse:
            for tag in ("32", "64"):
                z = full.astype(np.float64 if tag == "64" else np.float32)
                z[:, ti] = o["y" + tag]
                o["lp" + tag] = X.standard_normal_log_prob(z, o["row" + tag])
        # the flow's input: column perm[j] holds the layer's column j (forward); the inverse's input is the layer's output
        flow_in = np.empty_like(full)
        if inverse:
            flow_in = full
        else:
            flow_in[:, perm] = full
        case["fwd" if not inverse else "inv"] = (full, xt, raw, o, flow_in)
    _cases.clear()          # (one case at a time: the parametrisation is ordered by case)
    _cases[key] = case
    return case


def _copies(t, rows):
    """[batch, ...] -> [copies, ROWS, ...]: every copy bit-equal to the first"""
    v = t.reshape(rows // ROWS, ROWS, *t.shape[1:])
    assert torch.equal(torch.nan_to_num(v), torch.nan_to_num(v[:1].expand_as(v))), "copies of a row differ"
    return v[0].cpu().numpy()


def _check(what, case, direction, got_all, lad, K, tails, forward_ratio, fused=False):
    full, xt, raw, o, _ = case[direction]
    ti, ii = case["ti"], case["ii"]
    inverse = direction == "inv"
    assert np.array_equal(got_all[:, ii].view(np.uint32), full[:, ii].view(np.uint32)), what + ": identity columns"
    got = got_all[:, ti]
    inbox = (np.abs(xt) <= X.TAIL_BOUND) if tails == "linear" else np.ones(xt.shape, bool)
    assert np.array_equal(got[~inbox].view(np.uint32), xt[~inbox].view(np.uint32)), what + ": outside the box"
    for r in (OUTSIDE_ROWS if tails == "linear" else ()):
        assert lad[r] == 0.0, (what, r, float(lad[r]))
    keep = knot_case_keep(got[inbox], o["y32"][inbox], np.zeros(int(inbox.sum())), np.zeros(int(inbox.sum())),
                          2 if inverse else 0, inverse, what)
    sel = np.zeros(xt.shape, bool)
    sel[inbox] = keep
    if fused and inverse:   # (the worst element against its own allowance: exact_logits.assert_elements_within_allowance)
        X.assert_elements_within_allowance(got[sel], o["y32"][sel], o["y64"][sel], o["cond_y"][sel], OUT_TOL, what + " z")
    else:
        assert_fp32_parity(got[sel], o["y32"][sel], o["y64"][sel], OUT_TOL, what + " z", cond=o["cond_y"][sel])
    # (rows with a discriminant rounded below zero in the inverse -- a NaN here or in the reference -- are left out, as
    #  helpers.knot_case_keep leaves their elements out)
    rows_ok = (sel.sum(1) == inbox.sum(1)) & np.isfinite(o["row32"]) & (np.isfinite(lad) if inverse else True)
    assert rows_ok.mean() >= 0.95, (what, float(rows_ok.mean()))
    worst = X.assert_row_allowance(lad[rows_ok], o["row64"][rows_ok], o["row32"][rows_ok], o["cond_row"][rows_ok], LAD_TOL,
                                   what + " logabsdet per row", bulk=0.995)
    e = np.abs(lad[rows_ok].astype(np.float64) - o["row64"][rows_ok]).mean()
    e_ref = np.abs(o["row32"][rows_ok].astype(np.float64) - o["row64"][rows_ok]).mean()
    _report({"config": what, "what": "logabsdet per row", "mean_ratio": e / e_ref, "worst_over_allowance": worst})
    if forward_ratio or inverse:
        assert_error_ratio(lad[rows_ok], o["row32"][rows_ok], o["row64"][rows_ok], what + " logabsdet per row")


def _matrix():
    m = [("k8x", K, "linear", False, "") for K in range(2, 17)] + [("k8x", K, "linear", False, "") for K in (20, 24, 32)]
    m += [(e, K, "linear", False, "") for K in (2, 3, 8, 10, 16, 32) for e in ("k8h_w8", "k8h_w4", "k8")
          if not (e == "k8h_w8" and K == 32)]     # (32 bins at this width: the LDS budget leaves K8h four waves)
    m += [(e, 8, "linear", False, "") for e in ("k8s_w8", "k8s_w4", "k8c")]
    m += [("k8", K, None, False, "") for K in (3, 8, 10)]
    m += [(e, 8, "linear", True, "") for e in ("k8h_w8", "k8")]
    m += [(e, 8, "linear", False, "") for e in ("k7", "k7b", "gemm_k1", "gemm_k1_pipelined")]
    m += [(e, K, "linear", False, "odd") for K in (8, 10) for e in ("k8x", "k8h_w4", "k8")]
    m += [(e, 8, "linear", False, "two_layer") for e in ("k8x", "k8h_w8", "k8")]
    return sorted(m, key=lambda c: (c[1], str(c[2]), c[3], c[4], c[0] in ("k7", "k7b", "gemm_k1", "gemm_k1_pipelined")))


@pytest.mark.parametrize("engine,K,tails,context,variant", _matrix())
def test_engine_spline_on_exact_logits(engine_switches, engine, K, tails, context, variant):
    from nflows_amd import ops
    layer_by_layer = engine in ("k7", "k7b", "gemm_k1", "gemm_k1_pipelined")
    case = _case(K, tails, context, hidden=128 if layer_by_layer else X.HIDDEN, variant=variant)   # (K7 reads 128 hidden features)
    switches, rows, k8s, expect = _engine(engine, K)
    if tails is None:
        expect = ("rqs_resnet_kernel<", "tails=none", "K=%d," % K)
    engine_switches(switches["path"], switches["engine"], k8s)
    import os
    os.environ.update(switches.get("env", {}))
    flow = copy.deepcopy(case["flow"]).to(DEV)
    ctx = None if case["context"] is None else case["context"].repeat(rows // ROWS, 1).to(DEV)
    what = "%s K=%d tails=%s%s %s" % (engine, K, tails, " context" if context else "", variant)
    forward_ratio = not (engine.startswith(("k8x", "k8h")) and K != 8)     # (the allowance alone: see the module docstring)
    _status(what, clear=True)
    redo, redo_inverse = [], []

    def redone():       # row blocks the f16 engines handed to the exact kernel, outside the +-1e30 blocks
        b = (ops._last_redo != 0).nonzero().flatten().cpu().numpy()
        return [int(i) for i in b if (i * 128) % ROWS >= HUGE_ROWS]
    with torch.no_grad():
        x = torch.from_numpy(case["fwd"][4]).repeat(rows // ROWS, 1).to(DEV)
        z, lad = flow._transform(x, context=ctx)
        label_f = ops.last_layer_kernel()
        if engine.startswith(("k8h", "k8s", "k8x", "k8c")):
            redo += redone()
        lp = flow.log_prob(x, context=ctx)
        y = torch.from_numpy(case["inv"][4]).repeat(rows // ROWS, 1).to(DEV)
        xi, ladi = flow._transform.inverse(y, context=ctx)
        label_i = ops.last_layer_kernel()
        if engine.startswith(("k8h", "k8s", "k8x", "k8c")):
            redo_inverse += redone()
    for label, inv in ((label_f, 0), (label_i, 1)):
        for piece in expect:
            assert piece in label, "%s ran %r, expected %r" % (what, label, expect)
        assert ("inverse=1" in label) == bool(inv), label
    assert not redo, "%s: row blocks %s redone by the exact kernel" % (what, redo[:8])
    # (in the inverse a block with a discriminant rounded below zero -- a NaN result, on the inputs ON a knot -- is the
    #  exact kernel's by design: those blocks are still held to the oracle below, and counted in the report)
    z, lad, lp, xi, ladi = (_copies(t, rows) for t in (z, lad, lp, xi, ladi))
    xi = xi[:, case["perm"]]        # (the flow's inverse output in the coordinates of the layer under test)
    fused = engine.startswith(("k8x", "k8h", "k8s", "k8c"))
    _check(what + " forward", case, "fwd", z, lad, K, tails, forward_ratio, fused)
    _check(what + " inverse", case, "inv", xi, ladi, K, tails, forward_ratio, fused)
    o = case["fwd"][3]
    assert np.array_equal(np.isinf(lp), np.isinf(o["lp32"])), what + ": log_prob inf pattern"
    fin = np.isfinite(o["lp32"]) & np.isfinite(o["lp64"])
    X.assert_row_allowance(lp[fin], o["lp64"][fin], o["lp32"][fin], o["cond_row"][fin], LAD_TOL, what + " log_prob per row",
                           bulk=0.995)
    if forward_ratio:
        assert_error_ratio(lp[fin], o["lp32"][fin], o["lp64"][fin], what + " log_prob per row")
    _status(what)
    if K == 8 and tails == "linear" and not context and not variant and engine in ("k8x", "k8h_w8", "k8s_w8", "k8s_w4", "k8c"):
        _fused_z[engine] = (z, lad)
    _report({"config": what, "kernels": [label_f, label_i], "rows": rows, "inverse_blocks_redone": len(redo_inverse)})


@pytest.mark.parametrize("engine", ["k8x", "k8h", "k8"])
def test_captured_logits_are_the_exact_logits(monkeypatch, engine):
    """The premise: at 8 bins the diagnostic twins of K8x / K8h / K8 return the host's exact logits bit for bit, forward
    and inverse (a difference would be a GEMM finding, not a tolerance)."""
    from nflows_amd import ops
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ
    case = _case(8)
    _status("capture", clear=True)
    monkeypatch.setattr(RQ, "conditioner_engine", {"k8x": "f16x3", "k8h": "f16x2", "k8": "bf16x3"}[engine])
    monkeypatch.setattr(ops, "K8S_ENABLED", False)
    layer = copy.deepcopy(case["flow"]._transform._transforms[0]).to(DEV)
    rows = 16384
    for direction in ("fwd", "inv"):
        full, _, raw, _, _ = case[direction]
        x = torch.from_numpy(full).repeat(rows // ROWS, 1).to(DEV)
        with torch.no_grad(), ops.capture_last_layer_logits() as cap:
            layer.inverse(x) if direction == "inv" else layer(x)
        _status("capture %s %s" % (engine, direction))
        assert cap.launches == 1 and cap.logits is not None, (engine, direction, ops.last_layer_kernel())
        want = torch.from_numpy(X.divided(raw.reshape(ROWS, -1), 8, "linear").astype(np.float32))
        got = cap.logits[:, :want.shape[1]].reshape(rows // ROWS, *want.shape)
        assert torch.equal(got.cpu(), want[None].expand_as(got)), "%s %s: captured logits differ from the exact ones" % (engine, direction)


@pytest.mark.parametrize("rows", [8192, 16384])
def test_logits_capture_is_never_silently_ignored(rows):
    """Batches K8s / K8c would serve: under capture_last_layer_logits the launch goes to K8h's twin (ops.use_tile16 returns
    0), so the capture holds the logits -- it used to stay empty with launches == 0."""
    from nflows_amd import ops
    case = _case(8)
    _status("capture", clear=True)
    layer = copy.deepcopy(case["flow"]._transform._transforms[0]).to(DEV)
    full, _, raw, _, _ = case["fwd"]
    x = torch.from_numpy(full).repeat(rows // ROWS, 1).to(DEV)
    with torch.no_grad():
        layer(x)
        plain = ops.last_layer_kernel()
        with ops.capture_last_layer_logits() as cap:
            layer(x)
    _status("capture %d rows" % rows)
    assert "k8s::" in plain or "k8c::" in plain, plain      # (the batch is one the small-batch kernels serve)
    assert cap.launches == 1 and cap.logits is not None, ops.last_layer_kernel()
    want = torch.from_numpy(X.divided(raw.reshape(ROWS, -1), 8, "linear").astype(np.float32))
    got = cap.logits[:, :want.shape[1]].reshape(rows // ROWS, *want.shape)
    assert torch.equal(got.cpu(), want[None].expand_as(got))


def test_report_fused_steps_engines_agreement():
    """Reported, not asserted: whether K8x / K8h / K8s / K8c give the same bits on identical exact logits (8 bins)."""
    if len(_fused_z) < 2:
        pytest.skip("the engine cases did not run in this session")
    names = sorted(_fused_z)
    ref = names[0]
    out = {}
    for n in names[1:]:
        a, b = _fused_z[ref], _fused_z[n]
        out["%s_vs_%s" % (n, ref)] = {"z_bits_differ": int((a[0].view(np.uint32) != b[0].view(np.uint32)).sum()),
                                     "lad_bits_differ": int((a[1].view(np.uint32) != b[1].view(np.uint32)).sum())}
    _report({"config": "fused_steps_agreement", "elements": int(_fused_z[ref][0].size), "result": out})
    print("\n[fused-steps agreement] %r" % out)
