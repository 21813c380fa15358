"""K1-backward's per-spline arithmetic -- `rqs_backward` of nflows_amd/csrc/rqs_bwd.hip, compiled for the host
(tests/_hostcore/rqs_f32_host.py) -- on the case table of tests/k1_backward_cases.py, under the rules the GPU test
(tests/test_gpu_k1_backward.py) applies to the kernel: per-row allowance against float64 autograd, the reference's NaN
pattern, exact identity in the tails, one-sided truths on the knots.  Also what keeps the table honest: the caps are
recomputed from the reference's fp32 autograd, every case is admitted by the host build at half its cap, and the
autograd truth is cross-checked against central differences of the C oracle.  CPU only, seconds.  -s for the figures."""
import ctypes
import shutil

import numpy as np
import pytest

import k1_backward_cases as kc
from _hostcore import rqs_f32_host

NAMES = [c.name for c in kc.CASES]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return rqs_f32_host.build(str(tmp_path_factory.mktemp("k1bwd")))


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_backward(lib, case, p, instance=0):
    """(status, [gx, gparams]) of the host build: `instance` 8 = the compiled K = 8 instance, 0 = run-time K."""
    x = np.ascontiguousarray(p["x"], dtype=np.float32)
    pr = kc.packed(p["uw"], p["uh"], p["ud"])
    gx, gp = np.empty_like(x), np.empty_like(pr)
    spec = kc.product_spec(case)
    status = lib.host_rqs_backward(instance, int(case.inverse), x.size, ctypes.byref(spec), P(x), P(pr), P(p["wy"]), P(p["wl"]),
                                   P(gx), P(gp))
    return status, [gx, gp]


def test_the_table_covers_what_it_says():
    by = lambda **kw: [c for c in kc.CASES if all(getattr(c, k) == v for k, v in kw.items())]   # noqa: E731
    assert 38 <= len(kc.CASES) <= 44
    for tails in (True, False):
        assert by(K=40, tails=tails)
        for inverse in (False, True):
            assert by(K=8, tails=tails, inverse=inverse, divisor=0.0) and by(K=8, tails=tails, inverse=inverse, divisor=kc.DIVISOR)
            assert by(K=2, tails=tails, inverse=inverse) and by(tails=tails, inverse=inverse, loss="y") and by(tails=tails, inverse=inverse, loss="lad")
            assert [c for c in by(tails=tails, inverse=inverse) if "saturated" in c.name]
    for inverse in (False, True):
        assert by(box=kc.RECT, inverse=inverse) and by(ident=True, inverse=inverse) and by(mins=(0.02, 0.02, 0.1), inverse=inverse)
        assert set(c.K for c in by(inverse=inverse)) >= {2, 3, 5, 8, 10, 16, 40}
    # what the cases are there for: a bin at its minimum width, a saturated derivative logit on both branches
    p = kc.prepared(next(c.name for c in by(tails=True, inverse=False) if "saturated" in c.name))
    soft = np.exp(p["uw"] / kc.DIVISOR - (p["uw"] / kc.DIVISOR).max(axis=1, keepdims=True))
    assert np.mean((soft / soft.sum(axis=1, keepdims=True)).min(axis=1) < 1e-4) > 0.5
    for case in by(K=2):
        ud = kc.prepared(case.name)["ud"]
        assert (ud > 20.0).mean() > 0.03 and (ud < -20.0).mean() > 0.03


@pytest.mark.parametrize("name", NAMES)
def test_table_on_the_host_build(lib, name):
    """The rule at the group's cap -- and ADMISSION: the host build misses at most half the cap, so that the rule does not
    ask of the kernel what a correct fp32 evaluation of these formulas cannot give."""
    case, p = kc.BY_NAME[name], kc.prepared(name)
    cap = kc.GRAD_CAP[(case.tails, case.inverse)]
    for instance in [0] + ([8] if case.K == 8 else []):
        status, got = host_backward(lib, case, p, instance)
        assert status == 0, (name, instance, status)
        share = kc.assert_rows(got, p, cap, what="%s [instance %d]" % (name, instance), verbose=True)
        assert share <= 0.5 * cap, "%s [instance %d] is not admitted: %.4f %% of the rows outside, half the cap is %.4f %%" % (
            name, instance, 100.0 * share, 50.0 * cap)


def test_the_count_is_the_projects_gradient_rule(lib):
    """`k1_backward_cases.rows_outside` counts what `helpers.assert_gradient_rows`, the project's gradient rule, counts
    (on cases without non-finite entries, which that helper has no pattern rule for): one rule, not two."""
    from helpers import assert_gradient_rows
    for name in ("k8_box_inv_s1.5", "k8_box_inv_raw40_d12_div_saturated", "k2_box_inv_s1.5_d12", "k8_tails_fwd_s1.5"):
        case, p = kc.BY_NAME[name], kc.prepared(name)
        for got in (host_backward(lib, case, p)[1], p["ref"]):
            bad, keep = kc.rows_outside(got, p)
            assert keep.all()
            share = assert_gradient_rows(got, p["truth"], p["cond"], keep, 1.0, tol=kc.GRAD_TOL, what=name)
            assert share == bad.mean(), name


def test_caps_are_the_reference_fp32s_own_shares():
    """REFERENCE_GRAD_OUTSIDE is what the rule counts on the reference's fp32 autograd (oracle/eager.py in float32) over
    the table; nothing of the product enters."""
    got = kc.reference_gradient_shares()
    print(got)
    assert got == kc.REFERENCE_GRAD_OUTSIDE
    for key, (bad, rows) in got.items():
        assert kc.GRAD_CAP[key] == max(2.0 * bad / rows, 1e-3)
    knots = kc.knot_reference_shares()
    print(knots)
    assert knots == kc.KNOT_REFERENCE_OUTSIDE
    for key, (bad, rows) in knots.items():
        assert kc.KNOT_CAP[key] == max(2.0 * bad / rows, 1e-3)


@pytest.mark.parametrize("name", ["k8_tails_fwd_s1.5", "k8_tails_inv_s1.5", "k8_box_fwd_s1.5", "k8_box_inv_s1.5"])
def test_autograd_truth_matches_central_differences(name):
    """The float64 autograd through the eager port against central differences of the C oracle in float64, at K9's two
    step sizes.  Rows whose two quotients disagree (a knot inside the stencil) are left out, at most 2 % of them (K9's
    FD_DROP_CAP); on the others the two truths agree to 1e-6 (1 + |g|), the agreement asked of the two step sizes."""
    case, p = kc.BY_NAME[name], kc.prepared(name)
    n = 512
    args = [p[k][:n] for k in ("x", "uw", "uh", "ud", "wy", "wl")]
    a, b = (kc.fd_gradients(case, *args, h) for h in kc.FD_STEPS)
    keep = np.ones(n, dtype=bool)
    for ga, gb in zip(a, b):
        with np.errstate(invalid="ignore"):
            keep &= (np.abs(ga - gb) <= kc.FD_AGREE * (1.0 + np.abs(ga))).reshape(n, -1).all(axis=1)
    assert 1.0 - keep.mean() <= 0.02, (name, keep.mean())
    worst = 0.0
    for fd, t in zip(a, p["truth"]):
        d = (np.abs(fd - t[:n]) / (1.0 + np.abs(t[:n]))).reshape(n, -1)[keep]
        worst = max(worst, float(d.max()))
    print("%-24s %d of %d rows kept, worst |fd - autograd| / (1 + |g|) = %.2e" % (name, int(keep.sum()), n, worst))
    assert worst <= kc.FD_AGREE


# ------------------------------------------------------------------------------------------------------ NaN pattern
def test_derivative_logit_below_minus_88_gives_zero_not_nan(lib):
    """K = 2, unit box, inverse, widths / heights at scale 3, derivative logits at scale 25, seed 0: row 4092 has a
    derivative logit of -116.5.  `sigmoid_beta` evaluated 1 / (1 + exp_noclamp(116.5)), and exp_noclamp past 88.7 is
    fma(inf, lo, inf) with lo <= 0: NaN, where the reference's fp32 autograd has (-)0.  Fixed by taking exp(z) itself
    below -87.  The non-finite pattern of the whole vector is the reference's in both directions."""
    for inverse in (False, True):
        case = kc.Case("probe", 2, False, inverse, kc.UNIT, 0.0, 3.0, 25.0, False, None, "both", 0)
        p = kc.probe_inputs(0)
        assert p["ud"][4092, 0] < -116.0
        status, got = host_backward(lib, case, p)
        ref = kc.autograd_gradients(case, *(p[k] for k in ("x", "uw", "uh", "ud", "wy", "wl")), np.float32)
        assert status == 0
        n = p["x"].size
        assert np.array_equal(kc.nonfinite_pattern(got, n), kc.nonfinite_pattern(ref, n)), inverse
        assert got[1][4092, 4] == 0.0


@pytest.mark.parametrize("tails", [True, False])
@pytest.mark.parametrize("K", [2, 8])
def test_nan_pattern_with_extreme_derivative_logits(lib, K, tails):
    """Derivative logits at -120, -104, -90, -88, -87, -86, -21, 21, 30, 120 (both sides of every threshold of softplus
    and its derivative, with and without the identity initialisation's beta): no NaN / inf where the reference's fp32
    has none, and the rows meet the gradient rule against float64."""
    values = np.array([-120.0, -104.0, -90.0, -88.0, -87.0, -86.0, -21.0, 21.0, 30.0, 120.0], dtype=np.float32)
    for inverse in (False, True):
        for ident in (False, True):
            case = kc.Case("extreme", K, tails, inverse, None if tails else kc.UNIT, 0.0, 1.5, 1.5, ident, None, "both", 8800 + K)
            x, uw, uh, ud = kc.inputs(case, 1024)
            rng = np.random.RandomState(5)
            ud[:] = values[rng.randint(0, values.size, size=ud.shape)]
            wy, wl = kc.weights(case, 1024)
            p = kc.truth_for(case, x, uw, uh, ud, wy, wl)
            p.update(x=x, uw=uw, uh=uh, ud=ud, wy=wy, wl=wl, outside=kc.outside_box(case, x))
            for instance in [0] + ([8] if K == 8 else []):
                status, got = host_backward(lib, case, p, instance)
                assert status == 0
                assert np.array_equal(kc.nonfinite_pattern(got, 1024), kc.nonfinite_pattern(p["ref"], 1024)), (inverse, ident)
                rbad, rkeep = kc.rows_outside(p["ref"], p)
                cap = max(2.0 * rbad[rkeep].mean(), 5e-3)     # (1024 rows: the reference's own share, at least 5 rows)
                kc.assert_rows(got, p, cap, what="extreme K=%d tails=%d inverse=%d ident=%d" % (K, tails, inverse, ident), verbose=True)


# ------------------------------------------------------------------------------------------------------------ knots
@pytest.mark.parametrize("name", kc.KNOT_CASES)
def test_inputs_on_the_knots(lib, name):
    """Inputs on every knot, next to it, on and next to the box ends: each row against the float64 gradient one `delta`
    to the left OR to the right (k1_backward_cases.prepared_knots), at twice the share the reference's own fp32 leaves
    outside under the same rule -- and, as in the table, the host build at half of that."""
    pk = kc.prepared_knots(name)
    case = pk["case"]
    for instance in [0] + ([8] if case.K == 8 else []):
        status, got = host_backward(lib, case, pk, instance)
        share = kc.assert_knot_rows(got, status, pk, kc.KNOT_CAP[name], what="%s [instance %d]" % (name, instance), verbose=True)
        assert share <= 0.5 * kc.KNOT_CAP[name], (name, instance, share)


@pytest.mark.parametrize("inverse", [False, True])
def test_right_end_where_the_search_epsilon_vanishes(lib, inverse):
    """The reference searches with the last knot moved up by 1e-6 (torchutils.searchsorted); on a box whose end is 32 that
    is below half an ulp, an input ON the end finds no bin and the reference fails with an index error.  The forward
    kernels answer with the identity, logabsdet 0 and NFA_STATUS_OUTSIDE_DOMAIN; the backward with the identity's
    gradient and the same status -- for the same inputs as the host build of the forward evaluation."""
    from nflows_amd import _native as N, ops
    K, n = 8, 8
    rng = np.random.RandomState(11)
    for tails, kw in ((True, dict(tail_bound=32.0)), (False, dict(left=-32.0, right=32.0, bottom=-32.0, top=32.0))):
        spec = ops.make_rqs_spec(K, "linear" if tails else None, **kw)
        x = np.array([32.0, np.nextafter(np.float32(32.0), np.float32(0.0)), -32.0, 1.0, 32.0, 0.0, -7.0, 31.0], dtype=np.float32)
        pr = rng.randn(n, 3 * K + (-1 if tails else 1)).astype(np.float32)
        wy, wl = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
        for instance in (0, 8):
            y, lad, gx, gp = np.empty_like(x), np.empty_like(x), np.empty_like(x), np.empty_like(pr)
            fwd = lib.host_rqs_forward(instance, int(inverse), n, ctypes.byref(spec), P(x), P(pr), P(y), P(lad))
            bwd = lib.host_rqs_backward(instance, int(inverse), n, ctypes.byref(spec), P(x), P(pr), P(wy), P(wl), P(gx), P(gp))
            assert fwd == bwd == N.STATUS_OUTSIDE_DOMAIN
            on_end = x == np.float32(32.0)
            assert np.array_equal(y[on_end], x[on_end]) and not lad[on_end].any()
            assert np.array_equal(gx[on_end], wy[on_end]) and not gp[on_end].view(np.uint32).any()
            strictly = np.abs(x) < np.float32(32.0)      # (one ulp below the end included: that one is an ordinary input)
            assert np.all(lad[strictly] != 0) and np.all(gp[strictly].any(axis=1)) and np.isfinite(gp).all() and np.isfinite(gx).all()
