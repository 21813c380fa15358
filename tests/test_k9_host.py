"""The sibling splines' arithmetic of the PRODUCT on the CPU (nflows_amd/csrc/splines_lq.hip compiled for the host on the
real helpers of rqs_math.hpp: tests/_hostcore/splines_lq_host.py):
  * forward: `linear_eval` / `quadratic_eval` / `cubic_eval`, run-time-K and K = 8 / 10 instances, against the reference's
    vectors (splines_lq.npz, splines_cubic.npz) with the rule the oracle and the GPU kernels are held to;
  * backward: the bodies of the three backward kernels against the reference's autograd (splines_lq_grads.npz) -- the
    rule of the GPU test: error against the float64 gradient <= 4 x the reference's own fp32 error + 2e-5 x scale.
CPU only; catches an algebra error in the kernel source before a GPU sees it (the inverse quadratic root's implicit
differentiation was developed this way)."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from _hostcore import splines_lq_host
from helpers import LAD_TOL, OUT_TOL, assert_sibling_spline_parity, parse_kwargs

KIND = {"linear": 0, "quadratic": 1, "cubic": 2}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return splines_lq_host.build(str(tmp_path_factory.mktemp("lqhost")))


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "splines_lq_grads.npz"))


def P(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def spec_of(K, kw):
    from nflows_amd import ops
    kw = dict(kw)
    tails = kw.pop("tails", None)
    return ops.make_rqs_spec(K, tails if tails == "linear" else None, **kw)


def rows(t):
    return np.ascontiguousarray(t.reshape(-1, t.shape[-1]), dtype=np.float32)


def forward_case(lib, g, name, kind, logits, kw):
    x = g[name + "/x"]
    xs = np.ascontiguousarray(x.reshape(-1), dtype=np.float32)
    K = logits[0].shape[-1]
    spec = spec_of(K, kw)
    L = [rows(t) for t in logits[:2]] + [np.ascontiguousarray(t.reshape(-1), dtype=np.float32) for t in logits[2:]]
    L += [None] * (4 - len(L))
    nh = logits[1].shape[-1] if kind == "quadratic" else 0
    count = 0
    for inverse in (False, True):
        pre = name + ("/inv_" if inverse else "/")
        for kt in [0] + ([K] if K in (8, 10) else []):
            y, lad = np.empty_like(xs), np.empty_like(xs)
            status = lib.lq_forward(KIND[kind], kt, int(inverse), xs.size, ctypes.byref(spec), nh, P(xs), P(L[0]), P(L[1]),
                                    P(L[2]), P(L[3]), P(y), P(lad))
            assert status == 0, (name, inverse, kt)
            what = "%s%s [instance %d]" % (name, " inverse" if inverse else "", kt)
            assert_sibling_spline_parity(y.reshape(x.shape), g[pre + "y"], g[pre + "y64"], OUT_TOL, 5e-5, what + " y")
            assert_sibling_spline_parity(lad.reshape(x.shape), g[pre + "lad"], g[pre + "lad64"], LAD_TOL, 1e-3, what + " lad")
            if kw.get("tails") == "linear":
                tb = np.float32(kw["tail_bound"])
                outside = ~((xs >= -tb) & (xs <= tb))
                assert np.array_equal(y[outside].view(np.uint32), xs[outside].view(np.uint32)), what
                assert np.all(lad[outside] == 0), what
            count += 1
    return count


def test_linear_and_quadratic_forward_values(lib, golden_dir):
    g = np.load(os.path.join(golden_dir, "splines_lq.npz"))
    count = 0
    for name, kind, kw in g["meta"]:
        logits = [g["%s/logits%d" % (name, i)] for i in range(1 if kind == "linear" else 2)]
        count += forward_case(lib, g, str(name), str(kind), logits, parse_kwargs(kw))
    assert count >= 28


def test_cubic_forward_values(lib, golden_dir):
    g = np.load(os.path.join(golden_dir, "splines_cubic.npz"))
    count = 0
    for name, kind, kw in g["meta"]:
        logits = [g["%s/logits%d" % (name, i)] for i in range(4)]
        count += forward_case(lib, g, str(name), "cubic", logits, parse_kwargs(kw))
    assert count >= 4


def backward_case(lib, G, name, kind, worst):
    x = np.ascontiguousarray(G[name + "/x"].reshape(-1), dtype=np.float32)
    n_logits = {"linear": 1, "quadratic": 2, "cubic": 4}[kind]
    logits = [G["%s/logits%d" % (name, i)] for i in range(n_logits)]
    K = logits[0].shape[-1]
    spec = spec_of(K, dict((m[0], parse_kwargs(m[2])) for m in G["meta"])[name])
    L = [rows(t) for t in logits[:2]] + [np.ascontiguousarray(t.reshape(-1), dtype=np.float32) for t in logits[2:]]
    L += [None] * (4 - len(L))
    nh = logits[1].shape[-1] if kind == "quadratic" else 0
    gy = np.ascontiguousarray(G[name + "/wy"].reshape(-1), dtype=np.float32)
    gl = np.ascontiguousarray(G[name + "/wl"].reshape(-1), dtype=np.float32)
    for inverse in (0, 1):
        gx = np.empty_like(x)
        g = [np.empty_like(t) if t is not None else None for t in L]
        status = lib.lq_backward(KIND[kind], inverse, x.size, ctypes.byref(spec), nh, P(x), P(L[0]), P(L[1]), P(L[2]), P(L[3]),
                                 P(gy), P(gl), P(gx), P(g[0]), P(g[1]), P(g[2]), P(g[3]))
        assert status == 0
        pre = name + "/" + ("inv_" if inverse else "")
        for got, key in [(gx, "gx")] + [(g[i], "glogits%d" % i) for i in range(n_logits)]:
            truth, ref = G[pre + key + "64"], G[pre + key]
            got = got.reshape(truth.shape)
            err, ref_err = np.abs(got - truth).max(), np.abs(ref.astype(np.float64) - truth).max()
            limit = 4 * ref_err + 2e-5 * (1 + np.abs(truth).max())
            assert err <= limit, "%s%s: %.3e > %.3e" % (pre, key, err, limit)
            worst.append(err / limit)


def test_backward_adjoints(lib, G):
    worst = []
    for name, kind, _ in G["meta"]:
        backward_case(lib, G, str(name), str(kind), worst)
    assert len(worst) == 2 * (8 * 2 + 8 * 3 + 6 * 5 + 1 * 2 + 1 * 3)   # every case of the fixture, both directions


def test_inverse_quadratic_root_is_differentiated_without_cancellation(lib, G):
    """Flat bins (equal heights at the two knots: qa -> 0) make (-1 + qb / r) cancel in the chain through the closed-form
    root; the kernel differentiates the root implicitly.  On the unconstrained fixtures the height-logit gradient of
    the inverse is then at least 10 x closer to float64 than the reference's own fp32 autograd."""
    meta = dict((m[0], parse_kwargs(m[2])) for m in G["meta"])
    for name in ("uquad_k8", "uquad_k10", "uquad_k4"):
        x = np.ascontiguousarray(G[name + "/x"], dtype=np.float32)
        w, h = rows(G[name + "/logits0"]), rows(G[name + "/logits1"])
        spec = spec_of(w.shape[1], meta[name])
        gx, g0, g1 = np.empty_like(x), np.empty_like(w), np.empty_like(h)
        lib.lq_backward(1, 1, x.size, ctypes.byref(spec), h.shape[1], P(x), P(w), P(h), None, None, P(G[name + "/wy"]),
                        P(G[name + "/wl"]), P(gx), P(g0), P(g1), None, None)
        truth, ref = G[name + "/inv_glogits164"], G[name + "/inv_glogits1"]
        assert np.abs(g1 - truth).max() * 10 <= np.abs(ref - truth).max(), name


# ---------------------------------------------------------------------------------------------------------------------
# The case table of tests/k9_cases.py under the float64-truth rules of tests/helpers.py (the GPU suite runs the same
# cases and rules through the kernels: tests/test_gpu_k9.py).  Run with -s for the per-case figures.
import k9_cases  # noqa: E402
from helpers import assert_gradient_rows, assert_sibling_truth_parity  # noqa: E402


def host_forward(lib, kind, K, kw, inverse, x, logits, kt):
    spec = spec_of(K, kw)
    L = [np.ascontiguousarray(a) for a in logits[:2]] + [np.ascontiguousarray(a.reshape(-1)) for a in logits[2:]]
    L += [None] * (4 - len(L))
    nh = logits[1].shape[-1] if kind == "quadratic" else 0
    y, lad = np.empty_like(x), np.empty_like(x)
    status = lib.lq_forward(KIND[kind], kt, int(inverse), x.size, ctypes.byref(spec), nh, P(x), P(L[0]), P(L[1]), P(L[2]),
                            P(L[3]), P(y), P(lad))
    return y, lad, status


def host_backward(lib, kind, K, kw, inverse, x, logits, wy, wl):
    spec = spec_of(K, kw)
    L = [np.ascontiguousarray(a) for a in logits[:2]] + [np.ascontiguousarray(a.reshape(-1)) for a in logits[2:]]
    L += [None] * (4 - len(L))
    nh = logits[1].shape[-1] if kind == "quadratic" else 0
    gx = np.empty_like(x)
    g = [np.empty_like(t) if t is not None else None for t in L]
    status = lib.lq_backward(KIND[kind], int(inverse), x.size, ctypes.byref(spec), nh, P(x), P(L[0]), P(L[1]), P(L[2]), P(L[3]),
                             P(wy), P(wl), P(gx), P(g[0]), P(g[1]), P(g[2]), P(g[3]))
    assert status == 0
    return [gx] + [a.reshape(t.shape) for a, t in zip(g, logits)]


@pytest.mark.parametrize("name", [c.name for c in k9_cases.CASES])
def test_table_forward(lib, name):
    """Values and logabsdet of every case against the float64 oracle, at the share a case must reach to be in the table
    (at most 0.05 % outside; the kernels are held to 0.1 %).  K = 8 / 10: the run-time-K and the compile-time instance,
    bit for bit the same."""
    case, p = k9_cases.BY_NAME[name], k9_cases.prepared(name)
    kw = k9_cases.spec_kwargs(case)
    y, lad, status = host_forward(lib, case.kind, case.K, kw, case.inverse, p["x"], p["logits"], 0)
    assert_sibling_truth_parity((y, lad), p["ref"][:2], p["truth"], p["cond"], p["x"], status, case.inverse,
                                None if case.box else k9_cases.TAIL_BOUND, bulk=k9_cases.HOST_SHARE, what=name, verbose=True)
    if case.K in (8, 10):
        y2, lad2, status2 = host_forward(lib, case.kind, case.K, kw, case.inverse, p["x"], p["logits"], case.K)
        assert status2 == status
        assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)) and np.array_equal(lad.view(np.uint32), lad2.view(np.uint32))


@pytest.mark.parametrize("name", [c.name for c in k9_cases.CASES])
def test_table_backward(lib, name):
    """The backward bodies against central differences of the float64 oracle, under the caps the real reference's own
    fp32 autograd sets (k9_cases.GRAD_CAP)."""
    case, g = k9_cases.BY_NAME[name], k9_cases.prepared_gradients(name)
    assert 1.0 - g["keep"].mean() <= k9_cases.FD_DROP_CAP, "the difference quotient's two step sizes disagree on too many rows"
    got = host_backward(lib, case.kind, case.K, k9_cases.spec_kwargs(case), case.inverse, g["x"], g["logits"], g["wy"], g["wl"])
    assert_gradient_rows(got, g["truth"], g["cond"], g["keep"], k9_cases.GRAD_CAP[(case.kind, case.inverse)],
                         outside=k9_cases.outside_box(case, g["x"]), gy=g["wy"], tol=k9_cases.GRAD_TOL, what=name, verbose=True)


def test_gradient_caps_are_the_references(golden_dir):
    """k9_cases.REFERENCE_GRAD_OUTSIDE is what the gradient rule leaves outside on the real reference's fp32 autograd."""
    assert k9_cases.reference_gradient_shares(golden_dir) == k9_cases.REFERENCE_GRAD_OUTSIDE
    for key, (bad, rows_) in k9_cases.REFERENCE_GRAD_OUTSIDE.items():
        assert k9_cases.GRAD_CAP[key] == max(2.0 * bad / rows_, 1e-3)


def edge_cases(golden_dir):
    """(name, kind, K, kw, inverse, x, logits, ref, truth, cond) of tests/golden/splines_lq_edges.npz: the REAL reference on
    and next to the ends of the box; conditioning from the float64 oracle."""
    g = np.load(os.path.join(golden_dir, "splines_lq_edges.npz"))
    for name, kind, kw in g["meta"]:
        name, kind, kw = str(name), str(kind), parse_kwargs(kw)
        x = g[name + "/x"]
        logits = [g["%s/logits%d" % (name, i)] for i in range({"linear": 1, "quadratic": 2, "cubic": 4}[kind])]
        K = logits[0].shape[1]
        for inverse in (False, True):
            pre = name + ("/inv_" if inverse else "/")
            cond = k9_cases.value_truth(kind, K, kw, x, logits, inverse)["cond"]
            yield (name + (" inverse" if inverse else ""), kind, K, kw, inverse, x, logits, (g[pre + "y"], g[pre + "lad"]),
                   (g[pre + "y64"], g[pre + "lad64"]), cond)


def pooled_edge_ratios(pool):
    """Condition 4 per kind, direction and output on the pooled cases of the edge fixture (4 x 512 elements)."""
    from helpers import assert_trimmed_error_ratio
    for key in sorted(pool):
        e_got, e_ref, mag = (np.concatenate(v) for v in zip(*pool[key]))
        assert_trimmed_error_ratio(e_got, e_ref, mag, what="edges pooled %s %s %s" % key, verbose=True)


def test_box_edges_against_the_reference(lib, golden_dir):
    """Inputs on the box ends, one ulp inside and in the outer 0.5 % of the box, against the real reference's vectors:
    the rule of the table with the share of condition 3 at 99.5 %.  A case has 512 elements, of which the 99.9 %
    quantile would be an interpolation between the two worst -- a rule on the maximum, which there cannot be --, so
    condition 4 is applied to the four cases of a kind and direction together (2048 elements)."""
    count, pool = 0, {}
    for name, kind, K, kw, inverse, x, logits, ref, truth, cond in edge_cases(golden_dir):
        for kt in [0] + ([K] if K in (8, 10) else []):
            y, lad, status = host_forward(lib, kind, K, kw, inverse, x, logits, kt)
            fig = assert_sibling_truth_parity((y, lad), ref, truth, cond, x, status, inverse, kw.get("tail_bound"),
                                              bulk=k9_cases.EDGE_SHARE, what="edges " + name, verbose=kt == 0, ratios=False)
            if kt == 0:
                for nm in ("y", "lad"):
                    pool.setdefault((kind, "inverse" if inverse else "forward", nm), []).append(fig[nm]["errors"])
            count += 1
    assert count == 36
    pooled_edge_ratios(pool)


def test_cubic_inverse_leaves_the_box_in_the_reference_too(golden_dir):
    """The known quirk of the cubic inverse at the top of the box (cubic.py:212-224: when no root of the three-root branch
    falls inside the bin +- 1e-5, the first is taken).  Element 258 of cubic_k5_s3 in the edge fixture -- input exactly
    +3.0, float64 result 3.0 -- comes back as 11.9457 from the REAL reference's fp32, and a third of the inputs at +3.0
    come back up to 1e-4 outside the box.  The kernel restates that selection and keeps it."""
    g = np.load(os.path.join(golden_dir, "splines_lq_edges.npz"))
    x, y, y64 = g["cubic_k5_s3/x"], g["cubic_k5_s3/inv_y"], g["cubic_k5_s3/inv_y64"]
    assert x[258] == np.float32(3.0) and abs(y64[258] - 3.0) < 1e-9 and abs(y[258] - 11.9457) < 1e-3
    for name in ("cubic_k8_s1.5", "cubic_k8_s3", "cubic_k5_s1.5", "cubic_k5_s3"):
        top = g[name + "/x"] == np.float32(3.0)
        outside = np.abs(g[name + "/inv_y"][top]) > 3.0
        assert top.sum() == 64 and 10 <= outside.sum() <= 32, (name, int(outside.sum()))
