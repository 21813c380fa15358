"""The table of tests/cdf_shared_cases.py (K6, nflows_amd/csrc/rqs_shared.hip) on the CPU:
  * every case, and every edge case, with the ORACLE's float32 result in the implementation's place -- its elements, and
    their row sums formed in fp32 one term after the other -- under the rules tests/test_gpu_cdf_shared.py applies to
    the kernel.  No case may set a rule that a correct fp32 evaluation cannot meet: the oracle has to meet each with room
    (`ROOM`), and its own figure stands next to the case in `ORACLE_ROW_SUMS`;
  * K6's plans at the LDS boundary, from the host shim of the launch planner (tests/launch_plan_shim.py);
  * the golden fixture of the four CDF classes: the conditions that the real reference alone has to meet on it.
CPU only."""
import os
import shutil

import numpy as np
import pytest

import cdf_shared_cases as C

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

ROOM = 0.5   # the oracle's fp32 row sums use at most half of their allowance, on every row of every case

# case -> the largest |fp32 row sum - float64 row sum| / allowance of the oracle's float32 over the case's rows (F > 1),
# as this test computes it; held to the recomputed figure below within 0.02 (libm's last bits may differ between hosts)
ORACLE_ROW_SUMS = {
    "f3_k8_fwd_box_s3": 0.088, "f3_k10_inv_box_s1.5": 0.063, "f3_k16_fwd_tails_s1.5": 0.106, "f3_k2_inv_tails_s3": 0.073,
    "f5_k10_fwd_box_s1.5": 0.038, "f5_k16_inv_box_s3": 0.062, "f5_k2_fwd_tails_s3": 0.009, "f5_k8_inv_tails_s1.5": 0.054,
    "f32_k16_fwd_box_s3": 0.037, "f32_k2_inv_box_s1.5": 0.041, "f32_k8_fwd_tails_s1.5": 0.042, "f32_k10_inv_tails_s3": 0.264,
    "f2x3x4_k2_fwd_box_s1.5": 0.011, "f2x3x4_k8_inv_box_s3": 0.446, "f2x3x4_k10_fwd_tails_s3": 0.053,
    "f2x3x4_k16_inv_tails_s1.5": 0.042,
    "f100_k8_fwd_box_s3": 0.029, "f100_k10_inv_box_s1.5": 0.057, "f100_k16_fwd_tails_s1.5": 0.032, "f100_k2_inv_tails_s3": 0.242,
    "f255_k8_fwd_box_s1.5": 0.018, "f255_k10_inv_box_s3": 0.450, "f255_k2_fwd_tails_s3": 0.019, "f255_k8_inv_tails_s1.5": 0.047,
}


def oracle_as_implementation(p):
    """(y [B, *shape], lad [B]) an fp32 implementation would return if its elements were the oracle's."""
    ry, rl, status = p["ref"]
    B = ry.shape[0]
    rl = rl.reshape(B, -1)
    return ry, (C.fp32_row_sum(rl) if rl.shape[1] > 1 else rl.reshape(-1)), status


def test_table_covers_what_it_promises():
    F = {C.features(c.shape) for c in C.CASES}
    assert {1, 3, 5, 32, 24, 100, 255} <= F and (2, 3, 4) in {c.shape for c in C.CASES}
    assert {c.K for c in C.CASES} == {2, 8, 10, 16} and {c.scale for c in C.CASES} == {1.5, 3.0}
    for f in F:
        assert {(c.tails, c.inverse) for c in C.CASES if C.features(c.shape) == f} == {
            (None, False), (None, True), ("linear", False), ("linear", True)}, f
    for K in (2, 8, 10, 16):
        assert {c.tails for c in C.CASES if c.K == K} == {None, "linear"} and {c.inverse for c in C.CASES if c.K == K} == {False, True}
    assert len({c.name for c in C.CASES}) == len(C.CASES) == len({c.seed for c in C.CASES})
    assert set(ORACLE_ROW_SUMS) == {c.name for c in C.CASES if C.features(c.shape) > 1}


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_oracle_float32_meets_every_rule_of_the_table(name):
    case, p = C.BY_NAME[name], C.prepared(name)
    assert p["x"].shape[0] <= 256
    if case.tails == "linear":
        outside = ~C.in_box(p["x"], case.tails)
        assert 0.04 <= outside.mean() <= 0.05, name
    y, lad, status = oracle_as_implementation(p)
    fig = C.assert_values(y, lad, p["x"], p["ref"], p["truth"], p["cond"], case.tails, case.inverse, status, what="oracle " + name)
    assert fig["finite"] == 1.0 and fig["nan_on_one_side"] == 0.0 and fig["rows_judged"] == 1.0, (name, fig)
    if C.features(case.shape) > 1:
        worst = fig["row_sums"]["worst"]
        assert fig["row_sums"]["share"] == 1.0 and worst <= ROOM, (name, fig)
        assert abs(worst - ORACLE_ROW_SUMS[name]) <= 0.02, (name, worst)


@pytest.mark.parametrize("name", C.EDGE_NAMES)
def test_oracle_float32_meets_every_rule_on_the_knots(name):
    """The edge inputs: on every interior knot of every feature, one ulp to either side, and the ends of the box."""
    case, p = C.BY_NAME[name], C.edge_prepared(name)
    x = p["x"]
    assert x.shape[0] == 3 * (case.K - 1) + 4
    inside = C.in_box(x, case.tails)
    assert (~inside).sum() == (2 * C.features(case.shape) if case.tails == "linear" else 0)
    y, lad, status = oracle_as_implementation(p)
    fig = C.assert_values(y, lad, x, p["ref"], p["truth"], p["cond"], case.tails, case.inverse, status, what="oracle edges " + name,
                          min_rows=C.EDGE_MIN_ROWS)
    assert fig["finite"] >= 0.995 and fig["nan_on_one_side"] == 0.0, (name, fig)
    if "row_sums" in fig:
        assert fig["row_sums"]["share"] == 1.0 and fig["row_sums"]["worst"] <= ROOM, (name, fig)
    if case.tails is None and not case.inverse:
        # the reference's test_zeros_to_zeros / test_ones_to_ones (nonlinearities_test.py:52-66) on the oracle
        B = x.shape[0]
        ends = p["ref"][0].reshape(B, -1)[3 * (case.K - 1):3 * (case.K - 1) + 2]
        assert np.abs(ends[0]).max() <= 1e-5 and np.abs(ends[1] - 1.0).max() <= 1e-5


def test_k6_plans_at_the_lds_boundary():
    """K = 10, tails=None.  Hand-computed from `lds_floats` of nfa_rqs_shared_f32 (33 F table floats, 31 F staged logits,
    two images of R F floats, each piece rounded up to four floats, + 8): 240 features are the last to keep two rows per
    tile, 247 and 248 the last with one row (rows not / 16-byte aligned), 249 the first the kernel refuses.  The values
    tests/test_gpu_cdf_shared.py runs are the shim's (`cases.lds_boundary`); this test says they are the expected ones."""
    b = C.lds_boundary()
    assert b == C.Boundary(halved=240, single_unaligned=247, single_aligned=248, unsupported=249), b
    for F, (ok, R) in ((b.halved, (1, 2)), (b.single_unaligned, (1, 1)), (b.single_aligned, (1, 1)), (b.unsupported, (0, 1))):
        p = C.k6_plan(F, C.BOUNDARY_K, None)
        assert (p.ok, p.R) == (ok, R), (F, p)
        assert 1024 // F == 4 and (not p.ok or p.lds <= 64 * 1024) and (p.ok or p.lds > 64 * 1024), (F, p)
        assert C.k6_plan(F, C.BOUNDARY_K, None, 64) == p          # (the 64 rows of the GPU test do not change the plan)
    assert b.single_unaligned % 4 != 0 and b.single_aligned % 4 == 0 and (4 * b.halved * 2) % 16 == 0
    # which engine each case of the table takes: every one but the F = 255, K = 10 case is K6's
    fallback = [c.name for c in C.CASES if not C.k6_plan(C.features(c.shape), c.K, c.tails).ok]
    assert fallback == ["f255_k10_inv_box_s3"], fallback
    # the tile-boundary and second-pass shapes of the GPU test
    assert C.k6_plan(3, 8, "linear").R == 1024 // 3 and C.k6_plan(100, 8, "linear").R == 1024 // 100
    for cus in (1, 256, 304):
        rows = 2 * 8 * cus * 10 + 7
        tiles = (rows + 9) // 10
        grid = C.k6_grid(cus, 100, 8, "linear", rows)
        assert tiles > 8 * cus >= grid and tiles >= 2 * grid + 1, (cus, tiles, grid)


def test_golden_fixture_meets_the_conditions_stated_for_the_reference(golden_dir):
    """tests/golden/cdf_shared.npz: four classes x two tails x two shapes, batch 64, K = 8; no NaN anywhere; the real
    reference's fp32 against its own fp64 on [2, 3, 4], every class, both directions: y within 1.8e-5, logabsdet within
    3.9e-4, parameter gradients within 0.32 on a scale of at most 1.6e3 (make_golden_cdf_shared.py: `LIMITS`, and the
    parameter seeds it had to change to stay within them)."""
    G = C.golden(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "cdf_shared.npz")) < 1 << 20
    names = [str(n) for n, _, _ in G["meta"]]
    assert len(names) == 16 and {str(k) for _, k, _ in G["meta"]} == {"linear", "quadratic", "cubic", "rq"}
    for key in G.files:
        assert np.isfinite(G[key]).all() if G[key].dtype.kind == "f" else True, key
    for name in names:
        shape = G[name + "/y"].shape
        assert shape[0] == 64 and shape[1:] in ((2, 3, 4), (37,))
        assert [k for k in G.files if k.startswith(name + "/p/")], name
    for name in (n for n in names if n.endswith("2x3x4")):
        worst = {"y": 0.0, "lad": 0.0, "g": 0.0, "g scale": 0.0}
        for pre in (name + "/", name + "/inv_"):
            for k in ("y", "lad"):
                worst[k] = max(worst[k], float(np.abs(C.golden64(G, pre + k) - G[pre + k]).max()))
            for key in [k for k in G.files if k.startswith(pre + "g/") and not k.endswith("_d")]:
                worst["g"] = max(worst["g"], float(np.abs(C.golden64(G, key) - G[key]).max()))
                worst["g scale"] = max(worst["g scale"], float(np.abs(C.golden64(G, key)).max()))
        assert worst["y"] <= 1.8e-5 and worst["lad"] <= 3.9e-4 and worst["g"] <= 0.32 and worst["g scale"] <= 1.6e3, (name, worst)


def test_shared_parameter_gradients_of_the_kernel_source(golden_dir, tmp_path):
    """The rational-quadratic cases of cdf_shared.npz through `rqs_backward` of nflows_amd/csrc/rqs_bwd.hip compiled for
    the host (tests/_hostcore/rqs_f32_host.py), one spline per element on the broadcast logits, the logit gradients summed
    over the batch as autograd's expand does: input and parameter gradients of both directions under
    `helpers.close_to_truth`.  The inverse's width-logit gradients are the ones that missed it before
    `inverse_map_adjoint` (0.27 on a scale of 14 at [37] on the box, where the bound is 1.6e-3: DESIGN.md section 4, "K6")."""
    import ctypes
    import torch
    from _hostcore import rqs_f32_host
    from helpers import close_to_truth, parse_kwargs
    from nflows_amd import ops
    lib = rqs_f32_host.build(str(tmp_path))
    G = C.golden(golden_dir)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    names = ("unnormalized_widths", "unnormalized_heights", "unnormalized_derivatives")
    for name, kind, kw in G["meta"]:
        name, kw = str(name), parse_kwargs(kw)
        if str(kind) != "rq":
            continue
        tag = name.split("_", 1)[1]
        x = G["x/" + tag]
        B, n = x.shape[0], x.size
        params = [G["%s/p/%s" % (name, pn)] for pn in names]
        widths = [p.shape[-1] for p in params]
        packed = np.ascontiguousarray(np.concatenate([np.broadcast_to(p[None], (B,) + p.shape).reshape(n, -1) for p in params], axis=1))
        spec = ops.make_rqs_spec(kw["num_bins"], kw["tails"], tail_bound=kw["tail_bound"])
        xs, gy = np.ascontiguousarray(x.reshape(-1)), np.ascontiguousarray(G["Wy/" + tag].reshape(-1))
        gl = np.ascontiguousarray(np.repeat(G["Wl/" + tag], n // B))
        for inverse in (False, True):
            pre = name + ("/inv_" if inverse else "/")
            for kt in (0, 8):
                gx, gp = np.empty_like(xs), np.empty_like(packed)
                assert lib.host_rqs_backward(kt, int(inverse), n, ctypes.byref(spec), P(xs), P(packed), P(gy), P(gl), P(gx), P(gp)) == 0
                close_to_truth(torch.from_numpy(gx.reshape(x.shape)), G[pre + "gx"], C.golden64(G, pre + "gx"), pre + "gx")
                lo = 0
                for pn, w in zip(names, widths):
                    got = gp[:, lo:lo + w].reshape((B,) + x.shape[1:] + (w,)).astype(np.float64).sum(axis=0)
                    lo += w
                    close_to_truth(torch.from_numpy(got), G[pre + "g/" + pn], C.golden64(G, pre + "g/" + pn), "%sg/%s [instance %d]" % (pre, pn, kt))
