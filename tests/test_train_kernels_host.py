"""The table of tests/train_kernel_cases.py on the CPU: what keeps it honest before a GPU sees it.  Both yardsticks are
recomputed and held to half the stored caps; a torch emulation of the split-bf16 scheme (written from DESIGN.md, not from
the kernels: three bf16 pieces per operand, the six products hh, hm, mh, hl, lh, mm, one fp32 rounding of the accumulator
per product and 16-input k-step) passes every cap -- the scheme CAN satisfy the rule --; the same emulation with one
product dropped misses a cap by 3 x or more in every case that runs that arithmetic -- the rule is sharp --; and the
allowance bounds what one-ulp perturbations of the inputs do to the float64 truth.  CPU only.  -s for the figures."""
import numpy as np
import pytest
import torch

import train_kernel_cases as tk

K14_NAMES = [c.name for c in tk.K14_CASES]
K10_NAMES = [c.name for c in tk.K10_CASES]
SHARP = 3.0
PRODUCTS = ("lh", "hl", "mm", "mh", "hm", "hh")     # small terms first; first letter: the piece of the first operand
STAGE_ROWS = 32


# ------------------------------------------------------------------------------------------------- the emulated scheme
def _pieces(a):
    """[3, rows, k] float64: the bf16 pieces hi, mid, lo of a float32 array (exact in float64)"""
    from nflows_amd import ops
    return torch.stack([p.double() for p in ops.split_bf16x3(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))])


def _mfma_sum(acc, pa, pb, drop):
    """acc [M, N] float32 + sum over k of a[M, k] b[N, k], k in steps of 16: per step and product the 16 bf16 x bf16 terms
    exactly (float64 holds them) and ONE rounding of the accumulator to fp32."""
    k = pa.shape[2]
    pad = -k % 16
    if pad:
        pa, pb = torch.nn.functional.pad(pa, (0, pad)), torch.nn.functional.pad(pb, (0, pad))
    steps = (k + pad) // 16
    pa = pa.view(3, pa.shape[1], steps, 16).permute(0, 2, 1, 3)      # [3, steps, M, 16]
    pb = pb.view(3, pb.shape[1], steps, 16).permute(0, 2, 3, 1)      # [3, steps, 16, N]
    idx = {"h": 0, "m": 1, "l": 2}
    terms = [torch.matmul(pa[idx[p[0]]], pb[idx[p[1]]]) for p in PRODUCTS if p != drop]      # each [steps, M, N]
    acc = torch.from_numpy(np.array(acc, dtype=np.float32))
    for s in range(steps):
        for t in terms:
            acc = (acc.double() + t[s]).float()
    return acc.numpy()


def emulated_linear(drop=None):
    def linear(v, W, b):
        acc = np.zeros((v.shape[0], W.shape[0]), dtype=np.float32)
        if b is not None:
            acc = acc + np.asarray(b, dtype=np.float32)
        return _mfma_sum(acc, _pieces(v), _pieces(W), drop)
    return linear


def emulated_wgrad(drop=None):
    """K10 as DESIGN.md describes it: the batch rows are the k index, full 32-row stages on the matrix cores -- true fp32
    products, two rows per instruction, for I <= 32; the six bf16 products above --, the rows behind the last full stage
    and the bias gradient as plain fp32 sums."""
    def wgrad(x, gy):
        x, gy = tk._f32(x), tk._f32(gy)
        full = x.shape[0] // STAGE_ROWS * STAGE_ROWS
        gw = np.zeros((gy.shape[1], x.shape[1]), dtype=np.float32)
        if full and x.shape[1] > 32:
            gw = _mfma_sum(gw, _pieces(gy[:full].T), _pieces(x[:full].T), drop)
        elif full:
            for r in range(0, full, 2):
                two = gy[r:r + 2].astype(np.float64).T @ x[r:r + 2].astype(np.float64)
                gw = (gw.astype(np.float64) + two).astype(np.float32)
        for r in range(full, x.shape[0]):
            gw = gw + gy[r][:, None] * x[r][None, :]
        return gw, tk.wgrad_seq(x[:, :1], gy)[1]
    return wgrad


def k14_emulated(p, drop=None, skip_into_accumulator=False):
    return tk.stats_of(tk.k14_chain(p["e"], p["xp"], p["gp"], p["masks"], emulated_linear(drop), skip_into_accumulator),
                       p["truth"], p["case"].name)


def k10_emulated(p, drop=None):
    case = p["case"]
    return tk.stats_of(tk.k10_apply(p["problems"], emulated_wgrad(drop), case.need_bias), p["truth"], case.name)


def worst_excess(stats, caps):
    """the largest statistic / cap over arrays and statistics (caps of 0 -- exact arrays -- left out)"""
    return max([s[i] / caps[k][i] for k, s in stats.items() for i in range(3) if caps[k][i] > 0.0] or [0.0])


def runs_the_six_products(case):
    """K14 always; K10 above 32 inputs with at least one full stage"""
    return isinstance(case, tk.K14Case) or (case.I > 32 and case.B >= STAGE_ROWS)


# ------------------------------------------------------------------------------------------------------------ the table
def test_the_table_covers_what_it_says():
    k14, k10 = tk.K14_CASES, tk.K10_CASES
    assert 35 <= len(k14) <= 45 and 35 <= len(k10) <= 45
    assert set(c.di for c in k14) >= {4, 8, 12, 16, 20, 32, 36, 48, 64} and set(c.nb for c in k14) == {0, 1, 2, 3}
    assert set(c.H for c in k14) >= {128, 124, 64, 52, 4} and set(c.out for c in k14 if not c.made) >= {0, 4, 24, 32, 40, 368, 736}
    assert set(c.kind for c in k14) == {"plain", "x_rows", "g_rows", "g_cols", "bias_neg", "bias_pos", "zero_unit", "g_onecol"}
    assert sorted(set(c.made for c in k14 if c.made)) == [21, 63]
    for c in k14:       # the kernels' limits
        assert c.B % 128 == 0 and c.di % 4 == 0 and c.di <= 64 and c.H % 4 == 0 and c.H <= 128 and c.nb <= 3 and c.out % 4 == 0
    assert set(c.I for c in k10) >= {4, 32, 36, 64, 128, 200} and set(c.O for c in k10) >= {4, 40, 96, 128, 260, 736}
    assert set(c.B for c in k10) >= {0, 1, 15, 16, 31, 32, 33, 48, 100, 512, 1000, 1024} and max(c.B for c in k10) <= 1024
    assert set(c.count for c in k10) == {1, 2, 4, 8} and any(not c.need_bias for c in k10)
    assert set(c.kind for c in k10) == {"relu_x", "nonneg", "rows", "cols", "zero_cols"}
    assert set(tk.CAPS) == set(K14_NAMES + K10_NAMES)
    # what the special cases are there for
    p = tk.k14_prepared("bias_neg_out40")
    assert not p["masks"][1].any() and not p["truth"]["grads1"][0].any() and not p["truth"]["grads1"][1].any()
    assert tk.k14_prepared("bias_pos_out40")["masks"][1][:, :128].all()
    p = tk.k14_prepared("zero_unit_out40")
    assert not p["truth"]["saved1"][0][:, tk.ZERO_UNIT].any() and not p["truth"]["saved1"][1][:, tk.ZERO_UNIT].any()
    p = tk.k14_prepared("h52_hidden")
    for name in ("hidden", "saved0", "saved3", "grads0", "grads3"):     # the padded units: no allowance
        assert not p["truth"][name][1][:, 52:].any() and not p["truth"][name][0][:, 52:].any() and p["truth"][name][1][:, :52].any()
    assert p["truth"]["hidden"][1][:, :52].all()
    p = tk.k14_prepared("made21_h64")
    assert any((m == 0).any() for m in p["net"]["masks"]) and not p["truth"]["grad_inputs"][1][:, 21:].any()
    assert not p["truth"]["params"][1][:, 42:].any()
    p = tk.k10_prepared("zero_cols_i64")
    assert not p["truth"]["gw"][1][0, 96 // 3].any() and not p["truth"]["gw"][1][0, :, 32].any() and p["truth"]["gb"][1][0, 32] == 0.0
    x2 = [float(x.abs().max()) for x, _ in tk.k10_prepared("batched4_128x128")["problems"]]
    assert x2[3] > 4.0 * x2[0]


@pytest.mark.parametrize("name", K14_NAMES + K10_NAMES)
def test_yardsticks_are_within_half_the_stored_caps(name):
    """Y_ref (eager fp32) and Y_seq (sequential fp32) recomputed on the case's own inputs: each statistic at most cap / 2
    (the caps are stored rounded up, so a yardstick that moved would show here)."""
    if name in tk.K14_BY_NAME:
        yard = tk.k14_yardsticks(tk.k14_prepared(name))
    else:
        p = tk.k10_prepared(name)
        yard = tk.k10_yardsticks(p["problems"], p["truth"], p["case"].need_bias, name)
    half = dict((k, tuple(c / tk.PARITY for c in v)) for k, v in tk.CAPS[name].items())
    for label, stats in zip(("Y_ref", "Y_seq"), yard):
        tk.report(name + " " + label, stats, tk.CAPS[name])
        bad = tk.misses(stats, half)
        assert not bad, "%s %s above cap / 2: %s" % (name, label, bad)


@pytest.mark.parametrize("name", K14_NAMES + K10_NAMES)
def test_the_emulated_scheme_passes_and_one_dropped_product_does_not(name):
    """The scheme under every cap; without its mm product, and without hl, some statistic at least 3 x above its cap."""
    k14 = name in tk.K14_BY_NAME
    p = tk.k14_prepared(name) if k14 else tk.k10_prepared(name)
    run = k14_emulated if k14 else k10_emulated
    tk.assert_within_caps(name + " emulated", run(p), tk.CAPS[name], verbose=True)
    if runs_the_six_products(p["case"]):
        for drop in ("mm", "hl"):
            excess = worst_excess(run(p, drop), tk.CAPS[name])
            print("%-26s without %s: worst statistic %.1f x its cap" % (name, drop, excess))
            assert excess >= SHARP, "%s: the rule does not see a missing %s product (%.2f x the cap)" % (name, drop, excess)




def test_the_skip_summed_into_the_accumulator_misses_hidden():
    """CHANGED (1) pinned on the CPU: the same emulation with the second Linear of a block accumulating INTO h + b_1, as
    K14's forward kernel did until this table, misses the caps of `hidden` and of nothing else; summed in an accumulator
    of its own (the test above) it passes."""
    for name in ("di4_hidden", "out736"):
        stats = k14_emulated(tk.k14_prepared(name), skip_into_accumulator=True)
        tk.report(name + " skip into acc", stats, tk.CAPS[name])
        assert set(m[0] for m in tk.misses(stats, tk.CAPS[name])) == {"hidden"}, name


def test_the_one_column_case_is_exact():
    """CHANGED (3): a one-column gradient of signed powers of two makes grad_hidden exact in float32 -- caps of zero, the
    emulated scheme and both yardsticks bit for bit on the truth."""
    p = tk.k14_prepared("g_onecol_out40")
    assert tk.CAPS["g_onecol_out40"]["grad_hidden"] == (0.0, 0.0, 0.0)
    assert k14_emulated(p)["grad_hidden"] == (0.0, 0.0, 0.0)
    g = p["g"].numpy()
    assert (g != 0).sum() == g.shape[0] and set(np.abs(g[g != 0])) <= set(2.0 ** k for k in range(-3, 4))


# ---------------------------------------------------------------------------------------------- the allowance is a bound
# Two kinds of perturbation of the INPUTS (x; the output gradient where it enters a GEMM), 256 random draws each:
#   "u":     every element times (1 +- 2^-24) in float64 -- the unit roundoff the allowance is built from.  The truth must
#            stay within the allowance in EVERY element (first-order rigorous: ReLU is 1-Lipschitz, the masks are pinned).
#   "ulp32": every element moved to a float32 neighbour.  One float32 ulp is between 1 and 2 units of 2^-24 relative, so
#            a single-term element may move by up to twice its allowance; in sums of hundreds of terms random signs
#            average and the allowance holds with room -- checked on cases of that kind.
def _perturbed(a, rng, how):
    sign = np.where(rng.rand(*a.shape) < 0.5, -1.0, 1.0)
    if how == "u":
        return np.asarray(a, dtype=np.float64) * (1.0 + tk.U * sign)
    a = np.asarray(a, dtype=np.float32)
    return np.where(a != 0, np.nextafter(a, (sign * np.inf).astype(np.float32)), a).astype(np.float64)


def _assert_bounded(moved, truth, what):
    worst = 0.0
    for k, (t, A) in truth.items():
        d = np.abs(moved[k] - t)
        assert (d <= A * (1.0 + 1e-6)).all(), (what, k, float((d / np.where(A > 0, A, 1e-300)).max()))
        if (A > 0).any():
            worst = max(worst, float((d[A > 0] / A[A > 0]).max()))
    return worst


@pytest.mark.parametrize("name,how", [("nb2_out40", "u"), ("x_rows_out40", "u"), ("h52_hidden", "u"), ("made21_h64", "u"),
                                      ("di64_hidden", "u"), ("out736", "ulp32")])
def test_the_k14_allowance_bounds_input_perturbations(name, how):
    """x perturbed: the forward arrays; the output gradient perturbed (cases with a final Linear: without one it passes
    through closed masks unchanged, where the allowance is rightly zero): the backward arrays.  "ulp32" on the gradient of
    the 736-wide case only (sums of 736 terms)."""
    p = tk.k14_prepared(name)
    case, rng, worst = p["case"], np.random.RandomState(5), 0.0
    fwd = dict((k, p["truth"][k]) for k in tk.forward_arrays(case.nb, bool(case.out)))
    bwd = dict((k, p["truth"][k]) for k in tk.backward_arrays(case.nb, bool(case.out)))
    for _ in range(256):
        if how == "u":
            moved = tk.k14_forward_truth(p["e"], _perturbed(p["xp"], rng, how))[0]
            worst = max(worst, _assert_bounded(dict((k, v[0]) for k, v in moved.items()), fwd, name))
        if case.out:
            moved = tk.k14_backward_truth(p["e"], _perturbed(p["gp"], rng, how), p["masks"])
            worst = max(worst, _assert_bounded(dict((k, v[0]) for k, v in moved.items()), bwd, name))
    print("%-26s %s perturbations move the truth by at most %.3f of the allowance" % (name, how, worst))


@pytest.mark.parametrize("name,how", [("i128_o128", "u"), ("rows_i64", "u"), ("b33_i36", "u"), ("b1_i36", "u"), ("b1024_i36", "ulp32")])
def test_the_k10_allowance_bounds_input_perturbations(name, how):
    """x and gy perturbed in turn (both at once move a product by two units)"""
    p = tk.k10_prepared(name)
    rng, worst = np.random.RandomState(6), 0.0
    x, gy = (tk._f32(t).astype(np.float64) for t in p["problems"][0])
    truth = dict((k, (t[0], A[0])) for k, (t, A) in p["truth"].items())
    for trial in range(256):
        xs, gs = (_perturbed(x, rng, how), gy) if trial % 2 else (x, _perturbed(gy, rng, how))
        worst = max(worst, _assert_bounded({"gw": gs.T @ xs, "gb": gs.sum(axis=0)}, truth, name))
    print("%-26s %s perturbations move the truth by at most %.3f of the allowance" % (name, how, worst))
