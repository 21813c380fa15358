"""The cases of K32's exact-logit suite and K33's bit-for-bit suite (test infrastructure, not a conftest): shared by
tests/test_gpu_wide_exact.py, tests/test_gpu_wide_train_exact.py (device) and tests/test_wide_exact_host.py (host: the
recipes' exactness, stock torch against the exact values, the caps on the oracle's own fp32)."""
import numpy as np

import exact_logits as X

# ---- K32: (name, hidden width, D, bins, keywords of test_gpu_exact_logits._case) -- the smallest shapes that reach each
# mechanism; two residual blocks unless stated
# (`reseed`: 1 -- the second draw of the transformed inputs: see "Inputs and the reference's own tail" below)
K32_CASES = [("h256_k%d" % K, 256, 64, K, {"reseed": 1} if K in (10, 11) else {})
             for K in range(2, 17)]         # all 30 instances; T = 1 -> 2 at 5 / 6, 2 -> 3 at 11 / 12
K32_CASES += [
    ("h256_d62_k8", 256, 62, 8, {"variant": "odd", "reseed": 1}),       # 31 transformed features: a padded group,
    ("h256_d62_k11", 256, 62, 11, {"variant": "odd"}),                  # a half-used pair
    ("h256_two_layer_k8", 256, 64, 8, {"variant": "two_layer"}),        # second layer of a flow: logabsdet accumulated into
    ("h256_d128_k16", 256, 128, 16, {"features": 128, "num_blocks": 1}),   # 32 pairs, T = 3: the LDS / geometry limit
    ("h256_long_k8", 256, 64, 8, {"recipe": "long"}),                   # all three operand pieces on both sides
    ("h129_k5", 129, 64, 5, {"reseed": 1}),                             # Hp = 160: waves 5 .. 7 idle, folded scale
    ("h129_k12", 129, 64, 12, {}),
    ("h129_d6_k3", 129, 6, 3, {"features": 6, "reseed": 1}),              # 3 transformed, 2 pairs: six waves without one
    ("h160_k8", 160, 64, 8, {}),                                        # no hidden padding at five tiles
    ("h192_k6", 192, 64, 6, {}),
    ("h192_k11", 192, 64, 11, {"reseed": 1}),
    ("h256_blocks0_k8", 256, 64, 8, {"num_blocks": 0, "reseed": 1}),             # the `nb > 0` branches, the prefetch hand-over
    ("h256_blocks1_k8", 256, 64, 8, {"num_blocks": 1}),
    ("h256_blocks3_k8", 256, 64, 8, {"num_blocks": 3}),
]
# Inputs and the reference's own tail.  helpers.assert_error_ratio on 2048 rows compares the THIRD-worst row (the 99.9 %
# quantile) with 4 x the reference fp32's.  In the inverse an input within an ulp of a height knot beside a bin of
# derivative 1e-3 costs ANY fp32 evaluation an error of about 10 in that row's log-determinant (a root 2e-4 past the bin's
# end cancels the derivative's numerator; the oracle's fp32 has such rows in most cases, and the kernels' own fp32 knots
# differ from the oracle's by an ulp, so theirs fall on other rows).  Where the reference itself has exactly two such rows
# its quantile sits beneath a cliff and one more row of the reference's OWN size fails the rule.  A case's inputs must
# therefore satisfy, by the reference alone (`reference_tail_covered`, asserted in tests/test_wide_exact_host.py):
# 4 x its quantile >= its maximum, in both directions.  Seven cases (h256_k10, h256_k11, h256_d62_k8, h129_k5, h129_d6_k3,
# h192_k11, h256_blocks0_k8) miss that on the first draw of their transformed inputs and take the second (`reseed`: 1),
# which meets it; conditioners, logits and identity rows are unchanged.
K32_BY_NAME = {c[0]: c for c in K32_CASES}


def reference_tail_covered(case):
    """the condition above on a case's inputs: per direction (99.9 % quantile, maximum) of the reference fp32's per-row
    log-determinant error against float64, and whether 4 x the quantile covers the maximum"""
    figures = []
    for direction in ("fwd", "inv"):
        o = case[direction][3]
        fin = np.isfinite(o["row32"]) & np.isfinite(o["row64"])
        e = np.abs(o["row32"][fin].astype(np.float64) - o["row64"][fin])
        figures.append((float(np.quantile(e, 0.999)), float(e.max())))
    return all(4.0 * q >= m for q, m in figures), figures


def k32_case(name):
    """test_gpu_exact_logits._case of a K32 case (cached there, one case at a time)"""
    from test_gpu_exact_logits import _case
    _, hidden, _, K, more = K32_BY_NAME[name]
    return _case(K, "linear", False, hidden=hidden, **more)


def k32_conditioner(name, inverse=False):
    """(the conditioner under test, its identity rows, K) of a K32 case without the oracle: the premise test's inputs"""
    from test_gpu_exact_logits import _flow, _identity
    _, hidden, _, K, more = K32_BY_NAME[name]
    _, layer, _, _, fold = _flow(K, "linear", False, hidden, **{k: v for k, v in more.items() if k != "reseed"})
    ident = _identity(K, more.get("variant", ""), more.get("recipe", "dyadic"), len(layer.identity_features), inverse)
    return layer.transform_net, ident, K, fold


def check_k32(what, case, K, result):
    """The checks of a K32 case on `result` = {"z", "lad", "lp", "x", "ladi"} ([ROWS, ...] arrays in the coordinates of the
    layer under test): test_gpu_exact_logits._check in both directions under the rule of the `k8` engine (the same
    rqs_eval<K, ., linear tails, registers>: forward_ratio asserted, none of the FusedSteps relaxations), and log_prob per
    row as that suite checks it."""
    from helpers import LAD_TOL, assert_error_ratio
    from test_gpu_exact_logits import _check
    _check(what + " forward", case, "fwd", result["z"], result["lad"], K, "linear", True, False)
    _check(what + " inverse", case, "inv", result["x"], result["ladi"], K, "linear", True, False)
    o, lp = case["fwd"][3], result["lp"]
    assert np.array_equal(np.isinf(lp), np.isinf(o["lp32"])), what + ": log_prob inf pattern"
    fin = np.isfinite(o["lp32"]) & np.isfinite(o["lp64"])
    X.assert_row_allowance(lp[fin], o["lp64"][fin], o["lp32"][fin], o["cond_row"][fin], LAD_TOL, what + " log_prob per row",
                           bulk=0.995)
    assert_error_ratio(lp[fin], o["lp32"][fin], o["lp64"][fin], what + " log_prob per row")


def oracle_result(case):
    """the oracle's own fp32 result in the place of a kernel's: what `check_k32` must accept (the caps are conditions on the
    inputs)"""
    out = {}
    for direction, y, lad in (("fwd", "z", "lad"), ("inv", "x", "ladi")):
        full, _, _, o, _ = case[direction]
        got = full.copy()
        got[:, case["ti"]] = o["y32"]
        out[y], out[lad] = got, np.asarray(o["row32"], dtype=np.float32)
    out["lp"] = np.asarray(case["fwd"][3]["lp32"], dtype=np.float32)
    return out


# ---- K33: (features in, width, blocks, out, rows, recipe), each for one mechanism.  rows "cus": 64 x (CU count + 1)
CUS = "cus"
K33_SHAPES = [
    (3, 129, 1, 20, 64, "dyadic"),        # a 20-column `params` tile: the shape of the recorded compiler reordering
    (33, 160, 1, 44, 128, "dyadic"),      # g_x's second output tile at d_i = 33
    (32, 256, 2, 256, 64, "dyadic"),      # `out` exactly one 256-column chunk
    (8, 192, 2, 257, 64, "dyadic"),       # one column in a second chunk
    (16, 256, 2, 736, 128, "dyadic"),     # three chunks summed in accumulators of their own
    (16, 256, 2, 736, 128, "long"),       # ... with every bf16 piece of one factor of every product in use
    (64, 256, 3, 1472, 64, "dyadic"),
    (16, 256, 0, 0, 64, "dyadic"),        # hidden only, `g` zero-padded to Hp
    (6, 160, 1, 44, CUS, "dyadic"),       # second pass: the last 64 rows equal to those rows run alone
]
CLASS_WIDTHS = (129, 256)                 # ResidualNet(8, 40, hidden_features=H, num_blocks=2) at 128 rows


def bins_dividing(out):
    """a bin count whose 3 K - 1 parameters per feature divide `out` (the recipes ask for one; regimes are off)"""
    return next(K for K in range(1, out + 2) if out % (3 * K - 1) == 0)


def k33_problem(di, H, nb, out, rows, recipe, seed=21):
    """(net on the CPU, x [rows, di], g [rows, out] or [rows, H], exact forward, exact backward) of a K33 shape: dyadic x
    and g (long recipe: powers of two, one nonzero of g per row), every product checked by exact_logits._exact_linear"""
    from nflows_amd.nn.nets.resnet import ResidualNet
    rng = np.random.RandomState(seed)
    net = ResidualNet(di, out or 4, hidden_features=H, num_blocks=nb)
    K = bins_dividing(out or 4)
    if recipe == "long":
        X.long_mantissa_conditioner(net, K, "linear", seed=seed)
        x = X.long_identity_rows(rows, di, seed + 1)
        g = np.zeros((rows, out))
        g[np.arange(rows), rng.randint(0, out, rows)] = rng.choice((-1.0, 1.0), rows) * np.exp2(rng.randint(-2, 3, rows))
    else:
        X.dyadic_conditioner(net, K, "linear", seed=seed, regimes=False)
        x = X.identity_rows(rows, di, seed + 1)
        g = rng.randint(-4, 5, (rows, out or H)) / 2.0
    forward = X.exact_forward(net, x, with_final=bool(out))
    backward = X.exact_backward(net, forward, g, weight_grads=False, with_final=bool(out))
    return net, x, g, forward, backward


def class_problem(H, seed=31):
    """(net, x, g, exact forward, exact backward with every parameter gradient) of the class-path case: the weight
    gradients are [H, 128] x [128, H] products over the rows, whose budget `_exact_linear` checks on this data"""
    from nflows_amd.nn.nets.resnet import ResidualNet
    net = ResidualNet(8, 40, hidden_features=H, num_blocks=2)
    X.dyadic_conditioner(net, bins_dividing(40), "linear", seed=seed, regimes=False)
    x = X.identity_rows(128, 8, seed + 1)
    g = np.random.RandomState(seed + 2).randint(-4, 5, (128, 40)) / 2.0
    forward = X.exact_forward(net, x)
    return net, x, g, forward, X.exact_backward(net, forward, g)


def torch_chain(net, x, g, dtype, with_final=True):
    """stock torch on the CPU in `dtype`: every array K33 writes (tests/test_gpu_wide_train.py `chain`, through autograd)
    and every parameter's gradient, as float64 arrays in exact_forward's / exact_backward's layout"""
    import copy

    import torch
    from torch.nn import functional as F
    net = copy.deepcopy(net).to(dtype)
    xt = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    keep = []

    def held(t):
        t.retain_grad()
        keep.append(t)
        return t
    h = held(F.linear(xt, net.initial_layer.weight, net.initial_layer.bias))
    saved, pre = [], []
    for b in net.blocks:
        s0 = F.relu(h)
        a = held(F.linear(s0, b.linear_layers[0].weight, b.linear_layers[0].bias))
        s1 = F.relu(a)
        pre += [h, a]
        h = held(h + F.linear(s1, b.linear_layers[1].weight, b.linear_layers[1].bias))
        saved += [s0, s1]
    params = F.linear(h, net.final_layer.weight, net.final_layer.bias) if with_final else None
    (params if with_final else h).backward(torch.from_numpy(np.asarray(g)).to(dtype))
    n = lambda t: t.detach().double().numpy()
    # grads[2 k] = d loss / d h_k (the stream in front of block k), grads[2 k + 1] = d loss / d a_k
    out = {"hidden": n(h), "saved": [n(s) for s in saved], "params": n(params) if with_final else None,
           "g_hidden": n(h.grad), "grads": [n(p.grad) for p in pre], "g_x": n(xt.grad),
           "param_grads": {k: n(p.grad) for k, p in net.named_parameters() if p.grad is not None}}
    return out


def assert_equal_as_numbers(got, want, what):
    """np.array_equal over the arrays / lists / dicts of two results (a -0 for a +0 is not a finding)"""
    if want is None:
        assert got is None, what
    elif isinstance(want, dict):
        for k in want:
            assert_equal_as_numbers(got[k], want[k], "%s[%s]" % (what, k))
    elif isinstance(want, list):
        assert len(got) == len(want), what
        for j, (a, b) in enumerate(zip(got, want)):
            assert_equal_as_numbers(a, b, "%s[%d]" % (what, j))
    else:
        a, b = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert a.shape == b.shape, (what, a.shape, b.shape)
        bad = a != b
        assert not bad.any(), "%s: %d of %d elements differ, first at %s: %r for %r" % (
            what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(a[bad][0]), float(b[bad][0]))
