"""Cases, inputs, float64 truth, per-element allowance and rule for the conditioner's training kernels: K14
(nflows_amd/csrc/resnet_train.hip: the forward pass, the chain of input gradients and the packer) and K10
(nflows_amd/csrc/linear_wgrad.hip: weight and bias gradients).  tests/test_train_kernels_host.py holds the table to its
two yardsticks and to an emulation of the split-bf16 scheme on the CPU, tests/test_gpu_train_kernels.py runs the kernels
through it; both import everything from here.  Plain numpy and torch on the CPU; of `nflows_amd.ops` only the two
tensor-operation references `split_bf16x3` and `pack_resnet_hidden_train_reference`.

  * Truth (float64).  K14 forward: h = W_in x + b_in; per block t = relu(h), a = W_0 t + b_0, u = relu(a),
    h += W_1 u + b_1; params = W_f h + b_f.  K14 backward with the ReLU masks PINNED (on the GPU the ones the forward
    kernel produced, `saved[j] > 0`; on the CPU the float64 chain's own): g_h = g_params W_f; per block from the last to
    the first g_a = (g_h W_1) m_a, g_h += (g_a W_0) m_h; g_x = g_h W_in.  K10: gw = gy^T x, gb = column sums of gy.
    Arrays, as the kernels write them: hidden, params, saved{j} (saved[2k] = t_k, saved[2k+1] = u_k), grad_hidden,
    grads{j} (grads[2k+1] = g_a of block k, grads[2k] = g_h in front of block k), grad_inputs; gw, gb.
  * Allowance per element: the running forward-error bound with u = 2^-24.  y = W v + b with A(v) on its input:
    A(y) = |W| A(v) + u (|W||v| + |b|).  ReLU passes the allowance on (1-Lipschitz), a pinned mask multiplies it.  Skip:
    A(h') = A(h) + |W_1| A(u) + u (|h| + |W_1||u| + |b_1|); its backward twin g_h' = g_h + v m_h carries
    A(g_h) + A(v) m_h + u |g_h| m_h (where the mask is 0 nothing is added and nothing is rounded).  K10:
    A(gw) = u |gy|^T |x|, A(gb) = u x column sums of |gy| (the inputs are the kernel's own arrays).
  * Rule: ratio = |got - truth| / A per element; A == 0 (a zero column, a masked-out unit, the padded units of a narrow
    net, B = 0) means EXACTLY zero.  Per case and array the mean, the 99.9 % quantile and the maximum of the ratio,
    each under its cap.  No element is left out, there is no additive term.
  * Caps: 2 x max(Y_ref, Y_seq) per case, array and statistic (2: the project's parity factor), rounded up to two digits
    and stored below (`CAPS`; `python tests/train_kernel_cases.py` prints the literal).  Y_ref: the eager fp32 path
    (torch.nn.functional.linear, gy.t() @ x, on the CPU).  Y_seq: the same operations as a sequential fp32 chain --
    accumulator from the bias (zero for K10), inputs in their natural order, one rounding per multiply and per add."""
import collections
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
QUANTILE = 0.999
STATS = ("mean", "q99.9", "max")
PARITY = 2.0

# CHANGED.  What the table found on its first GPU run, and what became of it ("K14 / K10: how they
# are tested").
#   (1) A defect, fixed in the kernel: K14's forward kernel summed a block's second Linear INTO the residual stream
#       (`hs += b_1`, then gemm_from_tiles(hs, u, ...)), so each of that GEMM's 48 MFMAs rounded the accumulator at the size
#       of h: `hidden`, and saved{2k} of every later block, at 1.0 - 2.7 x their caps in all 24 cases with a block (di4_hidden:
#       mean 0.0514 / q99.9 0.432 / max 0.703 against 0.032 / 0.2 / 0.26).  The GEMM now has an accumulator of its own and
#       joins h with one addition.  No case changed for it; tests/test_train_kernels_host.py pins it on the CPU.
#   (2) Units that see a handful of inputs, an honest property of the scheme: every product is six MFMAs that each round
#       the accumulator, which starts at the bias, where the yardsticks round once per product.  A MADE's units of low
#       degree are such elements: at 13 of 16 seeds tried (pattern seed + 100 k) the EMULATED scheme misses a maximum of
#       params, saved1 or saved3 by 1.03 - 1.51 x (mean and quantile sit at 0.5 x).  Measured at the pattern seed 14036 of
#       made63_h128: saved1 q99.9 2.19 / max 4.19 against caps of 2.1 / 3.5 on the GPU, 2.12 / 4.19 in the emulation.  The
#       MADE cases are about masks and odd feature counts: they take the first seed at which the emulation passes.
#   (3) One-term elements on the matrix cores.  With a one-column output gradient every element of grad_hidden is ONE
#       product; the kernel's came out at up to 2.20 u (grads2, which passes them on: 2.06) against a cap of 2.0, where the
#       emulation -- an MFMA's 16 products summed exactly, one rounding -- has 1.28: the rounding inside the instruction,
#       not a wrong column.  The case is about the routing of a column (the swizzled images, the clamped fetch), so its
#       surviving column now holds signed powers of two, +-2^-3 .. 2^3: a product with one is exact in every piece,
#       grad_hidden has to be the float64 truth BIT FOR BIT (its caps are 0), and a wrong column or piece still shows.
CHANGED = {"made21_h64": dict(seed=14735), "made63_h128": dict(seed=14236), "g_onecol": dict(values="powers of two")}

K14Case = collections.namedtuple("K14Case", "name B di nb H out kind made seed")
K10Case = collections.namedtuple("K10Case", "name B I O count kind need_bias seed")


# ------------------------------------------------------------------------------------------------------------ the table
def _k14_table():
    rows = []

    def add(name, B=256, di=32, nb=1, H=128, out=40, kind="plain", made=0, seed=None):
        rows.append(K14Case(name, B, di, nb, H, out, kind, made, 14000 + len(rows) if seed is None else seed))

    # identity features: a quarter k-step, partial ones, a full one, two -> four initial k-steps (32 | 36), `k0 < di`
    for i, di in enumerate((4, 8, 12, 16, 20, 32, 36, 48, 64)):
        add("di%d_%s" % (di, "out40" if i % 2 else "hidden"), B=128, di=di, out=40 if i % 2 else 0)
    for nb in (0, 2, 3):
        add("nb%d_hidden" % nb, nb=nb, out=0)
        add("nb%d_out40" % nb, nb=nb)
    # hidden widths through the packer (padded units exactly zero); 128 is everywhere else
    for H, out in ((124, 0), (64, 24), (52, 0), (4, 0), (4, 24)):
        add("h%d_%s" % (H, "out%d" % out if out else "hidden"), B=128, di=16, nb=2, H=H, out=out)
    # the final Linear: the staged store's column tail; backward, a last k-step of 4 or 8 valid columns
    for out in (4, 24, 32, 368, 736):
        add("out%d" % out, out=out)
    for kind in ("x_rows", "g_rows", "g_cols", "bias_neg", "bias_pos", "zero_unit", "g_onecol"):
        add(kind + "_out40", nb=2, kind=kind)
    for kind in ("g_rows", "bias_neg", "zero_unit"):
        add(kind + "_hidden", nb=2, out=0, kind=kind)
    # K25: a MADE's masks through pack_made_train, odd feature counts (zero pad columns / rows only in the streams)
    add("made21_h64", di=24, nb=2, H=64, out=44, made=21, seed=CHANGED["made21_h64"]["seed"])
    add("made63_h128", di=64, nb=1, H=128, out=128, made=63, seed=CHANGED["made63_h128"]["seed"])
    assert len(set(r.name for r in rows)) == len(rows)
    return rows


def _k10_table():
    rows = []

    def add(name, B=256, I=64, O=96, count=1, kind="relu_x", need_bias=True):
        rows.append(K10Case(name, B, I, O, count, kind, need_bias, 10000 + len(rows)))

    # I <= 32: the fp32-MFMA kernel (128 x 32 result blocks); above: split bf16.  36, 200: clamped columns; 200: two blocks
    for I, O in ((4, 40), (32, 96), (36, 128), (64, 40), (128, 128), (200, 96)):
        add("i%d_o%d" % (I, O), I=I, O=O)
    for I, O in ((64, 4), (36, 96), (32, 128), (64, 260), (128, 736), (32, 260)):
        add("o%d_i%d" % (O, I), I=I, O=O)
    for B in (0, 1, 15, 16, 31, 32, 33, 48, 100, 512, 1000, 1024):
        add("b%d_i36" % B, B=B, I=36, O=40)
    for B in (1, 33, 100, 1000):
        add("b%d_i32" % B, B=B, I=32, O=40)
    for count in (1, 2, 4, 8):      # (four problems at 128 x 128: the 16-row stages; one: 32-row stages)
        add("batched%d_128x128" % count, I=128, O=128, count=count)
    add("batched4_128x128_nobias", I=128, O=128, count=4, need_bias=False)
    add("batched2_i32", B=100, I=32, O=96, count=2)
    add("batched8_i36", B=100, I=36, O=40, count=8)
    for kind in ("nonneg", "rows", "cols", "zero_cols"):
        # (nonneg at 64 rows: without cancellation Y_seq's own error grows with the batch; at 256 rows a dropped product is 1.2 x the cap)
        add(kind + "_i64", B=64 if kind == "nonneg" else 256, kind=kind)
    for kind in ("nonneg", "rows", "zero_cols"):
        add(kind + "_i32", I=32, kind=kind)
    assert len(set(r.name for r in rows)) == len(rows)
    return rows


K14_CASES = _k14_table()
K10_CASES = _k10_table()
K14_BY_NAME = dict((c.name, c) for c in K14_CASES)
K10_BY_NAME = dict((c.name, c) for c in K10_CASES)


# ------------------------------------------------------------------------------------------------------------ K14 inputs
def _uniform(gen, shape, bound):
    return (torch.rand(shape, generator=gen) * 2.0 - 1.0) * bound


def made_masks(D, H, nb, multiplier=2):
    """0/1 masks of a MADE with residual blocks in the usual degree scheme: input degrees 1 .. D, hidden degrees cycling
    over 1 .. D - 1, hidden -> hidden `>=`, outputs (multiplier per feature) strictly `>`.  [W_in, (W_0, W_1) per block, W_f]"""
    deg_in = torch.arange(1, D + 1)
    deg_h = torch.arange(H) % max(1, D - 1) + min(1, D - 1)
    deg_out = torch.arange(1, D + 1).repeat_interleave(multiplier)
    m_in = (deg_h[:, None] >= deg_in[None, :]).float()
    m_hh = (deg_h[:, None] >= deg_h[None, :]).float()
    m_f = (deg_out[:, None] > deg_h[None, :]).float()
    return [m_in] + [m_hh.clone() for _ in range(2 * nb)] + [m_f]


def k14_net(case):
    """The case's parameters as the packers take them (float32, the net's own sizes): dict w_in [H, D], b_in, blocks
    [(W_0, b_0, W_1, b_1)], final (W_f [rows, H], b_f) or None, masks or None.  torch.nn.Linear's initialisation; the
    blocks' second Linears are U(-1e-3, 1e-3) x 60 (the sharpening of test_gpu_grads._k14_net: every path carries signal)."""
    gen = torch.Generator().manual_seed(case.seed)
    D = case.made or case.di
    H = case.H
    net = {"w_in": _uniform(gen, (H, D), 1.0 / math.sqrt(D)), "b_in": _uniform(gen, (H,), 1.0 / math.sqrt(D)), "blocks": []}
    for _ in range(case.nb):
        net["blocks"].append([_uniform(gen, (H, H), 1.0 / math.sqrt(H)), _uniform(gen, (H,), 1.0 / math.sqrt(H)),
                              _uniform(gen, (H, H), 0.06), _uniform(gen, (H,), 0.06)])
    rows = 2 * case.made if case.made else case.out
    net["final"] = (_uniform(gen, (rows, H), 1.0 / math.sqrt(H)), _uniform(gen, (rows,), 1.0 / math.sqrt(H))) if rows else None
    net["masks"] = made_masks(D, H, case.nb) if case.made else None
    if case.kind in ("bias_neg", "bias_pos"):       # all masks of block 0 zero (h passes through) / all one
        net["blocks"][0][1] = torch.full((H,), -50.0 if case.kind == "bias_neg" else 50.0)
    if case.kind == "zero_unit":                    # a == 0 exactly: mask bit 0, as threshold_backward's `output > 0`
        net["blocks"][0][0][ZERO_UNIT, :] = 0.0
        net["blocks"][0][1][ZERO_UNIT] = 0.0
    net["blocks"] = [tuple(b) for b in net["blocks"]]
    return net


ZERO_UNIT = 7


def k14_data(case, rows=None, seed_offset=0):
    """(x [B, D], g [B, rows of the final Linear | 128]) float32: the inputs and the gradient the backward kernel starts
    from -- d loss / d params with a final Linear, d loss / d hidden (zero past the net's width) without."""
    B = case.B if rows is None else rows
    gen = torch.Generator().manual_seed(case.seed + 500 + seed_offset)
    D = case.made or case.di
    x = torch.randn(B, D, generator=gen)
    width = (2 * case.made if case.made else case.out) or 128
    g = torch.randn(B, width, generator=gen)
    if case.kind == "x_rows":
        x = x * torch.exp(3.0 * torch.randn(B, 1, generator=gen))
    if case.kind == "g_rows":
        g = g * torch.exp(4.0 * torch.randn(B, 1, generator=gen))
    if case.kind == "g_cols":
        g = g * torch.exp(4.0 * torch.randn(1, width, generator=gen))
    if case.kind == "g_onecol":
        keep = torch.zeros(width)
        keep[width // 2] = 1.0
        g = keep * torch.sign(g) * 2.0 ** torch.randint(-3, 4, (B, 1), generator=gen)      # (CHANGED (3))
    if not case.out and not case.made:
        g[:, case.H:] = 0.0
    return x.contiguous(), g.contiguous()


def _pad(a, shape):
    out = np.zeros(shape, dtype=np.float32)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def effective(net, di, out):
    """What the kernels compute with: `mask * weight` (exact in fp32), zero-padded to 128 units, `di` identity columns and
    `out` output rows.  numpy float32: W_in [128, di], b_in, blocks, W_f [out, 128] or None, b_f."""
    n = lambda t: t.detach().numpy().astype(np.float32)      # noqa: E731
    masks = net["masks"] or [None] * (2 + 2 * len(net["blocks"]))
    w = lambda t, m: n(t) if m is None else n(t) * n(m)      # noqa: E731
    e = {"W_in": _pad(w(net["w_in"], masks[0]), (128, di)), "b_in": _pad(n(net["b_in"]), (128,)), "blocks": [], "W_f": None, "b_f": None}
    for k, (w0, b0, w1, b1) in enumerate(net["blocks"]):
        e["blocks"].append((_pad(w(w0, masks[1 + 2 * k]), (128, 128)), _pad(n(b0), (128,)),
                            _pad(w(w1, masks[2 + 2 * k]), (128, 128)), _pad(n(b1), (128,))))
    if net["final"] is not None:
        e["W_f"] = _pad(w(net["final"][0], masks[-1]), (out, 128))
        e["b_f"] = _pad(n(net["final"][1]), (out,))
    return e


def padded(a, cols):
    """[B, cols] float32 with zero columns behind `a`'s own"""
    a = np.asarray(a, dtype=np.float32)
    return a if a.shape[1] == cols else _pad(a, (a.shape[0], cols))


def forward_arrays(nb, final):
    return ["hidden"] + (["params"] if final else []) + ["saved%d" % j for j in range(2 * nb)]


def backward_arrays(nb, final):
    return (["grad_hidden"] if final else []) + ["grads%d" % j for j in range(2 * nb)] + ["grad_inputs"]


# ------------------------------------------------------------------------------------------------- K14 truth and allowance
def _affine64(v, Av, W, b):
    aW = np.abs(W)
    y = v @ W.T
    A = Av @ aW.T + U * (np.abs(v) @ aW.T)
    if b is not None:
        y = y + b
        A = A + U * np.abs(b)
    return y, A


def k14_forward_truth(e, x):
    """{array: (truth, allowance)} of the forward arrays, and the float64 chain's own masks [2 nb] of [B, 128] bool."""
    d = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    x = d(x)
    out, masks = {}, []
    h, Ah = _affine64(x, np.zeros_like(x), d(e["W_in"]), d(e["b_in"]))
    for k, (w0, b0, w1, b1) in enumerate(e["blocks"]):
        t = np.maximum(h, 0.0)
        a, Aa = _affine64(t, Ah, d(w0), d(b0))
        u = np.maximum(a, 0.0)
        out["saved%d" % (2 * k)], out["saved%d" % (2 * k + 1)] = (t, Ah), (u, Aa)
        masks += [t > 0.0, u > 0.0]
        y, Ay = _affine64(u, Aa, d(w1), d(b1))
        Ah = Ah + Ay + U * np.abs(h)
        h = h + y
    out["hidden"] = (h, Ah)
    if e["W_f"] is not None:
        out["params"] = _affine64(h, Ah, d(e["W_f"]), d(e["b_f"]))
    return out, masks


def k14_backward_truth(e, g, masks):
    """{array: (truth, allowance)} of the backward arrays for the pinned `masks` ([2 nb] of [B, 128], bool or 0/1)."""
    d = lambda a: np.asarray(a, dtype=np.float64)      # noqa: E731
    g = d(g)
    out = {}
    if e["W_f"] is not None:
        gh, Agh = _affine64(g, np.zeros_like(g), d(e["W_f"]).T, None)
        out["grad_hidden"] = (gh, Agh)
    else:
        gh, Agh = g, np.zeros_like(g)
    for k in reversed(range(len(e["blocks"]))):
        w0, _, w1, _ = e["blocks"][k]
        mh, ma = d(masks[2 * k]), d(masks[2 * k + 1])
        ga, Aga = _affine64(gh, Agh, d(w1).T, None)
        ga, Aga = ga * ma, Aga * ma
        v, Av = _affine64(ga, Aga, d(w0).T, None)
        Agh = Agh + Av * mh + U * np.abs(gh) * mh
        gh = gh + v * mh
        out["grads%d" % (2 * k + 1)], out["grads%d" % (2 * k)] = (ga, Aga), (gh, Agh)
    out["grad_inputs"] = _affine64(gh, Agh, d(e["W_in"]).T, None)
    return out


# ------------------------------------------------------------------------------------------------------------- the rule
def ratio_stats(got, truth, allow, what=""):
    """(mean, 99.9 % quantile, max) of |got - truth| / allowance over every element with an allowance; the elements
    without one must be exactly the truth -- zero -- (asserted here: it is part of the rule, not a statistic)."""
    got = np.asarray(got, dtype=np.float64).reshape(truth.shape)
    zero = allow == 0.0
    if zero.any():
        # (the truth there is 0, or -- a gradient that a closed mask lets through unchanged -- an input value itself)
        bad = int(np.count_nonzero(got[zero] != truth[zero]))
        assert bad == 0, "%s: %d of %d elements without an allowance are not exactly their truth (0, or a value passed through)" % (
            what, bad, int(zero.sum()))
    if zero.all():
        return (0.0, 0.0, 0.0)
    r = np.abs(got[~zero] - truth[~zero]) / allow[~zero]
    return (float(r.mean()), float(np.quantile(r, QUANTILE)), float(r.max()))


def stats_of(got, truth, what=""):
    """{array: (mean, q, max)} for `got` {array: values} against `truth` {array: (truth, allowance)}; every array of the truth."""
    missing = set(truth) - set(got)
    assert not missing, "%s: arrays not judged: %s" % (what, sorted(missing))
    return dict((k, ratio_stats(got[k], t, A, "%s %s" % (what, k))) for k, (t, A) in truth.items())


def round_up(v, digits=2):
    if v <= 0.0:
        return 0.0
    step = 10.0 ** (math.floor(math.log10(v)) - digits + 1)
    return float("%.*g" % (digits + 2, math.ceil(v / step - 1e-9) * step))


def caps_from(*yardsticks):
    """{array: caps}: PARITY x the larger yardstick per statistic, rounded up to two digits."""
    return dict((k, tuple(round_up(PARITY * max(y[k][i] for y in yardsticks)) for i in range(3))) for k in yardsticks[0])


def misses(stats, caps):
    """[(array, statistic, value, cap)] of every statistic above its cap (a NaN is above every cap)."""
    return [(k, STATS[i], s[i], caps[k][i]) for k, s in sorted(stats.items()) for i in range(3) if not s[i] <= caps[k][i]]


def report(name, stats, caps=None):
    for k, s in sorted(stats.items()):
        line = "%-30s %-12s mean %9.3g  q99.9 %9.3g  max %9.3g" % (name, k, s[0], s[1], s[2])
        if caps is not None:
            line += "   caps %8.2g %8.2g %8.2g" % caps[k]
        print(line)


def assert_within_caps(name, stats, caps, verbose=False):
    if verbose:
        report(name, stats, caps)
    bad = misses(stats, caps)
    assert not bad, "%s: %s" % (name, "; ".join("%s %s %.3g > cap %.2g" % b for b in bad))


# ------------------------------------------------------------------------------------------------- arithmetics of a Linear
def linear_ref(v, W, b):
    """Y_ref: the eager fp32 path (torch.nn.functional.linear on the CPU)."""
    y = torch.nn.functional.linear(torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(W)),
                                   None if b is None else torch.from_numpy(np.ascontiguousarray(b)))
    return y.numpy()


def linear_seq(v, W, b):
    """Y_seq: accumulator from the bias, inputs in their natural order, one fp32 rounding per multiply and per add."""
    v, W = np.asarray(v, dtype=np.float32), np.asarray(W, dtype=np.float32)
    acc = np.zeros((v.shape[0], W.shape[0]), dtype=np.float32)
    if b is not None:
        acc = acc + np.asarray(b, dtype=np.float32)
    for k in range(v.shape[1]):
        acc = acc + v[:, k:k + 1] * W[None, :, k]
    return acc


def k14_chain(e, x, g, masks, linear, skip_into_accumulator=False):
    """Every array of both passes in fp32 with `linear(v, W, b)` as the arithmetic of a Linear (b: a vector, None, or --
    skip_into_accumulator, the kernels' form of the skip connection -- the [B, 128] accumulator h + b_1 the products are
    summed onto).  The backward pass runs through the pinned `masks`."""
    f = np.float32
    out = {}
    h = linear(np.asarray(x, dtype=f), e["W_in"], e["b_in"])
    for k, (w0, b0, w1, b1) in enumerate(e["blocks"]):
        t = np.maximum(h, f(0.0))
        u = np.maximum(linear(t, w0, b0), f(0.0))
        out["saved%d" % (2 * k)], out["saved%d" % (2 * k + 1)] = t, u
        h = linear(u, w1, h + b1) if skip_into_accumulator else h + linear(u, w1, b1)
    out["hidden"] = h
    gh = np.asarray(g, dtype=f)
    if e["W_f"] is not None:
        out["params"] = linear(h, e["W_f"], e["b_f"])
        gh = out["grad_hidden"] = linear(gh, np.ascontiguousarray(e["W_f"].T), None)
    for k in reversed(range(len(e["blocks"]))):
        w0, _, w1, _ = e["blocks"][k]
        ga = linear(gh, np.ascontiguousarray(w1.T), None) * masks[2 * k + 1].astype(f)
        gh = gh + linear(ga, np.ascontiguousarray(w0.T), None) * masks[2 * k].astype(f)
        out["grads%d" % (2 * k + 1)], out["grads%d" % (2 * k)] = ga, gh
    out["grad_inputs"] = linear(gh, np.ascontiguousarray(e["W_in"].T), None)
    return out


@functools.lru_cache(maxsize=None)
def k14_prepared(name):
    """Net, inputs, truth and the float64 chain's masks of a K14 case, once per process (shared, never modified)."""
    case = K14_BY_NAME[name]
    net = k14_net(case)
    x, g = k14_data(case)
    e = effective(net, case.di, case.out)
    xp, gp = padded(x.numpy(), case.di), padded(g.numpy(), case.out or 128)
    fwd, masks = k14_forward_truth(e, xp)
    truth = dict(fwd)
    truth.update(k14_backward_truth(e, gp, masks))
    assert sorted(truth) == sorted(forward_arrays(case.nb, bool(case.out)) + backward_arrays(case.nb, bool(case.out)))
    return dict(case=case, net=net, x=x, g=g, e=e, xp=xp, gp=gp, truth=truth, masks=masks)


def k14_yardsticks(p):
    """(stats of Y_ref, stats of Y_seq) of a prepared K14 case."""
    return tuple(stats_of(k14_chain(p["e"], p["xp"], p["gp"], p["masks"], lin), p["truth"], p["case"].name)
                 for lin in (linear_ref, linear_seq))


# ------------------------------------------------------------------------------------------------------------------ K10
def k10_data(case):
    """[(x [B, I], gy [B, O])] per problem, float32.  Problem q's x is scaled by 2^q: a swapped problem index shows."""
    gen = torch.Generator().manual_seed(case.seed)
    B, I, O = case.B, case.I, case.O
    out = []
    for q in range(case.count):
        x = torch.relu(torch.randn(B, I, generator=gen)) * 2.0 ** q
        gy = torch.randn(B, O, generator=gen)
        if case.kind == "nonneg":           # no cancellation: the ratio is the relative error (in units of u)
            gy = gy.abs()
        if case.kind == "rows":
            x = x * torch.exp(3.0 * torch.randn(B, 1, generator=gen))
        if case.kind == "cols":
            gy = gy * torch.exp(4.0 * torch.randn(1, O, generator=gen))
        if case.kind == "zero_cols":        # exactly zero rows / columns of gw and an exactly zero gb element
            gy[:, O // 3] = 0.0
            x[:, I // 2] = 0.0
        out.append((x.contiguous(), gy.contiguous()))
    return out


def k10_truth(problems, need_bias=True):
    """{"gw": (truth [count, O, I], allowance), "gb": ...} in float64 for [(x, gy)] (torch or numpy)."""
    d = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)      # noqa: E731
    gw = [(d(gy).T @ d(x), U * (np.abs(d(gy)).T @ np.abs(d(x)))) for x, gy in problems]
    out = {"gw": (np.stack([t for t, _ in gw]), np.stack([a for _, a in gw]))}
    if need_bias:
        out["gb"] = (np.stack([d(gy).sum(axis=0) for _, gy in problems]), np.stack([U * np.abs(d(gy)).sum(axis=0) for _, gy in problems]))
    return out


def _f32(a):
    return np.ascontiguousarray(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float32))


def wgrad_ref(x, gy):
    x, gy = torch.from_numpy(_f32(x)), torch.from_numpy(_f32(gy))
    return (gy.t() @ x).numpy(), gy.sum(dim=0).numpy()


def wgrad_seq(x, gy):
    x, gy = _f32(x), _f32(gy)
    gw, gb = np.zeros((gy.shape[1], x.shape[1]), dtype=np.float32), np.zeros(gy.shape[1], dtype=np.float32)
    for r in range(x.shape[0]):
        gw = gw + gy[r][:, None] * x[r][None, :]
        gb = gb + gy[r]
    return gw, gb


def k10_apply(problems, wgrad, need_bias=True):
    """{"gw": [count, O, I], "gb": [count, O]} of `wgrad(x, gy) -> (gw, gb)` over the problems."""
    got = [wgrad(x, gy) for x, gy in problems]
    out = {"gw": np.stack([g[0] for g in got])}
    if need_bias:
        out["gb"] = np.stack([g[1] for g in got])
    return out


def k10_yardsticks(problems, truth, need_bias=True, what=""):
    return tuple(stats_of(k10_apply(problems, w, need_bias), truth, what) for w in (wgrad_ref, wgrad_seq))


def k10_runtime_caps(problems, need_bias=True, what=""):
    """(truth, caps) for arrays that exist only at run time (slice lengths read from the device, arrays the kernels left):
    the same truth, yardsticks and factor as the stored caps."""
    truth = k10_truth(problems, need_bias)
    return truth, caps_from(*k10_yardsticks(problems, truth, need_bias, what))


@functools.lru_cache(maxsize=None)
def k10_prepared(name):
    case = K10_BY_NAME[name]
    problems = k10_data(case)
    return dict(case=case, problems=problems, truth=k10_truth(problems, case.need_bias))


# ------------------------------------------------------------------------------------------------------------- the caps
def compute_caps():
    caps = {}
    for c in K14_CASES:
        caps[c.name] = caps_from(*k14_yardsticks(k14_prepared(c.name)))
    for c in K10_CASES:
        p = k10_prepared(c.name)
        caps[c.name] = caps_from(*k10_yardsticks(p["problems"], p["truth"], c.need_bias, c.name))
    return caps


def _print_caps():
    caps = compute_caps()
    print("CAPS = {")
    for c in K14_CASES + K10_CASES:
        print("    %r: {%s}," % (c.name, ", ".join("%r: (%g, %g, %g)" % ((k,) + v) for k, v in sorted(caps[c.name].items()))))
    print("}")


# PARITY x max(Y_ref, Y_seq) of (mean, 99.9 % quantile, max) per case and array, rounded up to two digits.
# tests/test_train_kernels_host.py recomputes both yardsticks and holds each to HALF of these.
# CAPS-BEGIN
CAPS = {
    'di4_hidden': {'grad_inputs': (0.095, 0.57, 0.62), 'grads0': (0.13, 0.61, 0.83), 'grads1': (0.64, 5, 11), 'hidden': (0.032, 0.2, 0.26), 'saved0': (0.36, 3.5, 4.7), 'saved1': (0.059, 0.77, 1.1)},
    'di8_out40': {'grad_hidden': (0.66, 4.6, 7), 'grad_inputs': (0.018, 0.11, 0.13), 'grads0': (0.37, 4.1, 6.9), 'grads1': (0.12, 0.77, 0.91), 'hidden': (0.031, 0.2, 0.32), 'params': (0.0091, 0.066, 0.086), 'saved0': (0.36, 4.1, 5.7), 'saved1': (0.061, 0.73, 1.2)},
    'di12_hidden': {'grad_inputs': (0.093, 0.64, 0.72), 'grads0': (0.13, 0.54, 0.69), 'grads1': (0.63, 4.5, 6.1), 'hidden': (0.031, 0.2, 0.31), 'saved0': (0.35, 3.9, 6.2), 'saved1': (0.05, 0.57, 0.88)},
    'di16_out40': {'grad_hidden': (0.67, 4.8, 6.2), 'grad_inputs': (0.019, 0.14, 0.16), 'grads0': (0.37, 4.2, 6.2), 'grads1': (0.12, 0.71, 0.95), 'hidden': (0.03, 0.2, 0.28), 'params': (0.0076, 0.054, 0.11), 'saved0': (0.35, 4.1, 7.5), 'saved1': (0.05, 0.58, 0.87)},
    'di20_hidden': {'grad_inputs': (0.088, 0.72, 0.77), 'grads0': (0.13, 0.58, 0.77), 'grads1': (0.64, 4.4, 7), 'hidden': (0.029, 0.2, 0.32), 'saved0': (0.33, 4, 5.5), 'saved1': (0.044, 0.5, 0.79)},
    'di32_out40': {'grad_hidden': (0.66, 4.5, 7.6), 'grad_inputs': (0.018, 0.12, 0.14), 'grads0': (0.36, 4.2, 7.6), 'grads1': (0.12, 0.83, 1.1), 'hidden': (0.028, 0.19, 0.29), 'params': (0.0059, 0.044, 0.055), 'saved0': (0.33, 4.1, 7.3), 'saved1': (0.042, 0.41, 0.58)},
    'di36_hidden': {'grad_inputs': (0.089, 0.67, 0.98), 'grads0': (0.13, 0.56, 0.91), 'grads1': (0.63, 4.4, 8.7), 'hidden': (0.028, 0.19, 0.27), 'saved0': (0.34, 4.2, 5.6), 'saved1': (0.038, 0.41, 0.58)},
    'di48_out40': {'grad_hidden': (0.67, 4.8, 6.4), 'grad_inputs': (0.019, 0.13, 0.17), 'grads0': (0.36, 4.5, 6.4), 'grads1': (0.12, 0.77, 1.1), 'hidden': (0.028, 0.2, 0.26), 'params': (0.0054, 0.034, 0.05), 'saved0': (0.34, 4.3, 5.8), 'saved1': (0.037, 0.4, 0.65)},
    'di64_hidden': {'grad_inputs': (0.086, 0.66, 0.86), 'grads0': (0.13, 0.52, 0.72), 'grads1': (0.63, 4.3, 9.5), 'hidden': (0.028, 0.19, 0.31), 'saved0': (0.33, 4.1, 6.2), 'saved1': (0.034, 0.33, 0.55)},
    'nb0_hidden': {'grad_inputs': (0.63, 4.7, 5.9), 'hidden': (0.66, 4.6, 7.3)},
    'nb0_out40': {'grad_hidden': (0.66, 4.6, 7), 'grad_inputs': (0.12, 0.71, 0.96), 'hidden': (0.67, 4.5, 6.8), 'params': (0.13, 0.8, 1.4)},
    'nb2_hidden': {'grad_inputs': (0.015, 0.13, 0.23), 'grads0': (0.028, 0.37, 0.59), 'grads1': (0.096, 0.73, 1.3), 'grads2': (0.13, 0.61, 0.97), 'grads3': (0.63, 4.7, 8), 'hidden': (0.0014, 0.0087, 0.012), 'saved0': (0.33, 4, 6.1), 'saved1': (0.041, 0.44, 0.82), 'saved2': (0.014, 0.17, 0.29), 'saved3': (0.0016, 0.018, 0.037)},
    'nb2_out40': {'grad_hidden': (0.66, 4.7, 7.1), 'grad_inputs': (0.0029, 0.02, 0.03), 'grads0': (0.32, 4.2, 7.1), 'grads1': (0.018, 0.12, 0.18), 'grads2': (0.36, 4.2, 7.1), 'grads3': (0.12, 0.77, 1.3), 'hidden': (0.0014, 0.0091, 0.017), 'params': (0.00028, 0.0017, 0.0023), 'saved0': (0.33, 4.1, 7.6), 'saved1': (0.039, 0.41, 0.66), 'saved2': (0.014, 0.18, 0.34), 'saved3': (0.0019, 0.02, 0.039)},
    'nb3_hidden': {'grad_inputs': (0.0024, 0.021, 0.039), 'grads0': (0.0081, 0.34, 0.6), 'grads1': (0.015, 0.13, 0.21), 'grads2': (0.028, 0.38, 0.6), 'grads3': (0.09, 0.69, 1.1), 'grads4': (0.13, 0.57, 0.96), 'grads5': (0.64, 4.6, 7), 'hidden': (6.2e-05, 0.00042, 0.00068), 'saved0': (0.34, 4.2, 6.9), 'saved1': (0.039, 0.45, 0.9), 'saved2': (0.015, 0.19, 0.29), 'saved3': (0.0018, 0.02, 0.029), 'saved4': (0.00066, 0.0083, 0.014), 'saved5': (7.6e-05, 0.00084, 0.0016)},
    'nb3_out40': {'grad_hidden': (0.66, 4.7, 6.9), 'grad_inputs': (0.0005, 0.0035, 0.0057), 'grads0': (0.31, 4.1, 6.4), 'grads1': (0.003, 0.021, 0.03), 'grads2': (0.33, 4.2, 6.4), 'grads3': (0.018, 0.12, 0.21), 'grads4': (0.36, 4.2, 6.4), 'grads5': (0.12, 0.77, 1.4), 'hidden': (6e-05, 0.00041, 0.00065), 'params': (1.2e-05, 7.4e-05, 9.7e-05), 'saved0': (0.34, 4, 5.9), 'saved1': (0.037, 0.4, 0.69), 'saved2': (0.014, 0.17, 0.26), 'saved3': (0.0017, 0.019, 0.034), 'saved4': (0.00065, 0.0078, 0.013), 'saved5': (8.1e-05, 0.00079, 0.0015)},
    'h124_hidden': {'grad_inputs': (0.017, 0.11, 0.18), 'grads0': (0.031, 0.39, 0.54), 'grads1': (0.097, 0.77, 1.2), 'grads2': (0.13, 0.59, 0.86), 'grads3': (0.62, 4.2, 7), 'hidden': (0.0016, 0.011, 0.018), 'saved0': (0.34, 4.4, 8), 'saved1': (0.047, 0.59, 1.1), 'saved2': (0.016, 0.19, 0.29), 'saved3': (0.002, 0.024, 0.034)},
    'h64_out24': {'grad_hidden': (0.68, 4.3, 7.4), 'grad_inputs': (0.018, 0.13, 0.17), 'grads0': (0.37, 4.1, 7.4), 'grads1': (0.051, 0.33, 0.44), 'grads2': (0.41, 4.1, 7.4), 'grads3': (0.16, 0.83, 1.6), 'hidden': (0.0089, 0.06, 0.084), 'params': (0.0026, 0.015, 0.018), 'saved0': (0.33, 3.7, 5.2), 'saved1': (0.054, 0.55, 0.89), 'saved2': (0.035, 0.44, 0.55), 'saved3': (0.0066, 0.068, 0.094)},
    'h52_hidden': {'grad_inputs': (0.089, 0.7, 0.76), 'grads0': (0.098, 0.62, 0.83), 'grads1': (0.21, 1.5, 2), 'grads2': (0.22, 0.96, 1.1), 'grads3': (0.63, 4.1, 5.9), 'hidden': (0.015, 0.095, 0.13), 'saved0': (0.35, 4.1, 5.5), 'saved1': (0.057, 0.64, 0.94), 'saved2': (0.048, 0.57, 0.7), 'saved3': (0.0089, 0.11, 0.14)},
    'h4_hidden': {'grad_inputs': (0.46, 2.8, 3.1), 'grads0': (0.45, 1.6, 1.6), 'grads1': (0.57, 2.5, 2.6), 'grads2': (0.63, 1.8, 1.8), 'grads3': (0.83, 3.3, 3.3), 'hidden': (0.38, 2.3, 2.6), 'saved0': (0.46, 4.8, 6.2), 'saved1': (0.24, 2, 2.5), 'saved2': (0.3, 2.9, 3.6), 'saved3': (0.18, 0.99, 1.2)},
    'h4_out24': {'grad_hidden': (0.68, 4, 4.7), 'grad_inputs': (0.33, 1.7, 1.8), 'grads0': (0.58, 3.4, 3.6), 'grads1': (0.35, 1.4, 1.4), 'grads2': (0.63, 3.4, 3.6), 'grads3': (0.37, 1.8, 1.8), 'hidden': (0.34, 1.4, 1.4), 'params': (0.24, 1.2, 1.4), 'saved0': (0.29, 2.6, 2.9), 'saved1': (0.16, 1.4, 1.6), 'saved2': (0.21, 1.7, 1.8), 'saved3': (0.049, 0.76, 0.82)},
    'out4': {'grad_hidden': (0.81, 3.9, 5), 'grad_inputs': (0.035, 0.25, 0.39), 'grads0': (0.44, 3.6, 5), 'grads1': (0.23, 1.9, 2.8), 'hidden': (0.029, 0.2, 0.42), 'params': (0.0063, 0.035, 0.045), 'saved0': (0.33, 4.2, 7.7), 'saved1': (0.042, 0.44, 0.7)},
    'out24': {'grad_hidden': (0.67, 4.6, 6.4), 'grad_inputs': (0.022, 0.14, 0.2), 'grads0': (0.37, 4.3, 6.4), 'grads1': (0.14, 0.92, 1.4), 'hidden': (0.029, 0.2, 0.41), 'params': (0.0061, 0.04, 0.052), 'saved0': (0.33, 4.3, 6.2), 'saved1': (0.04, 0.43, 0.81)},
    'out32': {'grad_hidden': (0.66, 4.4, 7.5), 'grad_inputs': (0.021, 0.14, 0.19), 'grads0': (0.36, 4.1, 7.5), 'grads1': (0.13, 0.81, 1.5), 'hidden': (0.028, 0.2, 0.28), 'params': (0.006, 0.039, 0.057), 'saved0': (0.33, 4.2, 6.2), 'saved1': (0.038, 0.44, 0.75)},
    'out368': {'grad_hidden': (0.62, 4.8, 7.9), 'grad_inputs': (0.012, 0.057, 0.093), 'grads0': (0.33, 4.2, 6.5), 'grads1': (0.077, 0.37, 0.53), 'hidden': (0.028, 0.19, 0.32), 'params': (0.006, 0.038, 0.077), 'saved0': (0.34, 4.1, 6.5), 'saved1': (0.04, 0.43, 0.67)},
    'out736': {'grad_hidden': (0.62, 4.6, 7), 'grad_inputs': (0.012, 0.056, 0.13), 'grads0': (0.34, 4.3, 7), 'grads1': (0.074, 0.35, 0.42), 'hidden': (0.029, 0.2, 0.33), 'params': (0.0061, 0.039, 0.071), 'saved0': (0.33, 4.1, 6.1), 'saved1': (0.041, 0.44, 0.8)},
    'x_rows_out40': {'grad_hidden': (0.67, 4.8, 7.6), 'grad_inputs': (0.0028, 0.019, 0.024), 'grads0': (0.31, 4.3, 7.6), 'grads1': (0.017, 0.11, 0.18), 'grads2': (0.35, 4.3, 7.6), 'grads3': (0.12, 0.73, 1.2), 'hidden': (0.0021, 0.024, 0.038), 'params': (0.00043, 0.0045, 0.0063), 'saved0': (0.53, 9.9, 17), 'saved1': (0.065, 1.4, 2.8), 'saved2': (0.023, 0.4, 0.72), 'saved3': (0.0034, 0.069, 0.13)},
    'g_rows_out40': {'grad_hidden': (0.66, 4.5, 8.6), 'grad_inputs': (0.0033, 0.022, 0.032), 'grads0': (0.33, 4.1, 8.6), 'grads1': (0.019, 0.13, 0.2), 'grads2': (0.36, 4.1, 8.6), 'grads3': (0.12, 0.79, 1.3), 'hidden': (0.0013, 0.0087, 0.015), 'params': (0.00027, 0.0017, 0.0024), 'saved0': (0.33, 4, 7), 'saved1': (0.035, 0.4, 0.68), 'saved2': (0.014, 0.17, 0.31), 'saved3': (0.0017, 0.018, 0.029)},
    'g_cols_out40': {'grad_hidden': (2.4, 14, 18), 'grad_inputs': (0.0077, 0.049, 0.06), 'grads0': (1.2, 12, 18), 'grads1': (0.045, 0.29, 0.44), 'grads2': (1.3, 12, 18), 'grads3': (0.31, 1.9, 3.5), 'hidden': (0.0014, 0.0088, 0.014), 'params': (0.00028, 0.0017, 0.0024), 'saved0': (0.34, 4.1, 7.8), 'saved1': (0.041, 0.45, 0.97), 'saved2': (0.015, 0.17, 0.29), 'saved3': (0.002, 0.02, 0.035)},
    'bias_neg_out40': {'grad_hidden': (0.66, 4.5, 6.9), 'grad_inputs': (0.019, 0.13, 0.22), 'grads0': (0.36, 4, 6.7), 'grads1': (0, 0, 0), 'grads2': (0.36, 4, 6.7), 'grads3': (0.12, 0.75, 1.1), 'hidden': (0.0003, 0.0021, 0.0033), 'params': (6.4e-05, 0.00041, 0.00061), 'saved0': (0.32, 4, 6.8), 'saved1': (0, 0, 0), 'saved2': (0.0031, 0.04, 0.062), 'saved3': (0.00038, 0.0046, 0.011)},
    'bias_pos_out40': {'grad_hidden': (0.66, 4.6, 7.5), 'grad_inputs': (0.0016, 0.011, 0.014), 'grads0': (0.19, 3.7, 7.5), 'grads1': (0.018, 0.12, 0.27), 'grads2': (0.35, 4.3, 7.5), 'grads3': (0.12, 0.75, 1.4), 'hidden': (0.014, 0.072, 0.11), 'params': (0.0018, 0.0086, 0.012), 'saved0': (0.33, 4.1, 7.2), 'saved1': (3.7, 16, 18), 'saved2': (0.16, 1.6, 2.4), 'saved3': (0.014, 0.12, 0.18)},
    'zero_unit_out40': {'grad_hidden': (0.66, 4.7, 7), 'grad_inputs': (0.0029, 0.019, 0.034), 'grads0': (0.32, 4.1, 7), 'grads1': (0.019, 0.12, 0.18), 'grads2': (0.36, 4.1, 7), 'grads3': (0.13, 0.81, 1.4), 'hidden': (0.0014, 0.0091, 0.014), 'params': (0.00028, 0.0018, 0.0026), 'saved0': (0.34, 4.1, 8.5), 'saved1': (0.039, 0.41, 0.73), 'saved2': (0.015, 0.18, 0.32), 'saved3': (0.0018, 0.019, 0.034)},
    'g_onecol_out40': {'grad_hidden': (0, 0, 0), 'grad_inputs': (0.0072, 0.051, 0.065), 'grads0': (0.0076, 0.16, 0.35), 'grads1': (0.051, 0.41, 0.65), 'grads2': (0.031, 0.25, 0.5), 'grads3': (0.29, 2.4, 2.4), 'hidden': (0.0014, 0.0088, 0.017), 'params': (0.00028, 0.0018, 0.0028), 'saved0': (0.33, 4, 8.4), 'saved1': (0.041, 0.44, 0.73), 'saved2': (0.014, 0.18, 0.32), 'saved3': (0.0018, 0.019, 0.032)},
    'g_rows_hidden': {'grad_inputs': (0.014, 0.097, 0.17), 'grads0': (0.027, 0.32, 0.51), 'grads1': (0.084, 0.66, 1.2), 'grads2': (0.12, 0.57, 0.74), 'grads3': (0.63, 4.5, 7.9), 'hidden': (0.0014, 0.0086, 0.014), 'saved0': (0.34, 4.2, 6.9), 'saved1': (0.039, 0.43, 0.64), 'saved2': (0.015, 0.17, 0.29), 'saved3': (0.0019, 0.021, 0.034)},
    'bias_neg_hidden': {'grad_inputs': (0.081, 0.64, 0.9), 'grads0': (0.12, 0.52, 0.7), 'grads1': (0, 0, 0), 'grads2': (0.13, 0.58, 0.74), 'grads3': (0.64, 4.6, 7.1), 'hidden': (0.0003, 0.0022, 0.0033), 'saved0': (0.33, 4.2, 7), 'saved1': (0, 0, 0), 'saved2': (0.0032, 0.041, 0.066), 'saved3': (0.00041, 0.0045, 0.0071)},
    'zero_unit_hidden': {'grad_inputs': (0.014, 0.11, 0.16), 'grads0': (0.027, 0.35, 0.55), 'grads1': (0.087, 0.64, 1.1), 'grads2': (0.13, 0.55, 0.82), 'grads3': (0.63, 4.6, 7.3), 'hidden': (0.0014, 0.0091, 0.02), 'saved0': (0.33, 4.1, 6.6), 'saved1': (0.043, 0.44, 0.74), 'saved2': (0.014, 0.17, 0.32), 'saved3': (0.0018, 0.019, 0.035)},
    'made21_h64': {'grad_hidden': (0.71, 4.5, 6.1), 'grad_inputs': (0.19, 1.3, 2.1), 'grads0': (0.5, 4, 6.1), 'grads1': (0.21, 1.5, 2.1), 'grads2': (0.56, 4, 6.1), 'grads3': (0.25, 1.6, 2), 'hidden': (0.22, 1.3, 1.7), 'params': (0.13, 1.5, 2.1), 'saved0': (0.36, 3.8, 6.9), 'saved1': (0.14, 2.1, 3), 'saved2': (0.18, 1.7, 2.3), 'saved3': (0.094, 1.5, 1.9)},
    'made63_h128': {'grad_hidden': (0.66, 4.4, 6.8), 'grad_inputs': (0.16, 1.4, 1.9), 'grads0': (0.51, 3.8, 6.8), 'grads1': (0.19, 1.5, 2.2), 'hidden': (0.29, 1.9, 3.3), 'params': (0.16, 2, 3.6), 'saved0': (0.35, 4.1, 6.2), 'saved1': (0.078, 1.8, 3.4)},
    'i4_o40': {'gb': (0.46, 2, 2), 'gw': (0.72, 3.1, 3.2)},
    'i32_o96': {'gb': (0.54, 3.4, 3.5), 'gw': (0.69, 6.5, 7.5)},
    'i36_o128': {'gb': (0.6, 2.7, 2.8), 'gw': (0.71, 5.2, 7.8)},
    'i64_o40': {'gb': (0.39, 1.5, 1.5), 'gw': (0.66, 5.3, 6.4)},
    'i128_o128': {'gb': (0.62, 3.3, 3.3), 'gw': (0.69, 5.3, 6.8)},
    'i200_o96': {'gb': (0.62, 4.2, 4.5), 'gw': (0.7, 4.8, 7.7)},
    'o4_i64': {'gb': (0.58, 1.3, 1.3), 'gw': (0.68, 3.9, 4.1)},
    'o96_i36': {'gb': (0.55, 2.6, 2.6), 'gw': (0.69, 5.2, 7.5)},
    'o128_i32': {'gb': (0.59, 4, 4.2), 'gw': (0.72, 5, 5.9)},
    'o260_i64': {'gb': (0.51, 2.9, 3), 'gw': (0.68, 5.1, 7.2)},
    'o736_i128': {'gb': (0.58, 3.7, 4.3), 'gw': (0.7, 5.1, 9.4)},
    'o260_i32': {'gb': (0.61, 5.6, 6.6), 'gw': (0.69, 5, 8.5)},
    'b0_i36': {'gb': (0, 0, 0), 'gw': (0, 0, 0)},
    'b1_i36': {'gb': (0, 0, 0), 'gw': (0.68, 2, 2)},
    'b15_i36': {'gb': (0.58, 1.9, 1.9), 'gw': (0.75, 4.6, 4.8)},
    'b16_i36': {'gb': (0.64, 2.4, 2.5), 'gw': (0.81, 4.6, 4.8)},
    'b31_i36': {'gb': (0.59, 3.1, 3.1), 'gw': (0.73, 4.2, 4.7)},
    'b32_i36': {'gb': (0.59, 1.9, 1.9), 'gw': (0.73, 4.1, 6.3)},
    'b33_i36': {'gb': (0.58, 2.2, 2.2), 'gw': (0.8, 5.7, 7)},
    'b48_i36': {'gb': (0.67, 3.4, 3.5), 'gw': (0.73, 5, 7.5)},
    'b100_i36': {'gb': (0.59, 2.5, 2.5), 'gw': (0.7, 4.8, 5.1)},
    'b512_i36': {'gb': (0.39, 2, 2), 'gw': (0.68, 5.1, 5.4)},
    'b1000_i36': {'gb': (0.47, 2.2, 2.2), 'gw': (0.68, 5.1, 5.3)},
    'b1024_i36': {'gb': (0.57, 2.6, 2.6), 'gw': (0.68, 4.6, 5.2)},
    'b1_i32': {'gb': (0, 0, 0), 'gw': (0.75, 2, 2)},
    'b33_i32': {'gb': (0.4, 1.4, 1.4), 'gw': (0.74, 5.1, 6.3)},
    'b100_i32': {'gb': (0.48, 2, 2.1), 'gw': (0.7, 4.6, 8.6)},
    'b1000_i32': {'gb': (0.4, 1.6, 1.6), 'gw': (0.67, 3.9, 6.4)},
    'batched1_128x128': {'gb': (0.51, 3.1, 3.2), 'gw': (0.67, 5.3, 7.7)},
    'batched2_128x128': {'gb': (0.53, 4, 4.1), 'gw': (0.67, 5.1, 8.1)},
    'batched4_128x128': {'gb': (0.51, 3.4, 3.5), 'gw': (0.68, 5.2, 9.9)},
    'batched8_128x128': {'gb': (0.54, 4.9, 5.4), 'gw': (0.68, 5.1, 13)},
    'batched4_128x128_nobias': {'gw': (0.68, 4.9, 9.1)},
    'batched2_i32': {'gb': (0.58, 4.1, 4.2), 'gw': (0.71, 4.5, 7.9)},
    'batched8_i36': {'gb': (0.5, 2.7, 2.8), 'gw': (0.7, 5.3, 6.8)},
    'nonneg_i64': {'gb': (2.9, 12, 13), 'gw': (2.3, 11, 13)},
    'rows_i64': {'gb': (0.55, 2, 2), 'gw': (3.2, 20, 36)},
    'cols_i64': {'gb': (0.54, 3.3, 3.4), 'gw': (0.68, 5.6, 7.4)},
    'zero_cols_i64': {'gb': (0.58, 3.2, 3.3), 'gw': (0.69, 5.4, 7.6)},
    'nonneg_i32': {'gb': (5.9, 20, 20), 'gw': (4.7, 21, 22)},
    'rows_i32': {'gb': (0.53, 4.3, 4.4), 'gw': (2.9, 18, 19)},
    'zero_cols_i32': {'gb': (0.53, 2, 2), 'gw': (0.65, 4.3, 5)},
}
# CAPS-END


if __name__ == "__main__":
    _print_caps()
