"""Cases, inputs, float64 truth, per-element allowance and caps for K27: the conditioner training kernels WITH a context
(nflows_amd/csrc/resnet_train.hip, `nfa_resnet_hidden_forward_ctx_f32` / `nfa_resnet_backward_ctx_f32`).  The rule, the
yardsticks and the factor are tests/train_kernel_cases.py's; tests/test_ctx_train_host.py holds the table to its yardsticks
and to two mutants on the CPU, tests/test_gpu_ctx_train.py runs the kernels through it.

  * The context Linears are not the kernels': their outputs arrive as [B, 128] planes (float32, exact zeros past the net's
    width).  The planes are INPUTS: they carry no allowance.
  * GLU (a ResidualNet, x = [inputs | context]): h = W_in x + b_in; per block t = relu(h), a = W_0 t + b_0, u = relu(a),
    y = W_1 u + b_1 (array pre{k}), s = sigmoid(c_k), h += y s.
        A(h') = A(h) + s A(y) + u (|h| + 2 |y s| + |y| s (1 - s) |c|)        (the last term: the sigmoid's own evaluation)
    Backward, ReLU masks AND pre{k} pinned to what the forward pass left (pre in float32: an input of the backward kernel):
        g_c = g pre s (1 - s)  (plane_grads{k}),   A = A(g) |pre| s (1 - s) + u |g pre| (4 s (1 - s) + s^2 + s (1 - s) |c|) + T
        g_t = g s              (gated_grads{k}),   A = A(g) s + u |g| (2 s + s (1 - s) |c|) + T
        g_a = (g_t W_1) m_a, g_h = g + (g_a W_0) m_h as in train_kernel_cases.py.
    s^2: float32 forms 1 - s from a rounded s (eager's glu_backward does), an absolute error of u s in it.  T = 4 x 2^-126
    where the element has a term at all: a product of float32 numbers below the smallest normal number is rounded to a
    multiple of 2^-149 or flushed.  Where float32(s) (1 - float32(s)) is exactly zero IN FLOAT32 -- a logit past +17.4,
    where s rounds to 1, or past -103.9, where it rounds to 0 -- g_c must be EXACTLY zero (allowance 0, truth 0).
  * ADD (a MADE): a = W_0 t + (b_0 + plane_k): the plane joins |b| in the Linear's allowance, and h_0's likewise with the
    initial plane.  The backward pass is train_kernel_cases.py's; the planes' gradients are grads{2k+1} and grads0 (or the
    incoming gradient without a block).
  * Caps: PARITY x max(Y_ref, Y_seq) per case, array and statistic, stored below (`python tests/ctx_train_cases.py` prints
    the literal).  Y_ref: eager fp32 on the CPU (F.linear, F.glu's arithmetic: torch.sigmoid, one product); Y_seq: the
    sequential fp32 chain with numpy's float32 sigmoid."""
import collections
import functools
import math

import numpy as np
import torch

from train_kernel_cases import (U, PARITY, ratio_stats, caps_from, assert_within_caps, linear_ref, linear_seq,  # noqa: F401
                                stats_of, misses, report, made_masks, effective, padded, _affine64, _uniform)

TINY = 4.0 * 2.0 ** -126
CtxCase = collections.namedtuple("CtxCase", "name mode B d C nb H out kind made seed")


def _table():
    rows = []

    def add(name, mode="glu", B=128, d=16, C=16, nb=1, H=128, out=40, kind="plain", made=0, seed=None):
        rows.append(CtxCase(name, mode, B, d, C, nb, H, out, kind, made, 27000 + len(rows) if seed is None else seed))

    # concatenated width d + C: 4 (3 + 1), a padded odd sum (3 + 2 -> 8), 8, the INIT_KS boundary 32 | 36, 64
    for d, C, out in ((3, 1, 0), (3, 2, 40), (5, 3, 0), (16, 16, 40), (20, 16, 0), (48, 16, 40)):
        add("glu_w%d_%s" % (d + C, "out40" if out else "hidden"), d=d, C=C, out=out)
    for nb in (2, 3):
        add("glu_nb%d_hidden" % nb, B=256, nb=nb, out=0)
        add("glu_nb%d_out24" % nb, B=256, nb=nb, out=24)
    for H, out in ((64, 24), (4, 0)):
        add("glu_h%d_%s" % (H, "out%d" % out if out else "hidden"), d=8, C=4, nb=2, H=H, out=out)
    add("glu_saturated_hidden", nb=2, out=0, kind="saturated")
    add("glu_saturated_out40", nb=2, out=40, kind="saturated")
    # ADD: plain nets (the kernels know no masks), every block count with and without the final Linear, narrow widths
    add("add_nb0_hidden", mode="add", nb=0, out=0)
    add("add_nb0_out40", mode="add", nb=0, out=40)
    for nb in (1, 2, 3):
        add("add_nb%d_hidden" % nb, mode="add", B=256, d=36 if nb == 2 else 8, nb=nb, out=0)
        add("add_nb%d_out24" % nb, mode="add", B=256, d=36 if nb == 2 else 8, nb=nb, out=24)
    add("add_h4_hidden", mode="add", d=8, nb=2, H=4, out=0)
    # a MADE's masks through pack_made_train, odd feature counts
    # (seed: units of low degree see a handful of inputs, and every product of the scheme is six MFMAs that each round an
    #  accumulator that starts at the bias -- train_kernel_cases.py CHANGED (2).  As there, a MADE case takes the first seed
    #  27023 + 100 k at which the EMULATED scheme on the CPU (test_ctx_train_host.py) passes: at 27023 it misses params by
    #  1.10 / 2.06 against 1.0 / 1.4 and grads3's maximum by 2.201 against 2.2, and so did the kernels, figure for figure)
    add("add_made21_h64_c5", mode="add", B=256, d=24, C=5, nb=2, H=64, out=44, made=21, seed=27123)
    add("add_made63_h128_c16", mode="add", B=256, d=64, C=16, nb=1, H=128, out=128, made=63)
    assert len(set(r.name for r in rows)) == len(rows)
    return rows


CASES = _table()
BY_NAME = dict((c.name, c) for c in CASES)
SATURATED = (88.8, -88.8, 104.0, -104.0)
HUGE_COLUMN = 11          # the +-30 000 column of the saturated cases


def di_of(case):
    """columns of the kernels' identity input: [inputs | context] in GLU mode, padded to a multiple of 4"""
    if case.made:
        return case.d
    return ((case.d + case.C if case.mode == "glu" else case.d) + 3) // 4 * 4


def net_of(case):
    """train_kernel_cases.k14_net's layout (w_in [H, D], b_in, blocks, final, masks) plus the context Linears:
    ctx_blocks [(Wc [H, C], bc)] per block and, ADD, ctx_in (Wc, bc)."""
    gen = torch.Generator().manual_seed(case.seed)
    H, C = case.H, case.C
    D = case.made or (case.d + C if case.mode == "glu" else case.d)
    net = {"w_in": _uniform(gen, (H, D), 1.0 / math.sqrt(D)), "b_in": _uniform(gen, (H,), 1.0 / math.sqrt(D)), "blocks": []}
    for _ in range(case.nb):
        net["blocks"].append((_uniform(gen, (H, H), 1.0 / math.sqrt(H)), _uniform(gen, (H,), 1.0 / math.sqrt(H)),
                              _uniform(gen, (H, H), 0.06), _uniform(gen, (H,), 0.06)))
    rows = 2 * case.made if case.made else case.out
    net["final"] = (_uniform(gen, (rows, H), 1.0 / math.sqrt(H)), _uniform(gen, (rows,), 1.0 / math.sqrt(H))) if rows else None
    net["masks"] = made_masks(D, H, case.nb) if case.made else None
    # (the gates' logits at a few units: sigmoid away from 1/2, both signs)
    net["ctx_blocks"] = [(_uniform(gen, (H, C), 3.0 / math.sqrt(C)), _uniform(gen, (H,), 1.0)) for _ in range(case.nb)]
    net["ctx_in"] = (_uniform(gen, (H, C), 1.0 / math.sqrt(C)), _uniform(gen, (H,), 1.0 / math.sqrt(C))) if case.mode == "add" else None
    return net


def data_of(case, rows=None, seed_offset=0):
    """(x [B, D] -- GLU: [inputs | context] --, g, planes [nb] of [B, 128], initial plane or None), float32.  The planes
    are the context Linears' eager fp32 outputs, zero past H."""
    B = case.B if rows is None else rows
    gen = torch.Generator().manual_seed(case.seed + 500 + seed_offset)
    net = net_of(case)
    ctx = torch.randn(B, case.C, generator=gen)
    if case.made:
        x = torch.randn(B, case.made, generator=gen)
    elif case.mode == "glu":
        x = torch.cat((torch.randn(B, case.d, generator=gen), ctx), dim=1)
    else:
        x = torch.randn(B, case.d, generator=gen)
    width = (2 * case.made if case.made else case.out) or 128
    g = torch.randn(B, width, generator=gen)
    if not case.out and not case.made:
        g[:, case.H:] = 0.0

    def plane(wc, bc):
        return torch.nn.functional.pad(torch.nn.functional.linear(ctx, wc, bc), (0, 128 - case.H)).contiguous()

    planes = [plane(wc, bc) for wc, bc in net["ctx_blocks"]]
    if case.kind == "saturated":
        for k, p in enumerate(planes):
            pick = torch.randint(0, 4, p.shape, generator=gen)
            p.copy_(torch.tensor(SATURATED)[pick])
            p[:, HUGE_COLUMN] = torch.where(torch.arange(B) % 2 == 0, 30000.0, -30000.0)
            p[:, case.H:] = 0.0
    initial = torch.relu(plane(*net["ctx_in"])) if case.mode == "add" else None
    return x.contiguous(), g.contiguous(), planes, initial


def forward_arrays(case):
    nb = case.nb
    return (["hidden"] + (["params"] if case.out or case.made else []) + ["saved%d" % j for j in range(2 * nb)]
            + (["pre%d" % k for k in range(nb)] if case.mode == "glu" else []))


def backward_arrays(case):
    nb = case.nb
    return ((["grad_hidden"] if case.out or case.made else []) + ["grads%d" % j for j in range(2 * nb)] + ["grad_inputs"]
            + (["plane_grads%d" % k for k in range(nb)] + ["gated_grads%d" % k for k in range(nb)] if case.mode == "glu" else []))


# ------------------------------------------------------------------------------------------------------ truth and allowance
def _d(a):
    return np.asarray(a.detach().numpy() if torch.is_tensor(a) else a, dtype=np.float64)


def sigmoid64(c):
    c = _d(c)
    e = np.exp(-np.abs(c))
    return np.where(c >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def forward_truth(case, e, x, planes, initial):
    """{array: (truth, allowance)} of the forward arrays and the float64 chain's own ReLU masks"""
    x = _d(x)
    out, masks = {}, []
    h, Ah = _affine64(x, np.zeros_like(x), _d(e["W_in"]), None)
    b_in = _d(e["b_in"])
    if case.mode == "add":
        h, Ah = h + b_in + _d(initial), Ah + U * (np.abs(b_in) + np.abs(_d(initial)))
    else:
        h, Ah = h + b_in, Ah + U * np.abs(b_in)
    for k, (w0, b0, w1, b1) in enumerate(e["blocks"]):
        t = np.maximum(h, 0.0)
        a, Aa = _affine64(t, Ah, _d(w0), None)
        if case.mode == "add":
            a, Aa = a + _d(b0) + _d(planes[k]), Aa + U * (np.abs(_d(b0)) + np.abs(_d(planes[k])))
        else:
            a, Aa = a + _d(b0), Aa + U * np.abs(_d(b0))
        u = np.maximum(a, 0.0)
        out["saved%d" % (2 * k)], out["saved%d" % (2 * k + 1)] = (t, Ah), (u, Aa)
        masks += [t > 0.0, u > 0.0]
        y, Ay = _affine64(u, Aa, _d(w1), _d(b1))
        if case.mode == "glu":
            c = _d(planes[k])
            s = sigmoid64(c)
            out["pre%d" % k] = (y, Ay)
            Ah = Ah + s * Ay + U * (np.abs(h) + 2.0 * np.abs(y * s) + np.abs(y) * s * (1.0 - s) * np.abs(c))
            h = h + y * s
        else:
            Ah = Ah + Ay + U * np.abs(h)
            h = h + y
    out["hidden"] = (h, Ah)
    if e["W_f"] is not None:
        out["params"] = _affine64(h, Ah, _d(e["W_f"]), _d(e["b_f"]))
    return out, masks


def gate_is_exactly_closed(c):
    """where float32(s) (1 - float32(s)) is exactly zero in float32: the gradient of the plane must be exactly zero"""
    s32 = sigmoid64(c).astype(np.float32)
    return (s32 * (np.float32(1.0) - s32)) == np.float32(0.0)


def backward_truth(case, e, g, masks, planes, pre):
    """{array: (truth, allowance)} of the backward arrays; `masks` [2 nb] pinned, `pre` [nb] (GLU) as the forward pass
    left it in float32"""
    g = _d(g)
    out = {}
    if e["W_f"] is not None:
        gh, Agh = _affine64(g, np.zeros_like(g), _d(e["W_f"]).T, None)
        out["grad_hidden"] = (gh, Agh)
    else:
        gh, Agh = g, np.zeros_like(g)
    for k in reversed(range(len(e["blocks"]))):
        w0, _, w1, _ = e["blocks"][k]
        mh, ma = _d(masks[2 * k]), _d(masks[2 * k + 1])
        if case.mode == "glu":
            c, p = _d(planes[k]), _d(pre[k])
            s = sigmoid64(c)
            q = 1.0 - s
            gp = np.abs(gh * p)
            gc = gh * p * s * q
            Agc = Agh * np.abs(p) * s * q + U * gp * (4.0 * s * q + s * s + s * q * np.abs(c)) + TINY * (gp > 0.0)
            closed = gate_is_exactly_closed(c)
            gc, Agc = np.where(closed, 0.0, gc), np.where(closed, 0.0, Agc)
            gt = gh * s
            Agt = Agh * s + U * np.abs(gh) * (2.0 * s + s * q * np.abs(c)) + TINY * (np.abs(gh) > 0.0)
            out["plane_grads%d" % k], out["gated_grads%d" % k] = (gc, Agc), (gt, Agt)
        else:
            gt, Agt = gh, Agh
        ga, Aga = _affine64(gt, Agt, _d(w1).T, None)
        ga, Aga = ga * ma, Aga * ma
        v, Av = _affine64(ga, Aga, _d(w0).T, None)
        Agh = Agh + Av * mh + U * np.abs(gh) * mh
        gh = gh + v * mh
        out["grads%d" % (2 * k + 1)], out["grads%d" % (2 * k)] = (ga, Aga), (gh, Agh)
    out["grad_inputs"] = _affine64(gh, Agh, _d(e["W_in"]).T, None)
    return out


# --------------------------------------------------------------------------------------------------------- the yardsticks
def sigmoid_ref(c):
    return torch.sigmoid(torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32))).numpy()


def sigmoid_seq(c):
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-c))).astype(np.float32)


def chain(case, e, x, g, masks, planes, initial, pre, linear, sigmoid, mutant=None):
    """Every array of both passes in fp32 with `linear` / `sigmoid` as the arithmetic; the backward pass through the pinned
    `masks` and, where `pre` is given, the pinned pre{k} (None: the chain's own).  mutant: "gate_c" gates with the logit
    itself, "pair_g" hands the second Linear g instead of g_t."""
    f = np.float32
    n = lambda a: np.asarray(a.detach().numpy() if torch.is_tensor(a) else a, dtype=f)      # noqa: E731
    out = {}
    own_pre = []
    h = linear(n(x), e["W_in"], e["b_in"] + n(initial) if case.mode == "add" else e["b_in"])
    for k, (w0, b0, w1, b1) in enumerate(e["blocks"]):
        t = np.maximum(h, f(0.0))
        u = np.maximum(linear(t, w0, b0 + n(planes[k]) if case.mode == "add" else b0), f(0.0))
        out["saved%d" % (2 * k)], out["saved%d" % (2 * k + 1)] = t, u
        y = linear(u, w1, b1)
        if case.mode == "glu":
            out["pre%d" % k] = y
            own_pre.append(y)
            h = h + y * (n(planes[k]) if mutant == "gate_c" else sigmoid(n(planes[k])))
        else:
            h = h + y
    out["hidden"] = h
    gh = n(g)
    if e["W_f"] is not None:
        out["params"] = linear(h, e["W_f"], e["b_f"])
        gh = out["grad_hidden"] = linear(gh, np.ascontiguousarray(e["W_f"].T), None)
    for k in reversed(range(len(e["blocks"]))):
        w0, _, w1, _ = e["blocks"][k]
        gt = gh
        if case.mode == "glu":
            s = sigmoid(n(planes[k]))
            p = n(pre[k]) if pre is not None else own_pre[k]
            out["plane_grads%d" % k] = ((f(1.0) - s) * s) * gh * p          # (glu_backward's order)
            gt = out["gated_grads%d" % k] = gh * s
        ga = linear(gh if mutant == "pair_g" else gt, np.ascontiguousarray(w1.T), None) * masks[2 * k + 1].astype(f)
        gh = gh + linear(ga, np.ascontiguousarray(w0.T), None) * masks[2 * k].astype(f)
        out["grads%d" % (2 * k + 1)], out["grads%d" % (2 * k)] = ga, gh
    out["grad_inputs"] = linear(gh, np.ascontiguousarray(e["W_in"].T), None)
    return out


def _linear_with_plane(linear):
    """`linear(v, W, b)` where b may be a [B, 128] accumulator start (bias + plane): Y_ref adds it behind the product"""
    def call(v, W, b):
        if b is None or np.ndim(b) == 1:
            return linear(v, W, b)
        if linear is linear_seq:
            return linear(v, W, b)
        return linear(v, W, None) + np.asarray(b, dtype=np.float32)
    return call


@functools.lru_cache(maxsize=None)
def prepared(name):
    """`prepare(case)` of a case of the table, once per process (shared, never modified)"""
    return prepare(BY_NAME[name])


def prepare(case):
    """Net, inputs, truth and the float64 chain's masks of a case.  The backward truth here runs through the float64
    chain's own masks and its own pre{k} rounded to float32."""
    net = net_of(case)
    x, g, planes, initial = data_of(case)
    di = di_of(case)
    out = (2 * case.made + 3) // 4 * 4 if case.made else case.out
    e = effective(net, di, out)
    xp, gp = padded(x.numpy(), di), padded(g.numpy(), out or 128)
    fwd, masks = forward_truth(case, e, xp, planes, initial)
    pre = [fwd["pre%d" % k][0].astype(np.float32) for k in range(case.nb)] if case.mode == "glu" else None
    truth = dict(fwd)
    truth.update(backward_truth(case, e, gp, masks, planes, pre))
    assert sorted(truth) == sorted(forward_arrays(case) + backward_arrays(case))
    return dict(case=case, net=net, x=x, g=g, planes=planes, initial=initial, e=e, xp=xp, gp=gp, truth=truth, masks=masks,
                pre=pre, di=di, out=out)


def yardsticks(p, mutant=None):
    """(stats of Y_ref, stats of Y_seq) of a prepared case (or of a mutant of them)"""
    return tuple(stats_of(chain(p["case"], p["e"], p["xp"], p["gp"], p["masks"], p["planes"], p["initial"], p["pre"],
                                _linear_with_plane(lin), sig, mutant), p["truth"], p["case"].name)
                 for lin, sig in ((linear_ref, sigmoid_ref), (linear_seq, sigmoid_seq)))


def compute_caps():
    return dict((c.name, caps_from(*yardsticks(prepared(c.name)))) for c in CASES)


def _print_caps():
    caps = compute_caps()
    print("CAPS = {")
    for c in CASES:
        print("    %r: {%s}," % (c.name, ", ".join("%r: (%g, %g, %g)" % ((k,) + v) for k, v in sorted(caps[c.name].items()))))
    print("}")


# PARITY x max(Y_ref, Y_seq) of (mean, 99.9 % quantile, max) per case and array, rounded up to two digits
# (`python tests/ctx_train_cases.py` prints this literal).
# CAPS-BEGIN
CAPS = {
    'glu_w4_hidden': {'gated_grads0': (0.56, 2.4, 2.7), 'grad_inputs': (0.069, 0.4, 0.44), 'grads0': (0.064, 0.33, 0.44), 'grads1': (0.23, 1.6, 2.1), 'hidden': (0.093, 1.3, 2.2), 'plane_grads0': (0.34, 2.5, 2.9), 'pre0': (0.015, 0.082, 0.12), 'saved0': (0.39, 3.7, 5.6), 'saved1': (0.063, 0.82, 1.6)},
    'glu_w5_out40': {'gated_grads0': (0.47, 2.6, 3.7), 'grad_hidden': (0.66, 4.4, 6.4), 'grad_inputs': (0.024, 0.14, 0.14), 'grads0': (0.37, 4.1, 6.4), 'grads1': (0.11, 0.59, 0.87), 'hidden': (0.088, 1.2, 1.8), 'params': (0.02, 0.14, 0.18), 'plane_grads0': (0.38, 2.1, 2.6), 'pre0': (0.015, 0.085, 0.12), 'saved0': (0.35, 3.9, 5), 'saved1': (0.066, 0.85, 1.6)},
    'glu_w8_hidden': {'gated_grads0': (0.55, 2.4, 2.8), 'grad_inputs': (0.059, 0.47, 0.52), 'grads0': (0.058, 0.3, 0.37), 'grads1': (0.24, 1.7, 2.6), 'hidden': (0.087, 1.2, 1.7), 'plane_grads0': (0.34, 2.3, 2.8), 'pre0': (0.013, 0.076, 0.088), 'saved0': (0.35, 3.8, 6.4), 'saved1': (0.057, 0.64, 1.5)},
    'glu_w32_out40': {'gated_grads0': (0.46, 2.7, 4.2), 'grad_hidden': (0.64, 4.6, 6.9), 'grad_inputs': (0.025, 0.16, 0.25), 'grads0': (0.36, 4.2, 6.9), 'grads1': (0.11, 0.64, 1.1), 'hidden': (0.086, 1.5, 2.5), 'params': (0.011, 0.072, 0.15), 'plane_grads0': (0.38, 2.2, 3.2), 'pre0': (0.0082, 0.044, 0.059), 'saved0': (0.33, 4.3, 7.6), 'saved1': (0.038, 0.43, 0.69)},
    'glu_w36_hidden': {'gated_grads0': (0.55, 2.3, 3), 'grad_inputs': (0.062, 0.46, 0.68), 'grads0': (0.058, 0.29, 0.36), 'grads1': (0.23, 1.6, 2.6), 'hidden': (0.085, 1.3, 2.8), 'plane_grads0': (0.35, 2.2, 2.7), 'pre0': (0.0077, 0.039, 0.063), 'saved0': (0.34, 4.2, 5.8), 'saved1': (0.039, 0.41, 0.61)},
    'glu_w64_out40': {'gated_grads0': (0.47, 2.6, 3.7), 'grad_hidden': (0.67, 4.8, 6.8), 'grad_inputs': (0.026, 0.17, 0.26), 'grads0': (0.37, 4.3, 6.2), 'grads1': (0.11, 0.64, 0.85), 'hidden': (0.083, 1.5, 2.6), 'params': (0.0091, 0.054, 0.076), 'plane_grads0': (0.38, 2.2, 3.3), 'pre0': (0.0062, 0.033, 0.038), 'saved0': (0.33, 4, 8.6), 'saved1': (0.033, 0.32, 0.52)},
    'glu_nb2_hidden': {'gated_grads0': (0.32, 2.2, 2.8), 'gated_grads1': (0.55, 2.3, 2.8), 'grad_inputs': (0.015, 0.13, 0.16), 'grads0': (0.019, 0.16, 0.32), 'grads1': (0.06, 0.43, 0.67), 'grads2': (0.058, 0.28, 0.36), 'grads3': (0.23, 1.8, 2.7), 'hidden': (0.008, 0.19, 0.59), 'plane_grads0': (0.24, 2.1, 2.5), 'plane_grads1': (0.35, 2.2, 2.8), 'pre0': (0.0078, 0.042, 0.071), 'pre1': (0.00067, 0.0036, 0.0051), 'saved0': (0.32, 4.1, 6.3), 'saved1': (0.038, 0.4, 0.84), 'saved2': (0.041, 1.2, 2), 'saved3': (0.0033, 0.035, 0.061)},
    'glu_nb2_out24': {'gated_grads0': (0.27, 2.3, 3.4), 'gated_grads1': (0.46, 2.5, 3.3), 'grad_hidden': (0.69, 4.8, 6.8), 'grad_inputs': (0.0071, 0.055, 0.076), 'grads0': (0.36, 4.3, 6.7), 'grads1': (0.03, 0.21, 0.3), 'grads2': (0.39, 4.3, 6.7), 'grads3': (0.12, 0.76, 1.1), 'hidden': (0.0084, 0.21, 0.75), 'params': (0.00099, 0.007, 0.0091), 'plane_grads0': (0.24, 2, 2.7), 'plane_grads1': (0.37, 2.2, 3), 'pre0': (0.0083, 0.047, 0.065), 'pre1': (0.00068, 0.0037, 0.0053), 'saved0': (0.32, 4.1, 6.5), 'saved1': (0.042, 0.43, 0.82), 'saved2': (0.043, 1.2, 3.2), 'saved3': (0.0035, 0.039, 0.075)},
    'glu_nb3_hidden': {'gated_grads0': (0.28, 2.2, 2.8), 'gated_grads1': (0.31, 2.2, 2.7), 'gated_grads2': (0.55, 2.4, 3.2), 'grad_inputs': (0.0033, 0.027, 0.038), 'grads0': (0.006, 0.15, 0.26), 'grads1': (0.015, 0.11, 0.2), 'grads2': (0.017, 0.16, 0.26), 'grads3': (0.059, 0.44, 0.64), 'grads4': (0.058, 0.29, 0.37), 'grads5': (0.23, 1.5, 2.1), 'hidden': (0.00072, 0.02, 0.076), 'plane_grads0': (0.2, 2.1, 2.7), 'plane_grads1': (0.23, 2.1, 2.6), 'plane_grads2': (0.35, 2.2, 2.7), 'pre0': (0.0081, 0.043, 0.074), 'pre1': (0.00075, 0.0042, 0.0065), 'pre2': (5.7e-05, 0.00031, 0.00049), 'saved0': (0.34, 4.2, 7.3), 'saved1': (0.041, 0.46, 0.97), 'saved2': (0.043, 1.2, 2.8), 'saved3': (0.0039, 0.04, 0.067), 'saved4': (0.004, 0.15, 0.79), 'saved5': (0.00028, 0.003, 0.0054)},
    'glu_nb3_out24': {'gated_grads0': (0.24, 2.3, 3.6), 'gated_grads1': (0.27, 2.2, 3.9), 'gated_grads2': (0.46, 2.5, 3.7), 'grad_hidden': (0.68, 4.6, 7.2), 'grad_inputs': (0.0019, 0.014, 0.018), 'grads0': (0.34, 4.2, 6.1), 'grads1': (0.008, 0.057, 0.1), 'grads2': (0.35, 4.2, 6.1), 'grads3': (0.031, 0.2, 0.41), 'grads4': (0.38, 4.2, 6.1), 'grads5': (0.12, 0.74, 1.1), 'hidden': (0.00072, 0.016, 0.057), 'params': (8.3e-05, 0.00055, 0.0011), 'plane_grads0': (0.2, 1.9, 3.3), 'plane_grads1': (0.24, 2, 3.4), 'plane_grads2': (0.37, 2.1, 3.2), 'pre0': (0.0084, 0.049, 0.071), 'pre1': (0.0007, 0.004, 0.0059), 'pre2': (6e-05, 0.00033, 0.00052), 'saved0': (0.33, 3.9, 7.3), 'saved1': (0.04, 0.41, 0.65), 'saved2': (0.042, 1.2, 2.5), 'saved3': (0.0034, 0.034, 0.061), 'saved4': (0.004, 0.14, 0.63), 'saved5': (0.0003, 0.0033, 0.0083)},
    'glu_h64_out24': {'gated_grads0': (0.3, 2.2, 2.9), 'gated_grads1': (0.46, 2.4, 3.5), 'grad_hidden': (0.68, 4.5, 6), 'grad_inputs': (0.029, 0.2, 0.26), 'grads0': (0.36, 4.1, 5.6), 'grads1': (0.059, 0.33, 0.46), 'grads2': (0.41, 4.1, 5.6), 'grads3': (0.13, 0.67, 1.1), 'hidden': (0.037, 0.48, 0.95), 'params': (0.0085, 0.051, 0.059), 'plane_grads0': (0.26, 1.9, 2.7), 'plane_grads1': (0.37, 2, 2.6), 'pre0': (0.019, 0.11, 0.15), 'pre1': (0.0038, 0.021, 0.041), 'saved0': (0.37, 4.1, 5.6), 'saved1': (0.059, 0.62, 1.1), 'saved2': (0.084, 1.5, 2.5), 'saved3': (0.014, 0.14, 0.23)},
    'glu_h4_hidden': {'gated_grads0': (0.49, 2.1, 2.4), 'gated_grads1': (0.61, 2.7, 3), 'grad_inputs': (0.51, 3.7, 4), 'grads0': (0.39, 1.3, 1.3), 'grads1': (0.32, 1.4, 1.6), 'grads2': (0.61, 1.7, 1.7), 'grads3': (0.39, 1.5, 1.5), 'hidden': (0.38, 1.7, 1.7), 'plane_grads0': (0.31, 1.8, 2), 'plane_grads1': (0.38, 2.2, 2.3), 'pre0': (0.19, 0.94, 1.1), 'pre1': (0.12, 0.6, 0.66), 'saved0': (0.28, 3, 3.3), 'saved1': (0.16, 1.5, 1.5), 'saved2': (0.18, 2, 2.2), 'saved3': (0.086, 0.99, 1.2)},
    'glu_saturated_hidden': {'gated_grads0': (0.038, 0.35, 0.45), 'gated_grads1': (0.023, 0.34, 0.46), 'grad_inputs': (0.015, 0.12, 0.16), 'grads0': (0.019, 0.15, 0.34), 'grads1': (0.055, 0.4, 0.49), 'grads2': (0.062, 0.31, 0.39), 'grads3': (0.22, 1.6, 2.1), 'hidden': (0.13, 2.1, 3.2), 'plane_grads0': (0.0054, 0.05, 0.081), 'plane_grads1': (0.0059, 0.058, 0.067), 'pre0': (0.0079, 0.044, 0.07), 'pre1': (0.00069, 0.0037, 0.0056), 'saved0': (0.35, 4.1, 6), 'saved1': (0.041, 0.42, 0.76), 'saved2': (0.15, 2.6, 4.4), 'saved3': (0.0034, 0.035, 0.062)},
    'glu_saturated_out40': {'gated_grads0': (0.15, 2.4, 3.1), 'gated_grads1': (0.25, 2.6, 3.9), 'grad_hidden': (0.66, 4.7, 6.5), 'grad_inputs': (0.0072, 0.05, 0.064), 'grads0': (0.33, 4.4, 6.1), 'grads1': (0.03, 0.18, 0.27), 'grads2': (0.37, 4.4, 6.1), 'grads3': (0.11, 0.59, 0.76), 'hidden': (0.13, 2.1, 3), 'params': (0.00096, 0.0071, 0.0096), 'plane_grads0': (0.0018, 0.019, 0.022), 'plane_grads1': (0.0017, 0.016, 0.021), 'pre0': (0.0079, 0.044, 0.07), 'pre1': (0.00064, 0.0033, 0.0046), 'saved0': (0.33, 4.1, 6), 'saved1': (0.039, 0.4, 0.72), 'saved2': (0.15, 2.6, 4), 'saved3': (0.0031, 0.033, 0.057)},
    'add_nb0_hidden': {'grad_inputs': (0.64, 4.4, 7.1), 'hidden': (0.75, 5.3, 6.3)},
    'add_nb0_out40': {'grad_hidden': (0.66, 4.8, 6.8), 'grad_inputs': (0.12, 0.65, 1.1), 'hidden': (0.77, 5.1, 7.2), 'params': (0.17, 1.2, 1.8)},
    'add_nb1_hidden': {'grad_inputs': (0.072, 0.61, 0.68), 'grads0': (0.13, 0.57, 1), 'grads1': (0.63, 4.6, 7.3), 'hidden': (0.076, 0.42, 0.82), 'saved0': (0.54, 4.6, 6.8), 'saved1': (0.36, 5.3, 7.9)},
    'add_nb1_out24': {'grad_hidden': (0.69, 4.7, 7.5), 'grad_inputs': (0.018, 0.13, 0.19), 'grads0': (0.3, 4, 7.5), 'grads1': (0.14, 0.93, 1.4), 'hidden': (0.075, 0.39, 0.66), 'params': (0.012, 0.064, 0.11), 'saved0': (0.5, 4.3, 6.2), 'saved1': (0.35, 5.3, 11)},
    'add_nb2_hidden': {'grad_inputs': (0.011, 0.076, 0.11), 'grads0': (0.033, 0.44, 0.79), 'grads1': (0.076, 0.54, 0.79), 'grads2': (0.13, 0.55, 0.88), 'grads3': (0.62, 4.7, 8.6), 'hidden': (0.0032, 0.016, 0.024), 'saved0': (0.53, 5.4, 8.7), 'saved1': (0.23, 3.6, 6), 'saved2': (0.035, 0.29, 0.43), 'saved3': (0.0098, 0.18, 0.28)},
    'add_nb2_out24': {'grad_hidden': (0.68, 4.5, 6.6), 'grad_inputs': (0.0024, 0.017, 0.023), 'grads0': (0.21, 3.8, 6.1), 'grads1': (0.018, 0.12, 0.2), 'grads2': (0.31, 3.9, 6.6), 'grads3': (0.14, 0.95, 1.7), 'hidden': (0.0034, 0.017, 0.025), 'params': (0.00048, 0.0024, 0.0033), 'saved0': (0.54, 5.5, 7.8), 'saved1': (0.25, 3.7, 6.9), 'saved2': (0.036, 0.3, 0.41), 'saved3': (0.012, 0.17, 0.29)},
    'add_nb3_hidden': {'grad_inputs': (0.0015, 0.0094, 0.013), 'grads0': (0.011, 0.38, 0.61), 'grads1': (0.011, 0.078, 0.14), 'grads2': (0.031, 0.42, 0.74), 'grads3': (0.079, 0.56, 0.88), 'grads4': (0.13, 0.61, 0.89), 'grads5': (0.64, 5.1, 8.6), 'hidden': (0.00024, 0.0012, 0.0017), 'saved0': (0.52, 4.6, 6.9), 'saved1': (0.33, 5.2, 8.9), 'saved2': (0.044, 0.36, 0.67), 'saved3': (0.016, 0.25, 0.44), 'saved4': (0.0025, 0.021, 0.039), 'saved5': (0.00066, 0.011, 0.019)},
    'add_nb3_out24': {'grad_hidden': (0.69, 4.8, 7.4), 'grad_inputs': (0.00031, 0.002, 0.0024), 'grads0': (0.16, 3.6, 7.2), 'grads1': (0.0023, 0.016, 0.027), 'grads2': (0.22, 3.9, 7.2), 'grads3': (0.018, 0.13, 0.2), 'grads4': (0.3, 4, 7.2), 'grads5': (0.15, 0.94, 1.5), 'hidden': (0.00026, 0.0013, 0.0021), 'params': (3.5e-05, 0.0002, 0.00026), 'saved0': (0.53, 4.4, 6.4), 'saved1': (0.35, 5.5, 9.2), 'saved2': (0.047, 0.35, 0.66), 'saved3': (0.017, 0.27, 0.51), 'saved4': (0.003, 0.023, 0.033), 'saved5': (0.00074, 0.013, 0.03)},
    'add_h4_hidden': {'grad_inputs': (0.48, 2.8, 4.1), 'grads0': (0.47, 1.8, 1.8), 'grads1': (0.61, 3.2, 3.4), 'grads2': (0.65, 1.8, 1.8), 'grads3': (0.74, 3.1, 3.2), 'hidden': (0.32, 1.6, 1.8), 'saved0': (0.43, 3.6, 4.1), 'saved1': (0.3, 3.6, 4.6), 'saved2': (0.25, 2.3, 2.8), 'saved3': (0.21, 2.1, 2.3)},
    'add_made21_h64_c5': {'grad_hidden': (0.7, 4.6, 6.6), 'grad_inputs': (0.17, 1.2, 1.8), 'grads0': (0.44, 3.7, 5.8), 'grads1': (0.2, 1.4, 1.7), 'grads2': (0.53, 3.9, 6.6), 'grads3': (0.25, 1.7, 2), 'hidden': (0.17, 1.1, 1.8), 'params': (0.084, 1.1, 1.5), 'saved0': (0.55, 5.1, 7.6), 'saved1': (0.53, 6.1, 8.6), 'saved2': (0.19, 1.6, 2.4), 'saved3': (0.3, 4.5, 6.7)},
    'add_made63_h128_c16': {'grad_hidden': (0.66, 4.5, 6.5), 'grad_inputs': (0.15, 1.2, 1.8), 'grads0': (0.46, 3.9, 6.4), 'grads1': (0.19, 1.3, 2.1), 'hidden': (0.26, 1.7, 2.8), 'params': (0.1, 1.2, 2.1), 'saved0': (0.61, 5.6, 7.9), 'saved1': (0.57, 7.1, 12)},
}
# CAPS-END


if __name__ == "__main__":
    _print_caps()
