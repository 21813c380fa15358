"""The table of tests/ar_spline_cases.py on the CPU, with a stand-in in each kernel's place: no case may ask what correct
fp32 arithmetic cannot give, and the rules are sharp.

K13's stand-in: the split-bf16 emulation of tests/test_train_kernels_host.py -- three bf16 pieces per operand, six
products per 16-column k-step, starting from the bias; K13's k-step ks holds columns ks * 8 .. ks * 8 + 7 of both lane
halves (half * 128 + ks * 8 + j) -- with the kernel's two accumulators (the leading product alone, the five small ones
together) and the hardware's rounding of the accumulator once per product and lane half, followed by the host build of
`rqs_eval_flat8` and the kernel's order of the log-determinant sum (per chunk and lane half feature after feature, the two
halves, then the chunks).
K12's stand-in: the step blocks of `ops.pack_made_schedule` walked in fp32 as maf_inverse_cases.walk_schedule walks them
in float64, with the kernel's summation order per lane (`dot_rows`: one FMA chain over the lane's chunks; `dot_rows_64`:
one partial sum per group of LPS chunks, (p0 + p1) + (p2 + p3)) and the DPP butterfly (a balanced tree over the lanes),
followed by the host build of the register form `rqs_eval<KT, true, true, true>` and the sequential fp32 sum of the T
log-derivatives.

CPU only.  -s for the figures."""
import ctypes
import shutil

import numpy as np
import pytest
import torch

import ar_spline_cases as A
import maf_inverse_cases as mi
import test_train_kernels_host as tkh
import train_kernel_cases as tk
from _hostcore import rqs_f32_host

_libs = []


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if not _libs:
        _libs.append(rqs_f32_host.build(str(tmp_path_factory.mktemp("arspline"))))
    return _libs[0]


def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------ K13's stand-in
K13_COLUMNS = np.concatenate([np.r_[ks * 8:ks * 8 + 8, 128 + ks * 8:128 + ks * 8 + 8] for ks in range(16)])


PRODUCTS = ("lh", "hl", "mm", "mh", "hm", "hh")     # NFA_MFMA6_SPLIT's order; first letter: the piece of the weight
HALVES = 2              # roundings of the accumulator per MFMA: the hardware adds the eight columns of lane half 0, rounds,
                        # then those of lane half 1 (measured on an MI355X: with ONE rounding per 16-column k-step the
                        # emulation agreed with the device bit for bit on 85 - 90 % of the elements at H <= 128, where the
                        # second half's columns are zero padding, and on 29 - 56 % at H = 132, 252, 256)


def k13_accumulate(bias, pw, ph, drop=None, split=True, halves=HALVES):
    """[M, N] float32: bias [M] + W [M, 256] h [N, 256]^T from the pieces pw, ph [3, rows, 256] (columns in k-step
    order) the way K13 accumulates: per k-step the six products, each rounded into its accumulator once per lane half;
    `split`: the five small products on an accumulator of their own, added to the leading one's at the end."""
    idx = {"h": 0, "m": 1, "l": 2}
    width = 16 // halves
    a = pw.view(3, pw.shape[1], 256 // width, width).permute(0, 2, 1, 3)      # [3, slices, M, width]
    b = ph.view(3, ph.shape[1], 256 // width, width).permute(0, 2, 3, 1)      # [3, slices, width, N]
    terms = dict((p, torch.matmul(a[idx[p[0]]], b[idx[p[1]]])) for p in PRODUCTS if p != drop)      # exact in float64
    acc = torch.from_numpy(np.array(np.broadcast_to(_f32(bias)[:, None], (pw.shape[1], ph.shape[1]))))
    small = torch.zeros_like(acc)
    for ks in range(16):
        for p in PRODUCTS:
            if p == drop:
                continue
            for s in range(ks * halves, (ks + 1) * halves):
                if split and p != "hh":
                    small = (small.double() + terms[p][s]).float()
                else:
                    acc = (acc.double() + terms[p][s]).float()
    return (acc + small).numpy()


def emulated_logits(hidden, W, b, drop=None, split=True):
    """[rows, W rows] float32: K13's accumulators (weights first operand, hidden second; from the bias)"""
    rows, H = hidden.shape
    hp, Wp = np.zeros((rows, 256), np.float32), np.zeros((W.shape[0], 256), np.float32)
    hp[:, :H], Wp[:, :H] = hidden, W
    hp, Wp = hp[:, K13_COLUMNS], Wp[:, K13_COLUMNS]
    out = np.empty((rows, W.shape[0]), np.float32)
    for r in range(0, rows, 256):
        ph = tkh._pieces(hp[r:r + 256])
        for s in range(0, W.shape[0], 256):
            out[r:r + 256, s:s + 256] = k13_accumulate(b[s:s + 256], tkh._pieces(Wp[s:s + 256]), ph, drop, split).T
    return out


def k13_lad(l):
    """[rows] float32: the kernel's order of the row sum of l [rows, nf]"""
    rows, nf = l.shape
    groups = (nf + 7) // 8 * 2
    lp = np.zeros((rows, groups * 4), np.float32)
    lp[:, :nf] = l
    lp = lp.reshape(rows, groups, 2, 2)
    total = None
    for g0 in range(0, groups, A.GROUPS_PER_CHUNK):
        acc = np.zeros((rows, 2), np.float32)
        for g in range(g0, min(groups, g0 + A.GROUPS_PER_CHUNK)):
            acc = acc + lp[:, g, :, 0]
            acc = acc + lp[:, g, :, 1]
        part = acc[:, 0] + acc[:, 1]
        total = part if total is None else total + part
    return total


def k13_standin(lib, net, x, hidden, first, inverse, divisor=0.0, drop=None, split=True):
    """(out [rows, D], lad [rows], status)"""
    W, b = A.final_rows(net, first)
    nf = x.shape[1] - first
    logits = _f32(emulated_logits(_f32(hidden), W, b, drop, split).reshape(-1, 23))
    xt = _f32(x[:, first:]).reshape(-1)
    y, l = np.empty_like(xt), np.empty_like(xt)
    spec = A.device_spec(8, divisor)
    status = lib.host_rqs_forward_flat8(int(inverse), xt.size, ctypes.byref(spec), _P(xt), _P(logits), _P(y), _P(l))
    out = np.array(x, dtype=np.float32)
    out[:, first:] = y.reshape(-1, nf)
    return out, k13_lad(l.reshape(-1, nf)), status


# ------------------------------------------------------------------------------------------------------ K12's stand-in
def _fma(a, b, c):
    return (a * b + c.astype(np.float64)).astype(np.float32)


def lane_dot(w, v, lps, use64, keep=None):
    """[B, R] float32: R rows w [R, k] on B vectors v [B, k] in the kernel's order.  `keep`: only the first `keep` lanes
    enter the butterfly (a mutant: without its last stage lane 0 holds the sum of lanes 0 .. 7)."""
    R, k = w.shape
    B = v.shape[0]
    groups = -(-(k // 4) // lps)
    wq, vq = np.zeros((R, groups * lps * 4)), np.zeros((B, groups * lps * 4))
    wq[:, :k], vq[:, :k] = w, v
    wq, vq = wq.reshape(1, R, groups, lps, 4), vq.reshape(B, 1, groups, lps, 4)
    if use64:
        assert k == 256
        part = []
        for g in range(groups):
            t = (wq[:, :, g, :, 0] * vq[:, :, g, :, 0]).astype(np.float32)
            for c in (1, 2, 3):
                t = _fma(wq[:, :, g, :, c], vq[:, :, g, :, c], t)
            part.append(t)
        lane = (part[0] + part[1]) + (part[2] + part[3]) if groups == 4 else part[0] + part[1]
    else:
        lane = np.zeros((B, R, lps), np.float32)
        for g in range(groups):
            for c in range(4):
                lane = _fma(wq[:, :, g, :, c], vq[:, :, g, :, c], lane)
    if keep:
        lane = lane[..., :keep]
    while lane.shape[-1] > 1:
        lane = lane[..., 0::2] + lane[..., 1::2]
    return lane[..., 0]


def k12_standin(lib, schedule, z, H, T, K, lps=16, divisor=0.0, dot=lane_dot):
    """(x [B, D] with columns < T found, lad [B], hidden [B, H], status); `dot`: the dot product (a mutant's, in
    test_k12_mutants_on_the_stand_in)"""
    blocks_f, block_at, layout = schedule
    blocks_f, block_at = blocks_f.cpu().numpy(), block_at.cpu().numpy()
    n, is_res, final_src, stream_vec, num_vectors, Hp, Xp, max_block = layout[:8]
    B, D = z.shape
    P = A.params_per_feature(K)
    xs = np.zeros((B, Xp), np.float32)
    vecs = np.zeros((num_vectors, B, Hp), np.float32)
    lad = np.zeros(B, np.float32)
    spec = A.device_spec(K, divisor)
    status = 0
    for t in range(T + 1):
        blk = blocks_f[int(block_at[t]) * 256:int(block_at[t + 1]) * 256]
        units, rows, out_rows, out_bias = (int(v) for v in blk[:4].view(np.int32))
        for u in range(units):
            e = blk[16 + 8 * u:24 + 8 * u]
            j, kp, src, dst, add_stream, set_stream = (int(v) for v in e[1:7].view(np.int32))
            w = blk[rows:rows + kp]
            rows += kp
            v = dot(w[None], xs[:, :kp] if src < 0 else vecs[src][:, :kp], lps, kp == 256)[:, 0] + e[0]
            if add_stream:
                v = vecs[stream_vec][:, j] + v
            if set_stream:
                vecs[stream_vec][:, j] = v
            if dst >= 0:
                vecs[dst][:, j] = np.where(v < 0, np.float32(0), v)
        assert rows == out_rows
        if t == T:
            break
        wf = blk[out_rows:out_bias].reshape(P, Hp)
        p = _f32(dot(wf, vecs[final_src], lps, Hp == 256) + blk[out_bias:out_bias + P])
        zt = _f32(z[:, t])
        y, l = np.empty_like(zt), np.empty_like(zt)
        status |= lib.host_rqs_forward_regs(K, 1, B, ctypes.byref(spec), _P(zt), _P(p), _P(y), _P(l))
        lad = lad + l
        xs[:, t] = y
    x = np.zeros((B, D), np.float32)
    x[:, :T] = xs[:, :T]
    return x, lad, vecs[final_src][:, :H].copy(), status


def _schedule(p):
    from nflows_amd import ops
    return ops.pack_made_schedule(p["net"], p["T"], A.params_per_feature(p["case"].K))


def _k12_run(lib, p, z=None):
    case = p["case"]
    return k12_standin(lib, _schedule(p), p["z"] if z is None else z, case.H, p["T"], case.K, case.lps)


def computed_caps(name):
    """2 x the larger yardstick of `hidden` on the stand-in's own x, rounded up to two digits"""
    if not _libs:
        import tempfile
        _libs.append(rqs_f32_host.build(tempfile.mkdtemp(prefix="arspline")))
    p = A.k12_prepared(name)
    x = _k12_run(_libs[0], p)[0]
    return A.caps_from(A.k12_hidden_yardsticks(p, x))


# ================================================================================================================ tests
def test_the_table_covers_what_it_says():
    grids = dict(((c.rows, c.D - c.first), A.k13_grid(c.rows, c.D - c.first)) for c in A.K13_CASES)
    assert grids[(384, 105)] == (3, 2, False) and grids[(1024, 105)] == (8, 2, True) and grids[(512, 313)] == (4, 4, True)
    assert grids[(128, 109)][1] == 2 and grids[(128, 209)][1] == 3 and grids[(128, 104)][1] == 1
    assert {c.rows for c in A.K13_CASES} >= {1, 127, 128, 129, 300}
    assert {c.H for c in A.K13_CASES} >= {4, 60, 128, 132, 252, 256}
    for c in A.K12_CASES:
        p = A.k12_prepared(c.name)
        units = A.units_per_step(_schedule(p), p["T"])
        assert A.k12_fits(_schedule(p)), c.name + ": outside K12's LDS budget"
        if not c.random_mask:
            assert p["T"] == min(c.H, c.D - 1)
        if c.blocks == 1 and not c.residual and not c.random_mask and c.H <= 2 * (c.D - 1):
            assert max(units) <= 4, (c.name, max(units))          # the read-ahead entries only
        if c.blocks == 5 or (c.D, c.H) == (20, 256):
            assert max(units) > 4, (c.name, max(units))           # both unit paths
        if c.name.startswith("d20_h30_n2_ff_rand"):
            assert 0 in units[:-1], "a step without a unit"
    assert A.k12_prepared("d260_h256_n1_res_k8_b16")["T"] == 256
    assert A.k12_prepared("d300_h240_n1_res_k8_b16")["T"] == 240
    assert sum(c.lps == 32 for c in A.K12_CASES) == 2


_dropped = {}


def _k13_dropped_misses(lib, name, inverse):
    if (name, inverse) not in _dropped:
        p = A.k13_prepared(name, inverse)
        case = p["case"]
        out, lad, status = k13_standin(lib, p["net"], p["x"], p["hidden"], case.first, inverse, drop="mm")
        try:
            A.k13_assert(p, inverse, out, lad, status, name + " mm dropped")
            _dropped[(name, inverse)] = False
        except AssertionError:
            _dropped[(name, inverse)] = True
    return _dropped[(name, inverse)]


@pytest.mark.parametrize("name,inverse", A.K13_PARAMS)
def test_k13_table_on_the_stand_in(lib, name, inverse):
    p = A.k13_prepared(name, inverse)
    case = p["case"]
    # the yardstick itself in the kernel's place: the inputs are fair
    ry, rl, rstatus = p["ref"]
    ref_out = p["x"].copy()
    ref_out[:, case.first:] = ry
    A.k13_assert(p, inverse, ref_out, cs_row_sum(rl), rstatus, name + " yardstick")
    out, lad, status = k13_standin(lib, p["net"], p["x"], p["hidden"], case.first, inverse)
    assert np.array_equal(out[:, :case.first].view(np.uint32), p["x"][:, :case.first].view(np.uint32))
    A.k13_assert(p, inverse, out, lad, status, name + " stand-in")
    _k13_dropped_misses(lib, name, inverse)


def cs_row_sum(l):
    return A.cs.fp32_row_sum(np.asarray(l).reshape(l.shape[0], -1))


# how many of the 70 (case, direction) pairs the emulation WITHOUT the mid * mid product misses (the rule is sharp:
# a product of relative size 2^-16 missing from the logits shows)
K13_MM_DROPPED_MISSES = 70


def test_the_emulation_without_mid_mid_fails_the_k13_table(lib):
    misses = sorted(k for k in A.K13_PARAMS if _k13_dropped_misses(lib, *k))
    print("mid * mid dropped: %d of %d (case, direction) pairs miss a rule" % (len(misses), len(A.K13_PARAMS)))
    assert len(misses) == K13_MM_DROPPED_MISSES, (len(misses), misses)


def test_the_single_accumulator_is_pinned_on_the_wide_cases(lib):
    """The defect the table found, in the emulation: with all six products on ONE accumulator (and the hardware's two
    roundings per product and k-step) the mean error against float64 of every case with H >= 252 is 1.53 - 3.44 x that of
    the kernel's two accumulators, and the single accumulator misses a rule somewhere in these ten (case, direction)
    pairs.  Both sides of the ratio are emulations (float64 products, explicit roundings) on the same inputs, so it does not
    depend on how the host's F.linear rounds (the yardstick is only printed: one accumulator 1.35 - 2.65 x its mean
    error, two 0.76 - 1.18 x; on the device one accumulator reached 2.5 x and missed the 2 x rule).  The bound: 192
    roundings at the sum's own magnitude against 32 is sqrt(6) = 2.4 x in the logits, diluted by the spline's own
    rounding, which both share and which is about as large as the two-accumulator logits' error: sqrt((6 + 1) / 2) =
    1.9 x expected, 1.25 x asked."""
    missed = 0
    for name in [c.name for c in A.K13_CASES if c.H >= 252]:
        for inverse in (False, True):
            p = A.k13_prepared(name, inverse)
            case = p["case"]
            ratio = {}
            for split in (True, False):
                out, lad, status = k13_standin(lib, p["net"], p["x"], p["hidden"], case.first, inverse, split=split)
                got, ty, ry = out[:, case.first:], p["truth"][0], p["ref"][0]
                fin = (np.abs(p["x"][:, case.first:]) <= A.TAIL_BOUND) & np.isfinite(got) & np.isfinite(ry)
                ratio[split] = float(np.abs(got[fin] - ty[fin]).mean() / np.abs(ry[fin] - ty[fin]).mean())
                if not split:
                    try:
                        A.k13_assert(p, inverse, out, lad, status, name + " single accumulator")
                    except AssertionError:
                        missed += 1
            print("%-24s %s mean error over the yardstick's: two accumulators %.2f, one %.2f" % (
                name, "inv" if inverse else "fwd", ratio[True], ratio[False]))
            assert ratio[False] >= 1.25 * ratio[True], (name, inverse, ratio)
    assert missed >= 1


@pytest.mark.parametrize("D,H", A.EXACT_K13)
@pytest.mark.parametrize("inverse", [False, True])
def test_k13_exact_logits_on_the_stand_in(lib, D, H, inverse):
    p = A.exact_k13_prepared(D, H, inverse)
    out, lad, status = k13_standin(lib, p["net"], p["x"], p["hidden"], 0, inverse, divisor=p["divisor"])
    # the emulated accumulators are the exact logits bit for bit
    W, b = A.final_rows(p["net"], 0)
    assert np.array_equal(emulated_logits(p["hidden"], W, b), p["raw"].reshape(A.EXACT_ROWS, -1).astype(np.float32))
    A.assert_exact_rule(out, lad, p["x"], p["o"], inverse, status, "exact K13 d%d h%d" % (D, H))


@pytest.mark.parametrize("D,H,first,rows", A.ONE_LAD_K13)
@pytest.mark.parametrize("inverse", [False, True])
def test_k13_one_log_derivative_per_row_on_the_stand_in(lib, D, H, first, rows, inverse):
    p = A.one_lad_k13_prepared(D, H, first, rows, inverse)
    out, lad, status = k13_standin(lib, p["net"], p["x"], p["hidden"], first, inverse)
    A.assert_one_lad(p, out[:, first:], lad, status, inverse, "one lad K13 d%d c%d" % (D, first))
    # a `lad_part` in the wrong chunk shows only if the chunks are told apart: the inside feature walks over all of them
    assert len(set(p["col"] // 104)) == A.k13_grid(rows, D - first)[1]


@pytest.mark.parametrize("name", A.K12_NAMES)
def test_k12_table_on_the_stand_in(lib, name):
    p = A.k12_prepared(name)
    x, lad, hidden, status = _k12_run(lib, p)
    caps = A.K12_HIDDEN_CAPS[name]
    A.k12_assert(p, x, lad, hidden, status, name + " stand-in", caps=caps, verbose=True)
    # the stored caps, recomputed: the yardsticks stay within half of them
    for y in A.k12_hidden_yardsticks(p, x):
        for s, c in zip(y, caps):
            assert tk.PARITY * s <= c, (name, y, caps)
    # float64 walk of the same blocks on the stand-in's x: the schedule computes the MADE
    row = 0
    params, _, h = mi.walk_schedule(_schedule(p), torch.from_numpy(x[row].astype(np.float64)))
    h64, params64 = A.made_forward(x[row:row + 1].astype(np.float64), p["arrays"], p["case"].residual)
    assert np.allclose(h.numpy()[:p["case"].H], h64[0], rtol=1e-12, atol=1e-12)
    assert np.allclose(params.numpy().reshape(-1), params64[0, :p["T"] * params.shape[1]], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", A.K12_NAMES)
def test_k12_table_on_the_yardstick(name):
    """The yardstick itself in the kernel's place -- the free-running fp32 chain on the CPU (F.linear per Linear, the
    oracle's float32 spline) and the eager fp32 hidden vector of its x -- through every rule: the inputs are fair."""
    p = A.k12_prepared(name)
    case, T = p["case"], p["T"]
    x, lad = A.chain(p["z"], p["arrays"], case.residual, case.K, T, tk.linear_ref)
    hidden = A.made_forward(x, p["arrays"], case.residual, tk.linear_ref)[0]
    A.k12_assert(p, x, lad, hidden, 0, name + " yardstick", caps=A.K12_HIDDEN_CAPS[name], verbose=True)


def full_inverse_standin(lib, p, z):
    """(x [B, D], lad [B]) of the class's whole inverse with stand-ins: K12's, then on its `hidden` K13's for the tail's
    columns (8 bins) or a plain fp32 Linear and the host build of the register form (10 bins: the GEMM and K5)."""
    case, T = p["case"], p["T"]
    x, lad, hidden, status = _k12_run(lib, p, z)
    if case.K == 8:
        out, lad_tail, st = k13_standin(lib, p["net"], z, hidden, T, True)
        x[:, T:] = out[:, T:]
    else:
        P = A.params_per_feature(case.K)
        W, b = A.final_rows(p["net"], T, P)
        logits = _f32(tk.linear_ref(hidden, W, b).reshape(-1, P))
        zt = _f32(z[:, T:]).reshape(-1)
        y, l = np.empty_like(zt), np.empty_like(zt)
        st = lib.host_rqs_forward_regs(case.K, 1, zt.size, ctypes.byref(A.device_spec(case.K)), _P(zt), _P(logits), _P(y), _P(l))
        x[:, T:] = y.reshape(z.shape[0], -1)
        lad_tail = cs_row_sum(l.reshape(z.shape[0], -1))
    assert (status | st) in (0, 2)
    return x, lad + lad_tail


@pytest.mark.parametrize("name", A.FULL_INVERSE_NAMES)
def test_full_inverse_on_the_stand_ins(lib, name):
    p = A.k12_prepared(name)
    case, T = p["case"], p["T"]
    assert T < case.D
    z = A.full_inverse_inputs(case)
    x, lad = full_inverse_standin(lib, p, z)
    x32, lad32, x64, lad64 = _full_chains(name)
    mi.assert_parity(x, x32, x64, name + " inverse x")
    mi.assert_parity(lad, lad32, lad64, name + " inverse lad")


_chains = {}


def _full_chains(name):
    """(x32, lad32, x64, lad64) of the whole inverse's yardstick and truth, computed once"""
    if name not in _chains:
        p = A.k12_prepared(name)
        case = p["case"]
        z = A.full_inverse_inputs(case)
        _chains[name] = (A.chain(z, p["arrays"], case.residual, case.K, case.D, tk.linear_ref) +
                         A.chain(z.astype(np.float64), p["arrays"], case.residual, case.K, case.D))
    return _chains[name]


@pytest.mark.parametrize("name", [c.name for c in A.K12_CASES if min(c.D, c.H) <= 64 and c.lps == 16])
def test_k12_free_running_chain_on_the_stand_in(lib, name):
    p = A.k12_prepared(name)
    case, T = p["case"], p["T"]
    assert T <= 64
    z = A.k12_inputs(case, A.FREE_ROWS)
    x, lad, _, _ = _k12_run(lib, p, z)
    x32, lad32 = A.chain(z, p["arrays"], case.residual, case.K, T, tk.linear_ref)
    x64, lad64 = A.chain(z.astype(np.float64), p["arrays"], case.residual, case.K, T)
    mi.assert_parity(x[:, :T], x32[:, :T], x64[:, :T], name + " x")
    mi.assert_parity(lad, lad32, lad64, name + " lad")


@pytest.mark.parametrize("D,H,K,residual,blocks", A.EXACT_K12)
def test_k12_exact_logits_on_the_stand_in(lib, D, H, K, residual, blocks):
    from nflows_amd import ops
    p = A.exact_k12_prepared(D, H, K, residual, blocks)
    sched = ops.pack_made_schedule(p["net"], p["T"], A.params_per_feature(K))
    assert A.k12_fits(sched)
    x, lad, hidden, status = k12_standin(lib, sched, p["z"], H, p["T"], K, divisor=p["divisor"])
    A.assert_exact_rule(x[:, :p["T"]], lad, p["zt"], p["o"], True, status, "exact K12 d%d h%d" % (D, H))


@pytest.mark.parametrize("name", ["d20_h30_n5_res_k10_b37", "d64_h48_n2_res_k8_b16"])
def test_k12_one_log_derivative_per_row_on_the_stand_in(lib, name):
    p = A.one_lad_k12_prepared(name)
    x, lad, _, status = _k12_run(lib, p, p["z"])
    t = A.k12_truth(p, x)
    A.assert_one_lad(dict(col=p["col"], ref=t["ref"], truth=t["truth"], cond=t["cond"]), x[:, :p["T"]], lad, status, True, name + " one lad")


def test_k12_mutants_on_the_stand_in(lib):
    """What the table sees of two of K12's mutants, pinned on the CPU: a butterfly without its last stage (the lanes of the
    upper half row missing from every sum) and a dot product that takes the other summation order (`kp == 256` through
    dot_rows: nothing but the order of a sum changes, and no rule may notice)."""
    name = "d260_h256_n1_res_k8_b16"
    p = A.k12_prepared(name)
    sched = _schedule(p)
    other_order = lambda w, v, lps, use64: lane_dot(w, v, lps, False)      # noqa: E731
    x, lad, hidden, status = k12_standin(lib, sched, p["z"], 256, p["T"], 8, dot=other_order)
    A.k12_assert(p, x, lad, hidden, status, name + " other order", caps=A.K12_HIDDEN_CAPS[name])
    half_sums = lambda w, v, lps, use64: lane_dot(w, v, lps, use64, keep=8)      # noqa: E731
    x, lad, hidden, status = k12_standin(lib, sched, p["z"], 256, p["T"], 8, dot=half_sums)
    with pytest.raises(AssertionError):
        A.k12_assert(p, x, lad, hidden, status, name + " half sums", caps=A.K12_HIDDEN_CAPS[name])
