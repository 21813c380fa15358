"""K13 (`rqs_made_output_kernel`) and K12 (`made_inverse_kernel<8 / 10, LPS>`) on the device against the float64 truth of
tests/ar_spline_cases.py, element by element: the table, the exact-logit cases, one log-derivative per row and what the
wrappers leave alone.  tests/test_ar_spline_host.py runs the same cases and rules on the CPU with stand-ins.

Which branch ran is asserted from outside the kernels: the label of `ops.last_layer_kernel()`, the grid from the shapes
(`ar_spline_cases.k13_grid`), the schedule's unit counts, call counters on the two ops where the class is called.
Columns a kernel must not write are checked on a prefilled `out=` buffer (both ops take one).  -s for the figures."""
import copy

import numpy as np
import pytest
import torch

import ar_spline_cases as A
import maf_inverse_cases as mi
import train_kernel_cases as tk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.25


def _status():
    from nflows_amd import ops
    w = ops._status_word(torch.device(DEV))
    s = int(w.item())
    w.zero_()
    return s


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _k13(net, x, hidden, first, inverse, divisor=0.0, out=None):
    """(out, lad) of K13 on device tensors; asserts the kernel that ran"""
    from nflows_amd import ops
    packed = ops.pack_made_output(net, 23, first_feature=first)
    r = ops.made_output_spline(x, hidden, packed, A.device_spec(8, divisor), first_column=first, inverse=inverse, out=out)
    assert r is not None, "K13 declined the shape"
    assert ops.last_layer_kernel() == "rqs_made_output_kernel<inverse=%d>" % int(inverse)
    return r


@pytest.mark.parametrize("name,inverse", A.K13_PARAMS)
def test_k13_table(name, inverse):
    p = A.k13_prepared(name, inverse)
    case = p["case"]
    row_blocks, chunks, renumbered = A.k13_grid(case.rows, case.D - case.first)
    assert renumbered == (name in ("d105_h64_c0_b1024", "d313_h64_c0_b512"))
    net = copy.deepcopy(p["net"]).to(DEV)
    x, hidden = _dev(p["x"]), _dev(p["hidden"])
    out, lad = _k13(net, x, hidden, case.first, inverse)
    status = _status()
    A.k13_assert(p, inverse, out.cpu().numpy(), lad.cpu().numpy(), status, name)
    # with a prefilled `out=`: the same bits in the transformed columns, the others untouched (ragged batches: through
    # the padded copy)
    buf = torch.full_like(x, SENTINEL)
    out2, lad2 = _k13(net, x, hidden, case.first, inverse, out=buf)
    _status()
    assert out2 is buf and torch.all(buf[:, :case.first] == SENTINEL)
    assert np.array_equal(_bits(buf[:, case.first:]), _bits(out[:, case.first:])) and np.array_equal(_bits(lad2), _bits(lad))


@pytest.mark.parametrize("D,H", A.EXACT_K13)
@pytest.mark.parametrize("inverse", [False, True])
def test_k13_exact_logits(D, H, inverse):
    p = A.exact_k13_prepared(D, H, inverse)
    out, lad = _k13(copy.deepcopy(p["net"]).to(DEV), _dev(p["x"]), _dev(p["hidden"]), 0, inverse, divisor=p["divisor"])
    A.assert_exact_rule(out.cpu().numpy(), lad.cpu().numpy(), p["x"], p["o"], inverse, _status(), "exact K13 d%d h%d" % (D, H))


@pytest.mark.parametrize("D,H,first,rows", A.ONE_LAD_K13)
@pytest.mark.parametrize("inverse", [False, True])
def test_k13_one_log_derivative_per_row(D, H, first, rows, inverse):
    p = A.one_lad_k13_prepared(D, H, first, rows, inverse)
    out, lad = _k13(copy.deepcopy(p["net"]).to(DEV), _dev(p["x"]), _dev(p["hidden"]), first, inverse)
    A.assert_one_lad(p, out.cpu().numpy()[:, first:], lad.cpu().numpy(), _status(), inverse, "one lad K13 d%d c%d" % (D, first))
    outside = np.abs(p["x"]) > A.TAIL_BOUND
    assert np.array_equal(_bits(out)[:, first:][outside[:, first:]], p["x"].view(np.uint32)[:, first:][outside[:, first:]])


@pytest.mark.parametrize("inverse", [False, True])
def test_what_made_output_spline_leaves_alone(inverse):
    """Rows evaluated alone are bit-equal to the same rows inside a larger batch (whole blocks and the ragged copy), two
    calls give equal bits, and the columns below first_column of a prefilled `out=` stay as they were."""
    case = A.K13_BY_NAME["d105_h64_c1_b300"]
    p = A.k13_prepared(case.name, inverse)
    net = copy.deepcopy(p["net"]).to(DEV)
    x, hidden = _dev(p["x"]), _dev(p["hidden"])
    first = case.first
    whole, lad = _k13(net, x, hidden, first, inverse)
    again, lad_again = _k13(net, x, hidden, first, inverse)
    assert np.array_equal(_bits(whole[:, first:]), _bits(again[:, first:])) and np.array_equal(_bits(lad), _bits(lad_again))
    for rows in (slice(0, 128), slice(128, 256), slice(256, 300), slice(17, 18), slice(100, 229)):
        buf = torch.full((rows.stop - rows.start, case.D), SENTINEL, device=DEV)
        part, lad_part = _k13(net, x[rows].contiguous(), hidden[rows].contiguous(), first, inverse, out=buf)
        assert torch.all(buf[:, :first] == SENTINEL)
        assert np.array_equal(_bits(part[:, first:]), _bits(whole[rows, first:])), rows
        assert np.array_equal(_bits(lad_part), _bits(lad[rows])), rows
    _status()


# ================================================================================================================== K12
def _k12(p, z, monkeypatch, K, H, T, lps=16, divisor=0.0, net=None):
    """(x, lad, hidden) of K12 as numpy arrays for z [B, D] (numpy), the [B, D] buffer prefilled: the columns >= T are
    not K12's to write.  Asserts the kernel that ran."""
    from nflows_amd import ops
    net = copy.deepcopy(p["net"] if net is None else net).to(DEV)
    schedule = ops.pack_made_schedule(net, T, A.params_per_feature(K))
    if lps == 32:
        monkeypatch.setenv("NFA_K12_LPS", "32")
    else:
        monkeypatch.delenv("NFA_K12_LPS", raising=False)
    buf = torch.full(z.shape, SENTINEL, device=DEV)
    r = ops.made_rqs_inverse(_dev(z), schedule, H, T, A.device_spec(K, divisor), out=buf)
    assert r is not None, "K12 declined the shape"
    assert ops.last_layer_kernel() == "made_rqs_inverse_kernel<K=%d, lanes_per_sample=%d>" % (K, lps)
    x, lad, hidden = r
    assert x is buf and torch.all(buf[:, T:] == SENTINEL), "K12 wrote a column >= T"
    return x.cpu().numpy(), lad.cpu().numpy(), hidden.cpu().numpy(), schedule


@pytest.mark.parametrize("name", A.K12_NAMES)
def test_k12_table(monkeypatch, name):
    p = A.k12_prepared(name)
    case, T = p["case"], p["T"]
    x, lad, hidden, schedule = _k12(p, p["z"], monkeypatch, case.K, case.H, T, case.lps)
    status = _status()
    units = A.units_per_step(schedule, T)
    if case.blocks == 5 or (case.D, case.H) == (20, 256):
        assert max(units) > 4          # both unit paths
    if not case.random_mask:
        assert T == min(case.H, case.D - 1)
    x[:, T:] = 0.0
    A.k12_assert(p, x, lad, hidden, status, name, caps=A.K12_HIDDEN_CAPS[name], verbose=True)


@pytest.mark.parametrize("name", [c.name for c in A.K12_CASES if min(c.D, c.H) <= 64 and c.lps == 16])
def test_k12_free_running_chain(monkeypatch, name):
    p = A.k12_prepared(name)
    case, T = p["case"], p["T"]
    z = A.k12_inputs(case, A.FREE_ROWS)
    x, lad, _, _ = _k12(p, z, monkeypatch, case.K, case.H, T)
    _status()
    x32, lad32 = A.chain(z, p["arrays"], case.residual, case.K, T, tk.linear_ref)
    x64, lad64 = A.chain(z.astype(np.float64), p["arrays"], case.residual, case.K, T)
    mi.assert_parity(x[:, :T], x32[:, :T], x64[:, :T], name + " x")
    mi.assert_parity(lad, lad32, lad64, name + " lad")


@pytest.mark.parametrize("name", A.FULL_INVERSE_NAMES)
def test_full_inverse_of_the_class_holds_the_chain_rule(monkeypatch, name):
    """T < D, every table case with H < D - 1: the class's `inverse` is K12, then K13's tail on K12's `hidden` (8 bins; 10
    bins: the GEMM and K5), held to the float64 chain over all D columns."""
    from nflows_amd import ops
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform as AR
    p = A.k12_prepared(name)
    case, T = p["case"], p["T"]
    assert T < case.D and case.H < case.D - 1
    t = AR(features=case.D, hidden_features=case.H, num_bins=case.K, tails="linear", tail_bound=A.TAIL_BOUND,
           num_blocks=case.blocks, use_residual_blocks=case.residual, random_mask=case.random_mask)
    t.autoregressive_net.load_state_dict(p["net"].state_dict())
    t = t.to(DEV).eval()
    calls = {"k12": 0, "k13": 0}
    real12, real13 = ops.made_rqs_inverse, ops.made_output_spline

    def count12(*a, **k):
        r = real12(*a, **k)
        calls["k12"] += r is not None
        return r

    def count13(*a, **k):
        r = real13(*a, **k)
        calls["k13"] += r is not None
        return r
    monkeypatch.setattr(ops, "made_rqs_inverse", count12)
    monkeypatch.setattr(ops, "made_output_spline", count13)
    if case.lps == 32:
        monkeypatch.setenv("NFA_K12_LPS", "32")
    else:
        monkeypatch.delenv("NFA_K12_LPS", raising=False)
    z = A.full_inverse_inputs(case)
    with torch.no_grad():
        x, lad = t.inverse(_dev(z))
    assert _status() in (0, 2)
    assert calls == {"k12": 1, "k13": int(case.K == 8)}, calls
    x32, lad32 = A.chain(z, p["arrays"], case.residual, case.K, case.D, tk.linear_ref)
    x64, lad64 = A.chain(z.astype(np.float64), p["arrays"], case.residual, case.K, case.D)
    mi.assert_parity(x.cpu().numpy(), x32, x64, name + " inverse x")
    mi.assert_parity(lad.cpu().numpy(), lad32, lad64, name + " inverse lad")


@pytest.mark.parametrize("D,H,K,residual,blocks", A.EXACT_K12)
def test_k12_exact_logits(monkeypatch, D, H, K, residual, blocks):
    p = A.exact_k12_prepared(D, H, K, residual, blocks)
    T = p["T"]
    x, lad, hidden, _ = _k12(p, p["z"], monkeypatch, K, H, T, divisor=p["divisor"])
    A.assert_exact_rule(x[:, :T], lad, p["zt"], p["o"], True, _status(), "exact K12 d%d h%d" % (D, H))
    # the hidden vector is a function of the biases alone: the same exact row for every sample
    h_exact, _ = A.made_forward(np.zeros((1, D)), A.made_arrays(p["net"]), residual)
    assert np.array_equal(hidden, np.broadcast_to(h_exact.astype(np.float32), hidden.shape))


@pytest.mark.parametrize("name", ["d20_h30_n5_res_k10_b37", "d64_h48_n2_res_k8_b16"])
def test_k12_one_log_derivative_per_row(monkeypatch, name):
    p = A.one_lad_k12_prepared(name)
    case, T = p["case"], p["T"]
    x, lad, _, _ = _k12(p, p["z"], monkeypatch, case.K, case.H, T)
    status = _status()
    x[:, T:] = 0.0
    t = A.k12_truth(p, x)
    A.assert_one_lad(dict(col=p["col"], ref=t["ref"], truth=t["truth"], cond=t["cond"]), x[:, :T], lad, status, True, name + " one lad")
    outside = np.abs(p["z"][:, :T]) > A.TAIL_BOUND
    assert np.array_equal(x[:, :T].view(np.uint32)[outside], p["z"][:, :T].view(np.uint32)[outside])


def test_k12_k13_packs_follow_the_parameters_and_the_masks(monkeypatch):
    """The K12 schedule and the K13 output pack of the class are rebuilt when a parameter changes in place, after
    `invalidate_packed_weights()` when it changed through `.data`, and when `load_state_dict` brings other masks: every
    result bit for bit a fresh copy's, one K12 and one K13 launch per `inverse`, one K13 launch per `forward`."""
    import nflows_amd
    from nflows_amd import ops
    from nflows_amd.transforms import MaskedPiecewiseRationalQuadraticAutoregressiveTransform as AR

    def build(seed):
        torch.manual_seed(seed)
        return AR(features=12, hidden_features=48, num_bins=8, tails="linear", tail_bound=3.0, use_residual_blocks=False,
                  random_mask=True).eval()
    layer = build(60).to(DEV)
    assert layer._sequential_steps() == 11
    x = torch.randn(64, 12, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    calls = {"k12": 0, "k13": 0}
    real12, real13 = ops.made_rqs_inverse, ops.made_output_spline

    def count12(*a, **k):
        r = real12(*a, **k)
        calls["k12"] += r is not None
        return r

    def count13(*a, **k):
        r = real13(*a, **k)
        calls["k13"] += r is not None
        return r
    monkeypatch.setattr(ops, "made_rqs_inverse", count12)
    monkeypatch.setattr(ops, "made_output_spline", count13)

    def both(t):
        with torch.no_grad():
            calls.update(k12=0, k13=0)
            forward = t(x)
            assert calls == {"k12": 0, "k13": 1}, calls
            calls.update(k12=0, k13=0)
            inverse = t.inverse(x)
            assert calls == {"k12": 1, "k13": 1}, calls
        assert _status() in (0, 2)
        return forward + inverse

    def fresh():
        return both(copy.deepcopy(layer))

    def same(a, b):
        return all(torch.equal(p, q) for p, q in zip(a, b))

    def different(a, b):   # (the forward pass and the inverse pass, each on its own)
        return not same(a[:2], b[:2]) and not same(a[2:], b[2:])
    net = layer.autoregressive_net
    written = list(net.final_layer.parameters()) + [net.initial_layer.weight]
    first = both(layer)
    assert same(first, fresh())
    with torch.no_grad():
        for p in written:
            p.mul_(2)
    doubled = both(layer)
    assert same(doubled, fresh()) and different(doubled, first)
    for p in written:
        p.data.mul_(0.5)
    nflows_amd.invalidate_packed_weights()
    halved = both(layer)
    assert same(halved, fresh()) and same(halved, first)
    other = build(61)
    masks = [k for k in other.state_dict() if k.endswith(".mask")]
    assert any(not torch.equal(other.state_dict()[k], layer.state_dict()[k].cpu()) for k in masks)
    layer.load_state_dict(other.state_dict())
    loaded = both(layer)
    assert same(loaded, both(other.to(DEV))) and different(loaded, halved)
