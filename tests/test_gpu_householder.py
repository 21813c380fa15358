"""K24 (HouseholderSequence, SVDLinear, QRLinear) and NaiveLinear on the GPU against the reference's float32 / float64
results (tests/golden/hh_*.npz, naive_linear_*.npz, hh_flow.npz; written by tests/golden/make_golden_householder.py) under
the project's parity rule -- `compare()` of tests/test_gpu_headline_parity.py: error against float64 at most 2 x the
reference-float32's own on maximum (+ four ulps), mean and 99.9 % quantile -- and the properties of the kernel that are
exact."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import LAD_TOL, OUT_TOL
from householder_cases import (ALL_CASES, GOLDEN, KINDS, LINEAR_CASES, case_id, case_inputs, golden, layer_of,
                               naive_golden, new_layer, state_of, truth)
from test_gpu_headline_parity import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rows_equal(lad):
    return bool((lad == lad[0]).all())


def check_both_directions(t, g, x, tag, suffix=""):
    with torch.no_grad():
        y, lad = t(dev(x))
        xi, ladi = t.inverse(dev(g["y"]))
    assert y.shape == x.shape and lad.shape == (x.shape[0],) and rows_equal(lad) and rows_equal(ladi)
    compare(tag, "y", y.cpu().numpy(), g["y" + suffix], truth(g, "y"), OUT_TOL)
    compare(tag, "x", xi.cpu().numpy(), g["xi" + suffix], truth(g, "xi"), OUT_TOL)
    return lad, ladi


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_parity_both_directions(case, kind):
    cls, features, count = case
    g = golden(cls, features, count, kind)
    x, _ = case_inputs(cls, features, count, kind)
    tag = "householder %s D=%d K=%d %s" % (cls, features, count, kind)
    lad, ladi = check_both_directions(layer_of(g, cls, features, count).to(DEV), g, x, tag)
    if cls == "seq":
        assert not lad.any() and not ladi.any()      # exactly zero
    else:
        compare(tag, "logabsdet", lad[:1].cpu().numpy(), g["lad"], truth(g, "lad"), LAD_TOL)
        compare(tag, "logabsdet(inverse)", ladi[:1].cpu().numpy(), g["ladi"], truth(g, "ladi"), LAD_TOL)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", LINEAR_CASES, ids=case_id)
def test_parity_in_cached_eval_mode(case, kind):
    cls, features, count = case
    g = golden(cls, features, count, kind)
    x, _ = case_inputs(cls, features, count, kind)
    t = layer_of(g, cls, features, count).to(DEV).eval()
    t.use_cache(True)
    tag = "householder %s D=%d K=%d %s eval_cached" % (cls, features, count, kind)
    lad, ladi = check_both_directions(t, g, x, tag, "_cached")
    compare(tag, "logabsdet", lad[:1].cpu().numpy(), g["lad_cached"], truth(g, "lad"), LAD_TOL)
    compare(tag, "logabsdet(inverse)", ladi[:1].cpu().numpy(), g["ladi_cached"], truth(g, "ladi"), LAD_TOL)
    assert t.cache.weight.shape == t.cache.inverse.shape == (features, features) and t.cache.logabsdet.dim() == 0
    t.train()
    assert t.cache.weight is None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_round_trip_like_the_reference(case, kind):
    """inverse(forward(x)) against x: the reference's own float32 round trip (its inverse of ITS forward output, both
    in the fixture) is the yardstick."""
    cls, features, count = case
    g = golden(cls, features, count, kind)
    x, _ = case_inputs(cls, features, count, kind)
    t = layer_of(g, cls, features, count).to(DEV)
    with torch.no_grad():
        y, lad = t(dev(x))
        back, ladi = t.inverse(y)
    assert torch.equal(lad, -ladi)
    compare("householder %s D=%d K=%d %s" % (cls, features, count, kind), "round trip", back.cpu().numpy(), g["xi"],
            x.astype(np.float64), OUT_TOL)


def run_gradients(t, g, source, r, inverse):
    t.zero_grad()
    xin = dev(source).requires_grad_(True)
    out, lad = t.inverse(xin) if inverse else t(xin)
    ((out * dev(r)).sum() + lad.sum()).backward()
    return xin.grad, {n: p.grad for n, p in t.named_parameters()}


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_gradients(case, kind, inverse):
    """Gradients of sum(out * r) + sum(logabsdet) in both directions (the inverse at the reference's float32 forward
    output) with respect to the inputs and every parameter, against the reference's float64 autograd with its float32
    autograd as the yardstick; the parameter gradients bit-identical between two runs."""
    cls, features, count = case
    g = golden(cls, features, count, kind)
    x, r = case_inputs(cls, features, count, kind)
    t = layer_of(g, cls, features, count).to(DEV)
    source = g["y"] if inverse else x
    g_in, g_params = run_gradients(t, g, source, r, inverse)
    tag = "householder %s D=%d K=%d %s %s" % (cls, features, count, kind, "inverse" if inverse else "forward")
    pre = "gradinv/" if inverse else "grad/"
    compare(tag, "grad inputs", g_in.cpu().numpy(), g[pre + "inputs"], truth(g, pre + "inputs"), OUT_TOL)
    for n, v in g_params.items():
        compare(tag, "grad " + n, v.cpu().numpy(), g[pre + n], truth(g, pre + n), OUT_TOL)
    again_in, again = run_gradients(t, g, source, r, inverse)
    assert torch.equal(again_in, g_in)
    for n, v in g_params.items():
        assert torch.equal(again[n], v), n


@pytest.mark.parametrize("case", [("seq", 2, 2), ("seq", 5, 3), ("svd", 2, 2), ("svd", 5, 4), ("svd", 16, 10),
                                  ("svd", 100, 100), ("svd", 128, 128), ("seq", 128, 128)], ids=case_id)
def test_identity_initialisation_passes_through_exactly(case):
    cls, features, count = case
    t = new_layer(cls, features, count).to(DEV)
    x = torch.randn(777, features, device=DEV)
    with torch.no_grad():
        y, lad = t(x)
        back, ladi = t.inverse(x)
    if cls == "seq" and count % 2:
        x = x.clone()
        x[:, count // 2] *= -1          # the unpaired last reflection flips one coordinate, exactly
    assert torch.equal(y, x) and torch.equal(back, x)
    if cls == "seq":
        assert not lad.any() and not ladi.any()
    else:    # SVDLinear's own rounding of sum log d: d is the float32 nearest to eps + softplus(logit)
        want = float(torch.log(torch.nn.functional.softplus(t.unconstrained_diagonal.detach().double()) + t.eps).sum())
        assert rows_equal(lad) and abs(float(lad[0]) - want) <= 1e-7 * max(1.0, abs(want)) + 1e-12
        assert torch.equal(lad, -ladi) and abs(float(lad[0])) < features * 6e-8


def random_layer(cls, features, count, seed=0):
    torch.manual_seed(seed)
    t = new_layer(cls, features, count)
    with torch.no_grad():
        for n, p in t.named_parameters():
            if n.endswith("q_vectors") or n == "bias":
                p.normal_()
            elif n == "unconstrained_diagonal":
                p.add_(0.5 * torch.randn_like(p))
    return t.to(DEV)


@pytest.mark.parametrize("case", [("seq", 5, 3), ("svd", 5, 4), ("qr", 5, 3), ("seq", 64, 40), ("svd", 64, 10),
                                  ("qr", 64, 10), ("svd", 128, 34), ("qr", 128, 128)], ids=case_id)
def test_rows_do_not_depend_on_the_batch(case):
    t = random_layer(*case, seed=4)
    features = case[1]
    x = torch.randn(1500, features, device=DEV)
    with torch.no_grad():
        y, lad = t(x)
        xi, _ = t.inverse(x)
        for rows in (1, 5, 63, 65, 257):
            ys, lads = t(x[:rows].clone())
            xs, _ = t.inverse(x[:rows].clone())
            assert torch.equal(ys, y[:rows]) and torch.equal(xs, xi[:rows]) and torch.equal(lads, lad[:rows]), rows
        tail, _ = t(x[1400:1405].clone())
        assert torch.equal(tail, y[1400:1405])
        empty, lad0 = t(x[:0])
        assert empty.shape == (0, features) and lad0.shape == (0,)
        empty, lad0 = t.inverse(x[:0])
        assert empty.shape == (0, features) and lad0.shape == (0,)


def test_a_zero_q_vector_gives_the_reference_s_non_finite_pattern():
    t = random_layer("seq", 5, 3, seed=2)
    t.q_vectors.data[1] = 0
    x = torch.randn(300, 5, device=DEV)
    with torch.no_grad():
        y, lad = t(x)
        t._use_kernel = False
        want, _ = t(x)             # the reference's op sequence: (2 / 0) * 0 = nan in every column
    assert torch.isnan(want).all() and torch.isnan(y).all() and not lad.any()


@pytest.mark.parametrize("cls", ["svd", "qr"])
def test_more_rows_than_one_pass_of_the_grid(cls):
    """The persistent loop: the planner's grid is at most 8 workgroups per CU of at most 256 rows (forward) and of 64
    rows (backward, `nfa_householder_backward_slabs`), so this row count gives every workgroup a second tile and leaves
    a tail.  Forward and gradients against the same rows run in small separate calls, bit for bit."""
    from nflows_amd import _native as N
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = cus * 8 * 256 + 77
    assert N.load().nfa_householder_backward_slabs(rows, 5, 4, 4) * 64 < rows
    t = random_layer(cls, 5, 4 if cls == "svd" else 3, seed=9)
    x = torch.randn(rows, 5, device=DEV)
    picks = [slice(0, 300), slice(rows // 2 + 11, rows // 2 + 411), slice(rows - 200, rows)]
    with torch.no_grad():
        y, lad = t(x)
        xi, _ = t.inverse(x)
        for s in picks:
            ys, _ = t(x[s].clone())
            xs, _ = t.inverse(x[s].clone())
            assert torch.equal(ys, y[s]) and torch.equal(xs, xi[s])
    assert rows_equal(lad)
    xin = x.clone().requires_grad_(True)
    out, lad = t(xin)
    w = torch.randn(5, device=DEV)
    ((out * w).sum() + lad.sum()).backward()
    big = {n: p.grad.clone() for n, p in t.named_parameters()}
    for s in picks:
        t.zero_grad()
        xs = x[s].clone().requires_grad_(True)
        outs, _ = t(xs)
        (outs * w).sum().backward()
        assert torch.equal(xs.grad, xin.grad[s])
    t64 = copy.deepcopy(t).double()
    t64.zero_grad()
    out64, lad64 = t64(x.double())
    ((out64 * w.double()).sum() + lad64.sum()).backward()
    for n, p in t64.named_parameters():     # a sum over half a million rows: float64 on both sides, rounded once here
        scale = float(p.grad.abs().max())
        assert torch.allclose(big[n].double(), p.grad, rtol=1e-5, atol=1e-6 * scale), n


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [("seq", 5, 3), ("seq", 64, 10), ("svd", 5, 4), ("svd", 64, 10), ("qr", 5, 3),
                                  ("qr", 64, 10)], ids=case_id)
def test_generic_path_parity(case, kind):
    """`_use_kernel = False` and float64 inputs: the reference's sequence on stock device ops, same rule, same fixtures."""
    cls, features, count = case
    g = golden(cls, features, count, kind)
    x, _ = case_inputs(cls, features, count, kind)
    t = layer_of(g, cls, features, count).to(DEV)
    t._use_kernel = False
    for m in t.modules():
        m._use_kernel = False
    tag = "householder generic %s D=%d K=%d %s" % (cls, features, count, kind)
    check_both_directions(t, g, x, tag)
    t64 = layer_of(g, cls, features, count).to(DEV).double()
    with torch.no_grad():
        y64, lad64 = t64(dev(x).double())
    assert y64.dtype == torch.float64
    compare(tag + " float64", "y", y64.float().cpu().numpy(), g["y"], truth(g, "y"), OUT_TOL)
    if cls != "seq":
        compare(tag + " float64", "logabsdet", lad64[:1].float().cpu().numpy(), g["lad"], truth(g, "lad"), LAD_TOL)


@pytest.mark.parametrize("cls", ["seq", "svd", "qr"])
def test_other_ranks_and_sizes_take_the_generic_path(cls):
    t = random_layer(cls, 6, 4, seed=7)
    x = torch.randn(4, 3, 6, device=DEV)
    with torch.no_grad():
        y, lad = t(x.reshape(12, 6))
        y3, lad3 = t(x)
        back3, _ = t.inverse(y3)
    assert y3.shape == (4, 3, 6) and lad3.shape == (4,) and torch.allclose(y3.reshape(12, 6), y, atol=1e-5)
    assert torch.allclose(back3, x, atol=1e-4)
    wide = random_layer(cls, 130, 4, seed=8)       # past the kernel's 128 features
    xw = torch.randn(50, 130, device=DEV)
    with torch.no_grad():
        yw, ladw = wide(xw)
        backw, _ = wide.inverse(yw)
        y64, lad64 = copy.deepcopy(wide).double()(xw.double())
    assert torch.allclose(yw.double(), y64, atol=1e-4) and torch.allclose(backw, xw, atol=1e-3)
    assert abs(float(ladw[0]) - float(lad64[0])) < 1e-4
    xw.requires_grad_(True)
    out, ladw = wide(xw)
    (out.sum() + ladw.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in wide.parameters())


@pytest.mark.parametrize("cls", ["seq", "svd", "qr"])
def test_parameter_writes_are_seen_by_the_next_call(cls):
    t = random_layer(cls, 64, 10, seed=5)
    x = torch.randn(512, 64, device=DEV)

    def fresh_copy():
        f = new_layer(cls, 64, 10).to(DEV)
        f.load_state_dict(t.state_dict())
        return f

    with torch.no_grad():
        before, _ = t(x)
    for p in t.parameters():
        p.data[..., 7] += 0.25
    with torch.no_grad():
        after, lad = t(x)
        want, want_lad = fresh_copy()(x)
    assert not torch.equal(after, before) and torch.equal(after, want) and torch.equal(lad, want_lad)
    opt = torch.optim.SGD(t.parameters(), lr=0.05)
    y, lad = t(x)
    (-(lad.mean()) + (y ** 3).mean()).backward()     # (not y ** 2: a rotation keeps the norm, no gradient there)
    opt.step()
    with torch.no_grad():
        stepped, lad = t(x)
        want, want_lad = fresh_copy()(x)
        inv, _ = t.inverse(x)
        want_inv, _ = fresh_copy().inverse(x)
    assert not torch.equal(stepped, after) and torch.equal(stepped, want) and torch.equal(lad, want_lad)
    assert torch.equal(inv, want_inv)


@pytest.mark.parametrize("features", [5, 64])
@pytest.mark.parametrize("mode", ["train", "eval_cached"])
def test_naive_linear_parity(features, mode):
    from nflows_amd.transforms import NaiveLinear
    g = naive_golden(features)
    x, _ = case_inputs("naive", features, 0, "trained")
    t = NaiveLinear(features)
    t.load_state_dict(state_of(g), strict=True)
    t = t.to(DEV)
    suffix = ""
    if mode == "eval_cached":
        t.eval()
        t.use_cache(True)
        suffix = "_cached"
    tag = "naive_linear D=%d %s" % (features, mode)
    lad, ladi = check_both_directions(t, g, x, tag, suffix)
    compare(tag, "logabsdet", lad[:1].cpu().numpy(), g["lad" + suffix], truth(g, "lad"), LAD_TOL)
    compare(tag, "logabsdet(inverse)", ladi[:1].cpu().numpy(), g["ladi" + suffix], truth(g, "ladi"), LAD_TOL)


def build_flow(features=16, hidden=32, count=10):
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms import (CompositeTransform, PiecewiseRationalQuadraticCouplingTransform, QRLinear,
                                       RandomPermutation, SVDLinear)
    from nflows_amd.utils.torchutils import create_alternating_binary_mask
    ts = []
    for i in range(4):
        ts.append(RandomPermutation(features))
        ts.append(SVDLinear(features, count) if i < 2 else QRLinear(features, count))
        ts.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=create_alternating_binary_mask(features, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=hidden, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=3.0))
    return Flow(CompositeTransform(ts), StandardNormal([features]))


def test_flow_with_svd_and_qr_layers_matches_the_reference_samples_and_trains():
    import nflows_amd
    g = np.load(os.path.join(GOLDEN, "hh_flow.npz"))
    flow = build_flow()
    state = {k[len("state/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}
    assert sorted(state) == sorted(flow.state_dict())
    flow.load_state_dict(state, strict=True)
    flow = flow.to(DEV).eval()
    x = dev(g["x"])
    with torch.no_grad():
        lp = flow.log_prob(x)
        z, lad = flow._transform(x)
        xs, ladi = flow._transform.inverse(dev(g["z"]))
    nflows_amd.check_status()
    tag = "hh_flow"
    compare(tag, "log_prob", lp.cpu().numpy(), g["log_prob"], truth(g, "log_prob"), LAD_TOL)
    compare(tag, "z", z.cpu().numpy(), g["z"], truth(g, "z"), OUT_TOL)
    compare(tag, "logabsdet", lad.cpu().numpy(), g["lad"], truth(g, "lad"), LAD_TOL)
    compare(tag, "x from z", xs.cpu().numpy(), g["x_from_z"], truth(g, "x_from_z"), OUT_TOL)
    compare(tag, "logabsdet(inverse)", ladi.cpu().numpy(), g["ladi"], truth(g, "ladi"), LAD_TOL)
    from nflows_amd import ops
    calls = []

    class Hook:
        def begin(self, name):
            calls.append(name)

        def end(self, token, nbytes):
            pass

    ops.set_launch_hook(Hook())
    try:
        with torch.no_grad():
            flow._transform(x)
    finally:
        ops.set_launch_hook(None)
    assert calls.count("householder") == 4, calls        # one K24 launch per linear layer
    # Flow.sample round trip: samples go back to noise and forward again to themselves
    with torch.no_grad():
        torch.manual_seed(0)
        samples = flow.sample(256)
        noise, _ = flow._transform(samples)
        again, _ = flow._transform.inverse(noise)
    nflows_amd.check_status()
    assert samples.shape == (256, 16) and torch.isfinite(samples).all()
    assert torch.allclose(again, samples, atol=2e-4)
    # one Adam step of the maximum-likelihood loss moves every parameter of the four linear layers
    flow.train()
    names = ("q_vectors", "unconstrained_diagonal", "upper_entries", "log_upper_diag", "bias")
    linear = {n: p for n, p in flow.named_parameters() if n.split(".")[-1] in names and "transform_net" not in n}
    assert len(linear) == 2 * 4 + 2 * 4
    before = {n: p.detach().clone() for n, p in linear.items()}
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    loss = -flow.log_prob(x).mean()
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    for n, p in linear.items():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[n]), n
