"""K16 (LULinear) on the GPU against the reference's float32 / float64 results (tests/golden/lu_linear_d*_*.npz,
lu_flow.npz; written by tests/golden/make_golden_lu.py) under the project's parity rule -- `compare()` of
tests/test_gpu_headline_parity.py: error against float64 at most 2 x the reference-float32's own on maximum (+ four
ulps), mean and 99.9 % quantile -- and the properties of the kernel that are exact."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import LAD_TOL, OUT_TOL
from test_gpu_headline_parity import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = ("lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")
ROWS = {2: 4096, 5: 4096, 64: 1280, 100: 800, 128: 640}
FEATURES = sorted(ROWS)
KINDS = ("rand", "trained")


def golden(features):
    """All parts of both parameter sets of one D, merged (tests/golden/lu_linear_d{D}_{kind}_{part}.npz)."""
    import glob
    merged = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "lu_linear_d%d_*.npz" % features))):
        with np.load(path) as z:
            merged.update({k: z[k] for k in z.files})
    assert merged, "no fixture for %d features" % features
    return merged


def inputs_of(features, kind):
    """The generator's inputs and loss weights, from the same seeds."""
    rng = np.random.RandomState(1000 * features + (1 if kind == "rand" else 2))
    x = rng.randn(ROWS[features], features).astype(np.float32)
    r = rng.randn(ROWS[features], features).astype(np.float32)
    return x, r


def truth(g, name):
    return g[name].astype(np.float64) + g[name + "_d"].astype(np.float64)


def layer_of(g, features, kind, **kw):
    from nflows_amd.transforms import LULinear
    t = LULinear(features, **kw)
    t.load_state_dict({n: torch.from_numpy(g["%s/%s" % (kind, n)]) for n in PARAMS})
    return t.to(DEV)


def random_layer(features, seed=0):
    from nflows_amd.transforms import LULinear
    torch.manual_seed(seed)
    t = LULinear(features, identity_init=False)
    with torch.no_grad():
        t.bias.normal_()
    return t.to(DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rows_equal(lad):
    return bool((lad == lad[0]).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("features", FEATURES)
@pytest.mark.parametrize("mode", ["train", "eval_cached"])
def test_parity_both_directions(features, kind, mode):
    g = golden(features)
    x, _ = inputs_of(features, kind)
    t = layer_of(g, features, kind)
    pre = kind + "/"
    if mode == "eval_cached":
        t.eval()
        t.use_cache(True)
    suffix = "_cached" if mode == "eval_cached" else ""
    tag = "lu_linear D=%d %s %s" % (features, kind, mode)
    with torch.no_grad():
        y, lad = t(dev(x))
        xi, ladi = t.inverse(dev(g[pre + "y"]))
    assert y.shape == (x.shape[0], features) and lad.shape == (x.shape[0],) and rows_equal(lad) and rows_equal(ladi)
    compare(tag, "y", y.cpu().numpy(), g[pre + "y" + suffix], truth(g, pre + "y"), OUT_TOL)
    compare(tag, "x", xi.cpu().numpy(), g[pre + "xi" + suffix], truth(g, pre + "xi"), OUT_TOL)
    compare(tag, "logabsdet", lad[:1].cpu().numpy(), g[pre + "lad" + suffix], truth(g, pre + "lad"), LAD_TOL)
    compare(tag, "logabsdet(inverse)", ladi[:1].cpu().numpy(), g[pre + "ladi" + suffix], truth(g, pre + "ladi"), LAD_TOL)
    if mode == "eval_cached":   # the reference's methods still fill the cache
        t._check_forward_cache()
        t._check_inverse_cache()
        assert t.cache.weight.shape == t.cache.inverse.shape == (features, features) and t.cache.logabsdet.dim() == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("features", FEATURES)
def test_round_trip_like_the_reference(features, kind):
    """inverse(forward(x)) against x: the reference's own float32 round trip (its inverse of ITS forward output, both
    in the fixture) is the yardstick."""
    g = golden(features)
    x, _ = inputs_of(features, kind)
    t = layer_of(g, features, kind)
    with torch.no_grad():
        y, lad = t(dev(x))
        back, ladi = t.inverse(y)
    assert torch.equal(lad, -ladi)
    compare("lu_linear D=%d %s" % (features, kind), "round trip", back.cpu().numpy(), g[kind + "/xi"], x.astype(np.float64), OUT_TOL)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("features", FEATURES)
def test_gradients(features, kind):
    g = golden(features)
    x, r = inputs_of(features, kind)
    t = layer_of(g, features, kind)
    xin = dev(x).requires_grad_(True)
    y, lad = t(xin)
    ((y * dev(r)).sum() + lad.sum()).backward()
    tag = "lu_linear D=%d %s" % (features, kind)
    pre = kind + "/grad_"
    compare(tag, "grad inputs", xin.grad.cpu().numpy(), g[pre + "inputs"], truth(g, pre + "inputs"), OUT_TOL)
    for n in PARAMS:
        compare(tag, "grad " + n, getattr(t, n).grad.cpu().numpy(), g[pre + n], truth(g, pre + n), OUT_TOL)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("features", FEATURES)
def test_inverse_direction_gradients(features, kind):
    """Gradients of sum(x * r) + sum(logabsdet) through `inverse` at the reference's float32 forward output, with respect
    to that input and all four parameters, against the reference's float64 autograd (its float32 autograd the yardstick)."""
    g = golden(features)
    _, r = inputs_of(features, kind)
    t = layer_of(g, features, kind)
    yin = dev(g[kind + "/y"]).requires_grad_(True)
    x, ladi = t.inverse(yin)
    ((x * dev(r)).sum() + ladi.sum()).backward()
    tag = "lu_linear D=%d %s inverse" % (features, kind)
    pre = kind + "/gradinv_"
    compare(tag, "grad inputs", yin.grad.cpu().numpy(), g[pre + "inputs"], truth(g, pre + "inputs"), OUT_TOL)
    for n in PARAMS:
        compare(tag, "grad " + n, getattr(t, n).grad.cpu().numpy(), g[pre + n], truth(g, pre + n), OUT_TOL)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("features", [5, 64, 128])
def test_gradients_through_a_fused_permutation_equal_permuting_outside(features, inverse):
    """in_perm (forward) / out_scatter (inverse) inside the kernels and their transposes in the backward: every gradient
    equals, bit for bit, the one obtained with the permutation applied by index_select outside the layer."""
    from nflows_amd import ops
    torch.manual_seed(features)
    perm = torch.randperm(features, device=DEV)
    x0 = torch.randn(300, features, device=DEV)
    r = torch.randn(300, features, device=DEV)
    results = []
    for fused in (True, False):
        t = random_layer(features, seed=8)
        p = (t.lower_entries, t.upper_entries, t.unconstrained_upper_diag, t.bias)
        x = x0.clone().requires_grad_(True)
        if not inverse:
            y, lad = ops.lu_linear(x, *p, in_perm=perm) if fused else ops.lu_linear(x.index_select(1, perm), *p)
        elif fused:
            y, lad = ops.lu_linear(x, *p, inverse=True, out_scatter=perm)
        else:
            v, lad = ops.lu_linear(x, *p, inverse=True)
            y = v.index_select(1, torch.argsort(perm))     # y[:, perm[j]] = v[:, j]
        ((y * r).sum() + 0.5 * lad.sum()).backward()
        results.append([y.detach(), x.grad] + [q.grad for q in p])
    for name, a, b in zip(("outputs", "grad inputs") + PARAMS, *results):
        assert torch.equal(a, b), name
    assert results[0][1].abs().sum() > 0 and all(torch.isfinite(v).all() for v in results[0])


@pytest.mark.parametrize("features", [2, 5, 16, 64, 100, 128])
def test_identity_factors_pass_through_exactly(features):
    """L = I, off-diagonal U = 0: y = diag * x + b and x = (y - b) / diag to the last bit; the diagonal is the
    correctly rounded softplus(logit) + eps (float64, rounded once)."""
    from nflows_amd.transforms import LULinear
    torch.manual_seed(features)
    t = LULinear(features, identity_init=True)
    with torch.no_grad():
        t.unconstrained_upper_diag.add_(0.5 * torch.randn(features))
        t.bias.normal_()
    t = t.to(DEV)
    diag = (torch.nn.functional.softplus(t.unconstrained_upper_diag.detach().double()) + t.eps).float()
    x = torch.randn(777, features, device=DEV)
    with torch.no_grad():
        y, lad = t(x)
        back, _ = t.inverse(x)
    assert torch.equal(y, x * diag + t.bias)
    assert torch.equal(back, (x - t.bias) / diag)
    want = torch.log(torch.nn.functional.softplus(t.unconstrained_upper_diag.detach().double()) + t.eps).sum().float()
    assert rows_equal(lad) and abs(float(lad[0]) - float(want)) <= 1.2e-7 * abs(float(want))


@pytest.mark.parametrize("features", [5, 64, 128])
def test_fused_permutation_and_accumulate_are_exact(features):
    from nflows_amd import ops
    t = random_layer(features, seed=1)
    p = (t.lower_entries, t.upper_entries, t.unconstrained_upper_diag, t.bias)
    torch.manual_seed(2)
    perm = torch.randperm(features, device=DEV)
    x = torch.randn(1000, features, device=DEV)
    running = torch.randn(1000, device=DEV)
    with torch.no_grad():
        y, lad = ops.lu_linear(x.index_select(1, perm), *p)
        y_fused, lad_fused = ops.lu_linear(x, *p, in_perm=perm)
        assert torch.equal(y, y_fused) and torch.equal(lad, lad_fused)
        acc = running.clone()
        y_acc, out = ops.lu_linear(x, *p, in_perm=perm, accumulate_into=acc)
        assert out is acc and torch.equal(y_acc, y) and torch.equal(acc, running + lad)
        v, ladi = ops.lu_linear(x, *p, inverse=True)
        scattered = torch.empty_like(v)
        scattered[:, perm] = v
        v_fused, ladi_fused = ops.lu_linear(x, *p, inverse=True, out_scatter=perm)
        assert torch.equal(v_fused, scattered) and torch.equal(ladi, ladi_fused)
        acc = running.clone()
        ops.lu_linear(x, *p, inverse=True, out_scatter=perm, accumulate_into=acc)
        assert torch.equal(acc, running + ladi)


@pytest.mark.parametrize("features", [5, 64, 128])
def test_rows_do_not_depend_on_the_batch(features):
    t = random_layer(features, seed=4)
    x = torch.randn(4096, features, device=DEV)
    with torch.no_grad():
        y, lad = t(x)
        xi, _ = t.inverse(x)
        for rows in (1, 5, 63, 65, 257):
            ys, lads = t(x[:rows].clone())
            xs, _ = t.inverse(x[:rows].clone())
            assert torch.equal(ys, y[:rows]) and torch.equal(xs, xi[:rows]) and torch.equal(lads, lad[:rows]), rows
        tail, _ = t(x[4000:4005].clone())
        assert torch.equal(tail, y[4000:4005])
        empty, lad0 = t(x[:0])
        assert empty.shape == (0, features) and lad0.shape == (0,)


def test_parameter_writes_are_seen_by_the_next_call():
    from nflows_amd.transforms import LULinear
    t = random_layer(64, seed=5)
    x = torch.randn(512, 64, device=DEV)

    def fresh_copy():
        f = LULinear(64).to(DEV)
        f.load_state_dict(t.state_dict())
        return f

    with torch.no_grad():
        before, _ = t(x)
    t.lower_entries.data[7] += 0.25
    t.unconstrained_upper_diag.data.mul_(1.5)
    with torch.no_grad():
        after, lad = t(x)
        want, want_lad = fresh_copy()(x)
    assert not torch.equal(after, before) and torch.equal(after, want) and torch.equal(lad, want_lad)
    opt = torch.optim.SGD(t.parameters(), lr=0.1)
    y, lad = t(x)
    (-(lad.mean()) + (y ** 2).mean()).backward()
    opt.step()
    with torch.no_grad():
        stepped, lad = t(x)
        want, want_lad = fresh_copy()(x)
        inv, _ = t.inverse(x)
        want_inv, _ = fresh_copy().inverse(x)
    assert not torch.equal(stepped, after) and torch.equal(stepped, want) and torch.equal(lad, want_lad)
    assert torch.equal(inv, want_inv)


def build_flow(features=16, hidden=32, layers=4):
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms import (CompositeTransform, LULinear, PiecewiseRationalQuadraticCouplingTransform,
                                       RandomPermutation)
    from nflows_amd.utils.torchutils import create_alternating_binary_mask
    ts = []
    for i in range(layers):
        ts.append(RandomPermutation(features))
        ts.append(LULinear(features, identity_init=True))
        ts.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=create_alternating_binary_mask(features, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=hidden, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=3.0))
    return Flow(CompositeTransform(ts), StandardNormal([features]))


def test_nsf_style_flow_matches_the_reference_and_trains():
    import nflows_amd
    g = np.load(os.path.join(GOLDEN, "lu_flow.npz"))
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
    tag = "nsf_lu_flow"
    compare(tag, "log_prob", lp.cpu().numpy(), g["log_prob"], truth(g, "log_prob"), LAD_TOL)
    compare(tag, "z", z.cpu().numpy(), g["z"], truth(g, "z"), OUT_TOL)
    compare(tag, "logabsdet", lad.cpu().numpy(), g["lad"], truth(g, "lad"), LAD_TOL)
    compare(tag, "x from z", xs.cpu().numpy(), g["x_from_z"], truth(g, "x_from_z"), OUT_TOL)
    compare(tag, "logabsdet(inverse)", ladi.cpu().numpy(), g["ladi"], truth(g, "ladi"), LAD_TOL)
    # the permutation in front of every LU layer is folded into its launch: one K16 per [RandomPermutation, LULinear]
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
    assert calls.count("lu_linear") == 4 and "permute_cols" not in calls, calls
    # one Adam step of the maximum-likelihood loss moves every LU parameter
    flow.train()
    lu_params = {n: p for n, p in flow.named_parameters()
                 if n.split(".")[-1] in PARAMS and "transform_net" not in n}
    assert len(lu_params) == 16
    before = {n: p.detach().clone() for n, p in lu_params.items()}
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    loss = -flow.log_prob(x).mean()
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    for n, p in lu_params.items():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[n]), n


# ---------------------------------------------------------------------------------------------------------------------
# the properties the reference's own LU test asserts, in this project's words
@pytest.mark.parametrize("features", [3, 20, 128])
def test_shapes_inverses_and_determinant(features):
    t = random_layer(features, seed=6)
    x = torch.randn(10, features, device=DEV)
    eye = torch.eye(features, device=DEV)
    for cached in (False, True):
        t.train()
        if cached:
            t.eval()
            t.use_cache(True)
        with torch.no_grad():
            y, lad = t(x)
            back, ladi = t.inverse(y)
            w, wi = t.weight(), t.weight_inverse()
        assert y.shape == (10, features) and lad.shape == (10,) and back.shape == (10, features) and ladi.shape == (10,)
        assert torch.allclose(back, x, atol=1e-4) and torch.allclose(lad + ladi, torch.zeros(10, device=DEV), atol=1e-6)
        assert torch.allclose(y, x @ w.t() + t.bias, atol=1e-4)
        assert torch.allclose(w @ wi, eye, atol=1e-4) and torch.allclose(wi @ w, eye, atol=1e-4)
        sign, slog = torch.linalg.slogdet(w.double())
        assert sign == 1 and abs(float(slog) - float(lad[0])) < 1e-4 and abs(float(t.logabsdet()) - float(lad[0])) < 1e-5


def test_float64_and_other_ranks_take_the_generic_device_path():
    t = random_layer(6, seed=7)
    x = torch.randn(4, 3, 6, device=DEV)
    with torch.no_grad():
        y, lad = t(x.reshape(12, 6))
        y3, lad3 = t(x)
        back3, _ = t.inverse(y3)
        t64 = copy.deepcopy(t).double()
        y64, lad64 = t64(x.reshape(12, 6).double())
    assert y3.shape == (4, 3, 6) and lad3.shape == (4,) and torch.allclose(y3.reshape(12, 6), y, atol=1e-5)
    assert torch.allclose(back3, x, atol=1e-4)
    assert y64.dtype == torch.float64 and torch.allclose(y64.float(), y, atol=1e-5) and abs(float(lad64[0]) - float(lad[0])) < 1e-5
