"""K17 (BatchNorm, ActNorm) and the two flow factories on the GPU against the reference's float32 / float64 results
(tests/golden/norm_*.npz, written by tests/golden/make_golden_norm.py) under the project's parity rule -- `compare()` of
tests/test_gpu_headline_parity.py with OUT_TOL / LAD_TOL of tests/helpers.py: error against float64 at most 2 x the
reference-float32's own on maximum (+ four ulps), mean and 99.9 % quantile -- and the properties of the kernels that are
exact."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

from helpers import LAD_TOL, OUT_TOL
from test_gpu_headline_parity import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = {2: 4096, 5: 4096, 64: 1280, 100: 800, 128: 640}
FEATURES = sorted(ROWS)


def golden(stem, features):
    merged = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "norm_%s_d%d_*.npz" % (stem, features)))):
        with np.load(path) as z:
            merged.update({k: z[k] for k in z.files})
    assert merged, "no fixture for %s, %d features" % (stem, features)
    return merged


def norm_inputs(features, batch, rows=None):
    """The generator's inputs and loss weights, from the same seeds (tests/golden/make_golden_norm.py: norm_inputs)."""
    rng = np.random.RandomState(5000 * features + batch)
    rows = ROWS[features] if rows is None else rows
    offset = rng.uniform(-3.0, 3.0, size=features)
    spread = np.exp(rng.uniform(np.log(0.2), np.log(5.0), size=features))
    x = (offset + spread * rng.randn(rows, features)).astype(np.float32)
    r = rng.randn(rows, features).astype(np.float32)
    return x, r


def truth(g, name):
    return g[name].astype(np.float64) + g[name + "_d"].astype(np.float64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rows_equal(lad):
    return bool((lad == lad[0]).all())


def batch_norm_of(g, features, buffers=None):
    from nflows_amd.transforms import BatchNorm
    t = BatchNorm(features)
    state = {"unconstrained_weight": torch.from_numpy(g["unconstrained_weight"]), "bias": torch.from_numpy(g["bias"]),
             "running_mean": torch.zeros(features), "running_var": torch.zeros(features)}
    if buffers is not None:
        state["running_mean"] = torch.from_numpy(g[buffers + "running_mean"])
        state["running_var"] = torch.from_numpy(g[buffers + "running_var"])
    t.load_state_dict(state)
    return t.to(DEV)


def random_batch_norm(features, seed=0):
    from nflows_amd.transforms import BatchNorm
    torch.manual_seed(seed)
    t = BatchNorm(features)
    with torch.no_grad():
        t.unconstrained_weight.add_(0.5 * torch.randn(features))
        t.bias.normal_()
        t.running_mean.normal_()
        t.running_var.uniform_(0.1, 4.0)
    return t.to(DEV)


def random_act_norm(features, seed=0):
    from nflows_amd.transforms import ActNorm
    torch.manual_seed(seed)
    t = ActNorm(features)
    with torch.no_grad():
        t.log_scale.normal_(0.0, 0.5)
        t.shift.normal_()
        t.initialized.fill_(True)
    return t.to(DEV)


# ------------------------------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("features", FEATURES)
def test_batch_norm_training_forward_and_running_buffers(features):
    g = golden("bn", features)
    t = batch_norm_of(g, features).train()
    tag = "batch_norm D=%d train" % features
    with torch.no_grad():
        for b in range(3):
            y, lad = t(dev(norm_inputs(features, b)[0]))
            if b == 0:
                assert y.shape == (ROWS[features], features) and lad.shape == (ROWS[features],) and rows_equal(lad)
                compare(tag, "y", y.cpu().numpy(), g["train_y"], truth(g, "train_y"), OUT_TOL)
                compare(tag, "logabsdet", lad[:1].cpu().numpy(), g["train_lad"], truth(g, "train_lad"), LAD_TOL)
            if b in (0, 2):
                pre = "after%d_" % (b + 1)
                for n in ("running_mean", "running_var"):
                    compare(tag, pre + n, getattr(t, n).cpu().numpy(), g[pre + n], truth(g, pre + n), OUT_TOL)


@pytest.mark.parametrize("features", FEATURES)
def test_batch_norm_eval_forward_inverse_and_round_trip(features):
    g = golden("bn", features)
    t = batch_norm_of(g, features, "after3_").eval()
    x, _ = norm_inputs(features, 0)
    tag = "batch_norm D=%d eval" % features
    with torch.no_grad():
        y, lad = t(dev(x))
        xi, ladi = t.inverse(dev(g["eval_y"]))
        back, ladb = t.inverse(y)
    assert rows_equal(lad) and rows_equal(ladi) and torch.equal(lad, -ladb)
    compare(tag, "y", y.cpu().numpy(), g["eval_y"], truth(g, "eval_y"), OUT_TOL)
    compare(tag, "logabsdet", lad[:1].cpu().numpy(), g["eval_lad"], truth(g, "eval_lad"), LAD_TOL)
    compare(tag, "x", xi.cpu().numpy(), g["inv_x"], truth(g, "inv_x"), OUT_TOL)
    compare(tag, "logabsdet(inverse)", ladi[:1].cpu().numpy(), g["inv_lad"], truth(g, "inv_lad"), LAD_TOL)
    # the reference's own float32 round trip (its inverse of ITS forward output) is the yardstick of ours
    compare(tag, "round trip", back.cpu().numpy(), g["inv_x"], x.astype(np.float64), OUT_TOL)


@pytest.mark.parametrize("mode", ["gtrain", "geval", "ginv"])
@pytest.mark.parametrize("features", FEATURES)
def test_batch_norm_gradients(features, mode):
    """Gradients of sum(y * r) + sum(logabsdet) with respect to the inputs and both parameters: training mode (through the
    batch statistics), eval mode, and through the eval inverse at the reference's float32 eval output."""
    g = golden("bn", features)
    x, r = norm_inputs(features, 0)
    t = batch_norm_of(g, features, None if mode == "gtrain" else "after3_")
    t.train(mode == "gtrain")
    t._use_kernel = "always"     # K17's own backward (small differentiated passes take the generic path by default)
    xin = dev(g["eval_y"] if mode == "ginv" else x).requires_grad_(True)
    y, lad = t.inverse(xin) if mode == "ginv" else t(xin)
    ((y * dev(r)).sum() + lad.sum()).backward()
    tag = "batch_norm D=%d %s" % (features, mode)
    pre = mode + "_"
    compare(tag, "grad inputs", xin.grad.cpu().numpy(), g[pre + "inputs"], truth(g, pre + "inputs"), OUT_TOL)
    for n in ("unconstrained_weight", "bias"):
        compare(tag, "grad " + n, getattr(t, n).grad.cpu().numpy(), g[pre + n], truth(g, pre + n), OUT_TOL)


@pytest.mark.parametrize("features", FEATURES)
def test_act_norm_initialisation_forward_inverse_and_gradients(features):
    from nflows_amd.transforms import ActNorm
    g = golden("an", features)
    x, r = norm_inputs(features, 0)
    t = ActNorm(features).to(DEV).train()
    tag = "act_norm D=%d" % features
    with torch.no_grad():
        y, lad = t(dev(x))                      # initialises
        assert bool(t.initialized) and rows_equal(lad)
        xi, ladi = t.inverse(dev(g["fwd_y"]))
        back, _ = t.inverse(y)
    for n in ("log_scale", "shift"):
        compare(tag, n, getattr(t, n).detach().cpu().numpy(), g[n], truth(g, n), OUT_TOL)
    compare(tag, "y", y.cpu().numpy(), g["fwd_y"], truth(g, "fwd_y"), OUT_TOL)
    compare(tag, "logabsdet", lad[:1].cpu().numpy(), g["fwd_lad"], truth(g, "fwd_lad"), LAD_TOL)
    compare(tag, "x", xi.cpu().numpy(), g["inv_x"], truth(g, "inv_x"), OUT_TOL)
    compare(tag, "logabsdet(inverse)", ladi[:1].cpu().numpy(), g["inv_lad"], truth(g, "inv_lad"), LAD_TOL)
    compare(tag, "round trip", back.cpu().numpy(), g["inv_x"], x.astype(np.float64), OUT_TOL)
    # the gradients at the REFERENCE's initialised float32 state (a loaded checkpoint)
    t = ActNorm(features)
    t.load_state_dict({"log_scale": torch.from_numpy(g["log_scale"]), "shift": torch.from_numpy(g["shift"]),
                       "initialized": torch.tensor(True)})
    t = t.to(DEV)
    t._use_kernel = "always"     # K17's own backward
    for pre, source, call in (("gfwd_", x, t), ("ginv_", g["fwd_y"], t.inverse)):
        t.zero_grad()
        xin = dev(source).requires_grad_(True)
        out, ll = call(xin)
        ((out * dev(r)).sum() + ll.sum()).backward()
        compare(tag, pre + "inputs", xin.grad.cpu().numpy(), g[pre + "inputs"], truth(g, pre + "inputs"), OUT_TOL)
        for n in ("log_scale", "shift"):
            compare(tag, pre + n, getattr(t, n).grad.cpu().numpy(), g[pre + n], truth(g, pre + n), OUT_TOL)


# ------------------------------------------------------------------------------------------ exact properties
# the slab partition of the column reduction (csrc/norm.hip: norm_slabs; tests/test_normalization_host.py holds the formula):
# D = 5: 51 row lanes, 1 632 rows per slab -- one slab up to B = 1 632, two from 1 633;  D = 64: 4 row lanes, 128 rows per
# slab -- one slab up to B = 128, two from 129, the cap of 1 024 slabs from B = 131 072.
STAT_SHAPES = sorted(set(
    [(65, d) for d in (1, 2, 5, 64, 100, 128, 784, 1024)] + [(4097, d) for d in (1, 2, 5, 64, 100, 128, 784, 1024)]
    + [(b, d) for b in (2, 3, 63, 64, 65, 128, 129, 1632, 1633, 4097, 131073, 262144) for d in (5, 64)] + [(262144, 128)]))


def ulps_apart(got, want):
    """|got - want| in units of the float32 spacing at `want`."""
    want32 = want.float()
    spacing = torch.maximum((torch.nextafter(want32.abs(), torch.full_like(want32, float("inf"))) - want32.abs()),
                            torch.full_like(want32, 2.0 ** -149))
    return ((got.double() - want32.double()).abs() / spacing.double()).max().item()


@pytest.mark.parametrize("batch,features", STAT_SHAPES)
def test_column_statistics_are_the_rounded_float64_result(batch, features):
    from nflows_amd import _native as N
    from nflows_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(batch * 1031 + features)
    offset = torch.rand(features, device=DEV, generator=gen) * 6 - 3
    spread = torch.exp(torch.rand(features, device=DEV, generator=gen) * 3.2 - 1.6)
    x = offset + spread * torch.randn(batch, features, device=DEV, generator=gen)
    mean, var = ops.column_stats(x)
    again = ops.column_stats(x.clone())
    assert torch.equal(mean, again[0]) and torch.equal(var, again[1])           # the same bits on every run
    x64 = x.double()
    assert mean.shape == var.shape == (features,) and mean.dtype == var.dtype == torch.float32
    assert ulps_apart(mean, x64.mean(0)) <= 1.0, (batch, features, N.load().nfa_norm_slab_count(batch, features))
    assert ulps_apart(var, x64.var(0)) <= 1.0, (batch, features, N.load().nfa_norm_slab_count(batch, features))
    if batch <= 4097:
        g = torch.randn(batch, features, device=DEV, generator=gen)
        sums = ops.column_sums(g, x)
        assert torch.equal(sums, ops.column_sums(g.clone(), x.clone()))
        want = torch.stack((g.double().sum(0), (g.double() * x64).sum(0)))
        scale = torch.stack((g.double().abs().sum(0), (g.double() * x64).abs().sum(0)))
        assert bool(((sums - want).abs() <= 1e-13 * scale).all())


@pytest.mark.parametrize("features", [2, 4, 5, 16, 64, 784])
def test_results_are_bit_identical_and_rows_do_not_depend_on_the_batch(features):
    bn, an = random_batch_norm(features, seed=3).eval(), random_act_norm(features, seed=4).eval()
    x = torch.randn(4096, features, device=DEV)
    with torch.no_grad():
        for t in (bn, an):
            y, lad = t(x)
            xi, ladi = t.inverse(x)
            y2, lad2 = t(x.clone())
            assert torch.equal(y, y2) and torch.equal(lad, lad2)
            # rows of whole float4s take the float4 lanes, a (here: identity) permutation the scalar lanes: the same bits
            same = torch.arange(features, device=DEV)
            ys, lads = t(x, in_perm=same)
            xis, ladis = t.inverse(x, out_scatter=same)
            assert torch.equal(ys, y) and torch.equal(lads, lad) and torch.equal(xis, xi) and torch.equal(ladis, ladi)
            for rows in (1, 5, 63, 65, 257):
                ys, lads = t(x[:rows].clone())
                xs, ladis = t.inverse(x[:rows].clone())
                assert torch.equal(ys, y[:rows]) and torch.equal(lads, lad[:rows]), rows
                assert torch.equal(xs, xi[:rows]) and torch.equal(ladis, ladi[:rows]), rows
            tail, _ = t(x[4000:4005].clone())
            assert torch.equal(tail, y[4000:4005])
            empty, lad0 = t(x[:0])
            assert empty.shape == (0, features) and lad0.shape == (0,)
            empty, lad0 = t.inverse(x[:0])
            assert empty.shape == (0, features) and lad0.shape == (0,)
        bn.train()
        a = bn(x)
        bn.running_mean.zero_(), bn.running_var.zero_()
        b = bn(x.clone())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])              # training mode: run to run


def test_initial_state():
    """A fresh BatchNorm in eval mode: weight 1, bias 0, running mean 0 and running VARIANCE 0 -- outputs are
    weight * (x / sqrt(eps)) (+ 0), with weight and sqrt(eps) correctly rounded; an uninitialised ActNorm in eval mode is the
    identity exactly, log-determinant 0."""
    from nflows_amd.transforms import ActNorm, BatchNorm
    x = torch.randn(333, 7, device=DEV)
    t = BatchNorm(7).to(DEV).eval()
    weight = (torch.nn.functional.softplus(t.unconstrained_weight.detach().double()) + t.eps).float()
    root = torch.full((7,), t.eps, dtype=torch.float64, device=DEV).sqrt().float()
    with torch.no_grad():
        y, lad = t(x)
    assert torch.equal(y, weight * (x / root))
    want = (torch.log(torch.nn.functional.softplus(t.unconstrained_weight.detach().double()) + t.eps)
            - 0.5 * np.log(t.eps)).sum()
    assert rows_equal(lad) and abs(float(lad[0]) - float(want)) <= 1.2e-7 * abs(float(want))
    assert not t.running_mean.any() and not t.running_var.any()          # eval mode leaves the buffers alone
    a = ActNorm(7).to(DEV).eval()
    with torch.no_grad():
        y, lad = a(x)
        back, ladi = a.inverse(x)
    assert torch.equal(y, x) and torch.equal(back, x) and not lad.any() and not ladi.any() and not bool(a.initialized)


# (BatchNorm has no inverse in training mode: InverseNotAvailable, as in the reference)
FUSED_CASES = [("batch_norm_train", False), ("batch_norm_eval", False), ("batch_norm_eval", True), ("act_norm", False),
               ("act_norm", True)]


@pytest.mark.parametrize("kind,inverse", FUSED_CASES)
@pytest.mark.parametrize("features", [5, 64, 300])
def test_fused_permutation_and_accumulate_equal_the_unfused_sequence(features, kind, inverse):
    """in_perm (forward) / out_scatter (inverse) and the accumulated log-determinant against index_select outside the
    layer: values and every gradient, bit for bit."""
    torch.manual_seed(features)
    perm = torch.randperm(features, device=DEV)
    x0 = torch.randn(300, features, device=DEV) * 2 + 1
    r = torch.randn(300, features, device=DEV)
    running = torch.randn(300, device=DEV)
    results = []
    for fused in (True, False):
        t = random_batch_norm(features, seed=8) if kind.startswith("batch_norm") else random_act_norm(features, seed=8)
        t.train(kind == "batch_norm_train")
        t._use_kernel = "always"     # K17's forward and backward
        x = x0.clone().requires_grad_(True)
        acc = running.clone()
        if not inverse:
            if fused:
                y, lad = t(x, in_perm=perm, logabsdet_accumulator=acc)
                assert lad is acc
            else:
                y, lad = t(x.index_select(1, perm))
                lad = running + lad
        elif fused:
            y, lad = t.inverse(x, out_scatter=perm, logabsdet_accumulator=acc)
        else:
            v, lad = t.inverse(x)
            y = v.index_select(1, torch.argsort(perm))     # y[:, perm[j]] = v[:, j]
            lad = running + lad
        ((y * r).sum() + 0.5 * lad.sum()).backward()
        results.append([y.detach(), lad.detach(), x.grad] + [q.grad for q in t.parameters()]
                       + ([t.running_mean.clone(), t.running_var.clone()] if kind.startswith("batch_norm") else []))
    for i, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), i
    assert results[0][2].abs().sum() > 0 and all(torch.isfinite(v).all() for v in results[0])
    # and without autograd (the kernel's own accumulate)
    t.eval()
    with torch.no_grad():
        acc = running.clone()
        if not inverse:
            y, _ = t(x0, in_perm=perm, logabsdet_accumulator=acc)
            want, lad = t(x0.index_select(1, perm))
        else:
            y, _ = t.inverse(x0, out_scatter=perm, logabsdet_accumulator=acc)
            v, lad = t.inverse(x0)
            want = v.index_select(1, torch.argsort(perm))
        assert torch.equal(y, want) and torch.equal(acc, running + lad)


def test_parameter_writes_are_seen_by_the_next_call():
    from nflows_amd.transforms import ActNorm, BatchNorm
    x = torch.randn(512, 64, device=DEV)
    for t, cls in ((random_batch_norm(64, seed=5).eval(), BatchNorm), (random_act_norm(64, seed=5).eval(), ActNorm)):
        def fresh_copy():
            f = cls(64).to(DEV).eval()
            f.load_state_dict(t.state_dict())
            return f

        first = next(t.parameters())
        with torch.no_grad():
            before, _ = t(x)
        first.data[7] += 0.25
        first.data.mul_(1.5)
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
        other = cls(64).to(DEV).eval()
        state = {k: (v + 0.125 if v.dtype == torch.float32 else v) for k, v in t.state_dict().items()}
        other.load_state_dict(state)
        t.load_state_dict(state)
        with torch.no_grad():
            assert torch.equal(t(x)[0], other(x)[0]) and not torch.equal(t(x)[0], stepped)


def test_act_norm_initialises_once_and_keeps_a_loaded_state():
    from nflows_amd.transforms import ActNorm
    x1 = torch.randn(700, 12, device=DEV) * 3 + 2
    x2 = torch.randn(700, 12, device=DEV) * 0.3 - 5
    t = ActNorm(12).to(DEV)
    t.eval()
    with torch.no_grad():
        t(x1)
    assert not bool(t.initialized) and not t.log_scale.any()             # eval mode never initialises
    t.train()
    y, _ = t(x1)
    assert bool(t.initialized)
    assert float(y.mean(0).abs().max()) < 1e-5 and float((y.std(0) - 1).abs().max()) < 1e-5
    kept = copy.deepcopy(t.state_dict())
    t(x2)
    assert all(torch.equal(v, kept[k]) for k, v in t.state_dict().items())   # the second batch does not
    loaded = ActNorm(12).to(DEV)
    loaded.load_state_dict(kept)
    loaded.train()
    out, _ = loaded(x2)
    assert all(torch.equal(v, kept[k]) for k, v in loaded.state_dict().items())   # nor is a loaded state overwritten
    assert torch.equal(out, t(x2)[0])


def test_other_ranks_and_float64_take_the_generic_device_path():
    from nflows_amd.transforms import ActNorm
    t = random_act_norm(6, seed=7).eval()
    img = torch.randn(5, 6, 4, 3, device=DEV)
    rows = img.permute(0, 2, 3, 1).reshape(-1, 6)
    with torch.no_grad():
        y4, lad4 = t(img)
        yr, ladr = t(rows)
        back4, ladb4 = t.inverse(y4)
        y64, lad64 = copy.deepcopy(t).double()(rows.double())
    assert y4.shape == img.shape and lad4.shape == (5,)
    assert float((y4.permute(0, 2, 3, 1).reshape(-1, 6) - yr).abs().max()) <= OUT_TOL * (1 + float(yr.abs().max()))
    assert float((lad4 - 12 * ladr[0]).abs().max()) <= LAD_TOL * (1 + abs(float(12 * ladr[0])))
    assert float((back4 - img).abs().max()) <= 1e-5 and float((ladb4 + lad4).abs().max()) <= 1e-5
    assert y64.dtype == torch.float64 and float((y64 - yr.double()).abs().max()) <= OUT_TOL * (1 + float(yr.abs().max()))
    assert abs(float(lad64[0]) - float(ladr[0])) <= LAD_TOL * (1 + abs(float(ladr[0])))
    fresh = ActNorm(6).to(DEV).train()           # per-channel initialisation from an image batch
    out, _ = fresh(img * 2 + 1)
    flat = out.permute(0, 2, 3, 1).reshape(-1, 6)
    assert bool(fresh.initialized) and float(flat.mean(0).abs().max()) < 1e-5 and float((flat.std(0) - 1).abs().max()) < 1e-5
    bn = random_batch_norm(6, seed=7).eval()
    with torch.no_grad():
        y, lad = bn(rows)
        y64, lad64 = copy.deepcopy(bn).double()(rows.double())
        one, _ = bn.train()(rows[:1])            # batch statistics of one row: NaN, as in the reference
    assert float((y64 - y.double()).abs().max()) <= OUT_TOL * (1 + float(y.abs().max()))
    assert abs(float(lad64[0]) - float(lad[0])) <= LAD_TOL * (1 + abs(float(lad[0])))
    assert torch.isnan(one).all()


# ------------------------------------------------------------------------------------------ the factories
class Hook:
    def __init__(self):
        self.calls = []

    def begin(self, name):
        self.calls.append(name)

    def end(self, token, nbytes):
        pass


def launches(fn):
    from nflows_amd import ops
    hook = Hook()
    ops.set_launch_hook(hook)
    try:
        with torch.no_grad():
            fn()
    finally:
        ops.set_launch_hook(None)
    return hook.calls


def build(key, **kw):
    from nflows_amd.flows import MaskedAutoregressiveFlow, SimpleRealNVP
    if key == "maf":
        return MaskedAutoregressiveFlow(features=8, hidden_features=32, num_layers=3, num_blocks_per_layer=2, **kw)
    return SimpleRealNVP(features=16, hidden_features=32, num_layers=4, num_blocks_per_layer=2, **kw)


@pytest.mark.parametrize("key", ["maf", "realnvp"])
def test_factory_flows_match_the_reference_and_train(key):
    import nflows_amd
    from nflows_amd.transforms import BatchNorm
    with np.load(os.path.join(GOLDEN, "norm_flow_%s.npz" % key)) as z:
        g = {k: z[k] for k in z.files}
    features = 8 if key == "maf" else 16

    def state(prefix):
        return {k[len(key + prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(key + prefix)}

    xa, xb, x = (dev(norm_inputs(features, 10 + i, 512)[0]) for i in range(3))
    tag = "factory " + key
    flow = build(key, batch_norm_between_layers=True)
    flow.load_state_dict(state("/start/"), strict=True)
    flow = flow.to(DEV).train()
    with torch.no_grad():
        lp_train = flow.log_prob(xa)
        flow.log_prob(xb)
    compare(tag, "log_prob (training mode)", lp_train.cpu().numpy(), g[key + "/train_log_prob"],
            truth(g, key + "/train_log_prob"), LAD_TOL)
    want = state("/state/")
    buffers = 0
    for k, v in flow.state_dict().items():       # two training passes filled the running buffers like the reference's
        if "running_" in k:
            name = "%s/buffers/%s" % (key, k)
            compare(tag, k, v.cpu().numpy(), g[name], truth(g, name), OUT_TOL)
            buffers += 1
    assert buffers == 2 * (3 if key == "maf" else 4)
    flow.load_state_dict(want, strict=True)
    flow.eval()
    with torch.no_grad():
        lp = flow.log_prob(x)
        z, lad = flow._transform(x)
        xs, ladi = flow._transform.inverse(dev(g[key + "/z"]))
    nflows_amd.check_status()
    compare(tag, "log_prob", lp.cpu().numpy(), g[key + "/log_prob"], truth(g, key + "/log_prob"), LAD_TOL)
    compare(tag, "z", z.cpu().numpy(), g[key + "/z"], truth(g, key + "/z"), OUT_TOL)
    compare(tag, "logabsdet", lad.cpu().numpy(), g[key + "/lad"], truth(g, key + "/lad"), LAD_TOL)
    compare(tag, "x from z", xs.cpu().numpy(), g[key + "/x_from_z"], truth(g, key + "/x_from_z"), OUT_TOL)
    compare(tag, "logabsdet(inverse)", ladi.cpu().numpy(), g[key + "/ladi"], truth(g, key + "/ladi"), LAD_TOL)
    # one K17 launch per normalisation layer, in both directions and in training mode (plus its statistics there)
    layers = 3 if key == "maf" else 4
    for fn in (lambda: flow._transform(x), lambda: flow._transform.inverse(x)):
        calls = launches(fn)
        assert calls.count("norm_map") == layers and "norm_stats" not in calls, calls
    flow.train()
    calls = launches(lambda: flow._transform(x))
    assert calls.count("norm_map") == layers and calls.count("norm_stats") == layers, calls
    # one Adam step in training mode moves every normalisation parameter and both running buffers
    norms = {n: m for n, m in flow.named_modules() if isinstance(m, BatchNorm)}
    assert len(norms) == layers
    before = {n: copy.deepcopy(m.state_dict()) for n, m in norms.items()}
    opt = torch.optim.Adam(flow.parameters(), lr=1e-3)
    loss = -flow.log_prob(xa).mean()
    loss.backward()
    opt.step()
    assert torch.isfinite(loss)
    for n, m in norms.items():
        for k, v in m.state_dict().items():
            assert torch.isfinite(v).all() and not torch.equal(v, before[n][k]), (n, k)
    assert all(torch.isfinite(p).all() for p in flow.parameters())


def test_a_permutation_next_to_a_normalisation_layer_is_folded():
    from nflows_amd.transforms import ActNorm, BatchNorm, CompositeTransform, RandomPermutation
    torch.manual_seed(3)
    stack = CompositeTransform([RandomPermutation(24), random_batch_norm(24, seed=1), RandomPermutation(24),
                                random_act_norm(24, seed=2)]).to(DEV).eval()
    plain = CompositeTransform(list(stack._transforms), fuse_permutations=False)
    x = torch.randn(500, 24, device=DEV)
    for fn, ref in ((lambda: stack(x), lambda: plain(x)), (lambda: stack.inverse(x), lambda: plain.inverse(x))):
        calls = launches(fn)
        assert calls.count("norm_map") == 2 and "permute_cols" not in calls, calls
        with torch.no_grad():
            (a, la), (b, lb) = fn(), ref()
        assert torch.equal(a, b) and float((la - lb).abs().max()) <= LAD_TOL * (1 + float(lb.abs().max()))
    assert isinstance(stack._transforms[1], BatchNorm) and isinstance(stack._transforms[3], ActNorm)


def test_without_the_option_the_factory_flow_keeps_its_one_launch_path():
    """SimpleRealNVP without batch_norm_between_layers is the composition `configs.simple_realnvp_flow` builds: the same
    launches (K11's whole-layer run), none of K17's."""
    from nflows_amd import configs
    torch.manual_seed(0)
    flow = build("realnvp").to(DEV).eval()
    same = configs.simple_realnvp_flow(features=16, hidden_features=32, num_layers=4, num_blocks_per_layer=2, seed=0).to(DEV).eval()
    x = torch.randn(1024, 16, device=DEV)
    with torch.no_grad():
        assert torch.equal(flow.log_prob(x), same.log_prob(x))
    from nflows_amd import ops
    counts = {"k11": 0, "k2": 0}
    whole, single = ops.affine_flow_mlp, ops._affine_coupling_launch

    def count(name, fn):
        def wrapped(*args, **kw):
            counts[name] += 1
            return fn(*args, **kw)
        return wrapped

    ops.affine_flow_mlp, ops._affine_coupling_launch = count("k11", whole), count("k2", single)
    try:
        for fn, direction in ((lambda: flow.log_prob(x), "inverse=0"), (lambda: flow._transform(x), "inverse=0"),
                              (lambda: flow._transform.inverse(x), "inverse=1")):
            counts["k11"] = counts["k2"] = 0
            calls = launches(fn)
            # ONE launch of K11 for the four couplings, none of the single-layer kernel, none of K17
            assert counts == {"k11": 1, "k2": 0}, counts
            ran = ops.last_layer_kernel()
            assert "affine_mlp_kernel<" in ran and "resnet=1" in ran and direction in ran, ran
            assert "norm_map" not in calls and "norm_stats" not in calls, calls
    finally:
        ops.affine_flow_mlp, ops._affine_coupling_launch = whole, single
    from nflows_amd.transforms.base import CompositeTransform
    with_norm = build("realnvp", batch_norm_between_layers=True).to(DEV).eval()
    with torch.no_grad():                        # (whole-layer runs are planned for no-grad passes)
        units, after = flow._transform._collect_run(list(flow._transform._transforms), 0, x, None, inverse=False)
        assert len(units) == 4 and after == 4       # one whole-layer run over all four couplings
        units, _ = with_norm._transform._collect_run(list(with_norm._transform._transforms), 0, x, None, inverse=False)
    assert not units                             # a normalisation layer between couplings ends the run
    assert isinstance(with_norm._transform, CompositeTransform)


def test_small_differentiated_passes_take_the_generic_path():
    """The dispatch rule (transforms/normalization.py: AUTOGRAD_MIN_ELEMENTS, from profiles/norm_time.json): under autograd
    fewer than 2^23 elements go down the generic path, more through K17; without autograd everything goes through K17.  Both
    paths give the same gradients to rounding."""
    from nflows_amd import ops
    from nflows_amd.transforms.normalization import AUTOGRAD_MIN_ELEMENTS

    def names(t, x):
        hook = Hook()
        ops.set_launch_hook(hook)
        try:
            y, lad = t(x)
        finally:
            ops.set_launch_hook(None)
        return hook.calls, y, lad

    assert AUTOGRAD_MIN_ELEMENTS == 1 << 23
    for t in (random_batch_norm(64, seed=9).train(), random_act_norm(64, seed=9)):
        small = torch.randn(1024, 64, device=DEV)
        big = torch.randn(AUTOGRAD_MIN_ELEMENTS // 64, 64, device=DEV)
        assert "norm_map" not in names(t, small)[0] and "norm_map" in names(t, big)[0]
        with torch.no_grad():
            assert "norm_map" in names(t, small)[0]
        grads = []
        for mode in (True, "always"):
            t._use_kernel = mode
            t.zero_grad()
            xin = small.clone().requires_grad_(True)
            calls, y, lad = names(t, xin)
            assert ("norm_map" in calls) == (mode == "always")
            ((y * y).sum() + lad.sum()).backward()
            grads.append([xin.grad] + [p.grad.clone() for p in t.parameters()])
        for a, b in zip(*grads):
            assert float((a - b).abs().max()) <= 1e-4 * (1 + float(b.abs().max()))
