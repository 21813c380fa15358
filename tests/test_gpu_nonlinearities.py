"""K18 (Exp, Tanh, LogTanh, LeakyReLU, Sigmoid / Logit, CauchyCDF / CauchyCDFInverse, CompositeCDFTransform) on the GPU against
the reference's float32 / float64 results (tests/golden/nonlin_*.npz, written by tests/golden/make_golden_nonlin.py) under the
project's parity rule -- `compare()` of tests/test_gpu_headline_parity.py with OUT_TOL / LAD_TOL of tests/helpers.py: error
against float64 at most 2 x the reference-float32's own on maximum (+ four ulps), mean and 99.9 % quantile -- and the
properties of the kernel that are exact."""
import os

import numpy as np
import pytest
import torch

from helpers import LAD_TOL, OUT_TOL
from nonlin_cases import GOLDEN, GRAD_SHAPES, KINDS, SHAPES, golden, make, nonlin_inputs, truth
from test_gpu_headline_parity import compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ids(shape):
    return "x".join(map(str, shape))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def layer(kind, use_kernel="always"):
    t = make(kind).to(DEV)
    t._use_kernel = use_kernel
    return t


def launches(fn):
    from nflows_amd import ops

    class Hook:
        calls = []

        def begin(self, name):
            self.calls.append(name)

        def end(self, token, nbytes):
            pass

    hook = Hook()
    hook.calls = []
    ops.set_launch_hook(hook)
    try:
        fn()
    finally:
        ops.set_launch_hook(None)
    return hook.calls


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_inverse_and_round_trip_against_the_reference(kind, shape):
    fwd, inv = golden(kind, shape, "fwd"), golden(kind, shape, "inv")
    x, _ = nonlin_inputs(kind, shape)
    t = layer(kind)
    config = "nonlin %s %s" % (kind, ids(shape))
    with torch.no_grad():
        calls = launches(lambda: t(dev(x)))
        y, lad = t(dev(x))
        xi, ladi = t.inverse(dev(fwd["y"]))       # at the reference's own float32 forward output
        back, _ = t.inverse(y)
    assert calls == ["nonlin"], calls             # K18, one launch
    assert y.shape == tuple(shape) and lad.shape == (shape[0],)
    compare(config, "y", y.cpu().numpy(), fwd["y"], truth(fwd, "y"), OUT_TOL)
    compare(config, "logabsdet", lad.cpu().numpy(), fwd["lad"], truth(fwd, "lad"), LAD_TOL)
    compare(config, "x", xi.cpu().numpy(), inv["x"], truth(inv, "x"), OUT_TOL)
    compare(config, "logabsdet(inverse)", ladi.cpu().numpy(), inv["lad"], truth(inv, "lad"), LAD_TOL)
    # the reference's own float32 round trip (its inverse of ITS forward output) is the yardstick of ours
    compare(config, "round trip", back.cpu().numpy(), inv["x"], x.astype(np.float64), OUT_TOL)


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_against_the_reference(kind, shape):
    x, r = nonlin_inputs(kind, shape)
    for part, inverse, source in (("grad", False, x), ("gradi", True, golden(kind, shape, "fwd")["y"])):
        g = golden(kind, shape, part)
        t = layer(kind)
        xin = dev(source).requires_grad_(True)
        y, lad = t.inverse(xin) if inverse else t(xin)
        ((y * dev(r)).sum() + lad.sum()).backward()
        config = "nonlin %s %s %s" % (kind, ids(shape), part)
        compare(config, "grad inputs", xin.grad.cpu().numpy(), g["inputs"], truth(g, "inputs"), OUT_TOL)
        if kind == "sigmoid_t":
            compare(config, "grad temperature", t.temperature.grad.cpu().numpy(), g["temperature"], truth(g, "temperature"),
                    OUT_TOL)


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_every_run_accumulation_and_views(kind):
    t = layer(kind)
    for shape in ((517, 5), (129, 67), (9, 4100), (37, 3, 5, 7), (5, 3, 32, 32)):
        x = dev(nonlin_inputs(kind, shape)[0])
        with torch.no_grad():
            y, lad = t(x)
            y2, lad2 = t(x.clone())
            assert torch.equal(y, y2) and torch.equal(lad, lad2), shape           # the same bits on every run
            flat_y, flat_lad = t(x.reshape(shape[0], -1))                          # 4-D and flattened view
            assert torch.equal(flat_y.reshape(shape), y) and torch.equal(flat_lad, lad), shape
            total = torch.randn(shape[0], device=DEV)
            from nflows_amd import ops
            acc = total.clone()
            ya, lada = ops.nonlinearity(x, t._kind, t._constants(), t._temperature(), accumulate_into=acc)
            assert lada is acc and torch.equal(ya, y) and torch.equal(acc, total + lad), shape
            xi, ladi = t.inverse(y)
            xi2, ladi2 = t.inverse(y.clone())
            assert torch.equal(xi, xi2) and torch.equal(ladi, ladi2), shape
            # a row's result depends on that row only: fewer rows, the same bits (rows regime: any count; pieces: same plan)
            if x.numel() // shape[0] <= 2048:
                ys, lads = t(x[:3].clone())
                assert torch.equal(ys, y[:3]) and torch.equal(lads, lad[:3]), shape
        empty, lad0 = t(x[:0])
        assert empty.shape == (0,) + tuple(shape[1:]) and lad0.shape == (0,)


@pytest.mark.parametrize("kind", KINDS)
def test_generic_paths(kind):
    """float64 inputs take the generic path and match the fixtures' float64; `_use_kernel=False` on float32 meets the parity
    rule; rank 1 and non-contiguous inputs take the generic path too."""
    shape = (1021, 67)
    fwd, inv = golden(kind, shape, "fwd"), golden(kind, shape, "inv")
    x, _ = nonlin_inputs(kind, shape)
    t64 = make(kind).double().to(DEV)
    with torch.no_grad():
        calls = launches(lambda: t64(dev(x).double()))
        y64, lad64 = t64(dev(x).double())
        xi64, ladi64 = t64.inverse(dev(fwd["y"]).double())
    assert "nonlin" not in calls and y64.dtype == lad64.dtype == torch.float64
    for got, want in ((y64, truth(fwd, "y")), (lad64, truth(fwd, "lad")), (xi64, truth(inv, "x")), (ladi64, truth(inv, "lad"))):
        # (the fixtures hold float64 as float32 + a float32 difference: 2^-24 of the difference is their own resolution)
        err = np.abs(got.cpu().numpy() - want)
        assert float(err.max()) <= 1e-12 * (1 + float(np.abs(want).max())) + 2.0 ** -24 * float(np.abs(want - want.astype(np.float32)).max())
    t = layer(kind, use_kernel=False)
    config = "nonlin generic %s" % kind
    with torch.no_grad():
        calls = launches(lambda: t(dev(x)))
        y, lad = t(dev(x))
        xi, ladi = t.inverse(dev(fwd["y"]))
    assert "nonlin" not in calls
    compare(config, "y", y.cpu().numpy(), fwd["y"], truth(fwd, "y"), OUT_TOL)
    compare(config, "logabsdet", lad.cpu().numpy(), fwd["lad"], truth(fwd, "lad"), LAD_TOL)
    compare(config, "x", xi.cpu().numpy(), inv["x"], truth(inv, "x"), OUT_TOL)
    compare(config, "logabsdet(inverse)", ladi.cpu().numpy(), inv["lad"], truth(inv, "lad"), LAD_TOL)
    k = layer(kind)
    with torch.no_grad():
        strided = dev(x)[:, ::2]
        assert "nonlin" not in launches(lambda: k(strided)) and "nonlin" not in launches(lambda: k(dev(x)[0]))
        ys, lads = k(strided)
        yc, ladc = k(strided.contiguous())
    assert float((ys - yc).abs().max()) <= OUT_TOL * (1 + float(yc.abs().max()))
    assert float((lads - ladc).abs().max()) <= LAD_TOL * (1 + float(ladc.abs().max()))


DOMAIN_CASES = [("exp", "inverse", 0.0), ("tanh", "inverse", 1.0), ("sigmoid", "inverse", 1.25), ("cauchy", "inverse", -0.25)]


@pytest.mark.parametrize("kind,direction,bad", DOMAIN_CASES)
@pytest.mark.parametrize("shape", [(300, 5), (7, 4100)], ids=ids)
def test_domain_errors_raise_and_clear(kind, direction, bad, shape):
    import nflows_amd
    from nflows_amd.transforms import CauchyCDFInverse, InputOutsideDomain, Logit
    t = layer(kind)
    good = torch.full(shape, 0.5, device=DEV)
    one_bad = good.clone()
    one_bad[shape[0] - 1, shape[1] - 2] = bad
    with torch.no_grad():
        with pytest.raises(InputOutsideDomain):
            t.inverse(one_bad)
        y, lad = t.inverse(good)                      # the status word is cleared: the next good call succeeds
        assert torch.isfinite(y).all() and torch.isfinite(lad).all()
        if kind in ("sigmoid", "cauchy"):             # the same through the InverseTransform classes' forward
            wrapped = (Logit() if kind == "sigmoid" else CauchyCDFInverse()).to(DEV)
            with pytest.raises(InputOutsideDomain):
                wrapped(one_bad)
            assert torch.equal(wrapped(good)[0], y)
    nflows_amd.check_status()


def test_a_data_write_to_the_temperature_is_seen_by_the_next_call():
    from nflows_amd.transforms import Sigmoid
    x = dev(nonlin_inputs("sigmoid", (1021, 67))[0])
    for learn in (False, True):
        t = Sigmoid(temperature=1.5, learn_temperature=learn).to(DEV)
        with torch.no_grad():
            before, _ = t(x)
            t.temperature.data.mul_(2)
            after, lad = t(x)
            fresh = Sigmoid(temperature=3.0, learn_temperature=learn).to(DEV)
            want, want_lad = fresh(x)
            back, ladb = t.inverse(after)
            want_back, want_ladb = fresh.inverse(after)
        assert not torch.equal(after, before) and torch.equal(after, want) and torch.equal(lad, want_lad)
        assert torch.equal(back, want_back) and torch.equal(ladb, want_ladb)
    t = Sigmoid(temperature=1.5, learn_temperature=True).to(DEV)
    opt = torch.optim.SGD(t.parameters(), lr=0.1)
    y, lad = t(x)
    (-(lad.mean()) + (y ** 2).mean()).backward()
    opt.step()
    with torch.no_grad():
        stepped, _ = t(x)
        fresh = Sigmoid(temperature=float(t.temperature.detach()[0]), learn_temperature=True).to(DEV)
        fresh.temperature.data.copy_(t.temperature.data)
        assert torch.equal(stepped, fresh(x)[0]) and float(t.temperature.detach()[0]) != 1.5


def test_composite_cdf_transform():
    """CompositeCDFTransform(Sigmoid(), PiecewiseRationalQuadraticCDF([5], tails=None)): runs, round-trips within the tolerance
    the reference's tests/transforms/nonlinearities_test.py uses for its round trips (assert_tensor_is_good + assertEqual at
    eps = 1e-3, :49-50, :159-160), opposite logabsdets."""
    from nflows_amd.transforms import CompositeCDFTransform, PiecewiseRationalQuadraticCDF, Sigmoid
    torch.manual_seed(4)
    t = CompositeCDFTransform(Sigmoid(), PiecewiseRationalQuadraticCDF([5], tails=None)).to(DEV)
    x = torch.randn(300, 5, device=DEV)
    with torch.no_grad():
        calls = launches(lambda: t(x))
        y, lad = t(x)
        back, ladb = t.inverse(y)
    assert calls.count("nonlin") == 2, calls
    assert y.shape == x.shape and lad.shape == (300,) and torch.isfinite(y).all() and torch.isfinite(lad).all()
    assert float((back - x).abs().max()) <= 1e-3 and float((lad + ladb).abs().max()) <= 1e-3


def test_logit_flow_log_prob_against_the_reference():
    import nflows_amd
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.transforms import (CompositeTransform, Logit, PiecewiseRationalQuadraticCouplingTransform,
                                       ReversePermutation)
    from nflows_amd.utils import torchutils
    with np.load(os.path.join(GOLDEN, "nonlin_flow.npz")) as z:
        g = {k: z[k] for k in z.files}
    D, H, K = 6, 32, 8
    layers = [Logit()]
    for i in range(2):
        layers.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=torchutils.create_alternating_binary_mask(D, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=H, num_blocks=2),
            num_bins=K, tails="linear", tail_bound=4.0))
        if i == 0:
            layers.append(ReversePermutation(D))
    flow = Flow(CompositeTransform(layers), StandardNormal([D]))
    flow.load_state_dict({k[len("state/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("state/")}, strict=True)
    flow = flow.to(DEV).eval()
    x = dev(np.random.RandomState(7999).uniform(0.01, 0.99, size=(512, D)).astype(np.float32))
    with torch.no_grad():
        calls = launches(lambda: flow.log_prob(x))
        lp = flow.log_prob(x)
    nflows_amd.check_status()
    assert calls.count("nonlin") == 1, calls
    compare("nonlin flow", "log_prob", lp.cpu().numpy(), g["log_prob"], truth(g, "log_prob"), LAD_TOL)
