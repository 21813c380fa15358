"""K18 at the shapes where its forward and backward kernels take paths that the fixture shapes do not reach, and
`GatedLinearUnit` on the device.

No fixtures here: the yardstick is the same class in float64 on its generic path (the reference's sequence by stock float64
device ops, itself held to the fixtures' float64 by test_gpu_nonlinearities.py::test_generic_paths) at the SAME float32
inputs.  K18 evaluates every element in float64 and rounds each result once, so against that yardstick it may be off by the
one rounding -- half an ulp, 2^-24 relative -- plus what two float64 formulations of the same quantity differ by.  The bound
is one whole ulp, 2^-23 |value|, plus 1e-9 absolute for the float64 side (row sums and the temperature gradient add at most
a few thousand float64 terms of magnitude <= 1e2: 1e4 * 1e2 * 2^-52 = 2e-10)."""
import numpy as np
import pytest
import torch

from nonlin_cases import KINDS, make, nonlin_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# N = 1: no sum, and the backward's row index by a division by one;  7 x 4096: a row cut into pieces, float4 lanes;
# 5 x 2047: one row per workgroup, scalar lanes, a row's sum by one wave;  3 x 2049: a single odd piece per row
EDGE_SHAPES = ((301, 1), (7, 4096), (5, 2047), (3, 2049))


def ids(shape):
    return "x".join(map(str, shape))


def close(got, want, what):
    want = want.double()
    err = (got.double() - want).abs()
    bound = 2.0 ** -23 * want.abs() + 1e-9
    worst = int(torch.argmax(err - bound))
    assert bool((err <= bound).all()), "%s: error %.3e at value %.6e (bound %.3e)" % (
        what, float(err.flatten()[worst]), float(want.flatten()[worst]), float(bound.flatten()[worst]))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=ids)
@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_backward_at_the_edges_of_the_plan(kind, shape):
    x, r = nonlin_inputs(kind, shape)
    k = make(kind).to(DEV)
    k._use_kernel = "always"
    wide = make(kind).double().to(DEV)
    source = torch.from_numpy(x).to(DEV)
    weights = torch.from_numpy(r).to(DEV)
    for inverse in (False, True):
        xin = source.clone().requires_grad_(True)
        xin64 = source.double().requires_grad_(True)
        y, lad = k.inverse(xin) if inverse else k(xin)
        y64, lad64 = wide.inverse(xin64) if inverse else wide(xin64)
        assert y.dtype == torch.float32 and y64.dtype == torch.float64
        what = "%s %s %s" % (kind, ids(shape), "inverse" if inverse else "forward")
        close(y.detach(), y64.detach(), what + " outputs")
        close(lad.detach(), lad64.detach(), what + " logabsdet")
        ((y * weights).sum() + lad.sum()).backward()
        ((y64 * weights.double()).sum() + lad64.sum()).backward()
        close(xin.grad, xin64.grad, what + " grad inputs")
        if kind == "sigmoid_t":
            close(k.temperature.grad, wide.temperature.grad, what + " grad temperature")
            k.temperature.grad = None
            wide.temperature.grad = None
        if not inverse:
            source = y.detach()      # the inverse pass starts from K18's own forward outputs


def test_gated_linear_unit_on_the_device():
    from nflows_amd.transforms import GatedLinearUnit
    rng = np.random.RandomState(5)
    x = torch.from_numpy(rng.randn(257, 1).astype(np.float32)).to(DEV)
    context = torch.from_numpy(rng.randn(257, 1).astype(np.float32)).to(DEV)
    t = GatedLinearUnit().to(DEV)
    with torch.no_grad():
        y, lad = t(x, context)
        back, ladi = t.inverse(y, context)
    gate = torch.sigmoid(context.double())
    assert y.shape == x.shape and lad.shape == (257,) and y.device == x.device
    # float32 stock ops: a sigmoid, a product, a logarithm -- a few ulps of the value each
    assert float((y.double() - x.double() * gate).abs().max()) <= 4 * 2.0 ** -23 * float(x.abs().max())
    assert float((lad.double() - torch.log(gate).reshape(-1)).abs().max()) <= 8 * 2.0 ** -23 * float(torch.log(gate).abs().max())
    assert torch.equal(ladi, -lad)
    assert float((back - x).abs().max()) <= 4 * 2.0 ** -23 * float(x.abs().max())
