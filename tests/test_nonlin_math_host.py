"""The per-element arithmetic of K18 -- nflows_amd/csrc/nonlin_math.hpp: `nonlin_eval`, `nonlin_grad`, `nonlin_constants`,
`nonlin_row_scale`, the functions the kernels of nonlin.hip call per lane -- compiled for the HOST from the product's source
(through tests/_hostcore/nonlin_host.cpp) at test time and held to the reference's vectors (tests/golden/nonlin_*.npz, written by tests/golden/make_golden_nonlin.py)
under the project's parity rule: `compare()` of tests/test_gpu_headline_parity.py with OUT_TOL / LAD_TOL -- error against
float64 at most 2 x the reference-float32's own on maximum (+ four ulps), mean and 99.9 % quantile; where the reference's
own error is zero, that is exactness.  The row sum is the kernels' rule, not their order: float64, rounded once.  The host
build replaces nothing but the device's float64 libm; CPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import LAD_TOL, OUT_TOL
from nonlin_cases import GRAD_SHAPES, KINDS, SHAPES, golden, nonlin_inputs, truth
from test_gpu_headline_parity import compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = os.path.join(ROOT, "tests", "_hostcore", "nonlin_host.cpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("nonlin_host")
    so = str(d / "nonlin_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nflows_amd", "csrc"), SRC, "-o", so])
    lib = ctypes.CDLL(so)
    p, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    lib.host_nonlin.argtypes = [i32, i32, i64, i64, f64, f64, f64, ctypes.c_float, p, p, p]
    lib.host_nonlin.restype = i32
    lib.host_nonlin_grad.argtypes = [i32, i32, i64, i64, f64, f64, f64, ctypes.c_float, p, p, p, p, p]
    lib.host_nonlin_grad.restype = None
    return lib


def abi_arguments(kind):
    """(kind code, p0, p1, p2, temperature) as the layer of the fixture kind hands them to the C ABI."""
    from nflows_amd import ops
    from nonlin_cases import make
    t = make(kind)
    c = tuple(float(v) for v in t._constants()) + (0.0,) * (3 - len(t._constants()))
    temperature = float(t.temperature.detach()[0]) if kind.startswith("sigmoid") else 0.0
    return (ops.NONLIN_KINDS[t._kind],) + c + (temperature,)


def evaluate(lib, kind, inverse, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows = x.shape[0]
    n = x.size // rows
    y, lad = np.empty_like(x), np.empty(rows, dtype=np.float32)
    code, p0, p1, p2, temperature = abi_arguments(kind)
    status = lib.host_nonlin(code, int(inverse), rows, n, p0, p1, p2, temperature, x.ctypes.data, y.ctypes.data, lad.ctypes.data)
    return y, lad, status


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_forward_and_inverse_against_the_reference(lib, kind, shape):
    fwd, inv = golden(kind, shape, "fwd"), golden(kind, shape, "inv")
    x, _ = nonlin_inputs(kind, shape)
    config = "nonlin_math %s %s" % (kind, "x".join(map(str, shape)))
    y, lad, status = evaluate(lib, kind, False, x)
    assert status == 0
    compare(config, "y", y, fwd["y"], truth(fwd, "y"), OUT_TOL)
    compare(config, "logabsdet", lad, fwd["lad"], truth(fwd, "lad"), LAD_TOL)
    xi, ladi, status = evaluate(lib, kind, True, fwd["y"])       # at the reference's own float32 forward output
    assert status == 0
    compare(config, "x", xi, inv["x"], truth(inv, "x"), OUT_TOL)
    compare(config, "logabsdet(inverse)", ladi, inv["lad"], truth(inv, "lad"), LAD_TOL)


@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", KINDS)
def test_backward_factors_against_the_reference(lib, kind, shape):
    """g_in = r * dy/dx + 1 * d(term)/dx is the gradient of sum(y * r) + sum(logabsdet); the temperature's is the float64
    sum of r * dy/dT + d(term)/dT, rounded once."""
    x, r = nonlin_inputs(kind, shape)
    rows, n = shape
    ones = np.ones(rows, dtype=np.float32)
    code, p0, p1, p2, temperature = abi_arguments(kind)
    for part, inverse, source in (("grad", 0, x), ("gradi", 1, golden(kind, shape, "fwd")["y"])):
        g = golden(kind, shape, part)
        source = np.ascontiguousarray(source, dtype=np.float32)
        gx, gt = np.empty_like(source), ctypes.c_double(0.0)
        lib.host_nonlin_grad(code, inverse, rows, n, p0, p1, p2, temperature, source.ctypes.data, r.ctypes.data,
                             ones.ctypes.data, gx.ctypes.data, ctypes.byref(gt))
        config = "nonlin_math %s %dx%d %s" % (kind, rows, n, part)
        compare(config, "grad inputs", gx, g["inputs"], truth(g, "inputs"), OUT_TOL)
        if kind == "sigmoid_t":
            compare(config, "grad temperature", np.array([gt.value], dtype=np.float32), g["temperature"],
                    truth(g, "temperature"), OUT_TOL)
        else:
            assert "temperature" not in g


def test_domain_errors_are_reported_and_nothing_else_is(lib):
    from nflows_amd import _native as N
    cases = {"exp": (0.0, -1.0), "tanh": (1.0, -1.0, 1.5), "sigmoid": (-0.25, 1.5), "cauchy": (-1e-3, 1.0 + 1e-3)}
    good = {"exp": 0.5, "tanh": 0.5, "sigmoid": 0.5, "cauchy": 0.5, "logtanh": 0.5, "leaky": 0.5, "sigmoid_t": 0.5}
    for kind in KINDS:
        for inverse in (False, True):
            for bad in (cases.get(kind, ()) if inverse else ()):
                _, _, status = evaluate(lib, kind, inverse, np.array([[good[kind], bad, good[kind]]], dtype=np.float32))
                assert status == N.STATUS_OUTSIDE_DOMAIN, (kind, bad)
            _, lad, status = evaluate(lib, kind, inverse, np.array([[good[kind], 0.25]], dtype=np.float32))
            assert status == 0 and np.isfinite(lad).all(), (kind, inverse)
    # the closed ends of [0, 1] are inside Sigmoid's and CauchyCDF's inverse domain (the reference tests < 0 and > 1)
    for kind in ("sigmoid", "cauchy"):
        assert evaluate(lib, kind, True, np.array([[0.0, 1.0]], dtype=np.float32))[2] == 0


def test_exact_cases(lib):
    """Exp's logabsdet of a one-element row is the input itself; LeakyReLU on the positive side is a copy; Sigmoid's inverse
    clamps to [eps, 1 - eps] first."""
    x = nonlin_inputs("exp", (4093, 1))[0]
    _, lad, _ = evaluate(lib, "exp", False, x)
    assert np.array_equal(lad, x[:, 0])
    x = np.abs(nonlin_inputs("leaky", (1021, 67))[0])
    for inverse in (False, True):
        y, lad, _ = evaluate(lib, "leaky", inverse, x)
        assert np.array_equal(y, x) and not lad.any()
    ends, _, status = evaluate(lib, "sigmoid", True, np.array([[0.0, 1.0, 1e-9]], dtype=np.float32))
    eps, top = 1e-6, 1.0 - 1e-6      # (in float64: the bounds of the reference's float64 run)
    want = np.array([np.log(eps) - np.log1p(-eps), np.log(top) - np.log1p(-top), np.log(eps) - np.log1p(-eps)])
    assert status == 0 and np.allclose(ends[0], want, rtol=1e-6)
