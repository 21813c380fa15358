"""FusedSteps::derivative (rqs_fused8.hpp), min_d + softplus(u kappa), compiled for the host the way tests/_hostcore/
rqs_f32_host.py compiles the evaluators: the correction of the rounding of 1 + exp(-|t|) takes 1.5 - 0.5 u1p for 1 / u1p
(round 10: no reciprocal).  Against float64 over the whole range of derivative logits, at kappa = 1 and at a power of two.

The bound, from the number formats (eps = 2^-24, the host's exp2f / log2f taken as correctly rounded):
  * |t| >= 17: exp(-|t|) < eps / 2 of 1, u1p = 1, the correction carries the whole term with factor exactly 1: two roundings
    (the fma onto min_d, the final add) -> 2 eps relative;
  * otherwise: the exponent -|u kl2e| carries <= 1.5 eps |t| log2(e) relative error of its own (the constant's rounding and the
    product's), i.e. <= 1.5 eps |t| exp(-|t|) / ln 2 <= 0.8 eps absolute in the softplus term; log2f, the product with ln 2 (its
    constant is rounded too) and the fma onto min_d: <= 2.5 eps relative to log1p <= ln 2; the linear factor is off by at most
    0.086 at u1p = sqrt 2, times |c| <= eps / 2 (u1p < 2): 0.043 eps absolute; the final add: eps / 2 relative.
  Together <= 4 eps relative + 1 eps absolute, values being >= min_d = 1e-3.
The old form (a true reciprocal) differs from the new one by at most 0.043 eps + one rounding: not measurable here, and that is
the point.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _hostcore import rqs_f32_host as H

HARNESS = r'''
extern "C" int host_fused_derivative(float kappa, float min_d, int64_t n, const float* u, float* d) {
    nfa::RqsDev sp;
    memset(&sp, 0, sizeof sp);
    sp.min_d = min_d;
    for (int64_t i = 0; i < n; ++i) {
        nfa::FusedSteps<false, 8> f;
        memset(&f, 0, sizeof f);
        f.kappa = kappa;
        f.kl2e = 1.44269502162933349609375f * kappa;
        float out = 0.0f;
        f.derivative<0>(u[i], out, sp);
        f.derivative<1>(u[i], out, sp);
        f.derivative<2>(u[i], out, sp);
        d[i] = out;
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("softplus_host"))
    csrc = os.path.join(H.ROOT, "nflows_amd", "csrc")
    math_src = open(os.path.join(csrc, "rqs_math.hpp")).read()
    cpp, so = os.path.join(out, "softplus_host.cpp"), os.path.join(out, "softplus_host.so")
    with open(cpp, "w") as f:
        f.write(math_src.replace('#include "common.hpp"', H.SHIM).replace("#pragma once", "", 1) + H._fused8_for_the_host(csrc) + HARNESS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           "-I" + os.path.join(H.ROOT, "include"), cpp, "-o", so])
    lib = ctypes.CDLL(so)
    lib.host_fused_derivative.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.host_fused_derivative.restype = ctypes.c_int
    return lib


@pytest.mark.parametrize("kappa", [1.0, 0.25])
def test_softplus_correction_without_a_reciprocal(lib, kappa):
    eps, min_d = 2.0 ** -24, 1e-3
    rng = np.random.RandomState(3)
    # true logits t = u kappa: dense around zero, where u1p runs through [1, 2]; the tails out to -100 and 200; the points
    # where 1 + exp(-|t|) is 1, sqrt 2 and 2
    t = np.concatenate([np.linspace(-20.0, 20.0, 200001), rng.uniform(-100.0, 200.0, 50000),
                        np.array([0.0, -0.0, 1e-30, -1e-30, 0.881373587, -0.881373587, 16.5, -16.5, 17.0, -17.0, 88.0, -88.0,
                                  200.0, -100.0])])
    u = (t / kappa).astype(np.float32)
    d = np.empty_like(u)
    assert lib.host_fused_derivative(kappa, min_d, u.size, u.ctypes.data_as(ctypes.c_void_p), d.ctypes.data_as(ctypes.c_void_p)) == 0
    tt = u.astype(np.float64) * kappa
    truth = float(np.float32(min_d)) + np.maximum(tt, 0.0) + np.log1p(np.exp(-np.abs(tt)))
    err = np.abs(d.astype(np.float64) - truth)
    allowed = 4 * eps * truth + eps
    worst = int(np.argmax(err / allowed))
    print("kappa %g: worst error %.3e of %.3e allowed at t = %g" % (kappa, err[worst], allowed[worst], tt[worst]))
    assert np.all(err <= allowed), (tt[worst], d[worst], truth[worst], err[worst], allowed[worst])
    # very negative logits: the softplus term itself, not only the sum, keeps its relative accuracy
    neg = tt <= -17.0
    term = d[neg].astype(np.float64) - float(np.float32(min_d))
    want = np.exp(tt[neg])
    big = want >= 1e-3 * eps   # (above the rounding of the sum onto min_d)
    assert np.all(np.abs(term[big] - want[big]) <= eps * float(np.float32(min_d)) + 4 * eps * want[big])
