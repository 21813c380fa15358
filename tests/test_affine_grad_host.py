"""`affine_element_grad` of nflows_amd/csrc/affine_math.hpp -- the per-element arithmetic of K25's backward kernel for
the affine autoregressive layer (`affine_ar_backward_kernel`, csrc/misc.hip) -- compiled for the HOST from the product's
header at test time, as tests/test_affine_host.py compiles its neighbours, and held to float64 autograd of
y = x * (softplus(u) + 1e-3) + shift and of its inverse.  The host build replaces nothing but the device's libm.  CPU only.

Rule (helpers.close_to_truth's, per element): the error against float64 is at most 4 x the error of the same
expressions evaluated by torch in float32, plus 2e-5 * (1 + max |truth|)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from maf_train_cases import affine_element_truth, within_truth_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#define __device__
#define __forceinline__ inline
#include "nflows_amd.h"
#include "affine_math.hpp"
#include <stdint.h>
using namespace nfa;
// other: the layer's input (forward) or output (inverse); one g_l per element
extern "C" void host_affine_element_grad(int64_t n, const float* other, const float* u, const float* g_y, const float* g_l,
                                         int inverse, float* g_x, float* g_u, float* g_shift) {
    for (int64_t i = 0; i < n; ++i) {
        if (inverse) affine_element_grad<true>(other[i], u[i], g_y[i], g_l[i], g_x[i], g_u[i], g_shift[i]);
        else affine_element_grad<false>(other[i], u[i], g_y[i], g_l[i], g_x[i], g_u[i], g_shift[i]);
    }
}
extern "C" float host_scale_of(float u) { return scale_of(u, NFA_SCALE_SOFTPLUS); }
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("affine_grad_host")
    cpp, so = str(d / "affine_grad_host.cpp"), str(d / "affine_grad_host.so")
    open(cpp, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "nflows_amd", "csrc"), cpp, "-o", so])
    lib = ctypes.CDLL(so)
    p = ctypes.c_void_p
    lib.host_affine_element_grad.argtypes = [ctypes.c_int64, p, p, p, p, ctypes.c_int, p, p, p]
    lib.host_affine_element_grad.restype = None
    lib.host_scale_of.argtypes = [ctypes.c_float]
    lib.host_scale_of.restype = ctypes.c_float
    return lib


def grid():
    """u over [-30, 30] (both sides of softplus1's u > 20 branch, and its edge), |x|, |g| up to 1e3 at every u."""
    g = torch.Generator().manual_seed(25)
    u = torch.cat((torch.linspace(-30.0, 30.0, 241), torch.tensor([20.0, 20.000002, 19.999998, 0.0, -0.0])))
    mags = torch.tensor([0.0, 1e-3, 0.3, 1.0, 7.0, 1e3])
    reps = 24
    u = u.repeat_interleave(reps)
    n = u.numel()

    def values():
        return mags[torch.randint(0, mags.numel(), (n,), generator=g)] * (2 * torch.rand(n, generator=g) - 1) * \
            torch.where(torch.rand(n, generator=g) < 0.5, 1.0, torch.rand(n, generator=g))

    return values(), u.float(), values(), values(), values()


@pytest.mark.parametrize("inverse", [False, True])
def test_affine_element_grad_against_float64_autograd(lib, inverse):
    x, u, shift, g_y, g_l = grid()
    truth = affine_element_truth(x, u, shift, g_y, g_l, inverse)
    ref32 = affine_element_truth(x, u, shift, g_y, g_l, inverse, dtype=torch.float32)
    # the kernel reads the layer's OUTPUT in the inverse direction: the float32 output the forward kernel wrote
    s32 = torch.nn.functional.softplus(u) + 1e-3
    other = ((x - shift) / s32) if inverse else x
    arrs = [np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (other, u, g_y, g_l)]
    n = u.numel()
    out = [np.empty(n, dtype=np.float32) for _ in range(3)]
    lib.host_affine_element_grad(n, *[a.ctypes.data for a in arrs], int(inverse), *[o.ctypes.data for o in out])
    for name, got, r, t in zip(("g_x", "g_u", "g_shift"), out, ref32, truth):
        assert np.isfinite(got).all(), name
        within_truth_rule(got, r.numpy(), t.numpy(), "%s %s" % ("inverse" if inverse else "forward", name))
    # the shift's gradient is g_y (forward) or -g_x (inverse) bit for bit
    want = -out[0] if inverse else arrs[2]
    assert np.array_equal(out[2].view(np.uint32), want.view(np.uint32))


def test_scale_gradient_is_exactly_one_where_softplus_returns_its_argument(lib):
    """u > 20: softplus1 returns u, so d scale / d u is 1 and g_u = g_y * x + g_l / s with no sigmoid factor."""
    u = np.array([20.5, 25.0, 30.0, 88.0], dtype=np.float32)
    x = np.array([3.0, -2.0, 0.5, 1.0], dtype=np.float32)
    g_y = np.array([1.5, 0.25, -4.0, 2.0], dtype=np.float32)
    g_l = np.array([0.5, -1.0, 2.0, 3.0], dtype=np.float32)
    out = [np.empty(4, dtype=np.float32) for _ in range(3)]
    lib.host_affine_element_grad(4, x.ctypes.data, u.ctypes.data, g_y.ctypes.data, g_l.ctypes.data, 0,
                                 *[o.ctypes.data for o in out])
    s = np.array([lib.host_scale_of(float(v)) for v in u], dtype=np.float32)
    assert np.array_equal(s, u + np.float32(1e-3))
    assert np.array_equal(out[1], g_y * x + g_l / s) and np.array_equal(out[0], g_y * s)
