"""HouseholderSequence / SVDLinear / QRLinear / NaiveLinear without a GPU: the class surface, the parameters the kernel
reads, the C ABI's argument checks, and K24's per-row arithmetic -- nflows_amd/csrc/householder_math.hpp, the text the
kernels include -- compiled for the HOST (tests/_hostcore/householder_host.cpp) and held to the reference's vectors
(tests/golden/hh_*.npz, written by tests/golden/make_golden_householder.py) under the project's parity rule: `compare()`
of tests/test_gpu_headline_parity.py with OUT_TOL / LAD_TOL.  The triangular stage is K16's device code (lu_tri.hpp) and
is checked on the GPU only."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import LAD_TOL, OUT_TOL
from householder_cases import (ALL_CASES, CASES, GOLDEN, KINDS, LINEAR_CASES, case_id, case_inputs, golden, layer_of,
                               naive_golden, new_layer, state_of, truth)
from nflows_amd import _native as N
from nflows_amd.transforms import HouseholderSequence, NaiveLinear, QRLinear, SVDLinear
from test_gpu_headline_parity import compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "_hostcore", "householder_host.cpp")


def test_constructor_errors():
    for bad in (0, -3, 2.5, "4", None):
        with pytest.raises(TypeError, match="features must be a positive integer"):
            HouseholderSequence(bad, 2)
        with pytest.raises(TypeError, match="transforms must be a positive integer"):
            HouseholderSequence(4, bad)
        with pytest.raises(TypeError, match="positive integer"):
            SVDLinear(bad, 2)
        with pytest.raises(TypeError, match="positive integer"):
            QRLinear(bad, 2)
        with pytest.raises(TypeError, match="positive integer"):
            NaiveLinear(bad)
    with pytest.raises(AssertionError):
        SVDLinear(4, 3)          # an even number of reflections per sequence
    for t in (SVDLinear(4, 2), QRLinear(4, 2), NaiveLinear(4)):
        for bad in (1, "yes", None):
            with pytest.raises(TypeError, match="boolean"):
                t.use_cache(bad)


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_parameters_match_the_reference_layout_and_load(case):
    cls, features, count = case
    names = {"seq": ["q_vectors"],
             "svd": ["bias", "unconstrained_diagonal", "orthogonal_1.q_vectors", "orthogonal_2.q_vectors"],
             "qr": ["bias", "upper_entries", "log_upper_diag", "orthogonal.q_vectors"]}[cls]
    t = new_layer(cls, features, count)
    assert [n for n, _ in t.named_parameters()] == names and sorted(t.state_dict()) == sorted(names)
    for kind in KINDS:
        state = state_of(golden(cls, features, count, kind))
        assert sorted(state) == sorted(names)
        for n, p in t.named_parameters():
            assert tuple(p.shape) == tuple(state[n].shape), n
        t.load_state_dict(state, strict=True)
        for n, p in t.named_parameters():
            assert torch.equal(p.detach(), state[n])
    assert t.features == features
    if cls != "seq":
        assert t.using_cache is False
    if cls == "svd":
        assert t.eps == 1e-3 and t.identity_init is True
    if cls == "qr":
        assert np.array_equal(t.upper_indices, np.triu_indices(features, 1))


def test_initial_q_vectors_are_the_reference_s():
    with np.load(os.path.join(GOLDEN, "hh_init.npz")) as z:
        for key in z.files:
            features, count = (int(v) for v in key.split("_")[1:])
            assert np.array_equal(HouseholderSequence(features, count).q_vectors.detach().numpy(), z[key]), key
    e = torch.eye(6)
    assert torch.equal(HouseholderSequence(6, 3).q_vectors.detach(), torch.stack([e[0], e[0], e[1]]))
    assert torch.equal(HouseholderSequence(4, 1).q_vectors.detach(), torch.eye(4)[:1])
    assert torch.equal(HouseholderSequence(5, 4).matrix(), torch.eye(5))      # pairs cancel
    with pytest.raises(IndexError):
        HouseholderSequence(2, 5)     # the odd last vector's one at column 5 // 2 = 2: past the features, as the reference


def test_initialisation_of_the_linear_layers():
    t = SVDLinear(9, 4, eps=1e-3)
    assert not t.bias.any() and torch.all(t.unconstrained_diagonal == float(np.log(np.exp(1 - 1e-3) - 1)))
    assert torch.allclose(t.diagonal, torch.ones(9), atol=1e-6) and torch.allclose(t.log_diagonal, torch.zeros(9), atol=1e-6)
    assert torch.allclose(t.weight(), torch.eye(9), atol=1e-6) and abs(float(t.logabsdet().detach())) < 1e-5
    torch.manual_seed(0)
    bound = 1.0 / np.sqrt(64)
    t = SVDLinear(64, 2, identity_init=False)
    assert 0.8 * bound < t.unconstrained_diagonal.abs().max() <= bound and not t.bias.any()
    t = QRLinear(64, 3)
    assert 0.8 * bound < t.upper_entries.abs().max() <= bound and 0.8 * bound < t.log_upper_diag.abs().max() <= bound
    upper = t._create_upper()
    assert torch.equal(upper.tril(-1), torch.zeros(64, 64)) and torch.equal(torch.diagonal(upper), torch.exp(t.log_upper_diag))
    assert upper[3, 17] == t.upper_entries[3 * 64 - 3 * 4 // 2 + (17 - 3 - 1)]


@pytest.mark.parametrize("cls", ["svd", "qr", "naive"])
def test_weight_methods_and_cache_semantics(cls):
    torch.manual_seed(3)
    t = NaiveLinear(6) if cls == "naive" else new_layer(cls, 6, 4)
    with torch.no_grad():
        for p in t.parameters():
            p.add_(0.2 * torch.randn_like(p))
    t = t.double()
    w, wi = t.weight(), t.weight_inverse()
    assert torch.allclose(w @ wi, torch.eye(6, dtype=torch.float64), atol=1e-10)
    assert abs(float(t.logabsdet()) - float(torch.linalg.slogdet(w)[1])) < 1e-10
    wi2, lad2 = t.weight_inverse_and_logabsdet()
    assert torch.allclose(wi2, wi, atol=1e-12) and abs(float(lad2) - float(t.logabsdet())) < 1e-12
    assert t.cache.weight is None and t.cache.inverse is None and t.cache.logabsdet is None
    t.use_cache(True)
    t.eval()
    t._check_forward_cache()
    assert torch.equal(t.cache.weight, t.weight()) and t.cache.inverse is None and t.cache.logabsdet is not None
    t._check_inverse_cache()
    assert torch.allclose(t.cache.inverse, wi, atol=1e-12)
    kept = t.cache.weight
    t.eval()
    assert t.cache.weight is kept
    t.train()                     # going back to training drops it
    assert t.cache.weight is None and t.cache.inverse is None and t.cache.logabsdet is None and t.using_cache is True


def test_naive_linear_surface():
    from nflows_amd.utils import torchutils
    torch.manual_seed(1)
    q = torchutils.random_orthogonal(7)
    assert q.shape == (7, 7) and torch.allclose(q @ q.t(), torch.eye(7), atol=1e-5)
    m = torch.randn(5, 5, dtype=torch.float64)
    assert abs(float(torchutils.logabsdet(m)) - float(torch.log(torch.abs(torch.det(m))))) < 1e-12
    t = NaiveLinear(7)
    assert [n for n, _ in t.named_parameters()] == ["bias", "_weight"] and t.weight() is t._weight
    assert torch.allclose(t._weight @ t._weight.t(), torch.eye(7), atol=1e-5) and not t.bias.any()
    t = NaiveLinear(64, orthogonal_initialization=False)
    assert 0.8 / 8 < t._weight.abs().max() <= 1 / 8
    for features in (5, 64):
        g = naive_golden(features)
        t = NaiveLinear(features)
        t.load_state_dict(state_of(g), strict=True)
        assert abs(float(t.double().logabsdet()) - float(truth(g, "lad")[0])) < 1e-6


def test_cpu_inputs_raise():
    from nflows_amd import ops
    x = torch.zeros(3, 4)
    for t in (HouseholderSequence(4, 2), SVDLinear(4, 2), QRLinear(4, 2), NaiveLinear(4)):
        for call in (t, t.inverse):
            with pytest.raises(NotImplementedError, match="no CPU fallback"):
                call(x)
            with pytest.raises(NotImplementedError, match="no CPU fallback"):
                call(x.double())
        if not isinstance(t, HouseholderSequence):
            t.eval()
            t.use_cache(True)
            with pytest.raises(NotImplementedError, match="no CPU fallback"):
                t(x)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.householder(x, q_first=torch.ones(2, 4))


def test_abi_argument_errors_without_gpu():
    lib = N.load()
    assert lib.nfa_abi_version() == N.ABI_VERSION == 19
    null = None
    q = ctypes.c_void_p(16)   # a non-NULL pointer that no check dereferences

    def fwd(batch, features, ka=1, kb=0, eps=1e-3, flags=0, diag=null, upper=null, logd=null):
        return lib.nfa_householder_f32(null, null, ka, null, kb, diag, upper, logd, null, null, null, batch, features, eps,
                                       flags, null)

    def bwd(batch, features, ka=1, kb=0, eps=1e-3, flags=0, diag=null, upper=null, logd=null, x=null, partials=null):
        return lib.nfa_householder_backward_f32(x, null, null, ka, null, kb, diag, upper, logd, null, null, partials, batch,
                                                features, eps, flags, null)

    for call in (fwd, bwd):
        assert call(0, 64) == N.OK                            # an empty batch is a no-op
        assert call(0, 64, flags=N.FLAG_INVERSE) == N.OK
        assert call(0, 128, ka=128, kb=128) == N.OK
        assert call(-1, 64) == N.ERR_INVALID_ARGUMENT
        assert call(4, 0) == N.ERR_INVALID_ARGUMENT
        assert call(4, 64, ka=-1) == N.ERR_INVALID_ARGUMENT
        assert call(4, 64, kb=-2) == N.ERR_INVALID_ARGUMENT
        assert call(4, 1) == N.ERR_UNSUPPORTED                # 2 <= features <= 128
        assert call(4, 129) == N.ERR_UNSUPPORTED
        assert call(4, 64, ka=129) == N.ERR_UNSUPPORTED       # at most 128 reflections per sequence
        assert call(4, 64, kb=129) == N.ERR_UNSUPPORTED
        assert call(4, 64, eps=-1.0) == N.ERR_INVALID_ARGUMENT
        assert call(4, 64, diag=q, upper=q, logd=q) == N.ERR_INVALID_ARGUMENT   # one middle stage at the most
        assert call(4, 64, upper=q) == N.ERR_INVALID_ARGUMENT                   # R's two parts come together
        assert call(4, 64, logd=q) == N.ERR_INVALID_ARGUMENT
        assert call(4, 64) == N.ERR_INVALID_ARGUMENT          # NULL data with rows to process
        assert call(4, 64, flags=64) == N.ERR_INVALID_ARGUMENT
    assert fwd(0, 64, flags=N.FLAG_INVERSE | N.FLAG_ACCUMULATE_LOGABSDET) == N.OK
    assert bwd(0, 64, flags=N.FLAG_ACCUMULATE_LOGABSDET) == N.ERR_INVALID_ARGUMENT
    assert bwd(4, 64, x=q) == N.ERR_INVALID_ARGUMENT                      # inputs and partials come together
    assert bwd(4, 64, partials=q) == N.ERR_INVALID_ARGUMENT
    assert bwd(4, 64, x=q, partials=q, upper=q, logd=q) == N.ERR_UNSUPPORTED   # the reductions: no triangular stage
    assert lib.nfa_householder_backward_slabs(0, 64, 2, 2) == 0 and lib.nfa_householder_backward_slabs(4, 200, 2, 2) == 0


def test_dispatch_rule():
    """The class docstrings' rule -- the kernel wherever it serves -- as `kernel_serves` decides it."""
    from nflows_amd.transforms.orthogonal import kernel_serves
    q = torch.zeros(10, 64)
    x = torch.zeros(8, 64)
    assert kernel_serves(x, 64, q) and kernel_serves(x, 64, q, q)
    assert kernel_serves(torch.zeros(8, 128), 128, torch.zeros(128, 128)) and kernel_serves(torch.zeros(8, 2), 2, torch.zeros(1, 2))
    assert not kernel_serves(x.double(), 64, q.double()) and not kernel_serves(torch.zeros(2, 4, 64), 64, q)
    assert not kernel_serves(torch.zeros(8, 130), 130, torch.zeros(4, 130))
    assert not kernel_serves(torch.zeros(8, 1), 1, torch.zeros(2, 1))
    assert not kernel_serves(torch.zeros(8, 16), 16, torch.zeros(130, 16))
    # QRLinear, from the table of DESIGN.md section 4 "K24": forward calls of wide layers with one or two reflections were
    # measured slower on the kernel -- without autograd at 262 144 rows, under autograd at 16 384 -- and take the stock ops
    wide = QRLinear(128, 2)
    small, big = torch.zeros(16384, 128), torch.zeros(16385, 128)
    assert not wide._kernel_pays(small, False) and wide._kernel_pays(big, False)       # the parameters require grad
    assert wide._kernel_pays(small, True) and wide._kernel_pays(big, True)
    with torch.no_grad():
        assert wide._kernel_pays(small, False) and not wide._kernel_pays(big, False)
        assert wide._kernel_pays(big, True)
    for other in (QRLinear(128, 10), QRLinear(64, 2), QRLinear(16, 1)):
        rows = torch.zeros(16385, other.features)
        assert other._kernel_pays(rows, False) and other._kernel_pays(rows[:8], False)
        with torch.no_grad():
            assert other._kernel_pays(rows, False) and other._kernel_pays(rows[:8], False)


# ---------------------------------------------------------------------------------------------------------------------
# the per-row arithmetic, compiled for the host
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("householder_host") / "householder_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "nflows_amd", "csrc"), SRC, "-o", so])
    lib = ctypes.CDLL(so)
    p, i32 = ctypes.c_void_p, ctypes.c_int
    lib.host_householder.argtypes = [p, p, ctypes.c_int64, i32, p, i32, p, i32, p, p, ctypes.c_double, i32]
    lib.host_householder.restype = ctypes.c_float
    return lib


def host_call(lib, x, inverse, q_first=None, q_second=None, diag=None, bias=None, eps=1e-3):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    held = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (q_first, q_second, diag, bias)]
    ptr = [None if a is None else a.ctypes.data for a in held]
    lad = lib.host_householder(x.ctypes.data, out.ctypes.data, x.shape[0], x.shape[1], ptr[0],
                               0 if held[0] is None else held[0].shape[0], ptr[1], 0 if held[1] is None else held[1].shape[0],
                               ptr[2], ptr[3], eps, int(inverse))
    return out, np.float32(lad)


def host_layer(lib, cls, g, x, inverse):
    if cls == "seq":
        return host_call(lib, x, inverse, q_first=g["p/q_vectors"])
    q1, q2 = g["p/orthogonal_1.q_vectors"], g["p/orthogonal_2.q_vectors"]
    first, second = (q1, q2) if inverse else (q2, q1)
    return host_call(lib, x, inverse, q_first=first, q_second=second, diag=g["p/unconstrained_diagonal"], bias=g["p/bias"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [c for c in ALL_CASES if c[0] != "qr"], ids=case_id)
def test_row_arithmetic_parity_both_directions(lib, case, kind):
    cls, features, count = case
    g = golden(cls, features, count, kind)
    x, _ = case_inputs(cls, features, count, kind)
    y, lad = host_layer(lib, cls, g, x, False)
    xi, ladi = host_layer(lib, cls, g, g["y"], True)
    tag = "householder host %s D=%d K=%d %s" % (cls, features, count, kind)
    compare(tag, "y", y, g["y"], truth(g, "y"), OUT_TOL)
    compare(tag, "x", xi, g["xi"], truth(g, "xi"), OUT_TOL)
    if cls == "seq":
        assert lad == 0 and ladi == 0
    else:
        compare(tag, "logabsdet", np.array([lad]), g["lad"], truth(g, "lad"), LAD_TOL)
        compare(tag, "logabsdet(inverse)", np.array([ladi]), g["ladi"], truth(g, "ladi"), LAD_TOL)


@pytest.mark.parametrize("features,count", [(2, 2), (5, 4), (16, 10), (100, 100), (128, 128)])
def test_row_arithmetic_identity_initialisation_is_exact(lib, features, count):
    """Pairs of equal unit vectors cancel exactly and the initial diagonal rounds to 1: the inputs come back bit for bit."""
    x = np.random.RandomState(features).randn(257, features).astype(np.float32)
    t = SVDLinear(features, count)
    g = {"p/" + k: v.numpy() for k, v in t.state_dict().items()}
    for cls in ("svd", "seq"):
        gg = g if cls == "svd" else {"p/q_vectors": g["p/orthogonal_1.q_vectors"]}
        for inverse in (False, True):
            y, lad = host_layer(lib, cls, gg, x, inverse)
            assert np.array_equal(y, x) and abs(float(lad)) <= features * 6e-8


def test_row_arithmetic_zero_vector_gives_the_reference_s_non_finite_pattern(lib):
    x = np.random.RandomState(0).randn(9, 5).astype(np.float32)
    q = np.random.RandomState(1).randn(3, 5).astype(np.float32)
    q[1] = 0
    y, _ = host_call(lib, x, False, q_first=q)
    assert np.isnan(y).all()      # 2 / 0 = inf, inf * 0 = nan in every column, as (2 / |q|^2) q gives the reference
