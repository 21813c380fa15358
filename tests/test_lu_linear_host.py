"""LULinear / Linear without a GPU: the class surface, the parameter layout the kernel reads, the C ABI's argument
checks (tests/golden/lu_linear_d*_*.npz: the reference's parameters, written by tests/golden/make_golden_lu.py)."""
import os

import numpy as np
import pytest
import torch

from nflows_amd import _native as N
from nflows_amd.transforms import Linear, LULinear
from nflows_amd.transforms.lu import lower_entry_index, upper_entry_index

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = ("lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")


def golden(features):
    """All parts of both parameter sets of one D, merged (tests/golden/lu_linear_d{D}_{kind}_{part}.npz)."""
    import glob
    merged = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "lu_linear_d%d_*.npz" % features))):
        with np.load(path) as z:
            merged.update({k: z[k] for k in z.files})
    assert merged, "no fixture for %d features" % features
    return merged


def test_constructor_errors():
    for bad in (0, -3, 2.5, "4", None):
        with pytest.raises(TypeError, match="positive integer"):
            LULinear(bad)
        with pytest.raises(TypeError, match="positive integer"):
            Linear(bad)
    t = LULinear(4)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="boolean"):
            t.use_cache(bad)
    base = Linear(3)
    for method in (base.weight, base.weight_inverse, base.logabsdet):
        with pytest.raises(NotImplementedError):
            method()
    with pytest.raises(NotImplementedError):
        base.forward_no_cache(torch.zeros(1, 3))
    with pytest.raises(NotImplementedError):
        base.inverse_no_cache(torch.zeros(1, 3))


@pytest.mark.parametrize("features", [2, 5, 64, 100, 128])
def test_parameters_match_the_reference_layout_and_load(features):
    g = golden(features)
    t = LULinear(features)
    assert list(dict(t.named_parameters())) == ["bias", "lower_entries", "upper_entries", "unconstrained_upper_diag"]
    assert sorted(t.state_dict()) == sorted(PARAMS)
    for kind in ("rand", "trained"):
        state = {n: torch.from_numpy(g["%s/%s" % (kind, n)]) for n in PARAMS}
        for n in PARAMS:
            assert tuple(getattr(t, n).shape) == tuple(state[n].shape), n
        t.load_state_dict(state, strict=True)
        for n in PARAMS:
            assert torch.equal(getattr(t, n).detach(), state[n])
    assert t.features == features and t.eps == 1e-3 and t.using_cache is False


def test_identity_initialisation():
    t = LULinear(37, identity_init=True, eps=1e-3)
    assert not t.lower_entries.any() and not t.upper_entries.any() and not t.bias.any()
    assert torch.all(t.unconstrained_upper_diag == float(np.log(np.exp(1 - 1e-3) - 1)))
    assert torch.allclose(t.upper_diag, torch.ones(37), atol=1e-6)
    assert torch.allclose(t.weight(), torch.eye(37), atol=1e-6) and abs(float(t.logabsdet())) < 1e-4
    t = LULinear(8, eps=0.25)   # eps is folded into the logit: the diagonal is 1 whatever eps
    assert torch.allclose(t.upper_diag, torch.ones(8), atol=1e-6)


def test_random_initialisation_statistics():
    torch.manual_seed(0)
    features = 96
    t = LULinear(features, identity_init=False)
    bound = 1.0 / np.sqrt(features)
    assert not t.bias.any()
    for n in PARAMS[:3]:
        p = getattr(t, n).detach()
        assert p.abs().max() <= bound and p.abs().max() > 0.8 * bound, n
        assert abs(float(p.mean())) < 4 * bound / np.sqrt(3 * p.numel()) + 1e-3, n   # uniform: sd = bound / sqrt(3)
    for n in PARAMS[:2]:
        sd = float(getattr(t, n).detach().std())
        assert abs(sd - bound / np.sqrt(3)) < 0.05 * bound, n


@pytest.mark.parametrize("features", list(range(2, 129)))
def test_index_formulas_are_numpy_triangle_order(features):
    """What the kernel computes to find L[i, j] / U[i, j] in the flat parameters."""
    rows, cols = np.tril_indices(features, -1)
    assert np.array_equal(lower_entry_index(rows, cols), np.arange(rows.size))
    rows, cols = np.triu_indices(features, 1)
    assert np.array_equal(upper_entry_index(rows, cols, features), np.arange(rows.size))
    t = LULinear(features)
    assert np.array_equal(t.lower_indices, np.tril_indices(features, -1))
    assert np.array_equal(t.upper_indices, np.triu_indices(features, 1))


def test_dense_factors_and_weight_methods():
    g = golden(5)
    t = LULinear(5)
    t.load_state_dict({n: torch.from_numpy(g["trained/" + n]) for n in PARAMS})
    t = t.double()
    lower, upper = t._create_lower_upper()
    assert torch.equal(torch.diagonal(lower), torch.ones(5, dtype=torch.float64))
    assert torch.equal(lower.triu(1), torch.zeros_like(lower)) and torch.equal(upper.tril(-1), torch.zeros_like(upper))
    assert lower[3, 1] == t.lower_entries[lower_entry_index(3, 1)]
    assert upper[1, 4] == t.upper_entries[upper_entry_index(1, 4, 5)]
    assert torch.equal(torch.diagonal(upper), torch.nn.functional.softplus(t.unconstrained_upper_diag) + 1e-3)
    w, wi = t.weight(), t.weight_inverse()
    assert torch.allclose(w @ wi, torch.eye(5, dtype=torch.float64), atol=1e-12)
    assert abs(float(t.logabsdet()) - float(torch.linalg.slogdet(w)[1])) < 1e-12
    assert abs(float(t.logabsdet()) - (float(g["trained/lad"][0]) + float(g["trained/lad_d"][0]))) < 1e-12
    w2, lad = t.weight_and_logabsdet()
    wi2, lad2 = t.weight_inverse_and_logabsdet()
    assert torch.equal(w2, w) and torch.equal(wi2, wi) and lad == lad2 == t.logabsdet()


def test_cache_semantics():
    t = LULinear(6, identity_init=False)
    assert t.using_cache is False and t.cache.weight is None and t.cache.inverse is None and t.cache.logabsdet is None
    t.use_cache(True)
    assert t.using_cache is True
    t.eval()
    t._check_forward_cache()
    assert torch.equal(t.cache.weight, t.weight()) and torch.equal(t.cache.logabsdet, t.logabsdet())
    assert t.cache.inverse is None
    t._check_inverse_cache()
    assert torch.equal(t.cache.inverse, t.weight_inverse())
    kept = t.cache.weight
    t.eval()                      # staying in eval mode keeps the cache
    assert t.cache.weight is kept
    t.cache.logabsdet = None      # a single missing entry is refilled alone
    t._check_forward_cache()
    assert t.cache.weight is kept and t.cache.logabsdet is not None
    t.train()                     # going back to training drops it
    assert t.cache.weight is None and t.cache.inverse is None and t.cache.logabsdet is None
    assert t.using_cache is True
    t.use_cache(False)
    assert t.using_cache is False


def test_abi_argument_errors_without_gpu():
    lib = N.load()
    assert lib.nfa_abi_version() == N.ABI_VERSION >= 15
    null = None

    def fwd(batch, features, eps=1e-3, flags=0):
        return lib.nfa_lu_linear_f32(null, null, null, null, null, null, null, null, null, null, batch, features, eps,
                                     flags, null)

    def bwd(batch, features, eps=1e-3, flags=0):
        return lib.nfa_lu_linear_backward_f32(null, null, null, null, null, null, null, null, batch, features, eps, flags,
                                              null)

    for call in (fwd, bwd):
        assert call(0, 64) == N.OK                            # an empty batch is a no-op
        assert call(0, 64, flags=N.FLAG_INVERSE) == N.OK
        assert call(-1, 64) == N.ERR_INVALID_ARGUMENT
        assert call(4, 0) == N.ERR_INVALID_ARGUMENT
        assert call(4, -5) == N.ERR_INVALID_ARGUMENT
        assert call(4, 1) == N.ERR_UNSUPPORTED                # 2 <= features <= 128
        assert call(4, 129) == N.ERR_UNSUPPORTED
        assert call(4, 64, eps=-1.0) == N.ERR_INVALID_ARGUMENT
        assert call(4, 64) == N.ERR_INVALID_ARGUMENT          # NULL data with rows to process
        assert call(4, 64, flags=64) == N.ERR_INVALID_ARGUMENT
    assert fwd(0, 64, flags=N.FLAG_INVERSE | N.FLAG_ACCUMULATE_LOGABSDET) == N.OK
    assert bwd(0, 64, flags=N.FLAG_ACCUMULATE_LOGABSDET) == N.ERR_INVALID_ARGUMENT


def test_cpu_inputs_raise():
    from nflows_amd import ops
    t = LULinear(4)
    x = torch.zeros(3, 4)
    for call in (t, t.inverse, t.forward_no_cache, t.inverse_no_cache):
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            call(x)
    t.eval()
    t.use_cache(True)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        t(x)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        t(x.double())
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.lu_linear(x, t.lower_entries, t.upper_entries, t.unconstrained_upper_diag, t.bias)
