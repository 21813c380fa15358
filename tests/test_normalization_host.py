"""BatchNorm / ActNorm and the two flow factories without a GPU: the class surface, the state the reference's checkpoints
hold, the factories' module trees and seeded weights, the C ABI's argument checks and the slab partition of K17's column
reduction (tests/golden/norm_*.npz: the reference's results, written by tests/golden/make_golden_norm.py)."""
import os

import numpy as np
import pytest
import torch

from nflows_amd import _native as N
from nflows_amd.flows import Flow, MaskedAutoregressiveFlow, SimpleRealNVP
from nflows_amd.transforms import ActNorm, BatchNorm, InverseNotAvailable, Transform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FEATURES = (2, 5, 64, 100, 128)


def small(stem, features):
    with np.load(os.path.join(GOLDEN, "norm_%s_d%d_small.npz" % (stem, features))) as z:
        return {k: z[k] for k in z.files}


def flow_fixture(key):
    with np.load(os.path.join(GOLDEN, "norm_flow_%s.npz" % key)) as z:
        return {k: z[k] for k in z.files}


def state_of(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g if k.startswith(prefix)}


def test_constructor_errors():
    for bad in (0, -3, 2.5, "4", None):
        with pytest.raises(TypeError, match="positive integer"):
            BatchNorm(bad)
        with pytest.raises(TypeError, match="positive integer"):
            ActNorm(bad)


def test_batch_norm_surface():
    t = BatchNorm(7)
    assert isinstance(t, Transform) and t.training
    assert list(dict(t.named_parameters())) == ["unconstrained_weight", "bias"]
    assert list(dict(t.named_buffers())) == ["running_mean", "running_var"]
    assert list(t.state_dict()) == ["unconstrained_weight", "bias", "running_mean", "running_var"]
    for v in t.state_dict().values():
        assert tuple(v.shape) == (7,) and v.dtype == torch.float32
    assert t.eps == 1e-5 and t.momentum == 0.1
    assert not t.bias.any() and not t.running_mean.any() and not t.running_var.any()   # the initial running variance is ZERO
    assert torch.all(t.unconstrained_weight == float(np.log(np.exp(1 - 1e-5) - 1)))
    assert torch.allclose(t.weight, torch.ones(7), atol=1e-6)
    t = BatchNorm(3, eps=1e-2, momentum=0.5, affine=False)    # `affine` is accepted and ignored
    assert sorted(t.state_dict()) == ["bias", "running_mean", "running_var", "unconstrained_weight"]
    assert t.eps == 1e-2 and t.momentum == 0.5 and torch.allclose(t.weight, torch.ones(3), atol=1e-6)
    assert torch.equal(t.weight, torch.nn.functional.softplus(t.unconstrained_weight) + 1e-2)
    assert BatchNorm.supports_fused_permutation and ActNorm.supports_fused_permutation


def test_act_norm_surface():
    t = ActNorm(6)
    assert list(dict(t.named_parameters())) == ["log_scale", "shift"]
    assert list(t.state_dict()) == ["log_scale", "shift", "initialized"]
    assert t.initialized.dtype == torch.bool and t.initialized.shape == () and not bool(t.initialized)
    assert not t.log_scale.any() and not t.shift.any() and torch.equal(t.scale, torch.ones(6))
    with torch.no_grad():
        t.log_scale.fill_(0.5)
    assert torch.equal(t.scale, torch.exp(t.log_scale))
    scale, shift = t._broadcastable_scale_shift(torch.zeros(2, 6, 3, 3))
    assert scale.shape == shift.shape == (1, 6, 1, 1)
    scale, shift = t._broadcastable_scale_shift(torch.zeros(2, 6))
    assert scale.shape == shift.shape == (1, 6)


@pytest.mark.parametrize("features", FEATURES)
def test_fixture_states_load_strictly(features):
    g = small("bn", features)
    t = BatchNorm(features)
    for after in ("after1_", "after3_"):
        state = {"unconstrained_weight": torch.from_numpy(g["unconstrained_weight"]), "bias": torch.from_numpy(g["bias"]),
                 "running_mean": torch.from_numpy(g[after + "running_mean"]),
                 "running_var": torch.from_numpy(g[after + "running_var"])}
        t.load_state_dict(state, strict=True)
        for k, v in state.items():
            assert torch.equal(getattr(t, k).detach(), v), k
    g = small("an", features)
    a = ActNorm(features)
    state = {"log_scale": torch.from_numpy(g["log_scale"]), "shift": torch.from_numpy(g["shift"]),
             "initialized": torch.tensor(True)}
    a.load_state_dict(state, strict=True)
    assert bool(a.initialized) and torch.equal(a.log_scale.detach(), state["log_scale"])
    # the fixture itself: the float32 and the float64 reference differ (a non-zero yardstick for the 2 x rule)
    assert np.abs(g["log_scale_d"]).max() > 0 and np.abs(small("bn", features)["after3_running_var_d"]).max() > 0


def test_rank_and_mode_errors_come_before_the_device_check():
    t = BatchNorm(4)
    for bad in (torch.zeros(4), torch.zeros(2, 4, 1), torch.zeros(2, 4, 3, 3)):
        with pytest.raises(ValueError, match="Expected 2-dim inputs"):
            t(bad)
    with pytest.raises(InverseNotAvailable, match="only available in eval mode"):
        t.inverse(torch.zeros(2, 4))
    t.eval()
    with pytest.raises(ValueError, match="Expected 2-dim inputs"):
        t.inverse(torch.zeros(2, 4, 1))
    a = ActNorm(4)
    for bad in (torch.zeros(4), torch.zeros(2, 4, 3)):
        with pytest.raises(ValueError, match="2D or a 4D"):
            a(bad)
        with pytest.raises(ValueError, match="2D or a 4D"):
            a.inverse(bad)


def test_cpu_inputs_raise():
    from nflows_amd import ops
    x = torch.zeros(3, 4)
    for t in (BatchNorm(4), ActNorm(4)):
        for mode in (t.train, t.eval):
            mode()
            with pytest.raises(NotImplementedError, match="no CPU fallback"):
                t(x)
            with pytest.raises(NotImplementedError, match="no CPU fallback"):
                t(x.double())
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            t.inverse(x)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ActNorm(4)(torch.zeros(2, 4, 3, 3))
    b = BatchNorm(4)
    assert not b.running_mean.any() and not b.running_var.any()       # a refused call has not touched the buffers
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.batch_norm(x, b.unconstrained_weight, b.bias, b.running_mean, b.running_var)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.act_norm(x, torch.zeros(4), torch.zeros(4))
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.column_stats(x)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.column_sums(x, x)


def build(key, **kw):
    if key == "maf":
        return MaskedAutoregressiveFlow(features=8, hidden_features=32, num_layers=3, num_blocks_per_layer=2, **kw)
    return SimpleRealNVP(features=16, hidden_features=32, num_layers=4, num_blocks_per_layer=2, **kw)


@pytest.mark.parametrize("key,seed", [("maf", 21), ("realnvp", 22)])
def test_factories_reproduce_the_reference_tree_and_weights(key, seed):
    g = flow_fixture(key)
    torch.manual_seed(seed)
    flow = build(key, batch_norm_between_layers=True)
    assert isinstance(flow, Flow)
    init = state_of(g, key + "/init/")
    assert sorted(flow.state_dict()) == sorted(init)
    for k, v in flow.state_dict().items():
        assert v.shape == init[k].shape and v.dtype == init[k].dtype, k
        assert torch.equal(v, init[k]), k          # same construction order: the seed gives the reference's weights
    for prefix in ("/start/", "/state/"):
        flow.load_state_dict(state_of(g, key + prefix), strict=True)
    layers = list(flow._transform._transforms)
    norms = [t for t in layers if isinstance(t, BatchNorm)]
    assert len(norms) == (3 if key == "maf" else 4) and all(t.running_var.abs().sum() > 0 for t in norms)
    assert len(layers) == (9 if key == "maf" else 8)


def test_factories_signatures_and_options():
    import inspect
    assert list(inspect.signature(SimpleRealNVP.__init__).parameters)[1:] == [
        "features", "hidden_features", "num_layers", "num_blocks_per_layer", "use_volume_preserving", "activation",
        "dropout_probability", "batch_norm_within_layers", "batch_norm_between_layers"]
    assert list(inspect.signature(MaskedAutoregressiveFlow.__init__).parameters)[1:] == [
        "features", "hidden_features", "num_layers", "num_blocks_per_layer", "use_residual_blocks", "use_random_masks",
        "use_random_permutations", "activation", "dropout_probability", "batch_norm_within_layers",
        "batch_norm_between_layers"]
    defaults = {k: v.default for k, v in inspect.signature(MaskedAutoregressiveFlow.__init__).parameters.items()}
    assert defaults["use_residual_blocks"] is True and defaults["use_random_masks"] is False
    assert defaults["batch_norm_between_layers"] is False and defaults["dropout_probability"] == 0.0
    from nflows_amd import configs
    from nflows_amd.transforms import (AdditiveCouplingTransform, AffineCouplingTransform, RandomPermutation,
                                       ReversePermutation)
    plain = build("realnvp")
    assert [type(t) for t in plain._transform._transforms] == [AffineCouplingTransform] * 4
    same = configs.simple_realnvp_flow(features=16, hidden_features=32, num_layers=4, num_blocks_per_layer=2, seed=5)
    torch.manual_seed(5)
    again = build("realnvp")
    assert all(torch.equal(a, b) for a, b in zip(same.state_dict().values(), again.state_dict().values()))
    additive = build("realnvp", use_volume_preserving=True)
    assert all(type(t) is AdditiveCouplingTransform for t in additive._transform._transforms)
    maf = build("maf", use_random_permutations=True)
    assert [type(t) for t in maf._transform._transforms][::2] == [RandomPermutation] * 3
    assert [type(t) for t in build("maf")._transform._transforms][::2] == [ReversePermutation] * 3


def test_abi_argument_errors_without_gpu():
    lib = N.load()
    assert lib.nfa_abi_version() == N.ABI_VERSION >= 16
    null = None

    def fmap(batch, features, eps=1e-5, kind=0, flags=0):
        return lib.nfa_norm_map_f32(null, null, null, null, null, null, null, null, null, null, batch, features, eps, kind,
                                    flags, null)

    def bmap(batch, features, eps=1e-5, kind=0, flags=0):
        return lib.nfa_norm_map_backward_f32(null, null, null, null, null, null, null, null, null, batch, features, eps,
                                             kind, flags, null)

    for call in (fmap, bmap):
        for kind in (0, 1):
            assert call(0, 64, kind=kind) == N.OK                     # an empty batch is a no-op
            assert call(0, 1024, kind=kind, flags=N.FLAG_INVERSE) == N.OK
            assert call(4, 64, kind=kind) == N.ERR_INVALID_ARGUMENT   # NULL data with rows to process
        assert call(-1, 64) == N.ERR_INVALID_ARGUMENT
        assert call(4, 0) == N.ERR_INVALID_ARGUMENT
        assert call(4, -5) == N.ERR_INVALID_ARGUMENT
        assert call(4, 1025) == N.ERR_UNSUPPORTED                     # 1 <= features <= 1024
        assert call(4, 64, eps=-1.0) == N.ERR_INVALID_ARGUMENT
        assert call(4, 64, kind=2) == N.ERR_INVALID_ARGUMENT
        assert call(4, 64, flags=64) == N.ERR_INVALID_ARGUMENT
    assert fmap(0, 64, flags=N.FLAG_INVERSE | N.FLAG_ACCUMULATE_LOGABSDET) == N.OK
    assert bmap(0, 64, flags=N.FLAG_ACCUMULATE_LOGABSDET) == N.ERR_INVALID_ARGUMENT

    def stats(batch, features, ws=null):
        return lib.nfa_norm_column_stats_f32(null, null, null, null, ws, batch, features, null)

    def sums(batch, features):
        return lib.nfa_norm_column_sums_f32(null, null, null, null, null, null, null, batch, features, null)

    def batch_grad(batch, features):
        return lib.nfa_norm_batch_backward_f32(null, null, null, null, null, null, null, batch, features, null)

    for call in (stats, sums, batch_grad):
        assert call(-1, 64) == N.ERR_INVALID_ARGUMENT
        assert call(4, 0) == N.ERR_INVALID_ARGUMENT
        assert call(4, 1025) == N.ERR_UNSUPPORTED
        assert call(4, 64) == N.ERR_INVALID_ARGUMENT                  # NULL data
    assert stats(1, 64) == N.ERR_UNSUPPORTED and stats(0, 64) == N.ERR_UNSUPPORTED   # batch statistics need two rows
    assert batch_grad(0, 64) == N.OK


# the partition of K17's column reduction (csrc/norm.hip: norm_slabs): 256 // D row lanes per workgroup at D <= 256 (one above),
# 32 rows per row lane and slab, at most 1024 // ceil(D / 256) slabs
def expected_slabs(batch, features):
    tiles = -(-features // 256)
    lanes = 256 // features if tiles == 1 else 1
    slabs = max(1, min(-(-batch // (lanes * 32)), 1024 // tiles))
    per_slab = -(-batch // slabs)
    return -(-batch // per_slab)


def test_slab_partition_depends_on_the_shape_only():
    lib = N.load()
    for features in (1, 2, 5, 64, 100, 128, 256, 257, 784, 1024):
        for batch in (2, 3, 63, 64, 65, 127, 128, 129, 1632, 1633, 4097, 32768, 131072, 131073, 262144):
            got = lib.nfa_norm_slab_count(batch, features)
            assert got == expected_slabs(batch, features), (batch, features)
            assert lib.nfa_norm_workspace_bytes(batch, features) == got * 2 * features * 8
    # the boundaries the GPU test sits on both sides of
    assert [lib.nfa_norm_slab_count(b, 5) for b in (1632, 1633)] == [1, 2]
    assert [lib.nfa_norm_slab_count(b, 64) for b in (128, 129)] == [1, 2]
    assert [lib.nfa_norm_slab_count(b, 64) for b in (131072, 131073, 262144)] == [1024, 1017, 1024]   # (129 rows per slab: empty slabs are dropped)
    assert lib.nfa_norm_slab_count(5, 1025) == 0 and lib.nfa_norm_workspace_bytes(-1, 4) == 0
