"""OneByOneConvolution / SqueezeTransform without a GPU: the class surface, the state dict and the RNG order against
the reference's (tests/golden/conv1x1_c*_*.npz, squeeze.npz, conv_flow.npz; written by tests/golden/make_golden_conv.py),
and the argument checks of the two K19 entry points."""
import glob
import os

import numpy as np
import pytest
import torch

from nflows_amd import _native as N
from nflows_amd.transforms import LULinear, OneByOneConvolution, SqueezeTransform

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = ("lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")
KEYS = PARAMS + ("permutation._permutation",)
CHANNELS = (2, 3, 12, 48, 100, 128)


def golden(channels):
    merged = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "conv1x1_c%d_*_out.npz" % channels))):
        with np.load(path) as z:
            merged.update({k: z[k] for k in z.files})
    assert merged, "no fixture for %d channels" % channels
    return merged


def test_constructor_and_rank_errors():
    for bad in (0, -3, 2.5, "4", None):
        with pytest.raises(TypeError, match="positive integer"):
            OneByOneConvolution(bad)
    t = OneByOneConvolution(4)
    assert isinstance(t, LULinear) and t.features == 4 and t.eps == 1e-3 and t.using_cache is False
    assert OneByOneConvolution(4, True).using_cache is True
    for shape in ((4,), (3, 4), (3, 4, 5), (2, 4, 3, 3, 1)):
        for call in (t, t.forward, t.inverse):
            with pytest.raises(ValueError, match="Inputs must be a 4D tensor."):
                call(torch.zeros(shape))
    with pytest.raises(ValueError, match="4 channels"):
        t(torch.zeros(2, 5, 3, 3))
    for call in (t, t.inverse):   # a CPU tensor of the right shape: the package's usual refusal
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            call(torch.zeros(2, 4, 3, 3))
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            call(torch.zeros(2, 4, 3, 3, dtype=torch.float64))


@pytest.mark.parametrize("channels", CHANNELS)
def test_state_dict_matches_the_reference_and_loads(channels):
    g = golden(channels)
    t = OneByOneConvolution(channels)
    assert list(dict(t.named_parameters())) == ["bias", "lower_entries", "upper_entries", "unconstrained_upper_diag"]
    assert list(t.state_dict()) == ["bias", "lower_entries", "upper_entries", "unconstrained_upper_diag",
                                    "permutation._permutation"]
    for kind in ("rand", "trained"):
        state = {n: torch.from_numpy(g["%s/%s" % (kind, n)]) for n in KEYS}
        t.load_state_dict(state, strict=True)
        for n in PARAMS:
            assert torch.equal(getattr(t, n).detach(), state[n]), n
        assert torch.equal(t.permutation._permutation, state["permutation._permutation"])
        assert t.permutation._permutation.dtype == torch.int64 and t.permutation._dim == 1


@pytest.mark.parametrize("channels", CHANNELS)
def test_global_rng_is_consumed_in_the_reference_order(channels):
    """The permutation is drawn AFTER the parent's parameters: with the generator's seed the random initialisation and
    the permutation are the reference's, to the bit."""
    g = golden(channels)
    torch.manual_seed(channels * 7)            # make_golden_conv.py: layer_seed(channels, "rand")
    t = OneByOneConvolution(channels, identity_init=False)
    for n in KEYS[:3] + KEYS[4:]:
        got = t.state_dict()[n]
        assert torch.equal(got, torch.from_numpy(g["rand/" + n])), n
    torch.manual_seed(channels * 7 + 1)        # "trained": identity initialisation draws nothing before the permutation
    t = OneByOneConvolution(channels)
    assert torch.equal(t.permutation._permutation, torch.from_numpy(g["trained/permutation._permutation"]))
    assert sorted(t.permutation._permutation.tolist()) == list(range(channels))


def test_never_offered_a_fused_outer_permutation():
    from nflows_amd.transforms.base import _accepts_fused_permutation
    t = OneByOneConvolution(4)
    assert not _accepts_fused_permutation(t, torch.zeros(3, 4))
    assert not _accepts_fused_permutation(t, torch.zeros(3, 4, 2, 2))


def test_flow_fixture_state_dict_loads():
    from nflows_amd.nn.nets import ConvResidualNet
    from nflows_amd.transforms import ActNorm, CompositeTransform, PiecewiseRationalQuadraticCouplingTransform
    from nflows_amd.utils.torchutils import create_alternating_binary_mask
    g = np.load(os.path.join(GOLDEN, "conv_flow.npz"))
    ts = [SqueezeTransform(2)]
    for i in range(2):
        ts += [ActNorm(12), OneByOneConvolution(12), PiecewiseRationalQuadraticCouplingTransform(
            mask=create_alternating_binary_mask(12, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ConvResidualNet(i_, o_, hidden_channels=8, num_blocks=1),
            num_bins=4, tails="linear", tail_bound=3.0)]
    flow = CompositeTransform(ts)
    state = {k[len("state/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("state/")}
    assert sorted(state) == sorted(flow.state_dict())
    flow.load_state_dict(state, strict=True)
    assert "_transforms.2.permutation._permutation" in state


def test_squeeze_errors_and_output_shape():
    for bad in (1, 0, -2, 2.0, "2", None):
        with pytest.raises(ValueError, match="Factor must be an integer > 1."):
            SqueezeTransform(bad)
    t = SqueezeTransform()
    assert t.factor == 2 and t.get_output_shape(3, 8, 6) == (12, 4, 3)
    assert SqueezeTransform(3).get_output_shape(2, 9, 6) == (18, 3, 2)
    assert SqueezeTransform(4).get_output_shape(1, 9, 6) == (16, 2, 1)   # floor division, as the reference
    for shape in ((4,), (3, 4), (3, 4, 4), (2, 4, 4, 4, 1)):
        for call in (t.forward, t.inverse):
            with pytest.raises(ValueError, match="Expecting inputs with 4 dimensions"):
                call(torch.zeros(shape))
    for shape in ((2, 3, 5, 4), (2, 3, 4, 5)):
        with pytest.raises(ValueError, match="Input image size not compatible with the factor."):
            t(torch.zeros(shape))
    for channels in (1, 2, 3, 6, 18):       # the reference's check is c % 4, whatever the factor
        for u in (t, SqueezeTransform(3)):
            with pytest.raises(ValueError, match="Invalid number of channel dimensions."):
                u.inverse(torch.zeros(2, channels, 3, 3))
    with np.load(os.path.join(GOLDEN, "squeeze.npz")) as g:
        assert str(g["f2/inverse_raises"]) == "" and str(g["f3/inverse_raises"]) == "Invalid number of channel dimensions."
    for call, shape in ((t.forward, (2, 3, 4, 6)), (t.inverse, (2, 12, 2, 3))):
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            call(torch.zeros(shape))


def test_abi_argument_errors_without_gpu():
    lib = N.load()
    assert lib.nfa_abi_version() == N.ABI_VERSION >= 18
    assert "nfa_lu_conv1x1_f32" in N.EXPORTS and "nfa_lu_conv1x1_backward_f32" in N.EXPORTS
    null = None

    def fwd(batch, channels, height=4, width=4, eps=1e-3, flags=0):
        return lib.nfa_lu_conv1x1_f32(null, null, null, null, null, null, null, null, null, batch, channels, height,
                                      width, eps, flags, null)

    def bwd(batch, channels, height=4, width=4, eps=1e-3, flags=0):
        return lib.nfa_lu_conv1x1_backward_f32(null, null, null, null, null, null, null, batch, channels, height, width,
                                               eps, flags, null)

    for call in (fwd, bwd):
        assert call(0, 12) == N.OK                            # an empty batch is a no-op
        assert call(0, 12, flags=N.FLAG_INVERSE) == N.OK
        assert call(-1, 12) == N.ERR_INVALID_ARGUMENT
        assert call(4, 0) == N.ERR_INVALID_ARGUMENT
        assert call(4, -5) == N.ERR_INVALID_ARGUMENT
        for height, width in ((0, 4), (4, 0), (-1, 4), (4, -7)):
            assert call(4, 12, height, width) == N.ERR_INVALID_ARGUMENT
            assert call(0, 12, height, width) == N.ERR_INVALID_ARGUMENT
        assert call(4, 1) == N.ERR_UNSUPPORTED                # 2 <= channels <= 128
        assert call(4, 129) == N.ERR_UNSUPPORTED
        assert call(4, 12, eps=-1.0) == N.ERR_INVALID_ARGUMENT
        assert call(4, 12) == N.ERR_INVALID_ARGUMENT          # NULL data with pixels to process
        assert call(4, 12, flags=64) == N.ERR_INVALID_ARGUMENT
    assert fwd(0, 12, flags=N.FLAG_INVERSE | N.FLAG_ACCUMULATE_LOGABSDET) == N.OK
    assert bwd(0, 12, flags=N.FLAG_ACCUMULATE_LOGABSDET) == N.ERR_INVALID_ARGUMENT


def test_cpu_tensors_raise_in_the_functional():
    from nflows_amd import ops
    t = OneByOneConvolution(4)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.lu_conv1x1(torch.zeros(2, 4, 3, 3), t.lower_entries, t.upper_entries, t.unconstrained_upper_diag, t.bias)
