"""The elementwise nonlinearity transforms without a GPU: the class surface, the state the reference's checkpoints hold, the
C ABI's argument checks and the row-sum plan of K18 (nflows_amd/csrc/launch_plan.hpp: plan_row_sum, compiled for the host
from the product's source).  Fixtures: tests/golden/nonlin_*.npz, written by tests/golden/make_golden_nonlin.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nflows_amd import _native as N
from nflows_amd import transforms as T
from nonlin_cases import GOLDEN, KINDS, SHAPES, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_constructor_errors():
    for name in ("Exp", "Tanh", "LogTanh", "LeakyReLU", "Sigmoid", "Logit", "GatedLinearUnit", "CauchyCDF", "CauchyCDFInverse",
                 "CompositeCDFTransform"):
        assert issubclass(getattr(T, name), T.Transform), name
    for bad in (0, -1, -0.5):
        with pytest.raises(ValueError, match=r"^Cut point must be positive\.$"):
            T.LogTanh(cut_point=bad)
        with pytest.raises(ValueError, match=r"^Slope must be positive\.$"):
            T.LeakyReLU(negative_slope=bad)
    sig = {n: list(inspect.signature(getattr(T, n).__init__).parameters.items())[1:] for n in
           ("LogTanh", "LeakyReLU", "Sigmoid", "Logit", "CauchyCDF", "CauchyCDFInverse", "CompositeCDFTransform")}
    assert [(k, v.default) for k, v in sig["LogTanh"]] == [("cut_point", 1)]
    assert [(k, v.default) for k, v in sig["LeakyReLU"]] == [("negative_slope", 1e-2)]
    assert [(k, v.default) for k, v in sig["Sigmoid"]] == [("temperature", 1), ("eps", 1e-6), ("learn_temperature", False)]
    assert [(k, v.default) for k, v in sig["Logit"]] == [("temperature", 1), ("eps", 1e-6)]
    assert [k for k, _ in sig["CauchyCDF"]] == [k for k, _ in sig["CauchyCDFInverse"]] == ["location", "scale", "features"]
    assert [k for k, _ in sig["CompositeCDFTransform"]] == ["squashing_transform", "cdf_transform"]


def test_state_and_structure():
    s = T.Sigmoid(temperature=2.5)
    assert list(dict(s.named_buffers())) == ["temperature"] and not list(s.parameters())
    assert s.temperature.shape == (1,) and s.temperature.dtype == torch.float32 and float(s.temperature[0]) == 2.5
    p = T.Sigmoid(temperature=2.5, learn_temperature=True)
    assert list(dict(p.named_parameters())) == ["temperature"] and not list(p.buffers())
    assert isinstance(p.temperature, torch.nn.Parameter) and p.temperature.shape == (1,) and p.eps == 1e-6
    logit = T.Logit(temperature=3, eps=1e-4)
    assert isinstance(logit, T.InverseTransform) and isinstance(logit._transform, T.Sigmoid)
    assert list(logit.state_dict()) == ["_transform.temperature"] and logit._transform.eps == 1e-4
    inv = T.CauchyCDFInverse()
    assert isinstance(inv, T.InverseTransform) and isinstance(inv._transform, T.CauchyCDF) and not inv.state_dict()
    for cls in (T.Exp, T.Tanh, T.LogTanh, T.LeakyReLU, T.CauchyCDF, T.GatedLinearUnit):
        assert not cls().state_dict()
    lt = T.LogTanh(cut_point=2)
    alpha = (1 - np.tanh(np.tanh(2))) / 2
    assert lt.cut_point == 2 and lt.inv_cut_point == np.tanh(2) and lt.alpha == alpha
    assert lt.beta == np.exp((np.tanh(2) - alpha * np.log(2)) / alpha)
    lr = T.LeakyReLU(0.2)
    assert lr.negative_slope == 0.2 and torch.equal(lr.log_negative_slope, torch.log(torch.as_tensor(0.2)))
    sq = T.Sigmoid()
    comp = T.CompositeCDFTransform(sq, T.PiecewiseRationalQuadraticCDF([5], tails=None))
    assert isinstance(comp, T.CompositeTransform) and len(comp._transforms) == 3
    assert comp._transforms[0] is sq and isinstance(comp._transforms[2], T.InverseTransform) and comp._transforms[2]._transform is sq
    assert [k for k in comp.state_dict() if "temperature" in k] == ["_transforms.0.temperature", "_transforms.2._transform.temperature"]
    # the new classes take no part in the composite's permutation folding
    for cls in (T.Exp, T.Tanh, T.LogTanh, T.LeakyReLU, T.Sigmoid, T.CauchyCDF, T.GatedLinearUnit, T.Logit):
        assert not getattr(cls, "supports_fused_permutation", False)


def test_reference_state_loads_strictly():
    with np.load(os.path.join(GOLDEN, "nonlin_flow.npz")) as z:
        state = {k[len("state/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("state/")}
    assert "_transform._transforms.0._transform.temperature" in state
    from nflows_amd.distributions import StandardNormal
    from nflows_amd.flows import Flow
    from nflows_amd.nn.nets import ResidualNet
    from nflows_amd.utils import torchutils
    layers = [T.Logit()]
    for i in range(2):
        layers.append(T.PiecewiseRationalQuadraticCouplingTransform(
            mask=torchutils.create_alternating_binary_mask(6, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=32, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=4.0))
        if i == 0:
            layers.append(T.ReversePermutation(6))
    flow = Flow(T.CompositeTransform(layers), StandardNormal([6]))
    flow.load_state_dict(state, strict=True)
    for k, v in flow.state_dict().items():
        assert torch.equal(v, state[k]), k
    # a learnable temperature's checkpoint loads into the Parameter, a fixed one's into the buffer, under the same key
    for learn in (False, True):
        t = T.Sigmoid(learn_temperature=learn)
        t.load_state_dict({"temperature": torch.tensor([2.5])}, strict=True)
        assert float(t.temperature.detach()[0]) == 2.5
    # every fixture is there, holds finite numbers and a non-zero yardstick somewhere
    for kind in KINDS:
        for shape in SHAPES:
            for part in ("fwd", "inv"):
                name = "nonlin_%s_n%s_%s.npz" % (kind, "x".join(map(str, shape[1:])), part)
                with np.load(os.path.join(GOLDEN, name)) as z:
                    assert all(np.isfinite(z[k]).all() for k in z.files), name
                    assert os.path.getsize(os.path.join(GOLDEN, name)) < 1 << 20


def test_cpu_inputs_raise():
    from nflows_amd import ops
    x = torch.rand(3, 4) * 0.8 + 0.1
    for kind in KINDS:
        t = make(kind)
        for value in (x, x.double(), x[0]):
            with pytest.raises(NotImplementedError, match="no CPU fallback"):
                t(value)
            with pytest.raises(NotImplementedError, match="no CPU fallback"):
                t.inverse(value)
    for t in (T.Logit(), T.CauchyCDFInverse(), T.CompositeCDFTransform(T.Sigmoid(), T.IdentityTransform())):
        with pytest.raises(NotImplementedError, match="no CPU fallback"):
            t(x)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        T.GatedLinearUnit()(x, context=torch.zeros(3, 1))
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        ops.nonlinearity(x, "exp")


def test_abi_version_and_argument_errors_without_gpu():
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "nflows_amd.h")).read()
    declared = int(re.search(r"#define NFA_ABI_VERSION (\d+)", header).group(1))
    assert declared == N.ABI_VERSION == lib.nfa_abi_version() and declared >= 17
    for name, code in (("EXP", N.NONLIN_EXP), ("TANH", N.NONLIN_TANH), ("LOG_TANH", N.NONLIN_LOG_TANH),
                       ("LEAKY_RELU", N.NONLIN_LEAKY_RELU), ("SIGMOID", N.NONLIN_SIGMOID), ("CAUCHY_CDF", N.NONLIN_CAUCHY_CDF)):
        assert int(re.search(r"#define NFA_NONLIN_%s (\d+)" % name, header).group(1)) == code
    null = None
    constants = {N.NONLIN_LOG_TANH: (1.0, 0.3, 2.0), N.NONLIN_LEAKY_RELU: (0.1, 0.0, 0.0), N.NONLIN_SIGMOID: (1e-6, 0.0, 0.0)}

    def fwd(batch, n, kind=0, flags=0, p=None):
        p = constants.get(kind, (0.0, 0.0, 0.0)) if p is None else p
        return lib.nfa_nonlin_f32(null, null, null, null, null, null, batch, n, kind, p[0], p[1], p[2], flags, null)

    def bwd(batch, n, kind=0, flags=0, p=None):
        p = constants.get(kind, (0.0, 0.0, 0.0)) if p is None else p
        return lib.nfa_nonlin_backward_f32(null, null, null, null, null, null, null, batch, n, kind, p[0], p[1], p[2], flags, null)

    for call in (fwd, bwd):
        for kind in range(6):
            assert call(0, 64, kind) == N.OK                               # an empty batch is a no-op
            assert call(4, 64, kind) == N.ERR_INVALID_ARGUMENT             # NULL data with rows to process
            assert call(4, 0, kind) == N.ERR_INVALID_ARGUMENT              # N < 1
            assert call(4, -3, kind) == N.ERR_INVALID_ARGUMENT
            assert call(-1, 64, kind) == N.ERR_INVALID_ARGUMENT
        for kind in (-1, 6, 99):
            assert call(0, 64, kind) == N.ERR_INVALID_ARGUMENT             # unknown kind
        assert call(0, 64, flags=64) == N.ERR_INVALID_ARGUMENT
        assert call(0, 64, flags=N.FLAG_INVERSE) == N.OK
        assert call(0, 64, N.NONLIN_LEAKY_RELU, p=(0.0, 0.0, 0.0)) == N.ERR_INVALID_ARGUMENT
        assert call(0, 64, N.NONLIN_LEAKY_RELU, p=(-0.1, 0.0, 0.0)) == N.ERR_INVALID_ARGUMENT
        assert call(0, 64, N.NONLIN_LOG_TANH, p=(0.0, 0.3, 2.0)) == N.ERR_INVALID_ARGUMENT
        assert call(0, 64, N.NONLIN_SIGMOID, p=(-1e-6, 0.0, 0.0)) == N.ERR_INVALID_ARGUMENT
    assert fwd(0, 64, flags=N.FLAG_INVERSE | N.FLAG_ACCUMULATE_LOGABSDET) == N.OK
    assert bwd(0, 64, flags=N.FLAG_ACCUMULATE_LOGABSDET) == N.ERR_INVALID_ARGUMENT


PLAN_SRC = r'''
#include "launch_plan.hpp"
extern "C" void row_plan(int64_t batch, int64_t n, int64_t* out) {
    const nfa::RowSumPlan p = nfa::plan_row_sum(batch, n);
    out[0] = p.rows; out[1] = p.group; out[2] = p.pieces; out[3] = p.piece; out[4] = p.groups; out[5] = p.vec4;
}
'''


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("row_plan_host")
    cpp, so = str(d / "row_plan_host.cpp"), str(d / "row_plan_host.so")
    open(cpp, "w").write(PLAN_SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "nflows_amd", "csrc"), cpp, "-o", so])
    lib = ctypes.CDLL(so)
    lib.row_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    lib.row_plan.restype = None

    def call(batch, n):
        out = (ctypes.c_int64 * 6)()
        lib.row_plan(batch, n, out)
        return dict(zip(("rows", "group", "pieces", "piece", "groups", "vec4"), out))
    return call


PLAN_SHAPES = [(s[0], int(np.prod(s[1:]))) for s in SHAPES] + [(262144, 64), (64, 12288), (262144, 784), (256, 3072), (1, 1),
                                                                  (3, 2048), (3, 2049), (5, 1 << 22)]


@pytest.mark.parametrize("batch,n", PLAN_SHAPES)
def test_row_sum_plan_covers_every_element_once_in_an_order_the_shape_fixes(plan, batch, n):
    p = plan(batch, n)
    lib = N.load()
    assert p == plan(batch, n)                                # a function of (batch, n)
    assert lib.nfa_nonlin_pieces(batch, n) == p["pieces"]     # ... and the library plans the same
    assert lib.nfa_nonlin_workspace_bytes(batch, n) == (batch * p["pieces"] * 8 if p["pieces"] > 1 else 0)
    assert lib.nfa_nonlin_backward_workspace_bytes(batch, n) == p["groups"] * 8
    if n <= 2048:
        R, G = p["rows"], p["group"]
        assert p["pieces"] == 1 and 1 <= R and R * n <= 2048 and (R + 1) * n > 2048 - 3 * n
        assert G & (G - 1) == 0 and 1 <= G <= 64 and 256 % G == 0 and (G == 64 or G * 8 >= n) and (G == 1 or G * 4 < n)
        # workgroup w takes rows [w R, min(batch, (w + 1) R)): the ranges tile [0, batch n) without gap or overlap
        starts = np.arange(p["groups"], dtype=np.int64) * R
        ends = np.minimum(starts + R, batch)
        assert starts[0] == 0 and ends[-1] == batch and np.array_equal(starts[1:], ends[:-1]) and (ends > starts).all()
        # a row's order of addition depends on n alone: the same rows / group for every batch
        for other in (1, 7, batch + 13):
            q = plan(other, n)
            assert (q["rows"], q["group"], q["vec4"]) == (R, G, p["vec4"])
        # float4 lanes only where every workgroup's range starts on a float4
        assert bool(p["vec4"]) == ((R * n) % 4 == 0)
        # lane g of a row's group adds terms g, g + G, ...: together every term once
        seen = np.zeros(n, dtype=np.int64)
        for g in range(G):
            seen[g::G] += 1
        assert (seen == 1).all()
    else:
        S, L = p["pieces"], p["piece"]
        assert p["rows"] == 0 and p["groups"] == batch * S and L % 4 == 0
        assert (S - 1) * L < n <= S * L and (S == 1 or L >= 1024)       # no empty piece, none shorter than half a tile
        assert S == 1 or batch * (S - 1) < 1024 + batch                  # rows are cut only to fill the device
        assert bool(p["vec4"]) == (n % 4 == 0)
        edges = np.minimum(np.arange(S + 1, dtype=np.int64) * L, n)
        assert edges[0] == 0 and edges[-1] == n and (np.diff(edges) > 0).all()
    assert 0 < p["groups"] < 2 ** 31


def test_row_sum_plan_regimes(plan):
    """Several rows per workgroup for small N, one row per workgroup up to a tile, pieces of a row beyond -- and the fixture
    shapes sit where the issue wants them."""
    assert plan(4093, 1) == {"rows": 2048, "group": 1, "pieces": 1, "piece": 0, "groups": 2, "vec4": 1}
    assert plan(4093, 5)["rows"] == 408 and plan(4093, 5)["group"] == 1 and plan(4093, 5)["vec4"] == 1
    assert plan(1021, 67)["rows"] == 28 and plan(1021, 67)["group"] == 16
    assert plan(381, 256)["rows"] == 8 and plan(381, 256)["group"] == 32
    assert plan(37, 105)["rows"] == 16 and plan(37, 105)["groups"] == 3
    assert plan(9, 2047) == {"rows": 1, "group": 64, "pieces": 1, "piece": 0, "groups": 9, "vec4": 0}
    assert plan(23, 4100)["pieces"] == 4 and plan(23, 4100)["piece"] == 1028 and plan(23, 4100)["groups"] == 92
    assert plan(64, 12288)["pieces"] == 12 and plan(64, 12288)["piece"] == 1024
    assert plan(262144, 4100)["pieces"] == 1                           # enough rows: nothing is cut
    assert plan(0, 5)["groups"] == 0 and plan(5, 0)["groups"] == 0
