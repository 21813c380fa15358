"""CPU-only checks of the argument contract of every whole-layer entry point (K8, K8h, K8s, K8c, K8x, K11): the return
code for batch 0, bad arguments, each family limit and missing buffers.  None of these paths reaches the device, so the
library answers them through the C ABI with null pointers."""
import ctypes

import pytest

from nflows_amd import _native as N
from nflows_amd import ops

LOG2E = N.FLAG_LOGITS_LOG2E
NORMAL, SKIP = N.FLAG_STANDARD_NORMAL_LOG_PROB, N.FLAG_SKIP_OUTPUTS
UNKNOWN_FLAG = 1 << 20


def act(code):
    return code << N.FLAG_ACTIVATION_SHIFT


def pad(n):
    return n << N.FLAG_PAD_COLUMNS_SHIFT


_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer for the arguments the entry points check first (never read)


def applies(name, kw):
    return name != NO_LAYERS or "layers" not in kw


def base(**kw):
    p = dict(batch=128, D=8, dt=4, di=4, hidden=128, blocks=2, layers=2, K=8, tails="linear", beta=None, mbw=None, flags=0,
             ps=1, ce=4, act_scale=16.0, scale=N.SCALE_DEFAULT, bufs=None)
    p.update(kw)
    return p


def spec_of(p):
    s = ops.make_rqs_spec(p["K"], p["tails"], tail_bound=3.0)
    if p["beta"] is not None:
        s.softplus_beta = p["beta"]
    if p["mbw"] is not None:
        s.min_bin_width = p["mbw"]
    return s


# entry point -> (engine, call(lib, p)); `bufs` is the pointer every data buffer receives (None: null)
def _resnet(fn, extra=()):
    return lambda lib, p: getattr(lib, fn)(p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["layers"], p["bufs"], p["bufs"],
                                           p["bufs"], p["batch"], p["D"], p["dt"], p["di"], p["hidden"], p["blocks"],
                                           ctypes.byref(spec_of(p)), p["flags"], None, *extra)


def _coupling(lib, p):
    return lib.nfa_rqs_coupling_resnet_f32(p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["bufs"],
                                           p["batch"], p["D"], p["dt"], p["di"], p["hidden"], p["blocks"],
                                           ctypes.byref(spec_of(p)), p["flags"], None)


def _redo(lib, p):
    return lib.nfa_rqs_flow_resnet_redo_f32(p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["layers"], p["bufs"], p["bufs"],
                                            DUMMY, p["bufs"], p["batch"], p["D"], p["dt"], p["di"], p["hidden"],
                                            p["blocks"], ctypes.byref(spec_of(p)), p["flags"], None)


def _context(lib, p):
    return lib.nfa_rqs_flow_resnet_context_f32(p["bufs"], p["bufs"], p["ce"], p["bufs"], p["bufs"], p["bufs"],
                                               p["layers"], p["bufs"], p["bufs"], p["bufs"], p["batch"], p["D"], p["dt"],
                                               p["di"], p["hidden"], p["blocks"], ctypes.byref(spec_of(p)), p["flags"],
                                               None)


def _context_redo(lib, p):
    return lib.nfa_rqs_flow_resnet_context_redo_f32(p["bufs"], p["bufs"], p["ce"], p["bufs"], p["bufs"], p["bufs"],
                                                    p["layers"], p["bufs"], p["bufs"], DUMMY, p["bufs"], p["batch"],
                                                    p["D"], p["dt"], p["di"], p["hidden"], p["blocks"],
                                                    ctypes.byref(spec_of(p)), p["flags"], None)


def _stream(fn, extra=()):
    return lambda lib, p: getattr(lib, fn)(p["bufs"], p["bufs"], p["ps"], p["bufs"], p["layers"], p["bufs"], p["bufs"],
                                           p["bufs"], p["bufs"], p["batch"], p["D"], p["dt"], p["di"], p["hidden"],
                                           p["blocks"], ctypes.byref(spec_of(p)), p["flags"], None, *extra)


def _stream_context(lib, p):
    return lib.nfa_rqs_flow_resnet_context_f16x2_f32(p["bufs"], p["bufs"], p["ce"], p["bufs"], p["ps"], p["bufs"],
                                                     p["layers"], p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["batch"],
                                                     p["D"], p["dt"], p["di"], p["hidden"], p["blocks"],
                                                     ctypes.byref(spec_of(p)), p["flags"], None)


def _f16x3(fn, extra=()):
    return lambda lib, p: getattr(lib, fn)(p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["layers"], p["bufs"],
                                           p["bufs"], p["bufs"], p["bufs"], p["batch"], p["D"], p["dt"], p["di"],
                                           p["hidden"], p["blocks"], p["act_scale"], ctypes.byref(spec_of(p)),
                                           p["flags"], None, *extra)


def _affine(lib, p):
    return lib.nfa_affine_flow_mlp_f32(p["bufs"], p["bufs"], p["bufs"], p["bufs"], p["layers"], p["bufs"], p["bufs"],
                                       p["bufs"], p["batch"], p["D"], p["dt"], p["di"], p["hidden"], p["blocks"],
                                       p["scale"], p["flags"], None)


ENTRIES = {
    "nfa_rqs_coupling_resnet_f32": ("k8", _coupling),
    "nfa_rqs_flow_resnet_f32": ("k8", _resnet("nfa_rqs_flow_resnet_f32")),
    "nfa_rqs_flow_resnet_logits_f32": ("k8", _resnet("nfa_rqs_flow_resnet_logits_f32", (DUMMY,))),
    "nfa_rqs_flow_resnet_redo_f32": ("k8", _redo),
    "nfa_rqs_flow_resnet_context_f32": ("k8", _context),
    "nfa_rqs_flow_resnet_context_redo_f32": ("k8", _context_redo),
    "nfa_rqs_flow_resnet_f16x2_f32": ("k8h", _stream("nfa_rqs_flow_resnet_f16x2_f32")),
    "nfa_rqs_flow_resnet_f16x2_bins_f32": ("k8h", _stream("nfa_rqs_flow_resnet_f16x2_bins_f32", (DUMMY,))),
    "nfa_rqs_flow_resnet_f16x2_logits_f32": ("k8h", _stream("nfa_rqs_flow_resnet_f16x2_logits_f32", (DUMMY, DUMMY))),
    "nfa_rqs_flow_resnet_context_f16x2_f32": ("k8h", _stream_context),
    "nfa_rqs_flow_resnet_f16x2_tile16_f32": ("k8s", _stream("nfa_rqs_flow_resnet_f16x2_tile16_f32")),
    "nfa_rqs_flow_resnet_f16x2_tile16_bins_f32": ("k8s", _stream("nfa_rqs_flow_resnet_f16x2_tile16_bins_f32", (DUMMY,))),
    "nfa_rqs_flow_resnet_f16x2_colsplit_f32": ("k8c", _stream("nfa_rqs_flow_resnet_f16x2_colsplit_f32")),
    "nfa_rqs_flow_resnet_f16x3_f32": ("k8x", _f16x3("nfa_rqs_flow_resnet_f16x3_f32")),
    "nfa_rqs_flow_resnet_f16x3_logits_f32": ("k8x", _f16x3("nfa_rqs_flow_resnet_f16x3_logits_f32", (DUMMY,))),
    "nfa_affine_flow_mlp_f32": ("k11", _affine),
}
NO_LAYERS = "nfa_rqs_coupling_resnet_f32"   # (one layer: no num_layers argument)
SPLINE = [n for n, (e, _) in ENTRIES.items() if e != "k11"]
CONTEXT = ["nfa_rqs_flow_resnet_context_f32", "nfa_rqs_flow_resnet_context_redo_f32",
           "nfa_rqs_flow_resnet_context_f16x2_f32"]


@pytest.fixture(scope="module")
def lib():
    return N.load()


def test_every_whole_layer_entry_point_is_covered():
    names = [n for n in N.EXPORTS if n.startswith(("nfa_rqs_flow_resnet", "nfa_rqs_coupling_resnet"))]
    assert sorted(names + ["nfa_affine_flow_mlp_f32"]) == sorted(ENTRIES)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_batch_zero_is_a_no_op(lib, name):
    call = ENTRIES[name][1]
    assert call(lib, base(batch=0)) == N.OK
    # the density flags and their pad columns are not looked at before rows exist
    assert call(lib, base(batch=0, flags=NORMAL | SKIP | pad(7), D=8)) == N.OK


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_invalid_arguments(lib, name):
    engine, call = ENTRIES[name]
    bad = [dict(batch=-128), dict(dt=0), dict(di=0), dict(dt=-4), dict(layers=0), dict(blocks=-1), dict(D=0),
           dict(flags=UNKNOWN_FLAG), dict(flags=act(4)), dict(flags=act(7)),
           dict(flags=SKIP), dict(flags=pad(1)), dict(flags=NORMAL | N.FLAG_INVERSE),
           dict(flags=NORMAL | pad(7), D=4, dt=4, di=4, batch=128, bufs=DUMMY)]   # no density column left
    if engine == "k11":
        bad += [dict(dt=8, di=4, D=8), dict(flags=N.FLAG_RESIDUAL_BLOCKS, blocks=3), dict(flags=LOG2E)]
    else:
        bad += [dict(dt=12, D=8), dict(di=12, D=8), dict(flags=N.FLAG_RESIDUAL_BLOCKS)]
    if engine != "k8":
        bad.append(dict(flags=LOG2E))
    if engine in ("k8s", "k8c", "k11"):
        bad.append(dict(flags=act(N.ACTIVATION_TANH)))
    if engine in ("k8h", "k8s", "k8c"):
        bad += [dict(ps=0), dict(ps=5), dict(ps=1, blocks=16), dict(ps=-1)]
    if engine == "k8x":
        bad += [dict(act_scale=3.0), dict(act_scale=0.0), dict(act_scale=-16.0), dict(act_scale=float("nan"))]
    for kw in bad:
        if not applies(name, kw):
            continue
        assert call(lib, base(**kw)) == N.ERR_INVALID_ARGUMENT, kw
        if "bufs" not in kw:
            assert call(lib, base(batch=0, **{k: v for k, v in kw.items() if k != "batch"})) in (
                N.ERR_INVALID_ARGUMENT, N.OK), kw


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_invalid_before_unsupported_and_batch_zero(lib, name):
    engine, call = ENTRIES[name]
    # an argument error wins over a family limit, and batch 0 does not hide it
    for kw in [dict(flags=UNKNOWN_FLAG, hidden=64), dict(flags=act(5), batch=100), dict(dt=0, blocks=65),
               dict(flags=SKIP, batch=0), dict(layers=0, batch=0)]:
        if not applies(name, kw):
            continue
        assert call(lib, base(**kw)) == N.ERR_INVALID_ARGUMENT, kw


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_family_limits(lib, name):
    engine, call = ENTRIES[name]
    limits = [dict(hidden=64), dict(hidden=256), dict(D=132, dt=4, di=4), dict(D=10, dt=4, di=4), dict(batch=100),
              dict(batch=130), dict(blocks=65), dict(layers=4097), dict(D=128, dt=4, di=68), dict(D=128, dt=68, di=4)]
    if engine != "k11":
        limits += [dict(dt=6), dict(K=17), dict(K=33), dict(K=1), dict(beta=2.0)]
    if engine in ("k8s", "k8c"):
        limits += [dict(K=10), dict(K=4), dict(tails=None)]
    if engine in ("k8h", "k8x"):
        limits.append(dict(tails=None))
    if engine == "k8x":
        limits += [dict(flags=act(N.ACTIVATION_TANH)), dict(flags=act(N.ACTIVATION_LEAKY_RELU))]
    if engine == "k8h":
        limits.append(dict(K=4, flags=act(N.ACTIVATION_ELU)))
    if engine == "k8":
        limits += [dict(K=4, flags=act(N.ACTIVATION_ELU)), dict(K=10, flags=LOG2E), dict(K=8, flags=LOG2E | act(1))]
        if name != "nfa_rqs_flow_resnet_redo_f32":
            limits += [dict(tails=None, flags=act(N.ACTIVATION_TANH)), dict(tails=None, flags=LOG2E)]
    if engine == "k8c":
        limits.append(dict(ps=2))
    if engine == "k11":
        limits += [dict(scale=N.SCALE_GIVEN), dict(scale=N.SCALE_SOFTPLUS), dict(scale=99)]
    if name in CONTEXT:
        limits.append(dict(ce=61, di=4))
        if engine == "k8":
            limits.append(dict(flags=LOG2E))
        else:
            limits += [dict(ce=33, di=4), dict(D=128, dt=4, di=36, ce=4)]
    for kw in limits:
        if not applies(name, kw):
            continue
        assert call(lib, base(**kw)) == N.ERR_UNSUPPORTED, kw
        # a family limit is checked before batch 0 returns, except for the ragged batch itself
        if "batch" not in kw:
            assert call(lib, base(batch=0, **kw)) == N.ERR_UNSUPPORTED, kw


@pytest.mark.parametrize("name", sorted(SPLINE))
def test_spec_errors_come_before_family_limits(lib, name):
    call = ENTRIES[name][1]
    assert call(lib, base(batch=0, mbw=0.5)) == N.ERR_MIN_BIN_WIDTH
    assert call(lib, base(batch=0, mbw=0.5, hidden=64)) == N.ERR_MIN_BIN_WIDTH
    assert call(lib, base(mbw=0.5, batch=100)) == N.ERR_MIN_BIN_WIDTH
    assert call(lib, base(mbw=0.5, flags=UNKNOWN_FLAG)) == N.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_in_family_shape_with_null_buffers(lib, name):
    engine, call = ENTRIES[name]
    shapes = [dict(), dict(D=64, dt=32, di=32, blocks=0), dict(D=128, dt=64, di=64, blocks=2, layers=32, ps=2),
              dict(flags=N.FLAG_INVERSE), dict(flags=NORMAL | SKIP | pad(2)), dict(flags=N.FLAG_ACCUMULATE_LOGABSDET)]
    if engine == "k8c":   # (one parameter stage)
        shapes[2] = dict(D=128, dt=64, di=64, blocks=0, layers=32)
    if name in CONTEXT:
        shapes[2] = dict(D=128, dt=64, di=32, ce=32, blocks=2, layers=32, ps=2)
    if engine in ("k8", "k8h") or name == "nfa_rqs_flow_resnet_f16x3_f32":
        shapes += [dict(K=k) for k in (2, 3, 9, 10, 16, 20, 24, 32)]
    if engine in ("k8", "k8h"):
        shapes += [dict(K=10, flags=act(N.ACTIVATION_TANH)), dict(flags=act(N.ACTIVATION_ELU))]
    if engine == "k8h":
        shapes = [s for s in shapes if s.get("blocks", 2) <= 8]   # one parameter stage
        shapes.append(dict(D=128, dt=64, di=64 if name not in CONTEXT else 32, blocks=4, layers=32, ps=2))
    if engine == "k8" and name not in CONTEXT:
        shapes += [dict(K=8, flags=LOG2E), dict(tails=None, K=5)] if "redo" not in name and "logits" not in name else []
    if engine == "k11":
        shapes += [dict(dt=6, di=2), dict(scale=N.SCALE_ADDITIVE), dict(flags=N.FLAG_RESIDUAL_BLOCKS)]
    if name in CONTEXT:
        shapes += [dict(ce=1), dict(ce=28, di=4)]
    for kw in shapes:
        if not applies(name, kw):
            continue
        assert call(lib, base(**kw)) == N.ERR_INVALID_ARGUMENT, kw
        assert call(lib, base(batch=0, **kw)) == N.OK, kw


def test_entry_point_pointer_checks(lib):
    """The pointers an entry point needs beyond its launcher's (captures, redo words, context) are checked first."""
    null = None
    spec = ops.make_rqs_spec(8, "linear")
    s = ctypes.byref(spec)
    common = (128, 8, 4, 4, 128, 2)
    assert lib.nfa_rqs_flow_resnet_logits_f32(null, null, null, null, 2, null, null, null, 0, *common[1:], s, 0, null,
                                              null) == N.ERR_INVALID_ARGUMENT
    assert lib.nfa_rqs_flow_resnet_redo_f32(null, null, null, null, 2, null, null, null, null, 0, *common[1:], s, 0,
                                            null) == N.ERR_INVALID_ARGUMENT
    assert lib.nfa_rqs_flow_resnet_context_f32(null, null, 0, null, null, null, 2, null, null, null, 0, *common[1:], s,
                                               0, null) == N.ERR_INVALID_ARGUMENT
    assert lib.nfa_rqs_flow_resnet_context_redo_f32(null, null, 4, null, null, null, 2, null, null, null, null, 0,
                                                    *common[1:], s, 0, null) == N.ERR_INVALID_ARGUMENT
    assert lib.nfa_rqs_flow_resnet_context_f16x2_f32(null, null, -1, null, 1, null, 2, null, null, null, null, 0,
                                                     *common[1:], s, 0, null) == N.ERR_INVALID_ARGUMENT
    for fn in (lib.nfa_rqs_flow_resnet_f16x2_bins_f32, lib.nfa_rqs_flow_resnet_f16x2_tile16_bins_f32):
        assert fn(null, null, 1, null, 2, null, null, null, null, 0, *common[1:], s, 0, null, null) == \
            N.ERR_INVALID_ARGUMENT
    assert lib.nfa_rqs_flow_resnet_f16x2_logits_f32(null, null, 1, null, 2, null, null, null, null, 0, *common[1:], s, 0,
                                                    null, DUMMY, null) == N.ERR_INVALID_ARGUMENT
    assert lib.nfa_rqs_flow_resnet_f16x3_logits_f32(null, null, null, null, null, 2, null, null, null, null, 0,
                                                    *common[1:], 16.0, s, 0, null, null) == N.ERR_INVALID_ARGUMENT
