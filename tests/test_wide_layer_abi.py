"""CPU-only checks of the argument contract of K32's entry point (nfa_rqs_layer_resnet_wide_f32), in the manner of
tests/test_whole_layer_abi.py: none of these paths reaches the device, so the library answers them through the C ABI with
null pointers."""
import ctypes

import pytest

from nflows_amd import _native as N
from nflows_amd import ops

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer (never read)


def call(batch=128, D=8, dt=4, di=4, hidden=256, blocks=2, K=8, tails="linear", flags=0, bufs=None):
    spec = ops.make_rqs_spec(K, tails, tail_bound=3.0)
    return N.load().nfa_rqs_layer_resnet_wide_f32(bufs, bufs, bufs, bufs, bufs, bufs, bufs, batch, D, dt, di, hidden, blocks,
                                                  ctypes.byref(spec), flags, None)


def test_entry_point_is_bound():
    assert "nfa_rqs_layer_resnet_wide_f32" in N.EXPORTS and N.load().nfa_abi_version() == N.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(), dict(hidden=129), dict(hidden=1), dict(K=2), dict(K=16), dict(D=128, dt=64, di=64)])
def test_batch_zero_is_a_no_op(kw):
    assert call(batch=0, **kw) == N.OK


@pytest.mark.parametrize("kw", [dict(batch=-128), dict(dt=0), dict(di=0), dict(blocks=-1), dict(D=0), dict(hidden=0),
                                dict(dt=12, D=8), dict(flags=1 << 20), dict(flags=N.FLAG_LOGITS_LOG2E),
                                dict(flags=N.ACTIVATION_TANH << N.FLAG_ACTIVATION_SHIFT), dict(flags=N.FLAG_SKIP_OUTPUTS)])
def test_invalid_arguments_come_first(kw):
    assert call(**kw) == N.ERR_INVALID_ARGUMENT
    # ... before a family limit, and batch 0 does not hide them
    assert call(**dict(dict(hidden=257, K=17), **kw)) == N.ERR_INVALID_ARGUMENT
    assert call(**dict(kw, batch=0 if "batch" not in kw else kw["batch"])) == N.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kw", [dict(hidden=257), dict(K=17), dict(K=1), dict(K=20), dict(dt=6), dict(D=132), dict(batch=100),
                                dict(tails=None), dict(blocks=65), dict(D=128, dt=4, di=68), dict(D=128, dt=68, di=4)])
def test_family_limits(kw):
    assert call(**kw) == N.ERR_UNSUPPORTED
    assert call(bufs=DUMMY, **kw) == N.ERR_UNSUPPORTED


def test_missing_buffers_inside_the_family():
    assert call() == N.ERR_INVALID_ARGUMENT
    assert call(flags=N.FLAG_STANDARD_NORMAL_LOG_PROB | N.FLAG_SKIP_OUTPUTS, bufs=DUMMY) == N.ERR_UNSUPPORTED
