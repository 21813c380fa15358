"""CPU-only checks of the argument contract of K34's entry point (nfa_rqs_layer_made_wide_f32), in the manner of
tests/test_wide_layer_abi.py: none of these paths reaches the device, so the library answers them through the C ABI with
null pointers."""
import ctypes

import pytest

from nflows_amd import _native as N
from nflows_amd import ops

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer (never read)


def call(batch=128, row_length=8, features=8, hidden=256, linears=4, K=10, tails="linear", flags=N.FLAG_RESIDUAL_BLOCKS,
         bufs=None):
    spec = ops.make_rqs_spec(K, tails, tail_bound=3.0)
    return N.load().nfa_rqs_layer_made_wide_f32(bufs, bufs, bufs, bufs, bufs, bufs, bufs, batch, row_length, features, hidden,
                                                linears, ctypes.byref(spec), flags, None)


def test_entry_point_is_bound():
    assert "nfa_rqs_layer_made_wide_f32" in N.EXPORTS and N.load().nfa_abi_version() == N.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(), dict(hidden=129), dict(K=2), dict(K=16), dict(row_length=64, features=63),
                                dict(flags=0, linears=3)])
def test_batch_zero_is_a_no_op(kw):
    assert call(batch=0, **kw) == N.OK


@pytest.mark.parametrize("kw", [dict(batch=-128), dict(features=0), dict(row_length=4), dict(hidden=0), dict(linears=-1),
                                dict(linears=3), dict(flags=1 << 20), dict(flags=N.FLAG_SKIP_OUTPUTS)])
def test_invalid_arguments_come_first(kw):
    assert call(**kw) == N.ERR_INVALID_ARGUMENT
    # ... before a family limit, and batch 0 does not hide them
    assert call(**dict(dict(hidden=257, K=17), **kw)) == N.ERR_INVALID_ARGUMENT
    assert call(**dict(kw, batch=0 if "batch" not in kw else kw["batch"])) == N.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kw", [dict(hidden=257), dict(row_length=68, features=65), dict(K=17), dict(K=1), dict(tails=None),
                                dict(flags=N.FLAG_RESIDUAL_BLOCKS | N.FLAG_INVERSE), dict(row_length=10), dict(batch=100)])
def test_family_limits(kw):
    assert call(**kw) == N.ERR_UNSUPPORTED
    assert call(bufs=DUMMY, **kw) == N.ERR_UNSUPPORTED


def test_missing_buffers_inside_the_family():
    assert call() == N.ERR_INVALID_ARGUMENT
