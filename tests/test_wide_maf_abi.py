"""CPU-only checks of the argument contract of K36's entry point (nfa_affine_layer_made_wide_f32), in the manner of
tests/test_wide_made_abi.py: none of these paths reaches the device, so the library answers them through the C ABI with
null pointers."""
import ctypes

import pytest

from nflows_amd import _native as N

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer (never read)


def call(batch=128, row_length=8, features=8, hidden=256, linears=4, context=0, flags=N.FLAG_RESIDUAL_BLOCKS, bufs=None,
         ctx_buf=None):
    return N.load().nfa_affine_layer_made_wide_f32(bufs, ctx_buf, context, bufs, bufs, bufs, bufs, bufs, bufs, batch,
                                                   row_length, features, hidden, linears, flags, None)


def test_entry_point_is_bound():
    assert "nfa_affine_layer_made_wide_f32" in N.EXPORTS and N.load().nfa_abi_version() == N.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(), dict(hidden=129), dict(context=1), dict(context=64, row_length=64, features=64),
                                dict(row_length=64, features=63), dict(flags=0, linears=3)])
def test_batch_zero_is_a_no_op(kw):
    assert call(batch=0, **kw) == N.OK


@pytest.mark.parametrize("kw", [dict(batch=-128), dict(features=0), dict(row_length=4), dict(hidden=0), dict(linears=-1),
                                dict(linears=3), dict(context=-1), dict(flags=1 << 20), dict(flags=N.FLAG_SKIP_OUTPUTS)])
def test_invalid_arguments_come_first(kw):
    assert call(**kw) == N.ERR_INVALID_ARGUMENT
    # ... before a family limit, and batch 0 does not hide them
    assert call(**dict(dict(hidden=257, context=65), **kw)) == N.ERR_INVALID_ARGUMENT
    assert call(**dict(kw, batch=0 if "batch" not in kw else kw["batch"])) == N.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kw", [dict(hidden=257), dict(hidden=128), dict(row_length=68, features=65), dict(context=65),
                                dict(flags=N.FLAG_RESIDUAL_BLOCKS | N.FLAG_INVERSE), dict(row_length=10), dict(batch=100)])
def test_family_limits(kw):
    assert call(**kw) == N.ERR_UNSUPPORTED
    assert call(bufs=DUMMY, ctx_buf=DUMMY, **kw) == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("kw", [dict(), dict(context=3, bufs=DUMMY)])   # (no buffer at all; all but the context's)
def test_missing_buffers_inside_the_family(kw):
    assert call(**kw) == N.ERR_INVALID_ARGUMENT
