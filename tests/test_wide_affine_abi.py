"""CPU-only checks of the argument contract of K37's entry point (nfa_affine_layer_resnet_wide_f32), in the manner of
tests/test_wide_layer_abi.py: none of these paths reaches the device, so the library answers them through the C ABI with
null pointers."""
import ctypes
import os

import pytest

from nflows_amd import _native as N

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer (never read)
RESNET = N.FLAG_RESIDUAL_BLOCKS


def call(batch=128, D=8, dt=4, di=4, hidden=256, layers=2, scale=N.SCALE_DEFAULT, flags=RESNET, bufs=None):
    return N.load().nfa_affine_layer_resnet_wide_f32(bufs, bufs, bufs, bufs, bufs, bufs, bufs, batch, D, dt, di, hidden, layers,
                                                     scale, flags, None)


def test_entry_point_is_bound_and_declared():
    assert "nfa_affine_layer_resnet_wide_f32" in N.EXPORTS and N.load().nfa_abi_version() == N.ABI_VERSION
    header = os.path.join(os.path.dirname(__file__), "..", "include", "nflows_amd.h")
    assert "int nfa_affine_layer_resnet_wide_f32(" in open(header).read()


@pytest.mark.parametrize("kw", [dict(), dict(hidden=129), dict(hidden=1), dict(scale=N.SCALE_ADDITIVE), dict(scale=N.SCALE_GENERAL),
                                dict(D=128, dt=64, di=64), dict(dt=3, di=1, D=4), dict(flags=0, layers=3)])
def test_batch_zero_is_a_no_op(kw):
    assert call(batch=0, **kw) == N.OK


@pytest.mark.parametrize("kw", [dict(batch=-128), dict(dt=0), dict(di=0), dict(layers=-1), dict(layers=3), dict(D=0), dict(hidden=0),
                                dict(dt=6, D=8), dict(flags=1 << 20), dict(flags=N.FLAG_SKIP_OUTPUTS)])
def test_invalid_arguments_come_first(kw):
    assert call(**kw) == N.ERR_INVALID_ARGUMENT
    # ... before a family limit, and batch 0 does not hide them
    assert call(**dict(dict(hidden=257, scale=N.SCALE_GIVEN), **kw)) == N.ERR_INVALID_ARGUMENT
    assert call(**dict(kw, batch=0 if "batch" not in kw else kw["batch"])) == N.ERR_INVALID_ARGUMENT


# (the LDS sum -- exchange buffer, row tile, shares -- is at most 132 608 B inside the other limits: the row tile's limit,
#  features <= 128, is what a caller can reach of "the sum does not fit")
@pytest.mark.parametrize("kw", [dict(hidden=257), dict(D=128, dt=4, di=65), dict(D=128, dt=65, di=4), dict(scale=N.SCALE_GIVEN),
                                dict(scale=N.SCALE_SOFTPLUS), dict(D=132), dict(D=10), dict(batch=100), dict(layers=130),
                                dict(flags=RESNET | N.FLAG_STANDARD_NORMAL_LOG_PROB)])
def test_family_limits(kw):
    assert call(**kw) == N.ERR_UNSUPPORTED
    assert call(bufs=DUMMY, **kw) == N.ERR_UNSUPPORTED


def test_missing_buffers_inside_the_family():
    assert call() == N.ERR_INVALID_ARGUMENT
