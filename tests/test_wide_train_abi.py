"""CPU-only checks of K33's entry points (nfa_pack_resnet_wide_train_f32, nfa_resnet_wide_forward_f32,
nfa_resnet_wide_backward_f32) in the manner of tests/test_wide_layer_abi.py: the header, the bindings, the argument contract
through the C ABI with pointers that are never read, and `ops.resnet_wide_train_supported`'s table."""
import ctypes
import os

import pytest

from nflows_amd import _native as N
from nflows_amd import ops

_keep = ctypes.create_string_buffer(64)
DUMMY = ctypes.addressof(_keep)   # a non-null pointer (never read)
ENTRIES = ("nfa_pack_resnet_wide_train_f32", "nfa_resnet_wide_forward_f32", "nfa_resnet_wide_backward_f32")


def forward(batch=64, di=8, hidden=256, blocks=2, out=184, bufs=None):
    return N.load().nfa_resnet_wide_forward_f32(bufs, bufs, bufs, bufs, bufs, bufs, out, batch, di, hidden, blocks, None)


def backward(batch=64, di=8, hidden=256, blocks=2, out=184, bufs=None, g_hidden=None):
    return N.load().nfa_resnet_wide_backward_f32(g_hidden, bufs, out, bufs, bufs, bufs, bufs, bufs, batch, di, hidden, blocks,
                                                 None)


def test_entry_points_are_declared_and_bound():
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "nflows_amd.h")) as f:
        header = f.read()
    lib = N.load()
    for name in ENTRIES:
        assert name in N.EXPORTS and ("int %s(" % name) in header and getattr(lib, name).argtypes
    assert lib.nfa_abi_version() == N.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(), dict(hidden=129), dict(blocks=0, out=0), dict(di=64, blocks=3, out=32768)])
def test_batch_zero_is_a_no_op(kw):
    assert forward(batch=0, **kw) == N.OK and backward(batch=0, **kw) == N.OK


@pytest.mark.parametrize("kw", [dict(batch=-64), dict(di=0), dict(blocks=-1), dict(hidden=0), dict(out=-4)])
def test_invalid_arguments_come_first(kw):
    for call in (forward, backward):
        assert call(**kw) == N.ERR_INVALID_ARGUMENT
        assert call(**dict(dict(hidden=257), **kw)) == N.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("kw", [dict(hidden=128), dict(hidden=257), dict(blocks=4), dict(di=68), dict(di=6), dict(batch=96),
                                dict(out=6), dict(out=32772)])
def test_family_limits(kw):
    for call in (forward, backward):
        assert call(**kw) == N.ERR_UNSUPPORTED and call(bufs=DUMMY, **kw) == N.ERR_UNSUPPORTED


def test_missing_buffers_inside_the_family():
    assert forward() == N.ERR_INVALID_ARGUMENT and backward() == N.ERR_INVALID_ARGUMENT
    assert backward(bufs=DUMMY, g_hidden=DUMMY) == N.ERR_INVALID_ARGUMENT          # both incoming gradients
    assert backward(bufs=DUMMY, out=0) == N.ERR_INVALID_ARGUMENT                  # grad_params without the final Linear
    pack = N.load().nfa_pack_resnet_wide_train_f32
    assert pack(None, None, None, None, None, 0, 8, 8, 256, 0, None, None, None, None) == N.ERR_INVALID_ARGUMENT
    assert pack(DUMMY, DUMMY, None, None, None, 0, 9, 8, 256, 0, DUMMY, DUMMY, DUMMY, None) == N.ERR_INVALID_ARGUMENT
    assert pack(DUMMY, DUMMY, None, None, None, 0, 8, 8, 128, 0, DUMMY, DUMMY, DUMMY, None) == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("args,ok", [((64, 3, 129, 1), True), ((128, 64, 256, 3), True), ((64, 16, 256, 0), True),
                                     ((64, 8, 128, 1), False), ((64, 8, 257, 1), False), ((96, 8, 192, 1), False),
                                     ((0, 8, 192, 1), False), ((64, 65, 192, 1), False), ((64, 0, 192, 1), False),
                                     ((64, 8, 192, 4), False)])
def test_supported_table(args, ok):
    assert ops.resnet_wide_train_supported(*args) is ok
