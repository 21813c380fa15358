"""K26 (the float64 whole-layer kernel) on the host: its entry points, the layout of its packed stream and its gate."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nfa_pack_resnet_f64", "nfa_rqs_resnet_layer_f64")


def test_entry_points_are_declared_bound_and_exported():
    from nflows_amd import _native
    header = open(os.path.join(ROOT, "include", "nflows_amd.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _native.EXPORTS
    assert re.search(r"#define NFA_ABI_VERSION 19\b", header) and _native.ABI_VERSION == 19
    lib = _native.load()
    assert lib.nfa_abi_version() == 19
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None


def _net(di, H, nb, dt, P, seed=0):
    from nflows_amd.nn.nets.resnet import ResidualNet
    torch.manual_seed(seed)
    net = ResidualNet(di, dt * P, H, num_blocks=nb).double()
    with torch.no_grad():
        for p in net.parameters():   # (no zero left by the initialisation: a dropped element shows)
            p.copy_(torch.randn(p.shape, dtype=torch.float64))
    return net


def _unpack_matrix(stream, offset, ks, nt):
    """the documented layout, index by index: fragment ((kk nt + t) 64 + lane) holds W[16 t + (lane & 15)][4 kk + (lane >> 4)]"""
    w = np.full((16 * nt, 4 * ks), np.nan)
    kk, t, lane = np.meshgrid(np.arange(ks), np.arange(nt), np.arange(64), indexing="ij")
    w[16 * t + (lane & 15), 4 * kk + (lane >> 4)] = stream[offset + (kk * nt + t) * 64 + lane]
    return w


def _padded(a, shape):
    out = np.zeros(shape)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


@pytest.mark.parametrize("tails", ["linear", None])
@pytest.mark.parametrize("K", [2, 8, 32])
@pytest.mark.parametrize("H,di,nb", [(16, 1, 0), (24, 3, 2), (100, 32, 3), (128, 64, 2), (16, 64, 3), (128, 1, 0), (24, 32, 0),
                                     (100, 3, 2)])
def test_reference_pack_unpermutes_to_the_padded_weights(H, di, nb, K, tails):
    from nflows_amd import ops
    P = 3 * K - 1 if tails == "linear" else 3 * K + 1
    dt = 5 if K == 32 else 9
    net = _net(di, H, nb, dt, P)
    stream = ops.pack_resnet_f64_reference(net, dt, P).numpy()
    lay = ops.resnet_f64_layout(di, H, nb, dt, P)
    assert stream.shape == (lay["total"],) and stream.dtype == np.float64
    HP, NT, ksh = lay["HP"], lay["NT"], lay["ksh"]
    assert HP % 16 == 0 and HP - 16 < H <= HP and lay["F"] * P <= 128 and (lay["F"] < 4 or lay["F"] % 4 == 0 or lay["F"] == dt)
    np.testing.assert_array_equal(_unpack_matrix(stream, lay["w_in"], lay["ks0"], NT),
                                  _padded(net.initial_layer.weight.detach().numpy(), (HP, 4 * lay["ks0"])))
    np.testing.assert_array_equal(stream[lay["b_in"]:lay["b_in"] + HP], _padded(net.initial_layer.bias.detach().numpy(), (HP,)))
    for b, block in enumerate(net.blocks):
        for j, layer in enumerate(block.linear_layers):
            m = 2 * b + j
            np.testing.assert_array_equal(_unpack_matrix(stream, lay["w_blocks"] + m * ksh * NT * 64, ksh, NT),
                                          _padded(layer.weight.detach().numpy(), (HP, HP)))
            at = lay["b_blocks"] + m * HP
            np.testing.assert_array_equal(stream[at:at + HP], _padded(layer.bias.detach().numpy(), (HP,)))
    wf, bf = net.final_layer.weight.detach().numpy(), net.final_layer.bias.detach().numpy()
    seen = 0
    for c in range(lay["chunks"]):
        last = c == lay["chunks"] - 1
        nt = lay["NTL"] if last else lay["NTF"]
        lo, hi = c * lay["F"] * P, min((c + 1) * lay["F"], dt) * P
        assert hi - lo <= 16 * nt < hi - lo + 16
        np.testing.assert_array_equal(_unpack_matrix(stream, lay["w_final"] + c * ksh * lay["NTF"] * 64, ksh, nt),
                                      _padded(wf[lo:hi], (16 * nt, HP)))
        at = lay["b_final"] + c * lay["NTF"] * 16
        np.testing.assert_array_equal(stream[at:at + 16 * nt], _padded(bf[lo:hi], (16 * nt,)))
        seen += hi - lo
    assert seen == dt * P


def _layer(H=32, di=4, dt=4, K=8, tails="linear", **net_kw):
    from nflows_amd.nn.nets.resnet import ResidualNet
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ
    mask = torch.cat((torch.zeros(di), torch.ones(dt)))
    return RQ(mask, lambda i, o: ResidualNet(i, o, H, **net_kw), num_bins=K, tails=tails, tail_bound=3.0).double().eval()


def test_gate():
    from torch.nn import functional as F
    x = torch.zeros(4, 8, dtype=torch.float64)
    with torch.no_grad():
        good = _layer()
        assert good._float64_module_ok(None)                       # the layer itself qualifies ...
        assert not good._float64_layer_eligible(x, None)           # ... a CPU tensor does not
        assert type(good).fuse_float64_min_rows == 8192            # (the size rule's default: DESIGN.md section 4 "K26")
        assert _layer(tails=None)._float64_module_ok(None) and _layer(num_blocks=0)._float64_module_ok(None)
        assert not good._float64_module_ok(torch.zeros(4, 3, dtype=torch.float64))
        assert not _layer(context_features=3)._float64_module_ok(torch.zeros(4, 3, dtype=torch.float64))
        assert not _layer(activation=F.leaky_relu)._float64_module_ok(None)
        assert _layer(H=128)._float64_module_ok(None) and not _layer(H=129)._float64_module_ok(None)
        assert _layer(di=64)._float64_module_ok(None) and not _layer(di=65)._float64_module_ok(None)
        assert _layer(dt=64)._float64_module_ok(None) and not _layer(dt=65)._float64_module_ok(None)
        assert _layer(K=32)._float64_module_ok(None) and not _layer(K=33)._float64_module_ok(None)
        assert not _layer(use_batch_norm=True)._float64_module_ok(None)
        assert not _layer().float()._float64_module_ok(None)
        dropping = _layer(dropout_probability=0.5)
        assert dropping._float64_module_ok(None) and not dropping.train()._float64_module_ok(None)
        off = _layer()
        off.fuse_float64 = False
        assert not off._float64_module_ok(None)
    with torch.enable_grad():
        assert not good._float64_module_ok(None)


def test_environment_switch():
    code = ("from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ; "
            "print(int(RQ.fuse_float64))")
    for value, want in (("0", "0"), (None, "1")):
        env = {k: v for k, v in os.environ.items() if k != "NFA_K26"}
        if value is not None:
            env["NFA_K26"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, check=True, capture_output=True, text=True)
        assert out.stdout.strip().splitlines()[-1] == want
