"""K33 (csrc/resnet_train_wide.hip, autograd.ResidualNetWide) bit for bit.

On exact_logits' recipes every intermediate of the conditioner and of its backward chain is exact in fp32 in any order and
on any operand split (checked on the data by exact_logits._exact_linear: operand bits, the 2^24 q budget of every output,
the bf16 piece count of every product), so every array both kernels write is KNOWN: `hidden`, `saved[*]`, `params`,
`g_hidden`, `grads[*]`, `g_x` must equal exact_forward / exact_backward as numbers (a -0 for a +0 is not a finding), pad
columns exactly zero.  A wrong element -- a column guard off by one, a tile stored from the wrong row block, a dropped
low piece -- differs; no tolerance is involved.  tests/test_wide_exact_host.py holds the same exact values to stock torch
in float32 and float64 on the CPU.

Shapes (tests/wide_exact_cases.py K33_SHAPES), each for one mechanism: a 20-column `params` tile (the shape of the
recorded compiler reordering), g_x's second output tile at d_i = 33, `out` of exactly one 256-column chunk and
one column more (257: run as 260 columns, three of them zero pad rows of the final Linear under nonzero columns of g -- the
kernels take multiples of four, so the issue's 257 is not reachable as written), three chunks, 1472 columns on three blocks, hidden only, and a second pass of the persistent loop; the
long-mantissa recipe at 256 -> 736.  Through the class: every parameter's gradient of ResidualNet(8, 40, H, 2 blocks) at
H = 129 and 256 -- K10's weight and bias gradients on the [B, Hp] planes sliced to [:H, :H], the initial and final
Linear's included."""
import copy

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import wide_exact_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(net, x, g, di, H, nb, out):
    """both kernels on device copies of `net`'s parameters: {array name: tensors}"""
    from nflows_amd import ops
    dp = (di + 3) // 4 * 4
    Hp = (H + 31) // 32 * 32
    dev = copy.deepcopy(net).to(DEV)
    blocks = [(b.linear_layers[0].weight, b.linear_layers[0].bias, b.linear_layers[1].weight, b.linear_layers[1].bias)
              for b in dev.blocks]
    # (the kernels take `out` in multiples of four -- the backward kernel guards g_params in groups of four columns --: 257
    #  columns run as 260 with zero rows of the final Linear behind them, which is how a caller has to hand such a net
    #  over.  g is NOT zero in the pad columns (1.5): a column of g paired with another row of the final Linear shows in
    #  g_hidden; the pad columns of `params` must come back zero)
    out4 = (out + 3) // 4 * 4
    final = (F.pad(dev.final_layer.weight, (0, 0, 0, out4 - out)), F.pad(dev.final_layer.bias, (0, out4 - out))) if out else None
    fwd_w, bias, bwd_w = ops.pack_resnet_wide_train(dev.initial_layer.weight, dev.initial_layer.bias, blocks, final)
    xs = F.pad(torch.from_numpy(x).float(), (0, dp - di)).to(DEV)
    gs = torch.from_numpy(g).float()
    gs = (F.pad(gs, (0, out4 - out), value=1.5) if out else F.pad(gs, (0, Hp - H))).to(DEV)
    hidden, saved, params = ops.resnet_wide_forward(xs, fwd_w, bias, H, nb, out4)
    gx, grads, g_hidden = ops.resnet_wide_backward(gs, bwd_w, saved, dp, H, from_params=bool(out))
    ops.check_status()
    return {"hidden": hidden, "saved": list(saved), "params": params, "g_hidden": g_hidden, "grads": list(grads), "g_x": gx}


@pytest.mark.parametrize("shape", W.K33_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_every_array_equals_the_exact_values(shape):
    di, H, nb, out, rows, recipe = shape
    second_pass = rows == W.CUS
    rows = 64 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) if second_pass else rows
    net, x, g, forward, backward = W.k33_problem(di, H, nb, out, rows, recipe)
    got = _run(net, x, g, di, H, nb, out)
    want = {"hidden": forward["hidden"], "saved": forward["saved"], "params": forward["params"],
            "g_hidden": backward["g_hidden"], "grads": backward["grads"], "g_x": backward["g_x"]}
    width = {"params": out, "g_x": di}
    host = {}
    for key, value in got.items():
        planes = value if isinstance(value, list) else [value]
        cut = []
        for j, plane in enumerate(planes):
            if plane is None:
                cut.append(None)
                continue
            w = width.get(key, H)
            assert not plane[:, w:].any(), "%s[%d]: pad columns" % (key, j)
            cut.append(plane[:, :w].cpu().numpy())
        host[key] = cut if isinstance(value, list) else cut[0]
    W.assert_equal_as_numbers(host, want, str(shape))
    if second_pass:     # the last 64 rows, run alone, bit for bit
        alone = _run(net, x[-64:], g[-64:], di, H, nb, out)
        for key, value in got.items():
            a, b = (torch.stack(v) if isinstance(v, list) else v for v in (value, alone[key]))
            assert torch.equal(a[..., -64:, :], b), key


@pytest.mark.parametrize("H", W.CLASS_WIDTHS)
def test_parameter_gradients_through_the_class(monkeypatch, H):
    from nflows_amd.nn.nets.resnet import ResidualNet
    monkeypatch.setattr(ResidualNet, "fuse_wide_training_min_rows", 64)   # the kernel itself, whatever the size rule
    net, x, g, forward, backward = W.class_problem(H)
    dev = copy.deepcopy(net).to(DEV)
    xs = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
    out = dev(xs)
    assert type(out.grad_fn).__name__ == "ResidualNetWideBackward", out.grad_fn   # (fails without K33)
    assert np.array_equal(out.detach().cpu().numpy().astype(np.float64), forward["params"])
    out.backward(torch.from_numpy(g).float().to(DEV))
    got = {name: p.grad.cpu().numpy() for name, p in dev.named_parameters()}
    assert set(got) == set(backward["param_grads"])
    W.assert_equal_as_numbers(got, backward["param_grads"], "H=%d" % H)
    W.assert_equal_as_numbers(xs.grad.cpu().numpy(), backward["g_x"], "H=%d g_x" % H)
