"""The packed streams of the four wide whole-layer kernels (K32 / K34 / K36 / K37), pinned byte for byte: hidden width 136
(Hp = 160: a padded last tile, five active waves), 6 or 7 features (an odd pair, rows past d_t), K = 6.  Weights come from an
integer formula, so the bytes depend on no generator.  No GPU."""
import hashlib

import pytest
import torch

from nflows_amd import ops
from nflows_amd.nn.nets import MLP, ResidualNet
from nflows_amd.transforms.made import MADE

H, K = 136, 6
P = 3 * K - 1


def _fill(net):
    with torch.no_grad():
        for n, (_, p) in enumerate(net.named_parameters()):
            flat = p.reshape(p.shape[0], -1)
            i = torch.arange(flat.shape[0])[:, None]
            j = torch.arange(flat.shape[1])[None, :]
            p.copy_((((i * 37 + j * 11 + n * 5) % 64 - 32).float() / 64).reshape(p.shape))
    return net


def _digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _resnet():    # K32: d_i 4, d_t 3 padded to 4
    net = _fill(ResidualNet(4, 3 * P, hidden_features=H, num_blocks=2))
    return ops.pack_resnet_conditioner_wide(net, 3, P, pad_transform_to=4)


def _made_ff():   # K34: 7 features (an odd pair), feed-forward blocks
    net = _fill(MADE(7, H, num_blocks=2, output_multiplier=P, use_residual_blocks=False))
    return ops.pack_made_rqs_conditioner_wide(net, K)


def _made_ctx():  # K36: 6 features, residual blocks, 5 context features
    net = _fill(MADE(6, H, context_features=5, num_blocks=2, output_multiplier=2))
    return ops.pack_made_affine_conditioner_wide(net)


def _mlp():       # K37: d_i 4, d_t 3, two hidden layers
    net = _fill(MLP([4], [6], [H, H]))
    return ops.pack_affine_conditioner_wide(net, 3)


# packer -> (weights numel, sha256, biases numel, sha256)
PINNED = {
    "resnet": (_resnet, (376320, "70411a85960a6a422105d86656c397bb66b4fa6f90c21f92188c3e728d56d5d4",
                         928, "ffafa1b9a96855fbd8af2c5b04e2cc96d1d67f19ff499ec8e2e8e226ba704d6e")),
    "made_ff": (_made_ff, (284160, "a7873edd5e08b5be14dd99f4ad8da500d6c51f649ab8a141407899dd64ae4a11",
                           736, "51c3a9a27c39d46769a9c680b84fe4320b2d2e04091576db443e887935a8eb2c")),
    "made_ctx": (_made_ctx, (353280, "2c46e8977a94e29920785cd53c475ecb1fed1dee8c5b0bc170b81919942f707d",
                             992, "2633342b85d513fd72d5d7f5d6f3c032aed035e7a8b06c26c38fd76b33022788")),
    "mlp": (_mlp, (99840, "6234028e3182e114f36df6ac82f618a751b8f345bf10e99aa4fa3873d735038a",
                   352, "2e83109e6315cbcd5579349490abe30a2ff0d239e8600e0fdd774b6e477ff502")),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_wide_packed_stream_bytes(name):
    pack, want = PINNED[name]
    w, b = pack()
    assert (w.numel(), _digest(w), b.numel(), _digest(b)) == want
