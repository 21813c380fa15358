"""The launch hook of the per-layer launchers: every hooked launcher, called once at its smallest legal shape, records
its own name and the algorithmic bytes of its formula -- bench.py sums those bytes and the GPU tests count the names.
The expected numbers are worked out by hand from the formula in each case's comment, B = 128 rows throughout."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 128


class Recorder:
    def __init__(self):
        self.events = []

    def begin(self, name):
        return name

    def end(self, token, nbytes):
        self.events.append((token, nbytes))


def rand(*shape, dtype=torch.float32, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype).to(DEV)


def k1(ops):   # D = 4, d_t = 2, 2 bins, linear tails: P = 3 * 2 - 1 = 5 logits per feature
    spec = ops.make_rqs_spec(2, "linear", tail_bound=3.0)
    ops.rqs_coupling(rand(B, 4), rand(B, 10, seed=1), torch.tensor([1, 3], device=DEV), spec)


def lu_linear(ops):   # D = 4: 6 entries per triangle
    ops.lu_linear(rand(B, 4), rand(6, seed=1), rand(6, seed=2), rand(4, seed=3), rand(4, seed=4))


def householder(ops):   # D = 4, two reflections
    ops.householder(rand(B, 4), q_first=rand(2, 4, seed=1))


def lu_conv1x1(ops):   # C = 2, H = W = 2: one entry per triangle
    ops.lu_conv1x1(rand(B, 2, 2, 2), rand(1, seed=1), rand(1, seed=2), rand(2, seed=3), rand(2, seed=4))


def norm_stats(ops):
    ops.column_stats(rand(B, 4))


def norm_map(ops):
    ops.act_norm(rand(B, 4), rand(4, seed=1), rand(4, seed=2))


def nonlin(ops):   # n = 4 elements per row
    ops.nonlinearity(rand(B, 4), "tanh")


def diag_shared(ops):   # one shared row of N = 4: row stride 0
    ops.diag_normal_log_prob(rand(B, 4), rand(4, seed=1), rand(4, seed=2), 0.5)


def diag_per_row(ops):
    ops.diag_normal_log_prob(rand(B, 4), rand(B, 4, seed=1), rand(B, 4, seed=2), 0.5)


def mog(ops):   # D = 4, K = 1: outputs [B, 4 * 1 * 3]
    ops.mog_log_prob(rand(B, 4), rand(B, 12, seed=1), 1, 1e-2)


def diag_backward(ops):   # per-row parameters; forward and backward launch once each
    x = rand(B, 4).requires_grad_()
    ops.diag_normal_log_prob(x, rand(B, 4, seed=1), rand(B, 4, seed=2), 0.5).sum().backward()


def mog_backward(ops):
    x = rand(B, 4).requires_grad_()
    ops.mog_log_prob(x, rand(B, 12, seed=1), 1, 1e-2).sum().backward()


def k26(ops):   # the smallest layer of tests/test_gpu_f64_layer.py: D = 2 (d_i = d_t = 1), H = 16, no blocks; 2 bins: P = 5
    from nflows_amd.nn.nets.resnet import ResidualNet
    torch.manual_seed(0)
    net = ResidualNet(1, 5, 16, num_blocks=0).double().to(DEV)
    packed = ops.pack_resnet_f64(net, 1, 5)
    assert packed.numel() == 352   # resnet_f64_layout: 64 (W_in) + 256 (W_f) + 16 (b_in) + 16 (b_f) doubles
    spec = ops.make_rqs_spec(2, "linear", tail_bound=3.0)
    ops.rqs_resnet_layer_f64(rand(B, 2, dtype=torch.float64), packed, torch.tensor([0], device=DEV),
                             torch.tensor([1], device=DEV), 16, 0, spec)


def permute_cols(ops):   # a launcher without a hook name
    ops.permute_cols(rand(B, 4), torch.tensor([3, 0, 2, 1], device=DEV))


CASES = [   # (launch, under autograd, the recorded events)
    # 4 (B D + B d_t P + B D + B) = 4 (512 + 1280 + 512 + 128)
    (k1, False, [("rqs_coupling", 9728)]),
    # 4 (2 B D + B) = 4 (1024 + 128)
    (lu_linear, False, [("lu_linear", 4608)]),
    (householder, False, [("householder", 4608)]),
    # 4 (2 B C H W + B) = 4 (2048 + 128)
    (lu_conv1x1, False, [("lu_conv1x1", 8704)]),
    # 4 B D
    (norm_stats, False, [("norm_stats", 2048)]),
    # 4 (2 B D + B)
    (norm_map, False, [("norm_map", 4608)]),
    # 4 (2 B n + B)
    (nonlin, False, [("nonlin", 4608)]),
    # 4 (B n + 2 n rows + B (2 with logabsdet, else 1)), rows = 1 for a shared row, B per row: 4 (512 + 8 + 128)
    (diag_shared, False, [("diag_normal", 2592)]),
    # 4 (512 + 1024 + 128)
    (diag_per_row, False, [("diag_normal", 6656)]),
    # 4 (B D (1 + 3 K) + B) = 4 (2048 + 128)
    (mog, False, [("mog", 8704)]),
    # backward: 4 (2 B n + (4 B n per row, 2 n shared) + B) = 4 (1024 + 2048 + 128)
    (diag_backward, True, [("diag_normal", 6656), ("diag_normal_backward", 12800)]),
    # backward: 4 (2 B D (1 + 3 K) + B) = 4 (4096 + 128)
    (mog_backward, True, [("mog", 8704), ("mog_backward", 16896)]),
    # 8 (2 B D + B) + 8 packed doubles = 8 (512 + 128) + 8 * 352
    (k26, False, [("k26", 7936)]),
    (permute_cols, False, []),
]


@pytest.mark.parametrize("launch,grad,expected", CASES, ids=[c[0].__name__ for c in CASES])
def test_hook_records_name_and_bytes(launch, grad, expected):
    from nflows_amd import ops
    rec = Recorder()
    ops.set_launch_hook(rec)
    try:
        with torch.set_grad_enabled(grad):
            launch(ops)
    finally:
        ops.set_launch_hook(None)
    ops.check_status()
    assert rec.events == expected
