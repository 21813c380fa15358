"""Shared by the tests of the learned base densities (K20): the cases of tests/golden/make_golden_density.py -- shapes, seeded
operands -- and the fixtures' loader."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIAG_SHAPES = ((517, 1), (517, 5), (129, 67), (37, 3, 5, 7), (9, 4100))
DIAG_MODES = ("shared", "row")
MOG_SHAPES = ((517, 1, 1), (517, 5, 5), (129, 67, 3), (33, 7, 64), (5, 2100, 2))
MOG_WIDE = (129, 5, 5)
MOG_CASES = tuple(("plain", s) for s in MOG_SHAPES) + (("wide", MOG_WIDE),)
EPSILON = 1e-2
MADEMOG = dict(features=7, hidden_features=32, context_features=3, num_blocks=2, num_mixture_components=5)
FLOW = dict(D=6, H=32, K=8, C=3, rows=512)


def tag(shape):
    return "x".join(str(s) for s in shape)


def diag_inputs(mode, shape):
    """x [B, ...], the loss weights r [B] and the parameters: "shared" means / log_stds [1, N], "row" the encoder's [B, 2 N]
    output (means, then log stds), from the generator's seeds."""
    B, n = shape[0], int(np.prod(shape[1:]))
    rng = np.random.RandomState(9000 + 10 * DIAG_SHAPES.index(tuple(shape)) + DIAG_MODES.index(mode))
    x = (1.5 * rng.randn(*shape)).astype(np.float32)
    r = rng.randn(B).astype(np.float32)
    rows = 1 if mode == "shared" else B
    means = rng.randn(rows, n).astype(np.float32)
    log_stds = np.clip(0.5 * rng.randn(rows, n), -1.5, 1.5).astype(np.float32)
    if mode == "shared":
        return x, r, means, log_stds
    return x, r, np.concatenate([means, log_stds], axis=1)


def softplus64(u):
    return np.where(u > 20.0, u, np.log1p(np.exp(np.minimum(u, 20.0))))


def mog_inputs(kind, shape):
    """x [B, D], the loss weights r [B] and the MADE's final-layer output [B, D * K * 3] in the reference's interleaving.
    "wide": logits of +-30, unconstrained stds from -30 (std -> epsilon) to 2, x 50 standard deviations from every mean."""
    B, D, K = shape
    rng = np.random.RandomState(9500 + 10 * MOG_CASES.index((kind, tuple(shape))))
    x = (1.5 * rng.randn(B, D)).astype(np.float32)
    r = rng.randn(B).astype(np.float32)
    if kind == "plain":
        logits = rng.randn(B, D, K)
        means = 2.0 * rng.randn(B, D, K)
        u = rng.randn(B, D, K)
    else:
        logits = 30.0 * (rng.randint(0, 2, size=(B, D, K)) * 2 - 1)
        u = rng.uniform(-30.0, 2.0, size=(B, D, K))
        u[:, :, 0] = -30.0
        std = softplus64(u.astype(np.float32).astype(np.float64)) + EPSILON
        means = x.astype(np.float64)[:, :, None] - 50.0 * std * (rng.randint(0, 2, size=(B, D, K)) * 2 - 1)
    outputs = np.stack([logits, means, u], axis=-1).astype(np.float32).reshape(B, D * K * 3)
    return x, r, outputs


def module_inputs(which):
    """Inputs and raw context rows of the two module fixtures."""
    if which == "mademog":
        rng = np.random.RandomState(9901)
        return rng.randn(64, MADEMOG["features"]).astype(np.float32), rng.randn(64, MADEMOG["context_features"]).astype(np.float32)
    rng = np.random.RandomState(9902)
    return (rng.randn(FLOW["rows"], FLOW["D"]).astype(np.float32), rng.randn(FLOW["rows"], FLOW["C"]).astype(np.float32))


def golden(name):
    with np.load(os.path.join(GOLDEN, "density_%s.npz" % name)) as z:
        return {k: z[k] for k in z.files}


def truth(g, name):
    return g[name].astype(np.float64) + g[name + "_d"].astype(np.float64)


def conditional_flow(nf):
    """The conditional flow of density_flow.npz from the package `nf` exposes (the generator: the reference; the tests:
    nflows_amd): two rational-quadratic couplings with a context, ConditionalDiagonalNormal whose encoder is a Linear."""
    import torch
    D, H, K, C = FLOW["D"], FLOW["H"], FLOW["K"], FLOW["C"]
    layers = []
    for i in range(2):
        layers.append(nf.PiecewiseRationalQuadraticCouplingTransform(
            mask=nf.create_alternating_binary_mask(D, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: nf.ResidualNet(i_, o_, hidden_features=H, context_features=C, num_blocks=2),
            num_bins=K, tails="linear", tail_bound=4.0))
        if i == 0:
            layers.append(nf.ReversePermutation(D))
    return nf.Flow(nf.CompositeTransform(layers), nf.ConditionalDiagonalNormal([D], context_encoder=torch.nn.Linear(C, 2 * D)))
