"""Orthogonal transforms: a sequence of Householder reflections.

API of nflows/transforms/orthogonal.py: `HouseholderSequence(features, num_transforms)` with the parameter `q_vectors`
[num_transforms, features]; reflection k maps x to x - 2 (x . q_k) q_k / (q_k . q_k), `forward` applies them first to
last, `inverse` last to first (each is its own inverse), logabsdet is 0.  The initial vectors are the reference's: pairs
of equal unit vectors e_0, e_0, e_1, e_1, ... (a pair cancels: the identity) and, for an odd count, a last e_{K // 2}.

On a HIP device a float32 [batch, features] tensor with 2 <= features <= 128 and at most 128 reflections goes through
K24, which reads `q_vectors` as it is (an optimizer step or a `.data` write is seen by the next call); tensors that
require grad through K24-backward.  Dispatch: the kernel wherever it serves.  float64, other ranks and sizes outside that
range: the same steps by stock device ops (`_use_kernel = False` selects them too).
"""
import torch
from torch import nn

from .. import ops
from ..utils import typechecks as check
from .base import Transform
from .linear import _require_device

MAX_KERNEL_FEATURES = 128
MAX_KERNEL_TRANSFORMS = 128


def initial_q_vectors(features, num_transforms):
    half = num_transforms // 2
    q = torch.zeros(num_transforms, features)
    pairs = torch.arange(min(half, features))      # (rows past `features` pairs stay zero, as the reference's do)
    q[2 * pairs, pairs] = 1.0
    q[2 * pairs + 1, pairs] = 1.0
    if num_transforms % 2:
        q[-1, half] = 1.0
    return q


def reflect_rows(inputs, q_vectors, descending=False):
    """The sequence by stock tensor ops, any dtype and rank (features last)."""
    scales = 2.0 / torch.sum(q_vectors * q_vectors, dim=-1)
    order = range(q_vectors.shape[0] - 1, -1, -1) if descending else range(q_vectors.shape[0])
    outputs = inputs
    for k in order:
        q = q_vectors[k]
        outputs = outputs - (outputs @ q).unsqueeze(-1) * (scales[k] * q)
    return outputs


def kernel_serves(inputs, features, *q_vector_sets):
    return (inputs.dim() == 2 and inputs.dtype == torch.float32 and 2 <= features <= MAX_KERNEL_FEATURES
            and all(q.dtype == torch.float32 and 1 <= q.shape[0] <= MAX_KERNEL_TRANSFORMS for q in q_vector_sets))


def check_features(inputs, features):
    _require_device(inputs)
    if inputs.dim() < 2 or inputs.shape[-1] != features:
        raise ValueError("Expected inputs with %d features in the last dimension, got shape %s."
                         % (features, tuple(inputs.shape)))


class HouseholderSequence(Transform):
    _use_kernel = True

    def __init__(self, features, num_transforms):
        if not check.is_positive_int(features):
            raise TypeError("Number of features must be a positive integer.")
        if not check.is_positive_int(num_transforms):
            raise TypeError("Number of transforms must be a positive integer.")
        super().__init__()
        self.features = features
        self.num_transforms = num_transforms
        self.q_vectors = nn.Parameter(initial_q_vectors(features, num_transforms))

    def _run(self, inputs, inverse):
        check_features(inputs, self.features)
        if self._use_kernel and kernel_serves(inputs, self.features, self.q_vectors):
            return ops.householder(inputs, q_first=self.q_vectors, inverse=inverse)
        return reflect_rows(inputs, self.q_vectors, descending=inverse), inputs.new_zeros(inputs.shape[0])

    def forward(self, inputs, context=None):
        return self._run(inputs, False)

    def inverse(self, inputs, context=None):
        return self._run(inputs, True)

    def matrix(self):
        """The orthogonal [features, features] matrix of the whole sequence, on the parameters' device."""
        identity = torch.eye(self.features, dtype=self.q_vectors.dtype, device=self.q_vectors.device)
        return reflect_rows(identity, self.q_vectors, descending=True)
