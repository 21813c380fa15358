"""The linear layer W = Q1 diag(d) Q2 with Householder sequences Q1, Q2.

API of nflows/transforms/svd.py: `SVDLinear(features, num_householder, using_cache=False, identity_init=True, eps=1e-3)`
with `bias`, `unconstrained_diagonal` (d = eps + softplus(.)), and the submodules `orthogonal_1`, `orthogonal_2`
(HouseholderSequence: `q_vectors`); `num_householder` is even.  forward: y = Q1 (d * (Q2 x)) + b, inverse: the steps
undone in reverse, logabsdet = +- sum log d.

On a HIP device a float32 [batch, features] tensor goes through ONE K24 launch per call in both directions (2 <= features
<= 128, num_householder <= 128), which reads the parameters as they are; tensors that require grad through K24-backward.
Dispatch: the kernel wherever it serves.  With the cache on in eval mode the base class multiplies by the cached weight
matrix instead.  float64, other ranks and sizes outside the range: stock device ops (`_use_kernel = False` too).
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from .. import ops
from .linear import Linear
from .orthogonal import HouseholderSequence, check_features, kernel_serves, reflect_rows


class SVDLinear(Linear):
    _use_kernel = True

    def __init__(self, features, num_householder, using_cache=False, identity_init=True, eps=1e-3):
        super().__init__(features, using_cache)
        assert num_householder % 2 == 0
        self.eps = eps
        self.orthogonal_1 = HouseholderSequence(features=features, num_transforms=num_householder)
        self.unconstrained_diagonal = nn.Parameter(torch.zeros(features))
        self.orthogonal_2 = HouseholderSequence(features=features, num_transforms=num_householder)
        self.identity_init = identity_init
        self._initialize()

    def _initialize(self):
        with torch.no_grad():
            self.bias.zero_()
            if self.identity_init:   # the logit whose softplus is 1 - eps
                self.unconstrained_diagonal.fill_(float(np.log(np.exp(1 - self.eps) - 1)))
            else:
                bound = 1.0 / np.sqrt(self.features)
                self.unconstrained_diagonal.uniform_(-bound, bound)

    @property
    def diagonal(self):
        return self.eps + F.softplus(self.unconstrained_diagonal)

    @property
    def log_diagonal(self):
        return torch.log(self.diagonal)

    def logabsdet(self):
        # one number per layer: float64 from the logits, rounded once (as the kernel forms it)
        diagonal = self.eps + F.softplus(self.unconstrained_diagonal.double())
        return torch.sum(torch.log(diagonal)).to(self.unconstrained_diagonal.dtype)

    def _rows(self, rows, inverse, with_bias=True):
        """The map on the last dimension by stock tensor ops in the dtype of `rows` (any device)."""
        dt = rows.dtype
        q1, q2 = self.orthogonal_1.q_vectors.to(dt), self.orthogonal_2.q_vectors.to(dt)
        diagonal = self.eps + F.softplus(self.unconstrained_diagonal.to(dt))
        if not inverse:
            rows = reflect_rows(reflect_rows(rows, q2) * diagonal, q1)
            return rows + self.bias.to(dt) if with_bias else rows
        if with_bias:
            rows = rows - self.bias.to(dt)
        return reflect_rows(reflect_rows(rows, q1, descending=True) / diagonal, q2, descending=True)

    def _matrix(self, inverse):
        # float64 from the parameters, rounded once: a cached matrix is used for every row, nothing averages its error out
        identity = torch.eye(self.features, dtype=torch.float64, device=self.bias.device)
        return self._rows(identity, inverse, with_bias=False).t().to(self.bias.dtype)

    def weight(self):
        return self._matrix(False)

    def weight_inverse(self):
        return self._matrix(True)

    def _run(self, inputs, inverse):
        check_features(inputs, self.features)
        q1, q2 = self.orthogonal_1.q_vectors, self.orthogonal_2.q_vectors
        if self._use_kernel and kernel_serves(inputs, self.features, q1, q2):
            first, second = (q1, q2) if inverse else (q2, q1)
            return ops.householder(inputs, q_first=first, q_second=second,
                                   unconstrained_diagonal=self.unconstrained_diagonal, bias=self.bias, eps=self.eps,
                                   inverse=inverse)
        logabsdet = -self.logabsdet() if inverse else self.logabsdet()
        return self._rows(inputs, inverse), logabsdet * inputs.new_ones(inputs.shape[0])

    def forward_no_cache(self, inputs):
        return self._run(inputs, False)

    def inverse_no_cache(self, inputs):
        return self._run(inputs, True)
