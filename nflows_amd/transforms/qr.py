"""The linear layer W = Q R with a Householder sequence Q and an upper triangular R.

API of nflows/transforms/qr.py: `QRLinear(features, num_householder, using_cache=False)` with `bias`, `upper_entries`
(R's strict upper triangle, np.triu_indices order), `log_upper_diag` (R_ii = exp(.)) and the submodule `orthogonal`
(HouseholderSequence: `q_vectors`).  forward: y = Q (R x) + b, inverse: x = R^-1 (Q^T (y - b)) by substitution,
logabsdet = +- sum log_upper_diag.

On a HIP device a float32 [batch, features] tensor goes through ONE K24 launch per call in both directions (2 <= features
<= 128, num_householder <= 128), which reads the parameters as they are; tensors that require grad through K24-backward
and the device's GEMM (nflows_amd/autograd.py: Householder).  Dispatch (DESIGN.md section 4, K24's timings): the kernel
wherever it serves, except forward calls with features > 64 and num_householder <= 2 -- without autograd over more than
16 384 rows, under autograd over at most 16 384 --, which take the stock ops.  With the cache on
in eval mode the base class multiplies by the cached weight matrix instead.  float64, other ranks and sizes outside the
range: stock device ops (`_use_kernel = False` too).
"""
import numpy as np
import torch
from torch import nn

from .. import autograd as AG
from .. import ops
from .linear import Linear
from .lu import SOLVE_ROWS_PER_CALL
from .orthogonal import HouseholderSequence, check_features, kernel_serves, reflect_rows


class QRLinear(Linear):
    _use_kernel = True

    def __init__(self, features, num_householder, using_cache=False):
        super().__init__(features, using_cache)
        self.upper_indices = np.triu_indices(features, k=1)
        self.diag_indices = np.diag_indices(features)
        self.upper_entries = nn.Parameter(torch.zeros(features * (features - 1) // 2))
        self.log_upper_diag = nn.Parameter(torch.zeros(features))
        self.orthogonal = HouseholderSequence(features=features, num_transforms=num_householder)
        self._initialize()

    def _initialize(self):
        bound = 1.0 / np.sqrt(self.features)
        with torch.no_grad():
            self.upper_entries.uniform_(-bound, bound)
            self.log_upper_diag.uniform_(-bound, bound)
            self.bias.zero_()

    def _create_upper(self, dtype=None):
        """Dense R on the parameters' device: one scatter of the entries into a flat [D * D] buffer (row-major i * D + j,
        np.triu_indices order) plus the diagonal."""
        n = self.features
        entries = self.upper_entries if dtype is None else self.upper_entries.to(dtype)
        log_diag = self.log_upper_diag if dtype is None else self.log_upper_diag.to(dtype)
        rows, cols = torch.triu_indices(n, n, 1, device=entries.device)
        flat = entries.new_zeros(n * n).index_put((rows * n + cols,), entries)
        return flat.view(n, n) + torch.diag(torch.exp(log_diag))

    def logabsdet(self):
        # one number per layer: summed in float64, rounded once (as the kernel forms it)
        return torch.sum(self.log_upper_diag.double()).to(self.log_upper_diag.dtype)

    def _rows(self, rows, inverse, with_bias=True):
        """The map on the last dimension by stock tensor ops in the dtype of `rows` (any device)."""
        dt = rows.dtype
        upper = self._create_upper(dt)
        q = self.orthogonal.q_vectors.to(dt)
        if not inverse:
            rows = reflect_rows(rows @ upper.t(), q)
            return rows + self.bias.to(dt) if with_bias else rows
        if with_bias:
            rows = rows - self.bias.to(dt)
        rows = reflect_rows(rows, q, descending=True)
        flat = rows.reshape(-1, self.features)
        pieces = [torch.linalg.solve_triangular(upper, chunk.t(), upper=True).t()
                  for chunk in flat.split(SOLVE_ROWS_PER_CALL)]
        return (pieces[0] if len(pieces) == 1 else torch.cat(pieces)).reshape(rows.shape)

    def _matrix(self, inverse):
        # float64 from the parameters, rounded once: a cached matrix is used for every row, nothing averages its error out
        identity = torch.eye(self.features, dtype=torch.float64, device=self.bias.device)
        return self._rows(identity, inverse, with_bias=False).t().to(self.bias.dtype)

    def weight(self):
        return self._matrix(False)

    def weight_inverse(self):
        return self._matrix(True)

    def _kernel_pays(self, inputs, inverse):
        """False where K24 was measured slower than the stock ops (DESIGN.md section 4 "K24",
        profiles/householder_time.json): wide layers with one or two reflections, going forward."""
        if inverse or self.features <= 64 or self.orthogonal.num_transforms > 2:
            return True
        if AG.needs_grad(inputs, *self.parameters()):
            return inputs.shape[0] > 16384
        return inputs.shape[0] <= 16384

    def _run(self, inputs, inverse):
        check_features(inputs, self.features)
        q = self.orthogonal.q_vectors
        if self._use_kernel and kernel_serves(inputs, self.features, q) and self._kernel_pays(inputs, inverse):
            return ops.householder(inputs, q_first=q if inverse else None, q_second=None if inverse else q,
                                   upper_entries=self.upper_entries, log_upper_diag=self.log_upper_diag, bias=self.bias,
                                   eps=0.0, inverse=inverse)
        logabsdet = -self.logabsdet() if inverse else self.logabsdet()
        return self._rows(inputs, inverse), logabsdet * inputs.new_ones(inputs.shape[0])

    def forward_no_cache(self, inputs):
        return self._run(inputs, False)

    def inverse_no_cache(self, inputs):
        return self._run(inputs, True)
