"""The linear layer of the neural-spline-flow step, W = L U.

API of nflows/transforms/lu.py: `LULinear(features, using_cache=False, identity_init=True, eps=1e-3)` with parameters
`lower_entries` (L's strict lower triangle, np.tril_indices order; L's diagonal is 1), `upper_entries` (U's strict
upper triangle, np.triu_indices order), `unconstrained_upper_diag` (U_ii = softplus(.) + eps) and `bias`.

On a HIP device a float32 [batch, features] tensor goes through K16 in every mode -- forward L (U x) + b, inverse by two
substitutions -- which reads the four parameters as they are: nothing is packed, so an optimizer step or a `.data`
write is seen by the next call.  With the cache on in eval mode the reference multiplies by a cached L @ U (or its
inverse) instead: another rounding of the same map; `cache.weight` / `.inverse` / `.logabsdet` are still filled when
they are asked for through `_check_forward_cache` / `_check_inverse_cache`.  Next to a column Permutation inside
`CompositeTransform` the permutation is folded into the kernel's gather / scatter and the composite's
`total_logabsdet +=` into its store.  float64 and other ranks: the same steps by stock device ops.
"""
import numpy as np
import torch
from torch.nn import functional as F
from torch import nn

from .. import ops
from .linear import Linear, _require_device

MAX_KERNEL_FEATURES = 128


def lower_entry_index(i, j):
    """Position of L[i, j], i > j, in `lower_entries` (np.tril_indices(features, -1) order)."""
    return i * (i - 1) // 2 + j


def upper_entry_index(i, j, features):
    """Position of U[i, j], j > i, in `upper_entries` (np.triu_indices(features, 1) order)."""
    return i * features - i * (i + 1) // 2 + (j - i - 1)


def dense_factors(lower_entries, upper_entries, upper_diag):
    """(L, U) as dense [D, D] tensors from the flat parameters and U's diagonal (differentiable device tensor code)."""
    n = upper_diag.shape[0]
    dev = upper_diag.device
    li, lj = torch.tril_indices(n, n, -1, device=dev)    # row-major: np.tril_indices order
    ui, uj = torch.triu_indices(n, n, 1, device=dev)     # row-major: np.triu_indices order
    blank = upper_diag.new_zeros(n * n)
    lower = blank.index_put((li * n + lj,), lower_entries.to(upper_diag.dtype)).view(n, n) \
        + torch.eye(n, dtype=upper_diag.dtype, device=dev)
    upper = blank.index_put((ui * n + uj,), upper_entries.to(upper_diag.dtype)).view(n, n) + torch.diag(upper_diag)
    return lower, upper


SOLVE_ROWS_PER_CALL = 65536   # the device library's triangular solve returns an error at 262 144 right-hand sides


def solve_rows(lower, upper, rows):
    """x_row = U^-1 L^-1 c_row for every row of `rows` [B, D], by two triangular solves of stock device ops (both with
    the factor's stored diagonal, L's ones included), at most SOLVE_ROWS_PER_CALL right-hand sides per library call."""
    pieces = []
    for chunk in rows.split(SOLVE_ROWS_PER_CALL):
        t = torch.linalg.solve_triangular(lower, chunk.t(), upper=False)
        pieces.append(torch.linalg.solve_triangular(upper, t, upper=True).t())
    return pieces[0] if len(pieces) == 1 else torch.cat(pieces)


class LULinear(Linear):
    supports_fused_permutation = True   # K16 gathers / scatters columns and adds into a running logabsdet

    def __init__(self, features, using_cache=False, identity_init=True, eps=1e-3):
        super().__init__(features, using_cache)
        self.eps = eps
        self.lower_indices = np.tril_indices(features, k=-1)
        self.upper_indices = np.triu_indices(features, k=1)
        self.diag_indices = np.diag_indices(features)
        count = features * (features - 1) // 2
        self.lower_entries = nn.Parameter(torch.zeros(count))
        self.upper_entries = nn.Parameter(torch.zeros(count))
        self.unconstrained_upper_diag = nn.Parameter(torch.zeros(features))
        self._initialize(identity_init)

    def _initialize(self, identity_init):
        with torch.no_grad():
            self.bias.zero_()
            if identity_init:   # L = I, U = I: the logit whose softplus is 1 - eps
                self.lower_entries.zero_()
                self.upper_entries.zero_()
                self.unconstrained_upper_diag.fill_(float(np.log(np.exp(1 - self.eps) - 1)))
            else:
                bound = 1.0 / np.sqrt(self.features)
                for p in (self.lower_entries, self.upper_entries, self.unconstrained_upper_diag):
                    p.uniform_(-bound, bound)

    # ------------------------------------------------------------------ dense factors (device tensor code)
    @property
    def upper_diag(self):
        return F.softplus(self.unconstrained_upper_diag) + self.eps

    def _create_lower_upper(self):
        """Dense (L, U) on the parameters' device: each factor is one scatter of its entries into a flat [D * D]
        buffer at the positions `lower_entry_index` / `upper_entry_index` invert (row-major i * D + j), the diagonal
        (ones for L, `upper_diag` for U) added as a diagonal matrix."""
        return dense_factors(self.lower_entries, self.upper_entries, self.upper_diag)

    def weight(self):
        lower, upper = self._create_lower_upper()
        return lower @ upper

    def weight_inverse(self):
        # rows of the identity through the inverse map give W^-T (x_row = W^-1 c_row for every row c of I)
        lower, upper = self._create_lower_upper()
        eye = torch.eye(self.features, dtype=lower.dtype, device=lower.device)
        return solve_rows(lower, upper, eye).t()

    def logabsdet(self):
        return torch.sum(torch.log(self.upper_diag))

    # ------------------------------------------------------------------ the map
    def _kernel_serves(self, inputs):
        return (inputs.dim() == 2 and inputs.dtype == torch.float32 and self.lower_entries.dtype == torch.float32
                and 2 <= self.features <= MAX_KERNEL_FEATURES)

    def _check_inputs(self, inputs):
        _require_device(inputs)
        if inputs.dim() < 2 or inputs.shape[-1] != self.features:
            raise ValueError("Expected inputs with %d features in the last dimension, got shape %s."
                             % (self.features, tuple(inputs.shape)))

    def _generic(self, inputs, inverse):
        """The reference's sequence by stock device ops (float64, other ranks, features outside the kernel's range)."""
        lower, upper = self._create_lower_upper()
        if not inverse:
            outputs = F.linear(F.linear(inputs, upper), lower, self.bias)
            logabsdet = self.logabsdet()
        else:
            outputs = solve_rows(lower, upper, (inputs - self.bias).reshape(-1, self.features)).reshape(inputs.shape)
            logabsdet = -self.logabsdet()
        return outputs, logabsdet * inputs.new_ones(outputs.shape[0])

    def _run(self, inputs, inverse, perm, scatter, accumulator):
        self._check_inputs(inputs)
        if self._kernel_serves(inputs):
            return ops.lu_linear(inputs, self.lower_entries, self.upper_entries, self.unconstrained_upper_diag,
                                 self.bias, eps=self.eps, inverse=inverse, in_perm=perm, out_scatter=scatter,
                                 accumulate_into=accumulator)
        if perm is not None:
            inputs = inputs.index_select(1, perm)
        outputs, logabsdet = self._generic(inputs, inverse)
        if scatter is not None:
            outputs = outputs.index_select(1, torch.argsort(scatter))
        if accumulator is not None:
            accumulator += logabsdet
            logabsdet = accumulator
        return outputs, logabsdet

    def forward(self, inputs, context=None, in_perm=None, logabsdet_accumulator=None):
        """`in_perm`: the layer sees inputs[:, in_perm] (a preceding Permutation, fused); `logabsdet_accumulator`: a
        [batch] running total the layer's logabsdet is added to, which is then also the returned tensor."""
        return self._run(inputs, False, in_perm, None, logabsdet_accumulator)

    def inverse(self, inputs, context=None, out_scatter=None, logabsdet_accumulator=None):
        """`out_scatter`: layer column c is stored at outputs[:, out_scatter[c]] (a following Permutation.inverse)."""
        return self._run(inputs, True, None, out_scatter, logabsdet_accumulator)

    def forward_no_cache(self, inputs):
        return self._run(inputs, False, None, None, None)

    def inverse_no_cache(self, inputs):
        return self._run(inputs, True, None, None, None)
