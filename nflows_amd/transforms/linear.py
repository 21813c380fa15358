"""Linear transforms that parameterise a weight matrix: the abstract base.

API of nflows/transforms/linear.py: `Linear(features, using_cache=False)` owns `bias`, the `using_cache` flag and a
`cache` of (weight, inverse, logabsdet) that is used in eval mode only and dropped whenever the module goes back to
training mode; subclasses provide `forward_no_cache` / `inverse_no_cache`, `weight()`, `weight_inverse()` and
`logabsdet()`.  The cached path multiplies by the cached matrices with the device's GEMM; a subclass with a kernel of
its own (LULinear) overrides `forward` / `inverse`.

`NaiveLinear(features, orthogonal_initialization=True, using_cache=False)` holds the weight matrix itself (`_weight`) and
runs on stock device ops: `F.linear` going forward, an LU factorisation with `lu_solve` going back (both in float64,
rounded once), the log-determinant from the factor's diagonal.  It has no kernel of its own: a dense [B, D] x [D, D] float32 product is the vendor
library's ground (DESIGN.md section 4, K16's timings).
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from ..utils import torchutils
from ..utils import typechecks as check
from .base import Transform


class LinearCache:
    """The three things a linear transform can keep between eval-mode calls."""

    def __init__(self):
        self.invalidate()

    def invalidate(self):
        self.weight = None
        self.inverse = None
        self.logabsdet = None


def _require_device(inputs):
    if not inputs.is_cuda:
        raise NotImplementedError(
            "nflows_amd: inputs on %s; the MI355X path has no CPU fallback" % inputs.device)


class Linear(Transform):
    """Abstract: y = W x + b with W given by the subclass's parameters."""

    def __init__(self, features, using_cache=False):
        if not check.is_positive_int(features):
            raise TypeError("Number of features must be a positive integer.")
        super().__init__()
        self.features = features
        self.bias = nn.Parameter(torch.zeros(features))
        self.using_cache = using_cache
        self.cache = LinearCache()

    # ------------------------------------------------------------------ cache
    def _cache_active(self):
        return self.using_cache and not self.training

    def _fill_cache(self, want_inverse):
        c = self.cache
        missing_matrix = (c.inverse if want_inverse else c.weight) is None
        if missing_matrix and c.logabsdet is None:
            both = self.weight_inverse_and_logabsdet() if want_inverse else self.weight_and_logabsdet()
            matrix, c.logabsdet = both
        elif missing_matrix:
            matrix = self.weight_inverse() if want_inverse else self.weight()
        elif c.logabsdet is None:
            c.logabsdet = self.logabsdet()
            return
        else:
            return
        if want_inverse:
            c.inverse = matrix
        else:
            c.weight = matrix

    def _check_forward_cache(self):
        self._fill_cache(False)

    def _check_inverse_cache(self):
        self._fill_cache(True)

    def use_cache(self, mode=True):
        if not check.is_bool(mode):
            raise TypeError("Mode must be boolean.")
        self.using_cache = mode

    def train(self, mode=True):
        if mode:
            self.cache.invalidate()   # parameters are about to move: what was cached is stale
        return super().train(mode)

    # ------------------------------------------------------------------ the map
    def forward(self, inputs, context=None):
        _require_device(inputs)
        if not self._cache_active():
            return self.forward_no_cache(inputs)
        self._check_forward_cache()
        outputs = F.linear(inputs, self.cache.weight, self.bias)
        return outputs, self.cache.logabsdet * outputs.new_ones(outputs.shape[0])

    def inverse(self, inputs, context=None):
        _require_device(inputs)
        if not self._cache_active():
            return self.inverse_no_cache(inputs)
        self._check_inverse_cache()
        outputs = F.linear(inputs - self.bias, self.cache.inverse)
        return outputs, (-self.cache.logabsdet) * outputs.new_ones(outputs.shape[0])

    def weight_and_logabsdet(self):
        """(weight(), logabsdet()); a subclass that gets both cheaper together overrides this."""
        return self.weight(), self.logabsdet()

    def weight_inverse_and_logabsdet(self):
        """(weight_inverse(), logabsdet()); as above."""
        return self.weight_inverse(), self.logabsdet()

    def forward_no_cache(self, inputs):
        raise NotImplementedError()

    def inverse_no_cache(self, inputs):
        raise NotImplementedError()

    def weight(self):
        raise NotImplementedError()

    def weight_inverse(self):
        raise NotImplementedError()

    def logabsdet(self):
        raise NotImplementedError()


class NaiveLinear(Linear):
    """y = W x + b with an unconstrained W: O(D^3) per call for the determinant or the factorisation."""

    def __init__(self, features, orthogonal_initialization=True, using_cache=False):
        super().__init__(features, using_cache)
        if orthogonal_initialization:
            self._weight = nn.Parameter(torchutils.random_orthogonal(features))
        else:
            bound = 1.0 / np.sqrt(features)
            self._weight = nn.Parameter(torch.empty(features, features).uniform_(-bound, bound))

    def _factor(self):
        """(LU, pivots, log |det W|) from one factorisation, in float64: the factor serves every row of a call and the
        determinant is one number, so nothing averages a float32 factorisation's error out; results are rounded once."""
        lu, pivots = torch.linalg.lu_factor(self._weight.double())
        return lu, pivots, torch.sum(torch.log(torch.abs(torch.diagonal(lu)))).to(self._weight.dtype)

    def forward_no_cache(self, inputs):
        _require_device(inputs)
        outputs = F.linear(inputs, self._weight, self.bias)
        return outputs, self.logabsdet() * outputs.new_ones(inputs.shape[0])

    def inverse_no_cache(self, inputs):
        _require_device(inputs)
        lu, pivots, logabsdet = self._factor()
        outputs = torch.linalg.lu_solve(lu, pivots, (inputs - self.bias).double().t()).t().to(inputs.dtype)
        return outputs, (-logabsdet) * outputs.new_ones(inputs.shape[0])

    def weight(self):
        return self._weight

    def weight_inverse(self):
        return torch.inverse(self._weight.double()).to(self._weight.dtype)

    def weight_inverse_and_logabsdet(self):
        lu, pivots, logabsdet = self._factor()
        identity = torch.eye(self.features, dtype=self._weight.dtype, device=self._weight.device)
        return torch.linalg.lu_solve(lu, pivots, identity.double()).to(self._weight.dtype), logabsdet

    def logabsdet(self):
        return torchutils.logabsdet(self._weight.double()).to(self._weight.dtype)
