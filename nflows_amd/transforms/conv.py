"""The invertible 1x1 convolution of Glow: an LU linear layer over the channels of an image, behind a fixed channel
permutation.

API of nflows/transforms/conv.py: `OneByOneConvolution(num_channels, using_cache=False, identity_init=True)`, a subclass
of `LULinear` with the submodule `permutation = RandomPermutation(num_channels, dim=1)` (state dict: `bias`,
`lower_entries`, `upper_entries`, `unconstrained_upper_diag`, `permutation._permutation`).  Per pixel
forward y = L (U x[perm]) + b, inverse x[perm] = U^-1 (L^-1 (y - b)); logabsdet = +- H W sum_i log U_ii per image.

The reference permutes the channels, moves them last, flattens the pixels to rows, runs LULinear and undoes both.  On a
HIP device a float32 [B, C, H, W] tensor with 2 <= C <= 128 goes through K19 in every mode instead: one launch per
direction that reads and writes NCHW as it is, the permutation inside it (a plane of consecutive pixels is already the
column-major tile K16 works on).  float64, C == 1 and C > 128: the reference's own sequence by stock device ops.
"""
import torch

from .. import ops
from .linear import _require_device
from .lu import LULinear, MAX_KERNEL_FEATURES
from .permutations import RandomPermutation


class OneByOneConvolution(LULinear):
    supports_fused_permutation = False   # the permutation this layer needs is its own; 4-D inputs are never offered another

    def __init__(self, num_channels, using_cache=False, identity_init=True):
        super().__init__(num_channels, using_cache, identity_init)
        self.permutation = RandomPermutation(num_channels, dim=1)   # after the parameters: the reference's RNG order

    def _kernel_serves(self, inputs):
        return (inputs.dtype == torch.float32 and self.lower_entries.dtype == torch.float32
                and 2 <= self.features <= MAX_KERNEL_FEATURES)

    def _run(self, inputs, inverse):
        if inputs.dim() != 4:
            raise ValueError("Inputs must be a 4D tensor.")
        if inputs.shape[1] != self.features:
            raise ValueError("Expected inputs with %d channels, got shape %s." % (self.features, tuple(inputs.shape)))
        _require_device(inputs)
        perm = self.permutation._permutation
        if self._kernel_serves(inputs):
            return ops.lu_conv1x1(inputs, self.lower_entries, self.upper_entries, self.unconstrained_upper_diag,
                                  self.bias, eps=self.eps, inverse=inverse, channel_perm=perm)
        b, c, h, w = inputs.shape
        if not inverse:
            inputs = inputs.index_select(1, perm)
        rows = inputs.permute(0, 2, 3, 1).reshape(b * h * w, c)
        outputs, logabsdet = self._generic(rows, inverse)
        outputs = outputs.reshape(b, h, w, c).permute(0, 3, 1, 2)
        if inverse:
            outputs = outputs.index_select(1, self.permutation._inverse_permutation)
        return outputs, logabsdet.reshape(b, h * w).sum(1)

    def forward(self, inputs, context=None):
        return self._run(inputs, False)

    def inverse(self, inputs, context=None):
        return self._run(inputs, True)

    def forward_no_cache(self, inputs):
        return self._run(inputs, False)

    def inverse_no_cache(self, inputs):
        return self._run(inputs, True)
