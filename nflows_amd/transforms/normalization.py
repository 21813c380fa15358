"""Normalisation transforms: BatchNorm and ActNorm.

API of nflows/transforms/normalization.py: `BatchNorm(features, eps=1e-5, momentum=0.1, affine=True)` with parameters
`unconstrained_weight` (weight = softplus(.) + eps) and `bias`, buffers `running_mean` and `running_var` (initially ZERO,
both updated with the batch's mean and UNBIASED variance by every training-mode forward; `affine` is accepted and ignored;
no inverse in training mode), and `ActNorm(features)` with parameters `log_scale`, `shift` and the buffer `initialized`
(set by the first TRAINING-mode forward, which makes that batch's outputs zero-mean / unit-variance per column).

On a HIP device a float32 [batch, features] tensor with features <= 1024 goes through K17 (csrc/norm.hip) in every mode
(differentiated passes of fewer than 2^23 elements excepted: AUTOGRAD_MIN_ELEMENTS below, with its measurement):
one launch for the per-column map -- it reads the module's tensors as they are, so an optimizer step or a `.data` write is
seen by the next call --, two small launches in front of it for the batch statistics where they are taken (a deterministic
column reduction in float64).  Next to a column Permutation inside `CompositeTransform` the permutation is folded into the
kernel's gather / scatter and the composite's `total_logabsdet +=` into its store.  Everything else -- float64, ActNorm on
4-D images, wider inputs, batch statistics of fewer than two rows (NaN, as in the reference) -- runs the same sequence by
stock device ops.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from .. import ops
from ..utils import typechecks as check
from .base import InverseNotAvailable, Transform
from .linear import _require_device


# The dispatch rule of the differentiated passes, from profiles/norm_time.json (tools/norm_time.py on one MI355X, DESIGN.md
# section 4, K17).  Without autograd K17 is faster than the stock sequence in every measured case.  Under autograd its
# backward forms the [D] coefficient and parameter-gradient vectors with about two dozen small float64 launches of stock
# ops, and that host-bound part decides small shapes: BatchNorm training forward + backward, median call in us, K17 against
# generic -- 16 384 x 64: 471 / 351 and 16 384 x 128: 531 / 369 (K17 LOSES), 16 384 x 16: 441 / 373 and 262 144 x 16: 457 / 443
# (inside the spread, K17 behind on the median); 16 384 x 784: 550 / 685, 262 144 x 64: 580 / 739 and everything larger (K17
# wins, up to 3 x).  The losing shapes have at most 2^22 elements, the winning ones at least 1.28e7: passes that will be
# differentiated take the generic path below 2^23 elements.  (Measured for BatchNorm in training mode only; applied to the
# eval-mode and ActNorm gradients as well, whose backward has the same host-bound part.)
AUTOGRAD_MIN_ELEMENTS = 1 << 23


class _ColumnNorm(Transform):
    supports_fused_permutation = True   # K17 gathers / scatters columns and adds into a running logabsdet
    # measurement and test switch: True = the dispatch rule above, False = always the generic path, "always" = K17
    # wherever it serves the shape, whatever the rule says (tools/norm_time.py, tests/test_gpu_normalization.py)
    _use_kernel = True

    def _kernel_serves(self, inputs):
        if self._use_kernel is False:
            return False
        params = list(self.parameters(recurse=False))
        served = (inputs.dim() == 2 and inputs.dtype == torch.float32 and inputs.shape[1] == self.features
                  and self.features <= ops.NORM_MAX_FEATURES and all(p.dtype == torch.float32 for p in params))
        if served and self._use_kernel is True and inputs.numel() < AUTOGRAD_MIN_ELEMENTS and torch.is_grad_enabled() \
                and (inputs.requires_grad or any(p.requires_grad for p in params)):
            return False
        return served

    def _run(self, inputs, inverse, perm, scatter, accumulator):
        _require_device(inputs)
        if self._kernel_serves(inputs):
            return self._kernel(inputs, inverse, perm, scatter, accumulator)
        if perm is not None:
            inputs = inputs.index_select(1, perm)
        outputs, logabsdet = self._generic(inputs, inverse)
        if scatter is not None:
            outputs = outputs.index_select(1, torch.argsort(scatter))
        if accumulator is not None:
            accumulator += logabsdet
            logabsdet = accumulator
        return outputs, logabsdet


class BatchNorm(_ColumnNorm):
    """Batch normalisation of [batch, features] inputs; the inverse exists in eval mode only."""

    def __init__(self, features, eps=1e-5, momentum=0.1, affine=True):
        if not check.is_positive_int(features):
            raise TypeError("Number of features must be a positive integer.")
        super().__init__()
        self.features = features
        self.momentum = momentum
        self.eps = eps
        logit = np.log(np.exp(1 - eps) - 1)    # softplus(logit) + eps = 1
        self.unconstrained_weight = nn.Parameter(logit * torch.ones(features))
        self.bias = nn.Parameter(torch.zeros(features))
        self.register_buffer("running_mean", torch.zeros(features))
        self.register_buffer("running_var", torch.zeros(features))

    @property
    def weight(self):
        return F.softplus(self.unconstrained_weight) + self.eps

    @staticmethod
    def _check_rank(inputs):
        if inputs.dim() != 2:
            raise ValueError("Expected 2-dim inputs, got inputs of shape: {}".format(inputs.shape))

    def _update_running(self, mean, var):
        with torch.no_grad():
            self.running_mean.mul_(1 - self.momentum).add_(mean.detach() * self.momentum)
            self.running_var.mul_(1 - self.momentum).add_(var.detach() * self.momentum)

    def _kernel_serves(self, inputs):
        # (batch statistics of fewer than two rows: the reference's NaN, by the reference's sequence)
        return super()._kernel_serves(inputs) and not (self.training and inputs.shape[0] < 2)

    def _kernel(self, inputs, inverse, perm, scatter, accumulator):
        if self.training:
            mean, var = ops.column_stats(inputs)
            if perm is not None:
                mean, var = mean.index_select(0, perm), var.index_select(0, perm)
            self._update_running(mean, var)
        else:
            mean, var = self.running_mean, self.running_var
        return ops.batch_norm(inputs, self.unconstrained_weight, self.bias, mean, var, eps=self.eps, inverse=inverse,
                              batch_statistics=self.training, in_perm=perm, out_scatter=scatter, accumulate_into=accumulator)

    def _generic(self, inputs, inverse):
        weight = self.weight
        if inverse:
            spread = torch.sqrt(self.running_var + self.eps)
            outputs = spread * ((inputs - self.bias) / weight) + self.running_mean
            logabsdet = torch.sum(0.5 * torch.log(self.running_var + self.eps) - torch.log(weight))
        else:
            if self.training:
                mean, var = inputs.mean(0), inputs.var(0)
                self._update_running(mean, var)
            else:
                mean, var = self.running_mean, self.running_var
            outputs = weight * ((inputs - mean) / torch.sqrt(var + self.eps)) + self.bias
            logabsdet = torch.sum(torch.log(weight) - 0.5 * torch.log(var + self.eps))
        return outputs, logabsdet * inputs.new_ones(inputs.shape[0])

    def forward(self, inputs, context=None, in_perm=None, logabsdet_accumulator=None):
        """`in_perm`: the layer sees inputs[:, in_perm] (a preceding Permutation, fused); `logabsdet_accumulator`: a
        [batch] running total the layer's logabsdet is added to, which is then also the returned tensor."""
        self._check_rank(inputs)
        return self._run(inputs, False, in_perm, None, logabsdet_accumulator)

    def inverse(self, inputs, context=None, out_scatter=None, logabsdet_accumulator=None):
        """`out_scatter`: layer column c is stored at outputs[:, out_scatter[c]] (a following Permutation.inverse)."""
        if self.training:
            raise InverseNotAvailable("Batch norm inverse is only available in eval mode, not in training mode.")
        self._check_rank(inputs)
        return self._run(inputs, True, None, out_scatter, logabsdet_accumulator)


class ActNorm(_ColumnNorm):
    """Activation normalisation (Kingma & Dhariwal 2018) of [batch, features] or [batch, channels, H, W] inputs, with the
    data-dependent initialisation from the first training-mode batch."""

    def __init__(self, features):
        if not check.is_positive_int(features):
            raise TypeError("Number of features must be a positive integer.")
        super().__init__()
        self.features = features
        self.register_buffer("initialized", torch.tensor(False, dtype=torch.bool))
        self.log_scale = nn.Parameter(torch.zeros(features))
        self.shift = nn.Parameter(torch.zeros(features))

    @property
    def scale(self):
        return torch.exp(self.log_scale)

    def _broadcastable_scale_shift(self, inputs):
        shape = (1, -1, 1, 1) if inputs.dim() == 4 else (1, -1)
        return self.scale.view(shape), self.shift.view(shape)

    def _initialize(self, inputs):
        """log_scale = -log(std), shift = -mean(x / std) per column (per channel of 4-D inputs), std unbiased."""
        with torch.no_grad():
            if self._kernel_serves(inputs) and inputs.shape[0] >= 2:
                _, _, (mean, var) = ops.column_stats(inputs, return_f64=True)   # K17: the statistics in float64 ...
                std = torch.sqrt(var)
                log_scale, shift = (-torch.log(std)).float(), (-(mean / std)).float()   # ... each parameter rounded once
            else:
                rows = inputs
                if inputs.dim() == 4:
                    rows = inputs.permute(0, 2, 3, 1).reshape(-1, inputs.shape[1])
                std = rows.std(dim=0)
                log_scale, shift = -torch.log(std), -(rows / std).mean(dim=0)
            self.log_scale.data = log_scale.to(self.log_scale.dtype)
            self.shift.data = shift.to(self.shift.dtype)
            self.initialized.data = torch.ones_like(self.initialized)

    def _kernel(self, inputs, inverse, perm, scatter, accumulator):
        return ops.act_norm(inputs, self.log_scale, self.shift, inverse=inverse, in_perm=perm, out_scatter=scatter,
                            accumulate_into=accumulator)

    def _generic(self, inputs, inverse):
        scale, shift = self._broadcastable_scale_shift(inputs)
        pixels = inputs.shape[2] * inputs.shape[3] if inputs.dim() == 4 else 1
        if inverse:
            outputs = (inputs - shift) / scale
            logabsdet = -pixels * torch.sum(self.log_scale)
        else:
            outputs = scale * inputs + shift
            logabsdet = pixels * torch.sum(self.log_scale)
        return outputs, logabsdet * outputs.new_ones(inputs.shape[0])

    @staticmethod
    def _check_rank(inputs):
        if inputs.dim() not in (2, 4):
            raise ValueError("Expecting inputs to be a 2D or a 4D tensor.")

    def forward(self, inputs, context=None, in_perm=None, logabsdet_accumulator=None):
        """`in_perm` / `logabsdet_accumulator`: as `BatchNorm.forward`."""
        self._check_rank(inputs)
        _require_device(inputs)
        if self.training and not self.initialized:
            self._initialize(inputs if in_perm is None else inputs.index_select(1, in_perm))
        return self._run(inputs, False, in_perm, None, logabsdet_accumulator)

    def inverse(self, inputs, context=None, out_scatter=None, logabsdet_accumulator=None):
        """`out_scatter`: as `BatchNorm.inverse`."""
        self._check_rank(inputs)
        return self._run(inputs, True, None, out_scatter, logabsdet_accumulator)
