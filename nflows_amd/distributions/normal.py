"""The normal base distributions (reference: nflows/distributions/normal.py): `StandardNormal` (:11-50),
`ConditionalDiagonalNormal` (:53-132) and `DiagonalNormal` (:135-180).

`_log_prob` on a HIP float32 tensor is one fused kernel (StandardNormal: square, per-sample sum, -0.5*, -log_z; the
diagonal normals: K20 "diag", csrc/density.hip).  `_log_z` is a non-persistent float64 0-dim buffer exactly like the
reference, so state_dicts match.

The diagonal normals hand K20 a contiguous float32 device tensor of rank >= 2: `DiagonalNormal` its own [1, N] parameters
(one shared row), `ConditionalDiagonalNormal` the encoder's contiguous [B, 2 N] output whole -- both halves are read in
place and the gradient arrives as one [B, 2 N] tensor.  Everything else -- CPU tensors, float64, non-contiguous inputs, an
encoder output of another shape -- runs the reference's sequence on stock ops (`_generic_log_prob`).  `Flow` passes its
logabsdet as `logabsdet=`: on the kernel it is added inside the float64 row sum before the single rounding.
"""
import numpy as np
import torch
from torch import nn

from .. import ops
from ..utils import torchutils
from .base import Distribution


class StandardNormal(Distribution):
    """Zero-mean, unit-covariance Gaussian over tensors of shape `shape`."""

    def __init__(self, shape):
        super().__init__()
        self._shape = torch.Size(shape)
        self.register_buffer(
            "_log_z", torch.tensor(0.5 * np.prod(shape) * np.log(2 * np.pi), dtype=torch.float64),
            persistent=False)

    def _log_prob(self, inputs, context):
        if inputs.shape[1:] != self._shape:
            raise ValueError("Expected input of shape {}, got {}".format(self._shape, inputs.shape[1:]))
        return ops.standard_normal_log_prob(inputs)

    def _sample(self, num_samples, context):
        if context is None:
            return torch.randn(num_samples, *self._shape, device=self._log_z.device)
        rows = context.shape[0]
        draws = torch.randn(rows * num_samples, *self._shape, device=context.device)
        return torchutils.split_leading_dim(draws, [rows, num_samples])

    def _mean(self, context):
        if context is None:
            return self._log_z.new_zeros(self._shape)
        return context.new_zeros(context.shape[0], *self._shape)


def _shape_error(expected, got):
    return ValueError("Expected input of shape {}, got {}".format(expected, got))


def _generic_log_prob(inputs, means, log_stds, log_z):
    """The reference's sequence (normal.py:107-114) on stock ops."""
    norm_inputs = (inputs - means) * torch.exp(-log_stds)
    log_prob = -0.5 * torchutils.sum_except_batch(norm_inputs ** 2, num_batch_dims=1)
    log_prob -= torchutils.sum_except_batch(log_stds, num_batch_dims=1)
    log_prob -= log_z
    return log_prob


def _kernel_serves(inputs, *params):
    return (inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() >= 2 and inputs.is_contiguous()
            and inputs.numel() > 0
            and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.device == inputs.device for p in params))


class _DiagonalBase(Distribution):
    # test and measurement switch: False = always the generic path (tools/density_time.py, tests/test_gpu_density.py)
    _use_kernel = True

    def log_prob(self, inputs, context=None, logabsdet=None):
        """`Distribution.log_prob`; `logabsdet` [batch] (what `Flow` adds to the base density, flows/base.py:49) is added to
        the result -- on the kernel inside the float64 row sum, before the single rounding."""
        inputs = torch.as_tensor(inputs)
        context = None if context is None else torch.as_tensor(context)
        if context is not None and context.shape[0] != inputs.shape[0]:
            raise ValueError("Number of input items must be equal to number of context items.")
        return self._log_prob(inputs, context, logabsdet=logabsdet)


class ConditionalDiagonalNormal(_DiagonalBase):
    """A diagonal multivariate Normal whose parameters are functions of a context."""

    def __init__(self, shape, context_encoder=None):
        """shape: list, tuple or torch.Size, the shape of the input variables.
        context_encoder: callable or None, encodes the context to the distribution parameters ([..., 2 N]: means, then
            log stds); None: the identity."""
        super().__init__()
        self._shape = torch.Size(shape)
        if context_encoder is None:
            self._context_encoder = lambda x: x
        else:
            self._context_encoder = context_encoder
        self.register_buffer(
            "_log_z", torch.tensor(0.5 * np.prod(shape) * np.log(2 * np.pi), dtype=torch.float64), persistent=False)

    def _encode(self, context):
        if context is None:
            raise ValueError("Context can't be None.")
        params = self._context_encoder(context)
        if params.shape[-1] % 2 != 0:
            raise RuntimeError("The context encoder must return a tensor whose last dimension is even.")
        if params.shape[0] != context.shape[0]:
            raise RuntimeError("The batch dimension of the parameters is inconsistent with the input.")
        return params

    def _split(self, params):
        split = params.shape[-1] // 2
        means = params[..., :split].reshape(params.shape[0], *self._shape)
        log_stds = params[..., split:].reshape(params.shape[0], *self._shape)
        return means, log_stds

    def _compute_params(self, context):
        """Compute the means and log stds form the context."""
        return self._split(self._encode(context))

    def _log_prob(self, inputs, context, logabsdet=None):
        if inputs.shape[1:] != self._shape:
            raise _shape_error(self._shape, inputs.shape[1:])
        params = self._encode(context)
        n = int(np.prod(self._shape))
        if (self._use_kernel and params.dim() == 2 and params.shape[1] == 2 * n and _kernel_serves(inputs, params)
                and (logabsdet is None or _kernel_serves(inputs, logabsdet))):
            return ops.diag_normal_log_prob(inputs, params, None, self._log_z, logabsdet)   # the encoder output whole
        means, log_stds = self._split(params)
        assert means.shape == inputs.shape and log_stds.shape == inputs.shape
        log_prob = _generic_log_prob(inputs, means, log_stds, self._log_z)
        return log_prob if logabsdet is None else log_prob + logabsdet

    def _sample(self, num_samples, context):
        means, log_stds = self._compute_params(context)
        stds = torch.exp(log_stds)
        means = torchutils.repeat_rows(means, num_samples)
        stds = torchutils.repeat_rows(stds, num_samples)
        context_size = context.shape[0]
        noise = torch.randn(context_size * num_samples, *self._shape, device=means.device)
        samples = means + stds * noise
        return torchutils.split_leading_dim(samples, [context_size, num_samples])

    def _mean(self, context):
        means, _ = self._compute_params(context)
        return means


class DiagonalNormal(_DiagonalBase):
    """A diagonal multivariate Normal with trainable parameters."""

    def __init__(self, shape):
        """shape: list, tuple or torch.Size, the shape of the input variables."""
        super().__init__()
        self._shape = torch.Size(shape)
        self.mean_ = nn.Parameter(torch.zeros(shape).reshape(1, -1))
        self.log_std_ = nn.Parameter(torch.zeros(shape).reshape(1, -1))
        self.register_buffer(
            "_log_z", torch.tensor(0.5 * np.prod(shape) * np.log(2 * np.pi), dtype=torch.float64), persistent=False)

    def _log_prob(self, inputs, context, logabsdet=None):
        if inputs.shape[1:] != self._shape:
            raise _shape_error(self._shape, inputs.shape[1:])
        means, log_stds = self.mean_, self.log_std_
        if (self._use_kernel and _kernel_serves(inputs, means, log_stds)
                and (logabsdet is None or _kernel_serves(inputs, logabsdet))):
            return ops.diag_normal_log_prob(inputs, means, log_stds, self._log_z, logabsdet)
        # (the [1, N] parameters in the inputs' shape: the reference's broadcast serves one-dimensional shapes only)
        log_prob = _generic_log_prob(inputs, means.reshape(1, *self._shape), log_stds.reshape(1, *self._shape), self._log_z)
        return log_prob if logabsdet is None else log_prob + logabsdet

    def _sample(self, num_samples, context):
        raise NotImplementedError()

    def _mean(self, context):
        """The reference returns `self.mean`, an attribute that does not exist (normal.py:179-180: an AttributeError on
        every call); this returns the parameter it means, `self.mean_`."""
        return self.mean_
