"""The transforms of nflows/transforms/nonlinearities.py.

Elementwise nonlinearities (:18-223): `Exp`, `Tanh`, `LogTanh`, `LeakyReLU`, `Sigmoid` / `Logit`, `CauchyCDF` /
`CauchyCDFInverse`, `GatedLinearUnit` and `CompositeCDFTransform`, with the reference's names, constructor signatures, error
messages and state.  On a HIP device a contiguous float32 tensor of rank >= 2 goes through K18 (csrc/nonlin.hip): ONE launch
that reads the tensor once, writes the outputs and the per-row logabsdet (summed over everything but dimension 0 in float64,
in a fixed order, rounded once); Sigmoid's temperature is read from the module's own [1] tensor, so an optimizer step or a
`.data` write is seen by the next call.  Everything else -- float64, rank 1, non-contiguous inputs -- runs the reference's
sequence by stock device ops (`_generic`).  `GatedLinearUnit` is a gate from the context: stock ops, no kernel.

Batch-shared spline CDF transforms (:230-319, :386-467), the members of that module on the hot path: the spline coupling
layers apply them to their identity half when `apply_unconditional_transform=True` (coupling.py:318-330, :524-535).
Parameters have shape [*shape, K] and are shared by every sample.  Without grad the K6 kernel
builds each feature's knots once per workgroup in LDS; with grad the logits are broadcast over
the batch and the differentiable elementwise functional is used (autograd then reduces the
gradient over the batch, exactly like the reference's `_share_across_batch`).
"""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from .. import autograd as AG
from .. import ops
from ..utils import torchutils
from .base import CompositeTransform, InputOutsideDomain, InverseTransform, Transform
from .linear import _require_device
from .splines import rational_quadratic
from . import splines


# The dispatch rule of the differentiated passes: differentiated passes of fewer elements than this take the generic path.
# From profiles/nonlin_time.json (tools/nonlin_time.py): in no timed case, differentiated ones
# included, is K18 slower than the generic path beyond that path's own spread (the closest: Sigmoid forward + backward at
# 16 384 x 64, single calls, 228.6 us against 206.6 us [193.8-398.9]; back to back 81.4 against 198.3), so no shape is excepted.
AUTOGRAD_MIN_ELEMENTS = 0


class _Elementwise(Transform):
    """An elementwise map with a per-row logabsdet: K18 where it serves the tensor, the reference's sequence elsewhere."""
    _kind = None
    # measurement and test switch: True = the dispatch rule above, False = always the generic path, "always" = K18 wherever
    # it serves the tensor, whatever the rule says (tools/nonlin_time.py, tests/test_gpu_nonlinearities.py)
    _use_kernel = True
    # The generic path on float32 inputs runs the reference's sequence in float64 and rounds each result once.  The stock
    # float32 device functions are not as close to float64 as the reference's CPU ones: `Exp.inverse` by the device's float32
    # `log` had a mean error of 4.8e-8 against float64 on the 1021 x 67 fixture where the reference's own is 1.6e-8, and the
    # parity rule allows twice that.  False = the plain float32 sequence: tools/nonlin_time.py
    # times it as what stock ops cost without that guarantee.
    _generic_wide = True

    def _constants(self):
        return ()

    def _temperature(self):
        return None

    def _kernel_serves(self, inputs):
        if self._use_kernel is False:
            return False
        t = self._temperature()
        served = (inputs.dim() >= 2 and inputs.dtype == torch.float32 and inputs.is_contiguous() and inputs.numel() > 0
                  and (t is None or t.dtype == torch.float32))
        if served and self._use_kernel is True and inputs.numel() < AUTOGRAD_MIN_ELEMENTS \
                and AG.needs_grad(inputs, t):
            return False
        return served

    def _run(self, inputs, inverse):
        _require_device(inputs)
        if inputs.numel() == 0:
            return inputs.clone(), inputs.new_zeros(inputs.shape[0])
        if self._kernel_serves(inputs):
            return ops.nonlinearity(inputs, self._kind, self._constants(), self._temperature(), inverse=inverse)
        if inputs.dtype == torch.float32 and self._generic_wide:
            outputs, logabsdet = self._generic(inputs.double(), inverse)
            return outputs.to(torch.float32), logabsdet.to(torch.float32)
        return self._generic(inputs, inverse)

    def forward(self, inputs, context=None):
        return self._run(inputs, False)

    def inverse(self, inputs, context=None):
        return self._run(inputs, True)


class Exp(_Elementwise):
    _kind = "exp"

    def _generic(self, inputs, inverse):
        if not inverse:
            return torch.exp(inputs), torchutils.sum_except_batch(inputs, num_batch_dims=1)
        if torch.min(inputs) <= 0.:
            raise InputOutsideDomain()
        outputs = torch.log(inputs)
        return outputs, -torchutils.sum_except_batch(outputs, num_batch_dims=1)


class Tanh(_Elementwise):
    _kind = "tanh"

    def _generic(self, inputs, inverse):
        if not inverse:
            outputs = torch.tanh(inputs)
            logabsdet = torch.log(1 - outputs ** 2)
        else:
            if torch.min(inputs) <= -1 or torch.max(inputs) >= 1:
                raise InputOutsideDomain()
            outputs = 0.5 * torch.log((1 + inputs) / (1 - inputs))
            logabsdet = -torch.log(1 - inputs ** 2)
        return outputs, torchutils.sum_except_batch(logabsdet, num_batch_dims=1)


class LogTanh(_Elementwise):
    """Tanh with unbounded output: beyond +-cut_point the map continues as +-alpha * log(beta * |x|), alpha and beta set so
    that value and first derivative match tanh's at the cut point (float64 on the host, as the reference's numpy)."""
    _kind = "log_tanh"

    def __init__(self, cut_point=1):
        if cut_point <= 0:
            raise ValueError("Cut point must be positive.")
        super().__init__()
        self.cut_point = cut_point
        self.inv_cut_point = np.tanh(cut_point)
        self.alpha = (1 - np.tanh(np.tanh(cut_point))) / cut_point
        self.beta = np.exp((np.tanh(cut_point) - self.alpha * np.log(cut_point)) / self.alpha)

    def _constants(self):
        return (self.cut_point, self.alpha, self.beta)

    def _generic(self, inputs, inverse):
        cut = self.inv_cut_point if inverse else self.cut_point
        right = inputs > cut
        left = inputs < -cut
        middle = ~(right | left)
        outputs = torch.zeros_like(inputs)
        logabsdet = torch.zeros_like(inputs)
        if not inverse:
            outputs[middle] = torch.tanh(inputs[middle])
            outputs[right] = self.alpha * torch.log(self.beta * inputs[right])
            outputs[left] = self.alpha * -torch.log(-self.beta * inputs[left])
            logabsdet[middle] = torch.log(1 - outputs[middle] ** 2)
            logabsdet[right] = torch.log(self.alpha / inputs[right])
            logabsdet[left] = torch.log(-self.alpha / inputs[left])
        else:
            outputs[middle] = 0.5 * torch.log((1 + inputs[middle]) / (1 - inputs[middle]))
            outputs[right] = torch.exp(inputs[right] / self.alpha) / self.beta
            outputs[left] = -torch.exp(-inputs[left] / self.alpha) / self.beta
            logabsdet[middle] = -torch.log(1 - inputs[middle] ** 2)
            logabsdet[right] = -np.log(self.alpha * self.beta) + inputs[right] / self.alpha
            logabsdet[left] = -np.log(self.alpha * self.beta) - inputs[left] / self.alpha
        return outputs, torchutils.sum_except_batch(logabsdet, num_batch_dims=1)


class LeakyReLU(_Elementwise):
    _kind = "leaky_relu"

    def __init__(self, negative_slope=1e-2):
        if negative_slope <= 0:
            raise ValueError("Slope must be positive.")
        super().__init__()
        self.negative_slope = negative_slope
        self.log_negative_slope = torch.log(torch.as_tensor(self.negative_slope))

    def _constants(self):
        return (self.negative_slope,)

    def _generic(self, inputs, inverse):
        # (the reference's mask is a float32 CPU tensor, `.type(torch.Tensor)`; here it stays on the inputs' device and,
        #  for float64 inputs, in float64 with the slope's logarithm in float64 as well)
        slope = (1 / self.negative_slope) if inverse else self.negative_slope
        outputs = F.leaky_relu(inputs, negative_slope=slope)
        mask = (inputs < 0).to(inputs.dtype)
        log_slope = self.log_negative_slope.to(inputs.device) if inputs.dtype == torch.float32 else math.log(self.negative_slope)
        logabsdet = (-log_slope if inverse else log_slope) * mask
        return outputs, torchutils.sum_except_batch(logabsdet, num_batch_dims=1)


class Sigmoid(_Elementwise):
    _kind = "sigmoid"

    def __init__(self, temperature=1, eps=1e-6, learn_temperature=False):
        super().__init__()
        self.eps = eps
        if learn_temperature:
            self.temperature = nn.Parameter(torch.Tensor([temperature]))
        else:
            self.register_buffer("temperature", torch.Tensor([temperature]))

    def _constants(self):
        return (self.eps,)

    def _temperature(self):
        return self.temperature

    def _generic(self, inputs, inverse):
        temperature = self.temperature.to(inputs.dtype)   # (float64 with the widened float32 inputs)
        if not inverse:
            inputs = temperature * inputs
            outputs = torch.sigmoid(inputs)
            logabsdet = torchutils.sum_except_batch(torch.log(temperature) - F.softplus(-inputs) - F.softplus(inputs))
            return outputs, logabsdet
        if torch.min(inputs) < 0 or torch.max(inputs) > 1:
            raise InputOutsideDomain()
        inputs = torch.clamp(inputs, self.eps, 1 - self.eps)
        outputs = (1 / temperature) * (torch.log(inputs) - torch.log1p(-inputs))
        logabsdet = -torchutils.sum_except_batch(torch.log(temperature) - F.softplus(-temperature * outputs)
                                                 - F.softplus(temperature * outputs))
        return outputs, logabsdet


class Logit(InverseTransform):
    def __init__(self, temperature=1, eps=1e-6):
        super().__init__(Sigmoid(temperature=temperature, eps=eps))


class GatedLinearUnit(Transform):
    """A gate from the context: stock device ops, no kernel."""

    def __init__(self):
        super().__init__()

    def forward(self, inputs, context=None):
        _require_device(inputs)
        gate = torch.sigmoid(context)
        return inputs * gate, torch.log(gate).reshape(-1)

    def inverse(self, inputs, context=None):
        _require_device(inputs)
        gate = torch.sigmoid(context)
        return inputs / gate, -torch.log(gate).reshape(-1)


class CauchyCDF(_Elementwise):
    _kind = "cauchy_cdf"

    def __init__(self, location=None, scale=None, features=None):
        super().__init__()

    def _generic(self, inputs, inverse):
        if not inverse:
            outputs = (1 / np.pi) * torch.atan(inputs) + 0.5
            return outputs, torchutils.sum_except_batch(-np.log(np.pi) - torch.log(1 + inputs ** 2))
        if torch.min(inputs) < 0 or torch.max(inputs) > 1:
            raise InputOutsideDomain()
        outputs = torch.tan(np.pi * (inputs - 0.5))
        return outputs, -torchutils.sum_except_batch(-np.log(np.pi) - torch.log(1 + outputs ** 2))


class CauchyCDFInverse(InverseTransform):
    def __init__(self, location=None, scale=None, features=None):
        super().__init__(CauchyCDF(location=location, scale=scale, features=features))


class CompositeCDFTransform(CompositeTransform):
    def __init__(self, squashing_transform, cdf_transform):
        super().__init__([squashing_transform, cdf_transform, InverseTransform(squashing_transform)])


class PiecewiseRationalQuadraticCDF(Transform):
    def __init__(self, shape, num_bins=10, tails=None, tail_bound=1.0, identity_init=False,
                 min_bin_width=rational_quadratic.DEFAULT_MIN_BIN_WIDTH,
                 min_bin_height=rational_quadratic.DEFAULT_MIN_BIN_HEIGHT,
                 min_derivative=rational_quadratic.DEFAULT_MIN_DERIVATIVE):
        super().__init__()
        self.min_bin_width = min_bin_width
        self.min_bin_height = min_bin_height
        self.min_derivative = min_derivative
        self.tail_bound = tail_bound
        self.tails = tails
        if isinstance(shape, int):
            shape = (shape,)
        num_derivatives = (num_bins - 1) if self.tails == "linear" else (num_bins + 1)
        if identity_init:
            self.unnormalized_widths = nn.Parameter(torch.zeros(*shape, num_bins))
            self.unnormalized_heights = nn.Parameter(torch.zeros(*shape, num_bins))
            constant = np.log(np.exp(1 - min_derivative) - 1)
            self.unnormalized_derivatives = nn.Parameter(constant * torch.ones(*shape, num_derivatives))
        else:  # same RNG consumption order as the reference
            self.unnormalized_widths = nn.Parameter(torch.rand(*shape, num_bins))
            self.unnormalized_heights = nn.Parameter(torch.rand(*shape, num_bins))
            self.unnormalized_derivatives = nn.Parameter(torch.rand(*shape, num_derivatives))

    def _spline(self, inputs, inverse=False):
        if self.tails is not None and self.tails != "linear":
            raise RuntimeError("{} tails are not implemented.".format(self.tails))
        uw, uh, ud = self.unnormalized_widths, self.unnormalized_heights, self.unnormalized_derivatives
        if inputs.shape[1:] != uw.shape[:-1]:
            raise ValueError("Expected inputs of shape [batch, {}], got {}".format(
                tuple(uw.shape[:-1]), tuple(inputs.shape)))
        if AG.needs_grad(inputs, uw, uh, ud):
            batch = inputs.shape[0]

            def share(p):
                return p[None, ...].expand(batch, *p.shape)
            if self.tails is None:
                y, lad = rational_quadratic.rational_quadratic_spline(
                    inputs, share(uw), share(uh), share(ud), inverse=inverse,
                    min_bin_width=self.min_bin_width, min_bin_height=self.min_bin_height,
                    min_derivative=self.min_derivative)
            else:
                y, lad = rational_quadratic.unconstrained_rational_quadratic_spline(
                    inputs, share(uw), share(uh), share(ud), inverse=inverse, tails=self.tails,
                    tail_bound=self.tail_bound, min_bin_width=self.min_bin_width,
                    min_bin_height=self.min_bin_height, min_derivative=self.min_derivative)
            return y, torchutils.sum_except_batch(lad)
        spec = ops.make_rqs_spec(uw.shape[-1], self.tails, tail_bound=self.tail_bound,
                                 min_bin_width=self.min_bin_width, min_bin_height=self.min_bin_height,
                                 min_derivative=self.min_derivative)
        return ops.rqs_shared(inputs, uw, uh, ud, spec, inverse)

    def forward(self, inputs, context=None):
        return self._spline(inputs, inverse=False)

    def inverse(self, inputs, context=None):
        return self._spline(inputs, inverse=True)


def _share_across_batch(params, batch_size):
    return params[None, ...].expand(batch_size, *params.shape)


class PiecewiseLinearCDF(Transform):
    """Piecewise-linear CDF with one parameter set [*shape, K] shared by every sample
    (nonlinearities.py:230-263)."""

    def __init__(self, shape, num_bins=10, tails=None, tail_bound=1.0):
        super().__init__()
        self.tail_bound = tail_bound
        self.tails = tails
        self.unnormalized_pdf = nn.Parameter(torch.randn(*shape, num_bins))

    def _spline(self, inputs, inverse=False):
        pdf = _share_across_batch(self.unnormalized_pdf, inputs.shape[0])
        if self.tails is None:
            outputs, logabsdet = splines.linear_spline(inputs, pdf, inverse=inverse)
        else:
            outputs, logabsdet = splines.unconstrained_linear_spline(inputs, pdf, inverse=inverse, tails=self.tails,
                                                                     tail_bound=self.tail_bound)
        return outputs, torchutils.sum_except_batch(logabsdet)

    def forward(self, inputs, context=None):
        return self._spline(inputs, inverse=False)

    def inverse(self, inputs, context=None):
        return self._spline(inputs, inverse=True)


class PiecewiseQuadraticCDF(Transform):
    """Piecewise-quadratic CDF, parameters shared by every sample (nonlinearities.py:266-319):
    K width logits and K+1 (tails=None) or K-1 (linear tails) height logits per element."""

    def __init__(self, shape, num_bins=10, tails=None, tail_bound=1.0,
                 min_bin_width=splines.quadratic.DEFAULT_MIN_BIN_WIDTH,
                 min_bin_height=splines.quadratic.DEFAULT_MIN_BIN_HEIGHT):
        super().__init__()
        self.min_bin_width = min_bin_width
        self.min_bin_height = min_bin_height
        self.tail_bound = tail_bound
        self.tails = tails
        self.unnormalized_widths = nn.Parameter(torch.randn(*shape, num_bins))
        self.unnormalized_heights = nn.Parameter(torch.randn(*shape, num_bins + 1 if tails is None else num_bins - 1))

    def _spline(self, inputs, inverse=False):
        uw = _share_across_batch(self.unnormalized_widths, inputs.shape[0])
        uh = _share_across_batch(self.unnormalized_heights, inputs.shape[0])
        if self.tails is None:
            outputs, logabsdet = splines.quadratic_spline(inputs, uw, uh, inverse=inverse,
                                                          min_bin_width=self.min_bin_width,
                                                          min_bin_height=self.min_bin_height)
        else:
            outputs, logabsdet = splines.unconstrained_quadratic_spline(
                inputs, uw, uh, inverse=inverse, tails=self.tails, tail_bound=self.tail_bound,
                min_bin_width=self.min_bin_width, min_bin_height=self.min_bin_height)
        return outputs, torchutils.sum_except_batch(logabsdet)

    def forward(self, inputs, context=None):
        return self._spline(inputs, inverse=False)

    def inverse(self, inputs, context=None):
        return self._spline(inputs, inverse=True)


class PiecewiseCubicCDF(Transform):
    """Piecewise-cubic CDF, parameters shared by every sample (nonlinearities.py:322-383)."""

    def __init__(self, shape, num_bins=10, tails=None, tail_bound=1.0,
                 min_bin_width=splines.cubic.DEFAULT_MIN_BIN_WIDTH,
                 min_bin_height=splines.cubic.DEFAULT_MIN_BIN_HEIGHT):
        super().__init__()
        self.min_bin_width = min_bin_width
        self.min_bin_height = min_bin_height
        self.tail_bound = tail_bound
        self.tails = tails
        self.unnormalized_widths = nn.Parameter(torch.randn(*shape, num_bins))
        self.unnormalized_heights = nn.Parameter(torch.randn(*shape, num_bins))
        self.unnorm_derivatives_left = nn.Parameter(torch.randn(*shape, 1))
        self.unnorm_derivatives_right = nn.Parameter(torch.randn(*shape, 1))

    def _spline(self, inputs, inverse=False):
        batch = inputs.shape[0]
        params = [_share_across_batch(p, batch) for p in (self.unnormalized_widths, self.unnormalized_heights,
                                                          self.unnorm_derivatives_left,
                                                          self.unnorm_derivatives_right)]
        if self.tails is None:
            outputs, logabsdet = splines.cubic_spline(inputs, *params, inverse=inverse,
                                                      min_bin_width=self.min_bin_width,
                                                      min_bin_height=self.min_bin_height)
        else:
            outputs, logabsdet = splines.unconstrained_cubic_spline(
                inputs, *params, inverse=inverse, tails=self.tails, tail_bound=self.tail_bound,
                min_bin_width=self.min_bin_width, min_bin_height=self.min_bin_height)
        return outputs, torchutils.sum_except_batch(logabsdet)

    def forward(self, inputs, context=None):
        return self._spline(inputs, inverse=False)

    def inverse(self, inputs, context=None):
        return self._spline(inputs, inverse=True)
