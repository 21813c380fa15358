"""The squeeze of RealNVP / Glow: spatial blocks of factor x factor pixels become channels.

API of nflows/transforms/reshape.py: `SqueezeTransform(factor=2)`, `get_output_shape(c, h, w)`, forward
[B, C, H, W] -> [B, C f^2, H / f, W / f], inverse back, logabsdet = zeros, the reference's error messages.

Built on stock device ops -- view, permute, contiguous: exactly one copy of the tensor.  There is no kernel of this
project behind it on purpose: the map is a pure strided copy, and a copy kernel has nothing to win over the device's own.
"""
from ..utils import typechecks as check
from .base import Transform


def _require_device(inputs):
    if not inputs.is_cuda:
        raise NotImplementedError(
            "nflows_amd: inputs on %s; the MI355X path has no CPU fallback" % inputs.device)


class SqueezeTransform(Transform):
    def __init__(self, factor=2):
        super().__init__()
        if not check.is_int(factor) or factor <= 1:
            raise ValueError("Factor must be an integer > 1.")
        self.factor = factor

    def get_output_shape(self, c, h, w):
        return (c * self.factor * self.factor, h // self.factor, w // self.factor)

    def forward(self, inputs, context=None):
        if inputs.dim() != 4:
            raise ValueError("Expecting inputs with 4 dimensions")
        f = self.factor
        batch_size, c, h, w = inputs.size()
        if h % f != 0 or w % f != 0:
            raise ValueError("Input image size not compatible with the factor.")
        _require_device(inputs)
        blocks = inputs.reshape(batch_size, c, h // f, f, w // f, f)
        outputs = blocks.permute(0, 1, 3, 5, 2, 4).contiguous().view(batch_size, c * f * f, h // f, w // f)
        return outputs, inputs.new_zeros(batch_size)

    def inverse(self, inputs, context=None):
        if inputs.dim() != 4:
            raise ValueError("Expecting inputs with 4 dimensions")
        f = self.factor
        batch_size, c, h, w = inputs.size()
        if c < 4 or c % 4 != 0:   # (the reference's check, whatever the factor)
            raise ValueError("Invalid number of channel dimensions.")
        _require_device(inputs)
        blocks = inputs.reshape(batch_size, c // f ** 2, f, f, h, w)
        outputs = blocks.permute(0, 1, 4, 2, 5, 3).contiguous().view(batch_size, c // f ** 2, h * f, w * f)
        return outputs, inputs.new_zeros(batch_size)
