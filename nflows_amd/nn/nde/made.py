"""The density-estimator MADE (reference: nflows/nn/nde/made.py): `MADE` (:206-281) and `MixtureOfGaussiansMADE` (:284-426).

This is NOT the conditioner of the autoregressive transforms (`nflows_amd.transforms.made`): here the context enters by a
plain added `Linear` -- `temps += context_layer(context)`, no activation (made.py:196-197, :276-277) --, the initial layer is
followed by no activation in front of feed-forward blocks, and a feed-forward block ignores its context.  So the blocks
are this module's own; the masked layer is `transforms.made.MaskedLinear`, whose degrees, masks and state_dict keys are the
reference's (`weight`, `bias`, `mask`, `degrees`).  Module names are the reference's: `initial_layer`, `context_layer`,
`blocks.{i}.linear_layers.{0,1}` / `blocks.{i}.context_layer` / `blocks.{i}.batch_norm_layers.{0,1}` (residual) or
`blocks.{i}.linear` / `blocks.{i}.batch_norm` (feed-forward), `final_layer`.  The reference's module imports matplotlib
and never uses it; this one does not.

`MixtureOfGaussiansMADE.log_prob` is the MADE's forward pass on stock ops followed by ONE launch of K20 "mog"
(csrc/density.hip), which reads the final layer's [B, D * K * 3] output in place: on a HIP device, float32, contiguous,
K <= 64.  Everything else runs the reference's sequence on stock ops.

`MixtureOfGaussiansMADE.sample` is ONE launch of K30 (csrc/made_inverse.hip, the mixture element in the step loop of the
sequential samplers) on a HIP device with float32 parameters, K <= 16, residual or feed-forward blocks with ReLU, no
batch norm, no active dropout: the context rows are repeated, `torch.rand(B, D)` and THEN `torch.randn(B, D)` are drawn
on the device from the default generator (in that order, once each), the context terms are one GEMM, the kernel runs once.
Per feature t it chooses the component c as the smallest index whose running sum of exp(l_k - max l) exceeds
u[row, t] * (the sum over all k, in index order) -- K - 1 if none does -- and sets x_t = mean_c + normal[row, t] *
(softplus(ustd_c) + epsilon).  The draws differ from the host loop's for a given seed (that loop draws a Categorical and a
randn per feature); the distribution is the same.  `NFA_K30=0` or `_use_sample_kernel = False` give the host loop: the
reference's loop of D forward passes, which is also what runs on the CPU (with the reference's random stream) and
everywhere else outside the kernel's family or its size rule; its tensors are created on the context's device (the
reference creates them on the CPU).
"""
import os

import numpy as np
import torch
from torch import distributions, nn
from torch.nn import functional as F
from torch.nn import init

from ... import _cache, ops
from ...utils import torchutils


def MaskedLinear(**kwargs):
    """`transforms.made.MaskedLinear` (imported at the first use: that module imports this package's `functional`)."""
    from ...transforms.made import MaskedLinear as masked_linear
    return masked_linear(**kwargs)


def input_degrees(features):
    return torch.arange(1, features + 1)


class MaskedFeedforwardBlock(nn.Module):
    """A feedforward block based on a masked linear module (as many outputs as inputs); the context is ignored."""

    def __init__(self, in_degrees, autoregressive_features, context_features=None, random_mask=False, activation=F.relu,
                 dropout_probability=0.0, use_batch_norm=False, zero_initialization=False):
        super().__init__()
        features = len(in_degrees)
        self.batch_norm = nn.BatchNorm1d(features, eps=1e-3) if use_batch_norm else None
        self.linear = MaskedLinear(in_degrees=in_degrees, out_features=features,
                                   autoregressive_features=autoregressive_features, random_mask=random_mask, is_output=False)
        self.degrees = self.linear.degrees
        self.activation = activation
        self.dropout = nn.Dropout(p=dropout_probability)

    def forward(self, inputs, context=None):
        outputs = self.batch_norm(inputs) if self.batch_norm else inputs
        return self.dropout(self.activation(self.linear(outputs)))


class MaskedResidualBlock(nn.Module):
    """A residual block containing masked linear modules; the context is added behind the first of them."""

    def __init__(self, in_degrees, autoregressive_features, context_features=None, random_mask=False, activation=F.relu,
                 dropout_probability=0.0, use_batch_norm=False, zero_initialization=True):
        if random_mask:
            raise ValueError("Masked residual block can't be used with random masks.")
        super().__init__()
        features = len(in_degrees)
        if context_features is not None:
            self.context_layer = nn.Linear(context_features, features)
        self.use_batch_norm = use_batch_norm
        if use_batch_norm:
            self.batch_norm_layers = nn.ModuleList([nn.BatchNorm1d(features, eps=1e-3) for _ in range(2)])
        linear_0 = MaskedLinear(in_degrees=in_degrees, out_features=features,
                                autoregressive_features=autoregressive_features, random_mask=False, is_output=False)
        linear_1 = MaskedLinear(in_degrees=linear_0.degrees, out_features=features,
                                autoregressive_features=autoregressive_features, random_mask=False, is_output=False)
        self.linear_layers = nn.ModuleList([linear_0, linear_1])
        self.degrees = linear_1.degrees
        if torch.all(self.degrees >= in_degrees).item() != 1:
            raise RuntimeError("In a masked residual block, the output degrees can't be"
                               " less than the corresponding input degrees.")
        self.activation = activation
        self.dropout = nn.Dropout(p=dropout_probability)
        if zero_initialization:
            init.uniform_(self.linear_layers[-1].weight, a=-1e-3, b=1e-3)
            init.uniform_(self.linear_layers[-1].bias, a=-1e-3, b=1e-3)

    def forward(self, inputs, context=None):
        temps = inputs
        if self.use_batch_norm:
            temps = self.batch_norm_layers[0](temps)
        temps = self.activation(temps)
        temps = self.linear_layers[0](temps)
        if context is not None:
            temps = temps + self.context_layer(context)
        if self.use_batch_norm:
            temps = self.batch_norm_layers[1](temps)
        temps = self.activation(temps)
        temps = self.dropout(temps)
        temps = self.linear_layers[1](temps)
        return inputs + temps


class MADE(nn.Module):
    """Implementation of MADE.

    It can use either feedforward blocks or residual blocks (default is residual).
    Optionally, it can use batch norm or dropout within blocks (default is no)."""

    def __init__(self, features, hidden_features, context_features=None, num_blocks=2, output_multiplier=1,
                 use_residual_blocks=True, random_mask=False, activation=F.relu, dropout_probability=0.0,
                 use_batch_norm=False):
        if use_residual_blocks and random_mask:
            raise ValueError("Residual blocks can't be used with random masks.")
        super().__init__()
        self.initial_layer = MaskedLinear(in_degrees=input_degrees(features), out_features=hidden_features,
                                          autoregressive_features=features, random_mask=random_mask, is_output=False)
        if context_features is not None:
            self.context_layer = nn.Linear(context_features, hidden_features)
        block_constructor = MaskedResidualBlock if use_residual_blocks else MaskedFeedforwardBlock
        blocks = []
        prev_out_degrees = self.initial_layer.degrees
        for _ in range(num_blocks):
            blocks.append(block_constructor(in_degrees=prev_out_degrees, autoregressive_features=features,
                                            context_features=context_features, random_mask=random_mask,
                                            activation=activation, dropout_probability=dropout_probability,
                                            use_batch_norm=use_batch_norm, zero_initialization=True))
            prev_out_degrees = blocks[-1].degrees
        self.blocks = nn.ModuleList(blocks)
        self.final_layer = MaskedLinear(in_degrees=prev_out_degrees, out_features=features * output_multiplier,
                                        autoregressive_features=features, random_mask=random_mask, is_output=True)

    def forward(self, inputs, context=None):
        temps = self.initial_layer(inputs)
        if context is not None:
            temps = temps + self.context_layer(context)
        for block in self.blocks:
            temps = block(temps, context)
        return self.final_layer(temps)


class MixtureOfGaussiansMADE(MADE):
    # test and measurement switch: False = always the generic path (tools/density_time.py, tests/test_gpu_density.py)
    _use_kernel = True

    def __init__(self, features, hidden_features, context_features=None, num_blocks=2, num_mixture_components=5,
                 use_residual_blocks=True, random_mask=False, activation=F.relu, dropout_probability=0.0,
                 use_batch_norm=False, epsilon=1e-2, custom_initialization=True):
        if use_residual_blocks and random_mask:
            raise ValueError("Residual blocks can't be used with random masks.")
        super().__init__(features, hidden_features, context_features=context_features, num_blocks=num_blocks,
                         output_multiplier=3 * num_mixture_components, use_residual_blocks=use_residual_blocks,
                         random_mask=random_mask, activation=activation, dropout_probability=dropout_probability,
                         use_batch_norm=use_batch_norm)
        self.num_mixture_components = num_mixture_components
        self.features = features
        self.hidden_features = hidden_features
        self.epsilon = epsilon
        if custom_initialization:
            self._initialize()

    def forward(self, inputs, context=None):
        return super().forward(inputs, context=context)

    def _kernel_serves(self, inputs, outputs):
        return (self._use_kernel and inputs.is_cuda and inputs.dim() == 2 and inputs.numel() > 0
                and inputs.dtype == outputs.dtype == torch.float32 and inputs.is_contiguous() and outputs.is_contiguous()
                and 1 <= self.num_mixture_components <= ops.MOG_MAX_COMPONENTS)

    def log_prob(self, inputs, context=None):
        outputs = self.forward(inputs, context=context)
        if self._kernel_serves(inputs, outputs):
            return ops.mog_log_prob(inputs, outputs, self.num_mixture_components, self.epsilon)
        return mog_log_prob_generic(inputs, outputs, self.num_mixture_components, self.epsilon)

    # ---- K30: the sampler in one persistent kernel.  Its own switch, independent of K20's.
    _use_sample_kernel = os.environ.get("NFA_K30", "1") != "0"
    # Size rule (features <=, rows >) from profiles/mog_sample_time.json: the kernel does one MADE pass per sample whatever
    # the number of features, sixteen samples per workgroup; the host loop does one pass of GEMMs per FEATURE at full-device
    # rates.  At 262 144 rows the kernel is 1.7-5.1 x faster with 21-64 features but 0.68-0.70 x with 8 (1.08-1.09 x at
    # 65 536 rows); between 8 and 21 features nothing was measured there, and K23's bound of 16 is taken: such calls keep
    # the host loop they had.
    _SAMPLE_KERNEL_LOSES = ((16, 65536),)

    def _sample_kernel_net(self):
        """True where K30 serves this network: float32, residual or feed-forward blocks, ReLU, no batch norm, no active
        dropout, at most MADE_MAX_LINEARS Linears, 1 <= K <= 16.  The structure is read once per cache epoch."""
        def read():
            blocks = list(self.blocks)
            kinds = {type(b) for b in blocks}
            return (kinds <= {MaskedResidualBlock} or kinds <= {MaskedFeedforwardBlock}) and \
                len(ops._made_linears(self)) <= ops.MADE_MAX_LINEARS and \
                not any(isinstance(m, nn.BatchNorm1d) for m in self.modules()) and \
                all(p.dtype == torch.float32 for p in self.parameters()) and \
                self.final_layer.weight.shape[0] == 3 * self.num_mixture_components * self.features
        if not (1 <= self.num_mixture_components <= 16) or not _cache.keyed(self, "_sample_net_held", (_cache.epoch(),), read):
            return False
        for block in self.blocks:
            if block.activation is not F.relu or (self.training and block.dropout.p > 0.0):
                return False
        return True

    def _sample_kernel_plan(self):
        """(step blocks or None where the shape does not fit the LDS, packed context Linears) until a weight or mask changes"""
        def pack():
            linears = len(ops._made_linears(self))
            vectors = len(ops.made_context_layers(self))
            cap = ops.made_mog_block_cap(self.features, self.hidden_features, linears, vectors)
            schedule = ops.pack_mog_schedule(self, block_cap=cap) if cap > 0 else None
            return schedule, ops.pack_made_context(self) if schedule else None
        return _cache.keyed(self, "_mog_sample_cache", _cache.weights_key(self, self), pack)

    def _sample_kernel_serves(self, context):
        if not (self._use_sample_kernel and torch.is_tensor(context) and context.is_cuda and context.dim() == 2
                and context.dtype == torch.float32 and context.shape[0] > 0 and hasattr(self, "context_layer")
                and context.shape[1] == self.context_layer.weight.shape[1]
                and self.final_layer.weight.device == context.device):
            return False
        rows = context.shape[0]
        if any(self.features <= f and rows > r for f, r in self._SAMPLE_KERNEL_LOSES):
            return False
        return self._sample_kernel_net()

    def _sample_kernel(self, context, draws=None):
        """The samples [B, D] of K30 for the repeated context rows, or None where the kernel does not take the shape.
        `draws`: (uniforms, normals) in place of the generator's (tests)."""
        schedule, packed_context = self._sample_kernel_plan()
        if schedule is None:
            return None
        shape = (context.shape[0], self.features)
        if draws is None:
            uniforms = torch.rand(shape, device=context.device)      # (this order: documented above)
            normals = torch.randn(shape, device=context.device)
        else:
            uniforms, normals = draws
        terms = ops.made_mog_context_terms(context, packed_context)
        return ops.made_mog_sample(uniforms, normals, schedule, self.hidden_features, self.num_mixture_components,
                                   self.epsilon, terms)

    def sample(self, num_samples, context=None):
        if context is not None:
            context = torchutils.repeat_rows(context, num_samples)
        if self._sample_kernel_serves(context):
            with torch.no_grad():
                samples = self._sample_kernel(context)
            if samples is not None:
                return samples.reshape(-1, num_samples, self.features)
        with torch.no_grad():
            device = context.device
            samples = torch.zeros(context.shape[0], self.features, device=device)
            for feature in range(self.features):
                outputs = self.forward(samples, context)
                outputs = outputs.reshape(*samples.shape, self.num_mixture_components, 3)
                logits, means, unconstrained_stds = (outputs[:, feature, :, 0], outputs[:, feature, :, 1],
                                                     outputs[:, feature, :, 2])
                logits = torch.log_softmax(logits, dim=-1)
                stds = F.softplus(unconstrained_stds) + self.epsilon
                component_distribution = distributions.Categorical(logits=logits)
                components = component_distribution.sample((1,)).reshape(-1, 1)
                means, stds = (means.gather(1, components).reshape(-1), stds.gather(1, components).reshape(-1))
                samples[:, feature] = (means + torch.randn(context.shape[0], device=device) * stds).detach()
        return samples.reshape(-1, num_samples, self.features)

    def _initialize(self):
        # mixture coefficient logits near zero: approximately uniform coefficients
        self.final_layer.weight.data[::3, :] = self.epsilon * torch.randn(
            self.features * self.num_mixture_components, self.hidden_features)
        self.final_layer.bias.data[::3] = self.epsilon * torch.randn(self.features * self.num_mixture_components)
        # unconstrained standard deviations at the inverse of the softplus at 1: near 1 at initialization
        self.final_layer.weight.data[2::3] = self.epsilon * torch.randn(
            self.features * self.num_mixture_components, self.hidden_features)
        self.final_layer.bias.data[2::3] = torch.log(
            torch.exp(torch.Tensor([1 - self.epsilon])) - 1
        ) * torch.ones(self.features * self.num_mixture_components) + self.epsilon * torch.randn(
            self.features * self.num_mixture_components)


def mog_log_prob_generic(inputs, outputs, num_mixture_components, epsilon):
    """The reference's sequence (made.py:330-353) on stock ops."""
    outputs = outputs.reshape(*inputs.shape, num_mixture_components, 3)
    logits, means, unconstrained_stds = outputs[..., 0], outputs[..., 1], outputs[..., 2]
    log_mixture_coefficients = torch.log_softmax(logits, dim=-1)
    stds = F.softplus(unconstrained_stds) + epsilon
    return torch.sum(
        torch.logsumexp(
            log_mixture_coefficients
            - 0.5 * (np.log(2 * np.pi) + 2 * torch.log(stds) + ((inputs[..., None] - means) / stds) ** 2),
            dim=-1),
        dim=-1)
