"""Autoregressive transforms of configs 1 and 5 on the MI355X kernels
(reference: nflows/transforms/autoregressive.py:25-128 and :404-495).

forward : one MADE pass + ONE fused kernel (elementwise map + per-sample logabsdet sum).
inverse : the reference's D-step fixed-point loop (autoregressive.py:43-52): every step re-runs
          MADE on the current outputs and the elementwise inverse over all D features; after
          step t the first t features are final.  Same semantics, same number of passes.
"""
import os

import numpy as np
import torch
from torch.nn import functional as F

from .. import _cache
from .. import _native as N
from .. import ops
from . import made as made_module
from .base import RUN_SWITCHES, RunLayer, Transform, _Run, _run_plan
from .splines import rational_quadratic
from . import splines
from ..utils import torchutils


class _LazyRows:
    """`make()[index]`, with `make` called on the first access only."""

    def __init__(self, make):
        self._make, self._value = make, None

    def __getitem__(self, index):
        if self._value is None:
            self._value = self._make()
        return self._value[index]


def _own_run_plan(layer, tile16=0):
    """The plan of a layer as a run of one (K22, K29): the run planner's own packing and tables (`base._run_plan`), kept in
    the layer's own `__dict__`, so that a layer called on its own and the same layer inside a composite are served from one
    code path."""
    run = layer.__dict__.get("_own_run")
    if run is None:
        run = layer.__dict__["_own_run"] = _Run([(layer, None)])
    return _run_plan(layer, run, False, tile16)


def _device_rows(inputs):
    """A 2-D float32 device tensor with at least one row: what every kernel of this module takes."""
    return (torch.is_tensor(inputs) and inputs.dim() == 2 and inputs.dtype == torch.float32 and inputs.is_cuda
            and inputs.shape[0] >= 1)


def _context_served(context, context_features, rows=None):
    """None for a net without a context layer, or a 2-D float32 device tensor of the net's width -- and of `rows` rows
    where the caller gives them."""
    if context is None:
        return context_features == 0
    return (context_features > 0 and torch.is_tensor(context) and context.dim() == 2 and context.dtype == torch.float32
            and context.is_cuda and context.shape[1] == context_features and (rows is None or context.shape[0] == rows))


def _relu_without_active_dropout(net):
    """The MADE's activations and dropouts are plain attributes: read on every call."""
    relu = (F.relu, torch.relu)
    return net.__dict__.get("activation") in relu and all(
        b.__dict__.get("activation") in relu and (not b.dropout.training or b.dropout.p == 0.0) for b in net.blocks)


def _has_batch_norm(net):
    return any(isinstance(m, torch.nn.BatchNorm1d) for m in net.modules())


class AutoregressiveTransform(Transform):
    def __init__(self, autoregressive_net):
        super().__init__()
        self.autoregressive_net = autoregressive_net

    def forward(self, inputs, context=None):
        params = self.autoregressive_net(inputs, context)
        return self._elementwise_forward(inputs, params)

    # Set to False to run the reference's loop verbatim (D full passes, autoregressive.py:43-52).
    columnwise_inverse = True

    def inverse(self, inputs, context=None):
        net = self.autoregressive_net
        if (self.columnwise_inverse and inputs.dim() == 2 and isinstance(net, made_module.MADE)
                and net.is_deterministic() and hasattr(self, "_inverse_column")):
            return self._inverse_columnwise(inputs, context)
        return self._inverse_reference_loop(inputs, context)

    def _inverse_reference_loop(self, inputs, context=None):
        num_inputs = int(np.prod(inputs.shape[1:]))
        outputs = torch.zeros_like(inputs)
        logabsdet = None
        for _ in range(num_inputs):
            params = self.autoregressive_net(outputs, context)
            outputs, logabsdet = self._elementwise_inverse(inputs, params)
        return outputs, logabsdet

    def _inverse_columnwise(self, inputs, context=None):
        """Same result as the reference loop with O(D) instead of O(D^2) work in the output layer
        and the elementwise transform.

        In the reference loop, iteration t+1 recomputes ALL D*P conditioner outputs and ALL D
        elementwise inverses, although (by the autoregressive masks) only feature t changes: its
        parameters depend on features < t, which became final in earlier iterations, and the
        features it has not reached yet are multiplied by exactly-zero masked weights.  Here step
        t evaluates the hidden layers on the current outputs (unreached features still zero),
        takes only feature t's P rows of the final masked layer, inverts that one column and adds
        its log-derivative.  Identical up to summation order."""
        net = self.autoregressive_net
        batch, features = inputs.shape
        mult = self._output_dim_multiplier()
        final = net.final_layer
        bias = final.bias.view(features, mult)
        if torch.is_grad_enabled():
            weight = (final.weight * final.mask).view(features, mult, -1)
        else:   # (formed on first use: the kernels below pack their own copy of the output layer)
            weight = _LazyRows(lambda: final.masked_weight().view(features, mult, -1))
        outputs = torch.zeros_like(inputs)
        logabsdet = inputs.new_zeros(batch)
        if torch.is_grad_enabled():
            # differentiable form (training an inverse autoregressive flow, reparameterised
            # sampling): the tensor handed to the conditioner is saved by its first layer for the
            # weight gradient, so it is never written again -- every step writes its column into a
            # fresh copy, like the reference's out-of-place loop (autoregressive.py:43-52)
            for t in range(features):
                h = net.hidden(outputs, context)
                params_t = torch.addmm(bias[t], h, weight[t].t())
                column, lad_t = self._inverse_column(inputs[:, t], params_t)
                outputs = outputs.clone()
                outputs[:, t] = column
                logabsdet = logabsdet + lad_t
            return outputs, logabsdet
        # No-grad (sampling): `weight * mask` of every layer is formed once, and the first layer's
        # output -- bias + sum over the features found so far of column (x) masked weight column --
        # is carried along and grows by one rank-1 term per step (all still-zero features contribute
        # exact zeros to the reference's full product).
        #
        # The sequential part ends early: a hidden unit of degree d reads features < d only, so once
        # feature `last` = (largest hidden degree) - 1 is found every hidden activation is final, and
        # the remaining features -- each a function of that one hidden vector and its own P output
        # rows -- are inverted together: one GEMM for their parameters, one elementwise launch.
        # (MADE with H < D - 1 sequential degrees: D = 784, H = 256 leaves 256 sequential steps.)
        first = net.initial_layer
        sequential = min(features, self._sequential_steps())
        with net.frozen_masks():
            # the sequential features in one persistent kernel where there is one (K12), else step by step
            fast = self._sequential_kernel(inputs, context, sequential)
            if fast is not None:
                outputs, logabsdet, h = fast
            else:
                first_weight = first.masked_weight().t().contiguous()  # [D, H]: row t = feature t's weights
                pre = first.bias.detach().expand(batch, -1).contiguous() if first.bias is not None \
                    else inputs.new_zeros(batch, first_weight.shape[1])
                for t in range(sequential):
                    h = net.hidden_from_initial(pre, context)
                    params_t = torch.addmm(bias[t], h, weight[t].t())
                    column, lad_t = self._inverse_column(inputs[:, t], params_t)
                    outputs[:, t] = column
                    logabsdet += lad_t
                    if t + 1 < features:
                        pre.addr_(column, first_weight[t])
                if sequential < features:
                    h = net.hidden_from_initial(pre, context)
            if sequential < features:
                tail = self._output_layer_kernel(inputs, h, sequential, inverse=True, out=outputs) \
                    if hasattr(self, "_output_layer_kernel") and outputs.is_contiguous() else None
                if tail is not None:   # (K13: the remaining features' rows of the output layer inside the spline kernel)
                    logabsdet += tail[1]
                else:
                    rest = features - sequential
                    params = torch.addmm(bias[sequential:].reshape(-1), h, weight[sequential:].reshape(rest * mult, -1).t())
                    columns, lad_rest = self._elementwise_inverse(inputs[:, sequential:].contiguous(),
                                                                  params.view(batch, rest, mult))
                    outputs[:, sequential:] = columns
                    logabsdet += lad_rest
        return outputs, logabsdet

    def _sequential_kernel(self, inputs, context, sequential):
        """Hook: (outputs with the first `sequential` columns found, their logabsdet, the final hidden
        vector) from a kernel that runs all sequential steps itself, or None."""
        return None

    def _sequential_steps(self):
        """Number of leading features whose inversion changes a hidden activation of the MADE: the
        largest degree of any hidden unit (made.py: a unit of degree d is connected to inputs of
        degree <= d, i.e. features 0 .. d - 1)."""
        # (one device read per cache epoch: `degrees` / `mask` are registered buffers, a load_state_dict from a
        #  checkpoint with other random masks replaces them and advances the epoch)
        def read():
            net = self.autoregressive_net
            degrees = [net.initial_layer.degrees] + [b.degrees for b in net.blocks]
            return int(max(int(d.max()) for d in degrees))
        return _cache.keyed(self, "_sequential_steps_cache", (_cache.epoch(),), read)

    def _output_dim_multiplier(self):
        raise NotImplementedError()

    def _elementwise_forward(self, inputs, autoregressive_params):
        raise NotImplementedError()

    def _elementwise_inverse(self, inputs, autoregressive_params):
        raise NotImplementedError()


class _MadeKernelLayer(AutoregressiveTransform, RunLayer):
    """What MaskedAffineAutoregressiveTransform and MaskedPiecewiseRationalQuadraticAutoregressiveTransform share: the
    kernels that run the layer's MADE themselves and their gates.  The density pass of a run of such layers is one launch
    (K22 / K29: the run protocol of transforms/base.py, `RunLayer`; a layer called on its own is a run of one), the steps
    of the inverse are one persistent kernel (K23 / K28).  Where the two layers' gates differ the subclass says so, in a
    class attribute or an override beside its kernel."""

    unconditional_transform = None
    _forward_only_run = True
    _KIND = None                     # the family of the density kernel
    _HOOKS = ()                      # the functions the density kernel stands for
    _FLOAT32_WEIGHTS_ONLY = False    # the structural reads ask for a MADE in float32
    _COLUMNS_RECOUNTED = False       # `_all_columns` compares the held table's length with `features` on every call

    def _overridden(self, hooks, library):
        """True when a subclass (or an assignment to the class or the instance) replaced one of `hooks`, the functions a
        kernel of the class `library` stands for: such a layer runs the host's sequence with the user's function."""
        cls = type(self)
        return any(h in self.__dict__ or getattr(cls, h) is not getattr(library, h) for h in hooks)

    def _conditioner(self):
        return self._modules["autoregressive_net"]

    def _context_features(self):
        net = self._conditioner()
        return net.context_layer.weight.shape[1] if hasattr(net, "context_layer") else 0

    def _conditioner_shape(self):
        """What `_served_shape` makes of a MADE the density kernel runs inside the layer kernel -- plain MADE, hidden width
        <= 128, at most 64 context features, no batch norm --, or None.  Read once per cache epoch; the activations and the
        dropouts are plain attributes and are read on every call."""
        net = self._conditioner()

        def read():
            if type(net) is made_module.MADE and (not self._FLOAT32_WEIGHTS_ONLY
                                                  or net.initial_layer.weight.dtype == torch.float32):
                hidden, features = net.initial_layer.weight.shape
                if hidden <= 128 and self._context_features() <= 64 and not _has_batch_norm(net):
                    residual = bool(net.use_residual_blocks)
                    return self._served_shape(len(net.blocks) * (2 if residual else 1), residual, features,
                                              net.final_layer.weight.shape[0])
            return None
        shape = _cache.keyed(self, "_conditioner_shape_held", (_cache.epoch(), net), read)
        return shape if shape is not None and _relu_without_active_dropout(net) else None

    def _density_kernel_on(self):
        return self.fuse_conditioner

    def _run_kind(self, context):
        if not self._density_kernel_on() or torch.is_grad_enabled() or self._conditioner_shape() is None:
            return None
        return self._KIND if _context_served(context, self._context_features()) else None

    def _run_signature(self):
        return (self._KIND, self.features, self._conditioner_shape(), self._context_features()) + self._run_variant()

    def _fused_geometry(self, others=()):
        """(padded features, transformed features, identity features, pad value): the row length in multiples of four,
        the pad columns pass through; every feature is both read by the conditioner and transformed."""
        features = self.features
        return (features + 3) // 4 * 4, features, features, 0.0

    def _all_columns(self):
        dev = self._conditioner().initial_layer.weight.device
        held = self.__dict__.get("_columns_held")
        if held is None or held.device != dev or (self._COLUMNS_RECOUNTED and held.numel() != self.features):
            held = self.__dict__["_columns_held"] = torch.arange(self.features, device=dev)
        return held

    transform_features = property(_all_columns)   # (what the planner writes into the two halves of the layer's table)
    identity_features = property(_all_columns)

    def forward(self, inputs, context=None):
        if (_device_rows(inputs) and not self._user_hooks and self._run_kind(context) is not None
                and inputs.shape[1] == self.features and self._own_call_served(inputs, context)):
            fused = self._whole_layer(inputs, context)   # a run of one
            if fused is not None:
                return fused
        return self._forward_layer_by_layer(inputs, context)

    def _own_call_served(self, inputs, context):
        """What the layer's own `forward` asks of a call beyond the planner's questions."""
        return True

    def _whole_layer(self, inputs, context):
        return self._launch_run(lambda tile16=0: _own_run_plan(self, tile16), 1, self._fused_geometry(), inputs, context,
                                False, None, False)

    def _forward_layer_by_layer(self, inputs, context=None):
        return AutoregressiveTransform.forward(self, inputs, context)

    # ---- the persistent kernels of the inverse (K23, K28: csrc/made_inverse.hip)
    def _step_kernel_net(self, slot, served=lambda net: True):
        """The MADE when a persistent inverse kernel can run it -- plain MADE, ReLU, no batch norm, no active dropout, at most
        12 Linears, and what `served(net)` adds --, else None.  The structure is read once per cache epoch (kept in `slot`);
        activations and dropouts are plain attributes, read per call."""
        net = self._conditioner()
        if not _cache.keyed(self, slot, (_cache.epoch(), net), lambda: (
                type(net) is made_module.MADE and len(ops._made_linears(net)) <= ops.MADE_MAX_LINEARS
                and (not self._FLOAT32_WEIGHTS_ONLY or net.initial_layer.weight.dtype == torch.float32)
                and not _has_batch_norm(net) and served(net))):
            return None
        return net if _relu_without_active_dropout(net) else None

    def _step_kernel_plan(self, slot, key, net, steps, multiplier):
        """(step blocks of `ops.pack_made_schedule` or None where the shape does not fit the LDS, packed context Linears or
        None), kept in `slot` under `key` -- made of `_cache.weights_key`: until a parameter, a mask or a write through
        `.data` changes."""
        def pack():
            hidden = net.initial_layer.weight.shape[0]
            linears = len(ops._made_linears(net))
            vectors = len(ops.made_context_layers(net))
            cap = ops.made_block_cap(steps, hidden, linears, vectors)
            schedule = ops.pack_made_schedule(net, steps, multiplier, block_cap=cap, context=True) if cap > 0 else None
            return schedule, ops.pack_made_context(net) if schedule else None
        return _cache.keyed(self, slot, key, pack)


class MaskedAffineAutoregressiveTransform(_MadeKernelLayer):
    """MAF layer: y_d = softplus(u_d)+1e-3) * x_d + shift_d with (u, shift) = MADE(x)
    (autoregressive.py:64-128); parameters interleaved [B, D, 2]."""

    def __init__(self, features, hidden_features, context_features=None, num_blocks=2,
                 use_residual_blocks=True, random_mask=False, activation=F.relu,
                 dropout_probability=0.0, use_batch_norm=False):
        self.features = features
        net = made_module.MADE(features=features, hidden_features=hidden_features,
                               context_features=context_features, num_blocks=num_blocks,
                               output_multiplier=self._output_dim_multiplier(),
                               use_residual_blocks=use_residual_blocks, random_mask=random_mask,
                               activation=activation, dropout_probability=dropout_probability,
                               use_batch_norm=use_batch_norm)
        self._epsilon = 1e-3
        super().__init__(net)

    def _output_dim_multiplier(self):
        return 2

    def _elementwise_forward(self, inputs, autoregressive_params):
        return ops.affine_autoregressive(inputs, autoregressive_params, inverse=False)

    # ---- whole-layer kernel K22 (csrc/affine_made.hip): the MADE inside the layer kernel, runs of such layers in one
    #      launch.  The density pass only -- the inverse is sequential in the features and keeps its column-wise loop.
    fuse_conditioner = os.environ.get("NFA_K22", "1") != "0"   # class-level switch for A/B measurements
    _KIND = "k22"
    _HOOKS = ("forward", "_elementwise_forward", "_elementwise_inverse", "_output_dim_multiplier")
    _user_hooks = property(lambda self: self._overridden(self._HOOKS, MaskedAffineAutoregressiveTransform))

    def _served_shape(self, hidden_linears, residual, features, rows):
        """(hidden Linears, residual blocks?) of a MADE of the layer's width, at most 64 features, two rows per feature"""
        return (hidden_linears, residual) if features == self.features <= 64 and rows == 2 * features else None

    def _run_packed(self, geometry=None):
        net = self._conditioner()
        key = _cache.weights_key(self, net)   # (parameters and buffers: the masks are part of the key)
        return _cache.keyed(self, "_packed_made_cache", key, lambda: ops.pack_made_conditioner(net))

    def _launch_run(self, plan, num_layers, geometry, inputs, context, inverse, accumulate_into, standard_normal_log_prob):
        weights, biases, tables = plan()[:3]
        hidden_linears, residual_blocks = self._conditioner_shape()
        return ops.affine_flow_made(inputs, weights, biases, tables, self.features, hidden_linears, context, accumulate_into,
                                    num_layers=num_layers, standard_normal_log_prob=standard_normal_log_prob,
                                    pad=(geometry[0], geometry[3]), residual_blocks=residual_blocks)

    def _elementwise_inverse(self, inputs, autoregressive_params):
        return ops.affine_autoregressive(inputs, autoregressive_params, inverse=True)

    def _inverse_column(self, column, params):
        """One feature: params [B, 2] = (scale logit, shift); K2b with a single feature."""
        out, lad = ops.affine_autoregressive(column.reshape(-1, 1), params, inverse=True)
        return out.reshape(-1), lad

    # ---- persistent kernel K23 (csrc/made_inverse.hip): the whole inverse of the layer -- every feature, the context
    #      included -- in one launch: K12's step loop with the affine element.  Its own switch, independent of K22's.
    fuse_sequential_inverse = os.environ.get("NFA_K23", "1") != "0"
    _INVERSE_HOOKS = ("inverse", "_elementwise_inverse", "_inverse_column", "_output_dim_multiplier")
    # Size rule from profiles/maf_sample_time.json: the kernel does one MADE pass per sample whatever the number of
    # features, sixteen samples per workgroup; the host loop does one pass of GEMMs per FEATURE at full-device rates.  At
    # 262 144 rows the loop is 2.1 x faster with 8 features and 1.15 x with 16, and 1.6-3.1 x slower with 21-64; at
    # 16 384 rows the kernel is 1.7 x faster or better for every shape.
    _INVERSE_KERNEL_ROW_LIMIT = (16, 65536)   # (features <=, rows >): such a call takes the host loop

    def _inverse_kernel_serves_rows(self, rows):
        few, many = self._INVERSE_KERNEL_ROW_LIMIT
        return not (self.features <= few and rows > many)

    def _inverse_kernel_net(self):
        """The MADE when K23 can run it (`_step_kernel_net`): of the layer's width, at least two features, two rows each"""
        return self._step_kernel_net("_inverse_net_held", lambda net: (
            self.features >= 2 and net.initial_layer.weight.shape[1] == self.features
            and net.final_layer.weight.shape[0] == 2 * self.features))

    def _inverse_kernel_plan(self, net):
        return self._step_kernel_plan("_made_affine_cache", _cache.weights_key(self, net), net, self.features, 2)

    def inverse(self, inputs, context=None):
        if (self.fuse_sequential_inverse and not torch.is_grad_enabled() and _device_rows(inputs)
                and inputs.shape[1] == self.features and self._inverse_kernel_serves_rows(inputs.shape[0])
                and not self._overridden(self._INVERSE_HOOKS, MaskedAffineAutoregressiveTransform)):
            net = self._inverse_kernel_net()
            if net is not None and _context_served(context, self._context_features(), inputs.shape[0]):
                schedule, packed_context = self._inverse_kernel_plan(net)
                if schedule is not None:
                    terms = ops.made_context_terms(context, packed_context) if context is not None else None
                    fused = ops.made_affine_inverse(inputs, schedule, net.initial_layer.weight.shape[0], terms)
                    if fused is not None:
                        return fused
        return super().inverse(inputs, context)


RUN_SWITCHES.append((MaskedAffineAutoregressiveTransform, ("fuse_conditioner",)))


class MaskedPiecewiseRationalQuadraticAutoregressiveTransform(_MadeKernelLayer):
    """Autoregressive neural spline layer (autoregressive.py:404-495): per feature 3K-1 / 3K+1
    logits from MADE, the RQ functional elementwise, logabsdet summed per sample.  Runs as the
    fused coupling kernel with every feature transformed (d_t = D)."""

    def __init__(self, features, hidden_features, context_features=None, num_bins=10, tails=None,
                 tail_bound=1.0, num_blocks=2, use_residual_blocks=True, random_mask=False,
                 activation=F.relu, dropout_probability=0.0, use_batch_norm=False,
                 min_bin_width=rational_quadratic.DEFAULT_MIN_BIN_WIDTH,
                 min_bin_height=rational_quadratic.DEFAULT_MIN_BIN_HEIGHT,
                 min_derivative=rational_quadratic.DEFAULT_MIN_DERIVATIVE):
        self.num_bins = num_bins
        self.min_bin_width = min_bin_width
        self.min_bin_height = min_bin_height
        self.min_derivative = min_derivative
        self.tails = tails
        self.tail_bound = tail_bound
        net = made_module.MADE(features=features, hidden_features=hidden_features,
                               context_features=context_features, num_blocks=num_blocks,
                               output_multiplier=self._output_dim_multiplier(),
                               use_residual_blocks=use_residual_blocks, random_mask=random_mask,
                               activation=activation, dropout_probability=dropout_probability,
                               use_batch_norm=use_batch_norm)
        super().__init__(net)
        self._all_features = None

    def _output_dim_multiplier(self):
        if self.tails == "linear":
            return self.num_bins * 3 - 1
        if self.tails is None:
            return self.num_bins * 3 + 1
        raise ValueError

    def _wh_divisor(self):
        net = self.autoregressive_net
        return float(np.sqrt(net.hidden_features)) if hasattr(net, "hidden_features") else 0.0

    def _rqs_spec(self):
        """The spline's constants as every kernel of the layer takes them."""
        return ops.make_rqs_spec(self.num_bins, self.tails, tail_bound=self.tail_bound,
                                 min_bin_width=self.min_bin_width, min_bin_height=self.min_bin_height,
                                 min_derivative=self.min_derivative, wh_divisor=self._wh_divisor())

    _density_spec = _rqs_spec

    def _elementwise(self, inputs, autoregressive_params, inverse=False):
        N.require_device_f32("inputs", inputs, 2)
        batch, features = inputs.shape
        if self.tails not in (None, "linear"):
            raise ValueError
        cache = self._all_features if isinstance(self._all_features, dict) else {}
        cols = cache.get((features, inputs.device))
        if cols is None:
            cols = torch.arange(features, device=inputs.device)
            cache[(features, inputs.device)] = cols
            self._all_features = cache
        params = autoregressive_params.reshape(batch, features * self._output_dim_multiplier())
        return ops.rqs_coupling(inputs, params, cols, self._rqs_spec(), inverse=inverse)

    def _elementwise_forward(self, inputs, autoregressive_params):
        return self._elementwise(inputs, autoregressive_params)

    def _elementwise_inverse(self, inputs, autoregressive_params):
        return self._elementwise(inputs, autoregressive_params, inverse=True)

    # the MADE's output layer inside the spline kernel (K13, csrc/made_output.hip): the forward pass and the
    # last pass of the inverse never form the [batch, features * multiplier] parameter tensor
    fuse_output_layer = os.environ.get("NFA_K13", "1") != "0"

    def _output_layer_kernel(self, inputs, hidden, first_feature, inverse, out=None):
        """(outputs with the columns from `first_feature` on written, their logabsdet) from K13, or None."""
        net = self.autoregressive_net
        if not (self.fuse_output_layer and isinstance(net, made_module.MADE) and self.tails == "linear"
                and self.num_bins == 8 and inputs.dim() == 2 and inputs.is_cuda and inputs.dtype == torch.float32
                and not torch.is_grad_enabled() and hidden.shape[1] <= 256 and hidden.shape[1] % 4 == 0
                and inputs.shape[0] >= 1):
            return None
        final = net.final_layer
        key = (_cache.epoch(), first_feature) + tuple((t.data_ptr(), t._version) for t in (final.weight, final.bias, final.mask))
        # (one slot per first feature: 0 for the density pass, the number of sequential steps for the inverse's tail)
        packed = _cache.keyed(self, "_made_output_cache_%d" % first_feature, key,
                              lambda: ops.pack_made_output(net, self._output_dim_multiplier(), first_feature))
        return ops.made_output_spline(inputs, hidden, packed, self._rqs_spec(), first_column=first_feature, inverse=inverse,
                                      out=out)

    # ---- whole-layer kernel K29 (csrc/made_rqs.hip): the MADE and the spline inside one layer kernel, runs of such
    #      layers -- their permutations and the base density included -- in one launch.  The density pass only: the inverse
    #      keeps K12 / K28, K13's tail and the host loop.
    #      The switch (NFA_K29): "0" off; "2" serves 8 bins as well; anything else, unset and empty included, is the default 1:
    #      every bin count from 2 to 16 except 8, whose calls keep hidden GEMMs + K13 (existing tests pin that path; the 8-bin
    #      columns of profiles/ar_spline_density_time.json are recorded for a later change of that default).
    #      No size rule: in all 96 measured cases of that file (log_prob and _transform, 8 and 10 bins, with and without a
    #      context, 1 024 / 16 384 / 262 144 rows, 5-16 layers on 8-64 features) the one launch is 1.5-4.7 x faster per call
    #      than the layer-by-layer path, none slower.
    fuse_conditioner = {"0": 0, "2": 2}.get(os.environ.get("NFA_K29", "1").strip(), 1)
    _KIND = "k29"
    _HOOKS = ("forward", "_elementwise", "_elementwise_forward", "_output_dim_multiplier")
    _user_hooks = property(lambda self: self._overridden(self._HOOKS, MaskedPiecewiseRationalQuadraticAutoregressiveTransform))
    _FLOAT32_WEIGHTS_ONLY = True
    _COLUMNS_RECOUNTED = True    # (`features` is read off the net)

    @property
    def features(self):
        """Width of the rows the layer takes (the planner compares it with the input's)."""
        return self._conditioner().initial_layer.weight.shape[1]

    def _served_shape(self, hidden_linears, residual, features, rows):
        return (hidden_linears, residual, rows // features) if 1 <= features <= 64 else None

    def _conditioner_shape(self):
        """(hidden Linears, residual blocks?) of a MADE that K29 runs inside the layer kernel: in float32, at most 64
        features, 3 K - 1 rows per feature (read per call, as the tails are)."""
        shape = super()._conditioner_shape()
        if shape is None or self.tails != "linear" or shape[2] != 3 * self.num_bins - 1:
            return None
        return shape[:2]

    def _density_kernel_on(self):
        mode = self.fuse_conditioner
        return bool(mode) and 2 <= self.num_bins <= 16 and (self.num_bins != 8 or int(mode) >= 2)

    def _spline_constants(self):
        return (self.num_bins, float(self.tail_bound), float(self.min_bin_width), float(self.min_bin_height),
                float(self.min_derivative), self._wh_divisor())

    def _run_variant(self, geometry=None, tile16=0):
        # (K29's blobs depend on the bin count and on the divisor folded into them: part of the plan's key and the signature)
        return (self._spline_constants(),)

    def _run_packed(self, geometry=None):
        net = self._conditioner()
        # (parameters and buffers: the masks are part of the key; the divisor is an attribute of the net)
        key = (_cache.weights_key(self, net), self.num_bins, self._wh_divisor())
        return _cache.keyed(self, "_packed_made_rqs_cache", key, lambda: ops.pack_made_rqs_conditioner(net, self.num_bins))

    def _launch_run(self, plan, num_layers, geometry, inputs, context, inverse, accumulate_into, standard_normal_log_prob):
        weights, biases, tables = plan()[:3]
        hidden_linears, residual_blocks = self._conditioner_shape()
        return ops.rqs_flow_made(inputs, weights, biases, tables, self.features, hidden_linears, self._rqs_spec(), context,
                                 accumulate_into, num_layers=num_layers, standard_normal_log_prob=standard_normal_log_prob,
                                 pad=(geometry[0], geometry[3]), residual_blocks=residual_blocks)

    def _own_call_served(self, inputs, context):
        return context is None or context.shape[0] == inputs.shape[0]

    def _forward_layer_by_layer(self, inputs, context=None):
        net = self.autoregressive_net
        if (self.fuse_output_layer and isinstance(net, made_module.MADE) and inputs.dim() == 2 and inputs.is_cuda
                and inputs.dtype == torch.float32 and not torch.is_grad_enabled() and self.tails == "linear"
                and self.num_bins == 8):
            hidden = net.hidden(inputs, context)
            fused = self._output_layer_kernel(inputs, hidden, 0, inverse=False)
            if fused is not None:
                return fused
            return self._elementwise_forward(inputs, net.final_layer(hidden))
        return AutoregressiveTransform.forward(self, inputs, context)

    # persistent kernel for the sequential features of the inverse (K12, csrc/made_inverse.hip)
    fuse_sequential_inverse = os.environ.get("NFA_K12", "1") != "0"

    def _sequential_kernel(self, inputs, context, sequential):
        if not self.fuse_sequential_inverse or sequential < 1:
            return None
        fast = self._sequential_kernel_k12(inputs, context, sequential)
        if fast is None:   # K12's gate refused, or its entry point answered unsupported (one step block does not fit twice)
            fast = self._sequential_kernel_ctx(inputs, context, sequential)
        return fast

    def _sequential_kernel_k12(self, inputs, context, sequential):
        net = self.autoregressive_net
        if not (self.fuse_sequential_inverse and context is None and sequential >= 1
                and isinstance(net, made_module.MADE) and net.activation is F.relu
                and not hasattr(net, "context_layer") and self.tails == "linear" and self.num_bins in (8, 10)
                and not any(isinstance(m, torch.nn.BatchNorm1d) for m in net.modules())):
            return None
        key = (_cache.epoch(), sequential) + tuple((p.data_ptr(), p._version) for p in net.parameters())
        schedule = _cache.keyed(self, "_made_schedule_cache", key,
                                lambda: ops.pack_made_schedule(net, sequential, self._output_dim_multiplier()))
        hidden_features = net.initial_layer.weight.shape[0]
        return ops.made_rqs_inverse(inputs, schedule, hidden_features, sequential, self._rqs_spec())

    # ---- persistent kernel K28 (csrc/made_inverse.hip): the RQ element in K23's loop -- a context, 2 .. 16 bins, steps cut
    #      into continuation blocks -- for what K12 does not serve.  `fuse_sequential_inverse` (NFA_K12) switches both
    #      kernels, this one K28 alone.
    fuse_sequential_inverse_ctx = os.environ.get("NFA_K28", "1") != "0"
    _SEQUENTIAL_HOOKS = ("inverse", "_elementwise_inverse", "_inverse_column", "_output_dim_multiplier", "_elementwise")
    # Size rule from profiles/ar_spline_sample_time.json (hidden 128, two blocks): the kernel does one MADE pass per sample
    # whatever the number of features, sixteen samples per workgroup; the host loop one pass of GEMMs per FEATURE at
    # full-device rates.  At 65 536 rows the loop is 2.4 x faster with 6 features and 1.6 x with 8 (3.0 x and 1.8 x at
    # 262 144), with 16 features the kernel is 1.10 x faster at 65 536 rows and 0.97 x at 262 144, with 21-64 features 1.2-2.6 x
    # faster at both; at 16 384 rows the kernel is 1.5 x faster or better for every shape.  Between 16 384 and 65 536 rows, and
    # between 8 and 16 features, nothing was measured: such calls keep the loop, which is what they had.
    _SEQUENTIAL_CTX_ROW_LIMIT = (16, 16384)   # (features <=, rows >): such a call takes the host loop; None: no size rule

    def _sequential_ctx_serves_rows(self, features, rows):
        limit = self._SEQUENTIAL_CTX_ROW_LIMIT
        return limit is None or not (features <= limit[0] and rows > limit[1])

    def _sequential_ctx_net(self):
        """The MADE when K28 can run it (`_step_kernel_net`: in float32), else None."""
        return self._step_kernel_net("_sequential_ctx_net_held")

    def _sequential_ctx_plan(self, net, sequential):
        return self._step_kernel_plan("_made_schedule_ctx_cache", (_cache.weights_key(self, net), sequential), net,
                                      sequential, self._output_dim_multiplier())

    def _sequential_kernel_ctx(self, inputs, context, sequential):
        if not (self.fuse_sequential_inverse_ctx and self.tails == "linear" and 2 <= self.num_bins <= 16
                and _device_rows(inputs) and self._sequential_ctx_serves_rows(inputs.shape[1], inputs.shape[0])
                and not self._overridden(self._SEQUENTIAL_HOOKS, MaskedPiecewiseRationalQuadraticAutoregressiveTransform)):
            return None
        net = self._sequential_ctx_net()
        if (net is None or net.initial_layer.weight.shape[1] != inputs.shape[1]
                or not _context_served(context, self._context_features(), inputs.shape[0])):
            return None
        schedule, packed_context = self._sequential_ctx_plan(net, sequential)
        if schedule is None:
            return None
        terms = ops.made_context_terms(context, packed_context) if context is not None else None
        return ops.made_rqs_inverse_ctx(inputs, schedule, net.initial_layer.weight.shape[0], sequential, self._rqs_spec(), terms)

    def _inverse_column(self, column, params):
        """One feature: params [B, P]; the spline layer kernel with a single (transformed) feature."""
        out, lad = self._elementwise(column.reshape(-1, 1), params, inverse=True)
        return out.reshape(-1), lad


RUN_SWITCHES.append((MaskedPiecewiseRationalQuadraticAutoregressiveTransform, ("fuse_conditioner",)))


class _SiblingSplineAutoregressiveTransform(AutoregressiveTransform):
    """Shared part of the linear / quadratic / cubic autoregressive spline layers
    (autoregressive.py:196-401): MADE emits `_output_dim_multiplier()` logits per feature, the
    spline functional (K9) runs elementwise, logabsdet is summed per sample."""

    def _make_net(self, features, hidden_features, context_features, num_blocks, use_residual_blocks,
                  random_mask, activation, dropout_probability, use_batch_norm):
        return made_module.MADE(features=features, hidden_features=hidden_features,
                                context_features=context_features, num_blocks=num_blocks,
                                output_multiplier=self._output_dim_multiplier(),
                                use_residual_blocks=use_residual_blocks, random_mask=random_mask,
                                activation=activation, dropout_probability=dropout_probability,
                                use_batch_norm=use_batch_norm)

    def _wh_divisor(self):
        net = self.autoregressive_net
        return float(np.sqrt(net.hidden_features)) if hasattr(net, "hidden_features") else 0.0

    def _functional(self, inputs, params, inverse):
        """inputs [...], params [..., multiplier] -> (outputs, logabsdet) elementwise"""
        raise NotImplementedError()

    def _elementwise(self, inputs, autoregressive_params, inverse=False):
        # (inputs may be a subset of the features: the independent tail of the column-wise inverse)
        params = autoregressive_params.reshape(inputs.shape[0], inputs.shape[1], self._output_dim_multiplier())
        outputs, logabsdet = self._functional(inputs, params, inverse)
        return outputs, torchutils.sum_except_batch(logabsdet)

    def _elementwise_forward(self, inputs, autoregressive_params):
        return self._elementwise(inputs, autoregressive_params)

    def _elementwise_inverse(self, inputs, autoregressive_params):
        return self._elementwise(inputs, autoregressive_params, inverse=True)

    def _inverse_column(self, column, params):
        return self._functional(column, params, True)


class MaskedPiecewiseLinearAutoregressiveTransform(_SiblingSplineAutoregressiveTransform):
    """autoregressive.py:196-246: piecewise-linear CDF on [0, 1] per feature."""

    def __init__(self, num_bins, features, hidden_features, context_features=None, num_blocks=2,
                 use_residual_blocks=True, random_mask=False, activation=F.relu, dropout_probability=0.0,
                 use_batch_norm=False):
        self.num_bins = num_bins
        self.features = features
        super().__init__(self._make_net(features, hidden_features, context_features, num_blocks,
                                        use_residual_blocks, random_mask, activation, dropout_probability,
                                        use_batch_norm))

    def _output_dim_multiplier(self):
        return self.num_bins

    def _functional(self, inputs, params, inverse):
        return splines.linear_spline(inputs, params, inverse=inverse)


class MaskedPiecewiseQuadraticAutoregressiveTransform(_SiblingSplineAutoregressiveTransform):
    """autoregressive.py:249-334.  Only the width logits are divided by sqrt(hidden_features) when
    the net exposes it (:304-306; the height scaling is commented out in the reference)."""

    def __init__(self, features, hidden_features, context_features=None, num_bins=10, num_blocks=2,
                 tails=None, tail_bound=1.0, use_residual_blocks=True, random_mask=False, activation=F.relu,
                 dropout_probability=0.0, use_batch_norm=False,
                 min_bin_width=rational_quadratic.DEFAULT_MIN_BIN_WIDTH,
                 min_bin_height=rational_quadratic.DEFAULT_MIN_BIN_HEIGHT,
                 min_derivative=rational_quadratic.DEFAULT_MIN_DERIVATIVE):
        self.num_bins = num_bins
        self.min_bin_width = min_bin_width
        self.min_bin_height = min_bin_height
        self.min_derivative = min_derivative
        self.tails = tails
        self.tail_bound = tail_bound
        self.features = features
        super().__init__(self._make_net(features, hidden_features, context_features, num_blocks,
                                        use_residual_blocks, random_mask, activation, dropout_probability,
                                        use_batch_norm))

    def _output_dim_multiplier(self):
        return self.num_bins * 2 - 1 if self.tails == "linear" else self.num_bins * 2 + 1

    def _functional(self, inputs, params, inverse):
        K = self.num_bins
        uw, uh = params[..., :K], params[..., K:]
        if self._wh_divisor():
            uw = uw / self._wh_divisor()
        kw = dict(inverse=inverse, min_bin_width=self.min_bin_width, min_bin_height=self.min_bin_height)
        if self.tails is None:
            return splines.quadratic_spline(inputs, uw, uh, **kw)
        if self.tails == "linear":
            return splines.unconstrained_quadratic_spline(inputs, uw, uh, tails=self.tails,
                                                          tail_bound=self.tail_bound, **kw)
        raise ValueError


class MaskedPiecewiseCubicAutoregressiveTransform(_SiblingSplineAutoregressiveTransform):
    """autoregressive.py:337-401: cubic spline on [0, 1] per feature."""

    def __init__(self, num_bins, features, hidden_features, context_features=None, num_blocks=2,
                 use_residual_blocks=True, random_mask=False, activation=F.relu, dropout_probability=0.0,
                 use_batch_norm=False):
        self.num_bins = num_bins
        self.features = features
        super().__init__(self._make_net(features, hidden_features, context_features, num_blocks,
                                        use_residual_blocks, random_mask, activation, dropout_probability,
                                        use_batch_norm))

    def _output_dim_multiplier(self):
        return self.num_bins * 2 + 2

    def _functional(self, inputs, params, inverse):
        K = self.num_bins
        uw, uh = params[..., :K], params[..., K:2 * K]
        if self._wh_divisor():
            uw, uh = uw / self._wh_divisor(), uh / self._wh_divisor()
        return splines.cubic_spline(inputs, uw, uh, params[..., 2 * K:2 * K + 1], params[..., 2 * K + 1:2 * K + 2],
                                    inverse=inverse)
