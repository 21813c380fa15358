"""The Transform API -- the drop-in boundary of this package.

Mirrors nflows/transforms/base.py: `Transform.forward/inverse(inputs, context=None) ->
(outputs, logabsdet)` (:22-29), `CompositeTransform` (:32-60) and `InverseTransform` (:215-231).

MI355X-specific addition: `CompositeTransform` recognises a column `Permutation` that is
adjacent to a coupling layer and hands the permutation to the coupling kernel (gather on the way
in for `forward`, scatter on the way out for `inverse`), which removes one full read+write pass
over the [batch, features] activations per layer.  Folding a permutation is bit-identical to
running the two transforms one after the other (it only changes which column a kernel reads or
writes).  The whole-layer kernel is a different matter: it computes the conditioner's GEMMs in its
own summation order, so its results agree with the layer-by-layer path to fp32 rounding, not bit
for bit.  It works on full 128-row blocks; a ragged batch is padded with zero rows whose results are
dropped, so every row takes the same kernel and its result is bit-identical whatever the batch size
(rows are independent inside a block).  `CompositeTransform.fuse_layer_runs = False` and
`PiecewiseRationalQuadraticCouplingTransform.fuse_conditioner = False` select the layer-by-layer
path everywhere.
"""
import torch
from torch import nn

from .. import _cache
from .. import ops
from ..errors import InputOutsideDomain, InverseNotAvailable  # noqa: F401  (re-exported)


class Transform(nn.Module):
    """Base class of all transforms."""

    # weights arriving through load_state_dict / .to() / .cuda() / .double(): drop the packed copies
    def _load_from_state_dict(self, *args, **kwargs):
        _cache.invalidate()
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, *args, **kwargs):
        _cache.invalidate()
        return super()._apply(*args, **kwargs)

    def forward(self, inputs, context=None):
        raise NotImplementedError()

    def inverse(self, inputs, context=None):
        raise InverseNotAvailable()


def _is_column_permutation(t):
    from .permutations import Permutation
    return isinstance(t, Permutation) and t._dim == 1


def _accepts_fused_permutation(t, inputs):
    return (getattr(t, "supports_fused_permutation", False) and not getattr(t, "_user_hooks", False) and inputs.dim() == 2
            and inputs.dtype == torch.float32)   # (float64 flows take the generic device path; a user's hooks: the reference's sequence)


class RunLayer:
    """THE RUN PROTOCOL: what a layer provides so that `CompositeTransform` can hand a run of such layers -- with the
    column permutations between them -- to one launch of a whole-layer kernel.  The planner compares no kinds and knows no
    kernel; the first layer of a run answers for the run.  The implementers: `AffineCouplingTransform` (K11) and
    `PiecewiseRationalQuadraticCouplingTransform` (the K8 family) in coupling.py, and the two MADE-conditioned layers (K22,
    K29) through `_MadeKernelLayer` in autoregressive.py, which also runs a layer on its own as a run of one.

    Which layers form a run (read on every call, so kept to attribute reads):
      `_run_kind(context)`     the name of the kernel family the layer can join now (a string the planner only hands on), or None
      `_run_signature()`       a tuple; consecutive layers with equal signatures form one run
      `_user_hooks`, `unconditional_transform`, `features`      a layer with a user's hooks, with an unconditional
                               transform or of another width joins no run
      `_forward_only_run`      True: the density pass only, and a single layer is a run of one (otherwise two make a run)
      `_conditioner()`, `fuse_conditioner`, `_fused_geometry(others)`      the conditioner whose weights the plan follows,
                               the layer's switch (it may be set on an instance), the run's padded geometry
      `RUN_SWITCHES`           (class, names of its class-level A/B switches) entries, one line below each class
    The plan of a run (`_run_plan`: cached until a weight, a permutation or one of these answers changes):
      `_run_variant(geometry, tile16)`     hashable: what of the layer's state, besides weights and geometry, the packed
                               form depends on -- the engine and its constants; part of the plan's key
      `_run_packed(geometry)`  the layer's (weights, biases) blobs
      `_padded_split`          True: the tables take the geometry's padded transform / identity split
      `transform_features`, `identity_features`      the columns written into the two halves of the layer's table
      `_run_extras(layers, geometry, variant, tables)`     (f16 stream or None, K8x's blobs or None) of the run
    The launch:
      `_launch_run(plan, num_layers, geometry, inputs, context, inverse, accumulate_into, standard_normal_log_prob)`
                               `plan(tile16=0)` is the run's plan tuple; returns what the `ops` launcher returns
    The defaults below are those of a kernel with one packed form (K11, K22, K29)."""

    _forward_only_run = False
    _padded_split = False

    def _run_variant(self, geometry=None, tile16=0):
        return ()

    def _run_extras(self, layers, geometry, variant, tables):
        return None, None


RUN_SWITCHES = []   # [(class, names)]: appended to where a class that implements the run protocol is defined


def _switch_state():
    """The class-level A/B switches a run plan depends on."""
    return tuple([getattr(cls, name) for cls, names in RUN_SWITCHES for name in names])


def _layer_state(units):
    """Per-layer attributes a run plan depends on, re-read on every call: the layers' signatures (bins, tails,
    box, minimum sizes, engine ...), whether their conditioners are in training mode (active dropout), their
    unconditional transforms, and the A/B switches once more (they may be set on an instance)."""
    # (`_conditioner()`: the layer's conditioner from the plain `_modules` dict, without nn.Module's attribute fallback)
    return [(c._run_signature(), c._conditioner().training, c._modules.get("unconditional_transform") is None,
             c.fuse_conditioner, getattr(c, "fuse_final_linear", None)) for c, _ in units]


class _Run(list):
    """The units [(coupling, permutation or None)] of a run, with what is the same on every call kept beside
    them: the run's padded geometry (ops.fused_geometry over its layers) and how its weights are followed
    (_cache.RunWeights)."""

    def __init__(self, units):
        super().__init__(units)
        self._weights = _cache.RunWeights([c for c, _ in self])

    def geometry(self):
        held = self.__dict__.get("_geometry")
        if held is None:
            held = self[0][0]._fused_geometry(tuple(c for c, _ in self[1:]))
            self.__dict__["_geometry"] = held
        return held

    def weights_fingerprint(self):
        return self._weights.fingerprint()

    def verify_before_packing(self):
        self._weights.verify_before_packing()


def _permutation_key(p):
    perm = p._buffers["_permutation"]   # (the registered buffer, without nn.Module's attribute fallback)
    return id(perm), perm._version


def _run_weights_fingerprint(units):
    """What `_run_plan` keys the run's packed weights on: `_Run.weights_fingerprint()` -- one flat pass over the run
    (_cache.RunWeights) -- or, for a plain list of units, the per-layer keys."""
    if isinstance(units, _Run):
        return units.weights_fingerprint()
    return tuple([_cache.weights_key(c, c._conditioner()) for c, _ in units])


def _run_geometry(units):
    return units.geometry() if isinstance(units, _Run) else units[0][0]._fused_geometry(tuple(c for c, _ in units[1:]))


def _run_plan(owner, units, inverse, tile16=0):
    """Concatenated weight / bias blobs and the composed tables of a run, kept in `owner.__dict__["_run_plans"]` -- the
    composite's, or the layer's own for a run of one -- until a weight or a permutation changes.  (weights, biases, tables,
    f16 stream or None, K8x's (weights, biases, scales) or None); `tile16`: the mode of the f16 stream (ops.use_tile16)."""
    first = units[0][0]
    geometry = _run_geometry(units)   # one padded geometry for the run
    # (the key reads version counters only; the layers' packed blobs are looked at on a miss)
    variant = first._run_variant(geometry, tile16)
    ids = units.__dict__.get("_ids") if isinstance(units, _Run) else None
    if ids is None:
        ids = tuple([id(c) for c, _ in units])
        if isinstance(units, _Run):
            units.__dict__["_ids"] = ids
    key = (inverse, variant, geometry, ids, _run_weights_fingerprint(units),
           tuple([None if p is None else _permutation_key(p) for _, p in units]))
    cache = owner.__dict__.setdefault("_run_plans", {})
    plan = cache.get(key)
    if plan is None:
        # (a composite whose layers are runs of one -- MAF layers with a BatchNorm between them -- holds one plan per
        #  layer: with a fixed bound of 4 every call of an 8-layer flow rebuilt every plan, 0.9 ms each)
        if len(cache) > 4 + len(getattr(owner, "_transforms", ())):
            cache.clear()
        if isinstance(units, _Run):
            units.verify_before_packing()
        packed = [c._run_packed(geometry) for c, _ in units]
        weights = torch.cat([w for w, _ in packed], dim=0).contiguous()
        biases = torch.cat([b for _, b in packed]).contiguous()
        spec_layers = []
        for c, p in units:
            perm = None if p is None else p._permutation
            spec_layers.append((c.transform_features, c.identity_features,
                                None if inverse else perm, perm if inverse else None))
        Dp, dt4, di_u, _ = geometry
        split = first._padded_split
        tables = ops.flow_layer_tables(first.features, spec_layers, padded_features=Dp,
                                       padded_transform=dt4 if split else None, padded_identity=di_u if split else None)
        plan = cache[key] = (weights, biases, tables, *first._run_extras([c for c, _ in units], geometry, variant, tables))
    return plan


class CompositeTransform(Transform):
    """Applies transforms in the given order; log-determinants add up (base.py:45-52).

    Two levels of fusion on 2-D inputs (`fuse_permutations`): a column Permutation next to a
    coupling layer is folded into that layer's kernel, and a run of consecutive
    [Permutation, spline coupling] pairs whose conditioners the whole-layer kernel (K8) covers is
    executed in ONE launch (`fuse_layer_runs`): rows are independent across the whole run, so the
    kernel walks its rows through every layer without leaving LDS."""

    fuse_layer_runs = True  # class-level switch for A/B measurements

    def __init__(self, transforms, fuse_permutations=True):
        super().__init__()
        self._transforms = nn.ModuleList(transforms)
        self.fuse_permutations = fuse_permutations

    # ------------------------------------------------------------------ runs of K8 layers
    @staticmethod
    def _run_signature(coupling):
        return coupling._run_signature()

    def _collect_run(self, layers, start, inputs, context, inverse):
        """`_plan_run` behind a cache: which layers form a run depends on the call's shape (feature count, dtype,
        context, direction, grad mode), on the A/B switches and on per-layer attributes (`_run_signature`,
        training mode); the first two make the key, the last are re-read on every call (cheap attribute reads)
        and compared with what the cached plan saw.  Planning itself costs ~3 us per layer -- a 64-layer
        composite would spend more host time on it than the kernel takes on a small batch."""
        if not (self.fuse_layer_runs and inputs.dim() == 2 and inputs.shape[0] >= 1
                and inputs.dtype == torch.float32):
            return [], start
        ctx_key = None if context is None else (context.dim(), tuple(context.shape[1:]), context.dtype, context.is_cuda)
        key = (start, len(layers), inverse, inputs.shape[1], ctx_key, torch.is_grad_enabled(), _switch_state(),
               _cache.epoch())
        cache = self.__dict__.setdefault("_run_cache", {})
        hit = cache.get(key)
        if hit is not None:
            units, after, watched, seen = hit
            if len(layers) == len(watched) and all(a is b for a, b in zip(layers, watched)) \
                    and seen == self._watched_state(units, layers, after, inputs.shape[1], context):
                return units, after
        units, after = self._plan_run(layers, start, inputs, context, inverse)
        if units:   # (only runs are kept: "no run here" is decided afresh on every call)
            units = _Run(units)
            if len(cache) > 16 + len(layers):   # (layers that are runs of one: a run may start at every position)
                cache.clear()
            cache[key] = (units, after, list(layers), self._watched_state(units, layers, after, inputs.shape[1], context))
        return units, after

    @staticmethod
    def _joinable(t, features, context):
        kind = getattr(t, "_run_kind", None)   # whole-layer kernel this layer can join a run of
        # (a user's subclass, mixin or late assignment that overrides one of the reference's hooks joins none: coupling.py: _user_hooks)
        return (kind is not None and not t._user_hooks and t.unconditional_transform is None and t.features == features
                and kind(context) is not None)

    def _watched_state(self, units, layers, after, features, context):
        """What a cached plan is compared with on every call: the state of its layers and of the (up to two)
        layers behind it -- the run may have ended at one of them for a reason that no longer holds."""
        behind = [(t._run_signature(), self._joinable(t, features, context)) if getattr(t, "_run_kind", None) is not None else None
                  for t in layers[after:after + 2]]
        return _layer_state(units), behind

    def _plan_run(self, layers, start, inputs, context, inverse):
        """Longest run of units starting at `start`: forward a unit is [column Permutation]? +
        eligible coupling, inverse (layers already reversed) eligible coupling + [Permutation]?.
        Returns (units, next_index) with units = [(coupling, permutation or None)]."""
        units = []
        if not (self.fuse_layer_runs and inputs.dim() == 2 and inputs.shape[0] >= 1
                and inputs.dtype == torch.float32):
            return units, start

        def eligible(t):   # (K22 and K29 serve the density pass only: `_forward_only_run`)
            return self._joinable(t, inputs.shape[1], context) and not (inverse and getattr(t, "_forward_only_run", False))
        i, signature = start, None
        while i < len(layers):
            perm = None
            if not inverse:
                if _is_column_permutation(layers[i]) and i + 1 < len(layers) and eligible(layers[i + 1]):
                    perm, coupling, step = layers[i], layers[i + 1], 2
                elif eligible(layers[i]):
                    coupling, step = layers[i], 1
                else:
                    break
            else:
                if not eligible(layers[i]):
                    break
                coupling, step = layers[i], 1
                if i + 1 < len(layers) and _is_column_permutation(layers[i + 1]):
                    perm, step = layers[i + 1], 2
            sig = self._run_signature(coupling)
            if signature is not None and sig != signature:
                break
            signature = sig
            units.append((coupling, perm))
            i += step
        # (a coupling layer on its own has its whole-layer path in its own forward; an autoregressive layer is a run of one)
        if len(units) < (1 if units and getattr(units[0][0], "_forward_only_run", False) else 2):
            return [], start
        geometry = _run_geometry(units)
        ce = getattr(getattr(units[0][0], "transform_net", None), "context_features", None) or 0
        if geometry[0] > 128 or geometry[1] > 64 or geometry[2] + ce > 64:   # the run's padded geometry (ops.fused_geometry)
            return [], start
        return units, i

    def _run_plan(self, units, inverse, tile16=0):
        return _run_plan(self, units, inverse, tile16)

    def _run_fused(self, units, inputs, total, context, inverse, standard_normal_log_prob=False):
        """One launch for the run (ragged batches are padded to full 128-row blocks inside `ops`).  Returns
        the outputs (or log_prob with `standard_normal_log_prob`), or None when the kernel declines."""
        for _, p in units:
            if p is not None:
                p._check(inputs)
        head = units[0][0]._launch_run(lambda tile16=0: _run_plan(self, units, inverse, tile16), len(units),
                                       _run_geometry(units), inputs, context, inverse, total, standard_normal_log_prob)
        if head is None:
            return None
        return head[1] if standard_normal_log_prob else head[0]

    def standard_normal_log_prob(self, inputs, context=None):
        """Flow.log_prob (flows/base.py:42-49) for a StandardNormal base when the whole composite is ONE
        run of whole-layer kernels: the last layer's
        kernel adds -0.5 sum z^2 - 0.5 D log(2 pi) to the log-determinant while the rows are still
        on the chip, and z is never written.  Returns log_prob [batch], or None when the composite
        does not have that shape (the caller then takes the general route)."""
        if not self.fuse_permutations or inputs.dim() != 2:
            return None
        layers = list(self._transforms)
        units, after = self._collect_run(layers, 0, inputs, context, inverse=False)
        if not units or after != len(layers):
            return None
        return self._run_fused(units, inputs, None, context, inverse=False, standard_normal_log_prob=True)

    @staticmethod
    def _cascade(inputs, funcs, context):
        outputs = inputs
        total = inputs.new_zeros(inputs.shape[0])
        for func in funcs:
            outputs, logabsdet = func(outputs, context)
            total += logabsdet
        return outputs, total

    def forward(self, inputs, context=None):
        layers = list(self._transforms)
        if not self.fuse_permutations:
            return self._cascade(inputs, layers, context)
        outputs = inputs
        total = inputs.new_zeros(inputs.shape[0])
        i = 0
        while i < len(layers):
            units, after = self._collect_run(layers, i, outputs, context, inverse=False)
            if units:
                fused = self._run_fused(units, outputs, total, context, inverse=False)
                if fused is not None:
                    outputs, i = fused, after
                    continue
            t = layers[i]
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            if nxt is not None and _is_column_permutation(t) and _accepts_fused_permutation(nxt, outputs):
                t._check(outputs)
                # permutation folded into the layer's gather, `total += logabsdet` into its kernel
                outputs, _ = nxt.forward(outputs, context, in_perm=t._permutation,
                                         logabsdet_accumulator=total)
                i += 2
            elif _accepts_fused_permutation(t, outputs):
                outputs, _ = t.forward(outputs, context, logabsdet_accumulator=total)
                i += 1
            else:
                outputs, logabsdet = t(outputs, context)
                total += logabsdet
                i += 1
        return outputs, total

    def inverse(self, inputs, context=None):
        layers = list(self._transforms)[::-1]
        if not self.fuse_permutations:
            return self._cascade(inputs, (t.inverse for t in layers), context)
        outputs = inputs
        total = inputs.new_zeros(inputs.shape[0])
        i = 0
        while i < len(layers):
            units, after = self._collect_run(layers, i, outputs, context, inverse=True)
            if units:
                fused = self._run_fused(units, outputs, total, context, inverse=True)
                if fused is not None:
                    outputs, i = fused, after
                    continue
            t = layers[i]
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            if nxt is not None and _is_column_permutation(nxt) and _accepts_fused_permutation(t, outputs):
                nxt._check(outputs)
                # Permutation.inverse after the layer == scatter through the forward permutation
                outputs, _ = t.inverse(outputs, context, out_scatter=nxt._permutation,
                                       logabsdet_accumulator=total)
                i += 2
            elif _accepts_fused_permutation(t, outputs):
                outputs, _ = t.inverse(outputs, context, logabsdet_accumulator=total)
                i += 1
            else:
                outputs, logabsdet = t.inverse(outputs, context)
                total += logabsdet
                i += 1
        return outputs, total


class MultiscaleCompositeTransform(Transform):
    """Real NVP's multiscale architecture (nflows/transforms/base.py:63-212): after every transform
    but the last the result is halved along `split_dim`; the first half leaves as output (flattened),
    the second half feeds the next transform.  Bookkeeping only -- the transforms added do the work.
    Outputs are always [batch, total]."""

    def __init__(self, num_transforms, split_dim=1):
        if not (isinstance(split_dim, int) and split_dim > 0):
            raise TypeError("Split dimension must be a positive integer.")
        super().__init__()
        self._transforms = nn.ModuleList()
        self._output_shapes = []
        self._num_transforms = num_transforms
        self._split_dim = split_dim

    def add_transform(self, transform, transform_output_shape):
        """To be called `num_transforms` times.  `transform_output_shape`: the shape of one sample
        leaving `transform`.  Returns the shape that continues to the next transform (None after the
        last one)."""
        if len(self._transforms) == self._num_transforms:
            raise RuntimeError("Adding more than {} transforms is not allowed.".format(self._num_transforms))
        axis = self._split_dim - 1
        if axis >= len(transform_output_shape):
            raise ValueError("No split_dim in output shape")
        if transform_output_shape[axis] < 2:
            raise ValueError("Size of dimension {} must be at least 2.".format(self._split_dim))
        self._transforms.append(transform)
        if len(self._transforms) == self._num_transforms:   # the last transform's result is not split
            self._output_shapes.append(tuple(transform_output_shape))
            return None
        size = transform_output_shape[axis]
        leaves, continues = list(transform_output_shape), list(transform_output_shape)
        leaves[axis] = (size + 1) // 2     # torch.chunk gives the larger half first
        continues[axis] = size // 2
        self._output_shapes.append(tuple(leaves))
        return tuple(continues)

    def _require_complete(self):
        if self._num_transforms != len(self._transforms):
            raise RuntimeError("Expecting exactly {} transform(s) to be added.".format(self._num_transforms))

    def forward(self, inputs, context=None):
        if self._split_dim >= inputs.dim():
            raise ValueError("No split_dim in inputs.")
        self._require_complete()
        batch = inputs.shape[0]
        total = inputs.new_zeros(batch)
        pieces = []
        hiddens = inputs
        last = len(self._transforms) - 1
        for i, transform in enumerate(self._transforms):
            result, logabsdet = transform(hiddens, context)
            total = total + logabsdet
            if i < last:
                out, hiddens = torch.chunk(result, chunks=2, dim=self._split_dim)
                assert tuple(out.shape[1:]) == self._output_shapes[i]
            else:
                out = result
            pieces.append(out.reshape(batch, -1))
        return torch.cat(pieces, dim=-1), total

    def inverse(self, inputs, context=None):
        if inputs.dim() != 2:
            raise ValueError("Expecting NxD inputs")
        self._require_complete()
        batch = inputs.shape[0]
        chunks, start = [], 0
        for shape in self._output_shapes:
            n = 1
            for d in shape:
                n *= d
            chunks.append(inputs[:, start:start + n].reshape(batch, *shape))
            start += n
        total = inputs.new_zeros(batch)
        hiddens, logabsdet = self._transforms[-1].inverse(chunks[-1], context)
        total = total + logabsdet
        for transform, chunk in zip(reversed(self._transforms[:-1]), reversed(chunks[:-1])):
            hiddens, logabsdet = transform.inverse(torch.cat((chunk, hiddens), dim=self._split_dim), context)
            total = total + logabsdet
        return hiddens, total


class InverseTransform(Transform):
    """Swaps forward and inverse of a transform (base.py:215-231)."""

    def __init__(self, transform):
        super().__init__()
        self._transform = transform

    def forward(self, inputs, context=None):
        return self._transform.inverse(inputs, context)

    def inverse(self, inputs, context=None):
        return self._transform(inputs, context)
