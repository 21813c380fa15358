"""The packed-weight caches: their epochs, how the packs follow the parameters, and the keyed-cache helper.

The whole-layer kernels read re-tiled copies of the conditioner weights (ops.pack_*), cached per layer under
`weights_key` -- the parameters' (data_ptr, _version) -- or, for a run of layers, under `RunWeights.fingerprint`.
Writes that bypass the version counter (`p.data.copy_(...)`, `dist.broadcast(p.data)`, EMA weight swaps through `.data`)
are invisible to those signs; every cache key therefore also carries this module's epoch, which `invalidate()` advances.
`nflows_amd.invalidate_packed_weights()` is the public name; `load_state_dict`, `.to()/.cuda()` and
`parallel.broadcast_model` call it themselves, and so does every registration of a Parameter or buffer object on a
module (global hooks below): the cache keys read the version counters of a LIST of a conditioner's weights made once
per epoch instead of walking the module tree on every call.  Writes through a Parameter's own `.data` are noticed by
`WatchedParameter` and answered by a comparison of contents; the protocol is stated above `VERIFY_WEIGHTS_EVERY`.

`keyed(owner, slot, key, build)` is the one idiom every single-entry cache of the package goes through.
"""
import os

import torch

_epoch = 0
_data_epoch = 0


def epoch():
    return _epoch


def data_epoch():
    """Advances whenever the `.data` of a WATCHED parameter is read or assigned (below): somebody may have written through
    it.  The weight keys compare the CONTENTS of their parameters with the checksum on record when this has moved since they
    last looked (`weights_key`, `RunWeights.fingerprint` below) -- one batched comparison per event, and only layers whose
    contents really changed are repacked."""
    return _data_epoch


_base_data = torch._C.TensorBase.data


class WatchedParameter(torch.nn.Parameter):
    """A Parameter whose `.data` tells the packed-weight caches that it was touched (round 6).  A write through `.data`
    -- `p.data.copy_(ema)`, `dist.broadcast(p.data)`, `p.data.mul_(2)` -- reaches the storage without advancing the version
    counter the cache keys read: until round 5 the fused kernels then ran on the OLD packed weights until a periodic
    checksum noticed (up to 255 evaluations later, as an exception).  The reference reads `self.transform_net`'s
    parameters on every call (coupling.py:85); with this class the next call after such a write repacks from the new
    values: no stale evaluation, no exception, no device synchronisation on calls without such an event.  Parameters of
    the conditioners the fused kernels serve are re-classed in place (`watch`: same object, same identity for optimizers
    and DDP; pickling and state_dict are plain Parameter's).  Writes that avoid even this -- a view's `.data`, raw
    storage, foreign kernels on `data_ptr()` -- are left to the periodic checksum (NFA_VERIFY_WEIGHTS)."""

    @property
    def data(self):
        global _data_epoch
        _data_epoch += 1
        return _base_data.__get__(self, type(self))

    @data.setter
    def data(self, value):
        global _data_epoch
        _data_epoch += 1
        _base_data.__set__(self, value)


def watch(p):
    """re-class a plain Parameter as WatchedParameter, in place"""
    if type(p) is torch.nn.Parameter:
        p.__class__ = WatchedParameter


def invalidate():
    global _epoch
    _epoch += 1


def _on_registration(module, name, value):
    # a Parameter / buffer object (re)registered on any module: the per-layer lists of weights the cache keys
    # are built from (`weights_key`) may be stale
    invalidate()


def _install_hooks():
    try:
        from torch.nn.modules import module as _m
        _m.register_module_parameter_registration_hook(_on_registration)
        _m.register_module_buffer_registration_hook(_on_registration)
    except (ImportError, AttributeError):  # (older torch: the keys fall back to walking the module tree)
        return False
    return True


HOOKED = _install_hooks()


def keyed(owner, slot, key, build):
    """`build()`, kept in `owner.__dict__[slot]` with `key` and made again when the key changes"""
    cached = owner.__dict__.get(slot)
    if cached is None or cached[0] != key:
        cached = owner.__dict__[slot] = (key, build())
    return cached[1]


def _held_parameters(net):
    """[(the `_parameters` / `_buffers` dict of a leaf module, name, tensor)] of every parameter and buffer of `net`
    (buffers: the running statistics of batch-norm layers, folded into the packed weights).  The parameters are re-classed
    as WatchedParameter on the way: their `.data` then reports its use (writes through it reach no version counter)."""
    params = [(m._parameters, name, p) for m in net.modules() for name, p in m._parameters.items() if p is not None]
    for _, _, p in params:
        watch(p)
    return params + [(m._buffers, name, b) for m in net.modules() for name, b in m._buffers.items() if b is not None]


def _still_held(held, epoch):
    """A list of weights made once per epoch -- (epoch, net or nets, `_held_parameters` entries, ...) -- is still current:
    same epoch, and each held object still IS the entry of its module's dict.  The second catches swaps that bypass the
    registration hooks -- `torch.func.functional_call`, `stateless._reparametrize_module`, a direct
    `module._parameters[name] = other` -- and is checked on every call."""
    if held is None or held[0] != epoch or not HOOKED:
        return False
    for d, name, p in held[2]:
        if d.get(name) is not p:
            return False
    return True


class StalePackedWeights(RuntimeError):
    """NFA_VERIFY_WEIGHTS: a conditioner's weights changed without any of the signs the packed-weight caches look at --
    version counters, storage pointers, registrations, and (round 6) the `.data` of its Parameters (WatchedParameter):
    a write into raw storage, through a view's `.data`, by a foreign kernel.  The fused kernels have been using the OLD
    weights; `nflows_amd.invalidate_packed_weights()` after such writes is the remedy."""


# How the packed weights follow the parameters (round 6).
#   visible changes   in-place updates (version counters), rebound storage (data_ptr), (re)registered objects,
#                     load_state_dict / .to() (cache epoch): part of every weight key, the packs are rebuilt.
#   `.data`           reading or assigning the `.data` of a conditioner Parameter advances data_epoch(); the next
#                     use of a weight key compares the parameters' CONTENTS with the checksum recorded when the key was new
#                     (one synchronising comparison per layer, or one for a whole run) and, on a difference, advances the
#                     layer's `_data_salt` -- part of the key: repacked from the new values, nothing raised, and no call
#                     without such an event pays anything.
#   everything else   NFA_VERIFY_WEIGHTS=N (default 256; 0 = off, 1 = every use): every N-th use of a key repeats the
#                     comparison, staggered over the layers, and raises StalePackedWeights; also on every plan-cache miss of
#                     a run (RunWeights.verify_before_packing).  Skipped while a stream is being captured into a HIP graph.
# Per layer, in its `__dict__`: `_weights_list` (the held list of `weights_key`), `_contents` (the record of the layer's own
# key), `_contents_run` (the record of its slice of a run's fingerprint) and `_data_salt`.  The two records stay two: their
# use counts and key shapes differ (staggered periodic check against compare-on-miss).
VERIFY_WEIGHTS_EVERY = int(os.environ.get("NFA_VERIFY_WEIGHTS", "256") or 0)

_CHECKSUM_LAYOUTS = {}


def _checksum(params):
    """int64 [len(params)] on the parameters' device: per parameter the sum over its elements of (bit pattern as int32) x (an
    odd multiplier that depends on the position), modulo 2^64 -- exact, sensitive to the sign and the position of every
    element (round 5's fp32 norms were blind to a sign flip of a small entry), NaNs included (a bit pattern like any
    other).  fp32 parameters on one device: one concatenation, one multiply, one segmented sum; no synchronisation."""
    with torch.no_grad():
        params = [p.detach() for p in params]
        if not params:
            return torch.zeros(0, dtype=torch.int64)
        if not (all(p.dtype == torch.float32 for p in params) and len({p.device for p in params}) == 1):
            return torch.stack([(p.double().reshape(-1).view(torch.int64) >> 7).sum().cpu() + p.numel() for p in params])
        dev = params[0].device
        sizes = tuple(p.numel() for p in params)
        layout = _CHECKSUM_LAYOUTS.get((dev, sizes))
        if layout is None:
            if len(_CHECKSUM_LAYOUTS) > 64:
                _CHECKSUM_LAYOUTS.clear()
            sz = torch.tensor(sizes, device=dev)
            seg = torch.repeat_interleave(torch.arange(len(sizes), device=dev), sz)
            # (the position INSIDE the parameter: a parameter's checksum does not depend on what it is concatenated with)
            at = torch.arange(sum(sizes), dtype=torch.int64, device=dev) - (torch.cumsum(sz, 0) - sz)[seg]
            mult = ((at * 2654435761) % 2147483647) * 2 + 1
            layout = _CHECKSUM_LAYOUTS[(dev, sizes)] = (mult, seg)
        mult, seg = layout
        bits = torch.cat([p.reshape(-1) for p in params]).view(torch.int32).to(torch.int64)
        return torch.zeros(len(sizes), dtype=torch.int64, device=dev).index_add_(0, seg, bits * mult)


def _same_checksum(a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))    # (synchronises)


def _capturing(params):
    return bool(params) and params[0].is_cuda and torch.cuda.is_current_stream_capturing()


def _stale(owner):
    return StalePackedWeights(
        "the parameters of %s changed through a write the packed-weight caches cannot see (raw storage, a view's `.data`, a "
        "foreign kernel): call nflows_amd.invalidate_packed_weights() after such writes" % type(owner).__name__)


def _new_salt(owner):
    owner.__dict__["_data_salt"] = owner.__dict__.get("_data_salt", 0) + 1


def _data_event_answered(owner, slot, now, de):
    """The record `slot`, if there is one, takes `now` as its contents and `de` as the last `.data` event it answered"""
    state = owner.__dict__.get(slot)
    if state is not None:
        state[1], state[3] = now, de


def _track_contents(owner, slot, key, params, periodic=True, compare_now=False):
    """The record `owner.__dict__[slot]` = [visible key, checksum of the contents when the key was new, use count, data epoch]
    and what is done with it: a new key records (no synchronisation); a `.data` event since the record compares and, on a
    difference, advances `_data_salt` (repack, no exception); `periodic` counts uses and compares every
    NFA_VERIFY_WEIGHTS-th (`compare_now`: at once) -- a difference there is a write nothing announced: StalePackedWeights."""
    de = data_epoch()
    state = owner.__dict__.get(slot)
    if state is None or state[0] != key:
        # (the count starts at a per-layer offset: the layers of a flow are used once per call each, and 32 synchronising
        #  comparisons landing in ONE call were a 3 ms spike every 256th step)
        owner.__dict__[slot] = [key, _checksum(params), (id(owner) >> 6) % max(1, VERIFY_WEIGHTS_EVERY), de]
        return
    if state[3] != de:
        if _capturing(params):
            return
        now = _checksum(params)
        changed = not _same_checksum(now, state[1])
        _data_event_answered(owner, slot, now, de)
        if changed:
            _new_salt(owner)
        return
    if not VERIFY_WEIGHTS_EVERY or _capturing(params):
        return
    if periodic:
        state[2] += 1
    if (compare_now or (periodic and state[2] % VERIFY_WEIGHTS_EVERY == 0)) and not _same_checksum(_checksum(params), state[1]):
        owner.__dict__.pop(slot, None)
        raise _stale(owner)


def weights_key(owner, net):
    """Fingerprint of a conditioner's weights for the packed-weight caches: storage pointers and version counters of its
    parameters, read from a list made once per cache epoch (walking `net.parameters()` costs ~10 us per call and layer: a
    millisecond per `log_prob` of a 32-layer flow), and the layer's `_data_salt` (see above: writes through `.data`).
    In-place updates advance the counters; moves, `load_state_dict` and (re)registered Parameter objects advance the epoch;
    swaps that bypass the registration hooks are caught by `_still_held`."""
    e = epoch()
    held = owner.__dict__.get("_weights_list")
    if not _still_held(held, e) or held[1] is not net:
        held = owner.__dict__["_weights_list"] = (e, net, _held_parameters(net))
    # (data_ptr as well: `p.data = other` rebinds the storage without touching the counter)
    key = (e,) + tuple([(p.data_ptr(), p._version) for _, _, p in held[2]])
    _track_contents(owner, "_contents", key, [p for _, _, p in held[2]])
    return key + (owner.__dict__.get("_data_salt", 0),)


class RunWeights:
    """The weights of a whole run of layers in one flat pass (round 4).  `weights_key` layer by layer cost ~10 us per
    layer and call -- 0.3-0.4 ms per `log_prob` of a 32-layer flow, more than the kernel takes on 8 192 rows: the
    small-batch figures of bench.py were the HOST's.  Same signs as `weights_key` (epoch, identity of every held
    object in its module's dict, version counters, storage pointers), read from lists made once per epoch.
    `owners`: the layers of the run, each with `_conditioner()`."""

    def __init__(self, owners):
        self.owners = list(owners)
        self._flat = None   # (epoch, conditioners, `_held_parameters` entries of all of them, their tensors, per-layer bounds)
        self._data_seen = None   # data_epoch() of the last `.data` event answered
        self._verify_calls = 0

    def _flatten(self, epoch):
        nets = [c._conditioner() for c in self.owners]
        per_layer = [_held_parameters(net) for net in nets]
        entries = [e for held in per_layer for e in held]
        bounds, at = [], 0
        for held in per_layer:
            bounds.append((at, at + len(held)))
            at += len(held)
        self._flat = (epoch, nets, entries, [p for _, _, p in entries], bounds)
        return self._flat

    def fingerprint(self):
        e = epoch()
        flat = self._flat
        if not _still_held(flat, e):
            flat = self._flatten(e)
        else:
            for c, net in zip(self.owners, flat[1]):
                if c._conditioner() is not net:
                    flat = self._flatten(e)
                    break
        params = flat[3]
        key = (e, tuple([p._version for p in params]), tuple([p.data_ptr() for p in params]))
        every = VERIFY_WEIGHTS_EVERY
        de = data_epoch()
        if self._data_seen != de:
            # the `.data` of a watched parameter was touched since the run last looked (or this is its first use): every
            # layer's record is brought up to date -- ONE checksum over all parameters of the run, one synchronising
            # comparison; layers whose contents changed under an unchanged visible key get a new `_data_salt`
            if not _capturing(params):
                self._data_seen = de
                self._recheck(flat, key, de)
        elif every and params and not _capturing(params):
            # the periodic check: one layer at a time, every layer once per `every` calls (no call pays for all of them)
            n = self._verify_calls = self._verify_calls + 1
            stride = max(1, every // len(self.owners))
            if n % stride == 0:
                i = (n // stride) % len(self.owners)
                lo, hi = flat[4][i]
                _track_contents(self.owners[i], "_contents_run", (e, key[1][lo:hi], key[2][lo:hi]), params[lo:hi],
                                periodic=False, compare_now=True)
        return key + (tuple([c.__dict__.get("_data_salt", 0) for c in self.owners]),)

    def _recheck(self, flat, key, de):
        """A `.data` event (or the run's first use): per layer, contents on record under the layer's current visible key are
        compared with the contents now -- a difference, or no such record (the key moved since: nothing to compare with),
        advances the layer's `_data_salt`, i.e. its packs are rebuilt from the current values --, and the records are renewed."""
        params, bounds = flat[3], flat[4]
        now = _checksum(params)
        verdicts, rows = [], []
        for i, (c, (lo, hi)) in enumerate(zip(self.owners, bounds)):
            sub = (flat[0], key[1][lo:hi], key[2][lo:hi])
            state = c.__dict__.get("_contents_run")
            if state is not None and state[0] == sub and state[1].shape[0] == hi - lo:
                verdicts.append((state[1] == now[lo:hi]).all())
                rows.append(i)
            else:
                _new_salt(c)
            c.__dict__["_contents_run"] = [sub, now[lo:hi], 0, de]
            # (the layer's own record, `weights_key`: same event, same contents -- it must not answer it a second time)
            _data_event_answered(c, "_contents", now[lo:hi], de)
        if rows:
            for same, i in zip(torch.stack(verdicts).cpu().tolist(), rows):    # (the one synchronisation)
                if not same:
                    _new_salt(self.owners[i])

    def verify_before_packing(self):
        """Called on every plan-cache miss, before the layers' packed weights are looked up.  A miss does not mean the
        weights changed visibly -- the first inverse call, a batch that crosses the 16-sample-tile threshold, an evicted
        plan -- and the per-layer packs are keyed on version counters, storage pointers and the `.data` salt: a write that
        announced itself through none of them since the last pack would be packed into the NEW plan from the OLD blobs.
        So: a layer whose key is the one its checksum was recorded under is COMPARED now (StalePackedWeights on a
        difference); a layer with a new key gets its checksum recorded."""
        flat = self._flat
        if not VERIFY_WEIGHTS_EVERY or flat is None:
            return
        params = flat[3]
        if _capturing(params):
            return
        versions, ptrs = tuple([p._version for p in params]), tuple([p.data_ptr() for p in params])
        for c, (lo, hi) in zip(self.owners, flat[4]):
            _track_contents(c, "_contents_run", (flat[0], versions[lo:hi], ptrs[lo:hi]), params[lo:hi],
                            periodic=False, compare_now=True)
