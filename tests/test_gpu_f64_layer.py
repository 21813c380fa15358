"""K26: a whole float64 spline coupling layer in one launch (csrc/rqs_resnet_f64.hip) behind the float64 branch of
PiecewiseRationalQuadraticCouplingTransform.  Every case asserts through the launch hook that "k26" ran -- or, for the
fallbacks, that it did not.

Three float64 evaluations are compared where no reference vector exists:  T, stock torch on the device (oracle/eager.py's
expressions, nothing of the product);  O, the product with `fuse_float64 = False` (stock GEMMs, K5d);  N, K26.  O and N
are equally exact float64 evaluations under the same conditioning, so N is held to
    max|N - T| <= 4 max|O - T| + 1e-13 (1 + max|T|):
the factor covers the scatter of a maximum over ~1e5 elements; a wrong fragment index, a dropped bias or a mis-staged
k-chunk is off by six orders or more.
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)


def RQ():
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform
    return PiecewiseRationalQuadraticCouplingTransform


class Launches:
    def __init__(self):
        self.names = []

    def begin(self, name):
        self.names.append(name)

    def end(self, token, nbytes):
        pass


@pytest.fixture(autouse=True)
def restore_switch():
    from nflows_amd import ops
    for word in ops._status_words.values():   # (the status word is the process's: an earlier test's NaN rows leave their bit)
        word.zero_()
    min_rows = RQ().fuse_float64_min_rows
    RQ().fuse_float64_min_rows = 0   # (the kernel itself is under test at every batch size; the size rule has its own test)
    yield
    RQ().fuse_float64_min_rows = min_rows
    RQ().fuse_float64 = True
    ops.set_launch_hook(None)


def call(fn, *args, fused=True, **kw):
    """fn(*args) under no_grad with the switch set; returns (result, names of the hooked launches)"""
    from nflows_amd import ops
    RQ().fuse_float64 = fused
    rec = Launches()
    ops.set_launch_hook(rec)
    try:
        with torch.no_grad():
            res = fn(*args, **kw)
    finally:
        ops.set_launch_hook(None)
        RQ().fuse_float64 = True
    return res, rec.names


def ran_k26(names, times):
    assert names.count("k26") == times, names


def make_layer(D=64, H=128, nb=2, K=8, tails="linear", tail_bound=3.0, seed=0, mask=None, steep=True, **kw):
    """one coupling layer, float64 on the device, with steep splines (helpers.steepen's scales of the steep fixtures)"""
    from nflows_amd.nn.nets.resnet import ResidualNet
    torch.manual_seed(seed)
    mask = torch.arange(D) % 2 if mask is None else mask
    net_kw = {k: kw.pop(k) for k in list(kw) if k in ("activation", "use_batch_norm", "context_features", "dropout_probability")}
    t = RQ()(mask, lambda i, o: ResidualNet(i, o, H, num_blocks=nb, **net_kw), num_bins=K, tails=tails,
             tail_bound=tail_bound, **kw)
    if steep:
        P = 3 * K - 1 if tails == "linear" else 3 * K + 1
        with torch.no_grad():
            for name, p in t.named_parameters():
                if "linear_layers.1" in name:
                    p.mul_(10.0)
                elif "final_layer" in name:
                    v = p.view(p.shape[0] // P, P, *p.shape[1:])
                    v[:, :2 * K].mul_(60.0)
                    v[:, 2 * K:].mul_(6.0)
    return t.double().to(DEV).eval()


def rows(B, D, tails="linear", tail_bound=3.0, seed=1):
    g = torch.Generator().manual_seed(seed)
    if tails is None:
        return (0.01 + 0.98 * torch.rand(B, D, generator=g, dtype=torch.float64)).to(DEV)
    return (0.45 * tail_bound * torch.randn(B, D, generator=g, dtype=torch.float64)).to(DEV)


def truth_layer(t, x, inverse):
    """T for one layer: oracle/eager.py's expressions (stock torch, float64, on the device) with the layer's own settings"""
    from oracle import eager
    with torch.no_grad():
        ident, xt = x[:, t.identity_features], x[:, t.transform_features]
        K = t.num_bins
        params = t.transform_net(ident).reshape(x.shape[0], xt.shape[1], -1)   # (ResidualNet.forward: stock float64 ops)
        uw = params[..., :K] / np.sqrt(t.transform_net.hidden_features)
        uh = params[..., K:2 * K] / np.sqrt(t.transform_net.hidden_features)
        kw = dict(min_bin_width=t.min_bin_width, min_bin_height=t.min_bin_height, min_derivative=t.min_derivative)
        if t.tails == "linear":
            yt, lad = eager.rqs_unconstrained(xt, uw, uh, params[..., 2 * K:].clone(), inverse=inverse, tail_bound=t.tail_bound, **kw)
        else:
            yt, lad = eager.rqs_constrained(xt, uw, uh, params[..., 2 * K:], inverse=inverse, **kw)
        out = torch.empty_like(x)
        out[:, t.identity_features] = ident
        out[:, t.transform_features] = yt
        return out, lad.sum(dim=1)


def three_way(n, o, t, what):
    """rule 2 of the module docstring; returns the ratio max|N - T| / max|O - T|"""
    n, o, t = (v.detach().cpu().numpy() for v in (n, o, t))
    assert np.array_equal(np.isfinite(n), np.isfinite(t)), what
    en, eo = np.abs(n - t).max(), np.abs(o - t).max()
    print("%s: max|N-T| %.3e  max|O-T| %.3e  scale %.2e" % (what, en, eo, np.abs(t).max()))
    assert en <= 4 * eo + 1e-13 * (1 + np.abs(t).max()), "%s: N %.3e O %.3e" % (what, en, eo)
    return en / max(eo, 1e-300)


def check_layer_three_way(t, x, what, accumulate=False):
    for inverse in (False, True):
        fn = t.inverse if inverse else t.forward
        xin = x
        if inverse:   # (inverse inputs: points of the layer's range)
            xin = call(t.forward, x, fused=False)[0][0]
        kw = {}
        base = None
        if accumulate:
            base = torch.randn(x.shape[0], dtype=torch.float64, device=DEV)
        (yn, ln), names = call(fn, xin, logabsdet_accumulator=base.clone() if accumulate else None, **kw)
        ran_k26(names, 1)
        (yo, lo), names = call(fn, xin, logabsdet_accumulator=base.clone() if accumulate else None, fused=False, **kw)
        ran_k26(names, 0)
        yt, lt = truth_layer(t, xin, inverse)
        if accumulate:
            lt = base + lt
        tag = "%s %s" % (what, "inverse" if inverse else "forward")
        three_way(yn, yo, yt, tag + " y")
        three_way(ln, lo, lt, tag + " lad")
        assert torch.equal(yn[:, t.identity_features], xin[:, t.identity_features])


# ---------------------------------------------------------------------------------------------- 1. reference vectors
def _golden_flows(golden_dir):
    from helpers import parse_kwargs, steep_flow
    from test_gpu_flows import build, load_state
    g = np.load(os.path.join(golden_dir, "flows.npz"))
    for name, cfg in g["meta"]:
        if str(name) in ("nsf_small", "nsf_d64"):
            cfg = parse_kwargs(cfg)
            flow = build(cfg)
            load_state(flow, g, str(name))
            yield str(name), flow, g, cfg["L"]
    for case in ("steep_nsf_k8", "steep_nsf_k8_deep", "steep_nsf_k10"):
        flow, g, cfg = steep_flow(golden_dir, case)
        yield case, flow, g, cfg["L"]
    gb = np.load(os.path.join(golden_dir, "flows_bins.npz"))
    for name, cfg in gb["meta"]:
        if parse_kwargs(str(cfg)).get("activation", "relu") == "relu":
            flow, g, cfg = steep_flow(golden_dir, str(name), "flows_bins.npz")
            yield str(name), flow, g, cfg["L"]


def test_reference_float64_vectors(golden_dir):
    """The real reference's float64 results of the committed flows (flows.npz, flows_steep.npz, the ReLU cases of
    flows_bins.npz), log_prob and both directions, under the rule test_float64_flows_run_on_the_device applies to this
    path: max|got - ref| <= 1e-10 (1 + max|ref|)."""
    import nflows_amd
    for name, flow, g, L in _golden_flows(golden_dir):
        flow = flow.double().to(DEV).eval()
        x = torch.from_numpy(g[name + "/x"]).double().to(DEV)
        noise = torch.from_numpy(g[name + "/noise"]).double().to(DEV)
        lp, names = call(flow.log_prob, x)
        ran_k26(names, L)
        (z, lad), names = call(flow._transform, x)
        ran_k26(names, L)
        (xs, lad_inv), names = call(flow._transform.inverse, noise)
        ran_k26(names, L)
        nflows_amd.check_status()
        # (the switched-off path on the same vectors, printed beside K26's figures: DESIGN.md section 4 quotes both)
        off = [call(flow.log_prob, x, fused=False)[0], *call(flow._transform, x, fused=False)[0],
               *call(flow._transform.inverse, noise, fused=False)[0]]
        keys = ("log_prob64", "z64", "lad64", "inv_x64", "inv_lad64")
        for got, old, key in zip((lp, z, lad, xs, lad_inv), off, keys):
            ref = g[name + "/" + key]
            err, err_off = np.abs(got.cpu().numpy() - ref).max(), np.abs(old.cpu().numpy() - ref).max()
            print("%s %s: K26 %.3e, switched off %.3e (bound %.3e)" % (name, key, err, err_off, 1e-10 * (1 + np.abs(ref).max())))
            assert got.dtype == torch.float64 and err <= 1e-10 * (1 + np.abs(ref).max()), (name, key, err)


def test_reference_float64_vectors_tails_none(golden_dir):
    import nflows_amd
    from test_gpu_tails_none import _cases, _flow
    g, cases = _cases(golden_dir)
    for name, cfg in cases:
        t = _flow(g, name, cfg).double().to(DEV)
        x = torch.from_numpy(g[name + "/x"]).double().to(DEV)
        y = torch.from_numpy(g[name + "/y"]).double().to(DEV)
        (z, lad), names = call(t, x)
        ran_k26(names, cfg["L"])
        (xi, ladi), names = call(t.inverse, y)
        ran_k26(names, cfg["L"])
        nflows_amd.check_status()
        for got, key in ((z, "z64"), (lad, "lad64"), (xi, "inv_x64"), (ladi, "inv_lad64")):
            ref = g[name + "/" + key]
            err = np.abs(got.cpu().numpy() - ref).max()
            print("%s %s: %.3e (bound %.3e)" % (name, key, err, 1e-10 * (1 + np.abs(ref).max())))
            assert err <= 1e-10 * (1 + np.abs(ref).max()), (name, key, err)


# ---------------------------------------------------------------------------------------------- 2. three evaluations
def test_three_float64_evaluations():
    """One layer, 32 / 32 features, H = 128, two blocks, 8 bins, steepened (helpers.steepen), 4 096 rows: T from
    helpers.eager_oracle on the device, O and N from the product.  Measured max|N - T| / max|O - T| on one MI355X: z 5.1e-13 /
    5.1e-13, lad 9.11e-12 / 9.14e-12, inverse x 2.26e-12 / 2.26e-12, inverse lad 2.70e-11 / 2.70e-11 -- ratios 1.00
    (why, and what they were before the Linears' sums started at zero)."""
    from helpers import eager_oracle, steepen
    from nflows_amd import configs
    flow_cpu = steepen(configs.rq_nsf_flow(1, 64, 8, 128, 2, 3.0, seed=31), 8, 60.0, 6.0, 10.0).eval()
    g = torch.Generator().manual_seed(32)
    x, noise = 1.3 * torch.randn(4096, 64, generator=g), 1.3 * torch.randn(4096, 64, generator=g)
    T = eager_oracle(flow_cpu, x, noise, fp64_device=DEV)
    flow = copy.deepcopy(flow_cpu).double().to(DEV).eval()
    xd, nd = x.double().to(DEV), noise.double().to(DEV)
    (zn, ln), names = call(flow._transform, xd)
    ran_k26(names, 1)
    (xn, lin), names = call(flow._transform.inverse, nd)
    ran_k26(names, 1)
    (zo, lo), names = call(flow._transform, xd, fused=False)
    ran_k26(names, 0)
    (xo, lio), _ = call(flow._transform.inverse, nd, fused=False)
    for n, o, key in ((zn, zo, "z64"), (ln, lo, "lad64"), (xn, xo, "xi64"), (lin, lio, "ladi64")):
        three_way(n, o, torch.from_numpy(T[key]), "one layer " + key)


# ---------------------------------------------------------------------------------------------- 3. the spline stage exactly
@pytest.mark.parametrize("tails", ["linear", None])
@pytest.mark.parametrize("K,dt", [(2, 64), (8, 32), (10, 5), (32, 1), (8, 1), (10, 64), (32, 5), (2, 32)])
def test_spline_stage_bit_equal_with_constant_logits(K, dt, tails):
    """final_layer.weight = 0 and a random bias: the logits are the bias in both paths, so z (forward) and x (inverse)
    are bit-equal to the switched-off path -- the chunking of the final Linear and the logit indexing --, and lad
    differs by its summation order only: 8 eps sum|terms|."""
    D = dt + 32
    mask = torch.cat((torch.zeros(32), torch.ones(dt)))
    t = make_layer(D, 128, 2, K, tails, mask=mask, seed=K + dt)
    with torch.no_grad():
        t.transform_net.final_layer.weight.zero_()
        t.transform_net.final_layer.bias.copy_(3.0 * torch.randn(t.transform_net.final_layer.bias.shape, dtype=torch.float64))
    x = rows(100, D, tails)
    for inverse in (False, True):
        fn = t.inverse if inverse else t.forward
        (yn, ln), names = call(fn, x)
        ran_k26(names, 1)
        (yo, lo), names = call(fn, x, fused=False)
        ran_k26(names, 0)
        assert torch.equal(yn, yo), (K, dt, tails, inverse, float((yn - yo).abs().max()))
        # the terms: the switched-off path's per-element log-derivatives
        from nflows_amd import ops
        with torch.no_grad():
            params = t.transform_net(x[:, t.identity_features]).reshape(x.shape[0], dt, -1)
            _, terms = ops.rqs_elementwise(x[:, t.transform_features].contiguous(), params[..., :K], params[..., K:2 * K],
                                           params[..., 2 * K:], t._spec(), inverse)
        bound = 8 * EPS * terms.abs().sum(dim=1)
        assert bool(((ln - lo).abs() <= bound).all()), (K, dt, tails, inverse, float((ln - lo).abs().max()))


# ---------------------------------------------------------------------------------------------- 4. tiles and passes
def test_tiles_and_passes():
    """Row r of a batch is bit-equal to the same row evaluated alone, two identical calls are bit-equal, a guard band
    behind the outputs and logabsdet beyond B stay untouched -- at B = 1, 15, 16, 17, 100 and at a batch that gives a
    workgroup a second row block and ends in a ragged 16-row tile (from the launch plan)."""
    from nflows_amd import ops
    t = make_layer(64, 128, 2, 8)
    net = t.transform_net
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = ops.F64_LAYER_ROWS * cus + ops.F64_LAYER_ROWS + 5
    plan = ops.f64_layer_plan(big, cus)
    assert plan["tiles"] > plan["grid"] and big % 16 != 0 and big % ops.F64_LAYER_ROWS != 0
    packed = t._packed_resnet_f64()
    spec = t._spec()
    xall = rows(big, 64)
    for inverse in (False, True):
        (y_big, l_big), names = call(t.inverse if inverse else t.forward, xall)
        ran_k26(names, 1)
        label = ops.last_layer_kernel()
        assert "k26" in label and "grid=%d," % plan["grid"] in label and "tiles=%d" % plan["tiles"] in label, label
        (y_again, l_again), _ = call(t.inverse if inverse else t.forward, xall)
        assert torch.equal(y_big, y_again) and torch.equal(l_big, l_again)
        for r in (0, 15, 16, 63, 64, ops.F64_LAYER_ROWS * cus - 1, ops.F64_LAYER_ROWS * cus, ops.F64_LAYER_ROWS * cus + 17, big - 1):
            (y1, l1), _ = call(t.inverse if inverse else t.forward, xall[r:r + 1].contiguous())
            assert torch.equal(y1[0], y_big[r]) and torch.equal(l1[0], l_big[r]), (inverse, r)
        for B in (1, 15, 16, 17, 100):
            (yb, lb), names = call(t.inverse if inverse else t.forward, xall[:B].contiguous())
            ran_k26(names, 1)
            assert torch.equal(yb, y_big[:B]) and torch.equal(lb, l_big[:B]), (inverse, B)
            # the launch on buffers with a guard band: rows beyond B are neither read nor written
            guard = 37.0
            out = torch.full((B + 16, 64), guard, dtype=torch.float64, device=DEV)
            lad = torch.full((B + 16,), guard, dtype=torch.float64, device=DEV)
            xin = torch.full((B + 16, 64), float("nan"), dtype=torch.float64, device=DEV)
            xin[:B] = xall[:B]
            from nflows_amd import _native as N
            import ctypes
            rc = N.load().nfa_rqs_resnet_layer_f64(N.ptr(xin), N.ptr(packed), packed.numel(), N.ptr(t.identity_features),
                                                   N.ptr(t.transform_features), N.ptr(out), N.ptr(lad), None, B, 64, 32, 32,
                                                   net.hidden_features, len(net.blocks), ctypes.byref(spec),
                                                   N.FLAG_INVERSE if inverse else 0, N.stream_handle(torch.device(DEV)))
            assert rc == 0
            assert torch.equal(out[:B], y_big[:B]) and torch.equal(lad[:B], l_big[:B])
            assert bool((out[B:] == guard).all()) and bool((lad[B:] == guard).all())


# ---------------------------------------------------------------------------------------------- 5. shapes
@pytest.mark.parametrize("H,nb,D", [(16, 0, 2), (24, 1, 7), (100, 3, 64), (128, 5, 128), (128, 0, 7), (16, 5, 64), (24, 3, 128),
                                    (100, 1, 2)])
def test_shapes(H, nb, D):
    for even in (False, True):   # (both alternating masks: odd D gives the halves different sizes)
        mask = (torch.arange(D) + int(even)) % 2
        t = make_layer(D, H, nb, 8, mask=mask, seed=H + nb + D)
        check_layer_three_way(t, rows(256, D), "H%d nb%d D%d" % (H, nb, D))


@pytest.mark.parametrize("kw", [dict(min_bin_width=5e-3, min_bin_height=2e-2, min_derivative=1e-2), dict(tail_bound=1.0),
                                dict(tail_bound=3.0), dict(accumulate=True), dict(tails=None), dict(K=32), dict(K=2)])
def test_settings(kw):
    kw = dict(kw)
    accumulate = kw.pop("accumulate", False)
    t = make_layer(64, 128, 2, kw.pop("K", 8), seed=7, **kw)
    check_layer_three_way(t, rows(256, 64, t.tails, t.tail_bound), str(kw), accumulate=accumulate)


# ---------------------------------------------------------------------------------------------- 6. edges
@pytest.mark.parametrize("H,nb", [(128, 2), (100, 2), (24, 0), (24, 1)])
def test_non_finite_rows(H, nb):
    """NaN / +-inf / 1e300 in identity and transformed columns: the non-finite pattern of the switched-off path, finite
    rows bit-equal to a batch without the bad rows -- also at hidden widths that are no multiple of 16, whose zero-padded
    columns must not turn 0 x inf into a NaN of the whole row."""
    t = make_layer(64, H, nb, 8)
    x = rows(100, 64)
    bad = x.clone()
    idc, trc = [int(c) for c in t.identity_features[:4]], [int(c) for c in t.transform_features[:4]]
    for r, (c, v) in enumerate(zip(idc + trc, [float("nan"), float("inf"), float("-inf"), 1e300] * 2)):
        bad[3 + 7 * r, c] = v
    touched = [3 + 7 * r for r in range(8)]
    clean = [r for r in range(100) if r not in touched]
    for inverse in (False, True):
        fn = t.inverse if inverse else t.forward
        (yn, ln), names = call(fn, bad)
        ran_k26(names, 1)
        (yo, lo), _ = call(fn, bad, fused=False)
        for n, o in ((yn, yo), (ln, lo)):
            assert torch.equal(torch.isnan(n), torch.isnan(o)) and torch.equal(torch.isinf(n), torch.isinf(o)), (H, nb, inverse)
            assert torch.equal(n[torch.isinf(o)], o[torch.isinf(o)])
        (yc, lc), _ = call(fn, x[clean].contiguous())
        assert torch.equal(yn[clean], yc) and torch.equal(ln[clean], lc)


def test_tails_none_outside_the_box_raises():
    from nflows_amd.transforms import InputOutsideDomain
    t = make_layer(16, 32, 2, 8, tails=None)
    x = rows(64, 16, None)
    (_, _), names = call(t.forward, x)
    ran_k26(names, 1)
    x[7, int(t.transform_features[0])] = 1.5
    with pytest.raises(InputOutsideDomain):
        call(t.forward, x)


# ---------------------------------------------------------------------------------------------- 7. weights
def test_packed_weights_follow_the_parameters():
    t = make_layer(16, 32, 2, 8)
    x = rows(64, 16)
    call(t.forward, x)
    opt = torch.optim.Adam(t.parameters(), lr=1e-2)
    with torch.enable_grad():
        y, lad = t(x)
        (y.square().mean() - lad.mean()).backward()
    opt.step()
    for step in ("adam", "data"):
        if step == "data":
            for p in t.parameters():
                p.data.mul_(2)
        (yn, ln), names = call(t.forward, x)
        ran_k26(names, 1)
        fresh = copy.deepcopy(t)
        for slot in ("_packed_f64_cache", "_weights_list", "_contents"):
            fresh.__dict__.pop(slot, None)
        (yf, lf), names = call(fresh.forward, x)
        ran_k26(names, 1)
        assert torch.equal(yn, yf) and torch.equal(ln, lf), step


@pytest.mark.parametrize("H,di,nb,K,tails", [(24, 3, 2, 8, "linear"), (100, 3, 3, 10, None), (16, 1, 0, 2, "linear"),
                                             (128, 64, 2, 32, "linear"), (100, 33, 1, 8, "linear")])
def test_device_packer_is_the_reference_packer(H, di, nb, K, tails):
    """nfa_pack_resnet_f64 against ops.pack_resnet_f64_reference (held to the documented layout on the CPU), bit for bit"""
    from nflows_amd import ops
    dt = 7
    mask = torch.cat((torch.zeros(di), torch.ones(dt)))
    t = make_layer(di + dt, H, nb, K, tails, mask=mask, seed=H + di)
    P = t._transform_dim_multiplier()
    got = ops.pack_resnet_f64(t.transform_net, dt, P)
    want = ops.pack_resnet_f64_reference(copy.deepcopy(t.transform_net).cpu(), dt, P)
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), want)


# ---------------------------------------------------------------------------------------------- 8. fallbacks
def _user_subclass():
    class Mine(RQ()):
        def _piecewise_cdf(self, inputs, transform_params, inverse=False):
            return super()._piecewise_cdf(inputs, transform_params, inverse)
    return Mine


@pytest.mark.parametrize("case", ["grad", "context", "leaky_relu", "H256", "batch_norm", "unconditional", "user_hook", "switch"])
def test_fallbacks_keep_the_old_path(case, monkeypatch):
    from torch.nn import functional as F
    ctx = None
    kw = {}
    if case == "context":
        kw["context_features"] = 3
        ctx = torch.randn(64, 3, dtype=torch.float64, device=DEV)
    elif case == "leaky_relu":
        kw["activation"] = F.leaky_relu
    elif case == "batch_norm":
        kw["use_batch_norm"] = True
    elif case == "unconditional":
        kw["apply_unconditional_transform"] = True
    H = 256 if case == "H256" else 32
    t = make_layer(16, H, 2, 8, **kw)
    if case == "user_hook":
        t.__class__ = _user_subclass()
    x = rows(64, 16)

    def run(fused):
        from nflows_amd import ops
        RQ().fuse_float64 = fused
        rec = Launches()
        ops.set_launch_hook(rec)
        try:
            with (torch.enable_grad() if case == "grad" else torch.no_grad()):
                res = t(x, ctx) if ctx is not None else t(x)
        finally:
            ops.set_launch_hook(None)
            assert "k26" not in rec.names or (fused and case == "switch")
        return res, rec.names
    if case == "unconditional":
        # (today's path has no float64 unconditional transform: it raises, and with the switch on the same error comes
        #  from the same place -- the gate sends the layer there)
        for fused in (False, True):
            with pytest.raises(NotImplementedError, match="only float32 is implemented"):
                run(fused)
        return
    if case == "switch":
        (yn, ln), names = run(False)
    else:
        (yn, ln), names = run(True)
    ran_k26(names, 0)
    (yo, lo), names = run(False)
    ran_k26(names, 0)
    assert torch.equal(yn.detach(), yo.detach()) and torch.equal(ln.detach(), lo.detach())
    if case == "switch":   # ... and the same layer with the switch on does take the kernel
        _, names = run(True)
        ran_k26(names, 1)


def test_size_rule():
    """Conditioners wider than 32 keep the generic path below `fuse_float64_min_rows` rows (8 192: measured slower at
    1 024 rows of width 128, faster from 8 192 on); narrower ones take K26 at every size."""
    RQ().fuse_float64_min_rows = 8192
    wide, narrow = make_layer(16, 128, 2, 8), make_layer(16, 32, 2, 8)
    for t, B, times in ((wide, 1024, 0), (wide, 8191, 0), (wide, 8192, 1), (narrow, 1, 1), (narrow, 1024, 1)):
        x = rows(B, 16)
        (yn, ln), names = call(t.forward, x)
        ran_k26(names, times)
        if not times:
            (yo, lo), _ = call(t.forward, x, fused=False)
            assert torch.equal(yn, yo) and torch.equal(ln, lo)


# ---------------------------------------------------------------------------------------------- 9. round trip
def test_round_trip_of_the_baseline_flow():
    """inverse(forward(x)) of the 32-layer BASELINE flow in float64 at 2 048 rows: not worse than with the switch off
    (maximum <= 2 x the switched-off maximum).  Measured on one MI355X: 2.6e-9 with K26, 3.6e-9 switched off (DESIGN.md
    section 4, K26)."""
    from nflows_amd import configs
    flow = configs.rq_nsf_flow(num_layers=32, features=64, num_bins=8, hidden_features=128, seed=0)
    with torch.no_grad():
        for name, p in flow.named_parameters():   # (bench.py's steepening of the freshly initialised flow)
            if "final_layer" in name:
                p.mul_(4.0)
            elif "linear_layers.1" in name:
                p.mul_(30.0)
    flow = flow.double().to(DEV).eval()
    x = torch.randn(2048, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(DEV)
    err = {}
    for fused in (True, False):
        (z, _), names = call(flow._transform, x, fused=fused)
        ran_k26(names, 32 if fused else 0)
        (xr, _), names = call(flow._transform.inverse, z, fused=fused)
        ran_k26(names, 32 if fused else 0)
        err[fused] = float((xr - x).abs().max())
    print("round trip: K26 %.3e, switched off %.3e" % (err[True], err[False]))
    assert err[True] <= 2 * err[False], err
