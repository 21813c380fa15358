"""The sampling direction of the masked autoregressive affine flows (K23, csrc/made_inverse.hip): a restatement of the
reference's inverse in stock torch ops, the parity rule of the GPU tests, and a walk over the packed step blocks the way
the kernel walks them.

`layer_inverse` is AutoregressiveTransform.inverse (autoregressive.py:43-52) written out: D passes of the whole MADE
(`maf_cases.made_forward`) on the outputs so far, each followed by the affine inverse over all features
(autoregressive.py:109-121).  `restated_inverse` runs a flow's layers backwards with it (transforms/base.py:54-58,
permutations.py:31-43).  tests/test_maf_sample_host.py holds it to the fixture of the real reference."""
import copy

import numpy as np
import torch
from torch.nn import functional as F

import maf_cases

# the six shapes with weights a standard-normal draw can be pushed through in fp32 (the SHARPEN flows reach 4e52)
SAMPLING = dict(scale_final=0.5, scale_linear1=100.0)


def build_for_sampling(name):
    from nflows_amd import configs
    return configs.masked_affine_flow(**maf_cases.CASES[name], **SAMPLING).eval()


def layer_inverse(layer, z, context=None):
    net = layer.autoregressive_net
    x, lad = torch.zeros_like(z), None
    for _ in range(z.shape[1]):
        params = maf_cases.made_forward(net, x, context).view(-1, z.shape[1], 2)
        scale = F.softplus(params[..., 0]) + 1e-3
        x = (z - params[..., 1]) / scale
        lad = -torch.sum(torch.log(scale), dim=[1])
    return x, lad


def restated_inverse(flow, z, context=None):
    """(x, logabsdet) of flow._transform.inverse in the dtype of `z`; `flow` is used for its tensors only."""
    h, total = z, z.new_zeros(z.shape[0])
    for t in reversed(list(flow._transform._transforms)):
        if type(t).__name__.endswith("Permutation"):
            h = torch.index_select(h, 1, torch.argsort(t._permutation))
        else:
            h, lad = layer_inverse(t, h, context)
            total = total + lad
    return h, total


def inverse_pair(flow_cpu, z, context=None, fp64_device=None, fp32_device=None):
    """{x32, lad32, x64, lad64} as numpy arrays: the restatement in fp32 (the yardstick) and in fp64 (the truth), on the CPU
    or by the same stock ops on the devices given.  `z` is an fp32 tensor: both invert the same numbers."""
    out = {}
    with torch.no_grad():
        for tag, dtype, dev in (("32", torch.float32, fp32_device), ("64", torch.float64, fp64_device)):
            f = copy.deepcopy(flow_cpu).to(dtype)
            zz, cc = z.to(dtype), None if context is None else context.to(dtype)
            if dev is not None:
                f, zz, cc = f.to(dev), zz.to(dev), None if cc is None else cc.to(dev)
            x, lad = restated_inverse(f, zz, cc)
            out["x" + tag], out["lad" + tag] = x.cpu().numpy(), lad.cpu().numpy()
    return out


def fixture_z(flow_cpu, name, rows=None, seed=None):
    """fp32 z whose inverse stays small: the float64 density pass of the case's inputs (`maf_cases.fixture_inputs`, or
    `rows` fresh ones drawn the same way from `seed`), rounded.  Returns (z, context or None)."""
    if rows is None:
        x, context = maf_cases.fixture_inputs(name)
    else:
        cfg = maf_cases.CASES[name]
        g = torch.Generator().manual_seed(seed)
        x = 1.2 * torch.randn(rows, cfg["features"], generator=g)
        ce = cfg.get("context_features")
        context = None if ce is None else torch.randn(rows, ce, generator=g)
    with torch.no_grad():
        f64 = copy.deepcopy(flow_cpu).double()
        z = maf_cases.restated(f64, x.double(), None if context is None else context.double())[0]
    return z.float(), context


def error_figures(got, ref32, truth):
    got, ref32, truth = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref32, truth))
    e_got, e_ref = np.abs(got - truth), np.abs(ref32 - truth)
    return {"mean": (float(e_got.mean()), float(e_ref.mean())),
            "q999": (float(np.quantile(e_got, 0.999)), float(np.quantile(e_ref, 0.999))),
            "max": (float(e_got.max()), float(e_ref.max())),
            "above_4x_max": int((e_got > 4.0 * e_ref.max()).sum())}


def assert_parity(got, ref32, truth, what):
    """The project's rule (tests/test_gpu_steep.py): against the fp64 truth, mean and 99.9 % quantile of |error| at most
    2 x the fp32 yardstick's, at most three elements above 4 x the yardstick's maximum, everything finite."""
    got = np.asarray(got)
    assert np.isfinite(got).all(), what + ": non-finite results"
    assert np.isfinite(np.asarray(truth)).all() and np.isfinite(np.asarray(ref32)).all(), what + ": non-finite reference"
    f = error_figures(got, ref32, truth)
    print(what, f)
    for k in ("mean", "q999"):
        assert f[k][0] <= 2.0 * f[k][1], "%s: %s error vs float64 %.3e exceeds 2 x the yardstick's %.3e" % (
            what, k, f[k][0], f[k][1])
    assert f["above_4x_max"] <= 3, "%s: %d elements above 4 x the yardstick's maximum %.3e" % (
        what, f["above_4x_max"], f["max"][1])
    return f


# ---- the packed schedule, walked the way the kernel walks it ---------------------------------------------------------------

def walk_schedule(schedule, x, context_terms=None, block_cap=None):
    """Parameters [T, P] in float64 that K12 / K23's loop forms from the step blocks of `ops.pack_made_schedule` for one
    sample `x` (float64, [D]): per block the units in the order of the table -- dot product, bias, context term, residual
    add, ReLU --, and on a step's last block feature t's output rows on the hidden vector as it stands; then "feature t is
    found".  `context_terms`: float64 [C, >= H].  Asserts the block format on the way.  Also returns the number of
    continuation blocks per step."""
    blocks_f, block_at, layout = schedule
    blocks_f, block_at = blocks_f.cpu(), block_at.cpu()
    n, is_res, final_src, stream_vec, num_vectors, Hp, Xp, max_block = layout[:8]
    cfg = [layout[8 + 5 * l:13 + 5 * l] for l in range(n)]
    nblocks = block_at.numel() - 2
    assert blocks_f.numel() == int(block_at[-1]) * 256 and max_block % 256 == 0 and int(block_at[-1]) == int(block_at[-2])
    xs = torch.zeros(Xp, dtype=torch.float64)
    vecs = torch.zeros(num_vectors, Hp, dtype=torch.float64)
    params, continuation, t, in_layer_order = [], [0], 0, []
    for b in range(nblocks):
        blk = blocks_f[int(block_at[b]) * 256:int(block_at[b + 1]) * 256]
        assert 256 <= blk.numel() <= max_block and (block_cap is None or blk.numel() <= block_cap)
        hdr = blk[:16].view(torch.int32)
        units, rows, out_rows, out_bias, continued = (int(v) for v in hdr[:5])
        assert rows == 16 + 8 * units and continued in (0, 1) and not hdr[5:].any()
        for u in range(units):
            e = blk[16 + 8 * u:24 + 8 * u]
            bias = float(e[0])
            j, kp, src, dst, add_stream, set_stream, ctx_v = (int(v) for v in e[1:].view(torch.int32))
            assert [kp, src, dst, add_stream, set_stream] in cfg and 0 <= j < Hp
            in_layer_order.append(cfg.index([kp, src, dst, add_stream, set_stream]))
            w = blk[rows:rows + kp].double()
            rows += kp
            v = float(w @ (xs[:kp] if src < 0 else vecs[src, :kp])) + bias
            if ctx_v:
                assert context_terms is not None and ctx_v <= context_terms.shape[0]
                v = v + float(context_terms[ctx_v - 1, j])
            if add_stream:
                v = float(vecs[stream_vec, j]) + v
            if set_stream:
                vecs[stream_vec, j] = v
            if dst >= 0:
                vecs[dst, j] = max(v, 0.0)
        assert rows == out_rows
        if continued:
            assert units >= 1 and out_bias == 0, "a continuation block carries units only"
            continuation[-1] += 1
            continue
        assert in_layer_order == sorted(in_layer_order), "the units of a step run in layer order across its blocks"
        in_layer_order = []
        if out_bias == 0:          # the block behind the last step
            assert b == nblocks - 1
            break
        P = (out_bias - out_rows) // Hp
        assert out_bias == out_rows + P * Hp and out_bias + P <= blk.numel()
        wf = blk[out_rows:out_bias].double().view(P, Hp)
        params.append(wf @ vecs[final_src] + blk[out_bias:out_bias + P].double())
        xs[t] = x[t]          # "feature t found"
        t += 1
        continuation.append(0)
    return torch.stack(params), continuation[:t], vecs[final_src]
