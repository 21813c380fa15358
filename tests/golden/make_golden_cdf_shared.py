#!/usr/bin/env python3
"""Golden vectors and gradients of the four batch-shared CDF transforms -- PiecewiseLinearCDF, PiecewiseQuadraticCDF,
PiecewiseCubicCDF, PiecewiseRationalQuadraticCDF (nflows/transforms/nonlinearities.py:230-467): the REAL reference
(bayesiains/nflows, imported read-only as make_golden_nonlin.py does; its checkout is named by the environment variable
NFLOWS_REFERENCE) run on the CPU in float32 and float64.  Run in the build container only:

    NFLOWS_REFERENCE=<checkout of bayesiains/nflows> python tests/golden/make_golden_cdf_shared.py

Writes tests/golden/cdf_shared.npz, data only:
  meta                        rows (name, kind, keyword arguments of the class): kind in linear, quadratic, cubic, rq; tails
                              None and "linear" (tail_bound 3); shapes [2, 3, 4] and [37]; K = 8; batch 64
  x/{tails}_{shape}           the inputs [64, *shape], shared by the four kinds and by both directions: uniform over the box,
  Wy/.., Wl/..                linear tails one element in twenty outside it; the weights of the loss
                                  L = sum(Wy * y) + sum(Wl * logabsdet)
  {name}/p/{parameter}        the class's parameters, 1.5 x standard normal from a seeded generator (`parameter_seeds`, in the
                              order of `meta`: see "Seeds" below for how a seed is chosen)
  {name}/{,inv_}y, lad        outputs and logabsdet [64] of forward / inverse in float32
  {name}/{,inv_}gx            dL/dx; {name}/{,inv_}g/{parameter}: dL/dparameter (a sum over the batch through autograd's
                              expand), float32
  ..._d                       next to every result v: (float64 result minus float32 result) / s as float16, s a power of two
  scale_keys, scale_values    that puts the largest difference near 2^14 (one s per result, listed under its key) -- the
                              float64 result is v + s * d in float64, known to within 2^-11 of the float32 result's own
                              error, which is what a yardstick needs; the differences in float32 would put the file above
                              the repository's limit for one file
Every float32 and float64 result written is finite (asserted), and the worst float32 errors per kind are printed.
"""
import copy
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "_refshim"))
sys.path.insert(0, os.environ["NFLOWS_REFERENCE"])

import torch  # noqa: E402

from nflows.transforms import nonlinearities as ref  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

KINDS = {"linear": ref.PiecewiseLinearCDF, "quadratic": ref.PiecewiseQuadraticCDF, "cubic": ref.PiecewiseCubicCDF,
         "rq": ref.PiecewiseRationalQuadraticCDF}
SHAPES = ((2, 3, 4), (37,))
K, BATCH, TAIL_BOUND, SCALE = 8, 64, 3.0, 1.5


def tag(tails, shape):
    return "%s_%s" % ("tails" if tails else "box", "x".join(str(s) for s in shape))


def shared_inputs(tails, shape, seed):
    rng = np.random.RandomState(seed)
    n = BATCH * int(np.prod(shape))
    if tails is None:
        x = rng.rand(n)
    else:
        x = TAIL_BOUND * (2.0 * rng.rand(n) - 1.0)
        out = rng.permutation(n)[:n // 20]
        x[out] = np.where(rng.rand(out.size) < 0.5, -1.0, 1.0) * TAIL_BOUND * (1.0 + rng.rand(out.size) + 1e-3)
    return (x.astype(np.float32).reshape((BATCH,) + shape), rng.randn(BATCH, *shape).astype(np.float32),
            rng.randn(BATCH).astype(np.float32))


def pair(out, worst, name, v32, v64):
    v32, v64 = v32.detach().numpy(), v64.detach().numpy()
    assert np.isfinite(v32).all() and np.isfinite(v64).all(), name
    out[name] = v32
    d = v64 - v32.astype(np.float64)
    s = 2.0 ** (np.ceil(np.log2(max(float(np.abs(d).max()), 1e-300))) - 14)
    out[name + "_d"] = (d / s).astype(np.float16)
    out.setdefault("scales", {})[name] = s
    assert np.isfinite(out[name + "_d"]).all()
    key = name.split("/", 1)[1].replace("inv_", "").split("/")[0]
    worst[key] = max(worst.get(key, 0.0), float(np.abs(v64 - v32).max()))
    worst[key + " scale"] = max(worst.get(key + " scale", 0.0), float(np.abs(v64).max()))


# Seeds: inputs per (tails, shape), parameters per (kind, tails, shape): the first of the pattern's seed plus 0, 1000,
# 2000, ... whose draw meets the conditions below (`main` searches, prints and stores the seed it took).  They are
# conditions on the INPUTS, to be met by the reference alone, so that a comparison with it says something:
#   * no NaN in either direction, float32 or float64;
#   * on [2, 3, 4]: fp32 against fp64 at most 1.8e-5 in y and 3.9e-4 in logabsdet, parameter gradients within 0.32 on
#     a scale of at most 1.6e3 (`LIMITS`; tests/test_cdf_shared_host.py holds the file to them).  A draw with a bin of
#     nearly minimal width next to a steep one puts the reference's own fp32 off by more;
#   * every gradient, both directions: moving x and the parameters by half an fp32 ulp (three draws, as
#     tests/helpers.py's `conditioning` does) moves the float64 gradient by at most a quarter (`CONDITION_SHARE`) of the
#     bound it is tested under, 4 x the reference-fp32's own error + 2e-5 x scale (`helpers.close_to_truth`).  An fp32
#     evaluation inherits that movement from the rounding of its inputs alone and adds roundings of its own of the same
#     size; where the movement is of the size of the bound the bound measures the draw, not the evaluation.  (The
#     pattern's first draws had it at 0.7 x the bound for the rational-quadratic inverse on [2, 3, 4], 1.4 x with tails,
#     and 3.7 x for the cubic inverse with tails.)
INPUT_SEED = 9700
LIMITS = {"y": 1.8e-5, "lad": 3.9e-4, "g": 0.32, "g scale": 1.6e3}
CONDITION_SHARE = 0.25


def parameter_seed(kind, tails, shape):
    return 97000 + 100 * list(KINDS).index(kind) + 10 * (tails is not None) + SHAPES.index(shape)


def loss_gradients(layer, xn, wy, wl, inverse, dt):
    layer.zero_grad()
    x = torch.from_numpy(xn).to(dt).requires_grad_(True)
    y, lad = layer.inverse(x) if inverse else layer(x)
    assert lad.shape == (BATCH,)
    ((torch.from_numpy(wy).to(dt) * y).sum() + (torch.from_numpy(wl).to(dt) * lad).sum()).backward()
    return dict(y=y, lad=lad, gx=x.grad, **dict(("g/" + pn, p.grad.clone()) for pn, p in layer.named_parameters()))


def gradient_movement(layer64, xn, wy, wl, inverse, base, seed):
    """Per gradient: the largest change of the float64 result when x and the parameters move by half an fp32 ulp."""
    rng = np.random.RandomState(seed)
    worst = dict((k, 0.0) for k in base if k.startswith("g"))
    for _ in range(3):
        moved = copy.deepcopy(layer64)
        with torch.no_grad():
            for p in moved.parameters():
                p.mul_(torch.from_numpy(1.0 + (rng.randint(0, 2, size=tuple(p.shape)) * 2 - 1) * 2.0 ** -24))
        xm = xn.astype(np.float64) * (1.0 + (rng.randint(0, 2, size=xn.shape) * 2 - 1) * 2.0 ** -24)
        got = loss_gradients(moved, xm, wy, wl, inverse, torch.float64)
        for k in worst:
            d = (got[k] - base[k]).abs().max().item()
            worst[k] = max(worst[k], d if np.isfinite(d) else np.inf)
    return worst


def case(kind, tails, shape, xn, wy, wl, seed):
    """(arrays, worst) of one class: parameters from `seed`, both directions, float32 and float64."""
    name = "%s_%s" % (kind, tag(tails, shape))
    kw = dict(shape=list(shape), num_bins=K, tails=tails, tail_bound=TAIL_BOUND if tails else 1.0)
    layer = KINDS[kind](**kw)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(SCALE * torch.randn(p.shape, generator=gen))
    layer64 = copy.deepcopy(layer).double()
    out, worst = {}, {}
    for pn, p in layer.named_parameters():
        out["%s/p/%s" % (name, pn)] = p.detach().numpy().copy()
    for inverse in (False, True):
        pre = name + ("/inv_" if inverse else "/")
        res = [loss_gradients(lay, xn, wy, wl, inverse, dt) for lay, dt in ((layer, torch.float32), (layer64, torch.float64))]
        for k in res[0]:
            pair(out, worst, pre + k, res[0][k], res[1][k])
        for k, moved in gradient_movement(layer64, xn, wy, wl, inverse, res[1], seed + int(inverse)).items():
            bound = 4.0 * (res[0][k].double() - res[1][k]).abs().max().item() + 2e-5 * (1.0 + res[1][k].abs().max().item())
            worst["movement / bound"] = max(worst.get("movement / bound", 0.0), moved / bound)
    return name, kw, out, worst


def within_limits(worst, shape):
    return worst["movement / bound"] <= CONDITION_SHARE and (shape != (2, 3, 4) or all(worst[k] <= v for k, v in LIMITS.items()))


def main():
    out, meta, seeds = {}, [], []
    for ti, tails in enumerate((None, "linear")):
        for si, shape in enumerate(SHAPES):
            xn, wy, wl = shared_inputs(tails, shape, INPUT_SEED + 2 * ti + si)
            t_ = tag(tails, shape)
            out["x/" + t_], out["Wy/" + t_], out["Wl/" + t_] = xn, wy, wl
            for kind in KINDS:
                for attempt in range(200):
                    seed = parameter_seed(kind, tails, shape) + 1000 * attempt
                    try:
                        name, kw, arrays, worst = case(kind, tails, shape, xn, wy, wl, seed)
                    except AssertionError:      # (a NaN of the reference's: `pair`)
                        continue
                    if within_limits(worst, shape):
                        break
                else:
                    raise RuntimeError("no draw meets the conditions: %s %s %s" % (kind, tails, shape))
                scales = arrays.pop("scales")
                out.setdefault("scales", {}).update(scales)
                out.update(arrays)
                meta.append((name, kind, repr(kw)))
                seeds.append(seed)
                print(name, "seed", seed, "  ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    out["meta"] = np.array(meta)
    out["parameter_seeds"] = np.array(seeds, dtype=np.int64)
    scales = out.pop("scales")
    out["scale_keys"], out["scale_values"] = np.array(list(scales)), np.array(list(scales.values()), dtype=np.float64)
    path = os.path.join(HERE, "cdf_shared.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
