"""The cases of tests/golden/make_golden_householder.py as the host and the GPU tests of K24 share them: the fixture
loader, the generator's inputs from the same seeds, the layers with the fixture's parameters."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = {2: 4096, 5: 4096, 16: 2048, 64: 1280, 100: 800, 128: 640}
CASES = {
    "seq": [(2, 1), (5, 3), (64, 10), (100, 100), (128, 128), (16, 128)],
    "svd": [(2, 2), (5, 4), (64, 10), (100, 100), (128, 128)],
    "qr": [(2, 1), (5, 3), (64, 10), (128, 128)],
}
ALL_CASES = [(cls, f, k) for cls in ("seq", "svd", "qr") for f, k in CASES[cls]]
LINEAR_CASES = [c for c in ALL_CASES if c[0] != "seq"]
CLS_ID = {"seq": 1, "svd": 2, "qr": 3, "naive": 4}
KINDS = ("rand", "trained")
_cache = {}


def case_id(case):
    return "%s-%dx%d" % case


def golden(cls, features, count, kind):
    """All parts of one case, merged; loaded once and shared (read-only) among the tests."""
    key = (cls, features, count, kind)
    if key not in _cache:
        merged = {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, "hh_%s_d%d_k%d_%s_*.npz" % key))):
            with np.load(path) as z:
                merged.update({k: z[k] for k in z.files})
        assert merged, "no fixture for %s" % (key,)
        for v in merged.values():
            v.setflags(write=False)
        _cache[key] = merged
    return _cache[key]


def naive_golden(features):
    merged = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "naive_linear_d%d_*.npz" % features))):
        with np.load(path) as z:
            merged.update({k: z[k] for k in z.files})
    assert merged
    return merged


def case_inputs(cls, features, count, kind):
    """The generator's inputs and loss weights, from the same seeds."""
    seed = ((CLS_ID[cls] * 1000 + features) * 1000 + count) * 2 + (0 if kind == "rand" else 1)
    rng = np.random.RandomState(seed)
    x = rng.randn(ROWS[features], features).astype(np.float32)
    r = rng.randn(ROWS[features], features).astype(np.float32)
    return x, r


def truth(g, name):
    return g[name].astype(np.float64) + g[name + "_d"].astype(np.float64)


def state_of(g):
    return {k[2:]: torch.from_numpy(np.array(g[k])) for k in g if k.startswith("p/")}


def new_layer(cls, features, count, **kw):
    from nflows_amd.transforms import HouseholderSequence, QRLinear, SVDLinear
    return {"seq": HouseholderSequence, "svd": SVDLinear, "qr": QRLinear}[cls](features, count, **kw)


def layer_of(g, cls, features, count, **kw):
    t = new_layer(cls, features, count, **kw)
    t.load_state_dict(state_of(g), strict=True)
    return t
