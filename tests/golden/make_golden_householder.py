#!/usr/bin/env python3
"""Golden vectors of the Householder-based layers and NaiveLinear: the REAL reference (bayesiains/nflows, imported
read-only as make_golden_lu.py does) run on the CPU in float32 and float64.  Run in the build container only, with the
reference checkout's directory as the argument (or in NFLOWS_REFERENCE):

    python tests/golden/make_golden_householder.py <reference checkout>

Writes, next to this script, data only:
  hh_{cls}_d{D}_k{K}_{kind}_{part}.npz   cls = seq (HouseholderSequence), svd (SVDLinear), qr (QRLinear); (D, K) of CASES;
                      kind = "rand" or "trained" (make_layer below); part = params (the state dict as p/<name>, the
                      log-determinants, the parameter gradients), fwd, inv (outputs of the two directions, the inverse at
                      the float32 forward output), gradf, gradi (input gradients of the two)
  hh_init.npz         the reference's initial q_vectors for (6, 3), (4, 1), (8, 8)
  naive_linear_d{D}_{part}.npz   NaiveLinear, D = 5 and 64; part = params, fwd, inv
  hh_flow.npz         [RandomPermutation, SVDLinear(16, 10), RQ coupling] x 2 + [RandomPermutation, QRLinear(16, 10), RQ coupling] x 2
Every file is kept below 1 MiB, so: the split above, the row counts of make_golden_lu.py, inputs regenerated from their
seeds (`case_inputs`, numpy's RandomState stream is frozen) and every float64 result stored as the float32 result plus a
float32 difference (`*_d`).  The gradients are those of sum(y * r) + sum(logabsdet).
"""
import copy
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["NFLOWS_REFERENCE"]
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "_refshim"))
sys.path.insert(0, REF)

import torch  # noqa: E402

from nflows.distributions.normal import StandardNormal  # noqa: E402
from nflows.flows.base import Flow  # noqa: E402
from nflows.nn.nets import ResidualNet  # noqa: E402
from nflows.transforms.base import CompositeTransform  # noqa: E402
from nflows.transforms.coupling import PiecewiseRationalQuadraticCouplingTransform  # noqa: E402
from nflows.transforms.linear import NaiveLinear  # noqa: E402
from nflows.transforms.orthogonal import HouseholderSequence  # noqa: E402
from nflows.transforms.permutations import RandomPermutation  # noqa: E402
from nflows.transforms.qr import QRLinear  # noqa: E402
from nflows.transforms.svd import SVDLinear  # noqa: E402
from nflows.utils.torchutils import create_alternating_binary_mask  # noqa: E402

torch.set_num_threads(1)
warnings.filterwarnings("ignore")

ROWS = {2: 4096, 5: 4096, 16: 2048, 64: 1280, 100: 800, 128: 640}
CASES = {
    "seq": [(2, 1), (5, 3), (64, 10), (100, 100), (128, 128), (16, 128)],
    "svd": [(2, 2), (5, 4), (64, 10), (100, 100), (128, 128)],
    "qr": [(2, 1), (5, 3), (64, 10), (128, 128)],
}
CLS_ID = {"seq": 1, "svd": 2, "qr": 3, "naive": 4}
KINDS = ("rand", "trained")


def case_seed(cls, features, count, kind):
    return ((CLS_ID[cls] * 1000 + features) * 1000 + count) * 2 + (0 if kind == "rand" else 1)


def case_inputs(cls, features, count, kind):
    """Inputs and the fixed weights r of the gradient's loss; the tests regenerate them from the same seeds."""
    rng = np.random.RandomState(case_seed(cls, features, count, kind))
    x = rng.randn(ROWS[features], features).astype(np.float32)
    r = rng.randn(ROWS[features], features).astype(np.float32)
    return x, r


def make_layer(cls, features, count, kind):
    """rand: q_vectors standard normal, the other parameters uniform as identity_init=False gives them, a normal bias.
    trained: the identity initialisation perturbed -- 0.1 randn on q_vectors, 0.5 randn on the diagonal logits, a
    normal bias (QRLinear has no identity initialisation: its own uniform one)."""
    torch.manual_seed(case_seed(cls, features, count, kind) + 17)
    if cls == "seq":
        t = HouseholderSequence(features, count)
    elif cls == "svd":
        t = SVDLinear(features, count, identity_init=(kind == "trained"))
    else:
        t = QRLinear(features, count)
    with torch.no_grad():
        for name, p in t.named_parameters():
            if name.endswith("q_vectors"):
                if kind == "rand":
                    p.normal_()
                else:
                    p.add_(0.1 * torch.randn_like(p))
            elif name == "unconstrained_diagonal" and kind == "trained":
                p.add_(0.5 * torch.randn_like(p))
            elif name == "bias":
                p.normal_()
    return t


def pair(out, name, v32, v64):
    v32 = v32.detach().numpy()
    out[name] = v32
    out[name + "_d"] = (v64.detach().numpy() - v32.astype(np.float64)).astype(np.float32)


def layer_case(out, t, x, r, cached):
    t64 = copy.deepcopy(t).double()
    names = [n for n, _ in t.named_parameters()]
    for n, v in t.state_dict().items():
        out["p/" + n] = v.numpy().copy()
    with torch.no_grad():
        y, lad = t(x)
        y64, lad64 = t64(x.double())
        pair(out, "y", y, y64)
        pair(out, "lad", lad[:1], lad64[:1])
        xi, ladi = t.inverse(y)               # the inverse's input: the float32 forward output stored above
        xi64, ladi64 = t64.inverse(y.double())
        pair(out, "xi", xi, xi64)
        pair(out, "ladi", ladi[:1], ladi64[:1])
        if cached:
            te = copy.deepcopy(t).eval()
            te.use_cache(True)
            yc, ladc = te(x)
            xic, ladic = te.inverse(y)
            out["y_cached"], out["lad_cached"] = yc.numpy(), ladc[:1].numpy()
            out["xi_cached"], out["ladi_cached"] = xic.numpy(), ladic[:1].numpy()
    for direction, source in (("grad/", x), ("gradinv/", y)):   # forward: loss of (y, lad) at x; inverse: of (x, ladi) at y
        grads = []
        for layer, dt in ((t, torch.float32), (t64, torch.float64)):
            layer.zero_grad()
            xin = source.detach().clone().to(dt).requires_grad_(True)
            yy, ll = layer(xin) if direction == "grad/" else layer.inverse(xin)
            ((yy * r.to(dt)).sum() + ll.sum()).backward()
            params = dict(layer.named_parameters())
            grads.append([xin.grad] + [params[n].grad.clone() for n in names])
        for n, g32, g64 in zip(["inputs"] + names, *grads):
            pair(out, direction + n, g32, g64)


def part_of(key):
    for stem, part in (("grad/inputs", "gradf"), ("gradinv/inputs", "gradi"), ("y", "fwd"), ("xi", "inv")):
        if key in (stem, stem + "_d", stem + "_cached"):
            return part
    return "params"


def save(path, out):
    np.savez(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def make_flow(features=16, hidden=32, count=10):
    torch.manual_seed(24)
    ts = []
    for i in range(4):
        ts.append(RandomPermutation(features))
        ts.append(SVDLinear(features, count, identity_init=True) if i < 2 else QRLinear(features, count))
        ts.append(PiecewiseRationalQuadraticCouplingTransform(
            mask=create_alternating_binary_mask(features, even=(i % 2 == 0)),
            transform_net_create_fn=lambda i_, o_: ResidualNet(i_, o_, hidden_features=hidden, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=3.0))
    flow = Flow(CompositeTransform(ts), StandardNormal([features]))
    with torch.no_grad():
        for name, p in flow.named_parameters():   # default init gives near-identity splines and identity SVD layers
            if "final_layer" in name:
                p.mul_(4.0)
            elif "linear_layers.1" in name:
                p.mul_(30.0)
            elif name.endswith("q_vectors"):
                p.add_(0.1 * torch.randn_like(p))
            elif name.endswith("unconstrained_diagonal"):
                p.add_(0.5 * torch.randn(features))
            elif name.endswith("bias") and p.shape == (features,) and "transform_net" not in name:
                p.normal_()
    return flow


def flow_case(out, rows=512):
    flow = make_flow().eval()
    flow64 = copy.deepcopy(flow).double()
    for k, v in flow.state_dict().items():
        out["state/" + k] = v.numpy().copy()
    x = torch.from_numpy(np.random.RandomState(78).randn(rows, 16).astype(np.float32))
    out["x"] = x.numpy()
    with torch.no_grad():
        pair(out, "log_prob", flow.log_prob(x), flow64.log_prob(x.double()))
        z, lad = flow._transform(x)
        z64, lad64 = flow64._transform(x.double())
        pair(out, "z", z, z64)
        pair(out, "lad", lad, lad64)
        xs, ladi = flow._transform.inverse(z)      # the sample side: noise -> data, from the float32 z stored above
        xs64, ladi64 = flow64._transform.inverse(z.double())
        pair(out, "x_from_z", xs, xs64)
        pair(out, "ladi", ladi, ladi64)


def main():
    for cls in ("seq", "svd", "qr"):
        for features, count in CASES[cls]:
            for kind in KINDS:
                out = {}
                xn, rn = case_inputs(cls, features, count, kind)
                layer_case(out, make_layer(cls, features, count, kind), torch.from_numpy(xn), torch.from_numpy(rn),
                           cached=(cls != "seq"))
                for part in ("params", "fwd", "inv", "gradf", "gradi"):
                    save(os.path.join(HERE, "hh_%s_d%d_k%d_%s_%s.npz" % (cls, features, count, kind, part)),
                         {k: v for k, v in out.items() if part_of(k) == part})
    save(os.path.join(HERE, "hh_init.npz"),
         {"q_%d_%d" % fk: HouseholderSequence(*fk).q_vectors.detach().numpy() for fk in ((6, 3), (4, 1), (8, 8))})
    for features in (5, 64):
        torch.manual_seed(case_seed("naive", features, 0, "trained") + 17)
        t = NaiveLinear(features)
        with torch.no_grad():
            t._weight.add_(0.1 * torch.randn(features, features))
            t.bias.normal_()
        out = {}
        xn, rn = case_inputs("naive", features, 0, "trained")
        layer_case(out, t, torch.from_numpy(xn), torch.from_numpy(rn), cached=True)
        for part in ("params", "fwd", "inv"):   # (no gradients: the layer runs on stock ops, its autograd is the library's)
            save(os.path.join(HERE, "naive_linear_d%d_%s.npz" % (features, part)),
                 {k: v for k, v in out.items() if part_of(k) == part and not k.startswith("grad")})
    out = {}
    flow_case(out)
    save(os.path.join(HERE, "hh_flow.npz"), out)


if __name__ == "__main__":
    main()
