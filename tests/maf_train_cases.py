"""Shared cases of the K25 tests (MAF layers under autograd on K14 / K10, tests/test_made_train_host.py and
tests/test_gpu_maf_train.py): the gradient fixture of tests/golden/make_golden_maf_grads.py, the nets the gate of
`MADE._fusable` has to accept and refuse, and float64 truths written in tensor operations."""
import glob
import os

import numpy as np
import torch
from torch.nn import functional as F

import maf_cases

# case of maf_cases.CASES -> the number of layers whose gradients the fixture holds (None: the case's own).  One
# 128-wide layer's gradients are about half a megabyte in fp32 + fp64, so d36_random_perm keeps two of its four layers.
GRAD_CASES = {"d8_h32_reverse": None, "d36_random_perm": 2, "d6_l5": None}


def grad_case_config(name):
    cfg = dict(maf_cases.CASES[name])
    if GRAD_CASES[name] is not None:
        cfg["num_layers"] = GRAD_CASES[name]
    return cfg


def load_grads(golden_dir):
    """The index and every part file of the gradient fixture as one dict of numpy arrays."""
    index = np.load(os.path.join(golden_dir, "maf_grads.npz"))
    table = {k: index[k] for k in index.files}
    parts = sorted(glob.glob(os.path.join(golden_dir, "maf_grads.part*.npz")))
    assert len(parts) == int(index["parts"]), "maf_grads: %d part files, %d expected" % (len(parts), int(index["parts"]))
    for path in parts:
        part = np.load(path)
        table.update({k: part[k] for k in part.files})
    return table


def build_grad_flow(name, table):
    """The drop-in flow of a gradient case on the CPU in eval mode, rebuilt from its seed and held to the checksums of
    the reference's state_dict."""
    from nflows_amd import configs
    flow = configs.masked_affine_flow(**grad_case_config(name), **maf_cases.SHARPEN).eval()
    names, sums = maf_cases.checksums(flow.state_dict())
    assert [str(n) for n in table[name + "/param_names"]] == names, "state_dict keys differ from the reference's"
    want = table[name + "/param_checksums"]
    assert np.all(np.abs(sums - want) <= 1e-9 * (1 + np.abs(want))), name
    return flow


def flow_gradients(flow, x):
    """(loss, {"x": ..., parameter name: ...}) of loss = -log_prob(x).mean() through the flow's own autograd."""
    flow.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    loss = -flow.log_prob(x).mean()
    loss.backward()
    grads = {"x": x.grad.detach().clone()}
    for name, p in flow.named_parameters():
        grads[name] = p.grad.detach().clone()
    return loss.detach(), grads


# ---- the gate ----------------------------------------------------------------------------------------------------------

def made(features=8, hidden=32, blocks=2, multiplier=2, seed=0, **kw):
    from nflows_amd.transforms.made import MADE
    torch.manual_seed(seed)
    return MADE(features, hidden, num_blocks=blocks, output_multiplier=multiplier, **kw)


# (features, hidden, blocks, rows) the gate accepts: the shapes of the one-layer GPU test
ACCEPTED = [(2, 4, 2, 128), (8, 32, 2, 256), (36, 128, 3, 128), (63, 128, 1, 256), (64, 128, 2, 384)]


def refused():
    """name -> (net, rows, context or None, a context manager to enter or None): everything keeps the eager path."""
    hooked = made()
    hooked.blocks[0].linear_layers[0].register_forward_hook(lambda module, args, out: None)
    return {
        "feed-forward blocks": (made(use_residual_blocks=False), 256, None, None),
        "context": (made(context_features=3), 256, torch.randn(256, 3), None),
        "4 blocks": (made(blocks=4), 256, None, None),
        "hidden 50": (made(hidden=50), 256, None, None),
        "batch 200": (made(), 200, None, None),
        "autocast": (made(), 256, None, "autocast"),
        "an inner hook": (hooked, 256, None, None),
    }


# ---- float64 truths ----------------------------------------------------------------------------------------------------

def affine_element_truth(x, u, shift, g_y, g_l, inverse, dtype=torch.float64):
    """Autograd of y = x * (softplus(u) + 1e-3) + shift (or its inverse) with per-element log-derivative, in `dtype`:
    (g_x, g_u, g_shift) for loss = <y, g_y> + <l, g_l>, all elementwise (g_l already spread to the elements)."""
    x, u, shift = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, u, shift))
    s = F.softplus(u) + 1e-3
    if inverse:
        y, l = (x - shift) / s, -torch.log(s)
    else:
        y, l = x * s + shift, torch.log(s)
    ((y * g_y.to(dtype)).sum() + (l * g_l.to(dtype)).sum()).backward()
    return x.grad, u.grad, shift.grad


def within_truth_rule(got, ref32, truth, what, tol=2e-5):
    """helpers.close_to_truth's rule per ELEMENT: |got - truth| <= 4 |ref32 - truth| + tol (1 + max |truth|)."""
    got, ref32, truth = (np.asarray(a, dtype=np.float64) for a in (got, ref32, truth))
    allow = 4.0 * np.abs(ref32 - truth) + tol * (1.0 + np.abs(truth).max())
    err = np.abs(got - truth)
    worst = int(np.argmax(err - allow))
    assert np.all(err <= allow), "%s: element %d err %.3e, allowance %.3e" % (what, worst, err.flat[worst], allow.flat[worst])
