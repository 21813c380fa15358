#!/usr/bin/env python3
"""Golden GRADIENTS of the masked autoregressive affine flows (K25): the REAL reference's autograd, run on the CPU in
float32 and float64 through the flows make_golden_maf.py builds (its `reference_flow`: the reference's own classes,
imported read-only there).  Run in the build container only:

    python tests/golden/make_golden_maf_grads.py

For the cases of `maf_train_cases.GRAD_CASES` (tests/maf_cases.py's residual, context-free flows at their 256 rows) it
stores results only: loss = -log_prob(x).mean(), d loss / d x and d loss / d parameter for every parameter, each in
float32 (`.../g32/<name>`) and float64 (`.../g64/<name>`), and the names and checksums of the reference's state_dict
(configs.masked_affine_flow rebuilds the weights from the seed; nothing of them is stored).  The project takes no NEW committed
file above 1 MiB (the larger fixtures next to this one predate that limit) and one 128-wide layer's gradients take about
half of it, so the arrays are spread over maf_grads.npz (the index: `cases`, `parts`, the losses) and
maf_grads.partNN.npz; maf_train_cases.load_grads reads them back as one table.
"""
import glob
import os

import numpy as np

import make_golden_maf as ref_maf   # (puts the reference and tests/ on sys.path)
import torch

import maf_cases
import maf_train_cases

HERE = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 640 * 1024    # non-zero payload per file (masked-out gradients are zeros and compress away)


def gradients(flow, x):
    flow.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    loss = -flow.log_prob(x).mean()
    loss.backward()
    grads = {"x": x.grad.detach().clone()}
    for name, p in flow.named_parameters():
        grads[name] = p.grad.detach().clone()   # (flow.double() converts the parameters' .grad in place)
    return loss.detach().clone(), grads


def main():
    index, table = {}, {}
    for name in maf_train_cases.GRAD_CASES:
        cfg = maf_train_cases.grad_case_config(name)
        flow = ref_maf.reference_flow(**cfg)
        x, _ = maf_cases.fixture_inputs(name)
        names, sums = maf_cases.checksums(flow.state_dict())
        index[name + "/param_names"] = np.array(names).astype(str)
        index[name + "/param_checksums"] = sums
        loss32, g32 = gradients(flow.float(), x)
        loss64, g64 = gradients(flow.double(), x.double())
        index[name + "/loss32"], index[name + "/loss64"] = loss32.numpy(), loss64.numpy()
        worst = 0.0
        for k in g32:
            assert torch.isfinite(g32[k]).all() and torch.isfinite(g64[k]).all(), (name, k)
            assert g32[k].dtype == torch.float32 and g64[k].dtype == torch.float64
            table["%s/g32/%s" % (name, k)] = g32[k].numpy()
            table["%s/g64/%s" % (name, k)] = g64[k].numpy()
            worst = max(worst, float((g32[k].double() - g64[k]).abs().max() / (1.0 + g64[k].abs().max())))
        print("   %s: %d layers, loss %.6f, %d gradients, reference fp32 vs fp64: loss %.2e, gradients %.2e of their scale"
              % (name, cfg["num_layers"], float(loss64), len(g32), abs(float(loss32) - float(loss64)), worst))
    for old in glob.glob(os.path.join(HERE, "maf_grads.part*.npz")):
        os.remove(old)
    parts, current, used = [], {}, 0
    for key, value in table.items():
        size = int(np.count_nonzero(value)) * value.itemsize
        if current and used + size > PART_BYTES:
            parts.append(current)
            current, used = {}, 0
        current[key] = value
        used += size
    parts.append(current)
    total = 0
    for q, part in enumerate(parts):
        path = os.path.join(HERE, "maf_grads.part%02d.npz" % q)
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 1024 * 1024, path
        total += os.path.getsize(path)
    index["cases"] = np.array(list(maf_train_cases.GRAD_CASES)).astype(str)
    index["parts"] = np.array(len(parts))
    path = os.path.join(HERE, "maf_grads.npz")
    np.savez_compressed(path, **index)
    print("maf_grads: %d cases, %d part files, %d bytes" % (len(maf_train_cases.GRAD_CASES), len(parts),
                                                          total + os.path.getsize(path)))


if __name__ == "__main__":
    main()
