"""K32 (csrc/rqs_resnet_wide_kernel.hpp) under the exact-logit oracle of tests/test_gpu_exact_logits.py: every one of its
30 instances, element by element against float64 on logits known bit for bit.

The conditioners are exact_logits' recipes (tests/wide_exact_cases.py lists the cases and what each reaches): the dyadic
recipe at 256 hidden units (1 / sqrt(256) = 1 / 16 is folded into the final layer exactly), its folded-scale form at 129,
160 and 192 (the SCALED width / height rows are dyadic; the oracle takes the scaled logits with a divisor of 1), and the
long-mantissa recipe (every product has a factor with all three bf16 pieces in use).  Inputs as in that suite: on knots
and one ulp beside them, at +-B and one ulp inside / outside, +-1e30, +-0, rows wholly outside the box; every regime of
exact_logits.REGIMES.  ROWS distinct rows are repeated to the smallest multiple above 64 x the CU count, so that every CU
takes a second row block of the persistent loop; every copy must equal the first bit for bit.

Per case, forward, inverse and log_prob: the label k32::rqs_resnet_wide_kernel<inverse=?, K=?, tiles=Hp / 32>; a clean
status word (but for the documented negative-discriminant report); identity columns and outside-box elements bit-equal
to the input; rows wholly outside the box: log-determinant exactly 0; per element helpers.assert_fp32_parity with the
conditioning allowance; per row assert_row_allowance (bulk 0.995) and assert_error_ratio; rows_ok >= 0.95.  K32 evaluates
the spline with the `k8` engine's rqs_eval and is held to THAT engine's rule: the forward ratio asserted, none of the
FusedSteps relaxations.  Measured on the device: all 29 cases pass.  The transformed inputs of a
case must keep the REFERENCE's own third-worst row off a cliff of its error tail (wide_exact_cases.reference_tail_covered,
asserted on the host; DESIGN.md section 4, "K32 / K33: how they are tested" has the element that showed why).

K32 has no twin that shows its logits.  The premise -- the logits are the host's exact ones -- rests on
`test_hidden_gemms_give_the_exact_values`: K33's forward kernel (csrc/resnet_train_wide.hip) shares K32's hidden-GEMM code
(load_frag, kstep, gemm_exchange, exchange_store) and returns every intermediate."""
import copy

import numpy as np
import pytest
import torch

import exact_logits as X
import wide_exact_cases as W
from helpers import error_stats
from test_gpu_exact_logits import ROWS, _copies
from test_gpu_headline_parity import _report
from test_gpu_steep import _status

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def the_kernel_itself_whatever_the_size_rule(monkeypatch):
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ
    monkeypatch.setattr(RQ, "fuse_wide_min_rows", 0)


def _batch_rows():
    """the smallest multiple of ROWS above 64 x the CU count: every CU takes a second 64-row block"""
    return (64 * torch.cuda.get_device_properties(0).multi_processor_count // ROWS + 1) * ROWS


@pytest.mark.parametrize("name", [c[0] for c in W.K32_CASES])
def test_k32_spline_on_exact_logits(name):
    from nflows_amd import ops
    _, hidden, D, K, more = W.K32_BY_NAME[name]
    case = W.k32_case(name)
    rows = _batch_rows()
    flow = copy.deepcopy(case["flow"]).to(DEV)
    _status(name, clear=True)
    with torch.no_grad():
        x = torch.from_numpy(case["fwd"][4]).repeat(rows // ROWS, 1).to(DEV)
        z, lad = flow._transform(x)
        label_f = ops.last_layer_kernel()
        lp = flow.log_prob(x)
        y = torch.from_numpy(case["inv"][4]).repeat(rows // ROWS, 1).to(DEV)
        xi, ladi = flow._transform.inverse(y)
        label_i = ops.last_layer_kernel()
    tiles = (hidden + 31) // 32
    assert label_f == "k32::rqs_resnet_wide_kernel<inverse=0, K=%d, tiles=%d>" % (K, tiles), label_f
    assert label_i == "k32::rqs_resnet_wide_kernel<inverse=1, K=%d, tiles=%d>" % (K, tiles), label_i
    z, lad, lp, xi, ladi = (_copies(t, rows) for t in (z, lad, lp, xi, ladi))
    xi = xi[:, case["perm"]]        # (the flow's inverse output in the coordinates of the layer under test)
    W.check_k32("k32 " + name, case, K, {"z": z, "lad": lad, "lp": lp, "x": xi, "ladi": ladi})
    _status(name)
    figures = {}
    for direction, got in (("fwd", lad), ("inv", ladi)):     # kernel / yardstick per row: what DESIGN.md's table quotes
        o = case[direction][3]
        fin = np.isfinite(o["row32"]) & np.isfinite(o["row64"]) & np.isfinite(got)
        e, e_ref = (error_stats(np.abs(v[fin].astype(np.float64) - o["row64"][fin])) for v in (got, o["row32"]))
        figures[direction] = {k: e[k] / e_ref[k] for k in ("mean", "q999", "max")}
    _report({"config": "k32 " + name, "kernels": [label_f, label_i], "rows": rows, "row_error_ratios": figures})


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd_rows", "inv_rows"])
@pytest.mark.parametrize("name", [c[0] for c in W.K32_CASES])
def test_hidden_gemms_give_the_exact_values(name, inverse):
    """The premise of the cases above, as far as it can be shown: K33's forward kernel on the case's conditioner and
    identity rows (the forward direction's draw and the inverse direction's) returns `hidden`, every `saved` plane and
    `params` equal to exact_logits' values as numbers, pad columns exactly zero.  The packed parameters are the net's own (K33 folds no scale); at the folded-scale widths the final layer
    handed to the packer is the scaled fp32 one K32 holds (`scaled_final`), so that `params` are the exact scaled logits.
    ESTABLISHES: the hidden GEMM code K32 shares with K33 (fragment loads, k-steps, the exchange through LDS, the three
    bf16 pieces of both operands) gives the exact hidden values at every width, block count and recipe of the matrix.
    DOES NOT establish: K32's own packer (`pack_resnet_conditioner_wide`, its row order and folded scale), its own final
    Linear and its lane -> feature mapping of the logits -- those are covered by the spline oracle alone, which wrong
    logits would leave by orders of magnitude."""
    from nflows_amd import ops
    _status(name, clear=True)       # (whatever a failed case left in the status word)
    net, ident, K, fold = W.k32_conditioner(name, inverse)
    H, nb, di = net.hidden_features, len(net.blocks), ident.shape[1]
    final = X.scaled_final(net, K, "linear") if fold else None
    want = X.exact_forward(net, ident, final=final)
    dev = copy.deepcopy(net).to(DEV)
    blocks = [(b.linear_layers[0].weight, b.linear_layers[0].bias, b.linear_layers[1].weight, b.linear_layers[1].bias)
              for b in dev.blocks]
    wf, bf = (dev.final_layer.weight, dev.final_layer.bias) if final is None else (
        torch.from_numpy(final[0]).float().to(DEV), torch.from_numpy(final[1]).float().to(DEV))
    pad = -wf.shape[0] % 4      # (K33 takes `out` in multiples of four: zero rows behind 31 features' 713 logits)
    wf, bf = torch.nn.functional.pad(wf, (0, 0, 0, pad)), torch.nn.functional.pad(bf, (0, pad))
    fwd_w, bias, _ = ops.pack_resnet_wide_train(dev.initial_layer.weight, dev.initial_layer.bias, blocks, (wf, bf))
    x = torch.nn.functional.pad(torch.from_numpy(ident).float(), (0, -di % 4)).to(DEV)
    hidden, saved, params = ops.resnet_wide_forward(x, fwd_w, bias, H, nb, wf.shape[0])
    ops.check_status()
    got = {"hidden": hidden, "saved": list(saved), "params": params}
    for key in ("hidden", "saved"):
        for j, plane in enumerate(got[key] if key == "saved" else [got[key]]):
            assert not plane[:, H:].any(), "%s %s[%d]: pad columns" % (name, key, j)
    got = {"hidden": hidden[:, :H].cpu().numpy(), "saved": [s[:, :H].cpu().numpy() for s in saved],
           "params": params[:, :wf.shape[0] - pad].cpu().numpy()}
    assert not params[:, wf.shape[0] - pad:].any(), name + " params: pad columns"
    W.assert_equal_as_numbers(got, {k: want[k] for k in got}, name)
