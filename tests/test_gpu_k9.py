"""K9 (nflows_amd/csrc/splines_lq.hip) on the GPU through the drop-in functionals: the case table and the rules of
tests/k9_cases.py / tests/helpers.py that tests/test_k9_host.py applies to the host build of the same arithmetic -- values
and logabsdet against the float64 oracle, gradients against its central differences, the real reference's vectors on and
next to the box ends --, and what only the launch code can get wrong: logit layouts, tile tails, empty batches and the
persistent loops' second pass.  Run with -s for the per-case figures.  Needs an MI355X: `-m gpu`."""
import os

import numpy as np
import pytest
import torch

import k9_cases
from helpers import assert_gradient_rows, assert_sibling_truth_parity, assert_trimmed_error_ratio, parse_kwargs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c.name for c in k9_cases.CASES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    import nflows_amd
    from nflows_amd import ops as o
    assert os.path.exists(nflows_amd.native_library_path())
    return o


def take_status(ops):
    """The status word as a number (read and cleared): 0, 1 outside the domain, 2 negative discriminant."""
    from nflows_amd import InputOutsideDomain
    try:
        ops.check_status()
    except InputOutsideDomain:
        return 1
    except AssertionError:
        return 2
    return 0


def functional(kind, kw):
    from nflows_amd.transforms import splines
    tails = kw.get("tails") == "linear"
    return {"linear": (splines.linear_spline, splines.unconstrained_linear_spline),
            "quadratic": (splines.quadratic_spline, splines.unconstrained_quadratic_spline),
            "cubic": (splines.cubic_spline, splines.unconstrained_cubic_spline)}[kind][int(tails)]


def run(kind, kw, inverse, x, logits):
    """(y, lad) as device tensors; x / logits device tensors (any layout)."""
    return functional(kind, kw)(x, *logits, inverse=inverse, **kw)


def table_case(kind, K, inverse):
    return next(c for c in k9_cases.CASES if c.kind == kind and c.K == K and c.inverse == inverse)


# ------------------------------------------------------------------------------------------------- values, logabsdet
@pytest.mark.parametrize("name", NAMES)
def test_table_values(ops, name):
    """Every case of the table under `assert_sibling_truth_parity` at the kernels' share of 99.9 %.
    Measured on an MI355X: worst share 0.99923 (cubic inverse, K = 3, scale 3), trimmed-mean ratios 0.56 - 1.75, quantile
    ratios 0.08 - 1.89.  (With the reference's form of the inverse quadratic root, (-qb + r) / (2 qa), the kernels left 4 of
    the 3892 elements of quadratic_k10m1_inv_tails_s3 outside where the share admits 3 -- elements where that form
    cancels in a flat bin; `quadratic_inverse_root` in splines_lq.hip now evaluates the same root without the
    cancellation, and every quadratic inverse case has a share of 1.)"""
    case, p = k9_cases.BY_NAME[name], k9_cases.prepared(name)
    y, lad = run(case.kind, k9_cases.spec_kwargs(case), case.inverse, dev(p["x"]), [dev(a) for a in p["logits"]])
    status = take_status(ops)
    assert y.shape == (k9_cases.ROWS,) and lad.shape == (k9_cases.ROWS,)
    assert_sibling_truth_parity((host(y), host(lad)), p["ref"][:2], p["truth"], p["cond"], p["x"], status, case.inverse,
                                None if case.box else k9_cases.TAIL_BOUND, bulk=k9_cases.SHARE, what=name, verbose=True)


def test_box_edges_against_the_reference(ops, golden_dir):
    """tests/golden/splines_lq_edges.npz (the real reference on and next to the ends of the box): conditions 1 - 3 per
    case at a share of 99.5 %, condition 4 on the four cases of a kind and direction together, as on the host build."""
    g = np.load(os.path.join(golden_dir, "splines_lq_edges.npz"))
    pool = {}
    for name, kind, kw in g["meta"]:
        name, kind, kw = str(name), str(kind), parse_kwargs(kw)
        x = g[name + "/x"]
        logits = [g["%s/logits%d" % (name, i)] for i in range({"linear": 1, "quadratic": 2, "cubic": 4}[kind])]
        for inverse in (False, True):
            pre = name + ("/inv_" if inverse else "/")
            y, lad = run(kind, kw, inverse, dev(x), [dev(a) for a in logits])
            status = take_status(ops)
            cond = k9_cases.value_truth(kind, logits[0].shape[1], kw, x, logits, inverse)["cond"]
            fig = assert_sibling_truth_parity((host(y), host(lad)), (g[pre + "y"], g[pre + "lad"]), (g[pre + "y64"], g[pre + "lad64"]),
                                              cond, x, status, inverse, kw.get("tail_bound"), bulk=k9_cases.EDGE_SHARE,
                                              what="edges " + name + (" inverse" if inverse else ""), verbose=True, ratios=False)
            for nm in ("y", "lad"):
                pool.setdefault((kind, "inverse" if inverse else "forward", nm), []).append(fig[nm]["errors"])
    assert len(pool) == 12
    for key in sorted(pool):
        e_got, e_ref, mag = (np.concatenate(v) for v in zip(*pool[key]))
        assert_trimmed_error_ratio(e_got, e_ref, mag, what="edges pooled %s %s %s" % key, verbose=True)


def test_box_inputs_outside_raise(ops):
    from nflows_amd import InputOutsideDomain
    for kind in ("linear", "quadratic", "cubic"):
        for inverse in (False, True):
            x = torch.tensor([0.25, 1.0 + 1e-6, 0.75], device=DEV)
            logits = [torch.zeros(3, w, device=DEV) for w in k9_cases.logit_widths(kind, 8, 9)]
            with pytest.raises(InputOutsideDomain):
                run(kind, {}, inverse, x, logits)
    assert take_status(ops) == 0


# ------------------------------------------------------------------------------------------------------- gradients
def autograd_gradients(kind, kw, inverse, x, logits, wy, wl, poison=None):
    """[gx, g_logits..] through autograd on the functional.  `poison`: the gradient buffers come from torch.empty; blocks
    of their sizes are filled with this value and handed back to the caching allocator right before the backward pass,
    so that an element the kernel does not write most likely holds it (two runs with two values then differ there)."""
    x = dev(x).requires_grad_(True)
    logits = [dev(a).requires_grad_(True) for a in logits]
    y, lad = run(kind, kw, inverse, x, logits)
    loss = (y * dev(wy)).sum() + (lad * dev(wl)).sum()
    if poison is not None:
        junk = [torch.full_like(t, poison) for t in [x] + logits for _ in range(3)]
        del junk
    loss.backward()
    return [x.grad] + [a.grad for a in logits]


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("K", [8, 40])
@pytest.mark.parametrize("kind", ["linear", "quadratic", "cubic"])
def test_backward_writes_every_element(ops, kind, K):
    """Two backward passes over the same 4096 elements, the allocator's free blocks filled with two different values
    before each: every gradient entry has the same bits both times -- the kernel is deterministic, and an entry it left
    unwritten (the last lane of a tile, the tail of the batch) would show the fill."""
    for inverse in (False, True):
        case = table_case(kind, K, inverse)
        x, logits = k9_cases.inputs(case)
        wy, wl = k9_cases.weights(case)
        kw = k9_cases.spec_kwargs(case)
        a = autograd_gradients(kind, kw, inverse, x, logits, wy, wl, poison=1e30)
        b = autograd_gradients(kind, kw, inverse, x, logits, wy, wl, poison=-7.0)
        for ga, gb in zip(a, b):
            assert bits_equal(ga, gb), (kind, K, inverse)
    assert take_status(ops) == 0


@pytest.mark.parametrize("name", NAMES)
def test_table_gradients(ops, name):
    case, g = k9_cases.BY_NAME[name], k9_cases.prepared_gradients(name)
    assert 1.0 - g["keep"].mean() <= k9_cases.FD_DROP_CAP
    got = autograd_gradients(case.kind, k9_cases.spec_kwargs(case), case.inverse, g["x"], g["logits"], g["wy"], g["wl"])
    assert take_status(ops) == 0
    assert_gradient_rows([host(t) for t in got], g["truth"], g["cond"], g["keep"], k9_cases.GRAD_CAP[(case.kind, case.inverse)],
                         outside=k9_cases.outside_box(case, g["x"]), gy=g["wy"], tol=k9_cases.GRAD_TOL, what=name, verbose=True)


# --------------------------------------------------------------------------------------------------- launch code
def layouts(logits):
    """The same logits as (name, tensors): dense separate tensors; views into one packed [n, P] buffer; strided views
    with unrelated columns in between and behind; a packed buffer at a storage offset of one float."""
    n = logits[0].shape[0]
    widths = [a.shape[1] for a in logits]
    P = sum(widths)
    rng = np.random.RandomState(3)

    def views(buf, gap):
        out, at = [], 0
        for w in widths:
            out.append(buf[:, at:at + w])
            at += w + gap
        return out

    yield "dense", [dev(a) for a in logits]
    packed = dev(np.concatenate(logits, axis=1))
    yield "packed", views(packed, 0)
    wide = rng.randn(n, P + 3 * len(widths) + 2).astype(np.float32)
    at = 0
    for a, w in zip(logits, widths):
        wide[:, at:at + w] = a
        at += w + 3
    yield "strided", views(dev(wide), 3)
    buf = torch.empty(n * P + 1, device=DEV)
    buf[1:] = packed.reshape(-1)
    yield "packed at an offset of one float", views(buf[1:].view(n, P), 0)


@pytest.mark.parametrize("K", [8, 10, 5])
@pytest.mark.parametrize("kind", ["linear", "quadratic", "cubic"])
def test_logit_layouts_are_bit_identical(ops, kind, K):
    """tile_load (K = 8 / 10) and the scatter path (other K) of a packed buffer, aligned or not, and the per-lane gather
    of strided rows all stage the same logits: outputs and logabsdet bit for bit, both directions, both height counts."""
    n = 3 * 256 + 77
    rng = np.random.RandomState(100 + K)
    x = dev((k9_cases.TAIL_BOUND * (2.2 * rng.rand(n) - 1.1)).astype(np.float32))
    kw = dict(tails="linear", tail_bound=k9_cases.TAIL_BOUND)
    for nh in ((K - 1, K + 1) if kind == "quadratic" else (0,)):
        box = nh == K + 1           # (K + 1 heights: the constrained functional)
        xs = dev(rng.rand(n).astype(np.float32)) if box else x
        logits = [(2.0 * rng.randn(n, w)).astype(np.float32) for w in k9_cases.logit_widths(kind, K, nh)]
        for inverse in (False, True):
            want = None
            for name, tensors in layouts(logits):
                y, lad = run(kind, {} if box else kw, inverse, xs, tensors)
                if want is None:
                    want = (y, lad)
                assert torch.equal(y, want[0]) and torch.equal(lad, want[1]), (name, nh, inverse)
    assert take_status(ops) == 0


@pytest.mark.parametrize("K", [8, 40])
def test_batch_sizes_around_a_tile(ops, K):
    """n = 0, 1, 255, 256, 257: the first n elements of a block that test_table_values holds to the float64 truth give
    the bits they give inside the block (elements are independent); n = 0 gives empty outputs and no launch error."""
    for kind, inverse, sizes in (("linear", True, (0, 1, 256)), ("quadratic", False, (0, 255, 257)), ("cubic", True, (1, 255, 257))):
        case = table_case(kind, K, inverse)
        p = k9_cases.prepared(case.name)
        kw = k9_cases.spec_kwargs(case)
        y, lad = run(kind, kw, inverse, dev(p["x"]), [dev(a) for a in p["logits"]])
        for n in sizes:
            yn, ln = run(kind, kw, inverse, dev(p["x"][:n]), [dev(a[:n]) for a in p["logits"]])
            assert yn.shape == (n,) and ln.shape == (n,)
            assert torch.equal(yn, y[:n]) and torch.equal(ln, lad[:n]), (kind, n)
    assert take_status(ops) in (0, 2)


def element_tile(floor, slot):
    """launch_plan.hpp `plan_element_tile` for a slot of `slot` floats per element and 64 KiB of dynamic LDS."""
    T = 256
    while T > floor and T * slot * 4 > 65536:
        T >>= 1
    return T


def forward_plan(kind, K):
    """(tile, workgroups per CU) of `launch_lq`."""
    slot = {"linear": K, "quadratic": 2 * K + 1, "cubic": 2 * K + 2}[kind] | 1
    T = element_tile(32, slot)
    return T, min(8, max(1, (160 * 1024) // (T * slot * 4 + 64 + 256)))


def backward_plan(kind, K):
    """(tile, workgroups per CU) of `launch_lq_backward`."""
    slot = {"linear": K, "quadratic": 5 * K + 3, "cubic": 4 * K}[kind] | 1
    return element_tile(64, slot), 8


def repeated(arrays, n):
    reps = -(-n // arrays[0].shape[0])
    return [np.concatenate([a] * reps, axis=0)[:n] for a in arrays]


def assert_repeats(t, block, what):
    """Every repetition of the block inside `t` (and the partial one at the end) equals `block` bit for bit."""
    rows = block.shape[0]
    full = t.shape[0] // rows
    assert torch.equal(t[:full * rows].view((full, rows) + tuple(t.shape[1:])), block.unsqueeze(0).expand((full, rows) + tuple(t.shape[1:]))), what
    rest = t.shape[0] - full * rows
    assert torch.equal(t[full * rows:], block[:rest]), what


@pytest.mark.parametrize("inverse", [False, True])
def test_forward_persistent_loop_wraps(ops, inverse):
    """Quadratic, K = 40: the forward grid is limited by LDS to 3 workgroups of 128 elements per CU, so CUs x 3 x 128
    elements plus three tiles and 37 make every workgroup take a second tile, some a third, the last one a partial.
    The batch repeats the 4096-element block of the table that test_table_values holds to the float64 truth."""
    T, per_cu = forward_plan("quadratic", 40)
    assert (T, per_cu) == (128, 3)
    n = torch.cuda.get_device_properties(0).multi_processor_count * per_cu * T + 3 * T + 37
    case = table_case("quadratic", 40, inverse)
    p = k9_cases.prepared(case.name)
    kw = k9_cases.spec_kwargs(case)
    y0, lad0 = run("quadratic", kw, inverse, dev(p["x"]), [dev(a) for a in p["logits"]])
    big = repeated([p["x"]] + p["logits"], n)
    y, lad = run("quadratic", kw, inverse, dev(big[0]), [dev(a) for a in big[1:]])
    assert take_status(ops) in (0, 2)
    assert_repeats(y, y0, "outputs")
    assert_repeats(lad, lad0, "logabsdet")


@pytest.mark.parametrize("inverse", [False, True])
def test_backward_persistent_loop_wraps(ops, inverse):
    """The backward grid is 8 workgroups per CU whatever the slot; quadratic K = 40 has the halved tile (64 elements) and
    with it the smallest logit and gradient tensors that make the grid-stride loop advance: CUs x 8 x 64 elements plus
    three tiles and 37, about 85 MB of logits and gradients.  Gradients of every repetition of the block that
    test_table_gradients holds to the float64 truth are bit-equal to the block's own."""
    T, per_cu = backward_plan("quadratic", 40)
    assert (T, per_cu) == (64, 8) and backward_plan("linear", 40)[0] == 256 and backward_plan("quadratic", 8)[0] == 256
    n = torch.cuda.get_device_properties(0).multi_processor_count * per_cu * T + 3 * T + 37
    case = table_case("quadratic", 40, inverse)
    x, logits = k9_cases.inputs(case)
    wy, wl = k9_cases.weights(case)
    kw = k9_cases.spec_kwargs(case)
    want = autograd_gradients("quadratic", kw, inverse, x, logits, wy, wl, poison=1e30)
    # (the first GRAD_ROWS rows are the ones test_table_gradients checks: same inputs, same upstream gradients)
    g = k9_cases.prepared_gradients(case.name)
    assert all(np.array_equal(g[k], a[:k9_cases.GRAD_ROWS]) for k, a in (("x", x), ("wy", wy), ("wl", wl)))
    big = repeated([x] + logits + [wy, wl], n)
    got = autograd_gradients("quadratic", kw, inverse, big[0], big[1:-2], big[-2], big[-1], poison=-7.0)
    assert take_status(ops) == 0
    for t, block, nm in zip(got, want, ("gx", "g_widths", "g_heights")):
        assert_repeats(t, block, nm)
