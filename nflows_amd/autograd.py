"""Differentiable wrappers around the HIP kernels.

The reference is trained by autograd through eager ops (`loss = -flow.log_prob(x).mean();
loss.backward()`, examples/moons.ipynb cell 3).  These `torch.autograd.Function`s make the same
call pattern work on the fused kernels: forward = the forward kernel, backward = ONE HIP kernel
for the spline layers (`nfa_rqs_coupling_backward_f32`, which recomputes the layer from its
inputs) and for the affine autoregressive element (K25), a few elementwise device ops for the affine
coupling layer.  Everything stays on the GPU; there is no CPU path here either.
"""
import ctypes

import os

import torch
from torch.autograd.function import once_differentiable

from . import _native as N


def needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class RqsCoupling(torch.autograd.Function):
    """K1 forward + K1-backward."""

    @staticmethod
    def forward(ctx, inputs, params, tidx, spec, inverse, perm, scat):
        from . import ops
        out, lad = ops._rqs_coupling_launch(inputs, params, tidx, spec, inverse, perm, scat, None)
        ctx.save_for_backward(inputs, params, tidx, perm, scat)
        ctx.spec = spec
        ctx.inverse = bool(inverse)
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        from . import ops
        inputs, params, tidx, perm, scat = ctx.saved_tensors
        B, D = inputs.shape
        dev = inputs.device
        g_out = torch.zeros_like(inputs) if g_out is None else g_out.contiguous()
        g_lad = None if g_lad is None else g_lad.contiguous()
        g_in = torch.empty_like(inputs)
        g_params = torch.empty_like(params)
        with torch.cuda.device(dev):
            rc = N.load().nfa_rqs_coupling_backward_f32(
                N.ptr(inputs), N.ptr(params), N.ptr(tidx), N.ptr(perm), N.ptr(scat), N.ptr(g_out),
                N.ptr(g_lad), N.ptr(g_in), N.ptr(g_params), N.ptr(ops._status_word(dev)), B, D,
                tidx.numel(), ctypes.byref(ctx.spec), N.FLAG_INVERSE if ctx.inverse else 0,
                N.stream_handle(dev))
        N.check(rc)
        return g_in, g_params, None, None, None, None, None


class RqsElementwise(torch.autograd.Function):
    """K5 forward; backward through the K1-backward kernel on the packed [n, P] logits (one spline
    per "sample": features = 1)."""

    @staticmethod
    def forward(ctx, inputs, uw, uh, ud, spec, inverse):
        from . import ops
        y, lad = ops._rqs_elementwise_launch(inputs, uw, uh, ud, spec, inverse)
        ctx.save_for_backward(inputs, uw, uh, ud)
        ctx.spec = spec
        ctx.inverse = bool(inverse)
        return y, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, g_lad):
        from . import ops
        inputs, uw, uh, ud = ctx.saved_tensors
        spec = ctx.spec
        K = spec.num_bins
        nd_std = K - 1 if spec.tails == N.TAILS_LINEAR else K + 1
        if ud.shape[-1] != nd_std:
            raise NotImplementedError("nflows_amd: gradients need exactly %d derivative logits" % nd_std)
        n = inputs.numel()
        dev = inputs.device
        x = inputs.contiguous().view(n, 1)
        packed = torch.cat((uw.reshape(n, K), uh.reshape(n, K), ud.reshape(n, nd_std)), dim=1).contiguous()
        g_y = (torch.zeros_like(x) if g_y is None else g_y.contiguous().view(n, 1))
        g_lad = None if g_lad is None else g_lad.contiguous().view(n)
        g_in = torch.empty_like(x)
        g_packed = torch.empty_like(packed)
        col0 = torch.zeros(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            rc = N.load().nfa_rqs_coupling_backward_f32(
                N.ptr(x), N.ptr(packed), N.ptr(col0), None, None, N.ptr(g_y), N.ptr(g_lad), N.ptr(g_in),
                N.ptr(g_packed), N.ptr(ops._status_word(dev)), n, 1, 1, ctypes.byref(spec),
                N.FLAG_INVERSE if ctx.inverse else 0, N.stream_handle(dev))
        N.check(rc)
        return (g_in.view(inputs.shape), g_packed[:, :K].reshape(uw.shape),
                g_packed[:, K:2 * K].reshape(uh.shape), g_packed[:, 2 * K:].reshape(ud.shape), None, None)


class RqsElementwise64(torch.autograd.Function):
    """K5d forward; backward through nfa_rqs_elementwise_backward_f64 (float64: `flow.double()` training and
    gradient checks of the spline layers run on the device; the reference differentiates the same
    expressions by autograd, rational_quadratic.py:13-181)."""

    @staticmethod
    def forward(ctx, inputs, uw, uh, ud, spec, inverse):
        from . import ops
        y, lad = ops._rqs_elementwise_launch(inputs, uw, uh, ud, spec, inverse)
        ctx.save_for_backward(inputs, uw, uh, ud)
        ctx.spec = spec
        ctx.inverse = bool(inverse)
        return y, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, g_lad):
        from . import ops
        inputs, uw, uh, ud = ctx.saved_tensors
        spec = ctx.spec
        K = spec.num_bins
        nd = ud.shape[-1]
        n = inputs.numel()
        dev = inputs.device
        x = inputs.contiguous().view(-1)
        w, sw = ops._logit_rows(uw, n, K)
        h, sh = ops._logit_rows(uh, n, K)
        d, sd = ops._logit_rows(ud, n, nd) if nd else (uw.reshape(n, 0), 1)
        g_y = None if g_y is None else g_y.contiguous().view(-1)
        g_lad = None if g_lad is None else g_lad.contiguous().view(-1)
        g_in = torch.empty_like(x)
        g_w = torch.empty(n, K, dtype=x.dtype, device=dev)
        g_h = torch.empty(n, K, dtype=x.dtype, device=dev)
        g_d = torch.empty(n, nd, dtype=x.dtype, device=dev)
        with torch.cuda.device(dev):
            rc = N.load().nfa_rqs_elementwise_backward_f64(
                N.ptr(x), N.ptr(w), sw, N.ptr(h), sh, N.ptr(d) if nd else N.ptr(w), sd, nd, N.ptr(g_y), N.ptr(g_lad),
                N.ptr(g_in), N.ptr(g_w), N.ptr(g_h), N.ptr(g_d) if nd else None, n, ctypes.byref(spec),
                int(ctx.inverse), N.stream_handle(dev))
        N.check(rc)
        return (g_in.view(inputs.shape), g_w.view(uw.shape), g_h.view(uh.shape), g_d.view(ud.shape), None, None)


def _scale_and_grad(u, activation):
    """scale = act(u) and d scale / d u for the in-kernel activations (coupling.py:224-225,
    autoregressive.py:101)."""
    if activation == N.SCALE_DEFAULT:
        sg = torch.sigmoid(u + 2)
        return sg + 1e-3, sg * (1 - sg)
    sp = torch.nn.functional.softplus(u) + 1e-3
    ds = torch.sigmoid(u)
    if activation == N.SCALE_GENERAL:
        inside = (sp >= 0) & (sp <= 3)
        return sp.clamp(0, 3), ds * inside
    return sp, ds  # N.SCALE_SOFTPLUS


class AffineCoupling(torch.autograd.Function):
    """K2 forward; backward as a handful of elementwise device ops on the [B, d_t] halves."""

    @staticmethod
    def forward(ctx, inputs, params, scale, tidx, activation, inverse, perm, scat):
        from . import ops
        out, lad = ops._affine_coupling_launch(inputs, params, scale, tidx, activation, inverse, perm, scat, None)
        ctx.save_for_backward(inputs, params, scale, tidx, perm, scat, out)
        ctx.activation = activation
        ctx.inverse = bool(inverse)
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        inputs, params, scale, tidx, perm, scat, out = ctx.saved_tensors
        act = ctx.activation
        B, D = inputs.shape
        dt = tidx.numel()
        g_out = torch.zeros_like(inputs) if g_out is None else g_out
        g_lad = torch.zeros(B, device=inputs.device) if g_lad is None else g_lad
        # undo the fused permutations on the gradient side: layer-local column order
        g_loc = g_out if scat is None else g_out.index_select(1, scat)  # g wrt layer column c
        src = tidx if perm is None else perm[tidx]
        dstc = tidx if scat is None else scat[tidx]
        x_t = inputs.index_select(1, src)          # layer input of the transformed columns
        y_t = out.index_select(1, dstc)            # layer output of the transformed columns
        g_t = g_loc.index_select(1, tidx)
        shift = params[:, :dt]
        if act == N.SCALE_ADDITIVE:
            s, ds, u_grad = None, None, None
        elif act == N.SCALE_GIVEN:
            s, ds = scale, None
        else:
            s, ds = _scale_and_grad(params[:, dt:], act)
        gl = g_lad[:, None]
        if act == N.SCALE_ADDITIVE:
            g_x_t = g_t
            g_shift = -g_t if ctx.inverse else g_t
            g_s = None
        elif not ctx.inverse:  # y = x*s + shift, lad = sum log s
            g_x_t = g_t * s
            g_shift = g_t
            g_s = g_t * x_t + gl / s
        else:                  # x = (y - shift)/s, lad = -sum log s   (x_t holds y, y_t holds x)
            g_x_t = g_t / s
            g_shift = -g_x_t
            g_s = -g_x_t * y_t - gl / s
        g_loc_in = g_loc.clone()
        g_loc_in[:, tidx] = g_x_t
        g_in = g_loc_in if perm is None else torch.empty_like(g_loc_in).index_copy_(1, perm, g_loc_in)
        g_scale = None
        if act == N.SCALE_ADDITIVE:
            g_params = g_shift
        elif act == N.SCALE_GIVEN:
            g_params = torch.cat((g_shift, torch.zeros_like(g_shift)), dim=1)
            g_scale = g_s
        else:
            g_params = torch.cat((g_shift, g_s * ds), dim=1)
        return g_in, g_params, g_scale, None, None, None, None, None


class AffineAutoregressive(torch.autograd.Function):
    """K2b forward; K25's element kernel backward (`nfa_affine_autoregressive_backward_f32`: one launch, params
    interleaved [B, D, 2])."""

    @staticmethod
    def forward(ctx, inputs, params, inverse):
        from . import ops
        out, lad = ops._affine_autoregressive_launch(inputs, params, inverse)
        ctx.inverse = bool(inverse)
        ctx.save_for_backward(out if ctx.inverse else inputs, params)   # (what the backward kernel reads)
        ctx.set_materialize_grads(False)   # an unused output's gradient arrives as None: the kernel's null pointer
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        from . import ops
        if g_out is None and g_lad is None:
            return None, None, None
        seen, params = ctx.saved_tensors
        g_in, g_params = ops.affine_autoregressive_backward(None if ctx.inverse else seen, params,
                                                            seen if ctx.inverse else None, g_out, g_lad, ctx.inverse)
        return g_in, g_params, None


class StandardNormalLogProb(torch.autograd.Function):
    """Fused base log-density (+ logabsdet) forward; -z * g backward."""

    @staticmethod
    def forward(ctx, z, logabsdet):
        from . import ops
        out = ops._standard_normal_log_prob_launch(z, logabsdet)
        ctx.save_for_backward(z)
        ctx.has_lad = logabsdet is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        g_z = -z * g.reshape((-1,) + (1,) * (z.dim() - 1))
        return g_z, (g if ctx.has_lad else None)


class DiagNormalLogProb(torch.autograd.Function):
    """K20 "diag" forward + backward (ops.diag_normal_log_prob): one launch from the saved operands; per-row parameters get
    their gradients from that launch (the packed [B, 2 N] encoder output as one [B, 2 N] tensor), the shared row from K17's
    float64 column reduction.  The gradient of `logabsdet` is grad_log_prob itself."""

    @staticmethod
    def forward(ctx, inputs, means, log_stds, log_z, logabsdet):
        from . import ops
        out = ops._diag_normal_launch(inputs, means, log_stds, log_z, logabsdet)
        ctx.packed = log_stds is None
        ctx.save_for_backward(inputs, means, *(() if log_stds is None else (log_stds,)))
        ctx.has_add = logabsdet is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import ops
        inputs, means = ctx.saved_tensors[:2]
        log_stds = None if ctx.packed else ctx.saved_tensors[2]
        want_params = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        g_x, g_m, g_ls = ops._diag_normal_backward_launch(inputs, means, log_stds, g, want_params)
        return (g_x if ctx.needs_input_grad[0] else None, g_m if ctx.needs_input_grad[1] else None,
                g_ls if (not ctx.packed and ctx.needs_input_grad[2]) else None, None, g if ctx.has_add else None)


class MoGLogProb(torch.autograd.Function):
    """K20 "mog" forward + backward (ops.mog_log_prob): grad_outputs and grad_inputs in one launch from the saved operands."""

    @staticmethod
    def forward(ctx, inputs, outputs, num_components, epsilon, logabsdet):
        from . import ops
        out = ops._mog_launch(inputs, outputs, num_components, epsilon, logabsdet)
        ctx.save_for_backward(inputs, outputs)
        ctx.K, ctx.epsilon, ctx.has_add = num_components, epsilon, logabsdet is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from . import ops
        inputs, outputs = ctx.saved_tensors
        g_x, g_o = ops._mog_backward_launch(inputs, outputs, g, ctx.K, ctx.epsilon)
        return (g_x if ctx.needs_input_grad[0] else None, g_o if ctx.needs_input_grad[1] else None, None, None,
                g if ctx.has_add else None)


def _lu_parameter_grads(seen, g_seen, lower, upper, udiag, bias, eps, inverse, lad_weight):
    """The four parameter gradients of the LU layer from float64 rows: `seen` [rows, D] the layer's inputs and `g_seen`
    the gradients of its outputs, both as the layer itself sees them (after the gather / before the scatter);
    `lad_weight` = d loss / d (sum_i log U_ii) as a float64 scalar tensor, or None.  Formulas: LULinear's docstring."""
    # float64, rounded once: a parameter gradient is ONE number summed over the whole batch (features = 2 has a
    # single lower entry) -- nothing averages its rounding error out.  (Cost under training: not measured.)
    from .transforms.lu import dense_factors, solve_rows
    f64 = torch.float64
    logits = udiag.to(f64)
    diag = torch.nn.functional.softplus(logits) + eps
    dense_l, dense_u = dense_factors(lower.to(f64), upper.to(f64), diag)
    D = seen.shape[1]
    rows, cols = torch.tril_indices(D, D, -1, device=seen.device)
    urows, ucols = torch.triu_indices(D, D, 1, device=seen.device)
    if not inverse:
        a, g, sign = seen, g_seen, 1.0           # y = L (U a) + b,  g = dloss / dy
    else:
        # x = U^-1 L^-1 (y - b): the x side and the y-side gradient g = W^-T gx, both re-solved in float64 from
        # the saved inputs (the float32 output's own rounding would otherwise be the gradient's error)
        a = solve_rows(dense_l, dense_u, seen - bias.to(f64))
        g = solve_rows(dense_u.t(), dense_l.t(), g_seen)   # W^T = U^T L^T: lower factor U^T, upper factor L^T
        sign = -1.0
    d_l = sign * (g.t() @ (a @ dense_u.t()))
    d_u = sign * ((g @ dense_l).t() @ a)
    d_diag = torch.diagonal(d_u)
    if lad_weight is not None:
        d_diag = d_diag + sign * lad_weight / diag
    return (d_l[rows, cols].to(lower.dtype), d_u[urows, ucols].to(upper.dtype),
            (d_diag * torch.where(logits > 20.0, torch.ones_like(logits), torch.sigmoid(logits))).to(udiag.dtype),
            (sign * g.sum(0)).to(bias.dtype))


class LULinear(torch.autograd.Function):
    """K16 forward + K16-backward.  The kernel gives the input gradient; the parameter gradients are [D, D] reductions
    over the batch on the device's library GEMM in float64 (rounded once: every entry is one number summed over the whole
    batch), gathered from the triangles the parameters fill.

    With a = the rows on the x side of y = L (U a) + b and g = the gradient on the y side (forward: a = inputs,
    g = grad_outputs; inverse: both re-solved in float64 from the saved inputs and grad_outputs), h = U a:
        dL = +-tril(g^T h, -1)     dU = +-triu((g L)^T a)     db = +-sum_rows g       (- for the inverse direction)
    and the diagonal logits receive dU_ii and the log-determinant's +-sum(grad_logabsdet) / U_ii through softplus'."""

    @staticmethod
    def forward(ctx, inputs, lower, upper, udiag, bias, eps, inverse, perm, scat):
        from . import ops
        out, lad = ops._lu_linear_launch(inputs, (lower, upper, udiag, bias), eps, inverse, perm, scat, None)
        ctx.save_for_backward(inputs, lower, upper, udiag, bias, perm, scat)
        ctx.eps, ctx.inverse = eps, inverse
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        from . import ops
        inputs, lower, upper, udiag, bias, perm, scat = ctx.saved_tensors
        inverse = ctx.inverse
        g_out = torch.zeros_like(inputs) if g_out is None else g_out.contiguous()
        grads = [None] * 5
        if ctx.needs_input_grad[0]:
            grads[0] = ops._lu_linear_backward_launch(g_out, (lower, upper, udiag), ctx.eps, inverse, perm, scat)
        if any(ctx.needs_input_grad[1:5]):
            f64 = torch.float64
            # the rows as the layer itself sees them (without the fused permutation / scatter)
            seen = inputs.to(f64) if perm is None else inputs.to(f64).index_select(1, perm)
            g_seen = g_out.to(f64) if scat is None else g_out.to(f64).index_select(1, scat)
            grads[1:5] = _lu_parameter_grads(seen, g_seen, lower, upper, udiag, bias, ctx.eps, inverse,
                                             None if g_lad is None else g_lad.to(f64).sum())
        return tuple(grads) + (None, None, None, None)


class LUConv1x1(torch.autograd.Function):
    """K19 forward + K19-backward.  The kernel gives the input gradient; the parameter gradients are LULinear's float64
    formulas with the pixels as rows ([B HW, C] after the channel gather: forward the inputs' planes channel_perm,
    inverse the output gradient's).  logabsdet[b] = +- HW sum_i log U_ii, so its term into the diagonal logits is
    +- HW sum_b grad_logabsdet[b] / U_ii."""

    @staticmethod
    def forward(ctx, inputs, lower, upper, udiag, bias, eps, inverse, perm):
        from . import ops
        out, lad = ops._lu_conv1x1_launch(inputs, (lower, upper, udiag, bias), eps, inverse, perm, None)
        ctx.save_for_backward(inputs, lower, upper, udiag, bias, perm)
        ctx.eps, ctx.inverse = eps, inverse
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        from . import ops
        inputs, lower, upper, udiag, bias, perm = ctx.saved_tensors
        inverse = ctx.inverse
        g_out = torch.zeros_like(inputs) if g_out is None else g_out.contiguous()
        grads = [None] * 5
        if ctx.needs_input_grad[0]:
            grads[0] = ops._lu_conv1x1_backward_launch(g_out, (lower, upper, udiag), ctx.eps, inverse, perm)
        if any(ctx.needs_input_grad[1:5]):
            f64 = torch.float64
            C, hw = inputs.shape[1], inputs.shape[2] * inputs.shape[3]

            def pixel_rows(t, gathered):
                t = t.to(f64)
                if gathered and perm is not None:
                    t = t.index_select(1, perm)
                return t.permute(0, 2, 3, 1).reshape(-1, C)

            grads[1:5] = _lu_parameter_grads(pixel_rows(inputs, not inverse), pixel_rows(g_out, inverse), lower, upper,
                                             udiag, bias, ctx.eps, inverse,
                                             None if g_lad is None else hw * g_lad.to(f64).sum())
        return tuple(grads) + (None, None, None)


def _rows_outer_f64(g, x, chunk=1024):
    """g^T x of two float32 [B, D] tensors in float64, [D, D].  The library's GEMM gets no parallelism out of a
    [D, B] x [B, D] product with a small D and a long B (28 ms at 262 144 x 16, DESIGN.md section 4 "K24"), so the rows
    go in chunks as one batched product whose [D, D] results are added up; the same shape gives the same bits."""
    B, D = g.shape
    full = (B // chunk) * chunk
    total = g.new_zeros(D, D, dtype=torch.float64)
    if full:
        gb = g[:full].view(-1, chunk, D).to(torch.float64)
        xb = x[:full].view(-1, chunk, D).to(torch.float64)
        total = total + torch.bmm(gb.transpose(1, 2), xb).sum(0)
    if full < B:
        total = total + g[full:].to(torch.float64).t() @ x[full:].to(torch.float64)
    return total


class Householder(torch.autograd.Function):
    """K24 forward + K24-backward (ops.householder).  The backward kernel gives the input gradient and, per reflection k,
    S_k = sum_rows [b x + a g] (ops._householder_backward_launch), so dL/dv_k = - c_k S_k with c_k = 2 / (v_k . v_k) in
    float64; the diagonal logits receive the diagonal stage's sum and the log-determinant's +- sum(grad_logabsdet) / d_i
    through softplus'; the bias the float64 column sum of the gradient where the bias is applied.

    With a triangular stage (QRLinear) the reflections' part is the same kernel on the rows next to the reflections, and
    the triangular step is a launch of its own on either side of it:
        forward  y = Q (R x) + b:   h = R x,  (g_h, dQ) from the kernel at (h, g_y),  g_x = R^T g_h,   dR = triu(g_h^T x)
        inverse  x = R^-1 Q^T (y - b):   g_u = R^-T g_x,  (g_y, dQ) from the kernel at (y, g_u),       dR = -triu(g_u^T x)
    dR is a [D, D] reduction over the batch on the device's library GEMM in float64, as LULinear's; log_upper_diag
    receives dR_ii R_ii and +- sum(grad_logabsdet)."""

    @staticmethod
    def forward(ctx, inputs, qa, qb, diag, upper, logd, bias, eps, inverse):
        from . import ops
        out, lad = ops._householder_launch(inputs, (qa, qb, diag, upper, logd, bias), eps, inverse, None)
        ctx.save_for_backward(inputs, out, qa, qb, diag, upper, logd, bias)
        ctx.eps, ctx.inverse = eps, inverse
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        from . import ops
        inputs, out, qa, qb, diag, upper, logd, bias = ctx.saved_tensors
        eps, inverse = ctx.eps, ctx.inverse
        f64 = torch.float64
        sign = -1.0 if inverse else 1.0
        g_out = torch.zeros_like(inputs) if g_out is None else g_out.contiguous()
        lad_weight = None if g_lad is None else g_lad.to(f64).sum()
        grads = [None] * 7
        if not any(ctx.needs_input_grad[1:7]):
            grads[0], _ = ops._householder_backward_launch(None, g_out, (qa, qb, diag, upper, logd, bias), eps, inverse)
            return tuple(grads) + (None, None)
        if upper is None:
            g_in, sums = ops._householder_backward_launch(inputs, g_out, (qa, qb, diag, None, None, bias), eps, inverse)
            g_at_bias = g_in if inverse else g_out
        else:
            tri = (None, None, None, upper, logd, None)
            if not inverse:
                h, _ = ops._householder_launch(inputs, tri, eps, False, None, want_logabsdet=False)
                g_h, sums = ops._householder_backward_launch(h, g_out, (qa, qb, None, None, None, None), eps, False)
                g_in, _ = ops._householder_backward_launch(None, g_h, tri, eps, False)
                g_r, x_r, g_at_bias = g_h, inputs, g_out
            else:
                g_u, _ = ops._householder_backward_launch(None, g_out, tri, eps, True)
                g_in, sums = ops._householder_backward_launch(inputs, g_u, (qa, qb, None, None, None, bias), eps, True)
                g_r, x_r, g_at_bias = g_u, out, g_in
            D = inputs.shape[1]
            d_r = sign * _rows_outer_f64(g_r, x_r)
            rows, cols = torch.triu_indices(D, D, 1, device=inputs.device)
            grads[4] = d_r[rows, cols].to(upper.dtype)
            d_logd = torch.diagonal(d_r) * torch.exp(logd.to(f64))
            if lad_weight is not None:
                d_logd = d_logd + sign * lad_weight
            grads[5] = d_logd.to(logd.dtype)
        grads[0] = g_in
        row = 0
        for slot, q in ((1, qa), (2, qb)):
            if q is not None:
                q64 = q.to(f64)
                c = 2.0 / (q64 * q64).sum(1, keepdim=True)
                grads[slot] = (-c * sums[row:row + q.shape[0]]).to(q.dtype)
                row += q.shape[0]
        if diag is not None:
            logits = diag.to(f64)
            d = torch.nn.functional.softplus(logits) + eps
            d_d = sign * sums[row]
            if lad_weight is not None:
                d_d = d_d + sign * lad_weight / d
            grads[3] = (d_d * torch.where(logits > 20.0, torch.ones_like(logits), torch.sigmoid(logits))).to(diag.dtype)
        if bias is not None:
            grads[6] = (sign * g_at_bias.to(f64).sum(0)).to(bias.dtype)
        return tuple(grads) + (None, None)


class Nonlinearity(torch.autograd.Function):
    """K18 forward + K18-backward (ops.nonlinearity): the input gradient from the saved inputs in one launch, Sigmoid's
    temperature gradient from per-workgroup float64 partials folded in a fixed order."""

    @staticmethod
    def forward(ctx, inputs, temperature, code, constants, inverse):
        from . import ops
        out, lad = ops._nonlinearity_launch(inputs, temperature, code, constants, inverse, None)
        ctx.save_for_backward(inputs, temperature)
        ctx.code, ctx.constants, ctx.inverse = code, constants, inverse
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        from . import ops
        inputs, temperature = ctx.saved_tensors
        g_out = torch.zeros_like(inputs) if g_out is None else g_out
        g_lad = inputs.new_zeros(inputs.shape[0]) if g_lad is None else g_lad
        want_t = temperature is not None and ctx.needs_input_grad[1]
        g_in, g_t = ops._nonlinearity_backward_launch(inputs, temperature, g_out, g_lad, ctx.code, ctx.constants,
                                                      ctx.inverse, want_t)
        return (g_in if ctx.needs_input_grad[0] else None), g_t, None, None, None


class NormMap(torch.autograd.Function):
    """K17 forward and its gradients (BatchNorm / ActNorm, ops.batch_norm / ops.act_norm).

    The input gradient is one element-wise kernel.  Everything that is summed over the batch -- G1 = sum g and
    Gu = sum g * u per column, u the layer's input -- comes from K17's column reduction in float64; the parameter gradients
    and the coefficients of the batch-statistics gradient are [D] float64 expressions of G1, Gu and L = sum grad_logabsdet,
    rounded once (they are not hot).  With y = a ((u - m) / s) + t:
      BatchNorm forward   d bias = G1          d weight = (Gu - mean G1) / sd + L / weight
      BatchNorm inverse   d bias = -(sd / w) G1   d weight = -(sd / w^2) (Gu - bias G1) - L / weight
      ActNorm forward     d shift = G1         d log_scale = scale Gu + L
      ActNorm inverse     d shift = -G1 / scale   d log_scale = -(Gu - shift G1) / scale - L
    and d unconstrained_weight = d weight * softplus'.  With batch statistics the mean and the unbiased variance depend on
    the inputs:  grad_x = (w / s) (g - G1 / B - xh G2 / (B - 1)) - L (x - mean) / ((B - 1) (var + eps)),  G2 = sum g xh."""

    @staticmethod
    def forward(ctx, inputs, kind, eps, inverse, batch_statistics, perm, scat, *params):
        from . import ops
        out, lad = ops._norm_map_launch(inputs, kind, params, eps, inverse, perm, scat, None)
        ctx.save_for_backward(inputs, perm, scat, *params)
        ctx.kind, ctx.eps, ctx.inverse, ctx.batch_statistics = kind, eps, inverse, batch_statistics
        return out, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_lad):
        from . import ops
        inputs, perm, scat = ctx.saved_tensors[:3]
        params = ctx.saved_tensors[3:]
        kind, eps, inverse = ctx.kind, ctx.eps, ctx.inverse
        f64 = torch.float64
        g_out = torch.zeros_like(inputs) if g_out is None else g_out.contiguous()
        rows = inputs.shape[0]
        L = g_lad.to(f64).sum() if g_lad is not None else torch.zeros((), dtype=f64, device=inputs.device)
        need_params = any(ctx.needs_input_grad[7:9])
        G1 = Gu = None
        if need_params or ctx.batch_statistics:
            G1, Gu = ops.column_sums(g_out, inputs, g_columns=scat, u_columns=perm)   # in the layer's own column order
        d0 = d1 = None
        if kind == ops.NORM_BATCH_NORM:
            logits, bias, mean, var = (t.to(f64) for t in params)
            weight = torch.nn.functional.softplus(logits) + eps
            ve = var + eps
            sd = torch.sqrt(ve)
            if G1 is not None:
                if not inverse:
                    G2 = (Gu - mean * G1) / sd
                    d_weight, d1 = G2 + L / weight, G1
                else:
                    d_weight, d1 = -(sd / (weight * weight)) * (Gu - bias * G1) - L / weight, -(sd / weight) * G1
                d0 = d_weight * torch.where(logits > 20.0, torch.ones_like(logits), torch.sigmoid(logits))
        else:
            log_scale, shift = (t.to(f64) for t in params)
            scale = torch.exp(log_scale)
            if G1 is not None:
                if not inverse:
                    d0, d1 = scale * Gu + L, G1
                else:
                    d0, d1 = -(Gu - shift * G1) / scale - L, -G1 / scale
        g_in = None
        if ctx.needs_input_grad[0]:
            if ctx.batch_statistics:
                s32 = sd.float().to(f64)   # the divisor the forward kernel used
                G2 = (Gu - mean * G1) / s32
                coef = torch.stack((mean, s32, weight / s32, G1 / rows, G2 / (rows - 1), L / ((rows - 1) * ve))).float()
                g_in = ops._norm_batch_backward_launch(g_out, inputs, coef, perm, scat)
            else:
                g_in = ops._norm_map_backward_launch(g_out, kind, params, eps, inverse, perm, scat)
        grads = [g_in, None, None, None, None, None, None,
                 d0.to(params[0].dtype) if d0 is not None and ctx.needs_input_grad[7] else None,
                 d1.to(params[1].dtype) if d1 is not None and ctx.needs_input_grad[8] else None]
        return tuple(grads) + (None,) * (len(params) - 2)


class Linear(torch.autograd.Function):
    """y = x W^T + b (the conditioner layers).  Forward and the input gradient are library GEMMs;
    the weight and bias gradients -- a product whose reduction runs over the whole batch into a tiny
    result, which the library tiles into a handful of workgroups -- come from K10
    (`nfa_linear_wgrad_f32`: batch split over the chip, fp32 matrix cores, fixed-order sum)."""

    @staticmethod
    def forward(ctx, inputs, weight, bias):
        ctx.save_for_backward(inputs, weight)
        ctx.has_bias = bias is not None
        return torch.nn.functional.linear(inputs, weight, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        from . import ops
        inputs, weight = ctx.saved_tensors
        g_out = g_out.contiguous()
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        g_in = g_out @ weight if need_x else None
        g_w = g_b = None
        if need_w or need_b:
            got = ops.linear_wgrad(inputs, g_out, need_bias=need_b)
            if got is None:  # widths the kernel does not take
                g_w = g_out.t() @ inputs if need_w else None
                g_b = g_out.sum(0) if need_b else None
            else:
                g_w, g_b = got
        return g_in, (g_w if need_w else None), g_b


class SelectColumns(torch.autograd.Function):
    """inputs.index_select(1, columns) for DISTINCT columns (a coupling layer's identity split, coupling.py:82) whose
    backward writes the gradient with index_copy into a zero tensor: torch's own backward is index_add_ -- atomic adds,
    16 us per layer at 65 536 x 64 against 6 us -- because it cannot know the columns are distinct.  The backward is
    written with differentiable operations (out-of-place index_copy): double backward works."""

    @staticmethod
    def forward(ctx, inputs, columns):
        ctx.save_for_backward(columns)
        ctx.width = inputs.shape[1]
        return inputs.index_select(1, columns)

    @staticmethod
    def backward(ctx, grad):
        (columns,) = ctx.saved_tensors
        return grad.new_zeros(grad.shape[0], ctx.width).index_copy(1, columns, grad.contiguous()), None


def _columns_are_distinct(columns):
    """index_copy with repeated indices is nondeterministic and DROPS gradient: the identity split's columns are
    distinct for a mask alone, and through a fused Permutation only if that permutation is a bijection -- which the
    reference's Permutation never checks.  Checked once per index tensor and version (one synchronising comparison); the
    verdict lives ON the tensor object (round 5 kept a global table keyed by the raw address, which a freed and re-allocated
    index tensor of the same size could inherit)."""
    known = columns.__dict__.get("_nfa_distinct") if hasattr(columns, "__dict__") else None
    if known is None or known[0] != columns._version:
        known = (columns._version, bool(torch.unique(columns).numel() == columns.numel()))
        try:
            columns._nfa_distinct = known
        except AttributeError:   # (no instance dictionary: checked every time)
            pass
    return known[1]


def select_columns(inputs, columns):
    """`inputs[:, columns]`; under autograd through SelectColumns when the columns are distinct (torch's index_select,
    whose backward accumulates, otherwise)."""
    if torch.is_grad_enabled() and inputs.requires_grad and inputs.dim() == 2 and _columns_are_distinct(columns):
        return SelectColumns.apply(inputs, columns)
    return inputs.index_select(1, columns)


# K10 for the hidden Linears of a conditioner in one launch pair (A/B switch: NFA_K10_BATCHED=0)
BATCHED_WGRAD = os.environ.get("NFA_K10_BATCHED", "1") != "0"


class ResidualNetHidden(torch.autograd.Function):
    """K14: a ResidualNet (initial Linear + residual blocks, and with `with_final` the final Linear: resnet.py:92-100)
    under autograd -- `nfa_resnet_hidden_forward_f32` forward, `nfa_resnet_hidden_backward_f32` for the chain of input
    gradients through the hidden part, K10 (`nfa_linear_wgrad_f32`) for every weight / bias gradient on the arrays
    the two leave behind; the final Linear's input gradient is the backward kernel's first GEMM (round 4:
    `nfa_resnet_backward_f32`; a library GEMM before).  Arguments: the identity features
    [B, d_i], with_final, then W_in, b_in, (W_0, b_0, W_1, b_1) per block and, with_final, W_f, b_f."""

    @staticmethod
    def forward(ctx, x, with_final, *params):
        from . import ops
        hidden_params = params[:-2] if with_final else params
        nb = (len(hidden_params) - 2) // 4
        blocks = [hidden_params[2 + 4 * k: 6 + 4 * k] for k in range(nb)]
        final = params[-2:] if with_final else None
        w_in = params[0]
        ctx.di = x.shape[1]
        if ctx.di % 4:   # identity features in multiples of four: zero columns on both sides (tabular D = 6, 21, 43, 63 ...)
            pad = 4 - ctx.di % 4
            x = torch.nn.functional.pad(x.detach(), (0, pad))
            w_in = torch.nn.functional.pad(w_in.detach(), (0, pad))
        fwd_w, fwd_b, bwd_w, fbias = ops.pack_resnet_hidden_train(w_in, params[1], blocks, final)
        hidden, saved, out = ops.resnet_hidden_forward(x, fwd_w, fwd_b, nb, fbias, final[0].shape[0] if with_final else 0)
        ctx.nb, ctx.with_final, ctx.H = nb, with_final, params[0].shape[0]   # (H < 128: the arrays are zero-padded to 128)
        if with_final:
            ctx.save_for_backward(x.detach().contiguous(), saved, bwd_w, hidden, final[0])
            return out
        ctx.save_for_backward(x.detach().contiguous(), saved, bwd_w)
        return hidden if ctx.H == 128 else hidden[:, :ctx.H]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        return _resnet_hidden_backward(ctx, g_out, ctx.saved_tensors)


def _resnet_hidden_backward(ctx, g_out, saved_tensors, context=None):
    """K14's backward pass for ResidualNetHidden and MadeNet: (grad of x, None, then one gradient per parameter).
    `saved_tensors`: (x, saved, bwd_w) or, with the final Linear, (x, saved, bwd_w, hidden, W_f -- or a function
    that returns it, called only where the backward kernel does not take the width).
    `context` (K27, the Functions with a context): dict(mode, planes, pre, first_param) -- the pass goes through
    `ops.resnet_backward_ctx`, the second Linears' grad_outputs are the GATED gradients in GLU mode, and the dict
    receives `grads`, `g_hidden` and `plane_grads` (GLU) for the planes' gradients."""
    from . import ops
    nb, H = ctx.nb, ctx.H
    need = ctx.needs_input_grad[context["first_param"] if context else 2:]   # per parameter
    g_out = g_out.contiguous()

    def wgrad(inputs, grad_outputs, need_w, need_b, rows=None, cols=None):
        """(grad_weight, grad_bias) of a Linear; rows / cols: the net's own width inside the 128-wide arrays"""
        if not (need_w or need_b):
            return None, None
        got = ops.linear_wgrad(inputs, grad_outputs, need_bias=need_b)
        if got is None:   # widths K10 does not take
            got = (grad_outputs.t() @ inputs if need_w else None), (grad_outputs.sum(0) if need_b else None)
        g_w, g_b = (got[0] if need_w else None), got[1]
        if g_w is not None and (rows is not None or cols is not None):
            g_w = g_w[:rows, :cols].contiguous()
        if g_b is not None and rows is not None:
            g_b = g_b[:rows].contiguous()
        return g_w, g_b

    narrow = H if H != 128 else None
    tail = ()
    fused = gated = None
    if ctx.with_final:
        x, saved, bwd_w, hidden, w_f = saved_tensors
        tail = wgrad(hidden, g_out, need[-2], need[-1], cols=narrow)
        # the final Linear's input gradient inside the backward kernel (round 4; its W_f^T stages are in `bwd_w`)
        if ops.FUSED_FINAL_DGRAD and context is None:
            fused = ops.resnet_backward(g_out, bwd_w, saved, x.shape[1])
        elif ops.FUSED_FINAL_DGRAD and g_out.shape[1] % 4 == 0:
            got = ops.resnet_backward_ctx(context["mode"], g_out, bwd_w, saved, x.shape[1], context["planes"],
                                          context["pre"], from_params=True)
            fused, gated = (got[0], got[1], got[2]), got[4]
            context.update(plane_grads=got[3])
        if fused is None:
            g_hidden = g_out @ (w_f() if callable(w_f) else w_f)        # ... or one library GEMM
    else:
        x, saved, bwd_w = saved_tensors
        g_hidden = g_out
    if fused is not None:
        g_x, grads, g_hidden = fused      # (g_hidden [B, 128]: zero columns past a narrower net's width)
    else:
        if narrow is not None:
            g_hidden = torch.nn.functional.pad(g_hidden, (0, 128 - H))
        if context is None:
            g_x, grads = ops.resnet_hidden_backward(g_hidden, bwd_w, saved, x.shape[1])
        else:
            g_x, grads, g_hidden, plane_grads, gated = ops.resnet_backward_ctx(
                context["mode"], g_hidden, bwd_w, saved, x.shape[1], context["planes"], context["pre"])
            context.update(plane_grads=plane_grads)
    if context is not None:
        context.update(grads=grads, g_hidden=g_hidden)
    di = ctx.di if ctx.di != x.shape[1] else None      # (x was saved with its pad columns)
    out = [(g_x if di is None else g_x[:, :di]) if ctx.needs_input_grad[0] else None, None]
    out += wgrad(x, grads[0] if nb else g_hidden, need[0], need[1], rows=narrow, cols=di)
    # the 2 nb hidden Linears (all 128 -> 128 inside the padded arrays): ONE launch pair of K10 when every gradient
    # is wanted (a training step), layer by layer otherwise
    hidden_problems = []
    for k in range(nb):
        hidden_problems.append((saved[2 * k], grads[2 * k + 1]))
        if context is not None and gated is not None:   # GLU: the second Linear saw g sigmoid(c_k), not g
            hidden_problems.append((saved[2 * k + 1], gated[k]))
        else:
            hidden_problems.append((saved[2 * k + 1], grads[2 * k + 2] if k + 1 < nb else g_hidden))
    batched = None
    if nb and all(need[2:2 + 4 * nb]) and 2 * nb <= 8 and BATCHED_WGRAD:
        batched = ops.linear_wgrad_batched(hidden_problems, need_bias=True)
    if batched is not None:
        for g_w, g_b in batched:
            if narrow is not None:
                g_w, g_b = g_w[:narrow, :narrow].contiguous(), g_b[:narrow].contiguous()
            out += (g_w, g_b)
    else:
        for q, (inp, g_o) in enumerate(hidden_problems):
            out += wgrad(inp, g_o, need[2 + 2 * q], need[3 + 2 * q], rows=narrow, cols=narrow)
    return tuple(out) + tuple(tail)


class MadeNet(torch.autograd.Function):
    """K25: a MADE with residual blocks and no context (made.py: initial masked Linear, `h += L1(relu(L0(relu(h))))`
    per block, final masked Linear) under autograd on K14 and K10 -- the ResidualNet of `ResidualNetHidden` with its
    0/1 masks multiplied into the weights by the packer (`nfa_pack_made_train_f32`: no `mask * weight` tensors), and
    into K10's weight gradients on the way out (a masked-out weight's gradient is exactly zero, as autograd through
    `mask * weight` gives).  Arguments: inputs [B, D], masks = (mask of W_in, of W_0 and W_1 per block, of W_f), then
    W_in, b_in, (W_0, b_0, W_1, b_1) per block, W_f, b_f.  Feature counts and output widths that are no multiples
    of four run with zero pad columns on the inputs and zero pad rows of the final Linear, which exist only in the
    packed streams.  Deterministic: every kernel in it sums in a fixed order."""

    @staticmethod
    def forward(ctx, x, masks, *params):
        from . import ops
        nb = (len(params) - 4) // 4
        blocks = [params[2 + 4 * k: 6 + 4 * k] for k in range(nb)]
        final = params[-2:]
        ctx.di, ctx.rows = x.shape[1], final[0].shape[0]
        ctx.nb, ctx.with_final, ctx.H = nb, True, params[0].shape[0]
        x = x.detach()
        if ctx.di % 4:
            x = torch.nn.functional.pad(x, (0, 4 - ctx.di % 4))
        out4 = (ctx.rows + 3) // 4 * 4
        fwd_w, fwd_b, bwd_w, fbias = ops.pack_made_train(params[0], params[1], blocks, final, masks)
        hidden, saved, out = ops.resnet_hidden_forward(x, fwd_w, fwd_b, nb, fbias, out4)
        ctx.save_for_backward(x.contiguous(), saved, bwd_w, hidden, final[0], *masks)
        return out if out4 == ctx.rows else out[:, :ctx.rows]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        x, saved, bwd_w, hidden, w_f = ctx.saved_tensors[:5]
        masks = ctx.saved_tensors[5:]
        rows, pad = ctx.rows, -ctx.rows % 4
        if pad:
            g_out = torch.nn.functional.pad(g_out, (0, pad))

        def masked_final():   # (only where the backward kernel leaves the final Linear's input gradient to a GEMM)
            w = w_f if masks[-1] is None else w_f * masks[-1]
            return torch.nn.functional.pad(w, (0, 0, 0, pad)) if pad else w

        grads = list(_resnet_hidden_backward(ctx, g_out, (x, saved, bwd_w, hidden, masked_final)))
        if pad:   # the final Linear's gradients without the pad rows
            grads[-2] = None if grads[-2] is None else grads[-2][:rows].contiguous()
            grads[-1] = None if grads[-1] is None else grads[-1][:rows].contiguous()
        pairs = [(g, m) for g, m in zip(grads[2::2], masks) if g is not None and m is not None]
        if pairs:
            torch._foreach_mul_([g for g, _ in pairs], [m for _, m in pairs])
        return tuple(grads)


class ResidualNetHiddenCtx(torch.autograd.Function):
    """K27: `ResidualNetHidden` for a ResidualNet WITH a context (resnet.py:42-52, :92-100): the context is concatenated to
    the inputs by the caller (under autograd), every block's `context_layer` stays a stock Linear whose output, zero-padded
    to 128 columns, enters as a plane; the kernels gate t_k = W_1 relu(a_k) + b_1 with sigmoid(plane) and return the
    planes' gradients, from which autograd reaches the context Linears, the context and whatever produced it.
    Arguments: [inputs | context] [B, d_i + C], with_final, the number of blocks, one plane [B, 128] per block, then the
    parameters as `ResidualNetHidden` takes them.  Once-differentiable and deterministic."""

    @staticmethod
    def forward(ctx, x, with_final, nb, *rest):
        from . import ops
        planes, params = rest[:nb], rest[nb:]
        hidden_params = params[:-2] if with_final else params
        assert (len(hidden_params) - 2) // 4 == nb
        blocks = [hidden_params[2 + 4 * k: 6 + 4 * k] for k in range(nb)]
        final = params[-2:] if with_final else None
        w_in = params[0]
        ctx.di = x.shape[1]
        if ctx.di % 4:
            pad = 4 - ctx.di % 4
            x = torch.nn.functional.pad(x.detach(), (0, pad))
            w_in = torch.nn.functional.pad(w_in.detach(), (0, pad))
        fwd_w, fwd_b, bwd_w, fbias = ops.pack_resnet_hidden_train(w_in, params[1], blocks, final)
        hidden, saved, out, pre = ops.resnet_hidden_forward_ctx(ops.TRAIN_CTX_GLU, x, planes, fwd_w, fwd_b, nb, fbias,
                                                                final[0].shape[0] if with_final else 0)
        ctx.nb, ctx.with_final, ctx.H = nb, with_final, params[0].shape[0]
        planes = [p.detach() for p in planes]
        if with_final:
            ctx.save_for_backward(x.detach().contiguous(), saved, bwd_w, hidden, final[0], pre, *planes)
            return out
        ctx.save_for_backward(x.detach().contiguous(), saved, bwd_w, pre, *planes)
        return hidden if ctx.H == 128 else hidden[:, :ctx.H]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        from . import ops
        n = 5 if ctx.with_final else 3
        pre, planes = ctx.saved_tensors[n], ctx.saved_tensors[n + 1:]
        context = dict(mode=ops.TRAIN_CTX_GLU, planes=planes, pre=pre, first_param=3 + ctx.nb)
        grads = _resnet_hidden_backward(ctx, g_out, ctx.saved_tensors[:n], context)
        plane_grads = context["plane_grads"]
        return (grads[0], None, None) + tuple(plane_grads[k] for k in range(ctx.nb)) + tuple(grads[2:])


class MadeNetCtx(torch.autograd.Function):
    """K27: `MadeNet` for a MADE with residual blocks AND a context (made.py:129-137, :197-201): the net's and the blocks'
    `context_layer`s stay stock Linears; their outputs, zero-padded to 128 columns (the net's through its ReLU), enter as
    planes that the forward kernel adds to h_0 and to every a_k.  The backward pass is `MadeNet`'s: the gradient of
    block k's plane IS grads[2 k + 1], the initial plane's grads[0] (d loss / d hidden without a block) -- returned as
    views.  Arguments: inputs [B, D], masks, the number of blocks, the initial plane, one plane per block, then the
    parameters as `MadeNet` takes them."""

    @staticmethod
    def forward(ctx, x, masks, nb, initial_plane, *rest):
        from . import ops
        planes, params = rest[:nb], rest[nb:]
        assert (len(params) - 4) // 4 == nb
        blocks = [params[2 + 4 * k: 6 + 4 * k] for k in range(nb)]
        final = params[-2:]
        ctx.di, ctx.rows = x.shape[1], final[0].shape[0]
        ctx.nb, ctx.with_final, ctx.H = nb, True, params[0].shape[0]
        x = x.detach()
        if ctx.di % 4:
            x = torch.nn.functional.pad(x, (0, 4 - ctx.di % 4))
        out4 = (ctx.rows + 3) // 4 * 4
        fwd_w, fwd_b, bwd_w, fbias = ops.pack_made_train(params[0], params[1], blocks, final, masks)
        hidden, saved, out, _ = ops.resnet_hidden_forward_ctx(ops.TRAIN_CTX_ADD, x, planes, fwd_w, fwd_b, nb, fbias, out4,
                                                              initial_plane=initial_plane)
        ctx.save_for_backward(x.contiguous(), saved, bwd_w, hidden, final[0], *masks)
        return out if out4 == ctx.rows else out[:, :ctx.rows]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        from . import ops
        x, saved, bwd_w, hidden, w_f = ctx.saved_tensors[:5]
        masks = ctx.saved_tensors[5:]
        rows, pad, nb = ctx.rows, -ctx.rows % 4, ctx.nb
        if pad:
            g_out = torch.nn.functional.pad(g_out, (0, pad))

        def masked_final():
            w = w_f if masks[-1] is None else w_f * masks[-1]
            return torch.nn.functional.pad(w, (0, 0, 0, pad)) if pad else w

        context = dict(mode=ops.TRAIN_CTX_ADD, planes=(), pre=None, first_param=4 + nb)
        grads = list(_resnet_hidden_backward(ctx, g_out, (x, saved, bwd_w, hidden, masked_final), context))
        if pad:
            grads[-2] = None if grads[-2] is None else grads[-2][:rows].contiguous()
            grads[-1] = None if grads[-1] is None else grads[-1][:rows].contiguous()
        pairs = [(g, m) for g, m in zip(grads[2::2], masks) if g is not None and m is not None]
        if pairs:
            torch._foreach_mul_([g for g, _ in pairs], [m for _, m in pairs])
        g_all = context["grads"]
        g_initial = g_all[0] if nb else context["g_hidden"]
        return (grads[0], None, None, g_initial) + tuple(g_all[2 * k + 1] for k in range(nb)) + tuple(grads[2:])


def _dense_rows(t, n, width):
    return t.detach().reshape(n, width).contiguous()


class LinearSpline(torch.autograd.Function):
    """K9 linear spline forward + `nfa_linear_spline_backward_f32`."""

    @staticmethod
    def forward(ctx, inputs, unnormalized_pdf, spec, inverse):
        from . import ops
        y, lad = ops._linear_spline_launch(inputs, unnormalized_pdf, spec, inverse)
        ctx.save_for_backward(inputs, unnormalized_pdf)
        ctx.spec, ctx.inverse = spec, bool(inverse)
        return y, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, g_lad):
        inputs, pdf = ctx.saved_tensors
        K = ctx.spec.num_bins
        n, dev = inputs.numel(), inputs.device
        x = inputs.detach().contiguous().view(-1)
        rows = _dense_rows(pdf, n, K)
        g_y = torch.zeros_like(x) if g_y is None else g_y.contiguous().view(-1)
        g_lad = None if g_lad is None else g_lad.contiguous().view(-1)
        g_in, g_rows = torch.empty_like(x), torch.empty_like(rows)
        with torch.cuda.device(dev):
            rc = N.load().nfa_linear_spline_backward_f32(
                N.ptr(x), N.ptr(rows), N.ptr(g_y), N.ptr(g_lad), N.ptr(g_in), N.ptr(g_rows), n,
                ctypes.byref(ctx.spec), int(ctx.inverse), N.stream_handle(dev))
        N.check(rc)
        return g_in.view(inputs.shape), g_rows.view(pdf.shape), None, None


class QuadraticSpline(torch.autograd.Function):
    """K9 quadratic spline forward + `nfa_quadratic_spline_backward_f32`."""

    @staticmethod
    def forward(ctx, inputs, unnormalized_widths, unnormalized_heights, spec, inverse):
        from . import ops
        y, lad = ops._quadratic_spline_launch(inputs, unnormalized_widths, unnormalized_heights, spec, inverse)
        ctx.save_for_backward(inputs, unnormalized_widths, unnormalized_heights)
        ctx.spec, ctx.inverse = spec, bool(inverse)
        return y, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, g_lad):
        inputs, uw, uh = ctx.saved_tensors
        K, nh = ctx.spec.num_bins, uh.shape[-1]
        n, dev = inputs.numel(), inputs.device
        x = inputs.detach().contiguous().view(-1)
        w_rows, h_rows = _dense_rows(uw, n, K), _dense_rows(uh, n, nh)
        g_y = torch.zeros_like(x) if g_y is None else g_y.contiguous().view(-1)
        g_lad = None if g_lad is None else g_lad.contiguous().view(-1)
        g_in, g_w, g_h = torch.empty_like(x), torch.empty_like(w_rows), torch.empty_like(h_rows)
        with torch.cuda.device(dev):
            rc = N.load().nfa_quadratic_spline_backward_f32(
                N.ptr(x), N.ptr(w_rows), N.ptr(h_rows), nh, N.ptr(g_y), N.ptr(g_lad), N.ptr(g_in), N.ptr(g_w),
                N.ptr(g_h), n, ctypes.byref(ctx.spec), int(ctx.inverse), N.stream_handle(dev))
        N.check(rc)
        return g_in.view(inputs.shape), g_w.view(uw.shape), g_h.view(uh.shape), None, None


class CubicSpline(torch.autograd.Function):
    """K9 cubic spline forward + `nfa_cubic_spline_backward_f32`."""

    @staticmethod
    def forward(ctx, inputs, uw, uh, udl, udr, spec, inverse):
        from . import ops
        y, lad = ops._cubic_spline_launch(inputs, uw, uh, udl, udr, spec, inverse)
        ctx.save_for_backward(inputs, uw, uh, udl, udr)
        ctx.spec, ctx.inverse = spec, bool(inverse)
        return y, lad

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y, g_lad):
        inputs, uw, uh, udl, udr = ctx.saved_tensors
        K = ctx.spec.num_bins
        n, dev = inputs.numel(), inputs.device
        x = inputs.detach().contiguous().view(-1)
        w_rows, h_rows = _dense_rows(uw, n, K), _dense_rows(uh, n, K)
        l_rows, r_rows = _dense_rows(udl, n, 1), _dense_rows(udr, n, 1)
        g_y = torch.zeros_like(x) if g_y is None else g_y.contiguous().view(-1)
        g_lad = None if g_lad is None else g_lad.contiguous().view(-1)
        g_in, g_w, g_h = torch.empty_like(x), torch.empty_like(w_rows), torch.empty_like(h_rows)
        g_l, g_r = torch.empty_like(l_rows), torch.empty_like(r_rows)
        with torch.cuda.device(dev):
            rc = N.load().nfa_cubic_spline_backward_f32(
                N.ptr(x), N.ptr(w_rows), N.ptr(h_rows), N.ptr(l_rows), N.ptr(r_rows), N.ptr(g_y), N.ptr(g_lad),
                N.ptr(g_in), N.ptr(g_w), N.ptr(g_h), N.ptr(g_l), N.ptr(g_r), n, ctypes.byref(ctx.spec),
                int(ctx.inverse), N.stream_handle(dev))
        N.check(rc)
        return (g_in.view(inputs.shape), g_w.view(uw.shape), g_h.view(uh.shape), g_l.view(udl.shape),
                g_r.view(udr.shape), None, None)
