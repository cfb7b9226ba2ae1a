"""Elastic loss-aware quantisation (reference: QuantTorch/functions/elastic_quant_connect.py): the weight keeps full precision in
training and its gradient carries a "sawtooth" regulariser that pulls every weight towards the nearest level of a linear
(``lin_*``) or geometric (``exp_*``) set; inference projects the weight onto the set.

Device fp32 tensors run on two HIP kernels (csrc/loss_quant.hip): ``qt_level_project_f32`` for the projections and
``qt_weight_reg_f32`` for the regularisers, which evaluates a whole sawtooth (or two of them, subtracted from a gradient) in one
pass.  The sawtooth is described on the host as a table of terms, one per (level, interval) of the reference's loops, in their
order: ``res +-= (V(x) * [x op1 t1]) * [x op2 t2]``.  The thresholds and constants are formed in Python double from the same
expressions as upstream and rounded to fp32 once, which is what torch does with a Python scalar, so the kernel's results are the
reference's bit for bit.  CPU tensors (and tables past the kernel's capacity) evaluate the same table with torch operations.

Coefficients (``alpha``, ``beta``) are Python numbers or 1-element tensors (the layers' buffers, read on the device without a host
readback).  The two forms round ``(-c) * alpha`` differently upstream — double product vs fp32 product — and both are reproduced.

``QuantConv2d`` here is the deprecated Elastic conv op.  At package level ``functions.QuantConv2d`` stays the DoReFa one; upstream
the Elastic one shadows it there (QuantTorch/functions/__init__.py).  Reach this one through this module or ``ElasticNet``.
"""
import functools
import numbers
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from . import _fused
from .common import QtFunction, front  # noqa: F401  (front: re-exported like upstream)
from ..device import device  # noqa: F401

# term kinds and comparison codes of qt_reg_term (include/qt_hip.h)
L2_LIN, L2_EXP, L1, WQR_LIN, WQR_EXP_POS, WQR_EXP_NEG = range(6)
LT, LE, GT, GE = range(4)
_SUB = 1 << 8


def _f32(v) -> float:
    """A Python scalar as torch rounds it when it meets an fp32 tensor."""
    return float(np.float32(v))


def _table(rows):
    """[(kind, op1, t1, op2, t2, c, subtract)] -> int32 [n, 4] qt_reg_term array (floats stored as their bit patterns)."""
    t = np.zeros((len(rows), 4), np.float32)
    codes = np.zeros(len(rows), np.int32)
    for i, (kind, op1, t1, op2, t2, c, sub) in enumerate(rows):
        codes[i] = kind | (op1 << 4) | (op2 << 6) | (_SUB if sub else 0)
        t[i, 1:] = (_f32(t1), _f32(t2), _f32(c))
    out = t.view(np.int32)
    out[:, 0] = codes
    out.setflags(write=False)
    return out


def _coef_key(a):
    """Cache key of a coefficient: the tensor form only changes lin_l2's constant (fl(-c) instead of the double product)."""
    if isinstance(a, torch.Tensor):
        return "tensor"
    if not isinstance(a, numbers.Number):
        raise TypeError(f"coefficient: expected a number or a tensor, got {type(a)}")
    return float(a)


@functools.lru_cache(maxsize=256)
def lin_l2_terms(coef, top, bottom, size):
    delta = (top - bottom) / (size - 1)
    rows = []
    for i in range(size):
        c = bottom + i * delta
        k = -1 * c if coef == "tensor" else -1 * c * coef       # alpha*x + -1*(c)*alpha
        rows.append((L2_LIN, LE, c + delta / 2, GT, c - delta / 2, k, False))
    return _table(rows)


@functools.lru_cache(maxsize=256)
def exp_l2_terms(gamma, init, size):
    rows = [(L2_EXP, GT, 0, LE, (init * gamma + init) / 2, init, False),
            (L2_EXP, LE, 0, GT, (-init * gamma + -init) / 2, -init, False)]       # alpha*(x + init) = alpha*(x - (-init))
    cur = init
    for _ in range(size - 1):
        previous = cur
        cur *= gamma
        rows.append((L2_EXP, GT, (cur + previous) / 2, LE, (cur + gamma * cur) / 2, cur, False))
        rows.append((L2_EXP, LT, (-cur + -previous) / 2, GT, (-cur + -gamma * cur) / 2, -cur, False))
    return _table(rows)


@functools.lru_cache(maxsize=256)
def lin_l1_terms(top, bottom, size):
    delta = (top - bottom) / (size - 1)
    rows = []
    for i in range(size):
        c = bottom + i * delta
        rows.append((L1, LE, c + delta / 2, GT, c, 0, False))
        rows.append((L1, LT, c, GT, c - delta / 2, 0, True))
    return _table(rows)


@functools.lru_cache(maxsize=256)
def exp_l1_terms(gamma, init, size):
    rows = [(L1, GT, 0, LT, init, 0, True),
            (L1, GT, init, LE, (init * gamma + init) / 2, 0, False),
            (L1, LE, 0, GT, -init, 0, False),
            (L1, LT, -init, GT, (-init * gamma - init) / 2, 0, True)]
    cur = init
    for _ in range(size - 1):
        previous = cur
        cur *= gamma
        rows.append((L1, GT, (cur + previous) / 2, LT, cur, 0, True))
        rows.append((L1, GT, cur, LE, (cur + cur * gamma) / 2, 0, False))
        rows.append((L1, LE, -((+cur + previous) / 2), GT, -cur, 0, False))
        rows.append((L1, LT, -cur, GT, (-cur - cur * gamma) / 2, 0, True))
    return _table(rows)


def _decode(table):
    f = table.view(np.float32)
    for code, (t1, t2, c) in zip(table[:, 0].tolist(), f[:, 1:].tolist()):
        yield code & 15, (code >> 4) & 3, t1, (code >> 6) & 3, t2, c, bool(code & _SUB)


_CMP = {LT: torch.lt, LE: torch.le, GT: torch.gt, GE: torch.ge}


def reg_torch(x, table, a):
    """The sawtooth of ``table`` with coefficient ``a`` in torch operations, in the reference's operation order (the CPU path, and
    the device path of tables past the kernel's capacity)."""
    res = torch.zeros_like(x)
    for kind, op1, t1, op2, t2, c, sub in _decode(table):
        if kind == L2_LIN:
            v = a * x + (c * a if isinstance(a, torch.Tensor) else c)
        elif kind == L2_EXP:
            v = a * (x - c)
        elif kind == L1:
            v = a
        elif kind == WQR_LIN:
            v = a * (torch.sign(x) * torch.abs(x - c) + torch.abs(x) * torch.sign(x - c))
        elif kind == WQR_EXP_POS:
            v = a * (torch.sign(x) * torch.abs(x - c) + torch.abs(x))
        else:
            v = a * (torch.sign(x) * torch.abs(x - c) - torch.abs(x))
        v = v * _CMP[op1](x, t1).float() * _CMP[op2](x, t2).float()
        if sub:
            res -= v
        else:
            res += v
    return res


def _coef_on_device(a, x) -> bool:
    if isinstance(a, torch.Tensor):
        return a.numel() == 1 and a.dtype == torch.float32 and a.device == x.device and a.dim() <= max(x.dim(), 1)
    return isinstance(a, numbers.Number)


def _hip(x, *coefs) -> bool:
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 1
            and all(_coef_on_device(a, x) for a in coefs))


def apply_reg(x, table, a):
    """R(x) alone (the public ``*_deriv_*`` functions)."""
    if _hip(x, a) and len(table) <= ops.REG_TERMS_MAX:
        return ops.weight_reg(x, None, table, a)
    return reg_torch(x, table, a)


def regularised_grad(grad, w, table1, a1, table2, a2):
    """(grad - R1(w)) - R2(w): ONE kernel launch on the device (the gradient of QuantWeight* and of the dense ops' weight and bias)."""
    if _hip(w, a1, a2) and isinstance(grad, torch.Tensor) and grad.is_cuda and grad.dtype == torch.float32 \
            and grad.shape == w.shape and len(table1) + len(table2) <= ops.REG_TERMS_MAX:
        return ops.weight_reg(w.detach(), grad, table1, a1, table2, a2)
    g = grad.clone()
    g -= reg_torch(w, table1, a1)
    g -= reg_torch(w, table2, a2)
    return g


# ---- projections ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=256)
def lin_levels(top, bottom, size):
    """torch.arange(bottom, top + step, step) in fp32 (its length can differ from ``size``)."""
    step = (top - bottom) / (size - 1)
    return tuple(torch.arange(bottom, top + step, step=step).tolist())


@functools.lru_cache(maxsize=256)
def exp_levels(gamma, init, size):
    """The 2*size table of exp_proj: init*gamma^k at positions size-1-k and size+k — positive only, as upstream."""
    s = torch.ones(size * 2)
    for index in range(size):
        s[size - 1 - index] = init * (gamma ** index)
        s[size + index] = init * (gamma ** index)
    return tuple(s.tolist())


def _proj_torch(x, levels):
    d = torch.abs(x.unsqueeze(-1) - levels)
    return levels[torch.argmin(d, dim=-1)]


def project(x, levels):
    """Projection of ``x`` onto a host level table (tuple of fp32 values)."""
    if _hip(x) and len(levels) <= ops.LEVELS_MAX:
        return ops.level_project(x, levels)
    return _proj_torch(x, torch.tensor(levels, dtype=torch.float32).to(x.device))


def _proj_val(x, set):
    """Projection of ``x`` onto the 1-D tensor ``set``: set[argmin_j |x - set_j|] (first index on ties, NaN wins)."""
    if _hip(x) and not set.is_cuda and set.dtype == torch.float32 and set.dim() == 1 and 0 < set.numel() <= ops.LEVELS_MAX:
        return ops.level_project(x, set.tolist())
    return _proj_torch(x, set.to(x.device))


def lin_proj(x, top=1, bottom=-1, size=5):
    return project(x, lin_levels(top, bottom, size))


def exp_proj(x, gamma=2, init=0.25, size=5):
    return project(x, exp_levels(gamma, init, size))


# ---- regularisers ----------------------------------------------------------------------------------------------------------------

def lin_deriv_l2(x, alpha, top=1, bottom=-1, size=5):
    """Sawtooth alpha*(x - c) on (c - delta/2, c + delta/2] around each of ``size`` levels c from bottom to top."""
    return apply_reg(x, lin_l2_terms(_coef_key(alpha), top, bottom, size), alpha)


def exp_deriv_l2(x, alpha, gamma=2, init=0.25, size=5):
    """Sawtooth alpha*(x -+ c) around the levels +-init*gamma^k, k < size."""
    return apply_reg(x, exp_l2_terms(gamma, init, size), alpha)


def lin_deriv_l1(x, beta, top=1, bottom=-1, size=5):
    """+-beta steps around each linear level (the L1 pull)."""
    return apply_reg(x, lin_l1_terms(top, bottom, size), beta)


def exp_deriv_l1(x, beta, gamma=2, init=0.25 / 2, size=5):
    """+-beta steps around each geometric level."""
    return apply_reg(x, exp_l1_terms(gamma, init, size), beta)


def QuantWeightLin(top=1, bottom=-1, size=5):
    """Identity on the weight; backward: g - lin_deriv_l2(w, alpha) - lin_deriv_l1(w, beta) (one kernel on the device)."""
    class _QuantWeightOp(QtFunction):
        @staticmethod
        def forward(ctx, weight, alpha, beta):
            ctx.save_for_backward(weight)
            ctx.coefs = (alpha, beta)
            return weight

        @staticmethod
        def backward(ctx, output_grad):
            weight, = ctx.saved_tensors
            alpha, beta = ctx.coefs
            return regularised_grad(output_grad, weight, lin_l2_terms(_coef_key(alpha), top, bottom, size), alpha,
                                    lin_l1_terms(top, bottom, size), beta), None, None
    return _QuantWeightOp


def QuantWeightExp(gamma=2, init=0.25, size=5):
    """Identity on the weight; backward: g - exp_deriv_l2(w, alpha) - exp_deriv_l1(w, beta)."""
    class _QuantWeightOp(QtFunction):
        @staticmethod
        def forward(ctx, weight, alpha, beta):
            ctx.save_for_backward(weight)
            ctx.coefs = (alpha, beta)
            return weight

        @staticmethod
        def backward(ctx, output_grad):
            weight, = ctx.saved_tensors
            alpha, beta = ctx.coefs
            return regularised_grad(output_grad, weight, exp_l2_terms(gamma, init, size), alpha,
                                    exp_l1_terms(gamma, init, size), beta), None, None
    return _QuantWeightOp


def _dense_real(input, weight) -> bool:
    return (input.is_cuda and input.dtype == torch.float32 and weight.dtype == torch.float32 and input.dim() == 2
            and input.numel() > 0)


def dense_op(terms):
    """y = F.linear(x, W, b) forward on the six-term real route; backward: grad_x and grad_W = g^T x on the same route, then
    grad_W and grad_b each get ONE regulariser launch: (grad - R1(.)) - R2(.).  ``terms(a1) -> (table1, table2)``."""
    class _QuantDense(QtFunction):
        @staticmethod
        def forward(ctx, input, weight, bias, c1, c2):
            ctx.has_bias = bias is not None
            ctx.coefs = (c1, c2)
            ctx.save_for_backward(input, weight, bias)
            if _dense_real(input, weight):
                return ops.real_linear(input.detach().contiguous(), weight.detach(), bias.detach() if bias is not None else None)
            _fused.note_library_path(input, "loss-aware dense op: a non-fp32 dtype")
            return F.linear(input, weight, bias)

        @staticmethod
        def backward(ctx, grad_output):
            input, weight, bias = ctx.saved_tensors
            c1, c2 = ctx.coefs
            grad_input = grad_weight = grad_bias = None
            if ctx.needs_input_grad[0]:
                grad_input = _fused.real_matmul(grad_output, weight)
            if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
                t1, t2 = terms(c1)
            if ctx.needs_input_grad[1]:
                grad_weight = regularised_grad(_fused.real_matmul(grad_output.t(), input), weight, t1, c1, t2, c2)
            if bias is not None and ctx.needs_input_grad[2]:
                grad_bias = regularised_grad(grad_output.sum(0).squeeze(0), bias, t1, c1, t2, c2)
            return grad_input, grad_weight, grad_bias, None, None
    return _QuantDense


def QuantLinDense(size=5, bottom=-1, top=1):
    """autograd.Function class: y = W.x + b with the linear L2 + L1 regulariser on grad_W and grad_b."""
    return dense_op(lambda a: (lin_l2_terms(_coef_key(a), top, bottom, size), lin_l1_terms(top, bottom, size)))


def QuantLogDense(gamma=2, init=0.25, size=5):
    """autograd.Function class: y = W.x + b with the geometric L2 + L1 regulariser on grad_W and grad_b."""
    return dense_op(lambda a: (exp_l2_terms(gamma, init, size), exp_l1_terms(gamma, init, size)))


def QuantConv2d(size=5, bottom=-1, top=1, stride=1, padding=1, dilation=1, groups=1):
    """**Deprecated** (as upstream): conv op whose weight and bias gradients carry the linear L2 + L1 regulariser.  Forward and
    both gradients on the real routes of ``_fused.RealConv2dFn`` (groups == 1, numeric padding), then one regulariser launch per
    parameter."""
    warnings.warn("Deprecated conv op ! Huge cuda memory consumption due to torch.grad.cuda_grad.conv2d_input function.",
                  DeprecationWarning, stacklevel=2)
    args = (stride, padding, dilation, groups)

    class _QuantConv2d(QtFunction):
        @staticmethod
        def forward(ctx, input, weight, bias, alpha, beta):
            ctx.coefs = (alpha, beta)
            ctx.bias_ref = bias
            ctx.real = (input.is_cuda and input.dtype == torch.float32 and weight.dtype == torch.float32 and input.dim() == 4
                        and input.numel() > 0 and groups == 1 and not isinstance(padding, str))
            if ctx.real:
                return _fused.RealConv2dFn.forward(ctx, input, weight, bias, args)
            ctx.has_bias = bias is not None
            ctx.save_for_backward(input, weight)
            _fused.note_library_path(input, "loss-aware conv op: groups, string padding or a non-fp32 dtype")
            return F.conv2d(input, weight, bias, stride, padding, dilation, groups)

        @staticmethod
        def backward(ctx, grad_output):
            alpha, beta = ctx.coefs
            if ctx.real:
                grad_input, grad_weight, grad_bias, _ = _fused.RealConv2dFn.backward(ctx, grad_output)
            else:
                input, weight = ctx.saved_tensors
                grad_input = grad_weight = grad_bias = None
                if ctx.needs_input_grad[0]:
                    grad_input = _fused.lib_conv2d_input(input.shape, weight, grad_output, stride, padding, dilation, groups)
                if ctx.needs_input_grad[1]:
                    grad_weight = _fused.lib_conv2d_weight(input, weight.shape, grad_output, stride, padding, dilation, groups)
                if ctx.has_bias and ctx.needs_input_grad[2]:
                    grad_bias = grad_output.sum((0, 2, 3))
            t1, t2 = lin_l2_terms(_coef_key(alpha), top, bottom, size), lin_l1_terms(top, bottom, size)
            if grad_weight is not None:
                grad_weight = regularised_grad(grad_weight, ctx.saved_tensors[1], t1, alpha, t2, beta)
            if grad_bias is not None:
                grad_bias = regularised_grad(grad_bias, ctx.bias_ref, t1, alpha, t2, beta)
            return grad_input, grad_weight, grad_bias, None, None

    return _QuantConv2d
