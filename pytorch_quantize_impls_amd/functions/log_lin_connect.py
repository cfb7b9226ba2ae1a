"""Lin / Log fixed-point quantisers of "Convolutional Neural Networks using Logarithmic Data Representation"
(reference: QuantTorch/functions/log_lin_connect.py).  HIP device tensors go through qt_lin_quantize_f32 /
qt_log_quantize_f32 — or, when the levels are single bf16 terms, qt_linlog_quantize_bf16_f32, which also writes the one-term
operand plane of the next Lin / Log layer; CPU tensors evaluate the same expressions in torch.

Upstream defect kept out: ``LinQuant(lin_back=False).backward`` calls ``torch.clamp(Tensor, int, Tensor)``
(log_lin_connect.py:79), which raises under torch 2.x; here it evaluates the expression that line intends,
sign(g) * clamp(round(g/step)*step, 0, 2^fsr) (note: negative g therefore yields -0).
"""
import torch

from .. import lazy, ops, packed
from .common import QtFunction, front


def _is_dev(t):
    return t.is_cuda and t.dtype == torch.float32


def _kernel_takes(fsr, bit_width, log):
    """Parameter window of qt_log_quantize_f32 / qt_lin_quantize_f32 (csrc/elementwise.hip); configurations outside it
    (e.g. a 32-bit Log quantiser) run the torch expression on the device, like the reference."""
    return -60 <= fsr <= 60 and 1 <= bit_width <= (16 if log else 32)


def _quantize_and_tag(input, dtype, fsr, bit_width, with_sign):
    """The quantiser on a device fp32 tensor.  When every level is one bf16 term (ops.levels_exact_in_bf16) and the one-term route
    is on, the same launch writes the plane the next Lin / Log layer contracts and parks it on the result (packed.attach_levels),
    the way BinaryConnect hands over its sign planes; the returned values are the same bits either way."""
    from . import _fused
    if (_fused._cfg("LOGLIN_ONE_TERM") and input.dim() >= 2 and ops.levels_exact_in_bf16(dtype, fsr, bit_width)
            and not isinstance(input, torch.nn.Parameter)):       # (a parameter is a weight: the layers pack it themselves)
        y, planes, layout = ops.quantize_levels_bf16(input, dtype, fsr, bit_width, with_sign)
        return y if planes is None else packed.attach_levels(y, planes, layout)
    if dtype == "log":
        return ops.log_quantize(input, fsr, bit_width, with_sign)
    return ops.lin_quantize(input, fsr, bit_width, 1 if with_sign else 0)


def _log_expr(x, fsr, bit_width, with_sign):
    p = torch.pow(torch.ones_like(x) * 2, torch.clamp(torch.round(torch.log2(torch.abs(x))), fsr - 2 ** bit_width, fsr))
    return torch.sign(x) * p if with_sign else p


def _lin_expr(x, fsr, bit_width, mode):
    step = torch.tensor([2.0], dtype=torch.float32, device=x.device).pow(fsr - bit_width)
    top = float(2.0 ** fsr)
    if mode == 1:
        return torch.sign(x) * torch.clamp(torch.round(torch.abs(x) / step) * step, 0, top)
    q = torch.clamp(torch.round(x / step) * step, 0, top)
    return q if mode == 0 else torch.sign(x) * q


def quantize_spec(input, spec):
    """The forward of LinQuant / LogQuant for ``spec`` = (dtype, fsr, bit_width, with_sign) on a plain tensor: what a quantiser
    recorded on a deferred chain (lazy.levels) evaluates when the chain materialises."""
    dtype, fsr, bit_width, with_sign = spec
    if dtype == "lin" and bit_width == 32:
        return input
    if _is_dev(input) and _kernel_takes(fsr, bit_width, dtype == "log"):
        return _quantize_and_tag(input, dtype, fsr, bit_width, with_sign)
    return _log_expr(input, fsr, bit_width, with_sign) if dtype == "log" else _lin_expr(input, fsr, bit_width, 1 if with_sign else 0)


def _apply_recording(cls, input):
    """``apply`` of the quantiser Functions: on a deferred Lin / Log chain (lazy.py, kind "levels") the quantiser is recorded."""
    if isinstance(input, lazy.LazyActivation):
        out = lazy.levels(input, cls._qt_level_spec)
        if out is not None:
            return out
    return super(cls, cls).apply(input)


def LogQuant(fsr=7, bit_width=3, with_sign=True, lin_back=True):
    """autograd.Function class: forward [sign(x) *] 2^clamp(round(log2|x|), fsr - 2^bit_width, fsr); backward the
    identity (lin_back) or the same quantiser applied to the gradient, signed (log_lin_connect.py:9-41)."""

    class _LogQuant(QtFunction):
        _qt_level_spec = ("log", fsr, bit_width, bool(with_sign))

        @classmethod
        def apply(cls, input):
            return _apply_recording(cls, input)

        @staticmethod
        def forward(ctx, input):
            if _is_dev(input) and _kernel_takes(fsr, bit_width, True):
                return _quantize_and_tag(input, "log", fsr, bit_width, with_sign)
            return _log_expr(input, fsr, bit_width, with_sign)

        @staticmethod
        def backward(ctx, grad_output):
            if lin_back:
                return grad_output.clone()
            if _is_dev(grad_output) and _kernel_takes(fsr, bit_width, True):
                return ops.log_quantize(grad_output, fsr, bit_width, True)
            return _log_expr(grad_output, fsr, bit_width, True)

    return _LogQuant


def LinQuant(fsr=7, bit_width=3, with_sign=True, lin_back=True):
    """autograd.Function class: forward [sign(x) *] clamp(round(|x| / step) * step, 0, 2^fsr), step = 2^(fsr - bit_width)
    (bit_width 32: identity); backward the identity (lin_back) or the quantised gradient (log_lin_connect.py:43-80)."""

    class _LinQuant(QtFunction):
        _qt_level_spec = ("lin", fsr, bit_width, bool(with_sign))

        @classmethod
        def apply(cls, input):
            return _apply_recording(cls, input)

        @staticmethod
        def forward(ctx, input):
            if bit_width == 32:
                return input
            if _is_dev(input) and _kernel_takes(fsr, bit_width, False):
                return _quantize_and_tag(input, "lin", fsr, bit_width, with_sign)
            return _lin_expr(input, fsr, bit_width, 1 if with_sign else 0)

        @staticmethod
        def backward(ctx, grad_output):
            if bit_width == 32 or lin_back:
                return grad_output.clone()
            if _is_dev(grad_output) and _kernel_takes(fsr, bit_width, False):
                return ops.lin_quantize(grad_output, fsr, bit_width, 2)
            return _lin_expr(grad_output, fsr, bit_width, 2)

    return _LinQuant


def nnQuant(dtype="lin", fsr=7, bit_width=3, with_sign=True, lin_back=True):
    """nn.Module front of LinQuant / LogQuant (log_lin_connect.py:84-100)."""
    if dtype == "lin":
        return front(LinQuant(fsr=fsr, bit_width=bit_width, with_sign=with_sign, lin_back=lin_back))
    elif dtype == "log":
        return front(LogQuant(fsr=fsr, bit_width=bit_width, with_sign=with_sign, lin_back=lin_back))
    raise RuntimeError("Only 'log' and 'lin' dtype are supported !")


def Quant(input, dtype="lin", fsr=7, bit_width=3, with_sign=True, lin_back=True):
    """Functional form (log_lin_connect.py:103-118)."""
    if dtype == "lin":
        return LinQuant(fsr=fsr, bit_width=bit_width, with_sign=with_sign, lin_back=lin_back).apply(input)
    elif dtype == "log":
        return LogQuant(fsr=fsr, bit_width=bit_width, with_sign=with_sign, lin_back=lin_back).apply(input)
    raise RuntimeError("Only 'log' and 'lin' dtype are supported !")
