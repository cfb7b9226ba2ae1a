"""Weighted quantisation regularisation, WQR (reference: QuantTorch/functions/WQR_connect.py; "WQR" of
https://publik.tuwien.ac.at/files/publik_275437.pdf): the Elastic family's L2 sawtooth replaced by the WQR term
kapa * (sign(x)|x - c| + |x| sign(x - c)), with the same L1 steps.  Same two kernels and term tables as
``elastic_quant_connect`` (see there).

Upstream quirks kept: ``exp_deriv_WQR``'s negative ``init`` branch tests ``x < 0 & x < -(init + init*gamma)/2`` (so its interval
is unbounded below and overlaps the loop's), and ``QuantWLogDense``'s backward uses ``gamma=2, init=0.25`` whatever it was built
with.  Fixed: ``QuantWeightWExp.backward`` returns three gradients (upstream two, for three inputs: a TypeError in backward).
"""
import functools

from .common import front  # noqa: F401  (re-exported like upstream)
from .elastic_quant_connect import (WQR_EXP_NEG, WQR_EXP_POS, WQR_LIN, GT, LT, QtFunction, _coef_key, _table, apply_reg,  # noqa: F401
                                    dense_op, exp_deriv_l1, exp_l1_terms, lin_deriv_l1, lin_l1_terms, regularised_grad)
from ..device import device  # noqa: F401


@functools.lru_cache(maxsize=256)
def lin_wqr_terms(top, bottom, size):
    delta = (top - bottom) / (size - 1)
    rows = []
    for i in range(size):
        c = bottom + i * delta
        rows.append((WQR_LIN, GT, c - delta / 2, LT, c + delta / 2, c, True))
    return _table(rows)


@functools.lru_cache(maxsize=256)
def exp_wqr_terms(gamma, init, size):
    rows = [(WQR_EXP_POS, GT, 0, LT, (init + init * gamma) / 2, init, True),
            (WQR_EXP_NEG, LT, 0, LT, (-init - init * gamma) / 2, -init, True)]     # sign(x)|x + init| + -1*|x|, upstream's mask
    cur = init
    for _ in range(size - 1):
        previous = cur
        cur *= gamma
        rows.append((WQR_EXP_POS, GT, (cur + previous) / 2, LT, (cur + cur * gamma) / 2, cur, True))
        rows.append((WQR_EXP_POS, LT, (-cur - previous) / 2, GT, (-cur - cur * gamma) / 2, -cur, True))
    return _table(rows)


def lin_deriv_WQR(x, kapa, top=1, bottom=-1, size=5):
    return apply_reg(x, lin_wqr_terms(top, bottom, size), kapa)


def exp_deriv_WQR(x, kapa, gamma=2, init=0.25 / 2, size=5):
    return apply_reg(x, exp_wqr_terms(gamma, init, size), kapa)


def _weight_op(tables):
    class _QuantWeightOp(QtFunction):
        @staticmethod
        def forward(ctx, weight, kapa, beta):
            ctx.save_for_backward(weight)
            ctx.coefs = (kapa, beta)
            return weight

        @staticmethod
        def backward(ctx, output_grad):
            weight, = ctx.saved_tensors
            kapa, beta = ctx.coefs
            t1, t2 = tables
            return regularised_grad(output_grad, weight, t1, kapa, t2, beta), None, None
    return _QuantWeightOp


def QuantWeightWLin(top=1, bottom=-1, size=5):
    """Identity on the weight; backward: g - lin_deriv_WQR(w, kapa) - lin_deriv_l1(w, beta) (one kernel on the device)."""
    return _weight_op((lin_wqr_terms(top, bottom, size), lin_l1_terms(top, bottom, size)))


def QuantWeightWExp(gamma=2, init=0.25, size=5):
    """Identity on the weight; backward: g - exp_deriv_WQR(w, kapa) - exp_deriv_l1(w, beta)."""
    return _weight_op((exp_wqr_terms(gamma, init, size), exp_l1_terms(gamma, init, size)))


def QuantWLinDense(size=5, bottom=-1, top=1):
    """autograd.Function class: y = W.x + b with the linear WQR + L1 regulariser on grad_W and grad_b."""
    return dense_op(lambda _k: (lin_wqr_terms(top, bottom, size), lin_l1_terms(top, bottom, size)))


def QuantWLogDense(gamma=2, init=0.25, size=5):
    """autograd.Function class: y = W.x + b with the geometric WQR + L1 regulariser; like upstream the backward uses gamma=2,
    init=0.25 whatever ``gamma`` / ``init`` were given."""
    return dense_op(lambda _k: (exp_wqr_terms(2, 0.25, size), exp_l1_terms(2, 0.25, size)))
