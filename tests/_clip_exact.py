"""float64 restatement of the global gradient norm, the clip coefficient and ONE clipped optimiser step, with the bounds an fp32
implementation has to meet.  Companion of _optim_exact.py; derived the same way, from the number of fp32 roundings, not from any
implementation's error.

The norm.  total = sum g^2 over every gradient, norm = sqrt(total), from the float32 gradients in float64.  An fp32 evaluation that
squares each element, adds non-negative terms along some chain and takes the square root of the sum has a relative error of at most
(number of roundings on its longest chain) u, u = 2^-24, since every term is non-negative (no cancellation) — and the square root
halves the error of its argument, which is ignored here.  The longest chain of the multi-tensor pass (csrc/optim_step.hip):

    1   the square of an element
   16   in-lane additions: a lane owns up to 16 elements of a 4096-element unit, 17 in a last unit whose numel % 4 tail falls to it
        (the first addition, to an accumulator of 0, is exact)
    7   the wave tree: four steps inside a row of 16 lanes, three additions of the four rows
    3   the four waves of a workgroup, added in order
    0   the units' partials are added in float64 (error ~ 2^-53 per addition: nothing at this scale)
    1   the conversion of the float64 square root to float32
    1   the square root itself, counted as a full rounding although it is evaluated in float64
   --
   29   rounded up: NORM_ROUNDINGS = 32.       |norm - norm64| <= 32 u norm64

The coefficient is not given a bound of its own: it is DEFINED as the fp32 expression min(1, max_norm / (norm + 1e-6)) of the fp32
norm (``coef_f32``: three roundings, each reproduced exactly), the expression torch.nn.utils.clip_grad_norm_ states.  (torch itself
evaluates ``max_norm / tensor`` as ``tensor.reciprocal() * max_norm``, one rounding more, so its coefficient may differ from the
division's in the last bit; a step is always checked with the coefficient its implementation used.)

The clipped step is the step of _optim_exact.py on the gradient g * coef, evaluated in float64 from the float32 g and the float32
coef the implementation used.  The implementation rounds that product once more: SGD_ROUNDINGS + 1 and ADAM_ROUNDINGS + 1.
(In exp_avg_sq the gradient enters squared, so the extra rounding counts twice there; that chain — g + wd p, the square, two
products, one sum, three rounded hyper-parameters — uses 10 of its 16 roundings, so 17 covers the 12.)
"""
import numpy as np

import _optim_exact as X

U = X.U
NORM_ROUNDINGS = 32
SGD_CLIP_ROUNDINGS = X.SGD_ROUNDINGS + 1
ADAM_CLIP_ROUNDINGS = X.ADAM_ROUNDINGS + 1


def total_norm(grads):
    """float64 L2 norm over all ``grads`` (float32 arrays or tensors)."""
    return float(np.sqrt(sum(float(np.sum(np.square(X._f64(g)))) for g in grads)))


def norm_bound(norm64):
    return NORM_ROUNDINGS * U * norm64


def coef64(norm64, max_norm):
    return min(1.0, max_norm / (norm64 + 1e-6))


def coef_f32(norm, max_norm):
    """The fp32 expression of clip_grad_norm_ on an fp32 ``norm``: max_norm / (norm + 1e-6) clamped to at most 1, one rounding per
    operation, NaN kept.  Returns a numpy float32."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if q > np.float32(1.0) else np.float32(q)


def sgd_step(p, g, buf, coef, lr, momentum=0.0, weight_decay=0.0, nesterov=False):
    """_optim_exact.sgd_step on g * coef: (p64, buf64 or None, bound_p, bound_buf or None) with the bounds of SGD_ROUNDINGS + 1."""
    p64, b64, bp, bb = X.sgd_step(p, X._f64(g) * float(coef), buf, lr, momentum, weight_decay, nesterov)
    k = SGD_CLIP_ROUNDINGS / X.SGD_ROUNDINGS
    return p64, b64, bp * k, None if bb is None else bb * k


def adam_step(p, g, m, v, coef, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """_optim_exact.adam_step on g * coef: (p64, m64, v64, bound_p, bound_m, bound_v) with the bounds of ADAM_ROUNDINGS + 1."""
    p64, m64, v64, bp, bm, bv = X.adam_step(p, X._f64(g) * float(coef), m, v, step, lr, betas, eps, weight_decay)
    k = ADAM_CLIP_ROUNDINGS / X.ADAM_ROUNDINGS
    return p64, m64, v64, bp * k, bm * k, bv * k
