"""float64 restatement of ONE optimiser step from given fp32 state, and the bound an fp32 implementation has to meet.

The recurrences are those of torch.optim.SGD (dampening 0) and torch.optim.Adam (L2 weight decay, no amsgrad), evaluated in
float64 from the float32 values of p, g and the state (hyper-parameters as the Python floats the user wrote).  With
u = 2^-24 (the unit roundoff of fp32):

  SGD : |p - p64| <= 8 u S,   S = |p| + lr (1 + mu nesterov) (|mu b| + |g| + |wd p|);  buffer within 8 u (|mu b| + |g| + |wd p|)
  Adam: |p - p64| <= 16 u S,  S = |p| + (lr / bc1) Sm / denom,  Sm = |b1 m| + |(1 - b1) g| + |(1 - b1) wd p|;
        exp_avg within 16 u Sm;  exp_avg_sq within 16 u (|b2 v| + (1 - b2) (|g| + |wd p|)^2)

The constants are the numbers of fp32 roundings in each chain (hyper-parameters rounded to fp32 included), rounded up: at most 8
for SGD, at most 16 for Adam.  They are not tuned to any implementation; tests/test_optim_cpu.py pins them against torch's
own fp32 optimisers (which stay within 2.6 u S and 4.7 u S).
"""
import numpy as np

U = 2.0 ** -24
SGD_ROUNDINGS = 8
ADAM_ROUNDINGS = 16


def _f64(t):
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64)


def sgd_step(p, g, buf, lr, momentum=0.0, weight_decay=0.0, nesterov=False):
    """(p64, buf64 or None, bound_p, bound_buf or None) of one step; ``buf`` None = first step (buf = grad)."""
    p, g, buf = _f64(p), _f64(g), _f64(buf)
    d = g + weight_decay * p
    terms = np.abs(g) + np.abs(weight_decay * p)
    new_buf = bound_buf = None
    if momentum != 0:
        if buf is None:
            new_buf = d.copy()
        else:
            new_buf = momentum * buf + d
            terms = terms + np.abs(momentum * buf)
        bound_buf = SGD_ROUNDINGS * U * terms
        d = d + momentum * new_buf if nesterov else new_buf
    p64 = p - lr * d
    S = np.abs(p) + lr * (1.0 + momentum * bool(nesterov)) * terms
    return p64, new_buf, SGD_ROUNDINGS * U * S, bound_buf


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """(p64, m64, v64, bound_p, bound_m, bound_v) of step number ``step`` (1-based, counted after the increment)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    b1, b2 = betas
    d = g + weight_decay * p
    m64 = b1 * m + (1.0 - b1) * d
    v64 = b2 * v + (1.0 - b2) * d * d
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = np.sqrt(v64) / np.sqrt(bc2) + eps
    p64 = p - (lr / bc1) * m64 / denom
    Sm = np.abs(b1 * m) + np.abs((1.0 - b1) * g) + np.abs((1.0 - b1) * weight_decay * p)
    S = np.abs(p) + (lr / bc1) * Sm / denom
    bound_v = ADAM_ROUNDINGS * U * (np.abs(b2 * v) + (1.0 - b2) * (np.abs(g) + np.abs(weight_decay * p)) ** 2)
    return p64, m64, v64, ADAM_ROUNDINGS * U * S, ADAM_ROUNDINGS * U * Sm, bound_v


def worst(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0): <= 1 means every element lies within its bound."""
    err = np.abs(_f64(got) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def inputs(seed, shape, step=0):
    """The magnitudes the bound was pinned on: p spans 1e-4 ... 10, g spans 1e-6 ... 100 (both signs); every seventh gradient
    entry is zero on step 3.  float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    p = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 1, n)
    g = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 2, n)
    if step == 3:
        g[::7] = 0.0
    return p.astype(np.float32).reshape(shape), g.astype(np.float32).reshape(shape)
