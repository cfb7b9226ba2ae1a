"""Independent reference for the depthwise convs (groups == in_channels, out_channels = m * in_channels): numpy only, nothing
of the package's ops is imported.

* ``forward`` / ``grad_input`` with ``dtype=np.float32`` restate the PINNED summation order of include/qt_hip.h "Depthwise
  convolution": the accumulator starts at +0, the taps are added in row-major (i, j') order — grad_input: the multiplier index
  outermost — with one float32 multiply and one float32 add each, taps outside the image are skipped, the bias comes last.  numpy
  rounds every elementwise product and sum once to the array's dtype, so these give the bits the kernels must give.
* The same functions with ``dtype=np.float64``, and ``grad_weight`` (always float64), are the exact-arithmetic side.
* ``grad_weight_bound``: 1.01 (L + 1) 2^-24 sum |go x| per element, the standard bound of an fp32 sum of L rounded products in any
  order (each product carries one rounding, each of the L - 1 additions one more: gamma_L <= 1.01 L u for L u < 0.01).

``cases()`` is the pruned grid the GPU tests walk: every feasible PAIR of edge conditions at least once.
"""
import itertools

import numpy as np

STE = np.float32(1.001)
KINDS = ("raw", "binary", "ternary")


def pairs(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def out_hw(H, W, kernel, stride, padding, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pairs(kernel), pairs(stride), pairs(padding), pairs(dilation)
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def quantize(w, kind):
    """The weight quantisers on a float32 array: safeSign (x < 0 ? -1 : +1, so -0.0 and NaN give +1) and the fixed ternary
    thresholds (w >= 0.5 -> +1, w < -0.5 -> -1, else 0; NaN -> +1 like the reference's double safeSign)."""
    w = np.asarray(w, dtype=np.float32)
    if kind == "raw":
        return w.copy()
    if kind == "binary":
        return np.where(w < 0, np.float32(-1), np.float32(1)).astype(np.float32)
    if kind == "ternary":
        t = np.where(w >= np.float32(0.5), 1.0, np.where(w < np.float32(-0.5), -1.0, 0.0))
        return np.where(np.isnan(w), 1.0, t).astype(np.float32)
    raise ValueError(kind)


def _taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
    """Per tap t = i kw + j', in row-major order: (t, ho, hi, wo, wi) — the output rows / columns whose tap lies inside the image
    and the input rows / columns it reads."""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pairs(kernel), pairs(stride), pairs(padding), pairs(dilation)
    ho, wo = np.arange(Ho), np.arange(Wo)
    for i in range(kh):
        hi = ho * sh - ph + i * dh
        mh = (hi >= 0) & (hi < H)
        for j in range(kw):
            wi = wo * sw - pw + j * dw
            mw = (wi >= 0) & (wi < W)
            if mh.any() and mw.any():
                yield i * kw + j, ho[mh][:, None], hi[mh][:, None], wo[mw][None, :], wi[mw][None, :]


def forward(x, wq, bias, kernel, stride, padding, dilation, dtype=np.float32):
    """y[n, c m + j] in the pinned order; ``wq`` [C m, kh, kw] is the already quantised weight."""
    x = np.asarray(x, dtype=dtype)
    N, C, H, W = x.shape
    Cout = wq.shape[0]
    m = Cout // C
    Ho, Wo = out_hw(H, W, kernel, stride, padding, dilation)
    w2 = np.asarray(wq, dtype=dtype).reshape(Cout, -1)
    xr = np.repeat(x, m, axis=1)                      # channel c m + j reads input channel c
    acc = np.zeros((N, Cout, Ho, Wo), dtype=dtype)
    for t, ho, hi, wo, wi in _taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
        acc[:, :, ho, wo] = acc[:, :, ho, wo] + xr[:, :, hi, wi] * w2[None, :, t, None, None]
    if bias is not None:
        acc = acc + np.asarray(bias, dtype=dtype)[None, :, None, None]
    return acc


def grad_input(go, wq, in_shape, kernel, stride, padding, dilation, dtype=np.float32):
    """gx[n, c] in the pinned order: multiplier index j outermost, taps row-major.  For one (j, tap) every input position receives
    at most one term, so the scatter below adds to each accumulator in exactly that order."""
    go = np.asarray(go, dtype=dtype)
    N, C, H, W = in_shape
    Cout = wq.shape[0]
    m = Cout // C
    Ho, Wo = go.shape[2], go.shape[3]
    w2 = np.asarray(wq, dtype=dtype).reshape(Cout, -1)
    gx = np.zeros((N, C, H, W), dtype=dtype)
    for j in range(m):
        gj, wj = go[:, j::m], w2[j::m]
        for t, ho, hi, wo, wi in _taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
            gx[:, :, hi, wi] = gx[:, :, hi, wi] + gj[:, :, ho, wo] * wj[None, :, t, None, None]
    return gx


def grad_weight(x, go, kernel, stride, padding, dilation):
    """(gw [C m, kh, kw], sum |go x| per element, grad_bias [C m]) in float64."""
    x, go = np.asarray(x, dtype=np.float64), np.asarray(go, dtype=np.float64)
    N, C, H, W = x.shape
    Cout, Ho, Wo = go.shape[1], go.shape[2], go.shape[3]
    m = Cout // C
    kh, kw = pairs(kernel)
    xr = np.repeat(x, m, axis=1)
    gw, ab = np.zeros((Cout, kh * kw)), np.zeros((Cout, kh * kw))
    for t, ho, hi, wo, wi in _taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
        p = go[:, :, ho, wo] * xr[:, :, hi, wi]
        gw[:, t] = p.sum((0, 2, 3))
        ab[:, t] = np.abs(p).sum((0, 2, 3))
    return gw.reshape(Cout, kh, kw), ab.reshape(Cout, kh, kw), go.sum((0, 2, 3))


def grad_weight_bound(abs_sum, L):
    return 1.01 * (L + 1) * 2.0 ** -24 * abs_sum


def ste_mask(gw, w, thr=STE):
    """gw where |w| <= thr (w the UNquantised float32 weight), 0 elsewhere; thr 0: no mask."""
    if not thr > 0:
        return gw
    return np.where(np.abs(np.asarray(w, dtype=np.float32)).reshape(gw.shape) > np.float32(thr), 0.0, gw)


# ---- data ------------------------------------------------------------------------------------------------------------------------

def _rng(seed):
    return np.random.RandomState(int(seed) & 0x7fffffff)


def pm1(seed, shape):
    return np.where(_rng(seed).rand(*shape) < 0.5, -1.0, 1.0).astype(np.float32)


def gauss6(seed, shape):
    """Gaussian values whose magnitudes span six decades."""
    r = _rng(seed)
    return (r.randn(*shape) * 10.0 ** r.uniform(-3.0, 3.0, size=shape)).astype(np.float32)


def small_ints(seed, shape, lo=-3, hi=3):
    return _rng(seed).randint(lo, hi + 1, size=shape).astype(np.float32)


def weights(seed, shape):
    """Real-valued weights around the quantisers' decision points: uniform in [-1.6, 1.6], so that safeSign, both ternary
    thresholds and the STE bound 1.001 all split them."""
    return _rng(seed).uniform(-1.6, 1.6, size=shape).astype(np.float32)


def grid_weights(seed, shape):
    """Weights in {-1, 0, +1}: fixed points of the ternary quantiser (and, without the zeros, of safeSign)."""
    return _rng(seed).randint(-1, 2, size=shape).astype(np.float32)


def tie_share(w):
    """Share of the entries of ``w`` that sit exactly on a decision point: |w| == 0.5 or |w| == float32(1.001)."""
    a = np.abs(np.asarray(w, dtype=np.float32))
    return float(((a == np.float32(0.5)) | (a == STE)).mean())


# ---- the case grid ---------------------------------------------------------------------------------------------------------------

CHANNELS = (1, 3, 64, 65, 130)
MULTIPLIERS = (1, 2, 3)
BATCHES = (1, 3)
KERNELS = ((1, 1), (3, 3), (5, 5), (7, 7), (3, 5))
STRIDES = ((1, 1), (2, 2), (2, 1))
PADDINGS = ("0", "1", "half", "(2,0)", "3@k3")
DILATIONS = ((1, 1), (2, 2))
MAPS = ((1, 1), (7, 7), (14, 9), (33, 65), (5, 130))
LAYOUTS = ("nchw", "channels_last")
MAC_BUDGET = 3_000_000       # multiply-accumulates per case: keeps every case, and its numpy reference, to a fraction of a second


def _padding(tag, kernel):
    if tag == "half":
        return (kernel[0] // 2, kernel[1] // 2)
    if tag == "3@k3":            # wider than the kernel's reach; defined for the 3 x 3 kernel only
        return (3, 3) if kernel == (3, 3) else None
    return {"0": (0, 0), "1": (1, 1), "(2,0)": (2, 0)}[tag]


class Case(dict):
    __getattr__ = dict.__getitem__

    @property
    def id(self):
        return "C{C}m{m}N{N}-k{kernel[0]}x{kernel[1]}-s{stride[0]}{stride[1]}-p{padding[0]}{padding[1]}-d{dilation[0]}-{H}x{W}-{layout}".format(**self)


def _feasible():
    out = []
    for C, m, N, k, s, ptag, d, (H, W), lay in itertools.product(CHANNELS, MULTIPLIERS, BATCHES, KERNELS, STRIDES, PADDINGS,
                                                                  DILATIONS, MAPS, LAYOUTS):
        p = _padding(ptag, k)
        if p is None:
            continue
        Ho, Wo = out_hw(H, W, k, s, p, d)
        if Ho < 1 or Wo < 1 or N * C * m * Ho * Wo * k[0] * k[1] > MAC_BUDGET:
            continue
        out.append((C, m, N, k, s, ptag, d, (H, W), lay))
    return out


def _pairs_of(combo):
    return {(a, combo[a], b, combo[b]) for a in range(len(combo)) for b in range(a + 1, len(combo))}


def cases(extra=64, seed=20261019):
    """A deterministic subset of the full grid that covers every feasible pair of factor values (greedy, seeded), plus ``extra``
    further combinations drawn at random."""
    combos = _feasible()
    rng = _rng(seed)
    todo = set()
    for c in combos:
        todo |= _pairs_of(c)
    chosen = []
    while todo:
        sample = [combos[i] for i in rng.randint(0, len(combos), size=400)]
        best = max(sample, key=lambda c: len(_pairs_of(c) & todo))
        gain = _pairs_of(best) & todo
        if not gain:
            # rare pairs: take any combination that holds one of them
            a, va, b, vb = next(iter(todo))
            best = next(c for c in combos if c[a] == va and c[b] == vb)
            gain = _pairs_of(best) & todo
        chosen.append(best)
        todo -= gain
    for i in rng.randint(0, len(combos), size=extra):
        if combos[i] not in chosen:
            chosen.append(combos[i])
    return [Case(C=C, m=m, N=N, kernel=k, stride=s, padding=_padding(ptag, k), dilation=d, H=H, W=W, layout=lay)
            for C, m, N, k, s, ptag, d, (H, W), lay in chosen]


def all_pairs_covered(case_list):
    """Every feasible pair of factor values occurs in ``case_list`` (what ``cases`` promises)."""
    want = set()
    for c in _feasible():
        want |= _pairs_of(c)
    have = set()
    for c in case_list:
        for t in PADDINGS:          # several tags can name one padding (e.g. "1" and "half" at 3 x 3): credit each
            if _padding(t, c.kernel) == c.padding:
                have |= _pairs_of((c.C, c.m, c.N, c.kernel, c.stride, t, c.dilation, (c.H, c.W), c.layout))
    return want <= have
