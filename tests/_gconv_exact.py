"""Independent reference for the grouped convs with a few channels per group (x [N, G cin_g, H, W], w [G cout_g, cin_g, kh, kw]):
numpy only, nothing of the package's ops is imported.  The quantisers, the tap enumeration, the data generators and the summation
bound are those of tests/_dw_exact.py (pinned by tests/test_dw_exact_cpu.py); this file adds the sum over the group's channels.

* ``forward`` / ``grad_input`` with ``dtype=np.float32`` restate the PINNED summation order of include/qt_hip.h "Grouped
  convolution": the accumulator starts at +0; forward: the group's input channel ci ascending (outermost), then the taps in
  row-major order; grad_input: the group's output channel j ascending (outermost), then the taps; one float32 multiply and one
  float32 add per term, taps outside the image skipped, the bias last.  numpy rounds every elementwise product and sum once to the
  array's dtype, so these give the bits the kernels must give.
* The same functions with ``dtype=np.float64``, and ``grad_weight`` (always float64), are the exact-arithmetic side.
* ``grad_weight_bound``: 1.01 (L + 1) 2^-24 sum |go x| per element (the derivation is in tests/_dw_exact.py).

``cases()`` is the pruned grid the GPU tests walk: every feasible PAIR of edge conditions at least once.
"""
import itertools

import numpy as np

from _dw_exact import (STE, KINDS, pairs, out_hw, quantize, _taps, grad_weight_bound, ste_mask, _rng, pm1, gauss6, small_ints,  # noqa: F401
                       weights, grid_weights, tie_share)

MAX_CIN_G, MAX_TAPS, MAX_K = 32, 49, 512


def _dims(x_shape, w_shape, groups):
    N, C, H, W = x_shape
    Cout, cin_g = w_shape[0], w_shape[1]
    G = int(groups)
    assert C == G * cin_g and Cout % G == 0, (x_shape, w_shape, groups)
    return N, G, cin_g, Cout // G, Cout, H, W


def forward(x, wq, bias, groups, kernel, stride, padding, dilation, dtype=np.float32):
    """y[n, g cout_g + j] in the pinned order; ``wq`` [G cout_g, cin_g, kh, kw] is the already quantised weight."""
    x = np.asarray(x, dtype=dtype)
    N, G, cin_g, cout_g, Cout, H, W = _dims(x.shape, wq.shape, groups)
    Ho, Wo = out_hw(H, W, kernel, stride, padding, dilation)
    w3 = np.asarray(wq, dtype=dtype).reshape(Cout, cin_g, -1)
    first = (np.arange(Cout) // cout_g) * cin_g            # the first input channel of the group of every output channel
    acc = np.zeros((N, Cout, Ho, Wo), dtype=dtype)
    for ci in range(cin_g):
        xr = x[:, first + ci]
        for t, ho, hi, wo, wi in _taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
            acc[:, :, ho, wo] = acc[:, :, ho, wo] + xr[:, :, hi, wi] * w3[None, :, ci, t, None, None]
    if bias is not None:
        acc = acc + np.asarray(bias, dtype=dtype)[None, :, None, None]
    return acc


def grad_input(go, wq, in_shape, groups, kernel, stride, padding, dilation, dtype=np.float32):
    """gx[n, g cin_g + ci] in the pinned order: the group's output channel j outermost, taps row-major.  For one (j, tap) every
    input position receives at most one term, so the scatter below adds to each accumulator in exactly that order."""
    go = np.asarray(go, dtype=dtype)
    N, G, cin_g, cout_g, Cout, H, W = _dims(in_shape, wq.shape, groups)
    Ho, Wo = go.shape[2], go.shape[3]
    w4 = np.asarray(wq, dtype=dtype).reshape(G, cout_g, cin_g, -1)
    gx = np.zeros((N, G, cin_g, H, W), dtype=dtype)
    for j in range(cout_g):
        gj, wj = go[:, j::cout_g], w4[:, j]                # [N, G, Ho, Wo], [G, cin_g, taps]
        for t, ho, hi, wo, wi in _taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
            gx[:, :, :, hi, wi] = gx[:, :, :, hi, wi] + gj[:, :, None, ho, wo] * wj[None, :, :, t, None, None]
    return gx.reshape(N, G * cin_g, H, W)


def grad_weight(x, go, groups, cin_g, kernel, stride, padding, dilation):
    """(gw [G cout_g, cin_g, kh, kw], sum |go x| per element, grad_bias [G cout_g]) in float64."""
    x, go = np.asarray(x, dtype=np.float64), np.asarray(go, dtype=np.float64)
    N, C, H, W = x.shape
    Cout, Ho, Wo = go.shape[1], go.shape[2], go.shape[3]
    cout_g = Cout // int(groups)
    kh, kw = pairs(kernel)
    first = (np.arange(Cout) // cout_g) * cin_g
    gw, ab = np.zeros((Cout, cin_g, kh * kw)), np.zeros((Cout, cin_g, kh * kw))
    for ci in range(cin_g):
        xr = x[:, first + ci]
        for t, ho, hi, wo, wi in _taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
            p = go[:, :, ho, wo] * xr[:, :, hi, wi]
            gw[:, ci, t] = p.sum((0, 2, 3))
            ab[:, ci, t] = np.abs(p).sum((0, 2, 3))
    return gw.reshape(Cout, cin_g, kh, kw), ab.reshape(Cout, cin_g, kh, kw), go.sum((0, 2, 3))


# ---- the case grid ---------------------------------------------------------------------------------------------------------------

CIN_G = (1, 2, 3, 5, 16, 32)
COUT_G = (1, 3, 4, 17)
GROUPS = (1, 4, 5, 33)
BATCHES = (1, 3)
KERNELS = ((1, 1), (3, 3), (5, 5), (1, 3), (3, 1), (7, 7))
STRIDES = ((1, 1), (2, 2), (2, 1))
PADDINGS = ((0, 0), (1, 1), (3, 0))
DILATIONS = ((1, 1), (2, 2), (1, 2))
MAPS = ((5, 7), (9, 6), (4, 70))                # 70 columns: more than a wave of them
LAYOUTS = (("nchw", "nchw"), ("nchw", "channels_last"), ("channels_last", "nchw"), ("channels_last", "channels_last"))   # (x, y)
MAC_BUDGET = 3_000_000       # multiply-accumulates per case: keeps every case, and its numpy reference, to a fraction of a second
# K = cin_g kh kw exactly at the limit of 512 (no kernel of the grid reaches it), in both layouts of the result
K_LIMIT = ((32, 3, 4, 1, (4, 4), (1, 1), (1, 1), (1, 1), (5, 7), ("nchw", "channels_last")),
           (32, 17, 1, 3, (4, 4), (2, 1), (3, 0), (1, 1), (9, 6), ("channels_last", "nchw")))


class Case(dict):
    __getattr__ = dict.__getitem__

    @property
    def id(self):
        return ("g{G}i{cin_g}o{cout_g}N{N}-k{kernel[0]}x{kernel[1]}-s{stride[0]}{stride[1]}-p{padding[0]}{padding[1]}"
                "-d{dilation[0]}{dilation[1]}-{H}x{W}-{layout[0]}-{layout[1]}").format(**self)

    @property
    def geom(self):
        return self.kernel, self.stride, self.padding, self.dilation

    @property
    def shapes(self):
        """(x, w, y) shapes."""
        Ho, Wo = out_hw(self.H, self.W, *self.geom)
        return ((self.N, self.G * self.cin_g, self.H, self.W), (self.G * self.cout_g, self.cin_g) + tuple(self.kernel),
                (self.N, self.G * self.cout_g, Ho, Wo))


def _ok(combo):
    ci, co, G, N, k, s, p, d, (H, W), _lay = combo
    taps = k[0] * k[1]
    if taps > MAX_TAPS or ci * taps > MAX_K:
        return False
    Ho, Wo = out_hw(H, W, k, s, p, d)
    return Ho >= 1 and Wo >= 1 and N * G * co * Ho * Wo * ci * taps <= MAC_BUDGET


def _feasible():
    return [c for c in itertools.product(CIN_G, COUT_G, GROUPS, BATCHES, KERNELS, STRIDES, PADDINGS, DILATIONS, MAPS, LAYOUTS) if _ok(c)]


def _pairs_of(combo):
    return {(a, combo[a], b, combo[b]) for a in range(len(combo)) for b in range(a + 1, len(combo))}


def _case(combo):
    ci, co, G, N, k, s, p, d, (H, W), lay = combo
    return Case(cin_g=ci, cout_g=co, G=G, N=N, kernel=k, stride=s, padding=p, dilation=d, H=H, W=W, layout=lay)


def cases(extra=48, seed=20261020):
    """A deterministic subset of the full grid that covers every feasible pair of factor values (greedy, seeded), plus ``extra``
    further combinations drawn at random and the two K = 512 cases."""
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
            a, va, b, vb = next(iter(sorted(todo, key=repr)))
            best = next(c for c in combos if c[a] == va and c[b] == vb)
            gain = _pairs_of(best) & todo
        chosen.append(best)
        todo -= gain
    for i in rng.randint(0, len(combos), size=extra):
        if combos[i] not in chosen:
            chosen.append(combos[i])
    assert all(_ok(c) and c[0] * c[4][0] * c[4][1] == MAX_K for c in K_LIMIT)
    return [_case(c) for c in chosen + list(K_LIMIT)]


def all_pairs_covered(case_list):
    """Every feasible pair of factor values occurs in ``case_list`` (what ``cases`` promises)."""
    want = set()
    for c in _feasible():
        want |= _pairs_of(c)
    have = set()
    for c in case_list:
        have |= _pairs_of((c.cin_g, c.cout_g, c.G, c.N, c.kernel, c.stride, c.padding, c.dilation, (c.H, c.W), c.layout))
    return want <= have
