"""Exact float64 references for the XNOR-Net tap convs, shared by the tests (a plain module, not a conftest; nothing here imports
the package).  Every function works on any device and runs where its inputs live, chunked over images under a byte budget like
tests/_exact.py and tests/_grad_exact.py.

The layer computes  y = conv2d(x, sign(W) * alpha) + bias,  alpha = mean(|W|, (0, 1)): one scale per filter tap.  For +-1
activations that is  y = sum_t alpha_t D_t  with D_t the integer contraction over the input channels of tap t; the kernels form
it in Horner order on the fp32 accumulators (S_t = D_t + (alpha_{t-1} / alpha_t) S_{t-1}, y = alpha_{T-1} S_{T-1}).  The
references here are the defining sums: every D_t by an explicit unfold + matmul in float64 (exact integers), then
sum_t alpha_t [A] D_t in float64, taps in their natural order.

Designed operands make the comparison bit-exact: weights +-2^{e_t} give alpha_t = 2^{e_t}, so every Horner factor is a power of
two and every partial sum an integer multiple of the smallest term's quantum.  ``proves_exact_taps`` checks, for the actual
operands, that each partial sum S_t and the final y + bias stay below 2^24 quanta, i.e. are fp32 values whatever the order of the
additions inside a tap; a test demands bit equality only after that holds."""
import math

import torch
import torch.nn.functional as F

import _exact as X
import _grad_exact as G

F64, F32 = torch.float64, torch.float32
BUDGET = 1 << 30               # bytes of float64 temporaries per reference chunk

_pair = G._pair


def out_hw(H, W, kh, kw, stride=1, padding=0, dilation=1):
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def tap_alpha64(w: torch.Tensor) -> torch.Tensor:
    """alpha[kh * kw] = mean(|w|, (0, 1)) in float64, taps row-major."""
    return w.detach().to(F64).abs().mean(dim=(0, 1)).reshape(-1)


# ---- float64 references -------------------------------------------------------------------------------------------------------

def tap_sums64(x_pm1: torch.Tensor, sign_w: torch.Tensor, stride=1, padding=0, dilation=1, alpha=None, a_plane=None,
               budget: int = BUDGET) -> torch.Tensor:
    """The per-tap contractions D_t[n, co, ho, wo] = sum_ci x[n, ci, pixel(ho, wo, t)] sign_w[co, ci, t] in float64 (zero padding
    contributes 0; ``sign_w`` holds +-1 / 0, a zero weight being torch.sign's 0).  ``alpha`` None: D itself, [N, T, Cout, Ho, Wo].
    ``alpha`` [T]: sum_t alpha_t D_t -> [N, Cout, Ho, Wo]; with ``a_plane`` [N, H, W] as well: sum_t alpha_t A[pixel(m, t)] D_t."""
    N, C, H, W = (int(v) for v in x_pm1.shape)
    Cout, Cw, kh, kw = (int(v) for v in sign_w.shape)
    assert Cw == C
    T = kh * kw
    Ho, Wo = out_hw(H, W, kh, kw, stride, padding, dilation)
    geom = dict(dilation=_pair(dilation), padding=_pair(padding), stride=_pair(stride))
    w3 = sign_w.detach().to(F64).reshape(Cout, C, T)
    al = None if alpha is None else alpha.detach().to(F64).reshape(T).to(x_pm1.device)
    per_image = 8 * (C * T * Ho * Wo + C * H * W + (2 if al is not None else T + 1) * Cout * Ho * Wo + T * Ho * Wo)
    step = X.image_chunk(per_image, budget)
    out = torch.empty((N, Cout, Ho, Wo) if al is not None else (N, T, Cout, Ho, Wo), dtype=F64, device=x_pm1.device)
    for n0 in range(0, N, step):
        xs = x_pm1[n0:n0 + step].detach().to(F64)
        n = int(xs.shape[0])
        cols = F.unfold(xs, (kh, kw), **geom).reshape(n, C, T, Ho * Wo)
        ap = None
        if a_plane is not None:
            ap = F.unfold(a_plane[n0:n0 + n].detach().to(F64).unsqueeze(1), (kh, kw), **geom)      # [n, T, L], zero padded
        acc = torch.zeros((n, Cout, Ho * Wo), dtype=F64, device=xs.device) if al is not None else None
        for t in range(T):
            d = torch.matmul(w3[:, :, t], cols[:, :, t, :])                                          # [n, Cout, L]: exact integers
            if al is None:
                out[n0:n0 + n, t] = d.reshape(n, Cout, Ho, Wo)
                continue
            if ap is not None:
                d = d * ap[:, t, :].unsqueeze(1)
            acc += al[t] * d
        if al is not None:
            out[n0:n0 + n] = acc.reshape(n, Cout, Ho, Wo)
    return out


def _bias64(bias, like):
    return 0.0 if bias is None else bias.detach().to(F64).reshape(1, -1, 1, 1).to(like.device)


def xnor_conv64(x, w, bias=None, stride=1, padding=0, dilation=1, alpha=None, budget: int = BUDGET):
    """conv2d(x, sign(w) * mean(|w|, (0, 1)), bias) in float64 for a +-1 / 0 activation, alpha from ``w`` in float64 (or the
    designed ``alpha`` [T]), and the per-element magnitude bound  B = sum_t alpha_t (in-bounds, non-zero products of tap t) + |bias|.
    Returns (y, B), both [N, Cout, Ho, Wo]."""
    al = tap_alpha64(w) if alpha is None else alpha
    sw = torch.sign(w.detach())
    y = tap_sums64(x, sw, stride, padding, dilation, alpha=al, budget=budget) + _bias64(bias, x)
    B = tap_sums64(x.detach().abs(), sw.abs(), stride, padding, dilation, alpha=al, budget=budget)
    return y, B + (0.0 if bias is None else _bias64(bias, x).abs())


def xnor_rows64(x_sign, a_plane, w, bias=None, stride=1, padding=0, dilation=1, alpha=None, budget: int = BUDGET):
    """XNORConv2d(quant_input=True):  y[m, co] = sum_t alpha_t A[pixel(m, t)] D_t[m, co] + bias  from the sign image ``x_sign``
    (+-1, 0 where the pixel is all zero) and the per-pixel scale plane ``a_plane`` [N, H, W].  Returns (y, B) like xnor_conv64."""
    al = tap_alpha64(w) if alpha is None else alpha
    sw = torch.sign(w.detach())
    y = tap_sums64(x_sign, sw, stride, padding, dilation, alpha=al, a_plane=a_plane, budget=budget) + _bias64(bias, x_sign)
    B = tap_sums64(x_sign.detach().abs(), sw.abs(), stride, padding, dilation, alpha=al, a_plane=a_plane.detach().abs(), budget=budget)
    return y, B + (0.0 if bias is None else _bias64(bias, x_sign).abs())


def xnor_grad_input64(g, w, input_hw, stride=1, padding=0, alpha=None, bound: bool = True, budget: int = BUDGET):
    """grad wrt the input of conv2d(x, sign(w) * alpha): col2im((sign(w) alpha)^T . g) in float64, and the magnitude bound
    B = the same contraction of |g| with |sign(w)| alpha (None without ``bound``).  Returns (grad_x, B), both [N, Cin, H, W]."""
    al = tap_alpha64(w) if alpha is None else alpha.detach().to(F64)
    kh, kw = int(w.shape[2]), int(w.shape[3])
    wq = torch.sign(w.detach()).to(F64) * al.reshape(1, 1, kh, kw).to(w.device)
    gx = G.conv_grad_input64(g, wq, input_hw, stride, padding, budget=budget)
    if not bound:
        return gx, None
    return gx, G.conv_grad_input64(g.detach().abs(), wq.abs(), input_hw, stride, padding, budget=budget)


# ---- designed operands --------------------------------------------------------------------------------------------------------

def ramp_exps(T: int, span: int, base: int = 0):
    """Non-monotone tap exponents over ``span`` binades: a ramp from base up to base + span at tap (2 T) // 3, then a drop back
    to base + 1 at the last tap."""
    if T == 1:
        return [base]
    p = max(1, min(T - 2, (2 * T) // 3)) if T > 2 else 1
    up = [base + round(span * t / p) for t in range(p + 1)]
    down = [base + 1 + round((span - 1) * (T - 1 - t) / (T - p) * 0.5) for t in range(p + 1, T)]
    return up + down


def pow2_tap_weight(shape, tap_exps, seed: int, device, zero_taps=(), lone_zero=None) -> torch.Tensor:
    """Weights +-2^{e_t} (fair random signs): alpha_t = 2^{e_t} and every Horner factor a power of two.  ``zero_taps``: taps
    whose weights are all zero (alpha_t = 0); ``lone_zero``: one (co, ci, t) set to zero (sign 0; the caller then hands the
    designed alphas to the kernels, since mean(|w|) of that tap is no longer a power of two)."""
    Cout, Cin, kh, kw = (int(v) for v in shape)
    T = kh * kw
    assert len(tap_exps) == T
    s = G.pm1((Cout, Cin, T), seed, device, channels_last=False)
    e = torch.tensor([float(v) for v in tap_exps], dtype=F32, device=device)
    w = s * torch.exp2(e).reshape(1, 1, T)
    for t in zero_taps:
        w[:, :, int(t)] = 0.0
    if lone_zero is not None:
        w[lone_zero] = 0.0
    return w.reshape(Cout, Cin, kh, kw)


def designed_alpha(tap_exps, zero_taps=(), device="cpu") -> torch.Tensor:
    """The alphas pow2_tap_weight is designed for: 2^{e_t}, 0 for a zeroed tap (float64 [T])."""
    a = torch.tensor([0.0 if t in set(zero_taps) else 2.0 ** e for t, e in enumerate(tap_exps)], dtype=F64)
    return a.to(device)


def pow2_plane(shape, lo: int, hi: int, zero_frac: float, seed: int, device) -> torch.Tensor:
    """Per-pixel scale plane A[N, H, W] = 2^e, e uniform in [lo, hi] (both ends present), a share ``zero_frac`` of exact zeros
    (all-zero pixels)."""
    gen = G._gen(seed, device)
    e = torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=device)
    e.view(-1)[0], e.view(-1)[-1] = lo, hi
    a = torch.exp2(e.to(F32))
    if zero_frac:
        a = torch.where(torch.rand(tuple(shape), generator=gen, device=device) < zero_frac, 0.0, a)
    return a


def gauss_tap_weight(shape, seed: int, device, decades=None, tiny_tap=None) -> torch.Tensor:
    """N(0, 0.05) weights (nearly equal alphas); with ``decades`` each tap gets its own scale, log-uniform over that many
    decades, and ``tiny_tap`` (a tap index) is scaled by 2^-60 relative to the others."""
    Cout, Cin, kh, kw = (int(v) for v in shape)
    gen = G._gen(seed, device)
    w = torch.randn((Cout, Cin, kh * kw), generator=gen, device=device) * 0.05
    if decades:
        s = torch.pow(10.0, -decades * torch.rand((kh * kw,), generator=gen, device=device))
        s[0], s[-1] = 1.0, 10.0 ** -decades
        w = w * s.reshape(1, 1, -1)
    if tiny_tap is not None:
        w[:, :, int(tiny_tap)] *= 2.0 ** -60
    return w.reshape(Cout, Cin, kh, kw)


# ---- the exactness proof ------------------------------------------------------------------------------------------------------

def _pow2_exps(alpha):
    """Exponents of the non-zero entries of a power-of-two table (None for a zero entry); asserts that they are powers of two."""
    out = []
    for v in alpha.detach().to(F64).reshape(-1).tolist():
        if v == 0.0:
            out.append(None)
            continue
        m, e = math.frexp(v)
        assert m == 0.5, f"alpha {v!r} is not a power of two"
        out.append(e - 1)
    return out


def proves_exact_taps(alpha, count: int, bias=None, x_absmax: float = 1.0, x_quantum: int = 0, reverse: bool = False,
                      grad=None):
    """Proof that the Horner evaluation of  sum_t alpha_t D_t (+ bias)  is exact in fp32 whatever the order of the additions
    inside a tap.  ``alpha`` [T]: powers of two (0 = an all-zero tap) in the forward tap order, ``reverse`` for the flipped
    order of grad_x; ``count``: the most non-zero products one tap contributes to one output (Cin forward, Cout for grad_x);
    every product's other factor is an integer multiple of 2^x_quantum of magnitude <= x_absmax (1 and 0 for +-1 activations;
    the A plane's largest value and smallest exponent for the row-scaled conv; the gradient's for grad_x).
    After tap t the accumulator holds S_t = sum_{u <= t} (alpha_u / alpha_t) D_u: a multiple of the quantum
    2^{min_{u <= t} e_u + x_quantum - e_t} bounded by sum_{u <= t} 2^{e_u - e_t} count x_absmax; the condition is
    bound / quantum < 2^24 for every t, and for the final y + bias with the bias's own quantum, all inside the normal range.
    ``grad``: the gradient tensor of a grad_x case; its two-term fp16 split must reproduce it.  Returns (ok, reason)."""
    exps = _pow2_exps(alpha)
    if reverse:
        exps = exps[::-1]
    if grad is not None:
        _, ok = G.split_terms(grad, "f16x2")
        if not ok:
            return False, "the two-term fp16 split does not reproduce the gradient"
        q = G.quantum_exp(grad)
        if q is None:
            return True, "zero gradient"
        x_quantum, x_absmax = q, float(grad.detach().abs().max())
    mag, emin, worst, last = 0.0, None, 0.0, None
    for t, e in enumerate(exps):
        if e is None:
            continue
        mag += 2.0 ** e * count * x_absmax
        emin = e if emin is None else min(emin, e)
        unit = emin + x_quantum
        if unit - e < -126 or mag / 2.0 ** e >= 2.0 ** 127:
            return False, f"S_{t} leaves the normal fp32 range"
        r = mag / 2.0 ** unit
        if r >= 2.0 ** 24:
            return False, f"S_{t}: {r:.0f} quanta >= 2^24"
        worst, last = max(worst, r), e
    if last is None:
        return True, "every tap is zero"
    unit = emin + x_quantum
    if bias is not None and bool((bias != 0).any()):
        unit = min(unit, G.quantum_exp(bias))
        mag += float(bias.detach().abs().max())
    if unit < -126 or mag >= 2.0 ** 127:
        return False, "the result leaves the normal fp32 range"
    r = mag / 2.0 ** unit
    if r >= 2.0 ** 24:
        return False, f"y + bias: {r:.0f} quanta >= 2^24"
    return True, f"bound {max(worst, r):.0f} quanta < 2^24"


def max_span(T: int, count: int, x_absmax: float = 1.0, bias_quanta: int = 0, cap: int = 40) -> int:
    """The widest span of ramp_exps(T, span) that proves_exact_taps accepts for ``count`` products per tap of magnitude
    <= x_absmax quanta and a bias of up to ``bias_quanta`` quanta of the smallest tap."""
    best = 0
    for span in range(1, cap + 1):
        a = designed_alpha(ramp_exps(T, span))
        b = torch.tensor([float(bias_quanta)], dtype=F64) if bias_quanta else None
        if not proves_exact_taps(a, count, b, x_absmax)[0]:
            break
        best = span
    return best


def to_f32_exact(y64: torch.Tensor, what: str = "y") -> torch.Tensor:
    return G.to_f32_exact(y64, what)


# ---- per-element bound of the Gaussian cases ----------------------------------------------------------------------------------

def horner_bound(B: torch.Tensor, ksteps: int, taps: int) -> torch.Tensor:
    """|got - ref64| <= (S + 2 T + 16) 2^-23 B per output element: one accumulate rounding per MFMA k-step (S of them), one
    multiply per tap boundary plus the rounding of rho_t itself (2 T), the closing scale, the bias and the fp32 alpha sums
    (16); 2^-23 rather than 2^-24 allows for a truncating matrix-core accumulate."""
    return (ksteps + 2 * taps + 16) * 2.0 ** -23 * B


def worst_ratio(got: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf; a non-finite result as inf)."""
    err = (got.detach().to(F64) - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def value_report(got: torch.Tensor, want: torch.Tensor, what: str = "", limit: int = 8) -> str:
    """'' if got equals want bit for bit, else the count and the first mismatches ([n, c, y, x] indices)."""
    return G.mismatch_report(got, want, names=("n", "c", "y", "x")[:got.dim()], limit=limit, what=what)


# ---- the cases of tests/test_gpu_xnor_b256.py (the CPU module proves their designed operands exact) ---------------------------

BIAS_QUANTA = 8                # exact-case biases: integers in [-8, 8] times the smallest tap's alpha
A_EXPS = (-2, 2)               # exponents of the designed per-pixel scale plane
GRAD_AMP = 7                   # integer gradients in [-7, 7] times 2^exp
GRAD_EXPS = (-40, 30)
VARIANTS = ("plain", "mid", "lead", "lone")     # no zero / an all-zero tap in the middle / a leading one / a lone zero weight

# forward, exact: (id, B, Cin, Cout, H, k, stride, padding, dilation, variant, route of the float result, route of the threshold
# epilogues or None); routes as select_conv_taps (csrc/tile_select.h) selects them, asserted from the profiler's kernel names
FWD_CASES = [
    ("c256/valid", 8, 64, 256, 12, 3, 1, 0, 1, "mid", "ConvVPP256", "ConvVPP256"),
    ("c256/padded", 8, 64, 256, 12, 3, 1, 1, 1, "lead", "Conv128x128", "ConvPP256"),
    ("c192/valid", 8, 64, 192, 12, 3, 1, 0, 1, "lone", "ConvVPP256x192", "ConvVPP256x192"),
    ("c192/padded", 8, 64, 192, 12, 3, 1, 1, 1, "mid", "Conv128x128", "ConvPP256x192"),
    ("c200/valid", 8, 64, 200, 12, 3, 1, 0, 1, "lead", "ConvVPP256", "ConvVPP256"),
    ("c200/padded", 8, 64, 200, 12, 3, 1, 1, 1, "lone", "Conv128x128", "ConvPP256"),
    ("c128/valid", 8, 64, 128, 12, 3, 1, 0, 1, "mid", "ConvVPP128", "ConvVPP128"),
    ("c128/padded", 8, 64, 128, 12, 3, 1, 1, 1, "plain", "Conv128x128", "ConvPP128"),
    ("c64/valid", 8, 64, 64, 12, 3, 1, 0, 1, "lone", "ConvV64", "ConvV64"),
    ("c64/padded", 8, 64, 64, 12, 3, 1, 1, 1, "mid", "Conv128x128", "Conv64"),
    ("rows384/valid", 128, 64, 192, 27, 3, 1, 0, 1, "mid", "ConvVPP192", "ConvVPP192"),
    ("rows384/padded", 128, 64, 192, 27, 3, 1, 1, 1, "lead", "ConvPP192", "ConvPP192"),
    ("skinny/valid", 16, 512, 256, 10, 3, 1, 0, 1, "mid", "ConvVSkinny", "ConvVSkinny"),
    ("skinny/padded", 16, 512, 256, 10, 3, 1, 1, 1, "lone", "ConvSkinny", "ConvPP256"),
    ("v128x64", 64, 512, 256, 12, 3, 1, 0, 1, "lead", "ConvV128x64", "ConvV128x64"),
    ("v128x128", 64, 512, 512, 13, 3, 1, 0, 1, "mid", "ConvV128x128", "ConvV128x128"),
    # the padded ping-pong / 64-wide float instances need >= 200 tiles of 256 rows
    ("grid/pp256", 64, 64, 256, 30, 3, 1, 1, 1, "mid", "ConvPP256", None),
    ("grid/pp256x192", 64, 64, 192, 30, 3, 1, 1, 1, "lone", "ConvPP256x192", None),
    ("grid/pp128", 64, 64, 128, 30, 3, 1, 1, 1, "lead", "ConvPP128", None),
    ("grid/c64", 64, 64, 64, 30, 3, 1, 1, 1, "plain", "Conv64", None),
    # three k-steps per tap: boundaries alternate between the start and the middle of a 64-byte stage
    ("odd3/valid", 8, 192, 256, 12, 3, 1, 0, 1, "mid", "ConvVPP256", "ConvVPP256"),
    ("odd3/padded", 8, 192, 256, 12, 3, 1, 1, 1, "lone", "Conv128x128", "ConvPP256"),
    ("odd3/5x5/valid", 8, 192, 192, 13, 5, 1, 0, 1, "mid", "ConvVSkinny", "ConvVSkinny"),
    ("odd3/5x5/padded", 8, 192, 192, 13, 5, 1, 2, 1, "lead", "ConvSkinny", "ConvPP256x192"),
    ("odd9/valid", 8, 576, 256, 12, 3, 1, 0, 1, "lone", "ConvVSkinny", "ConvVSkinny"),
    ("odd9/padded", 8, 576, 256, 12, 3, 1, 1, 1, "mid", "ConvSkinny", "ConvPP256"),
    # other geometry, ragged sizes (M no multiple of a tile everywhere above; Cout = 72: no multiple of 32)
    ("1x1", 8, 64, 96, 11, 1, 1, 0, 1, "plain", "ConvVPP128", "ConvVPP128"),
    ("stride2", 8, 64, 128, 13, 3, 2, 1, 1, "mid", "Conv128x128", "ConvPP128"),
    ("aniso", 8, 64, 64, 12, 3, 1, (2, 1), 1, "lead", "Conv128x128", "Conv64"),
    ("dil2/valid", 8, 64, 256, 12, 3, 1, 0, 2, "lone", "ConvVPP256", "ConvVPP256"),
    ("dil2/padded", 8, 64, 256, 12, 3, 1, 2, 2, "mid", "Conv128x128", "ConvPP256"),
    ("cout72/valid", 8, 64, 72, 13, 3, 1, 0, 1, "mid", "ConvVPP128", "ConvVPP128"),
    ("cout72/padded", 8, 64, 72, 13, 3, 1, 1, 1, "lone", "Conv128x128", "ConvPP128"),
    # bench_models.alexnet_xnor conv2 .. conv5 at batch 256 (M = 186 624 and 43 264 rows)
    ("alexnet.conv2", 256, 192, 576, 27, 5, 1, 2, 1, "mid", "ConvPP192", "ConvPP192"),
    ("alexnet.conv3", 256, 576, 1152, 13, 3, 1, 1, 1, "lone", "ConvPP256x192", "ConvPP256x192"),
    ("alexnet.conv4", 256, 1152, 768, 13, 3, 1, 1, 1, "lead", "ConvPP256", "ConvPP256"),
    ("alexnet.conv5", 256, 768, 256, 13, 3, 1, 1, 1, "mid", "Conv128x128", "ConvPP256"),
]

# quant_input=True, Conv128<ElemFp4TapsRows>: (id, B, Cin, Cout, H, k, stride, padding)
ROWS_CASES = [
    ("tiny", 2, 64, 64, 5, 3, 1, 1),
    ("stride2", 4, 64, 96, 13, 3, 2, 1),
    ("5x5", 4, 64, 128, 12, 5, 1, 2),
    ("ragged", 3, 128, 200, 13, 3, 1, 1),
    ("alexnet.conv5", 256, 768, 256, 13, 3, 1, 1),
]

# grad_x, ElemF16Taps: (id, B, Cin, Cout, H, k, stride, padding, route of the transposed conv: its columns are Cin, its channels
# Cout, its padding k - 1 - padding — so padding = k - 1 reaches the un-padded configurations)
GRAD_CASES = [
    ("c128x128", 8, 64, 64, 12, 3, 1, 1, "Conv128x128"),
    ("skinny", 8, 64, 128, 12, 3, 1, 1, "ConvSkinny"),
    ("c64", 64, 64, 64, 30, 3, 1, 1, "Conv64"),
    ("pp128", 64, 128, 64, 30, 3, 1, 1, "ConvPP128"),
    ("pp192", 128, 192, 64, 27, 3, 1, 1, "ConvPP192"),
    ("pp256", 64, 256, 64, 30, 3, 1, 1, "ConvPP256"),
    ("pp256x192", 64, 192, 64, 30, 3, 1, 1, "ConvPP256x192"),
    ("v128x128", 32, 64, 128, 30, 3, 1, 2, "ConvV128x128"),
    ("v128x64", 32, 512, 128, 10, 3, 1, 2, "ConvV128x64"),
    ("v64", 8, 64, 64, 12, 3, 1, 2, "ConvV64"),
    ("vpp128", 8, 128, 64, 12, 3, 1, 2, "ConvVPP128"),
    ("vpp192", 128, 192, 64, 27, 3, 1, 2, "ConvVPP192"),
    ("vpp256", 8, 256, 64, 12, 3, 1, 2, "ConvVPP256"),
    ("vpp256x192", 8, 192, 64, 12, 3, 1, 2, "ConvVPP256x192"),
    ("vskinny", 8, 64, 128, 12, 3, 1, 2, "ConvVSkinny"),
    ("cout72", 8, 200, 72, 13, 3, 1, 1, "Conv128x128"),          # Cout % 8 == 0 but not % 64: nine k-steps per tap
    ("stride2", 8, 128, 128, 13, 3, 2, 1, "ConvSkinny"),         # the zero-dilated gradient
    ("alexnet.conv2", 256, 192, 576, 27, 5, 1, 2, "ConvPP192"),
    ("alexnet.conv3", 256, 576, 1152, 13, 3, 1, 1, "ConvPP256x192"),
    ("alexnet.conv4", 256, 1152, 768, 13, 3, 1, 1, "ConvPP256x192"),
    ("alexnet.conv5", 256, 768, 256, 13, 3, 1, 1, "ConvPP256"),
]


def case_seed(name: str) -> int:
    import zlib
    return zlib.crc32(name.encode()) % 10007


def tap_design(T: int, count: int, variant: str, x_absmax: float = 1.0, bias_quanta: int = BIAS_QUANTA, Cout: int = 1):
    """Tap exponents over the widest span the proof allows for the shape, the zeroed taps and the lone zero of ``variant``.
    Returns (tap_exps, zero_taps, lone_zero index or None)."""
    exps = ramp_exps(T, max_span(T, count, x_absmax, bias_quanta))
    if T == 1 or variant == "plain":
        return exps, (), None
    if variant == "mid":
        return exps, (T // 2,), None
    if variant == "lead":
        return exps, (0,), None
    assert variant == "lone", variant
    return exps, (), (Cout // 2, count // 3, T // 2)


def exact_bias(Cout: int, tap_exps, seed: int, device) -> torch.Tensor:
    """Integers in [-BIAS_QUANTA, BIAS_QUANTA] times the smallest tap's alpha."""
    q = torch.randint(-BIAS_QUANTA, BIAS_QUANTA + 1, (Cout,), generator=G._gen(seed, device), device=device).to(F32)
    return q * 2.0 ** min(tap_exps)
