"""Independent reference of the Lin / Log level chain, shared by the tests (a plain module, not a conftest): the quantisers restated
in plain torch from the formulas of functions/log_lin_connect.py, the one-term bf16 plane layout, and the chain

    conv -> + bias -> BatchNorm(eval) -> [ReLU] -> quantiser

with the conv in float64 on operands whose sums are exact in fp32 in any order.  Nothing here calls the package: no ops, no
HIP library, none of its quantisers.  Every function works on any device.

Lin (log_lin_connect.py:61-68), step = 2^(fsr - bits):  clamp(round(t / step) * step, 0, 2^fsr), with a sign bit
sign(t) * the same of |t|.  In fp32 every operation is exact or one IEEE rounding (step is a power of two), so the result is
defined bit for bit.  Log (:27-32):  [sign(t) *] 2^clamp(round(log2|t|), fsr - 2^bits, fsr).  The logarithm is evaluated in
float64 here and in fp32 (log2f) on the device, so where log2|t| sits within fp32 rounding of a half-integer the device may
land on the neighbouring level: ``log_ties`` marks those elements (|frac(log2|t|) - 1/2| < 2^-18, a few ulp of log2f for
|log2| <= 8), ``compare_levels`` lets them take either adjacent level and nothing else, and refuses a case in which more than
TIE_CAP of the elements are ties.  Lin comparisons exclude nothing.

torch.clamp is restated as a compare chain (NaN stays NaN, clamp(-0, 0, hi) stays -0): what ATen computes, without a
dependence on how a device's max instruction orders the two zeros.

Planes: a one-term bf16 plane holds the high half of each fp32 pattern, channels innermost, rows padded with zeros to a
``granule`` of 16 bytes (pixel planes, NHWC, optional zero halo of (hy, hx) pixels around every image) or 128 bytes (row
planes of the linear layers)."""
import torch
import torch.nn.functional as F

import _exact

TIE_WINDOW = 2.0 ** -18
TIE_CAP = 1e-4
NAN_FILL = 0x7FC1          # a bf16 NaN pattern no kernel writes: planes are pre-filled with it, an unwritten element shows up


# ---- quantisers ---------------------------------------------------------------------------------------------------------------

def _clamp(v, lo, hi):
    lo_t, hi_t = torch.full_like(v, lo), torch.full_like(v, hi)
    return torch.where(v < lo_t, lo_t, torch.where(v > hi_t, hi_t, v))


def lin_quant(t: torch.Tensor, fsr: int, bits: int, with_sign: bool) -> torch.Tensor:
    """LinQuant forward of an fp32 tensor, in fp32."""
    assert t.dtype == torch.float32
    step, top = 2.0 ** (fsr - bits), 2.0 ** fsr
    a = torch.abs(t) if with_sign else t
    q = _clamp(torch.mul(torch.round(torch.div(a, step)), step), 0.0, top)
    return torch.mul(torch.sign(t), q) if with_sign else q


def _pow2(e64: torch.Tensor) -> torch.Tensor:
    """2^e as fp32 for integer-valued float64 e (NaN stays NaN): ldexp, no transcendental."""
    nan = torch.isnan(e64)
    p = torch.ldexp(torch.ones_like(e64, dtype=torch.float32), torch.where(nan, torch.zeros_like(e64), e64).to(torch.int32))
    return torch.where(nan, torch.full_like(p, float("nan")), p)


def _log2_64(t):
    return torch.log2(torch.abs(t).to(torch.float64))


def log_quant(t: torch.Tensor, fsr: int, bits: int, with_sign: bool) -> torch.Tensor:
    """LogQuant forward of an fp32 tensor: the exponent from float64 log2 of the fp32 value."""
    assert t.dtype == torch.float32
    lo, hi = float(fsr - 2 ** bits), float(fsr)
    p = _pow2(_clamp(torch.round(_log2_64(t)), lo, hi))             # t = 0: -inf -> lo
    return torch.mul(torch.sign(t), p) if with_sign else p


def quantise(t, spec):
    dtype, fsr, bits, with_sign = spec
    return {"lin": lin_quant, "log": log_quant}[dtype](t, int(fsr), int(bits), bool(with_sign))


def log_ties(t: torch.Tensor, fsr: int, bits: int):
    """(tie mask, the other adjacent level as fp32 magnitude): finite non-zero t with lo - 1 < log2|t| < hi + 1 and log2|t| within
    TIE_WINDOW of a half-integer.  The other level is 2^clamp(e', lo, hi) with e' the neighbour round() did not choose."""
    lo, hi = float(fsr - 2 ** bits), float(fsr)
    l = _log2_64(t)
    ok = torch.isfinite(t) & (t != 0)
    l = torch.where(ok, l, torch.zeros_like(l))
    fl = torch.floor(l)
    tie = ok & (l > lo - 1) & (l < hi + 1) & (torch.abs((l - fl) - 0.5) < TIE_WINDOW)
    other = fl + (fl + 1) - torch.round(l)                           # floor + ceil - chosen (frac is near 1/2: ceil = floor + 1)
    return tie, _pow2(_clamp(other, lo, hi))


def compare_levels(got: torch.Tensor, t: torch.Tensor, spec, names=("n", "y", "x", "c"), what="", limit=8, cap=TIE_CAP):
    """``got`` (fp32, any shape) against quantise(t, spec), bit for bit; for Log, tie elements may hold the other adjacent level.
    Returns (ties, ties that took the other level, report) — report '' when equal, else the count and the first indices with
    the pre-quantiser value, _exact.mismatch_report style.  Asserts the tie share of the case against ``cap`` (TIE_CAP; only the
    helper's own unit test passes another)."""
    t = t.detach()
    want = quantise(t, spec)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    gi, wi = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    same = (gi == wi) | (torch.isnan(got) & torch.isnan(want))
    ties = moved = 0
    if spec[0] == "log":
        tie, other = log_ties(t, int(spec[1]), int(spec[2]))
        ties = int(tie.sum())
        assert ties <= cap * max(1, t.numel()), f"{what}: {ties} of {t.numel()} elements are log ties, over the cap {cap}"
        alt = torch.mul(torch.sign(t), other) if spec[3] else other
        took = tie & ~same & (gi == alt.contiguous().view(torch.int32))
        moved = int(took.sum())
        same = same | took
    bad = ~same
    cnt = int(bad.sum())
    if cnt == 0:
        return ties, moved, ""
    idx = bad.nonzero()[:limit].tolist()
    lines = [f"{what}: {cnt} of {bad.numel()} levels differ; first {len(idx)}:"]
    for ix in idx:
        pos = ", ".join(f"{n}={i}" for n, i in zip(names, ix))
        k = tuple(ix)
        lines.append(f"  ({pos}) got {float(got[k])!r} (0x{int(gi[k]) & 0xFFFFFFFF:08x}) want {float(want[k])!r} t={float(t[k])!r}")
    return ties, moved, "\n".join(lines)


# ---- plane codecs -------------------------------------------------------------------------------------------------------------

def plane_ld(C: int, granule: int = 16) -> int:
    """int16 elements per row of a one-term plane of C channels."""
    return (2 * int(C) + granule - 1) // granule * granule // 2


def bf16_exact(v: torch.Tensor) -> bool:
    """Every fp32 element has a zero low half (NaN included: its payload must sit in the high half)."""
    return not bool((v.contiguous().view(torch.int32) & 0xFFFF).any())


def encode_plane(y: torch.Tensor, halo=(0, 0), granule: int = 16) -> torch.Tensor:
    """fp32 [N, C, H, W] (any memory format) or [rows, C] of bf16-exact values -> int16 plane [N*(H+2hy)*(W+2hx), ld] / [rows, ld]."""
    assert y.dtype == torch.float32 and bf16_exact(y), "the values are not single bf16 terms"
    if y.dim() == 2:
        rows = y
        N = H = W = None
    else:
        N, C, H, W = (int(v) for v in y.shape)
        rows = y.permute(0, 2, 3, 1)
    C = int(rows.shape[-1])
    hi = (rows.contiguous().view(torch.int32) >> 16).to(torch.int16)
    ld = plane_ld(C, granule)
    if y.dim() == 2:
        out = torch.zeros((int(y.shape[0]), ld), dtype=torch.int16, device=y.device)
        out[:, :C] = hi
        return out
    hy, hx = (int(v) for v in halo)
    out = torch.zeros((N, H + 2 * hy, W + 2 * hx, ld), dtype=torch.int16, device=y.device)
    out[:, hy:hy + H, hx:hx + W, :C] = hi
    return out.view(-1, ld)


def decode_plane(plane: torch.Tensor, shape, halo=(0, 0), granule: int = 16, what="level plane") -> torch.Tensor:
    """int16 plane -> fp32 [N, H, W, C] of the interior (shape = (N, C, H, W)) or [rows, C] (shape = (rows, C)).  Asserts the
    plane's extent, that the pad channels and the halo are zero (a pre-filled NaN the launch did not overwrite fails here)."""
    if len(shape) == 2:
        R, C = (int(v) for v in shape)
        N, H, W, hy, hx = R, 1, 1, 0, 0
    else:
        N, C, H, W = (int(v) for v in shape)
        hy, hx = (int(v) for v in halo)
    ld = plane_ld(C, granule)
    assert plane.dtype == torch.int16 and tuple(plane.shape) == (N * (H + 2 * hy) * (W + 2 * hx), ld), \
        f"{what}: plane {tuple(plane.shape)} does not hold {tuple(shape)} with halo {(hy, hx)}"
    p = plane.view(N, H + 2 * hy, W + 2 * hx, ld)
    inner = p[:, hy:hy + H, hx:hx + W]
    pad = int(inner[..., C:].count_nonzero())
    assert pad == 0, f"{what}: {pad} pad-channel elements are not zero"
    border = int(p.count_nonzero()) - int(inner.count_nonzero())
    assert border == 0, f"{what}: {border} halo elements are not zero"
    v = (inner[..., :C].to(torch.int32) << 16).contiguous().view(torch.float32)
    return v.reshape(shape) if len(shape) == 2 else v


def nan_filled(rows: int, ld: int, device) -> torch.Tensor:
    """An output plane in which every element is the bf16 NaN pattern NAN_FILL."""
    return torch.full((int(rows), int(ld)), NAN_FILL, dtype=torch.int16, device=device)


# ---- designed operands --------------------------------------------------------------------------------------------------------
# Units of 2^-5: Lin activations m 2^-3 with 0 <= m <= 16 and Lin weights m 2^-2 with |m| <= 16 (the Lin(fsr=1, bits=4) /
# Lin(fsr=2, bits=4) levels), or Log activations +-2^e, e in [-3, 1], and Log weights +-2^e, e in [-2, 2]: |products| <= 256
# units.  The three-term image plane: k 2^-4 with |k| <= 64 (one bf16 term each) against the Lin weights: |products| <= 1024
# units of 2^-6.  The bias is a multiple of 2^-5.  ``assert_exact_bound`` states why every partial sum is then an fp32
# value whatever the order: integers of units below 2^24.

def _gen(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


def designed_activation(kind: str, shape, seed: int, device) -> torch.Tensor:
    g = _gen(seed, device)
    if kind == "lin":
        return torch.randint(0, 17, tuple(shape), generator=g, device=device).float() * 2.0 ** -3
    if kind == "log":
        e = torch.randint(-3, 2, tuple(shape), generator=g, device=device).float()
        s = torch.where(torch.rand(tuple(shape), generator=g, device=device) < 0.5, -1.0, 1.0)
        return s * torch.exp2(e)
    if kind == "image":
        return torch.randint(-64, 65, tuple(shape), generator=g, device=device).float() * 2.0 ** -4
    raise ValueError(kind)


def designed_weight(kind: str, shape, seed: int, device) -> torch.Tensor:
    g = _gen(seed, device)
    if kind == "log":
        e = torch.randint(-2, 3, tuple(shape), generator=g, device=device).float()
        s = torch.where(torch.rand(tuple(shape), generator=g, device=device) < 0.5, -1.0, 1.0)
        return s * torch.exp2(e)
    return torch.randint(-16, 17, tuple(shape), generator=g, device=device).float() * 2.0 ** -2


def designed_bias(C: int, seed: int, device) -> torch.Tensor:
    return torch.randint(-40, 41, (int(C),), generator=_gen(seed, device), device=device).float() * 2.0 ** -5


def assert_exact_bound(x: torch.Tensor, w: torch.Tensor, bias=None, what=""):
    """Every product of an element of x and one of w, and every bias value, is an integer multiple of u = the smaller of (largest
    power of two dividing all of x) * (the same of w) and the largest power of two dividing the bias, and Cin kh kw max|x| max|w| +
    max|bias| < 2^24 u: every partial sum of the conv, in any order, with the bias added at any point, is an integer below 2^24
    in units of u — an fp32 value, no rounding.  Returns the bound in units of u."""
    def quantum(t):
        a = t.detach().double().abs().reshape(-1)
        a = a[a > 0]
        if a.numel() == 0:
            return None
        m, e = torch.frexp(a)
        M = torch.ldexp(m, torch.full_like(e, 53)).to(torch.int64)
        return int((e.to(torch.int64) - 53 + torch.log2((M & -M).double()).round().to(torch.int64)).min())
    qx, qw = quantum(x), quantum(w)
    if qx is None or qw is None:
        return 0.0
    u = qx + qw
    bound = int(w[0].numel()) * float(x.abs().max()) * float(w.abs().max())
    if bias is not None and quantum(bias) is not None:
        u = min(u, quantum(bias))
        bound += float(bias.abs().max())
    assert u >= -126, f"{what}: the unit 2^{u} is below the normal fp32 range"
    assert bound < 2.0 ** (24 + u), f"{what}: Cin k^2 max|x| max|w| + max|b| = {bound} >= 2^24 units of 2^{u}"
    return bound / 2.0 ** u


# ---- the chain ----------------------------------------------------------------------------------------------------------------

def exact_conv_f32(x: torch.Tensor, w: torch.Tensor, bias=None, stride=1, padding=0, budget: int = 1 << 29) -> torch.Tensor:
    """conv2d(x, w) + bias as fp32 [N, Cout, Ho, Wo]: float64 unfold + matmul (_exact.conv64) in image chunks, asserted to be
    fp32 values (assert_exact_bound must hold for the operands)."""
    assert_exact_bound(x, w, bias, "exact_conv_f32")
    N, C, H, W = (int(v) for v in x.shape)
    Cout, _, k, _ = (int(v) for v in w.shape)
    step = _exact.image_chunk(_exact.conv_bytes_per_image(C, H, W, Cout, k, stride, padding), budget)
    parts = []
    for n0 in range(0, N, step):
        acc = _exact.conv64(x[n0:n0 + step], w, stride, padding)
        if bias is not None:
            acc = acc + bias.double().view(1, -1, 1, 1)
        a32 = acc.float()
        assert torch.equal(a32.double(), acc), "the float64 sums are not fp32 values"
        parts.append(a32)
    return torch.cat(parts)


def chain_pre_quant(x, w, bias, bn, relu: bool, channels_last: bool, stride=1, padding=0) -> torch.Tensor:
    """t = [relu](F.batch_norm(conv + bias)) as fp32 [N, Cout, Ho, Wo] in the named memory format: torch's own BatchNorm and ReLU
    of the device the tensors live on, applied to the exact fp32 conv result."""
    y = exact_conv_f32(x, w, bias, stride, padding)
    y = y.contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    t = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    return torch.relu(t) if relu else t
