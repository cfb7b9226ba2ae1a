"""Exact reference for the DoReFa int8 code kernels (the C4 inference chain), shared by the tests (a plain module, not a conftest).

Plain torch on any device, float64 arithmetic, nothing of the package's ops: the conv of int8 codes with +-1 weights is an integer
sum below 2^24 (conv64 of tests/_exact.py, checked against that bound), and the code epilogue is evaluated with ONE correctly
rounded fp32 result per kernel operation, in the kernels' order (csrc/mfma_gemm_kernel.h mode 2 and ElemI8::out, csrc/code_conv3x3.hip,
csrc/codes_i8.hip affine_codes_word; all compiled with -ffp-contract=off):

    v = fl(float(acc) * scale)  [v = fl(v + conv_bias)]              scale = fl(scale_host * scale_dev)
    v = max(v, 0)                                                      relu == 2 ("pre")
    t = fma(fl(fl(v - mean) * rs), weight, bias)                       device BatchNorm form
    t = fl(fl(v * alpha) + beta)                                       folded form
    t = fl(t + u)  |  fl(t + fl(fl(u * ra) + rb))  |  fl(t + fma(fl(fl(u - rmean) * rrs), rw, rb))      fp32 residual
    t = fl(t + fl(rscale * rc))                                        code residual
    t = max(t, 0)                                                      relu == 1
    q = rint(fl(levels * t)), half to even;  |q| > 127 or NaN -> code 0 and the range flag

Each step is formed in float64 and rounded to fp32 once.  For + - * that is the correctly rounded fp32 result (the product of two
fp32 values is exact in float64; a float64 sum rounded again to fp32 cannot double-round: 53 >= 2 * 24 + 2).  The fma is
(a * b) + c in float64, then .float().  That can double-round, but only where the float64 sum lies EXACTLY half way between two
neighbouring fp32 values while not being the exact sum (rounding to float64 is monotone, so it never carries a value across an
fp32 midpoint, only onto it).  Where the float64 sum is such a midpoint the correctly rounded fma is either the value the
reference took or its neighbour on the other side of the midpoint: one fp32 ulp lower or higher.  The reference follows both
through the rest of the chain and returns, per element, the smallest and the largest resulting code (``lo`` / ``hi``; equal to
``codes`` wherever the fma is unambiguous, in particular wherever it is exact).  They are the reference's own uncertainty, used
by ``compare_codes``' waiver rule for realistic parameters and nowhere else.

Code planes follow ops.CodePlanes: int8 [N * (H + 2hy) * (W + 2hx), ld] NHWC pixels, a zero border of (hy, hx) pixels around every
image, zero pad bytes past C."""
from dataclasses import dataclass
from typing import Optional

import torch

import _exact as X


def code_ld(C: int, granule: int = 16) -> int:
    """Row stride in bytes of a code plane (ops.code_ld_bytes, restated so that the helper needs no HIP library)."""
    return max(granule, (int(C) + granule - 1) // granule * granule)


# ---- code planes ------------------------------------------------------------------------------------------------------------

def encode_plane(q: torch.Tensor, halo=(0, 0), ld: Optional[int] = None) -> torch.Tensor:
    """Integer codes [N, C, H, W] (|q| <= 128) -> int8 plane [N * (H + 2hy) * (W + 2hx), ld] with zero border and zero pad bytes."""
    N, C, H, W = (int(v) for v in q.shape)
    hy, hx = (int(v) for v in halo)
    ld = code_ld(C) if ld is None else int(ld)
    assert ld >= C and int(q.min()) >= -128 and int(q.max()) <= 127
    plane = torch.zeros((N, H + 2 * hy, W + 2 * hx, ld), dtype=torch.int8, device=q.device)
    plane[:, hy:hy + H, hx:hx + W, :C] = q.permute(0, 2, 3, 1).to(torch.int8)
    return plane.view(N * (H + 2 * hy) * (W + 2 * hx), ld)


def check_plane_zeros(plane: torch.Tensor, N: int, H: int, W: int, C: int, halo=(0, 0), what="code plane"):
    """Every border byte and every pad byte past C of a code plane must be zero."""
    hy, hx = (int(v) for v in halo)
    p = plane.reshape(N, H + 2 * hy, W + 2 * hx, -1)
    inner = p[:, hy:hy + H, hx:hx + W]
    nz_all, nz_inner = int(p.count_nonzero()), int(inner.count_nonzero())
    assert nz_all == nz_inner, f"{what}: {nz_all - nz_inner} non-zero bytes in the halo border"
    nz_pad = int(inner[..., C:].count_nonzero())
    assert nz_pad == 0, f"{what}: {nz_pad} non-zero pad bytes past channel {C}"


def decode_plane(plane: torch.Tensor, N: int, H: int, W: int, C: int, halo=(0, 0), what="code plane") -> torch.Tensor:
    """int8 plane [N * (H + 2hy) * (W + 2hx), ld] -> int64 codes [N, C, H, W] of the interior; asserts the zero border and pad."""
    assert plane.dtype == torch.int8
    check_plane_zeros(plane, N, H, W, C, halo, what)
    hy, hx = (int(v) for v in halo)
    p = plane.reshape(N, H + 2 * hy, W + 2 * hx, -1)
    return p[:, hy:hy + H, hx:hx + W, :C].permute(0, 3, 1, 2).to(torch.int64)


# ---- exact accumulator ------------------------------------------------------------------------------------------------------

def exact_acc(codes_nchw: torch.Tensor, w_int: torch.Tensor, stride=1, padding=0) -> torch.Tensor:
    """conv64 of integer codes with integer weights, float64 [n, Cout, Ho, Wo].  Asserts |acc| <= 127 * C * k * k < 2^24 (times the
    largest |weight|): every partial sum is an integer below 2^53, so the result is the exact sum and (float)acc is exact."""
    C, kh, kw = (int(v) for v in w_int.shape[1:])
    wmax = float(w_int.abs().max()) if w_int.numel() else 0.0
    bound = 127 * C * kh * kw * max(1.0, wmax)
    assert bound < (1 << 24), f"127 * C * k * k * max|w| = {bound} >= 2^24"
    assert float(codes_nchw.abs().max()) <= 128
    acc = X.conv64(codes_nchw, w_int, stride, padding)
    amax = float(acc.abs().max()) if acc.numel() else 0.0
    assert amax <= bound + 1e-9, f"|acc| = {amax} > {bound}"
    return acc


# ---- fp32 operations, one rounding each --------------------------------------------------------------------------------------

def _d(x):
    return x.to(torch.float64)


def f_mul(a, b):
    return (_d(a) * _d(b)).to(torch.float32)


def f_add(a, b):
    return (_d(a) + _d(b)).to(torch.float32)


def f_sub(a, b):
    return (_d(a) - _d(b)).to(torch.float32)


def f_fma(a, b, c):
    """(r, alt): r = the float64 value of a * b + c rounded to fp32; alt = the fp32 neighbour the correctly rounded fma could be
    instead (where the float64 sum is an fp32 midpoint without being an fp32 value), else r itself."""
    s = _d(a) * _d(b) + _d(c)
    r = s.to(torch.float32)
    side = torch.where(s > _d(r), torch.full_like(r, float("inf")), torch.full_like(r, float("-inf")))
    nxt = torch.nextafter(r, side)
    amb = (s != _d(r)) & ((_d(r) + _d(nxt)) * 0.5 == s) & torch.isfinite(nxt)
    return r, torch.where(amb, nxt, r)


def f_relu(t):
    """``t < 0 ? 0 : t`` — NaN stays NaN."""
    return torch.where(t < 0, torch.zeros_like(t), t)


def f32_scalar(v, device=None) -> torch.Tensor:
    return torch.as_tensor(v, dtype=torch.float32, device=device).reshape(())


def kernel_scale(scale, scale_dev=None, device=None) -> torch.Tensor:
    """The fp32 scale the conv kernels multiply with: ``scale`` as a float argument, times the device scalar if there is one."""
    s = f32_scalar(scale, device)
    return s if scale_dev is None else f_mul(s, f32_scalar(scale_dev, device).to(s.device))


@dataclass
class Epi:
    """Arguments of the code epilogue; per-channel vectors are fp32 [C] (channels = the LAST dimension of the value tensors).
    Device form: ``stats`` = (mean, rs) with (alpha, beta) = BatchNorm (weight, bias); folded form: stats None."""
    alpha: torch.Tensor
    beta: torch.Tensor
    levels: float
    stats: Optional[tuple] = None
    relu: int = 1                          # 0 none, 1 behind BatchNorm and residual, 2 in front of the BatchNorm
    res_f32: Optional[torch.Tensor] = None   # [..., C] like the value
    res_affine: Optional[tuple] = None       # (ra, rb) folded | (rw, rb, (rmean, rrs)) device form
    res_codes: Optional[torch.Tensor] = None  # integer [..., C]
    rscale: float = 0.0


def conv_value(acc: torch.Tensor, scale: torch.Tensor, conv_bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ElemI8::out: v = fl(float(acc) * scale), then fl(v + bias) where the conv has a bias.  acc: exact integers, channels last."""
    v = f_mul(acc.to(torch.float32), scale)
    return v if conv_bias is None else f_add(v, conv_bias.to(torch.float32))


def quantise(t: torch.Tensor, levels: float):
    """(code int64, ok bool, q fp32): q = rint(fl(levels * t)) half to even; ok = |q| <= 127 (false for NaN); code 0 where not ok."""
    q = torch.round(f_mul(t, f32_scalar(levels, t.device)))
    ok = q.abs() <= 127.0
    return torch.where(ok, q, torch.zeros_like(q)).to(torch.int64), ok, q


def epilogue(v: torch.Tensor, p: Epi) -> dict:
    """The code epilogue on the fp32 value ``v`` [..., C].  Returns codes (int64), flag (any code out of range / NaN), flag_head (the
    head kernel's flag value: 1, or 3 where some |q| > 2047 or NaN), t (fp32, behind the ReLU), lo / hi (the smallest / largest code
    over the fma results the reference cannot tell apart)."""
    v = v.to(torch.float32)
    if p.relu == 2:
        v = f_relu(v)
    if p.stats is not None:
        mean, rs = p.stats
        t0, t0_alt = f_fma(f_mul(f_sub(v, mean), rs), p.alpha, p.beta)
    else:
        t0 = t0_alt = f_add(f_mul(v, p.alpha), p.beta)
    u = u_alt = None
    if p.res_f32 is not None:
        u = u_alt = p.res_f32.to(torch.float32)
        if p.res_affine is not None:
            if len(p.res_affine) > 2 and p.res_affine[2] is not None:
                rmean, rrs = p.res_affine[2]
                u, u_alt = f_fma(f_mul(f_sub(u, rmean), rrs), p.res_affine[0], p.res_affine[1])
            else:
                u = u_alt = f_add(f_mul(u, p.res_affine[0]), p.res_affine[1])

    def tail(t, uu):
        if uu is not None:
            t = f_add(t, uu)
        if p.res_codes is not None:
            t = f_add(t, f_mul(f32_scalar(p.rscale, t.device), p.res_codes.to(torch.float32)))
        if p.relu == 1:
            t = f_relu(t)
        return (t,) + quantise(t, p.levels)

    t, code, ok, q = tail(t0, u)
    out = {"codes": code, "t": t, "flag": not bool(ok.all()), "lo": code, "hi": code}
    out["flag_head"] = 0 if bool(ok.all()) else (1 if bool((q.abs() <= 2047.0)[~ok].all()) else 3)
    for ta, ua in ((t0_alt, u), (t0, u_alt)):
        if (ta is not t0 and not torch.equal(ta, t0)) or (ua is not u and not torch.equal(ua, u)):
            alt = tail(ta, ua)[1]
            out["lo"], out["hi"] = torch.minimum(out["lo"], alt), torch.maximum(out["hi"], alt)
    return out


def sensitive(ref: dict) -> torch.Tensor:
    """Elements whose code changes when t moves by one fp32 ulp: the reference's own uncertainty."""
    return (ref["lo"] != ref["codes"]) | (ref["hi"] != ref["codes"])


# ---- comparison -------------------------------------------------------------------------------------------------------------

WAIVER_PER_MILLION = 1


def mismatch_report(got, want, acc=None, t=None, images=None, limit: int = 8, what="") -> str:
    """'' if got == want, else the count and the first ``limit`` (n, y, x, c) with the exact sum, t and both codes.
    got / want / acc / t: [n, H, W, C]."""
    diff = got != want
    cnt = int(diff.sum())
    if cnt == 0:
        return ""
    idx = diff.nonzero()[:limit].tolist()
    lines = [f"{what}: {cnt} of {diff.numel()} codes differ; first {len(idx)}:"]
    for n, y, x, c in idx:
        s = f"  (n={n if images is None else int(images[n])}, y={y}, x={x}, c={c}) got {int(got[n, y, x, c])} want {int(want[n, y, x, c])}"
        if acc is not None:
            s += f" acc={float(acc[n, y, x, c]):.0f}"
        if t is not None:
            s += f" t={float(t[n, y, x, c])!r}"
        lines.append(s)
    return "\n".join(lines)


def compare_codes(got: torch.Tensor, ref: dict, designed: bool, acc=None, images=None, what=""):
    """The waiver rule.  Designed cases: zero mismatches.  Realistic cases: a mismatching element passes only if the kernel's code
    is the reference's lo or hi variant of that element.  Returns (waived, message): message is '' or the report of what fails;
    the caller sums ``waived`` over a case and holds it to ``waiver_cap``."""
    want = ref["codes"]
    diff = got != want
    if not bool(diff.any()):
        return 0, ""
    if designed:
        return 0, mismatch_report(got, want, acc, ref["t"], images, what=what + " (designed: nothing is waived)")
    ok = diff & ((got == ref["lo"]) | (got == ref["hi"]))
    bad = diff & ~ok
    if bool(bad.any()):
        return int(ok.sum()), mismatch_report(torch.where(bad, got, want), want, acc, ref["t"], images, what=what + " (outside +-1 ulp of t)")
    return int(ok.sum()), ""


def waiver_cap(numel: int) -> int:
    """At most one waived element per million compared elements of a case."""
    return int(numel) * WAIVER_PER_MILLION // 1_000_000


# ---- operands ---------------------------------------------------------------------------------------------------------------

def _gen(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


def random_codes(shape, lo: int, hi: int, seed: int, device) -> torch.Tensor:
    """Uniform integer codes in [lo, hi], int64, drawn on ``device`` by a seeded generator."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed, device), device=device, dtype=torch.int64)


def pm1_weights(Cout, Cin, k, seed, device) -> torch.Tensor:
    return (torch.randint(0, 2, (Cout, Cin, k, k), generator=_gen(seed, device), device=device) * 2 - 1).to(torch.float32)


def designed_shift(K: int, levels: float = 15.0) -> int:
    """log2 of the divisor that brings the sum of K codes uniform in 0..3 times +-1 weights (standard deviation sqrt(3.5 K)) to a
    levels * t of standard deviation ~40, inside int8; at least 2 (t stays on the 1/4 grid of the biases) and at most 5, so that
    1 / 32 of uniformly spread sums are exact ties (see designed_params)."""
    import math
    return max(2, min(5, round(math.log2(max(1.0, math.sqrt(3.5 * K) * levels / 40.0)))))


def designed_params(C: int, shift: int, seed: int, device, form: str = "device"):
    """Operands for which every step of the epilogue is exact: scale = 1/4, rs = 2^-(shift-1), weight = +-2, mean = k/4 and
    bias = j/4 with small integers k, j (folded form: alpha = +-2^-(shift-2), beta = j/4).  Then
        t = +-(acc - k) / 2^shift + j/4,
    a multiple of 2^-shift below 2^10, and levels * t is exact; it lands on x.5 iff +-(acc - k) + j 2^(shift-2) = 2^(shift-1) mod
    2^shift: 2^-shift of uniformly spread sums.  A code residual with rscale = 1/4 and an fp32 residual of multiples of 1/4 keep t
    on the grid.  Returns (scale, alpha, beta, stats or None)."""
    assert 2 <= shift <= 6
    g = _gen(seed, device)
    sign = (torch.randint(0, 2, (C,), generator=g, device=device) * 2 - 1).to(torch.float32)
    k = torch.randint(-8, 9, (C,), generator=g, device=device).to(torch.float32)
    j = torch.randint(-4, 13, (C,), generator=g, device=device).to(torch.float32)
    if form == "device":
        return 0.25, sign * 2.0, j / 4, (k / 4, torch.full((C,), 2.0 ** -(shift - 1), device=device))
    return 0.25, sign * 2.0 ** -(shift - 2), j / 4, None


def realistic_params(C: int, K: int, seed: int, device, form: str = "device", code_max: int = 15):
    """BatchNorm statistics like bench_models.randomize_bn (mean 3 N(0,1), variance U(50, 100), weight U(0.5, 1.5), bias 0.1 N(0,1)),
    and a conv scale fl(inv_levels * E) with E = mean|W| of a weight +-E sized so that the conv's value has the spread those
    statistics expect (standard deviation ~4, which keeps |levels * t| inside int8).  Returns (scale, E, alpha, beta, stats or None): device form (weight, bias, (mean,
    rs)), folded form alpha = weight * rs, beta = bias - mean * alpha rounded once each."""
    g = _gen(seed, device)
    mean = torch.randn(C, generator=g, device=device) * 3
    var = torch.rand(C, generator=g, device=device) * 50 + 50
    w = torch.rand(C, generator=g, device=device) + 0.5
    b = torch.randn(C, generator=g, device=device) * 0.1
    rs = (1.0 / torch.sqrt(var.double() + 1e-5)).float()
    e2 = sum(v * v for v in range(code_max + 1)) / (code_max + 1)
    inv = float(torch.tensor(1.0) / torch.tensor(float(code_max)))
    E = torch.tensor(4.0 / ((K * e2) ** 0.5 * inv), dtype=torch.float32, device=device) * 1.0123
    if form == "device":
        return inv, E, w, b, (mean, rs)
    alpha = (w * rs)
    return inv, E, alpha, b - mean * alpha, None


CANCEL_OFFSET = 65536.0


def cancelling_params(C: int, K: int, seed: int, device, code_max: int = 15):
    """realistic_params in the device form with a large common offset that the BatchNorm bias takes out again: mean - 2^16 and
    bias - 2^16 rs weight (rounded once).  t keeps the spread of the realistic case, but the product inside the fma is ~7000
    while t is ~1, so an epilogue that rounds the product before it adds the bias (a multiply and an add in place of the fma) is off
    by up to half an ulp of 7000, 2.4e-4: a few codes in a thousand change.  The integer sums of a layer take only a few thousand
    values per channel, so without this the fma's single rounding decides a code too rarely for a test to rely on.  Every rounding
    of the chain is still the reference's own, one per operation."""
    inv, E, w, b, (mean, rs) = realistic_params(C, K, seed, device, "device", code_max)
    b = (b.double() - CANCEL_OFFSET * rs.double() * w.double()).float()
    return inv, E, w, b, (mean - CANCEL_OFFSET, rs)


def edge_channels(alpha, beta, stats, levels=15.0):
    """The edge channels of test_gpu_exact_b256's _affine carried over to the code epilogue (in place): zero, negative-zero and NaN
    weight, +-1e6 and +-inf bias, a huge rs, and two channels whose every element is q = 127 / q = 128.  Codes that leave int8 or
    are NaN: code 0 and the range flag."""
    alpha[0], beta[0] = 0.0, 0.5
    alpha[1], beta[1] = 0.0, -1.0
    beta[2], beta[3] = 1e6, -1e6
    alpha[4], beta[4] = -0.0, 1.0
    alpha[5] = float("nan")
    beta[6], beta[7] = float("inf"), float("-inf")
    if stats is not None:
        stats[1][8] = 1e30
    # the int8 edge itself, whatever the sum: weight 0 leaves t = bias; levels * t = 127 is the last code, 128 the first to go
    levels = float(levels)
    alpha[9], beta[9] = 0.0, 127.0 / levels
    alpha[10], beta[10] = 0.0, 128.0 / levels
