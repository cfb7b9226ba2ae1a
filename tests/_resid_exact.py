"""Exact reference for the residual pass of the sign chain (qt_bn_add_sign_f32), shared by the tests (a plain module, not a conftest).

torch on the CPU and numpy, float64 arithmetic, none of the package's packers or ops.  Per element, ONE correctly rounded fp32 result
per kernel operation, in the kernel's order (csrc/resid_sign.hip, compiled with -ffp-contract=off):

    t = fma(fl(fl(x - mean[c]) * rs[c]), weight[c], bias[c])
    s = fl(t + r)
    v = s < lo ? lo : (s > hi ? hi : s)      with a Hardtanh (NaN stays NaN), else v = s
    bit = [v < 0]                            -0.0, ties and NaN give 0

The rounding helpers are those of tests/_codes_exact.py (each step formed in float64 and rounded to fp32 once; the fma can
double-round only where the float64 sum is an fp32 midpoint without being the exact sum — ``f_fma`` returns the neighbour the correctly
rounded fma could be instead, and the reference follows it to the end and reports the elements where it changes v: ``ambiguous``).

Planes (include/qt_hip.h): sign plane uint32 [N Ho Wo][ldb], bit (c & 31) of word (c >> 5) is channel c, 1 <=> negative, everything
past C zero; nibble plane uint32 [N (Ho + 2 hy) (Wo + 2 hx)][ldn], channel c in nibble (c & 7) of word (c >> 3), +1 = 0x2, -1 = 0xA,
channels >= C and border pixels zero words."""
import numpy as np
import torch

from _codes_exact import WAIVER_PER_MILLION, f_add, f_fma, f_mul, f_sub, waiver_cap  # noqa: F401  (re-exported for the tests)

SUBNORMAL = float(np.float32(2.0 ** -149))


def packed_ld(C: int) -> int:
    return max(4, ((int(C) + 31) // 32 + 3) // 4 * 4)


def pixel_ld_nib(C: int) -> int:
    return max(4, ((int(C) + 7) // 8 + 3) // 4 * 4)


def _per_channel(p, like):
    return p.view(1, -1, 1, 1).expand_as(like)


def _clamp(s, hardtanh):
    if hardtanh is None:
        return s
    lo, hi = (torch.tensor(float(v), dtype=torch.float32) for v in hardtanh)
    return torch.where(s < lo, lo.expand_as(s), torch.where(s > hi, hi.expand_as(s), s))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise equality of fp32 BIT PATTERNS (NaN payloads aside: two NaNs count as the same)."""
    return (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))


def reference(x, mean, rs, weight, bias, r, hardtanh=None) -> dict:
    """x, r: fp32 [N, C, Ho, Wo] on the CPU; mean, rs, weight, bias: fp32 [C].  Returns t, s, v (fp32 [N, C, Ho, Wo]), neg (bool) and
    ambiguous (bool: the float64 evaluation of the fma cannot tell two fp32 neighbours apart AND the choice changes v)."""
    x, r = x.detach().cpu().float(), r.detach().cpu().float()
    mean, rs, weight, bias = (_per_channel(p.detach().cpu().float(), x) for p in (mean, rs, weight, bias))
    m = f_mul(f_sub(x, mean), rs)
    t, t_alt = f_fma(m, weight, bias)
    s, s_alt = f_add(t, r), f_add(t_alt, r)
    v, v_alt = _clamp(s, hardtanh), _clamp(s_alt, hardtanh)
    return {"t": t, "s": s, "v": v, "neg": v < 0, "ambiguous": ~same_bits(v, v_alt)}


def sign_plane(neg: torch.Tensor, ld=None) -> np.ndarray:
    """bool [N, C, Ho, Wo] -> uint32 [N Ho Wo, ld]."""
    neg = neg.cpu().numpy().astype(bool)
    N, C, H, W = neg.shape
    ld = packed_ld(C) if ld is None else int(ld)
    out = np.zeros((N * H * W, ld), dtype=np.uint32)
    rows = neg.transpose(0, 2, 3, 1).reshape(N * H * W, C)
    for c in range(C):
        out[:, c >> 5] |= rows[:, c].astype(np.uint32) << np.uint32(c & 31)
    return out


def nib_plane(neg: torch.Tensor, halo=(0, 0), ld=None) -> np.ndarray:
    """bool [N, C, Ho, Wo] -> uint32 [N (Ho + 2 hy) (Wo + 2 hx), ld] with zero border pixels."""
    neg = neg.cpu().numpy().astype(bool)
    N, C, H, W = neg.shape
    hy, hx = (int(v) for v in halo)
    ld = pixel_ld_nib(C) if ld is None else int(ld)
    out = np.zeros((N, H + 2 * hy, W + 2 * hx, ld), dtype=np.uint32)
    rows = neg.transpose(0, 2, 3, 1)
    for c in range(C):
        nibble = np.where(rows[..., c], np.uint32(0xA), np.uint32(0x2))
        out[:, hy:hy + H, hx:hx + W, c >> 3] |= nibble << np.uint32(4 * (c & 7))
    return out.reshape(N * (H + 2 * hy) * (W + 2 * hx), ld)


# ---- operand classes -------------------------------------------------------------------------------------------------------------

def _gen(seed):
    g = torch.Generator()
    g.manual_seed(int(seed))
    return g


#: the sums the designed class places in channel 0, in this order, at the first pixels of the tensor (as many as fit)
def designed_targets(hardtanh):
    lo, hi = hardtanh if hardtanh is not None else (-1.0, 1.0)
    return [0.0, -0.0, SUBNORMAL, -SUBNORMAL, float(lo), float(hi), float("nan"), float("inf"), float("-inf")]


def designed(shape, seed: int, hardtanh=None, fma_case: bool = True) -> dict:
    """Dyadic BatchNorm parameters, integer conv values and dyadic residuals: every step is exact, nothing is ambiguous.

    Channel 0 (mean 3, rs 0.5, weight -1, bias -0.0) carries the placed sums: where x == mean, t = fma(+0, -1, -0.0) = -0.0, so
    s = -0.0 + r is exactly the placed r: 0 (from r = +0), -0.0, +- the smallest subnormal, lo, hi, NaN, +-inf.
    Channel 1 (``fma_case``; mean -2^-12, rs 1, weight 1 + 2^-12, bias -(1 + 2^-11)) holds x = 1 everywhere and, at its first pixel,
    r = -2^-25: m = 1 + 2^-12, m * weight = 1 + 2^-11 + 2^-24 exactly, so the fma gives t = 2^-24 and s = 2^-25 > 0 (bit 0), while a
    separately rounded product (1 + 2^-11, the tie goes to even) gives t = 0 and s = -2^-25 < 0 (bit 1)."""
    N, C, H, W = shape
    g = _gen(seed)
    mean = torch.randint(-8, 9, (C,), generator=g).float()
    rs = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=g)]
    weight = torch.randint(-6, 7, (C,), generator=g).float() * 0.25
    weight[weight == 0] = 0.75
    bias = torch.randint(-16, 17, (C,), generator=g).float() * 0.125
    x = torch.randint(-40, 41, shape, generator=g).float()
    r = torch.randint(-64, 65, shape, generator=g).float() * 0.0625
    mean[0], rs[0], weight[0], bias[0] = 3.0, 0.5, -1.0, -0.0
    targets = designed_targets(hardtanh)
    placed = min(len(targets), N * H * W)
    for i, tv in enumerate(targets[:placed]):                      # pixels in (n, h, w) order
        n, h, w = i // (H * W), (i % (H * W)) // W, i % W
        x[n, 0, h, w] = 3.0
        r[n, 0, h, w] = tv
    has_fma = bool(fma_case and C >= 2)
    if has_fma:
        mean[1], rs[1], weight[1], bias[1] = -(2.0 ** -12), 1.0, 1.0 + 2.0 ** -12, -(1.0 + 2.0 ** -11)
        x[:, 1] = 1.0                  # (every pixel: t = 2^-24 exactly, never an fp32 midpoint)
        r[0, 1, 0, 0] = -(2.0 ** -25)
    return {"x": x, "r": r, "mean": mean, "rs": rs, "weight": weight, "bias": bias, "placed": placed, "fma_case": has_fma,
            "var": 1.0 / (rs.double() ** 2)}


def realistic(shape, seed: int) -> dict:
    """Gaussian BatchNorm statistics over several decades, integer conv values around the mean, a Gaussian residual."""
    N, C, H, W = shape
    g = _gen(seed)
    decade = 10.0 ** (torch.rand((C,), generator=g) * 4.0 - 2.0)                 # 0.01 ... 100
    mean = torch.randn((C,), generator=g) * decade
    var = (decade * (0.5 + torch.rand((C,), generator=g))) ** 2
    rs = (1.0 / torch.sqrt(var.double() + 1e-5)).float()
    weight = 1.0 + 0.5 * torch.randn((C,), generator=g)
    bias = torch.randn((C,), generator=g)
    x = torch.round(torch.randn(shape, generator=g) * torch.sqrt(var).view(1, C, 1, 1) * 2.0 + mean.view(1, C, 1, 1))
    r = torch.randn(shape, generator=g) * 1.5
    return {"x": x.float(), "r": r.float(), "mean": mean.float(), "rs": rs, "weight": weight.float(), "bias": bias.float()}


# ---- the case matrix of tests/test_gpu_resid_sign.py (shared with the CPU test that pins the ambiguity share) ---------------------

CHANNELS = (3, 4, 20, 32, 33, 36, 64, 100)
SHAPES = ((1, 1, 1), (2, 3, 5), (3, 7, 7), (2, 14, 14))
RESIDUALS = ("nchw", "cl", "cl_pitch", "cl_misaligned")
SUMS = ("inplace", "separate", "absent")
PLANES = ("sign", "nib", "both")
HALOS = ((0, 0), (1, 1), (2, 1))
HARDTANHS = (None, (-1.0, 1.0), (-0.5, 2.0))


def combos(C: int, shape):
    """Option tuples (residual form, sum, planes, halo, hardtanh) of one (C, shape) case: sum x planes in full (3 x 3), the halo and
    the Hardtanh rotating so that each of their values occurs three times, and all four residual forms; the rotation starts
    somewhere else in every case.  Two more tuples ask for the sum in NCHW storage ("nchw")."""
    k = CHANNELS.index(C) + len(CHANNELS) * SHAPES.index(tuple(shape))
    out = []
    for i in range(9):
        a, b = i % 3, i // 3
        out.append((RESIDUALS[(i + k) % 4], SUMS[a], PLANES[b], HALOS[(a + b + k) % 3], HARDTANHS[(a + 2 * b + k // 3) % 3]))
    # the sum in NCHW storage (written through the LDS tile), behind a residual of either storage
    out.append(("nchw", "nchw", PLANES[k % 3], HALOS[(k + 1) % 3], HARDTANHS[k % 3]))
    out.append((RESIDUALS[1 + k % 3], "nchw", PLANES[(k + 1) % 3], HALOS[k % 3], HARDTANHS[(k + 1) % 3]))
    return out


def seed_of(C: int, shape, i: int) -> int:
    return 1000 * C + 10 * (shape[0] * 100 + shape[1] * 10 + shape[2]) + i
