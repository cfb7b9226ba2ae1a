"""Operands, planes and cases of the matrix-core GEMM route tests (tests/test_gpu_gemm_routes.py; pinned without a device by
tests/test_gemm_exact_cpu.py).

The operand planes are built HERE, in torch, from integer matrices: the project's packers are not on the path, so a packer bug
can neither mask nor mimic a GEMM bug.  Formats (include/qt_hip.h): a row is ``ld`` uint32 words, zero from element K on;
  fp4   element k = nibble k % 8 of word k / 8 (bits 4 (k % 8) ..): +1 -> 0x2, -1 -> 0xA, 0 -> 0x0 (FP4-E2M1);
  int8  element k = byte k of the row;
  bf16 / fp16  element k = the 16 bits at byte 2 k of the row.
Values are chosen so that every partial sum, in any accumulation order, is an integer below 2^24 (``abs_bound``): the fp64
product is then the only right answer and every comparison of the GPU module is torch.equal.  Scales are powers of two.

Everything is generated on the CPU from fixed seeds (the same numbers wherever the module runs) and is moved to the device by the
GPU module."""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

ELEMS = ("ElemFp4", "ElemFp4Out<1>", "ElemFp4Out<2>", "ElemBf16", "ElemF16", "ElemI8")
FAMILY = {"ElemFp4": "fp4", "ElemFp4Out<1>": "fp4", "ElemFp4Out<2>": "fp4", "ElemBf16": "bf16", "ElemF16": "f16", "ElemI8": "i8"}
OUT_DTYPE = {"ElemFp4Out<1>": torch.bfloat16, "ElemFp4Out<2>": torch.float16}       # every other element class stores fp32
PER_WORD = {"fp4": 8, "bf16": 2, "f16": 2, "i8": 4}                                  # elements per uint32 word of a row
HALF_OF = {"bf16": torch.bfloat16, "f16": torch.float16}
EXACT = 1 << 24
# the eleven configurations launch_gemm_auto (csrc/mfma_gemm.hip) can launch
AUTO_RUNGS = ("CfgSkinny512", "CfgSkinny", "PP256", "PP384x192", "PP192", "PP128", "Cfg64_1", "Cfg256_0", "Cfg192_0", "Cfg128_0", "Cfg64_0")
# sentinels of the result buffers: NaNs with a payload no kernel produces (a NaN bias leaves as the canonical quiet NaN)
SENTINEL = {torch.float32: 0x7FC5A5A5, torch.bfloat16: 0x7FE5, torch.float16: 0x7FE5}
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


# ---- integer operands ---------------------------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def uniform_ints(seed, rows, K, lo, hi):
    """[rows, K] int64, uniform in lo .. hi: every row and every column its own pattern."""
    return torch.randint(lo, hi + 1, (rows, K), generator=_gen(seed), dtype=torch.int64)


def ternary(seed, rows, K):
    """-1 / 0 / +1 with a fifth of zeros."""
    g = _gen(seed)
    s = torch.randint(0, 2, (rows, K), generator=g, dtype=torch.int64) * 2 - 1
    return s * (torch.rand((rows, K), generator=g) >= 0.2)


def correlated_pm1(seed, rows, K, base_seed, max_rate):
    """+-1 rows that are noisy signed copies of ONE base vector (flip rate per row uniform in [0.02, max_rate], so no two rows are
    alike; random sign per row): the sums of two such operands are large, and with odd K odd — exact ties where the output format
    spaces integers by 2."""
    g = _gen(seed)
    base = torch.randint(0, 2, (1, K), generator=_gen(base_seed), dtype=torch.int64) * 2 - 1
    rate = 0.02 + torch.rand((rows, 1), generator=g) * (max_rate - 0.02)
    sign = torch.randint(0, 2, (rows, 1), generator=g, dtype=torch.int64) * 2 - 1
    flip = torch.rand((rows, K), generator=g) < rate
    return torch.where(flip, -base, base) * sign


# ---- planes ---------------------------------------------------------------------------------------------------------------------

def _padded(q, width):
    rows, K = q.shape
    assert K <= width
    full = torch.zeros((rows, width), dtype=torch.int64)
    full[:, :K] = q
    return full


def nib_plane(q, ld):
    """-1 / 0 / +1 matrix -> fp4 nibble plane, uint8 [rows, 4 ld] (byte j = nibble 2 j | nibble 2 j + 1 << 4)."""
    assert int(q.abs().max()) <= 1
    full = _padded(q, 8 * ld)
    nib = torch.where(full == 0, 0x0, torch.where(full < 0, 0xA, 0x2))
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8).contiguous()


def nib_decode(plane):
    """uint8 nibble plane -> (values [rows, 8 ld] int64, nibbles [rows, 8 ld]); a nibble that is none of 0x0 / 0x2 / 0xA is an error."""
    b = plane.to(torch.int64)
    nib = torch.stack([b & 0xF, b >> 4], dim=2).reshape(plane.shape[0], -1)
    assert bool(((nib == 0x0) | (nib == 0x2) | (nib == 0xA)).all())
    return torch.where(nib == 0x2, 1, torch.where(nib == 0xA, -1, 0)), nib


def i8_plane(q, ld):
    """int8 code plane, int8 [rows, 4 ld]."""
    assert int(q.abs().max()) <= 127
    return _padded(q, 4 * ld).to(torch.int8).contiguous()


def half_plane(q, ld, dtype):
    """bf16 / fp16 plane of small integers (|q| <= 8: exact in both formats), dtype [rows, 2 ld]."""
    assert int(q.abs().max()) <= 8
    return _padded(q, 2 * ld).to(dtype).contiguous()


def make_plane(family, q, ld):
    if family == "fp4":
        return nib_plane(q, ld)
    if family == "i8":
        return i8_plane(q, ld)
    return half_plane(q, ld, HALF_OF[family])


def decode_plane(family, plane):
    """plane -> (integer values over the whole row stride, the raw storage units as integers): the pad is zero where the RAW units are."""
    if family == "fp4":
        return nib_decode(plane)
    if family == "i8":
        return plane.to(torch.int64), plane.to(torch.int64)
    return plane.double().to(torch.int64), plane.view(torch.int16).to(torch.int64)


def abs_bound(xq, wq):
    """An upper bound of every |partial sum| in any order: sum_k max_m |x[m, k]| max_n |w[n, k]| >= max_mn sum_k |x[m, k]| |w[n, k]|."""
    return int((xq.abs().amax(0) * wq.abs().amax(0)).sum())


def abs_sum_max(xq, wq):
    """max_mn sum_k |x[m, k]| |w[n, k]| itself (small cases)."""
    return int((xq.abs().double() @ wq.abs().double().t()).max())


# ---- cases ----------------------------------------------------------------------------------------------------------------------

def k_pair(family, ld):
    """(K a few elements short of the stride's capacity, K about half of it): a tail inside the last stage, and a row with whole zero
    stages.  ld = 32 words: 250 / 130 nibbles, 61 / 35 bf16 or fp16 elements, 125 / 70 bytes."""
    cap = PER_WORD[family] * ld
    d1, d2 = {"fp4": (6, 2), "bf16": (3, 3), "f16": (3, 3), "i8": (3, 6)}[family]
    return cap - max(1, min(d1, cap // 4)), cap // 2 + min(d2, cap // 8)


@dataclass
class Case:
    """One launch.  bias: None / "int" / "frac" / "nan" / "inf"; scale: (host scale, device scale or None) — powers of two;
    kind: "uniform" (the family's full range) or "corr" (correlated +-1, fp4 only); y: (ldy - N, offset of Y in elements)."""
    name: str
    elem: str
    rung: str
    M: int
    N: int
    ld: int
    K: int
    bias: Optional[str] = None
    scale: Tuple[float, Optional[float]] = (1.0, None)
    kind: str = "uniform"
    y: Tuple[int, int] = (3, 0)
    wmax: int = 1              # int8: weight codes in -wmax .. wmax (1: the +-1 / 0 codes; 15: 4-bit DoReFa weight codes)
    variant: int = 0           # qt_nib_gemm_variant's number (fp4 -> fp32 only)
    seed: int = field(default=0)

    @property
    def family(self):
        return FAMILY[self.elem]

    @property
    def out_dtype(self):
        return OUT_DTYPE.get(self.elem, torch.float32)

    @property
    def ldy(self):
        return self.N + self.y[0]

    @property
    def max_abs_code(self):
        return 127 * self.wmax

    @property
    def total_scale(self):
        return self.scale[0] * (1.0 if self.scale[1] is None else self.scale[1])

    def __post_init__(self):
        if not self.seed:
            self.seed = (hash_name(self.name) % 100000) + 17


def hash_name(s):
    h = 0
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def operands(c: Case):
    """(x [M, K], w [N, K]) int64 on the CPU."""
    f = c.family
    if c.kind == "corr":
        assert f == "fp4"
        return (correlated_pm1(c.seed, c.M, c.K, c.seed + 7, 0.2), correlated_pm1(c.seed + 1, c.N, c.K, c.seed + 7, 0.2))
    if f == "fp4":
        return ternary(c.seed, c.M, c.K), ternary(c.seed + 1, c.N, c.K)
    if f == "i8":
        return uniform_ints(c.seed, c.M, c.K, -127, 127), uniform_ints(c.seed + 1, c.N, c.K, -c.wmax, c.wmax)
    return uniform_ints(c.seed, c.M, c.K, -8, 8), uniform_ints(c.seed + 1, c.N, c.K, -8, 8)


def bias_of(c: Case):
    """fp32 [N] on the CPU, or None.  "int": integers; "frac": 24-bit fractions of magnitude >= 2^-20, so that sum + bias is exact
    in fp64 and rounds in fp32; "nan": integers with NaN in two columns; "inf": integers with +-1e5 (past fp16's 65504) in four."""
    if c.bias is None:
        return None
    g = _gen(c.seed + 2)
    b = torch.randint(-9, 10, (c.N,), generator=g, dtype=torch.int64).float()
    if c.bias == "frac":
        b = torch.randn((c.N,), generator=g) * 3
        b = torch.where(b.abs() < 2.0 ** -20, torch.full_like(b, 0.5), b)
    elif c.bias == "nan":
        b[nan_columns(c.N)] = float("nan")
    elif c.bias == "inf":
        b[1::max(2, c.N // 2 - 1)] = 1e5
        b[2::max(2, c.N // 2 - 1)] = -1e5
    else:
        assert c.bias == "int"
    return b


def nan_columns(N):
    return sorted({N // 3, N - 1})


def expected(sum64, c: Case, bias):
    """fl32(sum * scale + bias) — the power-of-two scale and the fp64 sum are exact, so this is ONE rounding, whichever of
    fma / multiply-then-add the kernel uses — and for the half results one more round-to-nearest-even by .to(dtype), the rule
    of tests/_half_cases.py rne_of_fl32.  ``sum64``: the fp64 product, on any device; ``bias`` on the same one."""
    y = sum64 * c.total_scale
    if bias is not None:
        y = y + bias.double()
    y = y.float()
    return y if c.out_dtype is torch.float32 else y.to(c.out_dtype)


def tie_share(y32, dtype):
    """Share of fp32 values exactly half way between two neighbours of ``dtype`` (normal range)."""
    p = 8 if dtype is torch.bfloat16 else 11
    a = y32.double().abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=1e-30)))
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (p - 1))
    return float(((torch.remainder(a, ulp) * 2 == ulp) & (a > 0) & torch.isfinite(a)).double().mean())


# (rung, M, N, row stride in words): the smallest shapes found that keep each rung of select_gemm (csrc/tile_select.h) with M
# and N off the tile grid.  The GPU module does not take the rung from this table as truth: it asks the describe entry points.
DENSE_SHAPES = [
    ("CfgSkinny512", 250, 70, 128),
    ("CfgSkinny", 509, 130, 64),
    ("CfgSkinny", 250, 70, 64),
    ("PP256", 8189, 1279, 32),
    ("PP384x192", 11003, 1150, 32),
    ("PP192", 8189, 1150, 32),
    ("PP128", 8189, 630, 32),
    ("Cfg64_1", 600, 70, 32),
    ("Cfg256_0", 8189, 1279, 36),
    ("Cfg192_0", 8189, 1150, 36),
    ("Cfg128_0", 8189, 630, 36),
    ("Cfg64_0", 600, 70, 36),
    ("Cfg64_0", 5, 7, 4),
]
LONG_K_SHAPES = [("CfgSkinny512", 250, 70, 1152), ("CfgSkinny", 509, 130, 1152)]     # the stage ring wraps many times
# scale forms of the entry points that take one (qt_f16_gemm, qt_i8_gemm): host alone, host x device, device alone
SCALES = [(0.125, None), (4.0, 0.03125), (1.0, 2.0)]


def _bias_modes(elem):
    return (None, "int", "frac") if FAMILY[elem] == "fp4" else (None, "int")


def dense_cases():
    """One case per (element class, shape of DENSE_SHAPES), each at the two K of k_pair; bias and scale forms cycle."""
    out = []
    for e, elem in enumerate(ELEMS):
        fam = FAMILY[elem]
        for i, (rung, M, N, ld) in enumerate(DENSE_SHAPES):
            modes = _bias_modes(elem)
            for j, K in enumerate(k_pair(fam, ld)):
                out.append(Case(f"{elem} {rung} {M}x{N} ld{ld} K{K}", elem, rung, M, N, ld, K, bias=modes[(i + j + e) % len(modes)],
                                scale=SCALES[(i + j) % 3] if fam in ("f16", "i8") else (1.0, None),
                                wmax=15 if (fam == "i8" and rung == "Cfg64_1" and j == 0) else 1))
    return out


def long_k_cases():
    """ld = 1152 words on the skinny rungs.  The half results use correlated operands with odd K = 9209: sums of 3300 .. 9209, where
    fp16 spaces integers by 2, 4 and 8 (and bf16 by 16 .. 64)."""
    out = []
    for elem in ELEMS:
        fam = FAMILY[elem]
        for rung, M, N, ld in LONG_K_SHAPES:
            K = k_pair(fam, ld)[0]
            half = elem in OUT_DTYPE
            out.append(Case(f"{elem} long K {rung} {M}x{N} ld{ld}", elem, rung, M, N, ld, K - 1 + K % 2 if half else K,
                            bias="int" if rung == "CfgSkinny" else None, kind="corr" if half else "uniform",
                            scale=(2.0, 0.25) if fam in ("f16", "i8") else (1.0, None)))
    return out


# the half epilogue's two store paths: (name, N, ldy - N, offset of Y in elements).  16-byte stores need N % 8 == 0, ldy % 8 == 0
# and a 16-byte aligned Y; every other row takes the element-wise path.
STORE_PATHS = [("wide", 0, 8, 0), ("N odd", -1, 9, 0), ("ldy odd", 0, 5, 0), ("Y offset", 0, 8, 1)]
STORE_TILES = [("PP256", 8189, 1272, 128), ("CfgSkinny512", 250, 72, 128)]
TIE_K = 1017        # odd; correlated sums of 366 .. 1017: bf16 spaces them by 2 (every odd sum a tie) and by 4


def store_path_cases():
    """bf16: correlated operands at odd K = 1017 with an integer bias (odd in half of the columns: the even sums above 512 that
    lie half way between multiples of 4) — the tie cases; fp16 (exact up to 2048): the same sums plus a fractional bias, so every
    output rounds.  Plus the fp32 classes on the same two tiles with N % 4 == 0: the dwordx4 store path of the fp32 epilogue."""
    out = []
    for elem in ("ElemFp4Out<1>", "ElemFp4Out<2>"):
        for rung, M, N, ld in STORE_TILES:
            for path, dn, dld, off in STORE_PATHS:
                out.append(Case(f"{elem} store {path} {rung} {M}x{N + dn}", elem, rung, M, N + dn, ld, TIE_K,
                                bias="int" if elem == "ElemFp4Out<1>" else "frac", kind="corr", y=(dld, off)))
    for elem in ("ElemFp4", "ElemBf16", "ElemF16", "ElemI8"):
        fam = FAMILY[elem]
        for rung, M, N, ld in STORE_TILES:
            out.append(Case(f"{elem} store wide {rung} {M}x{N}", elem, rung, M, N, ld, k_pair(fam, ld)[0], bias="int", y=(4, 0),
                            scale=(0.5, 0.5) if fam in ("f16", "i8") else (1.0, None)))
    return out


def is_tie_case(c: Case):
    return c.elem == "ElemFp4Out<1>" and c.kind == "corr" and c.K == TIE_K


def special_cases():
    """NaN in the bias (every class: NaN in that column and nowhere else), and fp16 overflow to +-inf."""
    out = []
    for elem in ELEMS:
        for rung, M, N, ld in (("CfgSkinny512", 250, 72, 128), ("Cfg64_1", 600, 70, 32)):
            out.append(Case(f"{elem} NaN bias {rung} {M}x{N}", elem, rung, M, N, ld, k_pair(FAMILY[elem], ld)[0], bias="nan",
                            y=(8, 0) if N % 8 == 0 else (3, 0)))
    for rung, M, N, ld in (("CfgSkinny512", 250, 72, 128), ("Cfg64_1", 600, 70, 32)):
        out.append(Case(f"ElemFp4Out<2> overflow {rung} {M}x{N}", "ElemFp4Out<2>", rung, M, N, ld, k_pair("fp4", ld)[0], bias="inf",
                        y=(8, 0) if N % 8 == 0 else (3, 0)))
    return out


# explicit variants of qt_nib_gemm_variant -> GemmCfg alias (csrc/tile_select.h gemm_variant_cfg)
VARIANTS = {5: "Cfg256_0", 6: "Cfg256_1", 7: "Cfg128_1", 8: "Cfg64_1", 9: "Cfg128_0", 10: "Cfg64_0", 15: "Cfg192_1", 16: "Cfg192_0",
            20: "PP256", 21: "PP128", 22: "PP192", 23: "PP64", 24: "PP384x192", 30: "CfgSkinny", 31: "CfgSkinny512"}
GENERIC_VARIANTS = (5, 9, 10, 16)


def variant_cases():
    """30 / 31 outside their automatic range (M = 1000: several row tiles); every other variant at one ragged shape with partial row
    and column tiles of every tile size (the generic kernels on a stride that is no whole stage)."""
    out = []
    for v, rung in VARIANTS.items():
        M, N, ld = (1000, 130, 128) if v in (30, 31) else (601, 301, 36 if v in GENERIC_VARIANTS else 32)
        out.append(Case(f"variant {v} {rung} {M}x{N} ld{ld}", "ElemFp4", rung, M, N, ld, k_pair("fp4", ld)[0],
                        bias=(None, "int", "frac")[v % 3], variant=v))
    return out


REFUSALS = [(30, 96), (31, 64)]         # (variant, row stride in words) -> QT_ERR_ALIGNMENT, Y untouched


def all_dense_cases():
    return dense_cases() + long_k_cases() + store_path_cases() + special_cases() + variant_cases()


# ---- the batched family: qt_i8_gemm_splitk --------------------------------------------------------------------------------------

@dataclass
class SplitKCase:
    name: str
    rung: str
    M: int
    N: int
    nslice: int
    kslice: int
    K: int                     # ends inside the last slice
    seed: int

    @property
    def ld(self):              # words: nslice * kslice bytes, a whole number of 128-byte stages
        return self.nslice * self.kslice // 4

    @property
    def ldy(self):
        return (self.N + 3) // 4 * 4 + 4

    @property
    def y_stride(self):
        return (self.M + 2) * self.ldy + 4


SPLITK_SHAPES = [("PP256", 300, 250), ("PP192", 300, 190), ("PP192", 256, 190), ("PP128", 300, 120), ("PP64", 300, 60), ("PP64", 15, 7)]


def splitk_cases():
    out = []
    for i, (rung, M, N) in enumerate(SPLITK_SHAPES):
        for nslice, kslice, K in ((1, 128, 100), (3, 128, 300)):
            out.append(SplitKCase(f"splitk {rung} {M}x{N} nslice{nslice}", rung, M, N, nslice, kslice, K, 900 + 10 * i + nslice))
    return out


def splitk_operands(c: SplitKCase):
    return uniform_ints(c.seed, c.M, c.K, -127, 127), uniform_ints(c.seed + 1, c.N, c.K, -1, 1)
