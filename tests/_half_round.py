"""Round-to-nearest-even from float32 to bf16 / fp16 BIT PATTERNS, and the exact way back: numpy integer arithmetic only, no
torch and no numpy float16 cast — the reference side of the "_h" streaming convs (include/qt_hip.h "Depthwise and grouped
convolution on half-precision operands"): RNE(float32 restatement on the upcast operands).  Pinned against
``torch.Tensor.to(dtype)`` by tests/test_half_streaming_cpu.py.

fp32 is 1 | 8 | 23 bits (bias 127), bf16 1 | 8 | 7 (bias 127), fp16 1 | 5 | 10 (bias 15).  NaN goes to the canonical quiet NaN of
the target with the sign kept; compare NaNs as a class (``is_nan``)."""
import numpy as np

FORMATS = {"bf16": dict(inf=0x7F80, one=0x3F80, half=0x3F00, mant=7), "fp16": dict(inf=0x7C00, one=0x3C00, half=0x3800, mant=10)}


def _bits32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)


def _rne_shift(v, s):
    """v >> s (uint64 arrays, s >= 1 elementwise) rounded to nearest, ties to even."""
    q = v >> s
    rem = v & ((np.uint64(1) << s) - np.uint64(1))
    halfway = np.uint64(1) << (s - np.uint64(1))
    up = (rem > halfway) | ((rem == halfway) & ((q & np.uint64(1)) == 1))
    return q + up.astype(np.uint64)


def rne_bf16(x):
    """uint16 bf16 patterns of float32 ``x`` (any shape)."""
    u = _bits32(x)
    sign = (u >> np.uint64(16)) & np.uint64(0x8000)
    mag = u & np.uint64(0x7FFFFFFF)
    r = _rne_shift(mag, np.full(mag.shape, 16, dtype=np.uint64))          # a carry out of the mantissa moves into the exponent: inf at the top
    r = np.where(mag > 0x7F800000, np.uint64(0x7FC0), r)
    return (sign | r).astype(np.uint16)


def rne_fp16(x):
    """uint16 fp16 patterns of float32 ``x``: gradual underflow below 2^-14, overflow to inf from 65520 on."""
    u = _bits32(x)
    sign = (u >> np.uint64(16)) & np.uint64(0x8000)
    mag = u & np.uint64(0x7FFFFFFF)
    e = (mag >> np.uint64(23)).astype(np.int64)                            # biased fp32 exponent
    m = (mag & np.uint64(0x7FFFFF)) | np.where(e > 0, np.uint64(0x800000), np.uint64(0))      # 24-bit significand (fp32 subnormal: no hidden bit)
    # normal fp16 results: drop 13 mantissa bits of (exponent | mantissa) re-biased by 127 - 15
    norm = _rne_shift(np.where(e >= 113, mag - np.uint64(112 << 23), np.uint64(0)), np.full(mag.shape, 13, dtype=np.uint64))
    # subnormal fp16 results: value = m 2^(e - 150) in units of 2^-24 -> shift right by 126 - e (at least 14; 25 and more give 0 or 1 ulp)
    sh = np.clip(126 - np.maximum(e, 1), 14, 40).astype(np.uint64)
    sub = _rne_shift(m, sh)
    r = np.where(e >= 113, norm, sub)
    r = np.where(r >= 0x7C00, np.uint64(0x7C00), r)                        # overflow (and inf itself)
    r = np.where(mag > 0x7F800000, np.uint64(0x7E00), r)
    return (sign | r).astype(np.uint16)


def bf16_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def fp16_to_f32(b):
    b = np.asarray(b, dtype=np.uint16).astype(np.uint32)
    sign = (b & np.uint32(0x8000)) << np.uint32(16)
    e = ((b >> np.uint32(10)) & np.uint32(0x1F)).astype(np.int64)
    m = (b & np.uint32(0x3FF)).astype(np.int64)
    val = np.where(e == 0, m * 2.0 ** -24, (1024 + m) * 2.0 ** (e - 25.0))                     # exact in float64
    out = val.astype(np.float32).view(np.uint32)                           # exact: 11 significant bits, exponents inside fp32's
    out = np.where(e == 31, np.uint32(0x7F800000) | (m.astype(np.uint32) << np.uint32(13)), out)
    return (out.astype(np.uint32) | sign).view(np.float32)


ROUND = {"bf16": rne_bf16, "fp16": rne_fp16}
UPCAST = {"bf16": bf16_to_f32, "fp16": fp16_to_f32}


def is_nan(bits, fmt):
    return (np.asarray(bits, dtype=np.uint16) & np.uint16(0x7FFF)) > FORMATS[fmt]["inf"]


def same_bits(got, want, fmt):
    """Equal 16-bit patterns, NaN compared as a class.  Returns (ok, number of differing elements)."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    gn, wn = is_nan(got, fmt), is_nan(want, fmt)
    bad = (gn != wn) | (~gn & (got != want))
    return not bad.any(), int(bad.sum())


def half_ulp(v64, fmt):
    """Half a unit in the last place of the target format at |v64| (float64 array): the margin of ONE rounding to nearest."""
    mant = FORMATS[fmt]["mant"]
    emin = -126 if fmt == "bf16" else -14
    a = np.abs(np.asarray(v64, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -200)))
    # a value that rounds up to the next binade has the larger spacing there; taking the binade of |v| itself is the smaller
    # (stricter) margin except exactly at the carry, where the rounded value is a power of two and both spacings admit it
    return 2.0 ** (np.maximum(e, emin) - mant - 1)
