"""Cases and input generation of the half-precision (bf16 / fp16) fixtures, shared by tests/golden/make_golden_half.py (which
runs the reference on them) and tests/test_half_cpu.py / test_gpu_half.py (which regenerate the same inputs).

Everything comes from the package's counter PRNG (synth), is rounded to the half dtype with torch's CPU conversion
(round-to-nearest-even, the same everywhere) and travels as uint16 bit patterns.

Independent random +-1 operands give sums below ~370, almost all representable in either dtype, so they could not tell
round-to-nearest-even from truncation.  The ``corr`` cases therefore use CORRELATED operands: every activation row and every
weight row is a noisy copy of one base +-1 vector (conv: one base sign per input channel, the same at every pixel and tap),
per-row flip rate uniform in [0, 0.1], random per-row sign; for ternary weights a fifth of the entries is then pushed inside
(-0.5, 0.5) so that it quantises to zero.
"""
import hashlib

import numpy as np
import torch

from pytorch_quantize_impls_amd import synth

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
KINDS = ("binary", "ternary")
#: (significand bits incl. the hidden one, bit pattern of 1.0, of 0.5, of +inf, smallest normal)
FORMAT = {"bf16": (8, 0x3F80, 0x3F00, 0x7F80, 0x0080), "fp16": (11, 0x3C00, 0x3800, 0x7C00, 0x0400)}


def bits(t: torch.Tensor) -> np.ndarray:
    """uint16 bit patterns of a half tensor (contiguous, logical order)."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(a: np.ndarray, dt) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).view(dt)


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(bits(t).tobytes()).hexdigest()


def edge_bits(name: str) -> np.ndarray:
    """0, -0, +-smallest subnormal, +-smallest normal, +-0.5, +-(0.5 one ulp either side), +-1, +-(1 one ulp above), +-inf, nan."""
    _, one, half, inf, minnorm = FORMAT[name]
    pos = [0x0000, 0x0001, minnorm, half - 1, half, half + 1, one, one + 1, inf]
    v = []
    for p in pos:
        v += [p, p | 0x8000]
    v += [inf + 1, (inf + 1) | 0x8000, 0x7FFF]          # NaNs of both signs
    while len(v) % 8:                                   # whole 16-byte vectors as well as a ragged tail in the 2-D view
        v.append(one)
    return np.array(v, dtype=np.uint16)


def _flip(x: np.ndarray, rate: np.ndarray, seed: int) -> np.ndarray:
    u = synth.uniform01(seed, x.size).reshape(x.shape)
    return np.where(u < rate, -x, x).astype(np.float32)


def pm1_rows(seed: int, rows: int, K: int, corr: bool) -> np.ndarray:
    """[rows, K] +-1 fp32: fair coins, or noisy signed copies of the base vector of ``seed & ~0xFF``."""
    if not corr:
        return synth.pm1(seed, (rows, K))
    base = synth.pm1(seed & ~0xFF, (1, K))
    rate = (0.1 * synth.uniform01(seed + 1, rows)).reshape(rows, 1)
    sign = synth.pm1(seed + 2, (rows, 1))
    return _flip(np.broadcast_to(base, (rows, K)).copy(), rate, seed + 3) * sign


def weight_rows(seed: int, rows: int, K: int, corr: bool, kind: str) -> np.ndarray:
    """Real-valued [rows, K] fp32 weight whose quantised image is random (uniform in [-1.2, 1.2)) or correlated."""
    if not corr:
        return synth.uniform(seed, (rows, K), -1.2, 1.2)
    s = pm1_rows(seed, rows, K, True)
    mag = synth.uniform(seed + 4, (rows, K), 0.55, 1.2)
    if kind == "ternary":
        mag = np.where(synth.uniform01(seed + 5, rows * K).reshape(rows, K) < 0.2, np.float32(0.25), mag)
    return (s * mag).astype(np.float32)


def bias_vec(seed: int, n: int, mode: str):
    if mode == "none":
        return None
    if mode == "zero":
        return np.zeros((n,), dtype=np.float32)
    return (synth.normal(seed, (n,)) * 2.0).astype(np.float32)


def quantise(w: torch.Tensor, kind: str) -> torch.Tensor:
    """The deterministic quantiser's image by plain comparisons (what the layers multiply with)."""
    one = torch.ones((), dtype=w.dtype)
    if kind == "binary":
        return torch.where(w < 0, -one, one)
    return torch.where(w >= 0.5, one, torch.where(w < -0.5, -one, torch.zeros((), dtype=w.dtype)))


BIAS_MODES = ("nonzero", "zero", "none")


def linear_cases():
    """K in {31, 33, 96, 4097} x (batch, N) in {5, 128} x {7, 96}, bias mode cycling; K = 4097 uses correlated operands.
    Every case has gradients (case 5)."""
    out = []
    i = 0
    for K in (31, 33, 96, 4097):
        for B in (5, 128):
            for N in (7, 96):
                out.append({"name": f"lin_K{K}_B{B}_N{N}", "K": K, "B": B, "N": N, "bias": BIAS_MODES[i % 3], "corr": K == 4097,
                            "seed": 0x51000 + 0x100 * i, "grads": True})
                i += 1
    return out


def linear_inputs(case, kind: str, name: str):
    """(x [+-1], w, b or None) as CPU tensors of the half dtype."""
    dt = DTYPES[name]
    s = case["seed"] + (0x40000 if kind == "ternary" else 0)
    x = torch.from_numpy(pm1_rows(s + 0x10, case["B"], case["K"], case["corr"])).to(dt)
    w = torch.from_numpy(weight_rows(s + 0x20, case["N"], case["K"], case["corr"], kind)).to(dt)
    b = bias_vec(s + 0x30, case["N"], case["bias"])
    return x, w, (torch.from_numpy(b).to(dt) if b is not None else None)


def grad_out(case_seed: int, shape, name: str) -> torch.Tensor:
    return torch.from_numpy(synth.normal(case_seed + 0x70, shape)).to(DTYPES[name])


def conv_cases():
    """Cin in {32, 64, 192}, k in {1, 3, 5}, stride in {1, 2}, padding in {0, 1, 2}; two correlated 192 -> 64 5 x 5 cases that
    exercise the rounding; AlexNet's conv2 is a digest-only forward case, left out of the gradients on purpose (its fp64
    backward on the CPU takes longer than the rest of the file together).  The 7-filter case (ragged channel count: the
    element-wise store of the half epilogue) is forward only, and the 1 x 1 case has stride 2: the fp32 weight-gradient routes
    the half backward feeds take the counted dense library for stride-1 1 x 1 convs and for fewer than ~32 filters, in fp32 as
    in half — not what these fixtures are about."""
    raw = (("conv_32_40_k3", 2, 32, 40, 9, 3, 1, 1, False, True),
           ("conv_64_64_k1_s2", 2, 64, 64, 8, 1, 2, 0, False, True),
           ("conv_64_48_k5_s2", 2, 64, 48, 11, 5, 2, 2, False, True),
           ("conv_192_64_k3_s2", 2, 192, 64, 9, 3, 2, 0, False, True),
           ("conv_32_7_k3", 2, 32, 7, 6, 3, 1, 1, False, False),
           ("conv_corr_s1", 4, 192, 64, 13, 5, 1, 2, True, True),
           ("conv_corr_s2", 4, 192, 64, 13, 5, 2, 1, True, True),
           ("conv_alexnet2", 8, 192, 576, 27, 5, 1, 2, False, False))
    out = []
    for i, (nm, B, Cin, Cout, H, k, s, p, corr, grads) in enumerate(raw):
        out.append({"name": nm, "B": B, "Cin": Cin, "Cout": Cout, "H": H, "k": k, "stride": s, "pad": p, "corr": corr,
                    "bias": "zero" if nm == "conv_corr_s2" else BIAS_MODES[i % 3], "seed": 0x61000 + 0x100 * i, "grads": grads})
    return out


def conv_inputs(case, kind: str, name: str):
    dt = DTYPES[name]
    s = case["seed"] + (0x40000 if kind == "ternary" else 0)
    B, Cin, Cout, H, k = case["B"], case["Cin"], case["Cout"], case["H"], case["k"]
    if case["corr"]:
        # one base sign per input channel, the same at every pixel and tap; flip rate and sign per image / per filter
        base = synth.pm1(s & ~0xFF, (1, Cin, 1, 1))
        rate = (0.1 * synth.uniform01(s + 0x11, B)).reshape(B, 1, 1, 1)
        x = _flip(np.broadcast_to(base, (B, Cin, H, H)).copy(), rate, s + 0x13) * synth.pm1(s + 0x12, (B, 1, 1, 1))
        rate = (0.1 * synth.uniform01(s + 0x21, Cout)).reshape(Cout, 1, 1, 1)
        sg = _flip(np.broadcast_to(base, (Cout, Cin, k, k)).copy(), rate, s + 0x23) * synth.pm1(s + 0x22, (Cout, 1, 1, 1))
        mag = synth.uniform(s + 0x24, (Cout, Cin, k, k), 0.55, 1.2)
        if kind == "ternary":
            mag = np.where(synth.uniform01(s + 0x25, mag.size).reshape(mag.shape) < 0.2, np.float32(0.25), mag)
        w = (sg * mag).astype(np.float32)
    else:
        x = synth.pm1(s + 0x10, (B, Cin, H, H))
        w = synth.uniform(s + 0x20, (Cout, Cin, k, k), -1.2, 1.2)
    b = bias_vec(s + 0x30, Cout, case["bias"])
    return (torch.from_numpy(np.ascontiguousarray(x)).to(dt), torch.from_numpy(np.ascontiguousarray(w)).to(dt),
            torch.from_numpy(b).to(dt) if b is not None else None)


def c2_inputs():
    """The C2 step's shape, 4096^3 in bf16 (digest only)."""
    x = torch.from_numpy(synth.pm1(0x71010, (4096, 4096))).to(torch.bfloat16)
    w = torch.from_numpy(synth.uniform(0x71020, (4096, 4096), -1.2, 1.2)).to(torch.bfloat16)
    return x, w


def exact_linear(x, wq, b):
    """fp64 x . wq^T + b: exact for +-1 / 0 operands (integers below 2^24 plus a half-precision bias)."""
    y = x.double() @ wq.double().t()
    return y if b is None else y + b.double()


def exact_conv(x, wq, b, stride, pad):
    return torch.nn.functional.conv2d(x.double(), wq.double(), None if b is None else b.double(), stride, pad)


def rne_of_fl32(y64: torch.Tensor, dt) -> torch.Tensor:
    """The rule the fixtures obey: fl32(exact sum + bias), then one round-to-nearest-even to the half dtype."""
    return y64.float().to(dt)


def not_representable_share(y64: torch.Tensor, dt) -> float:
    return float((y64.float().to(dt).double() != y64).double().mean())


def tie_share(y64: torch.Tensor, dt, name: str) -> float:
    """Share of outputs exactly half way between two neighbours of the dtype (what separates nearest-even from the rest)."""
    p = FORMAT[name][0]
    a = y64.float().double().abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=1e-30)))
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (p - 1))
    r = torch.remainder(a, ulp)
    return float(((r * 2 == ulp) & (a > 0)).double().mean())


def ulp_of(t64: torch.Tensor, name: str) -> torch.Tensor:
    """One unit in the last place of the half dtype at |t| (normal range; the subnormal step below it)."""
    p, _, _, _, minnorm = FORMAT[name]
    emin = -126 if name == "bf16" else -14
    e = torch.floor(torch.log2(torch.clamp(t64.abs(), min=2.0 ** emin)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - (p - 1))
