"""Exact float64 references for the backward contractions of the quantised layers, shared by the tests (a plain module, not a
conftest).  Every function works on any device; the references run where their inputs live, in float64, chunked under a byte
budget like tests/_exact.py.

Every backward contraction of these layers has one operand that is exact in 16 bits (+-1 / 0 weights or activations, k-bit
codes, odd integer DoReFa levels, an integer image).  With the other operand a small integer times a power of two, every
product and every partial sum is an integer multiple of the smallest product's quantum, below 2^24 of them: exact in fp32,
whatever the summation order.  ``proves_exact`` checks that claim for the actual tensors, emulating the route's split of the
real operand (two fp16 terms of x / s with a power-of-two s per tensor or per channel, or three bf16 terms); a test demands
bit equality only after it holds.  The routes' epilogues (fl(S * scale), chunked fp32 accumulation, the STE mask
!(|w| <= thr)) are restated here as the same fp32 operations in the same order."""
import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
STE_THRESHOLD = 1.001          # ops.STE_THRESHOLD (functions/binary_connect.py:37), restated
BUDGET = 1 << 30               # bytes of float64 temporaries per reference chunk


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(t) for t in v)


def _step(bytes_per_image: int, budget: int) -> int:
    return max(1, int(budget // max(1, int(bytes_per_image))))


# ---- float64 references -------------------------------------------------------------------------------------------------------

def conv_grad_input64(g: torch.Tensor, w: torch.Tensor, input_hw, stride=1, padding=0, budget: int = BUDGET) -> torch.Tensor:
    """grad wrt the input of conv2d(x, w) (no dilation, groups 1): col2im(W^T . g) in float64 -> [N, Cin, H, W]."""
    N, Cout, Ho, Wo = (int(v) for v in g.shape)
    Co2, Cin, kh, kw = (int(v) for v in w.shape)
    assert Co2 == Cout
    H, W = (int(v) for v in input_hw)
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    assert (H + 2 * ph - kh) // sh + 1 == Ho and (W + 2 * pw - kw) // sw + 1 == Wo, "shapes do not belong together"
    wt = w.detach().to(F64).reshape(Cout, Cin * kh * kw).t()
    out = torch.empty((N, Cin, H, W), dtype=F64, device=g.device)
    step = _step(8 * (2 * Cin * kh * kw * Ho * Wo + Cout * Ho * Wo + Cin * H * W), budget)
    for n0 in range(0, N, step):
        gs = g[n0:n0 + step].detach().to(F64).reshape(-1, Cout, Ho * Wo)
        out[n0:n0 + step] = F.fold(torch.matmul(wt, gs), (H, W), (kh, kw), padding=(ph, pw), stride=(sh, sw))
    return out


def conv_grad_weight64(x: torch.Tensor, g: torch.Tensor, kernel_hw, stride=1, padding=0, chunks=None,
                       budget: int = BUDGET):
    """grad wrt the weight of conv2d(x, w): sum over images and output positions of g x unfold(x), float64 [Cout, Cin, kh, kw].
    ``chunks``: a list of image counts that partitions the batch (the route's chunk plan) -> one partial sum per chunk."""
    N, Cin, H, W = (int(v) for v in x.shape)
    N2, Cout, Ho, Wo = (int(v) for v in g.shape)
    kh, kw = _pair(kernel_hw)
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    assert N2 == N and (H + 2 * ph - kh) // sh + 1 == Ho and (W + 2 * pw - kw) // sw + 1 == Wo
    chunks = [N] if chunks is None else [int(c) for c in chunks]
    assert sum(chunks) == N and min(chunks) > 0
    step = _step(8 * (2 * Cin * kh * kw + 2 * Cout) * Ho * Wo, budget)
    out, n0 = [], 0
    for cnt in chunks:
        acc = torch.zeros((Cout, Cin * kh * kw), dtype=F64, device=g.device)
        for m0 in range(n0, n0 + cnt, step):
            m1 = min(n0 + cnt, m0 + step)
            cols = F.unfold(x[m0:m1].detach().to(F64), (kh, kw), padding=(ph, pw), stride=(sh, sw))    # [n, Cin k k, L]
            gs = g[m0:m1].detach().to(F64).reshape(m1 - m0, Cout, Ho * Wo)
            acc += torch.matmul(gs, cols.transpose(1, 2)).sum(0)
        out.append(acc.view(Cout, Cin, kh, kw))
        n0 += cnt
    return out if len(chunks) > 1 else out[0]


def bias_grad64(g: torch.Tensor) -> torch.Tensor:
    """sum of the gradient over (n, y, x) per channel, float64."""
    return g.detach().to(F64).sum((0, 2, 3)) if g.dim() == 4 else g.detach().to(F64).sum(0)


def linear_grad_x64(g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """grad wrt x of x . w^T: g . w, float64."""
    return torch.matmul(g.detach().to(F64), w.detach().to(F64))


def linear_grad_w64(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """grad wrt w of x . w^T: g^T . x, float64."""
    return torch.matmul(g.detach().to(F64).t(), x.detach().to(F64))


# ---- the routes' fp32 epilogues -----------------------------------------------------------------------------------------------

def to_f32_exact(s64: torch.Tensor, what: str = "sum") -> torch.Tensor:
    """A float64 sum that the exactness proof says is an fp32 value -> that fp32 tensor (asserts the claim)."""
    s32 = s64.to(F32)
    assert torch.equal(s32.to(F64), s64), f"{what}: the float64 sum is not representable in fp32 (the proof does not hold)"
    return s32


def scaled(s32: torch.Tensor, scale) -> torch.Tensor:
    """fl(S * scale) in fp32: ``scale`` a Python float taken as fp32 (fl(1 / n) of ops._inv_f32) or a one-element fp32 tensor."""
    sc = scale.to(F32).reshape(()) if isinstance(scale, torch.Tensor) else torch.tensor(float(scale), dtype=F32)
    return torch.mul(s32, sc.to(s32.device))


def chunked_sum(partials64, scale=1.0, what: str = "dW") -> torch.Tensor:
    """dW = fl(S_0 scale); dW = fl(dW + fl(S_c scale)) for the chunks in order (the reduce kernels' accumulate flag)."""
    acc = None
    for i, s64 in enumerate(partials64 if isinstance(partials64, (list, tuple)) else [partials64]):
        v = scaled(to_f32_exact(s64, f"{what} chunk {i}"), scale)
        acc = v if acc is None else torch.add(acc, v)
    return acc


def ste_mask(dW: torch.Tensor, w: torch.Tensor, thr: float = STE_THRESHOLD) -> torch.Tensor:
    """The reduce kernels' mask: v = 0 where !(fabsf(w) <= thr) (thr as fp32; NaN weights are masked)."""
    keep = torch.le(w.detach().to(F32).abs(), torch.tensor(thr, dtype=F32, device=w.device))
    return torch.where(keep, dW, torch.zeros((), dtype=dW.dtype, device=dW.device))


def safe_sign(w: torch.Tensor) -> torch.Tensor:
    """safeSign: +1 for w >= 0, -1 below (functions/common.py)."""
    return torch.where(w.detach() >= 0, 1.0, -1.0).to(F32)


# ---- operand generators -------------------------------------------------------------------------------------------------------

def _gen(seed: int, device):
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    return gen


def grad_ints(shape, amp: int, seed: int, device, exp: int = 0, ch_exps=None, channels_last: bool = True,
              zeros: bool = True) -> torch.Tensor:
    """Gradient = integers in [-amp, amp] (no zeros unless ``zeros``) times 2^exp, or times 2^ch_exps[c] per channel (dim 1)."""
    gen = _gen(seed, device)
    q = torch.randint(-amp, amp + 1, tuple(shape), generator=gen, device=device).to(F32)
    if not zeros:
        q = torch.where(q == 0, float(amp), q)
    if ch_exps is not None:
        e = torch.as_tensor(ch_exps, dtype=F32, device=device)
        q = q * torch.exp2(e).reshape((1, -1) + (1,) * (len(shape) - 2))
    else:
        q = q * 2.0 ** exp
    if channels_last and len(shape) == 4:
        q = q.contiguous(memory_format=torch.channels_last)
    return q


def spread_exps(C: int, lo: int, hi: int, seed: int) -> torch.Tensor:
    """Per-channel exponents in [lo, hi] (host int tensor), both ends present."""
    e = torch.randint(lo, hi + 1, (C,), generator=_gen(seed, "cpu"))
    e[0], e[-1] = lo, hi
    return e


def pm1(shape, seed: int, device, zero_frac: float = 0.0, channels_last: bool = True) -> torch.Tensor:
    gen = _gen(seed, device)
    v = torch.where(torch.rand(tuple(shape), generator=gen, device=device) < 0.5, -1.0, 1.0)
    if zero_frac:
        v = torch.where(torch.rand(tuple(shape), generator=gen, device=device) < zero_frac, 0.0, v)
    return v.contiguous(memory_format=torch.channels_last) if channels_last and len(shape) == 4 else v


def int_uniform(shape, lo: int, hi: int, seed: int, device, channels_last: bool = True) -> torch.Tensor:
    v = torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed, device), device=device).to(F32)
    return v.contiguous(memory_format=torch.channels_last) if channels_last and len(shape) == 4 else v


def latent_weight(shape, seed: int, device, lo: float = -1.5, hi: float = 1.5) -> torch.Tensor:
    """Latent weights, some beyond the STE threshold, none exactly on it."""
    w = torch.empty(tuple(shape), device=device).uniform_(lo, hi, generator=_gen(seed, device))
    return torch.where((w.abs() - STE_THRESHOLD).abs() < 1e-4, 0.5 * w, w)


# ---- the exactness proof ------------------------------------------------------------------------------------------------------

def quantum_exp(t: torch.Tensor):
    """Largest k with every element an integer multiple of 2^k (None for an all-zero tensor)."""
    a = t.detach().to(F64).abs().reshape(-1)
    a = a[a > 0]
    if a.numel() == 0:
        return None
    m, e = torch.frexp(a)                                           # a = m 2^e, m in [0.5, 1)
    M = torch.ldexp(m, torch.full_like(e, 53)).to(torch.int64)      # exact 53-bit integer significand
    low = (M & -M).to(F64)                                          # its lowest set bit
    return int((e.to(torch.int64) - 53 + torch.log2(low).round().to(torch.int64)).min())


def _pow2_exp(absmax: torch.Tensor) -> torch.Tensor:
    """split_f16.hip write_scale: s = 2^k with absmax / s in [2^14, 2^15), k clamped to [-100, 100]; s = 1 for 0 / inf."""
    _, e = torch.frexp(absmax.to(F32))
    k = (e.to(torch.int64) - 15).clamp(-100, 100)
    ok = (absmax > 0) & torch.isfinite(absmax)
    return torch.where(ok, k, torch.zeros_like(k))


def split_terms(v: torch.Tensor, split: str, channel_dim=None):
    """The route's split of a real operand, emulated on the host types: "f16x2" = fp16 hi / lo of v / s with s a power of two
    per tensor (``channel_dim`` None) or per channel; "bf16x3" = three bf16 terms of v.  Returns (terms as float64 tensors in
    the units of v, whether they reproduce v exactly)."""
    v = v.detach().to(F32)
    if split == "bf16x3":
        hi = v.to(torch.bfloat16).to(F32)
        mid = (v - hi).to(torch.bfloat16).to(F32)
        lo = (v - hi - mid).to(torch.bfloat16).to(F32)
        terms = [hi.to(F64), mid.to(F64), lo.to(F64)]
    elif split == "f16x2":
        if channel_dim is None:
            k = _pow2_exp(v.abs().amax())
        else:
            dims = [d for d in range(v.dim()) if d != channel_dim]
            k = _pow2_exp(v.abs().amax(dim=dims, keepdim=True))
        s = torch.exp2(k.to(F64))                                       # exact for |k| <= 100
        y = v.to(F64) / s                                               # exact: s is a power of two
        hi = y.to(F32).to(torch.float16).to(F64)
        lo = (y - hi).to(F32).to(torch.float16).to(F64)                # y - hi is exact in fp32 (split_f16.hip)
        terms = [hi * s, lo * s]
        if not torch.equal(y.to(F32).to(F64), y):
            return terms, False
    else:
        raise ValueError(split)
    return terms, bool(torch.equal(terms[0] + terms[1] if len(terms) == 2 else (terms[0] + terms[1]) + terms[2], v.to(F64)))


def exact_in(v: torch.Tensor, dtype) -> bool:
    return bool(torch.equal(v.detach().to(dtype).to(F64), v.detach().to(F64)))


def proves_exact(a: torch.Tensor, b: torch.Tensor, contract, split_a: str = "bf16x3", a_channel_dim=None, split_b=None,
                 b_channel_dim=None, out_channel_dim=None, b_exact_in=(torch.float16, torch.bfloat16)):
    """Proof that every correct summation order of ``contract(a, b)`` gives the float64 value in fp32.  ``a``: the real operand
    the route splits (``split_a``, per tensor / per ``a_channel_dim``); ``b``: the operand as the kernel reads it (exact in
    fp16 and bf16 unless ``split_b`` says how the route splits it).  ``contract(p, q)`` is the float64 reference of the
    contraction (bilinear, non-negative on non-negative operands).  ``out_channel_dim``: the dimension of the result that sees
    one channel (``a_channel_dim``) of ``a`` only (a row of dW, the bias): the bound is then taken per channel, in units of
    that channel's quantum.  ``b_exact_in``: the 16-bit types the route reads ``b`` in.  Returns (ok, reason)."""
    ta, ok = split_terms(a, split_a, a_channel_dim)
    if not ok:
        return False, f"the {split_a} split does not reproduce the real operand"
    if split_b is None:
        if not all(exact_in(b, t) for t in b_exact_in):
            return False, "the exact operand is not exact in fp16 / bf16"
        tb = [b.detach().to(F64)]
    else:
        tb, ok = split_terms(b, split_b, b_channel_dim)
        if not ok:
            return False, f"the {split_b} split does not reproduce the second operand"
    qb = [q for q in (quantum_exp(t) for t in tb) if q is not None]
    sums = contract(sum(t.abs() for t in ta), sum(t.abs() for t in tb))
    if out_channel_dim is None:
        rows = [(ta, sums)]
    else:
        C = int(a.shape[a_channel_dim])
        rows = [([t.select(a_channel_dim, c) for t in ta], sums.select(out_channel_dim, c)) for c in range(C)]
    worst = None
    for terms, s in rows:
        qa = [q for q in (quantum_exp(t) for t in terms) if q is not None]
        if not qa or not qb:
            continue
        unit = min(qa) + min(qb)
        bound = float(s.max())
        if unit < -126 or bound >= 2.0 ** 127:
            return False, f"outside the normal fp32 range (unit 2^{unit}, bound {bound})"
        if bound >= 2.0 ** (24 + unit):
            return False, f"sum of |terms| {bound} >= 2^24 units of 2^{unit}"
        r = bound / 2.0 ** unit
        worst = r if worst is None else max(worst, r)
    return True, "zero operand" if worst is None else f"bound {worst:.0f} units < 2^24"


# ---- mismatch reports ---------------------------------------------------------------------------------------------------------

def mismatch_report(got: torch.Tensor, want: torch.Tensor, names=("co", "ci", "ky", "kx"), limit: int = 8, what: str = "") -> str:
    """'' if got equals want bit for bit (NaN == NaN), else the count and the first ``limit`` indices with both values."""
    assert tuple(got.shape) == tuple(want.shape), f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    g, w = got.detach().to(F64), want.detach().to(F64)
    diff = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
    cnt = int(diff.sum())
    if cnt == 0:
        return ""
    idx = diff.nonzero()[:limit].tolist()
    lines = [f"{what}: {cnt} of {diff.numel()} values differ; first {len(idx)}:"]
    for ix in idx:
        pos = ", ".join(f"{n}={i}" for n, i in zip(names, ix))
        lines.append(f"  ({pos}) got {float(g[tuple(ix)])!r} want {float(w[tuple(ix)])!r}")
    return "\n".join(lines)
