"""Exact reference for the threshold-bit convs on +-1 activations, shared by the tests (a plain module, not a conftest).

Every function works on any device.  The conv of +-1 activations with +-1 / 0 weights is a sum of at most Cin*k*k integers of
magnitude 1, so it is computed in float64 (explicit unfold + matmul: no algorithm choice that could round) and checked against
that bound — the result is then the exact integer.  The threshold predicate is the fused blocks' expression evaluated with
separate fp32 operations (the kernels compile with -ffp-contract=off):

    bit = fl(fl(fl(acc + bias) * alpha) + beta) < 0        (bit 1 <=> the activation is -1)

which is the form ops.integer_thresholds solves for.  Bit planes follow ops.BitPlanes (bit c of word c >> 5 of a pixel row,
1 = negative, bits past C zero); nibble planes ops.NibPlanes (channel c in nibble c & 7 of word c >> 3: +1 = 0x2, -1 = 0xA,
0 = 0x0) with a zero halo of (hy, hx) pixels around every image."""
import torch
import torch.nn.functional as F

NIB_POS, NIB_NEG = 0x2, 0xA


def _shifts(n, device):
    return torch.arange(n, device=device, dtype=torch.int32)


def packed_ld(C: int) -> int:
    """Words per row of a bit plane (ops.packed_ld, restated so that the helper needs no HIP library)."""
    return max(4, ((int(C) + 31) // 32 + 3) // 4 * 4)


def random_bit_words(rows: int, C: int, seed: int, device, ld=None) -> torch.Tensor:
    """int32 [rows, ld] of fair random bits for channels 0..C-1 (zeros past C), drawn on ``device`` by a seeded torch.Generator."""
    ld = packed_ld(C) if ld is None else int(ld)
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    nw = (int(C) + 31) // 32
    w = torch.randint(0, 1 << 32, (int(rows), nw), generator=gen, device=device, dtype=torch.int64)
    if C % 32:
        w[:, -1] &= (1 << (C % 32)) - 1
    w = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    out = torch.zeros((int(rows), ld), dtype=torch.int32, device=device)
    out[:, :nw] = w
    return out


def bits_of_words(words: torch.Tensor, C: int) -> torch.Tensor:
    """int32 [..., ld] bit-plane rows -> bool [..., C] (True = bit set = -1)."""
    nw = (int(C) + 31) // 32
    b = (words[..., :nw].unsqueeze(-1) >> _shifts(32, words.device)) & 1
    return b.reshape(*words.shape[:-1], nw * 32)[..., :C].bool()


def words_of_bits(bits: torch.Tensor, ld=None) -> torch.Tensor:
    """bool [..., C] -> int32 [..., ld] bit-plane rows (the inverse of bits_of_words)."""
    C = int(bits.shape[-1])
    ld = packed_ld(C) if ld is None else int(ld)
    nw = (C + 31) // 32
    b = F.pad(bits.to(torch.int64), (0, nw * 32 - C)).reshape(*bits.shape[:-1], nw, 32)
    w = (b << torch.arange(32, device=bits.device, dtype=torch.int64)).sum(-1)
    w = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
    return F.pad(w, (0, ld - nw))


def check_pad_bits(words: torch.Tensor, C: int, what="bit plane"):
    """Bits past C (and the pad words) of a bit plane must be zero."""
    nw = (int(C) + 31) // 32
    if C % 32:
        tail = words[..., nw - 1] & ~((1 << (C % 32)) - 1)
        assert not bool(tail.any()), f"{what}: bits past channel {C} are set"
    assert not bool(words[..., nw:].any()), f"{what}: pad words are not zero"


def pm1_nchw(words: torch.Tensor, N: int, H: int, W: int, C: int, dtype=torch.float64) -> torch.Tensor:
    """Bit-plane rows of N images [N*H*W, ld] -> +-1 [N, C, H, W] (bit set = -1)."""
    b = bits_of_words(words.reshape(N, H, W, -1), C)
    return (1 - 2 * b.to(dtype)).permute(0, 3, 1, 2)


def decode_nib(words: torch.Tensor, N: int, H: int, W: int, C: int, halo=(1, 1)) -> torch.Tensor:
    """Nibble halo plane [N*(H+2hy)*(W+2hx), ld] -> int32 nibble values [N, H, W, C] of the interior.  Asserts that every nibble
    of the plane is 0x0, 0x2 or 0xA, that the halo and the pad channels are zero."""
    hy, hx = (int(v) for v in halo)
    ld = int(words.shape[-1])
    nib = ((words.reshape(N, H + 2 * hy, W + 2 * hx, ld).unsqueeze(-1) >> (4 * _shifts(8, words.device))) & 0xF)
    nib = nib.reshape(N, H + 2 * hy, W + 2 * hx, ld * 8)
    bad = (nib != 0) & (nib != NIB_POS) & (nib != NIB_NEG)
    assert not bool(bad.any()), f"{int(bad.sum())} nibbles outside {{0x0, 0x2, 0xA}}"
    inner = nib[:, hy:hy + H, hx:hx + W]
    assert int(nib.count_nonzero()) == int(inner.count_nonzero()), "the halo of a nibble plane must be zero"
    assert not bool(inner[..., C:].any()), "pad channels of a nibble plane must be zero"
    return inner[..., :C]


def nib_to_bits(nib: torch.Tensor) -> torch.Tensor:
    """Nibble values of a +-1 activation -> bool (True = -1); a zero nibble inside the image is an error."""
    zero = nib == 0
    assert not bool(zero.any()), f"{int(zero.sum())} zero nibbles inside a +-1 activation"
    return nib == NIB_NEG


def conv64(x: torch.Tensor, w: torch.Tensor, stride=1, padding=0, dilation=1) -> torch.Tensor:
    """conv2d [n, C, H, W] x [Cout, C, kh, kw] -> [n, Cout, Ho, Wo] in float64 via unfold + matmul, no bias.  ``stride``,
    ``padding`` and ``dilation``: an int or an (h, w) pair each; the kernel need not be square."""
    n, C, H, W = (int(v) for v in x.shape)
    Cout, Cw, kh, kw = (int(v) for v in w.shape)
    assert Cw == C
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (padding, padding) if isinstance(padding, int) else padding
    dh, dw = (dilation, dilation) if isinstance(dilation, int) else dilation
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    cols = F.unfold(x.to(torch.float64), (kh, kw), dilation=(dh, dw), padding=(ph, pw), stride=(sh, sw))       # [n, C*kh*kw, Ho*Wo]
    return torch.matmul(w.to(torch.float64).reshape(Cout, C * kh * kw), cols).reshape(n, Cout, Ho, Wo)


def exact_conv(x: torch.Tensor, w: torch.Tensor, stride=1, padding=0) -> torch.Tensor:
    """conv64 of a +-1 (or 0) input with +-1 / 0 weights.  Asserts |acc| <= C*kh*kw: the result is the exact integer sum."""
    acc = conv64(x, w, stride, padding)
    kmax = int(w[0].numel())
    amax = float(acc.abs().max()) if acc.numel() else 0.0
    assert amax <= kmax, f"|acc| = {amax} > Cin*k*k = {kmax}: the operands are not +-1 / 0"
    return acc


def predicate(acc: torch.Tensor, bias, alpha: torch.Tensor, beta: torch.Tensor, cdim: int = 1):
    """The threshold bit and the folded value v, fp32 with one rounding per operation: v = fl(fl(fl(acc + bias) * alpha) + beta),
    bit = v < 0.  ``acc`` holds exact integers (any float dtype); channels along ``cdim``."""
    shape = [1] * acc.dim()
    shape[cdim] = -1
    t = acc.to(torch.float32)
    if bias is not None:
        t = torch.add(t, bias.to(torch.float32).reshape(shape))
    t = torch.mul(t, alpha.to(torch.float32).reshape(shape))
    v = torch.add(t, beta.to(torch.float32).reshape(shape))
    return torch.lt(v, 0), v


def mismatch_report(got: torch.Tensor, want: torch.Tensor, acc=None, v=None, images=None, limit: int = 8, what="") -> str:
    """'' if got == want, else the mismatch count and the first ``limit`` (n, y, x, c) with the exact sum and the folded value.
    got / want: bool [n, H, W, C]; acc / v: the same layout (or None); images: the batch index of each of the n images."""
    diff = got != want
    cnt = int(diff.sum())
    if cnt == 0:
        return ""
    idx = diff.nonzero()[:limit].tolist()
    lines = [f"{what}: {cnt} of {diff.numel()} bits differ; first {len(idx)}:"]
    for n, y, x, c in idx:
        s = f"  (n={n if images is None else int(images[n])}, y={y}, x={x}, c={c}) got {int(got[n, y, x, c])} want {int(want[n, y, x, c])}"
        if acc is not None:
            s += f" acc={float(acc[n, y, x, c]):.0f}"
        if v is not None:
            s += f" v={float(v[n, y, x, c])!r}"
        lines.append(s)
    return "\n".join(lines)


def image_chunk(bytes_per_image: int, budget: int = 1 << 30) -> int:
    """Images per reference chunk so that the chunk's largest temporary stays under ``budget`` bytes."""
    return max(1, int(budget // max(1, int(bytes_per_image))))


def conv_bytes_per_image(C: int, H: int, W: int, Cout: int, k: int, stride: int = 1, padding: int = 0) -> int:
    """float64 bytes of the unfolded input plus the result of one image (exact_conv's temporaries)."""
    Ho, Wo = (H + 2 * padding - k) // stride + 1, (W + 2 * padding - k) // stride + 1
    return 8 * Ho * Wo * (C * k * k + 2 * Cout) + 8 * C * H * W


def tie_flips(got: torch.Tensor, v64: torch.Tensor):
    """Real-valued layers, where the device's fp32 accumulation may round differently from float64: the bits that differ from the
    float64 predicate (v64 < 0) and the largest |v| among them relative to mean|v|.  Returns (flips, worst)."""
    diff = got != (v64 < 0)
    flips = int(diff.sum())
    if flips == 0:
        return 0, 0.0
    a = v64.abs()
    return flips, float(a[diff].max()) / float(a[torch.isfinite(a)].mean())
