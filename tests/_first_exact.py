"""Exact float64 references for the forward conv of a REAL-valued image with +-1 / 0 weights (BinConv2d / TerConv2d) or XNOR-Net's
sign(W) * alpha, the network's first layer (functions/_fused.py ``first_layer_conv_routes``), shared by the tests: a plain module,
not a conftest; nothing here imports the package.  Everything runs on the CPU in float64: the shapes are small.

The routes split the image for the matrix cores: two fp16 terms of x / s with a power-of-two s per tensor (the pack kernels) or
per tile (``first3x3``, ``first_direct``: the patch is split in LDS with the TILE's max|x|), or three bf16 terms.  An image of
integers m times ONE quantum 2^q with |m| < 2^21 is reproduced exactly by hi + lo of the pair split under every admissible scale
(max / s in [2^8, 2^15) for whatever region the maximum is taken over: x / s is then a multiple of 2^-13 or more, above fp16's
subnormal grid 2^-24, with at most 21 significant bits = 11 + (sign of lo) + 10) and by the bf16 triple (3 x 8 bits).
``assert_image`` checks that property for the actual tensor, for every scale from an element's own binade up to the tensor's.
With every product a multiple of 2^q times the weight's quantum and the sum of the |products| plus |bias| below 2^24 of those units
(``proves``: tests/_grad_exact.py ``proves_exact`` on the actual operands), every partial sum of every summation order is an fp32
value: the fp32 result must equal the float64 sum BIT FOR BIT, and the threshold bits are tests/_exact.py ``predicate`` of it.

The designs differ in what they populate.  The last term of a split (``lo`` of the pair, the third bf16 term) is non-zero only for
an element with more than 11 / 17 significant bits, and the bound of 2^24 units caps the amplitude of a dense image at 2^24 / K:
  * ``dense``   every pixel non-zero, |m| in [2^(b-1), 2^b) with b the largest the proof accepts;
  * ``sparse``  |m| in [2^20, 2^21) on a share of the pixels, the largest share (a power of 1/2) the proof accepts: the third bf16
                term stays populated at K = 363, where a dense image cannot reach 19 bits;
  * ``ramp``    |m| = r 2^e with r of 13 (pairs) / 19 (triples) bits and e growing along H, along W and with the channel, thinned
                like ``sparse``: neighbouring tiles get different scales, small channels sit next to large ones.
Every design holds +0 and -0 pixels and, for a batch of two or more, an all-zero last image (with one -0); a batch of three holds
an image whose rows from 31 on are zero: a ``first3x3`` tile (32 x 32 outputs, 34 x 34 patch) with max|x| = 0."""
import zlib

import torch
import torch.nn.functional as F

import _exact as X
import _grad_exact as G
import _xnor_exact as XN

F64, F32 = torch.float64, torch.float32
M_BITS = 21                     # |m| < 2^21: one bit of margin below the 22 the pair split holds
NEED_BITS = {"f16x2": 11, "bf16x3": 17}      # an element with more significant bits can have a non-zero last term (each bf16
                                             # term after the first gains a bit from the sign of the remainder: 8 + 9 + ...)
COVERAGE = 0.25                 # share of the non-zero elements whose last term must be non-zero
BIAS_QUANTA = 8
MIN_NONZERO = 6                 # non-zero elements below which a thinned design is no test
DESIGNS = ("dense", "sparse", "ramp")
QUANTA = (-18, -9)              # 2^q: max|x| ~ 2^2 (the speculative s2d scale stands) and ~ 2^11 (it is repacked)

_pair = G._pair
out_hw = XN.out_hw


def seed_of(*parts) -> int:
    return zlib.crc32("/".join(str(p) for p in parts).encode()) % 1000003


def _gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return g


# ---- weights ------------------------------------------------------------------------------------------------------------------

def weights(kind: str, shape, seed: int, x_bits: int = 13):
    """(latent weight the entry points take, the weight image they must compute with, the image's quantum exponent).
    "binary": +-0.75 -> +-1; "ternary": {-0.75, 0, 0.75} -> {-1, 0, 1}; "xnor": +-2^{e_t} per tap (alpha_t = 2^{e_t}, the image is
    the weight itself) over the span _xnor_exact.tap_design allows for images of ``x_bits`` bits."""
    Cout, C, kh, kw = (int(v) for v in shape)
    g = _gen(seed)
    if kind == "xnor":
        exps, _, _ = XN.tap_design(kh * kw, C, "plain", x_absmax=2.0 ** x_bits, bias_quanta=BIAS_QUANTA)
        w = XN.pow2_tap_weight(shape, exps, seed, "cpu")
        return w, w.clone(), min(exps)
    if kind == "binary":
        wq = torch.randint(0, 2, tuple(shape), generator=g).to(F32) * 2 - 1
    else:
        assert kind == "ternary", kind
        wq = torch.randint(-1, 2, tuple(shape), generator=g).to(F32)
    return wq * 0.75, wq, 0


def bias_of(Cout: int, unit_exp: int, seed: int) -> torch.Tensor:
    """Integers in [-8, 8] (a zero among them) times the unit 2^unit_exp of the products."""
    b = torch.randint(-BIAS_QUANTA, BIAS_QUANTA + 1, (Cout,), generator=_gen(seed)).to(F32)
    b[Cout // 2] = 0.0
    return b * 2.0 ** unit_exp


# ---- images -------------------------------------------------------------------------------------------------------------------

def _signed(mag, g):
    return mag * (torch.randint(0, 2, mag.shape, generator=g) * 2 - 1)


def _ramp_exps(C, H, W, span):
    """e[c, h, w] in [0, span]: about a third of the span along H, a third along W, the rest by channel."""
    sc = min(2, span // 3) if C > 1 else 0
    sh = (span - sc) // 2
    sw = span - sc - sh
    eh = (torch.arange(H) * sh) // max(H - 1, 1)
    ew = (torch.arange(W) * sw) // max(W - 1, 1)
    ec = (torch.arange(C) + 1) % (sc + 1)                       # 1, 2, 0, 1, ... : a small channel next to a large one
    return ec.view(C, 1, 1) + eh.view(1, H, 1) + ew.view(1, 1, W)


def image_ints(design: str, shape, split: str, level: int, seed: int, m_bits: int = M_BITS) -> torch.Tensor:
    """The integers m (int64 [N, C, H, W]) of ``design`` at fitting level ``level``: dense -> b = level bits; sparse / ramp -> a
    share 2^-level of the pixels; ``m_bits``: |m| < 2^m_bits (the XNOR cases, whose weights take some of the 24 bits).  The zeros of
    every design are planted by ``image``."""
    N, C, H, W = (int(v) for v in shape)
    g = _gen(seed)
    if design == "dense":
        b = int(level)
        return _signed(torch.randint(1 << (b - 1), 1 << b, (N, C, H, W), generator=g) if b > 1 else torch.ones((N, C, H, W), dtype=torch.int64), g)
    keep = torch.rand((N, C, H, W), generator=g) < 2.0 ** -level
    if design == "sparse":
        m = torch.randint(1 << (m_bits - 1), 1 << m_bits, (N, C, H, W), generator=g)
    else:
        assert design == "ramp", design
        rb = NEED_BITS[split] + 2
        r = torch.randint(1 << (rb - 1), 1 << rb, (N, C, H, W), generator=g) | 1
        m = r << _ramp_exps(C, H, W, m_bits - rb).unsqueeze(0)
    return _signed(m, g) * keep


def plant_zeros(x: torch.Tensor) -> torch.Tensor:
    """+0 and -0 pixels, the all-zero last image of a batch (with one -0), the zero rows from 31 on in the image before it."""
    N, C, H, W = (int(v) for v in x.shape)
    flat = x.view(N, C, H * W)
    if H * W >= 3:
        flat[0, :, 1] = 0.0
        flat[0, 0, 2] = -0.0
        if C > 1:
            flat[0, 1:, 2] = 0.0
    if N >= 2:
        x[N - 1] = 0.0
        x[N - 1].view(-1)[-1] = -0.0
    if N >= 3 and H > 31:
        x[N - 2, :, 31:, :] = 0.0
    if N >= 3 and H * W < 3:
        x[N - 2] = 0.0                                              # (a map too small for zero pixels beside non-zero ones)
    return x


def image(design: str, shape, split: str, level: int, q: int, seed: int, m_bits: int = M_BITS) -> torch.Tensor:
    return plant_zeros(image_ints(design, shape, split, level, seed, m_bits).to(F32) * 2.0 ** q)


def assert_image(x: torch.Tensor, q: int, m_bits: int = M_BITS) -> None:
    """x = m 2^q with integer |m| < 2^21, and the pair split reproduces every element under EVERY admissible scale: 2^k with the
    element's own |x| / 2^k below 2^15 (it is no larger than the maximum the scale was chosen for) and the tensor's at or above
    2^14 (no region has a larger maximum); the bf16 triple has no scale."""
    m = x.to(F64) / 2.0 ** q
    assert torch.equal(m, m.round()) and float(m.abs().max()) < 2.0 ** min(m_bits, M_BITS), "image is not m 2^q with |m| < 2^21"
    a = x.abs()
    if float(a.max()) == 0.0:
        return
    _, e = torch.frexp(a.to(F64))
    k_own = (e - 15).to(torch.int64)                             # |x| / 2^k_own in [2^14, 2^15)
    k_top = int(k_own[a > 0].max())
    for k in range(int(k_own[a > 0].min()), k_top + 1):
        sel = (a > 0) & (k_own <= k)
        y = x[sel].to(F64) / 2.0 ** k
        hi = y.to(F32).to(torch.float16).to(F64)
        lo = (y - hi).to(F32).to(torch.float16).to(F64)
        assert torch.equal(hi + lo, y), f"pair split with scale 2^{k} loses bits"
    _, ok = G.split_terms(x, "bf16x3")
    assert ok, "bf16 triple loses bits"


def coverage(x: torch.Tensor, split: str) -> float:
    """Share of the non-zero elements whose LAST term under ``split`` is non-zero."""
    terms, ok = G.split_terms(x, split)
    assert ok
    nz = x != 0
    return float((terms[-1][nz] != 0).double().mean()) if bool(nz.any()) else 0.0


# ---- reference and proof --------------------------------------------------------------------------------------------------------

def conv_ref64(x, wq, bias, stride=1, padding=0, dilation=1):
    """(conv2d(x, wq), conv2d(x, wq) + bias) in float64, [N, Cout, Ho, Wo] each (tests/_exact.py conv64: unfold + matmul)."""
    acc = X.conv64(x, wq, _pair(stride), _pair(padding), _pair(dilation))
    return acc, (acc if bias is None else acc + bias.to(F64).view(1, -1, 1, 1))


def proves(x, wq, bias, stride, padding, dilation, split: str, split_b=None):
    """tests/_grad_exact.py ``proves_exact`` for the conv, then the same bound with the bias inside it: the sum of the |products|
    plus |bias| stays below 2^24 units, the unit being the smaller of the products' quantum and the bias's.  Returns (ok, reason)."""
    def contract(a, b):
        return X.conv64(a, b, _pair(stride), _pair(padding), _pair(dilation))
    ok, why = G.proves_exact(x, wq, contract, split_a=split, split_b=split_b)
    if not ok or bias is None or not bool((bias != 0).any()) or not bool((x != 0).any()):
        return ok, why
    ta, _ = G.split_terms(x, split)
    tb = [wq.to(F64)] if split_b is None else G.split_terms(wq, split_b)[0]
    unit = min(v for v in (G.quantum_exp(t) for t in ta) if v is not None) + min(v for v in (G.quantum_exp(t) for t in tb) if v is not None)
    unit = min(unit, G.quantum_exp(bias))
    bound = float((contract(sum(t.abs() for t in ta), sum(t.abs() for t in tb)) + bias.to(F64).abs().view(1, -1, 1, 1)).max())
    if unit < -126 or bound >= 2.0 ** (24 + unit):
        return False, f"sum of |terms| + |bias| {bound} >= 2^24 units of 2^{unit}"
    return True, f"bound {bound / 2.0 ** unit:.0f} units < 2^24"


class Case:
    """Operands, reference and proof of one (geometry, kind, split, design): x [N, C, H, W] fp32, the latent weight ``w`` and its
    image ``wq``, ``bias``; acc64 / y64 the float64 conv without / with the bias; ``level`` what the fit arrived at."""

    def __init__(self, geom, kind, split, design, batch, q, split_b=None, x_bits=None, m_bits=M_BITS):
        C, Cout, k, st, pd, dl, H, W = geom
        kh, kw = _pair(k)
        self.geom, self.kind, self.split, self.design, self.batch, self.q, self.split_b = geom, kind, split, design, batch, q, split_b
        tag = (geom, kind, split, design, batch, q)
        xb = x_bits if x_bits is not None else NEED_BITS[split] + 2
        self.m_bits = m_bits
        self.w, self.wq, wexp = weights(kind, (Cout, C, kh, kw), seed_of("w", *tag), xb)
        self.bias = bias_of(Cout, q + wexp, seed_of("b", *tag))
        self.shape = (batch, C, H, W)
        levels = range(m_bits - 1, 0, -1) if design == "dense" else range(0, 16)
        self.ok, self.why, self.level = False, "no level fits", None
        for level in levels:
            x = image(design, self.shape, split, level, q, seed_of("x", *tag), m_bits)
            if int((x != 0).sum()) < min(MIN_NONZERO, C * H * W // 2):
                break                                                # too thin to be a test: the design does not fit this case
            ok, why = proves(x, self.wq, self.bias, st, pd, dl, split, split_b)
            if ok:
                self.ok, self.why, self.level, self.x = ok, why, level, x
                break
        assert self.ok, (tag, self.why)
        assert_image(self.x, q, m_bits)
        self.coverage = coverage(self.x, split)
        self.acc64, self.y64 = conv_ref64(self.x, self.wq, self.bias, st, pd, dl)
        self.y32 = G.to_f32_exact(self.y64, "conv + bias")
        self.Ho, self.Wo = int(self.y64.shape[2]), int(self.y64.shape[3])

    def nonzero_share(self):
        return float((self.x != 0).double().mean())


_CASES = {}


def case(geom, kind, split, design, batch=2, q=QUANTA[0], split_b=None, x_bits=None, m_bits=M_BITS) -> Case:
    """One Case per key, built once and shared (the tests leave it unchanged)."""
    key = (geom, kind, split, design, batch, q, split_b, x_bits, m_bits)
    if key not in _CASES:
        _CASES[key] = Case(geom, kind, split, design, batch, q, split_b, x_bits, m_bits)
    return _CASES[key]


def dense_reaches(K: int, split: str) -> bool:
    """Can a dense image populate the last term at this K?  K elements below 2^b and a bias of 8 units must stay below 2^24, and
    of the elements of b bits about 1 - 2^(NEED_BITS - b) have a non-zero last term: b = NEED_BITS + 2 keeps a margin over the 1/4
    demanded."""
    return K * (1 << (NEED_BITS[split] + 2)) + BIAS_QUANTA < 1 << 24


# ---- threshold sets -------------------------------------------------------------------------------------------------------------

def _tie_values(c: Case, seed: int) -> torch.Tensor:
    """theta[co]: fl32(acc + bias) of one output pixel of channel co whose window holds image content (else any pixel)."""
    t = G.to_f32_exact(c.y64, "conv + bias")
    N, Cout, Ho, Wo = (int(v) for v in t.shape)
    g = _gen(seed)
    th = torch.empty((Cout,), dtype=F32)
    for co in range(Cout):
        cand = (c.acc64[:, co] != 0).reshape(-1).nonzero().reshape(-1)
        flat = t[:, co].reshape(-1)
        pick = cand[int(torch.randint(0, int(cand.numel()), (1,), generator=g))] if cand.numel() else 0
        th[co] = flat[pick]
    return th


def affine_set(c: Case, seed: int):
    """(alpha, beta) of a threshold epilogue: alpha = +-2^j (and 0.3: a slope that rounds), beta = -fl(theta alpha) with theta the
    exact value of one output pixel of the channel, so that fl(fl(acc + bias) alpha) + beta = 0 EXACTLY there (a tie: bit 0) and the
    threshold sits inside the populated range; channels 0..7: alpha = 0 (beta 0.5, -1), -0, NaN, beta = +-inf, alpha = -1 / beta = -1,
    alpha = 0.3."""
    Cout = int(c.wq.shape[0])
    g = _gen(seed)
    th = _tie_values(c, seed + 1)
    alpha = torch.exp2(torch.randint(-3, 4, (Cout,), generator=g).to(F32)) * (torch.randint(0, 2, (Cout,), generator=g) * 2 - 1).to(F32)
    alpha[7::8] = 0.3
    beta = -torch.mul(th, alpha)
    alpha[0], beta[0] = 0.0, 0.5
    alpha[1], beta[1] = 0.0, -1.0
    alpha[2], beta[2] = -0.0, 1.0
    alpha[3] = float("nan")
    beta[4], beta[5] = float("inf"), float("-inf")
    alpha[6], beta[6] = -1.0, -1.0
    return alpha, beta


BN_EPS = 1e-5


def bn_set(c: Case, seed: int):
    """(running_mean, running_var, weight, bias) of an eval-mode BatchNorm2d whose fold (``fold_bn``) puts a tie on one output pixel
    of every channel: mean = theta, bias = 0 -> beta = -fl(theta alpha); channels 0..6 as in ``affine_set`` (weight 0 / -0 / NaN,
    bias +-inf and -1)."""
    Cout = int(c.wq.shape[0])
    g = _gen(seed)
    mean = _tie_values(c, seed + 1)
    var = torch.ones((Cout,), dtype=F32)
    var[1::2] = 3.0
    weight = torch.exp2(torch.randint(-2, 3, (Cout,), generator=g).to(F32)) * (torch.randint(0, 2, (Cout,), generator=g) * 2 - 1).to(F32)
    bias = torch.zeros((Cout,), dtype=F32)
    weight[0], bias[0] = 0.0, 0.5
    weight[1], bias[1] = 0.0, -1.0
    weight[2], bias[2] = -0.0, 1.0
    weight[3] = float("nan")
    bias[4], bias[5] = float("inf"), float("-inf")
    weight[6], bias[6] = -1.0, -1.0
    return mean, var, weight, bias


def fold_bn(mean, var, weight, bias, eps: float = BN_EPS):
    """(alpha, beta) of eval-mode BatchNorm, the fp32 operations of layers/fused.py fold_batchnorm restated."""
    invstd = 1.0 / torch.sqrt(var.to(F32) + eps)
    alpha = invstd * weight.to(F32)
    return alpha, bias.to(F32) - mean.to(F32) * alpha


def want_bits(c: Case, alpha, beta, pool: bool = False):
    """bool [N, Ho, Wo, Cout] (True = the bit is set) of _exact.predicate on the exact sum; ``pool``: the 2 x 2 / stride 2 max-pool
    between conv and BatchNorm: the AND of the window's bits (alpha < 0: the OR) — the pooled activation's own predicate, since
    x -> fl(fl(x alpha) + beta) is monotone.  Also the folded values v."""
    bits, v = X.predicate(c.acc64, c.bias, alpha, beta)
    bits, v = bits.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1)
    if not pool:
        return bits, v
    N, Ho, Wo, Cout = (int(t) for t in bits.shape)
    win = bits[:, :Ho // 2 * 2, :Wo // 2 * 2].reshape(N, Ho // 2, 2, Wo // 2, 2, Cout)
    return torch.where(alpha.view(1, 1, 1, -1) < 0, win.any(4).any(2), win.all(4).all(2)), None


# ---- the emulated route (CPU): split, then fp32 accumulation of the terms in a shuffled order ------------------------------------

MUTATIONS = ("drop_last", "scale_lo", "shift_tap")


def emulate(c: Case, seed: int, mutate=None) -> torch.Tensor:
    """fp32 [N, Cout, Ho, Wo]: the image split as the route splits it, every (term, k) product accumulated in fp32 in an order
    shuffled by ``seed``, the bias last.  ``mutate``: "drop_last" = without the last term; "scale_lo" = the last term doubled;
    "shift_tap" = one (term 0) tap reads its neighbour pixel's column.  Mutations of this emulation only."""
    C, Cout, k, st, pd, dl, H, W = c.geom
    kh, kw = _pair(k)
    terms, ok = G.split_terms(c.x, c.split)
    assert ok
    terms = [t.to(F32) for t in terms]
    if mutate == "drop_last":
        terms = terms[:-1]
    elif mutate == "scale_lo":
        terms[-1] = terms[-1] * 2.0
    cols = torch.cat([F.unfold(t, (kh, kw), dilation=_pair(dl), padding=_pair(pd), stride=_pair(st)) for t in terms], 1)   # [N, T K, L]
    w2 = c.wq.reshape(Cout, -1).repeat(1, len(terms))
    if mutate == "shift_tap":
        k0 = int((cols[:, :C * kh * kw] != 0).sum((0, 2)).argmax())
        cols[:, k0] = torch.roll(cols[:, k0], 1, -1)
    order = torch.randperm(int(cols.shape[1]), generator=_gen(seed)).tolist()
    acc = torch.zeros((c.batch, Cout, int(cols.shape[2])), dtype=F32)
    for kk in order:
        acc = torch.add(acc, torch.mul(w2[:, kk].view(1, Cout, 1), cols[:, kk].unsqueeze(1)))
    acc = torch.add(acc, c.bias.view(1, Cout, 1))
    return acc.view(c.batch, Cout, c.Ho, c.Wo)


def emulated_bits(y32: torch.Tensor, alpha, beta) -> torch.Tensor:
    """The threshold bits of an emulated fp32 result y (bias included): fl(fl(y alpha) + beta) < 0, [N, Ho, Wo, Cout]."""
    return X.predicate(y32, None, alpha, beta)[0].permute(0, 2, 3, 1)


# ---- float_linear ---------------------------------------------------------------------------------------------------------------

class LinearCase:
    """ops.float_linear: x [M, K] ("dense": one amplitude, the largest the proof accepts; "ramp": row r scaled by 2^(r mod span),
    thinned until the proof holds), the latent weight [N, K] -> +-1, a bias or None."""

    def __init__(self, M, N, K, split, design, with_bias, q=QUANTA[0]):
        tag = ("lin", M, N, K, split, design, with_bias)
        g = _gen(seed_of(*tag))
        self.split, self.design = split, design
        self.wq = torch.randint(0, 2, (N, K), generator=g).to(F32) * 2 - 1
        self.w = self.wq * 0.75
        self.bias = bias_of(N, q, seed_of("b", *tag)) if with_bias else None
        babs = 0.0 if self.bias is None else self.bias.to(F64).abs().view(1, -1)
        rb = NEED_BITS[split] + 2
        self.ok, self.why = False, "no level fits"
        for level in (range(M_BITS - 1, 0, -1) if design == "dense" else range(0, 16)):
            gx = _gen(seed_of("x", *tag))
            if design == "dense":
                m = _signed(torch.randint(1 << (level - 1), 1 << level, (M, K), generator=gx) if level > 1 else torch.ones((M, K), dtype=torch.int64), gx)
            else:
                r = torch.randint(1 << (rb - 1), 1 << rb, (M, K), generator=gx) | 1
                span = M_BITS - rb
                e = (torch.arange(M).view(M, 1) % (span + 1)).expand(M, K)
                m = _signed(r << e, gx) * (torch.rand((M, K), generator=gx) < 2.0 ** -level)
            x = m.to(F32) * 2.0 ** q
            x[0, 0], x[M - 1, K - 1] = 0.0, -0.0
            ok, why = G.proves_exact(x, self.wq, lambda a, b: a @ b.t() + babs, split_a=split)
            if ok:
                self.ok, self.why, self.x = ok, why, x
                break
        assert self.ok, (tag, self.why)
        assert_image(self.x, q)
        self.coverage = coverage(self.x, split)
        y64 = self.x.to(F64) @ self.wq.to(F64).t()
        self.y32 = G.to_f32_exact(y64 if self.bias is None else y64 + self.bias.to(F64), "x . w^T + bias")


_LINEAR = {}


def linear_case(*key) -> LinearCase:
    if key not in _LINEAR:
        _LINEAR[key] = LinearCase(*key)
    return _LINEAR[key]


LINEAR_SHAPES = ((5, 7, 31), (130, 70, 363), (257, 129, 1000))


def linear_cases():
    return [(M, N, K, split, design, wb) for (M, N, K) in LINEAR_SHAPES for split in ("f16x2", "bf16x3")
            for design in ("dense", "ramp") for wb in (False, True)]


# ---- the cases of tests/test_gpu_first_layer_exact.py (tests/test_first_exact_cpu.py proves every one) ---------------------------
# geometry: (C, Cout, k, stride, padding, dilation, H, W), k / stride / padding / dilation an int or an (h, w) pair

def K_of(geom) -> int:
    kh, kw = _pair(geom[2])
    return geom[0] * kh * kw


def designs_for(geom, split) -> tuple:
    return tuple(d for d in DESIGNS if d != "dense" or dense_reaches(K_of(geom), split))


FORWARD_RUNGS = ("first3x3", "first_direct", "s2d", "plain")          # what quant_conv2d_forward allows
BLOCK_RUNGS = ("first3x3", "direct3x3", "d2s")                         # what FusedConvPoolBnSign tries before it
NO_DIRECT_BLOCK = {"FIRST_3X3": False, "DIRECT_FIRST_LAYER": False}
NO_FIRST_DIRECT = {"FIRST_DIRECT": False}

#: rung -> the output forms it can deliver ("pool" = the block's pooled bits, made from the rung's un-pooled bits)
FORMS = {
    "first3x3": ("f32", "bits", "nib11", "nib22", "pool"),
    "direct3x3": ("bits", "nib11", "pool"),                            # planes only; the halo-1 nibble plane only
    "d2s": ("nib11", "nib22"),                                          # depth-to-space happens in the nibble epilogue
    "first_direct": ("f32", "bits", "nib11", "nib22", "pool"),
    "s2d": ("f32", "bits", "nib11", "nib22", "pool"),
    "plain": ("f32", "bits", "nib11", "nib22", "pool"),
    "first_direct_real": ("f32", "bits", "nib11", "nib22", "pool"),
    "bf16x6": ("f32", "bits", "nib11", "nib22", "pool"),
}
#: rung -> the splits of the image it exists under.  first3x3 is a pair kernel and stands aside under "bf16x3"; direct3x3 runs pairs
#: for <= 4 channels under "f16x2", triples otherwise; first_direct splits its patch into pairs whatever the switch says (it is run
#: under both settings, the proof is the pair split's); the XNOR rungs do not read the switch: pairs x pairs, triples x triples.
SPLITS = {
    "first3x3": ("f16x2",), "direct3x3": ("f16x2", "bf16x3"), "d2s": ("f16x2", "bf16x3"), "first_direct": ("f16x2", "bf16x3"),
    "s2d": ("f16x2", "bf16x3"), "plain": ("f16x2", "bf16x3"), "first_direct_real": ("f16x2",), "bf16x6": ("bf16x3",),
}


def table():
    """Every (rung, form, split) the closing test demands."""
    return [(r, f, s) for r in FORMS for f in FORMS[r] for s in SPLITS[r]]


class Group:
    """One operand set and the forms compared on it.  ``switch``: the FLOAT_SPLIT the rung runs under (None: the default "f16x2");
    ``split``: the split the rung then uses = the proof's; ``entry`` "forward" / "block" / "function" as in
    tests/test_gpu_first_layer_routes.py; ``storage`` "cl" / "nchw" / "view"."""

    def __init__(self, rung, entry, kind, geom, batch, forms, switch=None, split=None, designs=None, sw=None, storage="cl",
                 q=QUANTA[0], split_b=None, x_bits=None, m_bits=M_BITS, table_split=None):
        self.rung, self.entry, self.kind, self.geom, self.batch, self.forms = rung, entry, kind, geom, batch, tuple(forms)
        self.switch, self.split = switch, split or switch or "f16x2"
        self.table_split = table_split or self.split               # the row of ``table`` the group fills
        self.designs = tuple(designs) if designs is not None else designs_for(geom, self.split)
        self.sw, self.storage, self.q, self.split_b, self.x_bits, self.m_bits = dict(sw or {}), storage, q, split_b, x_bits, m_bits
        g = "x".join(str(v).replace(" ", "") for v in geom)
        self.id = "-".join(str(v) for v in (rung, entry, kind, g, f"n{batch}", self.switch or "default", storage, f"q{q}"))

    def case(self, design) -> Case:
        return case(self.geom, self.kind, self.split, design, self.batch, self.q, self.split_b, self.x_bits, self.m_bits)


def _groups():
    out = []

    def add(*a, **kw):
        out.append(Group(*a, **kw))

    FWD, BLK = ("f32", "bits", "nib11", "nib22"), ("bits", "nib11", "nib22", "pool")
    # ---- first3x3: 32 x 32 output tiles, a wave walks 8 rows: 33 x 35 crosses the tile edge in H and in W, batch 3 holds the zero tile
    big3 = (3, 64, 3, 1, 1, 1, 33, 35)
    add("first3x3", "forward", "ternary", big3, 3, FWD)
    add("first3x3", "block", "binary", big3, 3, BLK, q=QUANTA[1])
    add("first3x3", "forward", "binary", (1, 64, 3, 1, 1, 1, 1, 1), 3, FWD)
    add("first3x3", "block", "ternary", (2, 64, 3, 1, 1, 1, 2, 3), 1, BLK)
    add("first3x3", "forward", "binary", (4, 64, 3, 1, 1, 1, 9, 34), 2, FWD)
    for storage in ("nchw", "view"):
        add("first3x3", "forward", "ternary", (3, 64, 3, 1, 1, 1, 5, 7), 2, ("f32", "bits", "nib11"), storage=storage)
    # ---- direct3x3 (the block's rung; first3x3 wants 64 output channels, these have 32): 32-byte triple pixels, i.e. 3 .. 5 channels
    D = ("bits", "nib11", "pool")
    for switch in (None, "bf16x3"):
        add("direct3x3", "block", "binary", (3, 32, 3, 1, 1, 1, 6, 6), 2, D, switch=switch)
        add("direct3x3", "block", "ternary", (4, 32, 3, 1, 1, 1, 33, 35), 3, D, switch=switch)
    add("direct3x3", "block", "ternary", (5, 32, 3, 1, 1, 1, 6, 6), 2, D, split="bf16x3")            # five channels: triples
    add("direct3x3", "block", "binary", (3, 32, 3, 1, 1, 1, 2, 3), 1, ("bits", "nib11"))
    add("direct3x3", "block", "binary", (3, 32, 3, 1, 1, 1, 7, 5), 2, D, storage="view")
    add("direct3x3", "block", "ternary", (4, 32, 3, 1, 1, 1, 1, 1), 2, ("bits", "nib11"), storage="nchw")
    # ---- d2s (2 x 2 output blocks: even maps), the direct kernels switched off
    for switch in (None, "bf16x3"):
        add("d2s", "block", "binary", (3, 32, 3, 1, 1, 1, 6, 6), 2, ("nib11", "nib22"), switch=switch, sw=NO_DIRECT_BLOCK)
        add("d2s", "block", "ternary", (6, 32, 3, 1, 1, 1, 34, 32), 3, ("nib11", "nib22"), switch=switch, sw=NO_DIRECT_BLOCK)
    add("d2s", "block", "ternary", (6, 32, 3, 1, 1, 1, 2, 2), 1, ("nib11",), sw=NO_DIRECT_BLOCK, storage="nchw")
    add("d2s", "block", "binary", (3, 64, 3, 1, 1, 1, 4, 6), 2, ("nib11",), sw=NO_DIRECT_BLOCK, storage="view")
    # ---- first_direct: output tiles of <= 128 pixels (18 x 17 outputs: several), (H + 2p - k) % s != 0 in H only / W only / both / neither
    alex = lambda H, W: (3, 24, 11, 4, 2, 1, H, W)
    add("first_direct", "forward", "binary", alex(33, 35), 2, FWD)
    add("first_direct", "forward", "binary", alex(33, 35), 2, FWD, switch="bf16x3", split="f16x2", table_split="bf16x3")
    add("first_direct", "block", "ternary", (4, 24, 4, 2, 1, 1, 10, 10), 2, ("pool",), switch="bf16x3", split="f16x2", table_split="bf16x3")
    add("first_direct", "block", "binary", alex(35, 33), 2, ("bits", "nib22", "pool"))
    add("first_direct", "forward", "ternary", alex(33, 33), 1, ("f32", "bits"), storage="nchw")
    add("first_direct", "forward", "ternary", alex(35, 35), 2, ("f32", "bits"), storage="view", q=QUANTA[1])
    add("first_direct", "forward", "ternary", (4, 24, 4, 2, 1, 1, 10, 10), 2, FWD)
    add("first_direct", "forward", "binary", (2, 24, 2, 2, 0, 1, 9, 8), 2, ("f32", "bits"))                     # k == stride
    add("first_direct", "forward", "ternary", (1, 24, 3, 3, 1, 1, 10, 11), 2, ("f32", "bits", "nib11"))         # stride 3
    add("first_direct", "forward", "binary", (3, 40, 3, 2, 1, 1, 35, 33), 3, ("f32", "bits"))                  # 306 output pixels
    add("first_direct", "block", "ternary", (3, 40, 3, 2, 1, 1, 35, 33), 3, ("bits", "pool"), storage="nchw")
    add("first_direct", "forward", "binary", (3, 200, 4, 2, 1, 1, 10, 9), 2, ("f32", "bits"))                   # more channels than one workgroup's 192
    add("first_direct", "forward", "binary", (3, 24, 3, 2, 1, 1, 1, 1), 2, ("f32", "bits"))
    add("first_direct", "forward", "ternary", (3, 24, 3, 2, 1, 1, 2, 3), 1, ("f32", "bits"))
    # ---- s2d: the rounding to the stride adds a row only (33 x 35), a column only, both, neither; the stride-1 padded form
    for switch in (None, "bf16x3"):
        add("s2d", "forward", "binary", alex(33, 35), 2, FWD, switch=switch, sw=NO_FIRST_DIRECT)
        add("s2d", "forward", "ternary", (3, 24, 5, 1, 2, 1, 9, 6), 2, FWD, switch=switch)
        add("s2d", "forward", "binary", (3, 24, 3, 1, 1, 1, 6, 7), 2, ("f32", "bits"), switch=switch)       # K = 27: dense reaches the third term
        add("s2d", "block", "binary", alex(35, 33), 2, ("bits", "nib11", "pool"), switch=switch, sw=NO_FIRST_DIRECT)
    add("s2d", "forward", "ternary", alex(33, 33), 1, ("f32", "bits"), sw=NO_FIRST_DIRECT, storage="nchw")
    add("s2d", "forward", "ternary", alex(35, 35), 2, ("f32", "bits"), sw=NO_FIRST_DIRECT, q=QUANTA[1])
    add("s2d", "forward", "binary", alex(33, 35), 2, ("f32", "bits"), sw=NO_FIRST_DIRECT, storage="view", q=QUANTA[1])
    add("s2d", "forward", "binary", (4, 24, 4, 4, 0, 1, 9, 9), 2, ("f32", "bits"), sw=NO_FIRST_DIRECT)          # C s s = 64
    add("s2d", "forward", "ternary", (17, 24, 3, 1, 1, 1, 6, 5), 2, ("f32", "bits", "nib11"), switch="bf16x3")
    add("s2d", "forward", "binary", (6, 24, 3, 1, 1, 1, 1, 1), 2, ("f32", "bits"))
    add("s2d", "forward", "binary", (6, 24, 3, 1, 1, 1, 2, 3), 1, ("f32", "bits"), storage="nchw")
    # ---- plain: no padding, dilation, a non-square kernel / stride / padding
    for switch in (None, "bf16x3"):
        add("plain", "forward", "binary", (3, 24, 3, 1, 0, 1, 6, 7), 2, FWD, switch=switch)
        add("plain", "forward", "ternary", (3, 24, 3, 1, 0, 2, 7, 8), 2, ("f32", "bits"), switch=switch)
        add("plain", "forward", "ternary", (3, 24, (3, 5), (1, 2), (1, 0), 1, 9, 11), 2, ("f32", "bits"), switch=switch)
    add("plain", "block", "ternary", (3, 24, 3, 1, 1, 2, 6, 7), 2, ("bits", "nib11", "pool"))
    add("plain", "block", "binary", (3, 24, 3, 1, 0, 1, 35, 33), 3, ("bits", "pool"), switch="bf16x3", storage="nchw")
    add("plain", "forward", "binary", (3, 24, 3, 1, 0, 1, 3, 3), 1, ("f32", "bits"))                             # a 1 x 1 map
    add("plain", "forward", "ternary", (3, 24, (2, 3), 1, 0, 1, 3, 5), 2, ("f32", "bits"), storage="view")      # a 2 x 3 map
    # ---- XNOR: the weight image sign(W) alpha with power-of-two alphas per tap
    XF, XB = ("f32",), ("bits", "nib11", "nib22", "pool")
    real = dict(split="f16x2", split_b="f16x2", x_bits=18, m_bits=18)
    add("first_direct_real", "function", "xnor", alex(33, 35), 2, XF, **real)
    add("first_direct_real", "block", "xnor", alex(35, 33), 2, XB, **real)
    add("first_direct_real", "function", "xnor", (4, 24, 4, 2, 1, 1, 10, 10), 1, XF, storage="nchw", **real)
    add("first_direct_real", "block", "xnor", (3, 40, 3, 2, 1, 1, 35, 33), 3, ("bits", "pool"), storage="view", **real)
    six = dict(split="bf16x3", split_b="bf16x3", x_bits=19, m_bits=20)
    add("bf16x6", "function", "xnor", (3, 24, 3, 1, 1, 1, 6, 7), 2, XF, **six)
    add("bf16x6", "block", "xnor", (3, 24, 3, 1, 1, 1, 6, 7), 2, XB, **six)
    add("bf16x6", "function", "xnor", (3, 24, 5, 1, 2, 1, 9, 6), 1, XF, storage="nchw", **six)
    add("bf16x6", "block", "xnor", (2, 24, 3, 1, 1, 2, 33, 35), 3, ("bits", "pool"), storage="view", **six)
    return out


GROUPS = _groups()
