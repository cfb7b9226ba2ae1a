"""Depthwise and grouped streaming convs on bf16 / fp16 operands on the GPU: the six "_h" entries of csrc/dwconv.hip and
csrc/gconv.hip through ops.depthwise_conv2d* / ops.grouped_conv2d*, and BinConv2d / TerConv2d on the half routes of
functions/_fused.py (``depthwise_half_route`` / ``grouped_half_route``).

The contract (include/qt_hip.h "Depthwise and grouped convolution on half-precision operands"): every element is upcast exactly,
the arithmetic is that of the "_f32" entry, the fp32 result is rounded once to nearest even.  So

* forward and grad_input equal, BIT FOR BIT, RNE(float32 restatement of tests/_dw_exact.py / tests/_gconv_exact.py on the upcast
  operands), the rounding being the numpy one of tests/_half_round.py (pinned on the CPU by tests/test_half_streaming_cpu.py);
* grad_weight equals RNE("_f32" entry on the upcast operands) bit for bit, equals itself when run twice, and lies within
  ``grad_weight_bound`` of the float64 sum plus ONE rounding of the output type (half an ulp, taken at |float64 sum| + bound: the
  largest magnitude the fp32 value can have).

Bits are compared as 16-bit patterns with NaN as a class; no element is waived.  Every result is written into a view inside a
sentinel-filled buffer at an ODD element offset (2-byte, not 4-byte aligned).  All shapes are small."""
import copy

import numpy as np
import pytest
import torch

import _dw_exact as D
import _gconv_exact as G
import _half_round as HR
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, DorefaConv2d
from pytorch_quantize_impls_amd.utils.graphs import _no_collection_inside

pytestmark = pytest.mark.gpu

FMTS = {"bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = 0x5A5A
PAD = 67                      # odd: the guarded view starts 134 bytes into its buffer
DW_CASES, GC_CASES = D.cases(), G.cases()
STATS = dict(compared=0, differing=0, cases=0)       # what the module reports at its end: elements compared / found different


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    yield torch.device("cuda:0")
    print(f"\n[half streaming] cases {STATS['cases']}, elements compared {STATS['compared']}, differing bit patterns "
          f"{STATS['differing']}, waived 0, peak device memory {torch.cuda.max_memory_allocated() / 2 ** 20:.1f} MiB")


# ---- helpers -----------------------------------------------------------------------------------------------------------------------

def half_of(a32, fmt):
    """(bits, exact float32 upcast) of a float32 array rounded to ``fmt``."""
    bits = HR.ROUND[fmt](np.asarray(a32, dtype=np.float32))
    return bits, HR.UPCAST[fmt](bits)


def to_dev(dev, bits, fmt, layout="nchw"):
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(FMTS[fmt]).to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" and t.dim() == 4 else t


def f32_dev(dev, a, layout="nchw"):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" and t.dim() == 4 else t


def bits_of(t):
    t = t.detach().cpu()
    if t.dtype == torch.float32:
        return t.numpy()
    return t.view(torch.int16).numpy().view(np.uint16)


def guarded(dev, shape, layout, dtype):
    """(buffer, view): a dense tensor of ``shape`` in ``layout`` with PAD sentinel elements on either side."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        buf = torch.full((n + 2 * PAD,), 12345.0, dtype=torch.float32, device=dev)
    else:
        buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.int16, device=dev).view(dtype)
    mid = buf[PAD:PAD + n]
    if layout == "channels_last" and len(shape) == 4:
        N, C, H, W = shape
        return buf, mid.view(N, H, W, C).permute(0, 3, 1, 2)
    return buf, mid.view(*shape)


def intact(buf):
    raw = buf if buf.dtype == torch.float32 else buf.view(torch.int16)
    want = 12345.0 if buf.dtype == torch.float32 else SENTINEL
    return bool((raw[:PAD] == want).all() and (raw[-PAD:] == want).all())


def check(got_bits, want32, fmt, what):
    """``got_bits`` (uint16) against RNE(``want32``); counts into STATS."""
    want = HR.ROUND[fmt](want32)
    ok, n = HR.same_bits(got_bits, want, fmt)
    STATS["compared"] += int(want.size)
    STATS["differing"] += n
    assert ok, (what, fmt, n, int(want.size))
    return want


def quiet(fn, *a, **k):
    with np.errstate(all="ignore"):
        return fn(*a, **k)


def edge_weights(seed, shape, fmt):
    """Weights ON the ternary thresholds and the STE bound, and their neighbours in ``fmt`` (as exact float32 values)."""
    f = HR.FORMATS[fmt]
    pats = []
    for base in (f["half"], f["one"]):
        pats += [base - 1, base, base + 1]
    pats = np.array(pats + [p | 0x8000 for p in pats] + [0x0000, 0x8000, 0x0001, 0x8001], dtype=np.uint16)
    bits = pats[D._rng(seed).randint(0, len(pats), size=shape)]
    return bits, HR.UPCAST[fmt](bits)


def special_values(seed, shape, fmt, base32):
    """``base32`` rounded to ``fmt`` with NaN, +-inf and -0.0 sprinkled over about an eighth of it."""
    bits, _ = half_of(base32, fmt)
    r = D._rng(seed)
    inf = HR.FORMATS[fmt]["inf"]
    sp = np.array([inf | 1, 0x8000 | inf | 0x21, inf, 0x8000 | inf, 0x8000, 0x7FFF], dtype=np.uint16)
    hit = r.rand(*shape) < 0.125
    bits = np.where(hit, sp[r.randint(0, len(sp), size=shape)], bits).astype(np.uint16)
    return bits, HR.UPCAST[fmt](bits)


def operands(cls, seed, xs, ws, ys, fmt):
    """(x, w, go) as (bits, float32) pairs of data class ``cls``."""
    if cls == "ints":
        x, w, go = D.pm1(seed, xs), D.small_ints(seed + 1, ws), D.small_ints(seed + 2, ys)
    elif cls == "gauss":
        x, w, go = D.gauss6(seed, xs), D.weights(seed + 1, ws), D.gauss6(seed + 2, ys)
    elif cls == "edges":
        return half_of(D.gauss6(seed, xs) / 64, fmt), edge_weights(seed + 1, ws, fmt), half_of(D.small_ints(seed + 2, ys), fmt)
    else:
        return (special_values(seed, xs, fmt, D.pm1(seed, xs)), special_values(seed + 1, ws, fmt, D.weights(seed + 1, ws)),
                special_values(seed + 2, ys, fmt, D.small_ints(seed + 2, ys)))
    return half_of(x, fmt), half_of(w, fmt), half_of(go, fmt)


CLASSES = ("ints", "gauss", "edges", "special")


class Dw:
    """The depthwise family: shapes of a case, reference and ops calls."""
    cases = DW_CASES

    @staticmethod
    def shapes(c):
        Ho, Wo = D.out_hw(c.H, c.W, c.kernel, c.stride, c.padding, c.dilation)
        return (c.N, c.C, c.H, c.W), (c.C * c.m, 1) + tuple(c.kernel), (c.N, c.C * c.m, Ho, Wo)

    @staticmethod
    def layouts(c):
        return c.layout, c.layout

    @staticmethod
    def fwd_ref(c, x, wq, b):
        return quiet(D.forward, x, wq.reshape(wq.shape[0], *c.kernel), b, c.kernel, c.stride, c.padding, c.dilation)

    @staticmethod
    def gin_ref(c, go, wq, xs):
        return quiet(D.grad_input, go, wq.reshape(wq.shape[0], *c.kernel), xs, c.kernel, c.stride, c.padding, c.dilation)

    @staticmethod
    def gw_ref(c, x, go):
        gw, ab, gb = D.grad_weight(x, go, c.kernel, c.stride, c.padding, c.dilation)
        return gw[:, None], ab[:, None], gb

    @staticmethod
    def fwd(c, x, w, b, kind, out):
        return ops.depthwise_conv2d(x, w, b, c.stride, c.padding, c.dilation, kind=kind, out=out)

    @staticmethod
    def gin(c, xs, w, go, kind, out):
        return ops.depthwise_conv2d_grad_input(xs, w, go, c.stride, c.padding, c.dilation, kind=kind, out=out)

    @staticmethod
    def work(c, xs, ws):
        return ops.depthwise_grad_weight_work_floats(xs, ws, c.stride, c.padding, c.dilation)

    @staticmethod
    def gwt(c, x, go, w, thr, **kw):
        return ops.depthwise_conv2d_grad_weight(x, go, w, c.stride, c.padding, c.dilation, ste_threshold=thr, **kw)


class Gc:
    """The grouped family."""
    cases = GC_CASES

    @staticmethod
    def shapes(c):
        return c.shapes

    @staticmethod
    def layouts(c):
        return c.layout

    @staticmethod
    def fwd_ref(c, x, wq, b):
        return quiet(G.forward, x, wq, b, c.G, *c.geom)

    @staticmethod
    def gin_ref(c, go, wq, xs):
        return quiet(G.grad_input, go, wq, xs, c.G, *c.geom)

    @staticmethod
    def gw_ref(c, x, go):
        return G.grad_weight(x, go, c.G, c.cin_g, *c.geom)

    @staticmethod
    def fwd(c, x, w, b, kind, out):
        return ops.grouped_conv2d(x, w, b, c.stride, c.padding, c.dilation, c.G, kind=kind, out=out)

    @staticmethod
    def gin(c, xs, w, go, kind, out):
        return ops.grouped_conv2d_grad_input(xs, w, go, c.stride, c.padding, c.dilation, c.G, kind=kind, out=out)

    @staticmethod
    def work(c, xs, ws):
        return ops.grouped_grad_weight_work_floats(xs, ws, c.stride, c.padding, c.dilation, c.G)

    @staticmethod
    def gwt(c, x, go, w, thr, **kw):
        return ops.grouped_conv2d_grad_weight(x, go, w, c.stride, c.padding, c.dilation, c.G, ste_threshold=thr, **kw)


FAMS = {"dw": Dw, "gc": Gc}
ALL = [("dw", i) for i in range(len(DW_CASES))] + [("gc", i) for i in range(len(GC_CASES))]
IDS = [f"{f}-{FAMS[f].cases[i].id}" for f, i in ALL]


# ---- 1. the entries: forward and grad_input ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam,i", ALL, ids=IDS)
def test_forward_and_grad_input_are_rne_of_the_float32_restatement(dev, fam, i):
    """{bf16, fp16} x {raw, binary, ternary} per geometry case; the operand class and the weight dtype (the activation's, or fp32 as
    under autocast) rotate with the case, so every (class, kind, dtype, weight dtype) occurs many times over the table."""
    F, c = FAMS[fam], FAMS[fam].cases[i]
    xs, ws, ys = F.shapes(c)
    lx, ly = F.layouts(c)
    STATS["cases"] += 1
    for fi, fmt in enumerate(FMTS):
        for ki, kind in enumerate(D.KINDS):
            cls = CLASSES[(i + 2 * fi + ki) % 4]
            (xb, x32), (wb, w32), (gb_, g32) = operands(cls, 1000 * i + 10 * ki + fi, xs, ws, ys, fmt)
            w_f32 = (i + ki + fi) % 3 == 0
            wd = f32_dev(dev, w32) if w_f32 else to_dev(dev, wb, fmt)
            b32 = D.gauss6(7 + i, (ws[0],)) if (i + ki) % 2 == 0 else None
            if cls == "ints" and b32 is not None:
                b32 = D.small_ints(7 + i, (ws[0],))
            wq = D.quantize(w32, kind)
            buf, out = guarded(dev, ys, ly, FMTS[fmt])
            y = F.fwd(c, to_dev(dev, xb, fmt, lx), wd, None if b32 is None else f32_dev(dev, b32), kind, out)
            assert y is out and y.dtype == FMTS[fmt] and intact(buf)
            check(bits_of(y), F.fwd_ref(c, x32, wq, b32), fmt, ("forward", cls, kind, w_f32))
            buf, out = guarded(dev, xs, lx, FMTS[fmt])
            gx = F.gin(c, xs, wd, to_dev(dev, gb_, fmt, ly), kind, out)
            assert gx is out and intact(buf)
            check(bits_of(gx), F.gin_ref(c, g32, wq, xs), fmt, ("grad_input", cls, kind, w_f32))


# ---- 2. rounding on purpose ----------------------------------------------------------------------------------------------------------

def _grouped_7x7(dev, fmt, x32, w32, b32, kind="raw", cin_g=8):
    """ops.grouped_conv2d of a [1, 4 cin_g, 7, 7] input with a [4, cin_g, 7, 7] kernel and no padding: one output per group, the
    plain sum of cin_g * 49 = 392 products.  Returns (bits [4], float32 reference [4])."""
    xb, x32 = half_of(x32, fmt)
    wb, w32 = half_of(w32, fmt)
    y = ops.grouped_conv2d(to_dev(dev, xb, fmt), to_dev(dev, wb, fmt), None if b32 is None else f32_dev(dev, b32), 1, 0, 1, 4, kind=kind)
    ref = quiet(G.forward, x32, D.quantize(w32, kind), b32, 4, (7, 7), (1, 1), (0, 0), (1, 1))
    return bits_of(y).reshape(-1), ref.reshape(-1)


def _sum_design(total, n=392):
    """+-1 weights for an all-ones input of n terms whose sum is ``total`` (same parity as n)."""
    neg = (n - total) // 2
    assert 0 <= neg <= n and n - 2 * neg == total
    w = np.ones(n, np.float32)
    w[:neg] = -1.0
    return w


def test_exact_ties_of_the_output_type_round_to_even(dev):
    seen = set()
    ones = np.ones((1, 32, 7, 7), np.float32)
    # bf16 has 8 significant bits: odd integers in [257, 391] are exact ties between the even neighbours; 392 terms reach them
    for totals in ((258, 260, 262, 264), (390, 386, 300, 302)):            # sums s with s - 1 odd ... shifted by a bias of -1 below
        w = np.stack([_sum_design(t) for t in totals]).reshape(4, 8, 7, 7)
        bits, ref = _grouped_7x7(dev, "bf16", ones, w, np.full(4, -1.0, np.float32))
        assert all(int(v) % 2 == 1 and 257 <= v <= 391 for v in ref)
        want = check(bits, ref, "bf16", "bf16 ties")
        for v, b in zip(ref, HR.bf16_to_f32(want)):
            seen.add("bf16-up" if b > v else "bf16-down")
            assert abs(b - v) == 1.0
    # fp16 has 11: above 2048 the spacing is 2, odd sums (via a small integer bias) are ties; a raw weight of 6 reaches them
    for bias in (2049.0 - 6 * 340, 2051.0 - 6 * 340, 4098.0 - 6 * 340, 4102.0 - 6 * 340):
        w = np.stack([6.0 * _sum_design(340)] * 4).reshape(4, 8, 7, 7)
        bits, ref = _grouped_7x7(dev, "fp16", ones, w, np.full(4, bias, np.float32))
        want = check(bits, ref, "fp16", "fp16 ties")
        for v, b in zip(ref, HR.fp16_to_f32(want)):
            assert b != v and abs(b - v) in (1.0, 2.0)
            seen.add("fp16-up" if b > v else "fp16-down")
    # fp16 overflow with raw weights: 65519 -> 65504, 65520 -> inf
    w = np.zeros((4, 8, 7, 7), np.float32)
    w[:, 0, 0, 0] = 1.0
    x = np.zeros((1, 32, 7, 7), np.float32)
    x[0, ::8, 0, 0] = 32768.0
    for bias, pattern, tag in ((32751.0, 0x7BFF, "fp16-max"), (32752.0, 0x7C00, "fp16-overflow"), (-98288.0, 0xFC00, "fp16-overflow")):
        bits, ref = _grouped_7x7(dev, "fp16", x, w, np.full(4, bias, np.float32))
        check(bits, ref, "fp16", tag)
        assert (bits == pattern).all() and ref[0] == 32768.0 + bias
        seen.add(tag)
    # an fp16 subnormal result (3 * 2^-25 is a tie: -> 2^-23) and a subnormal input times 0.5 (2^-24 * 0.5 is a tie: -> 0)
    x[0, ::8, 0, 0] = 2.0 ** -24
    for wv, bias, pattern, tag in ((0.5, None, 0x0000, "fp16-subnormal-input"), (0.5, np.float32(2.0 ** -24), 0x0002, "fp16-subnormal-tie"),
                                   (1.0, np.float32(2.0 ** -23 + 2.0 ** -24), 0x0004, "fp16-subnormal-result"), (-1.0, None, 0x8001, "fp16-subnormal-result")):
        w[:, 0, 0, 0] = wv
        bits, ref = _grouped_7x7(dev, "fp16", x, w, None if bias is None else np.full(4, bias, np.float32))
        check(bits, ref, "fp16", tag)
        assert (bits == pattern).all(), (tag, bits)
        seen.add(tag)
    assert seen == {"bf16-up", "bf16-down", "fp16-up", "fp16-down", "fp16-max", "fp16-overflow", "fp16-subnormal-input",
                    "fp16-subnormal-tie", "fp16-subnormal-result"}, seen


# ---- 3. grad_weight ------------------------------------------------------------------------------------------------------------------

# the geometry tables, plus one small case per stage-1 kernel of gconv.hip (1 x 1 tile, 3 x 3 tile, the generic reduction)
GW_EXTRA = [G.Case(cin_g=4, cout_g=4, G=4, N=2, kernel=k, stride=(1, 1), padding=p, dilation=(1, 1), H=9, W=11, layout=lay)
            for k, p, lay in (((1, 1), (0, 0), ("nchw", "nchw")), ((3, 3), (1, 1), ("channels_last", "channels_last")),
                              ((5, 5), (2, 2), ("nchw", "channels_last")))]
GW_ALL = ALL + [("gcx", j) for j in range(len(GW_EXTRA))]
GW_IDS = IDS + [f"gcx-{c.id}" for c in GW_EXTRA]


@pytest.mark.parametrize("fam,i", GW_ALL, ids=GW_IDS)
def test_grad_weight_is_rne_of_the_f32_entry_repeatable_and_inside_the_bound(dev, fam, i):
    F = Gc if fam == "gcx" else FAMS[fam]
    c = GW_EXTRA[i] if fam == "gcx" else F.cases[i]
    xs, ws, ys = F.shapes(c)
    lx, ly = F.layouts(c)
    STATS["cases"] += 1
    fmt = ("bf16", "fp16")[i % 2]
    one = HR.FORMATS[fmt]["one"]
    # real values over six decades that stay inside fp16's range (|v| < 100), so the bound below is finite in both formats
    (xb, x32), (gb_, g32) = half_of(D.gauss6(5000 + i, xs) / 64, fmt), half_of(D.gauss6(5001 + i, ys) / 64, fmt)
    # weights around the STE bound: 1.0 (kept) and the next value above it (bf16: 1.0078125, masked; fp16: 1.0009765625, kept)
    wb, w32 = half_of(D.weights(5002 + i, ws), fmt)
    r = D._rng(5003 + i)
    sel = r.rand(*ws) < 0.3
    wb = np.where(sel, np.array([one, one + 1, one | 0x8000, (one + 1) | 0x8000], np.uint16)[r.randint(0, 4, size=ws)], wb).astype(np.uint16)
    w32 = HR.UPCAST[fmt](wb)
    thr = float(D.STE) if i % 3 else 0.0
    xd, gd = to_dev(dev, xb, fmt, lx), to_dev(dev, gb_, fmt, ly)
    need = F.work(c, xs, ws)
    # the "_f32" entry on the upcast operands
    gw32, gb32 = F.gwt(c, xd.float(), gd.float(), f32_dev(dev, w32), thr, want_bias=True)
    gw32, gb32 = gw32.cpu().numpy(), gb32.cpu().numpy()
    got = {}
    for w_f32 in (False, True):
        wd = f32_dev(dev, w32) if w_f32 else to_dev(dev, wb, fmt)
        dt = torch.float32 if w_f32 else FMTS[fmt]
        bw, ow = guarded(dev, ws, "nchw", dt)
        bb, ob = guarded(dev, (ws[0],), "nchw", dt)
        bk, work = guarded(dev, (need,), "nchw", torch.float32)
        gw, gb = F.gwt(c, xd, gd, wd, thr, out=ow, out_bias=ob, workspace=work)
        assert gw is ow and gb is ob and intact(bw) and intact(bb) and intact(bk)
        got[w_f32] = (bits_of(gw), bits_of(gb))
        gw2, gb2 = F.gwt(c, xd, gd, wd, thr, want_bias=True)
        assert np.array_equal(bits_of(gw2), got[w_f32][0]) and np.array_equal(bits_of(gb2), got[w_f32][1])          # repeatable
    # fp32 weight: the bits of the "_f32" entry; half weight: those bits rounded once
    assert np.array_equal(got[True][0].view(np.uint32), gw32.view(np.uint32)) and np.array_equal(got[True][1].view(np.uint32), gb32.view(np.uint32))
    STATS["compared"] += gw32.size + gb32.size
    check(got[False][0], gw32, fmt, "grad_weight")
    check(got[False][1], gb32, fmt, "grad_bias")
    # ... and inside the float64 bound plus one rounding
    gw64, ab, gb64 = F.gw_ref(c, x32, g32)
    L = c.N * ys[2] * ys[3]
    masked = (np.abs(w32) > D.STE) if thr > 0 else np.zeros(ws, bool)
    want64 = np.where(masked, 0.0, gw64.reshape(ws))
    bound = np.where(masked, 0.0, D.grad_weight_bound(ab.reshape(ws), L))
    val = HR.UPCAST[fmt](got[False][0]).astype(np.float64)
    assert (np.abs(val - want64) <= bound + HR.half_ulp(np.abs(want64) + bound, fmt)).all()
    if thr > 0:
        assert (val[masked] == 0).all() and (got[True][0][masked] == 0).all()
        kept_next = (wb & 0x7FFF) == one + 1
        assert fmt == "bf16" or not masked[kept_next].any()          # fp16's next value above 1.0 is below 1.001: kept
        assert fmt == "fp16" or masked[kept_next].all()
        assert not masked[(wb & 0x7FFF) == one].any()
    bb_ = D.grad_weight_bound(np.abs(g32.astype(np.float64)).sum((0, 2, 3)), L)
    assert (np.abs(HR.UPCAST[fmt](got[False][1]).astype(np.float64) - gb64) <= bb_ + HR.half_ulp(np.abs(gb64) + bb_, fmt)).all()


# ---- 4. layers -------------------------------------------------------------------------------------------------------------------------

LAYER_SHAPES = {"dw1": dict(C=19, cout=19, groups=19, H=7, W=9), "dw2": dict(C=16, cout=32, groups=16, H=14, W=5),
                "g2": dict(C=16, cout=24, groups=8, H=6, W=7), "g4": dict(C=32, cout=16, groups=8, H=5, W=11),
                "g8": dict(C=32, cout=20, groups=4, H=9, W=6)}


def _switches_on(monkeypatch):
    monkeypatch.setattr(_fused, "DEPTHWISE_HALF", True)
    monkeypatch.setattr(_fused, "GROUPED_HALF_MAX_CIN_G", 8)


def _make_layer(cls, s, dev, seed, stochastic=False):
    layer = cls(s["C"], s["cout"], 3, stride=1, padding=1, groups=s["groups"], bias=True, deterministic=not stochastic).to(dev)
    with torch.no_grad():
        layer.weight.copy_(f32_dev(dev, D.weights(seed, tuple(layer.weight.shape))))
        layer.bias.copy_(f32_dev(dev, D.gauss6(seed + 1, (s["cout"],)) / 8))
    return layer


def _layer_refs(s, x32, wq32, b32, go32):
    geom = ((3, 3), (1, 1), (1, 1), (1, 1))
    if s["groups"] == s["C"]:
        w3 = wq32.reshape(wq32.shape[0], 3, 3)
        return quiet(D.forward, x32, w3, b32, *geom), (None if go32 is None else quiet(D.grad_input, go32, w3, x32.shape, *geom))
    return (quiet(G.forward, x32, wq32, b32, s["groups"], *geom),
            None if go32 is None else quiet(G.grad_input, go32, wq32, x32.shape, s["groups"], *geom))


@pytest.mark.parametrize("shape", list(LAYER_SHAPES))
@pytest.mark.parametrize("cls", (BinConv2d, TerConv2d), ids=("bin", "ter"))
def test_layers_take_the_half_routes_with_the_reference_bits(dev, monkeypatch, cls, shape):
    """{.bfloat16(), .half(), fp32 under autocast to each} x {train deterministic, train stochastic, eval} x {NCHW, channels-last}
    x {+-1, real-valued} inputs: dtypes by the README's rule, bits equal to the composition of the references, no library path."""
    _switches_on(monkeypatch)
    s = LAYER_SHAPES[shape]
    fam = "depthwise" if s["groups"] == s["C"] else "grouped"
    kind = cls.kind
    xs = (2, s["C"], s["H"], s["W"])
    STATS["cases"] += 1
    n = 0
    for fmt, tdt in FMTS.items():
        for autocast in (False, True):
            for mode in ("det", "stoch", "eval"):
                for layout in ("nchw", "channels_last"):
                    for real in (False, True):
                        n += 1
                        layer = _make_layer(cls, s, dev, 40 + n, stochastic=mode == "stoch")
                        if not autocast:
                            layer = layer.to(tdt)
                        if mode == "eval":
                            layer.eval()
                        wdt = torch.float32 if autocast else tdt
                        xb, x32 = half_of(D.gauss6(900 + n, xs) / 16 if real else D.pm1(900 + n, xs), fmt)
                        xd = to_dev(dev, xb, fmt, layout).requires_grad_(mode != "eval")
                        lib, took = dict(_fused.LIBRARY_PATHS), _fused.STREAMING_HALF_STATS[fam]
                        calls = dict(_lib.call_counts)
                        torch.manual_seed(77 + n)
                        with torch.autocast("cuda", dtype=tdt, enabled=autocast), torch.set_grad_enabled(mode != "eval"):
                            y = layer(xd)
                        assert isinstance(y, torch.Tensor) and y.dtype == tdt and y.shape[1] == s["cout"]
                        # the weight image the kernels multiplied: Q(W) in training (the saved draw of a stochastic layer), the stored image in eval
                        w_up = layer.weight.detach().float().cpu().numpy()
                        if mode == "stoch":
                            torch.manual_seed(77 + n)
                            wq32 = layer._op.apply(layer.weight.detach()).float().cpu().numpy()
                            assert set(np.unique(wq32)) <= {-1.0, 0.0, 1.0}
                        elif mode == "det":
                            wq32 = D.quantize(w_up, kind)
                        else:
                            wq32 = w_up
                            assert set(np.unique(wq32)) <= {-1.0, 0.0, 1.0}
                        b32 = layer.bias.detach().to(tdt).float().cpu().numpy()          # an fp32 bias under autocast is rounded first
                        go32 = gb_ = None
                        if mode != "eval":
                            gb_, go32 = half_of(D.gauss6(1900 + n, tuple(y.shape)) / 16, fmt)
                        y32, gx32 = _layer_refs(s, x32, wq32, b32, go32)
                        check(bits_of(y), y32, fmt, ("layer y", fmt, autocast, mode, layout, real))
                        used = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
                        stem = "qt_dwconv2d" if fam == "depthwise" else "qt_gconv2d"
                        assert used.get(stem + "_h") == 1, used
                        if mode != "eval":
                            god = to_dev(dev, gb_, fmt, layout)
                            y.backward(god)
                            assert xd.grad.dtype == tdt and layer.weight.grad.dtype == wdt and layer.bias.grad.dtype == wdt
                            check(bits_of(xd.grad), gx32, fmt, ("layer gx", fmt, autocast, mode, layout, real))
                            # grad_weight / grad_bias: the "_f32" entry on the upcast operands with the layer's mask, rounded once
                            F = Dw if fam == "depthwise" else Gc
                            c = G.Case(cin_g=s["C"] // s["groups"], cout_g=s["cout"] // s["groups"], G=s["groups"], C=s["C"], m=s["cout"] // s["C"],
                                       N=2, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), H=s["H"], W=s["W"], layout=(layout, layout))
                            gw32, gb32 = F.gwt(c, xd.detach().float(), god.float(), f32_dev(dev, w_up), float(D.STE), want_bias=True)
                            if autocast:
                                assert torch.equal(layer.weight.grad, gw32) and torch.equal(layer.bias.grad, gb32)
                                STATS["compared"] += gw32.numel() + gb32.numel()
                            else:
                                check(bits_of(layer.weight.grad), gw32.cpu().numpy(), fmt, "layer gw")
                                check(bits_of(layer.bias.grad), gb32.cpu().numpy(), fmt, "layer gb")
                            used = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
                            assert used.get(stem + "_grad_input_h") == 1 and used.get(stem + "_grad_weight_h") == 1, used
                        assert dict(_fused.LIBRARY_PATHS) == lib and _fused.STREAMING_HALF_STATS[fam] == took + 1
    assert n == 48


def test_declining_cases_run_the_torch_expression_and_count_a_library_path(dev, monkeypatch):
    _switches_on(monkeypatch)
    s = LAYER_SHAPES["g4"]
    xb, x32 = half_of(D.pm1(3, (2, 32, 5, 11)), "bf16")
    x = to_dev(dev, xb, "bf16")

    def declines(layer, inp, ctx=None):
        lib, took, calls = sum(_fused.LIBRARY_PATHS.values()), sum(_fused.STREAMING_HALF_STATS.values()), dict(_lib.call_counts)
        with (ctx or torch.autocast("cuda", enabled=False)):
            y = layer(inp)
        assert sum(_fused.LIBRARY_PATHS.values()) >= lib + 1 and sum(_fused.STREAMING_HALF_STATS.values()) == took
        assert all(_lib.call_counts[k] == calls.get(k, 0) for k in ("qt_dwconv2d_h", "qt_gconv2d_h"))
        return y

    bf = _make_layer(BinConv2d, s, dev, 5).bfloat16()
    y = declines(bf, x, torch.autocast("cuda", dtype=torch.float16))                   # a bf16 model under fp16 autocast
    assert y.dtype == torch.float16
    dwd = DorefaConv2d(16, 16, 3, padding=1, groups=16, bit_width=1).to(dev).bfloat16()
    declines(dwd, to_dev(dev, half_of(D.pm1(4, (2, 16, 6, 6)), "bf16")[0], "bf16"))      # DoReFa keeps its path
    two = BinConv2d(8, 8, 3, padding=1, groups=2).to(dev).bfloat16()
    declines(two, to_dev(dev, half_of(D.pm1(5, (2, 8, 6, 6)), "bf16")[0], "bf16"))       # groups == 2
    monkeypatch.setattr(_fused, "GROUPED_HALF_MAX_CIN_G", 0)
    y_lib = declines(bf, x)                                                              # the grouped switch off
    monkeypatch.setattr(_fused, "GROUPED_HALF_MAX_CIN_G", 2)
    declines(bf, x)                                                                      # cin_g 4 above the constant
    dw = _make_layer(TerConv2d, LAYER_SHAPES["dw1"], dev, 6).half()
    xh = to_dev(dev, half_of(D.pm1(6, (2, 19, 7, 9)), "fp16")[0], "fp16")
    monkeypatch.setattr(_fused, "DEPTHWISE_HALF", False)
    declines(dw, xh)                                                                     # the depthwise switch off
    # ... and switched on, the route gives what the library expression gave on these exactly representable sums
    _switches_on(monkeypatch)
    took = _fused.STREAMING_HALF_STATS["grouped"]
    y_own = bf(x)
    assert _fused.STREAMING_HALF_STATS["grouped"] == took + 1
    ref = quiet(G.forward, x32, D.quantize(bf.weight.detach().float().cpu().numpy(), "binary"),
                bf.bias.detach().float().cpu().numpy(), 8, (3, 3), (1, 1), (1, 1), (1, 1))
    check(bits_of(y_own), ref, "bf16", "route on")
    assert y_lib.dtype == y_own.dtype == torch.bfloat16


# ---- 5. no host synchronisation: capture and replay ----------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ("bf16-depthwise", "fp16-grouped"))
def test_forward_and_backward_replay_from_a_captured_graph(dev, monkeypatch, which):
    _switches_on(monkeypatch)
    fmt, shape, cls = ("bf16", "dw2", TerConv2d) if which == "bf16-depthwise" else ("fp16", "g4", BinConv2d)
    s = LAYER_SHAPES[shape]
    layer = _make_layer(cls, s, dev, 60).to(FMTS[fmt])
    xs_, ys_ = (2, s["C"], s["H"], s["W"]), (2, s["cout"], s["H"], s["W"])
    xs = to_dev(dev, half_of(D.gauss6(61, xs_) / 16, fmt)[0], fmt).requires_grad_(True)
    gs = to_dev(dev, half_of(D.gauss6(62, ys_) / 16, fmt)[0], fmt)

    def step():
        layer.zero_grad(set_to_none=False)
        if xs.grad is not None:
            xs.grad.zero_()
        y = layer(xs)
        y.backward(gs)
        return y.detach()

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        torch.cuda.synchronize(dev)
        with _no_collection_inside(), torch.cuda.graph(graph, stream=stream):
            y_static = step()
    torch.cuda.synchronize(dev)
    stem = "qt_dwconv2d_h" if shape == "dw2" else "qt_gconv2d_h"
    for rep in range(2):                                                  # replayed twice, on new data each time
        x2 = to_dev(dev, half_of(D.gauss6(63 + rep, xs_) / 16, fmt)[0], fmt)
        g2 = to_dev(dev, half_of(D.gauss6(65 + rep, ys_) / 16, fmt)[0], fmt)
        with torch.no_grad():
            xs.copy_(x2)
            gs.copy_(g2)
        calls = _lib.call_counts[stem]
        graph.replay()
        torch.cuda.synchronize(dev)
        assert _lib.call_counts[stem] == calls                            # a replay, not a call
        got = (y_static.clone(), xs.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone())
        twin = copy.deepcopy(layer)
        twin.zero_grad(set_to_none=True)
        xe = x2.clone().requires_grad_(True)
        ye = twin(xe)
        ye.backward(g2)
        assert _lib.call_counts[stem] == calls + 1
        for a, b in zip(got, (ye.detach(), xe.grad, twin.weight.grad, twin.bias.grad)):
            assert a.dtype == FMTS[fmt] and torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- 6. alignment --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", list(FMTS))
def test_views_at_an_odd_element_offset_give_the_same_bits(dev, fmt):
    """Activations that are 2-byte but not 4-byte aligned: a view one element into its storage."""
    def odd(t):
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = flat[1:].view(t.shape) if t.is_contiguous() else flat[1:].view(t.shape[0], t.shape[2], t.shape[3], t.shape[1]).permute(0, 3, 1, 2)
        v.copy_(t)
        assert v.data_ptr() % 4 == 2 and v.stride() == t.stride()
        return v

    for layout in ("nchw", "channels_last"):
        x = to_dev(dev, half_of(D.gauss6(70, (2, 12, 9, 7)) / 16, fmt)[0], fmt, layout)
        for F, w_shape, groups, y_shape in ((Dw, (24, 1, 3, 3), 12, (2, 24, 9, 7)), (Gc, (8, 3, 3, 3), 4, (2, 8, 9, 7))):
            c = G.Case(G=groups, stride=(1, 1), padding=(1, 1), dilation=(1, 1))
            w = to_dev(dev, half_of(D.weights(71, w_shape), fmt)[0], fmt)
            go = to_dev(dev, half_of(D.gauss6(72, y_shape) / 16, fmt)[0], fmt, layout)
            y, gx = F.fwd(c, x, w, None, "ternary", None), F.gin(c, tuple(x.shape), w, go, "ternary", None)
            gw, gb = F.gwt(c, x, go, w, 1.001, want_bias=True)
            yo, gxo = F.fwd(c, odd(x), odd(w), None, "ternary", None), F.gin(c, tuple(x.shape), w, odd(go), "ternary", None)
            gwo, gbo = F.gwt(c, odd(x), odd(go), w, 1.001, want_bias=True)
            for a, b in ((y, yo), (gx, gxo), (gw, gwo), (gb, gbo)):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16))
            STATS["compared"] += y.numel() + gx.numel() + gw.numel() + gb.numel()


def test_module_totals(dev):
    """Runs last in the file: zero differing bit patterns over everything compared above (each comparison also asserted on its own)."""
    assert STATS["differing"] == 0
