"""Grouped BinConv2d / TerConv2d inside the fused inference chain, on the GPU: the plane forms of csrc/gconv.hip through
ops.grouped_conv2d_sign / ops.grouped_conv2d_from_bits, layers.fused.FusedGroupedBnSign and lazy.py under ``lazy.grouped_deferred()``.

The reference is independent of the package's packers: tests/_gconv_exact.py's float32 forward on the decoded +-1 image (which
reproduces qt_gconv2d_f32 bit for bit), then tests/_dw_planes.py's threshold bit and its two numpy plane packers.  Every comparison is
``np.array_equal`` / ``torch.equal``; every output buffer lies between sentinel words.  All shapes are small: the file runs in a few
seconds."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import _dw_planes as P
import _gconv_exact as X
from test_gpu_dwconv_chain import GEOMS
from pytorch_quantize_impls_amd import _lib, lazy, ops, utils
from pytorch_quantize_impls_amd.functions import BinaryConnect, _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, FusedConvPoolBnSign, FusedGroupedBnSign, fuse_sequential

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SENTINEL_F = 12345.0
PAD = 64                     # words: the guarded views stay 16-byte aligned
SIGN, F32, EAGER = "qt_gconv2d_sign", "qt_gconv2d_bits_f32", "qt_gconv2d_f32"

# (G, cin_g, cout_g): input spans of 8 / 48 / 72 / 20 / 136 / 32 channels — one to five plane words, word-boundary crossings, ld
# padding —, output groups that straddle output words, a partial last word, Cout % 4 != 0, input word != output word
GCC = ((4, 2, 1), (12, 4, 4), (9, 8, 3), (5, 4, 12), (17, 8, 8), (16, 2, 5))
MAPS = ((7, 7), (9, 8), (14, 14), (5, 17))
BATCHES = (1, 3)
HALOS = ((0, 0), (1, 1), (2, 1))          # besides "none": bit planes
ALPHAS = (1.0, -1.0, 0.0, 0.5)
KINDS = ("binary", "ternary", "raw")


class Case(dict):
    __getattr__ = dict.__getitem__


def _case(i):
    (G, ci, co), (H, W) = GCC[i % len(GCC)], MAPS[i % len(MAPS)]
    k, s, p, d = GEOMS[i % len(GEOMS)]
    N = BATCHES[(i // 2) % 2]
    return Case(i=i, G=G, cin_g=ci, cout_g=co, C=G * ci, Cout=G * co, H=H, W=W, N=N, kernel=k, stride=s, padding=p, dilation=d,
                id=f"g{G}i{ci}o{co}N{N}-k{k[0]}x{k[1]}-s{s[0]}{s[1]}-p{p[0]}{p[1]}-d{d[0]}-{H}x{W}")


# every geometry twice, with another (G, cin_g, cout_g), map and batch; no combination has cin_g kh kw > 512 (8 * 49 = 392)
CASES = [_case(i) for i in range(2 * len(GEOMS))]


def test_the_case_list_covers_every_axis_value():
    assert {(c.G, c.cin_g, c.cout_g) for c in CASES} == set(GCC) and {(c.H, c.W) for c in CASES} == set(MAPS)
    assert {(c.kernel, c.stride, c.padding, c.dilation) for c in CASES} == set(GEOMS) and len(GEOMS) == 7
    assert {c.N for c in CASES} == set(BATCHES)
    assert all(c.cin_g * c.kernel[0] * c.kernel[1] <= 512 for c in CASES)
    assert {c.cin_g for c in CASES} == {2, 4, 8} and {(c.C + 31) // 32 for c in CASES} >= {1, 2, 3, 5}
    assert any(c.Cout % 4 for c in CASES) and any(c.Cout % 32 for c in CASES)
    assert any(32 % c.cout_g for c in CASES)                                     # output groups that straddle output words
    # every halo, "none" and both planes at once are walked inside each designed case; every kind in the kinds test
    assert {i % 3 for i in range(len(CASES))} == {0, 1, 2} and {KINDS[i % 3] for i in range(len(CASES))} == set(KINDS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _geom(c):
    return c.kernel, c.stride, c.padding, c.dilation


def _to(dev, a, layout="nchw"):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" and t.dim() == 4 else t


def _guarded_words(dev, rows, ld):
    buf = torch.full((rows * ld + 2 * PAD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[PAD:PAD + rows * ld].view(rows, ld)


def _guarded_f32(dev, shape, layout):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL_F, dtype=torch.float32, device=dev)
    mid = buf[PAD:PAD + n]
    if layout == "channels_last":
        N, C, H, W = shape
        return buf, mid.view(N, H, W, C).permute(0, 3, 1, 2)
    return buf, mid.view(*shape)


def _intact(buf):
    v = SENTINEL if buf.dtype == torch.int32 else SENTINEL_F
    return bool((buf[:PAD] == v).all() and (buf[-PAD:] == v).all())


def _planes_of(dev, x):
    """ops.BitPlanes of the +-1 image x [N, C, H, W], packed by numpy."""
    N, C, H, W = x.shape
    return ops.BitPlanes(sign=_to(dev, P.pack_sign(x < 0)), rows=N * H * W, K=C)


def _run_sign(dev, c, x, w, b, alpha, beta, kind, halo=None, with_bits=False):
    """The planes of one launch as numpy arrays, written between sentinels: bits (halo None), nibble plane, or both."""
    Ho, Wo = X.out_hw(c.H, c.W, *_geom(c))
    kw, bufs = {}, []
    if halo is None or with_bits:
        bb, kw["out_sign"] = _guarded_words(dev, c.N * Ho * Wo, P.packed_ld(c.Cout))
        bufs.append(bb)
    if halo is not None:
        bn, kw["out_nib"] = _guarded_words(dev, c.N * (Ho + 2 * halo[0]) * (Wo + 2 * halo[1]), P.pixel_ld_nib(c.Cout))
        bufs.append(bn)
    before = _lib.call_counts.get(SIGN, 0)
    out, hw = ops.grouped_conv2d_sign(_planes_of(dev, x), _to(dev, w), None if b is None else _to(dev, b), _to(dev, alpha), _to(dev, beta),
                                      c.stride, c.padding, c.dilation, c.G, kind=kind, shape=x.shape, out_halo=halo, with_bits=with_bits,
                                      **kw)
    assert _lib.call_counts[SIGN] == before + 1 and hw == (Ho, Wo)
    assert all(_intact(b_) for b_ in bufs)
    if halo is None:
        assert isinstance(out, ops.BitPlanes) and out.sign is kw["out_sign"] and (out.rows, out.K) == (c.N * Ho * Wo, c.Cout)
        return out.sign.cpu().numpy()
    if with_bits:
        assert out[0].sign is kw["out_sign"] and out[1].words is kw["out_nib"]
        return out[0].sign.cpu().numpy(), out[1].words.cpu().numpy()
    assert isinstance(out, ops.NibPlanes) and out.words is kw["out_nib"] and out.K == c.Cout
    return out.words.cpu().numpy()


def _run_f32(dev, c, x, w, b, kind, layout):
    Ho, Wo = X.out_hw(c.H, c.W, *_geom(c))
    buf, out = _guarded_f32(dev, (c.N, c.Cout, Ho, Wo), layout)
    before = _lib.call_counts.get(F32, 0)
    y = ops.grouped_conv2d_from_bits(_planes_of(dev, x), x.shape, _to(dev, w), None if b is None else _to(dev, b), c.stride, c.padding,
                                     c.dilation, c.G, kind=kind, out=out)
    assert y is out and _intact(buf) and _lib.call_counts[F32] == before + 1
    return y


@functools.lru_cache(maxsize=None)
def _designed(i):
    """+-1 activations, weights in {-1, 0, +1}, a non-integer bias (odd cases: none); alpha cycles through {+1, -1, 0, 0.5} and
    beta = -fl(alpha t) with t an output the channel really takes, so fl(fl(y alpha) + beta) is exactly 0 there: ties, bit 0."""
    c = CASES[i]
    x = X.pm1(1000 + i, (c.N, c.C, c.H, c.W))
    w = X.grid_weights(1100 + i, (c.Cout, c.cin_g) + c.kernel)
    b = ((X.small_ints(1200 + i, (c.Cout,)) + np.float32(0.25)) * np.float32(1.3)).astype(np.float32) if i % 2 == 0 else None
    y = X.forward(x, w, b, c.G, *_geom(c))
    assert y.dtype == np.float32
    r = np.random.RandomState(1300 + i)
    alpha = np.array([ALPHAS[(k + i) % 4] for k in range(c.Cout)], dtype=np.float32)
    N, _, Ho, Wo = y.shape
    t = y[r.randint(0, N, c.Cout), np.arange(c.Cout), r.randint(0, Ho, c.Cout), r.randint(0, Wo, c.Cout)]
    beta = (-(alpha * t)).astype(np.float32)
    neg = P.threshold_bits(y, alpha, beta)
    z = y * alpha[None, :, None, None] + beta[None, :, None, None]
    ties = int(((z == 0) & (alpha != 0)[None, :, None, None]).sum())
    assert ties > 0 and not neg[z == 0].any()
    return Case(x=x, w=w, b=b, y=y, alpha=alpha, beta=beta, neg=neg, ties=ties)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_designed_operands_every_output_form(dev, i):
    c, r = CASES[i], _designed(i)
    assert r.ties > 0 and (r.w == 0).any()
    want_bits = P.pack_sign(r.neg)
    args = (dev, c, r.x, r.w, r.b, r.alpha, r.beta, "raw")
    got = _run_sign(*args)
    assert got.dtype == np.int32 and np.array_equal(got, want_bits)
    for halo in HALOS:
        assert np.array_equal(_run_sign(*args, halo=halo), P.pack_nib(r.neg, halo)), halo
    both = _run_sign(*args, halo=HALOS[i % 3], with_bits=True)                  # both planes from one launch
    assert np.array_equal(both[0], want_bits) and np.array_equal(both[1], P.pack_nib(r.neg, HALOS[i % 3]))
    # the weights are fixed points of the ternary quantiser: ``kind`` applies to the taps and changes nothing here
    assert np.array_equal(_run_sign(dev, c, r.x, r.w, r.b, r.alpha, r.beta, "ternary"), want_bits)
    # planes in, fp32 out: the value itself, in either layout, equal to the reference and to the fp32 kernel on the decoded image
    for layout in ("nchw", "channels_last"):
        y = _run_f32(dev, c, r.x, r.w, r.b, "raw", layout)
        assert np.array_equal(y.cpu().numpy(), r.y), layout
        e = ops.grouped_conv2d(_to(dev, r.x, layout), _to(dev, r.w), None if r.b is None else _to(dev, r.b), c.stride, c.padding,
                               c.dilation, c.G, kind="raw")
        assert torch.equal(y, e), layout
    y = ops.grouped_conv2d_from_bits(_planes_of(dev, r.x), r.x.shape, _to(dev, r.w), None, c.stride, c.padding, c.dilation, c.G)
    assert y.is_contiguous() and np.array_equal(y.cpu().numpy(), X.forward(r.x, r.w, None, c.G, *_geom(c)))
    y = ops.grouped_conv2d_from_bits(_planes_of(dev, r.x), r.x.shape, _to(dev, r.w), None, c.stride, c.padding, c.dilation, c.G,
                                     channels_last=True)
    assert y.is_contiguous(memory_format=torch.channels_last) and np.array_equal(y.cpu().numpy(), X.forward(r.x, r.w, None, c.G, *_geom(c)))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_kinds_classify_real_valued_weights(dev, i):
    """Real-valued weights around the quantisers' decision points, quantised inside the launch ("binary", "ternary" — with real
    zeros) or, "raw", an on-grid image; Gaussian (alpha, beta) with negative and zero alphas among the channels."""
    c, kind = CASES[i], KINDS[i % 3]
    x = X.pm1(2000 + i, (c.N, c.C, c.H, c.W))
    w = X.weights(2100 + i, (c.Cout, c.cin_g) + c.kernel)
    wq = X.quantize(w, "ternary" if kind == "raw" else kind)
    if kind != "binary":
        assert (wq == 0).any() and (wq > 0).any() and (wq < 0).any()
    w_in = wq if kind == "raw" else w
    b = X.gauss6(2200 + i, (c.Cout,)) if i % 2 == 1 else None
    y = X.forward(x, wq, b, c.G, *_geom(c))
    r = np.random.RandomState(2300 + i)
    alpha = r.randn(c.Cout).astype(np.float32)
    alpha[1::5] = 0
    beta = (r.randn(c.Cout) * 3).astype(np.float32)
    neg = P.threshold_bits(y, alpha, beta)
    assert neg.any() and not neg.all()
    assert np.array_equal(_run_sign(dev, c, x, w_in, b, alpha, beta, kind), P.pack_sign(neg))
    halo = HALOS[i % 3]
    assert np.array_equal(_run_sign(dev, c, x, w_in, b, alpha, beta, kind, halo=halo), P.pack_nib(neg, halo)), halo
    got = _run_f32(dev, c, x, w_in, b, kind, ("nchw", "channels_last")[i % 2])
    assert np.array_equal(got.cpu().numpy(), y)
    assert torch.equal(got, ops.grouped_conv2d(_to(dev, x), _to(dev, w_in), None if b is None else _to(dev, b), c.stride, c.padding,
                                               c.dilation, c.G, kind=kind))


@pytest.mark.parametrize("i", (0, 1, 2, 4, 5), ids=[CASES[i].id for i in (0, 1, 2, 4, 5)])
def test_extreme_sums_and_border_tap_counts(dev, i):
    """All-(+1) and all-(-1) images against all-(+1) weights: +-cin_g times the taps inside the image, the largest sums there are."""
    c = CASES[i]
    w = np.ones((c.Cout, c.cin_g) + c.kernel, dtype=np.float32)
    alpha = np.ones(c.Cout, dtype=np.float32)
    for sgn in (1.0, -1.0):
        x = np.full((c.N, c.C, c.H, c.W), sgn, dtype=np.float32)
        y = X.forward(x, w, None, c.G, *_geom(c))
        assert np.abs(y).max() == c.cin_g * c.kernel[0] * c.kernel[1] and len(np.unique(y)) > (c.padding != (0, 0))
        assert np.array_equal(_run_f32(dev, c, x, w, None, "raw", "nchw").cpu().numpy(), y)
        # the threshold between the border counts and the full count, on both sides of zero
        beta = np.full(c.Cout, -sgn * (np.abs(y).max() - 0.5), dtype=np.float32)
        neg = P.threshold_bits(y, alpha, beta)
        assert np.array_equal(_run_sign(dev, c, x, w, None, alpha, beta, "binary"), P.pack_sign(neg))
        assert np.array_equal(_run_sign(dev, c, x, w, None, alpha, beta, "raw", halo=(1, 1)), P.pack_nib(neg, (1, 1)))


def test_wrappers_check_their_operands(dev):
    x = X.pm1(1, (1, 16, 5, 5))
    pl = _planes_of(dev, x)
    w = _to(dev, X.grid_weights(2, (8, 4, 3, 3)))
    a = torch.ones(8, device=dev)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_sign(pl, w, None, torch.ones(7, device=dev), a, 1, 1, 1, 4, shape=x.shape)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_sign(pl, w, None, a.cpu(), a, 1, 1, 1, 4, shape=x.shape)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_sign(_to(dev, x), w, None, a, a, 1, 1, 1, 4)                   # an fp32 tensor: that form is not built
    with pytest.raises(ValueError):
        ops.grouped_conv2d_sign(pl, w, None, a, a, 1, 1, 1, 4)                            # no logical shape
    with pytest.raises(ValueError):
        ops.grouped_conv2d_sign(pl, w, None, a, a, 1, 1, 1, 4, shape=(1, 16, 5, 6))
    with pytest.raises(ValueError):
        ops.grouped_conv2d_sign(pl, w, None, a, a, 1, 1, 1, 4, shape=x.shape, out_halo=(-1, 0))
    with pytest.raises(ValueError):
        ops.grouped_conv2d_sign(pl, w, None, a, a, 1, 1, 1, 2, shape=x.shape)             # groups do not match the weight
    for cin_g in (1, 16):                                                                 # (3 and 6: no plane of 16 channels divides)
        with pytest.raises(ValueError):
            ops.grouped_conv2d_from_bits(pl, x.shape, _to(dev, X.grid_weights(2, (16, cin_g, 3, 3))), None, 1, 1, 1, 16 // cin_g)
    pl12 = _planes_of(dev, X.pm1(1, (1, 12, 5, 5)))
    with pytest.raises(ValueError):
        ops.grouped_conv2d_from_bits(pl12, (1, 12, 5, 5), _to(dev, X.grid_weights(2, (8, 3, 3, 3))), None, 1, 1, 1, 4)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_from_bits(pl, x.shape, _to(dev, X.grid_weights(2, (8, 4, 5, 10))), None, 1, 5, 1, 4)      # 50 taps
    # empty batch: planes of zero rows, nothing launched
    before = _lib.call_counts.get(SIGN, 0)
    empty = ops.BitPlanes(sign=pl.sign[:0], rows=0, K=16)
    out, hw = ops.grouped_conv2d_sign(empty, w, None, a, a, 1, 1, 1, 4, shape=(0, 16, 5, 5))
    assert out.sign.shape == (0, 4) and hw == (5, 5) and _lib.call_counts.get(SIGN, 0) == before


# ---- module level ----------------------------------------------------------------------------------------------------------------

def _pm1(shape, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g).float() * 2 - 1).to(dev)


def _run(c, g):
    """BatchNorm2d (random statistics and affine parameters, every third weight negative) -> Hardtanh -> BinaryConnect."""
    bn = nn.BatchNorm2d(c)
    bn.running_mean.copy_(torch.randn(c, generator=g) * 2)
    bn.running_var.copy_(torch.rand(c, generator=g) * 20 + 5)
    gamma = torch.rand(c, generator=g) + 0.5
    gamma[::3] *= -1
    bn.weight.data.copy_(gamma)
    bn.bias.data.copy_(torch.randn(c, generator=g) * 0.5)
    return [bn, nn.Hardtanh(inplace=True), BinaryConnect()]


def _ready(seq, dev):
    """Weights spread over [-1.5, 1.5] — the default initialisation lies inside the ternary dead zone — then the device and eval
    mode (which stores the quantised image)."""
    g = torch.Generator().manual_seed(23)
    for m in seq.modules():
        if isinstance(m, (BinConv2d, TerConv2d)):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * 3 - 1.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g))
    return seq.to(dev).eval()


def _triple(dev, grouped, pool=None, seed=5, tail_run=True):
    """pw 1x1 -> run -> ``grouped`` -> run -> pw 1x1 -> run, the un-modified modules; ``pool``: a MaxPool2d(2) between the grouped
    conv and its BatchNorm ("before_bn") or after its sign ("after_sign")."""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    cin, cout = grouped.in_channels, grouped.out_channels
    run = _run(cout, g)
    mid = [nn.MaxPool2d(2), *run] if pool == "before_bn" else ([*run, nn.MaxPool2d(2)] if pool == "after_sign" else run)
    mods = [BinConv2d(16, cin, 1), *_run(cin, g), grouped, *mid, BinConv2d(cout, 24, 1)]
    if tail_run:
        mods += _run(24, g)
    return _ready(nn.Sequential(*mods), dev)


def _value(t):
    return t.value() if isinstance(t, lazy.LazyActivation) else t


def _delta(after, before, name=None):
    if name is None:
        return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}
    return after.get(name, 0) - before.get(name, 0)


@pytest.fixture(autouse=True)
def _fresh_stats():
    start = lazy.DEFER_GROUPED
    lazy.STATS.clear()
    yield
    assert lazy.DEFER_GROUPED is start


@pytest.mark.parametrize("family,pool", (("binary", None), ("ternary", "before_bn"), ("binary", "after_sign"), ("ternary", None)))
def test_unmodified_triple_runs_as_fused_chains(dev, family, pool):
    make = BinConv2d if family == "binary" else TerConv2d
    seq = _triple(dev, make(32, 64, 3, padding=1, groups=8), pool)
    x = _pm1((3, 16, 10, 10), dev)
    with torch.no_grad(), lazy.grouped_deferred(True):
        with lazy.eager():
            e = seq(x)
        assert type(e) is torch.Tensor and e.shape == ((3, 24, 5, 5) if pool else (3, 24, 10, 10))
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        y = seq(x)
        stats, after = dict(lazy.STATS), dict(_lib.call_counts)
        assert isinstance(y, lazy.LazyActivation)
        got = y.value()
    assert torch.equal(got, e)
    # three convs deferred, the two chains between them ran fused, nothing was computed in fp32 on the way
    assert stats.get("deferred") == 3 and stats.get("fused") == 2 and stats.get("materialised", 0) == 0, stats
    assert _delta(after, before, SIGN) == 1 and _delta(after, before, EAGER) == 0 and _delta(after, before, F32) == 0
    assert not [k for k in after if k.startswith("qt_pool_affine_sign_pack") and _delta(after, before, k)]


def test_grouped_layer_followed_by_a_tensor_op_materialises_from_planes(dev):
    g = torch.Generator().manual_seed(17)
    torch.manual_seed(17)
    head = _ready(nn.Sequential(BinConv2d(8, 36, 1), *_run(36, g), TerConv2d(36, 27, 3, stride=2, padding=1, groups=9)), dev)
    tail = nn.Sequential(*_run(27, g)).to(dev).eval()
    x = _pm1((3, 8, 9, 8), dev, 4)
    with torch.no_grad(), lazy.grouped_deferred(True):
        with lazy.eager():
            e_conv = head(x)
            e_sign = tail(e_conv)
        before = dict(_lib.call_counts)
        y = head(x)
        assert isinstance(y, lazy.LazyActivation) and isinstance(y._qt.input, _fused.packed.PackedActivation)
        got = y * 1.0                                   # not in the grammar: the conv's own fp32 value, computed from the planes
        after = dict(_lib.call_counts)
        assert type(got) is torch.Tensor and torch.equal(got, e_conv)
        assert _delta(after, before, F32) == 1 and _delta(after, before, EAGER) == 0 and _delta(after, before, SIGN) == 0
        s = tail(head(x))                               # read after the sign: conv from the planes, the recorded run replayed
        assert isinstance(s, lazy.LazyActivation) and s._qt.signed
        assert torch.equal(s.value(), e_sign)


def test_explicit_fused_form_and_hipgraph_replay(dev):
    seq = _triple(dev, BinConv2d(32, 64, 3, padding=1, groups=8))
    x = _pm1((3, 16, 10, 10), dev)
    seq[0].binary_input = True              # the +-1 hint: nothing asks the device about the input while the graph is captured
    with torch.no_grad(), lazy.grouped_deferred(True):
        with lazy.eager():
            e = seq(x)
        fused = fuse_sequential(seq, fuse_conv=True, fold="device")
        assert [type(m) for m in fused] == [FusedConvPoolBnSign, FusedGroupedBnSign, FusedConvPoolBnSign]
        assert fused[0].out_nib_halo is None and fused[1].out_nib_halo == ((0, 0) if _fused._cfg("PAD_PLANES") else None)
        before = dict(_lib.call_counts)
        out = fused(x)
        assert _delta(dict(_lib.call_counts), before, SIGN) == 1 and _delta(dict(_lib.call_counts), before, EAGER) == 0
        assert isinstance(out, _fused.packed.PackedActivation) and out.shape == tuple(e.shape)
        want_neg = (e < 0).cpu().numpy()
        assert set(np.unique(e.cpu().numpy())) <= {-1.0, 1.0}
        assert np.array_equal(out.planes.sign.cpu().numpy(), P.pack_sign(want_neg))
        graph = utils.graphed(seq, x)
        assert torch.equal(_value(graph(x)), e)
        x2 = _pm1((3, 16, 10, 10), dev, 9)
        with lazy.eager():
            e2 = seq(x2)
        assert torch.equal(_value(graph(x2)), e2) and not torch.equal(e, e2)


def _declined(dev, name):
    if name == "groups2":
        return _triple(dev, BinConv2d(16, 16, 3, padding=1, groups=2), tail_run=False)
    if name == "cin_g3":
        return _triple(dev, BinConv2d(12, 12, 3, padding=1, groups=4), tail_run=False)
    if name == "cin_g6":
        return _triple(dev, TerConv2d(24, 24, 3, padding=1, groups=4), tail_run=False)
    if name == "taps50":
        return _triple(dev, BinConv2d(16, 16, (5, 10), padding=5, groups=4), tail_run=False)
    seq = _triple(dev, BinConv2d(32, 32, 3, padding=1, groups=8), tail_run=False)
    if name == "off_grid":
        seq[4].weight.data.mul_(0.3)
        seq[4].reset_quant_cache()
        assert not seq[4]._eval_on_grid()
    elif name == "training":
        seq[4].train()
    else:
        assert name == "on_grid"
    return seq


@pytest.mark.parametrize("name", ("groups2", "cin_g3", "cin_g6", "off_grid", "taps50", "training"))
def test_declined_layers_keep_their_launches_and_values(dev, name):
    """What the plane kernel does not take runs exactly as with the switch off: the same launches, counted entry by entry, the same
    values, no plane entry."""
    seq = _declined(dev, name)
    x = _pm1((2, 16, 9, 9), dev, 2)
    with torch.no_grad():
        with lazy.eager():
            e = seq(x)
        runs = {}
        for on in (False, True, False, True):             # the first pair warms the layers' caches
            with lazy.grouped_deferred(on):
                before = dict(_lib.call_counts)
                got = _value(seq(x))
                runs[on] = _delta(dict(_lib.call_counts), before)
            assert torch.equal(got, e), on
    assert runs[True] == runs[False] and SIGN not in runs[True] and F32 not in runs[True], (runs[True], runs[False])


def test_the_control_of_the_declined_cases_does_defer(dev):
    seq = _declined(dev, "on_grid")
    x = _pm1((2, 16, 9, 9), dev, 2)
    with torch.no_grad():
        with lazy.eager():
            e = seq(x)
        with lazy.grouped_deferred(True):
            before = dict(_lib.call_counts)
            got = _value(seq(x))
            d = _delta(dict(_lib.call_counts), before)
    assert torch.equal(got, e) and d.get(SIGN) == 1 and EAGER not in d


def test_fp32_tensor_input_is_never_deferred(dev):
    """A grouped layer at the head of a chain, and one behind a chain that materialised: today's launch, an fp32 tensor back."""
    g = torch.Generator().manual_seed(29)
    gl = BinConv2d(32, 32, 3, padding=1, groups=8)
    seq = _ready(nn.Sequential(gl, *_run(32, g), BinConv2d(32, 16, 1)), dev)
    x = _pm1((2, 32, 9, 9), dev, 6)
    with torch.no_grad():
        with lazy.eager():
            e = seq(x)
        with lazy.grouped_deferred(True):
            assert not lazy._conv_can_defer(gl, x) and lazy._conv_can_defer(gl, lazy._ShapeOnly((2, 32, 9, 9)))
            assert not lazy._conv_can_defer(gl, lazy._ShapeOnly((2, 32, 0, 9)))
            before = dict(_lib.call_counts)
            y = gl(x)
            assert type(y) is torch.Tensor and _delta(dict(_lib.call_counts), before, EAGER) == 1
            before = dict(_lib.call_counts)
            got = _value(seq(x))
            d = _delta(dict(_lib.call_counts), before)
        with lazy.grouped_deferred(False):
            assert not lazy._conv_can_defer(gl, lazy._ShapeOnly((2, 32, 9, 9)))
    assert torch.equal(got, e) and d.get(EAGER) == 1 and SIGN not in d and F32 not in d


def test_switch_off_is_the_launch_of_the_parent(dev):
    seq = _triple(dev, BinConv2d(32, 64, 3, padding=1, groups=8))
    x = _pm1((3, 16, 10, 10), dev)
    with torch.no_grad():
        with lazy.eager():
            e = seq(x)
        with lazy.grouped_deferred(False):
            before = dict(_lib.call_counts)
            got = _value(seq(x))
            d = _delta(dict(_lib.call_counts), before)
            mid = seq[:5](x)                              # pw -> run -> grouped: the grouped layer's own result
        with lazy.grouped_deferred(True):
            on = _value(seq(x))
    assert torch.equal(got, e) and torch.equal(on, e)
    assert d.get(EAGER) == 1 and SIGN not in d and F32 not in d, d
    assert type(mid) is torch.Tensor and mid.dtype == torch.float32 and mid.shape == (3, 64, 10, 10)


def test_fused_grouped_block_at_run_time(dev):
    g = torch.Generator().manual_seed(19)
    conv = _ready(BinConv2d(16, 24, 3, padding=1, groups=4), dev)
    blk = FusedGroupedBnSign(conv, _run(24, g)[0].to(dev).eval(), fold="device")
    xn = X.pm1(3, (1, 16, 5, 5))
    act = _fused.packed.PackedActivation(_planes_of(dev, xn), xn.shape)
    with torch.no_grad():
        out = blk(act)
        assert out.planes is not None and out.shape == (1, 24, 5, 5)
        e = nn.Sequential(conv, blk.bn, nn.Hardtanh(), BinaryConnect())
        with lazy.eager():
            want = e(_to(dev, xn))
        assert np.array_equal(out.planes.sign.cpu().numpy(), P.pack_sign((want < 0).cpu().numpy()))
        blk.out_nib_halo = (1, 1)
        nib = blk(act)                          # planes in, the consumer's nibble plane out
        assert nib.planes is None and nib.halo == (1, 1) and nib.nib.words.shape == (49, 4)
        assert np.array_equal(nib.nib.words.cpu().numpy(), P.pack_nib((want < 0).cpu().numpy(), (1, 1)))
        with pytest.raises(ValueError):
            blk(nib)                            # a nibble-only activation: in lazy.py the chain then materialises
        with pytest.raises(TypeError):
            blk(_to(dev, xn))                   # an fp32 device tensor: that form is not built
        conv.weight.data.mul_(0.3)              # off the quantiser's grid
        conv.reset_quant_cache()
        assert not conv._eval_on_grid()
        with pytest.raises(ValueError):
            blk(act)
