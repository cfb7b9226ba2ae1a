"""Depthwise BinConv2d / TerConv2d inside the fused inference chain, on the GPU: the plane forms of csrc/dwconv.hip through
ops.depthwise_conv2d_sign / ops.depthwise_conv2d_from_bits, layers.fused.FusedDepthwiseBnSign and lazy.py under
``lazy.depthwise_deferred()``.

The reference is independent of the package's packers: tests/_dw_exact.py's float32 forward (which reproduces qt_dwconv2d_f32 bit
for bit), then a numpy float32 multiply, a numpy float32 add and ``< 0``, packed with numpy into the two plane layouts
(tests/_dw_planes.py, pinned on hand-written words by tests/test_dwconv_chain_cpu.py).  Every comparison is ``np.array_equal`` /
``torch.equal``; every output buffer lies between sentinel words.  All shapes are small: the file runs in a few seconds."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import _dw_exact as D
import _dw_planes as P
from pytorch_quantize_impls_amd import _lib, lazy, ops, utils
from pytorch_quantize_impls_amd.functions import BinaryConnect, _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, FusedConvPoolBnSign, FusedDepthwiseBnSign, fuse_sequential
from pytorch_quantize_impls_amd.layers.fused import device_sign_fold

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SENTINEL_F = 12345.0
PAD = 64                     # words: the guarded views stay 16-byte aligned
SIGN, F32 = "qt_dwconv2d_sign", "qt_dwconv2d_bits_f32"

#            kernel  stride  padding dilation
GEOMS = (((3, 3), (1, 1), (1, 1), (1, 1)),
         ((3, 3), (2, 2), (1, 1), (1, 1)),
         ((5, 5), (1, 1), (2, 2), (1, 1)),
         ((1, 1), (1, 1), (0, 0), (1, 1)),
         ((7, 7), (1, 1), (3, 3), (1, 1)),        # 49 taps
         ((2, 3), (1, 1), (0, 0), (1, 1)),        # the generic tap form
         ((3, 1), (2, 1), (1, 0), (2, 1)))
CM = ((3, 1), (4, 1), (32, 1), (36, 1), (20, 2), (132, 1))       # partial word, Cout % 4 != 0, word boundaries, ld padding, m > 1
MAPS = ((7, 7), (9, 8), (14, 14), (5, 17))
BATCHES = (1, 3)
HALOS = ((0, 0), (1, 1), (2, 1))
ALPHAS = (1.0, -1.0, 0.0, 0.5)


class Case(dict):
    __getattr__ = dict.__getitem__


def _case(i):
    (C, m), (H, W) = CM[i % len(CM)], MAPS[i % len(MAPS)]
    k, s, p, d = GEOMS[i % len(GEOMS)]
    return Case(i=i, C=C, m=m, H=H, W=W, N=BATCHES[(i // 2) % 2], kernel=k, stride=s, padding=p, dilation=d,
                id=f"C{C}m{m}N{BATCHES[(i // 2) % 2]}-k{k[0]}x{k[1]}-s{s[0]}{s[1]}-p{p[0]}{p[1]}-d{d[0]}-{H}x{W}")


# every geometry twice, with another (C, m), map and batch: every value of every axis occurs, and every (input form, output form)
# pair is walked at every geometry inside each case
CASES = [_case(i) for i in range(2 * len(GEOMS))]


def test_the_case_list_covers_every_axis_value():
    for axis, want in (("kernel", {g[0] for g in GEOMS}), ("N", set(BATCHES))):
        assert {c[axis] for c in CASES} == want
    assert {(c.C, c.m) for c in CASES} == set(CM) and {(c.H, c.W) for c in CASES} == set(MAPS)
    assert {(c.kernel, c.stride, c.padding, c.dilation) for c in CASES} == set(GEOMS)


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


def _sources(dev, x, forms):
    for form in forms:
        yield form, (_planes_of(dev, x) if form == "planes" else _to(dev, x, form))


def _run_sign(dev, c, src, x_shape, w, b, alpha, beta, kind, halo=None, with_bits=False):
    """The planes of one launch as numpy arrays, written between sentinels: bits (halo None), nibble plane, or both."""
    Cout = c.C * c.m
    Ho, Wo = D.out_hw(c.H, c.W, *_geom(c))
    kw = {}
    bufs = []
    if halo is None or with_bits:
        bb, kw["out_sign"] = _guarded_words(dev, c.N * Ho * Wo, P.packed_ld(Cout))
        bufs.append(bb)
    if halo is not None:
        bn, kw["out_nib"] = _guarded_words(dev, c.N * (Ho + 2 * halo[0]) * (Wo + 2 * halo[1]), P.pixel_ld_nib(Cout))
        bufs.append(bn)
    before = _lib.call_counts.get(SIGN, 0)
    out, hw = ops.depthwise_conv2d_sign(src, _to(dev, w).unsqueeze(1), None if b is None else _to(dev, b), _to(dev, alpha), _to(dev, beta),
                                        c.stride, c.padding, c.dilation, kind=kind, shape=x_shape, out_halo=halo, with_bits=with_bits, **kw)
    assert _lib.call_counts[SIGN] == before + 1 and hw == (Ho, Wo)
    assert all(_intact(b_) for b_ in bufs)
    if halo is None:
        assert isinstance(out, ops.BitPlanes) and out.sign is kw["out_sign"] and (out.rows, out.K) == (c.N * Ho * Wo, Cout)
        return out.sign.cpu().numpy()
    if with_bits:
        assert out[0].sign is kw["out_sign"] and out[1].words is kw["out_nib"]
        return out[0].sign.cpu().numpy(), out[1].words.cpu().numpy()
    assert isinstance(out, ops.NibPlanes) and out.words is kw["out_nib"] and out.K == Cout
    return out.words.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _designed(i):
    """+-1 activations, weights in {-1, 0, +1}, integer bias; alpha cycles through {+1, -1, 0, 0.5} and beta = -alpha t with t an
    output the channel really takes, so y alpha + beta is exactly 0 there: ties, which must give bit 0."""
    c = CASES[i]
    Cout = c.C * c.m
    x = D.pm1(1000 + i, (c.N, c.C, c.H, c.W))
    w = D.grid_weights(1100 + i, (Cout,) + c.kernel)
    b = D.small_ints(1200 + i, (Cout,))
    y = D.forward(x, w, b, *_geom(c))
    assert y.dtype == np.float32 and np.array_equal(y, D.forward(x, w, b, *_geom(c), dtype=np.float64))      # exact integers
    r = np.random.RandomState(1300 + i)
    alpha = np.array([ALPHAS[(k + i) % 4] for k in range(Cout)], dtype=np.float32)
    N, _, Ho, Wo = y.shape
    t = y[r.randint(0, N, Cout), np.arange(Cout), r.randint(0, Ho, Cout), r.randint(0, Wo, Cout)]
    beta = (-alpha * t).astype(np.float32)
    neg = P.threshold_bits(y, alpha, beta)
    z = y * alpha[None, :, None, None] + beta[None, :, None, None]
    ties = int(((z == 0) & (alpha != 0)[None, :, None, None]).sum())
    assert ties > 0 and not neg[z == 0].any()
    return Case(x=x, w=w, b=b, y=y, alpha=alpha, beta=beta, neg=neg, ties=ties)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_designed_operands_every_input_and_output_form(dev, i):
    c, r = CASES[i], _designed(i)
    assert r.ties > 0
    want_bits = P.pack_sign(r.neg)
    first = {}
    for form, src in _sources(dev, r.x, ("nchw", "channels_last", "planes")):
        args = (dev, c, src, r.x.shape, r.w, r.b, r.alpha, r.beta, "raw")
        got = _run_sign(*args)
        assert got.dtype == np.int32 and np.array_equal(got, want_bits), (form, "bits")
        first.setdefault("bits", got)
        assert np.array_equal(got, first["bits"])                     # the plane input gives what the fp32 +-1 image gives
        for halo in HALOS:
            got = _run_sign(*args, halo=halo)
            assert np.array_equal(got, P.pack_nib(r.neg, halo)), (form, halo)
    # both planes from one launch
    both = _run_sign(dev, c, _planes_of(dev, r.x), r.x.shape, r.w, r.b, r.alpha, r.beta, "raw", halo=HALOS[i % 3], with_bits=True)
    assert np.array_equal(both[0], want_bits) and np.array_equal(both[1], P.pack_nib(r.neg, HALOS[i % 3]))
    # the weights are fixed points of the ternary quantiser: ``kind`` applies to the taps and changes nothing here
    assert np.array_equal(_run_sign(dev, c, _planes_of(dev, r.x), r.x.shape, r.w, r.b, r.alpha, r.beta, "ternary"), want_bits)
    # planes in, fp32 out: the value itself, in either layout
    for layout in ("nchw", "channels_last"):
        buf, out = _guarded_f32(dev, r.y.shape, layout)
        before = _lib.call_counts.get(F32, 0)
        y = ops.depthwise_conv2d_from_bits(_planes_of(dev, r.x), r.x.shape, _to(dev, r.w).unsqueeze(1), _to(dev, r.b), c.stride, c.padding,
                                           c.dilation, out=out)
        assert y is out and _intact(buf) and _lib.call_counts[F32] == before + 1
        assert np.array_equal(y.cpu().numpy(), r.y), layout
    y = ops.depthwise_conv2d_from_bits(_planes_of(dev, r.x), r.x.shape, _to(dev, r.w).unsqueeze(1), None, c.stride, c.padding, c.dilation)
    assert y.is_contiguous() and np.array_equal(y.cpu().numpy(), D.forward(r.x, r.w, None, *_geom(c)))
    # inside the package: the un-fused pair of launches writes the same sign plane (it needs Cout % 4 == 0)
    if (c.C * c.m) % 4 == 0:
        xt, wt = _to(dev, r.x, "channels_last"), _to(dev, r.w).unsqueeze(1)
        y32 = ops.depthwise_conv2d(xt, wt, _to(dev, r.b), c.stride, c.padding, c.dilation)
        pair = ops.pool_affine_sign_pack(y32, _to(dev, r.alpha), _to(dev, r.beta))[0].sign
        assert np.array_equal(pair.cpu().numpy(), want_bits)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_gaussian_operands_with_device_batchnorm_thresholds(dev, i):
    """Activations over six decades, real-valued weights quantised by the kernel, (alpha, beta) = this device's own eval BatchNorm
    thresholds, with negative and zero BatchNorm weights among the channels."""
    c = CASES[i]
    Cout = c.C * c.m
    kind = D.KINDS[i % 3]
    x = D.gauss6(2000 + i, (c.N, c.C, c.H, c.W))
    w = D.weights(2100 + i, (Cout,) + c.kernel)
    b = D.gauss6(2200 + i, (Cout,)) if i % 2 == 0 else None
    y = D.forward(x, D.quantize(w, kind), b, *_geom(c))
    g = torch.Generator().manual_seed(2300 + i)
    bn = nn.BatchNorm2d(Cout)
    bn.running_mean.copy_(torch.randn(Cout, generator=g))
    bn.running_var.copy_(torch.rand(Cout, generator=g) * 4 + 0.5)
    gamma = torch.rand(Cout, generator=g) + 0.5
    gamma[::3] *= -1
    gamma[1::5] = 0
    bn.weight.data.copy_(gamma)
    bn.bias.data.copy_(torch.randn(Cout, generator=g) * 0.3)
    bn = bn.to(dev).eval()
    for layout in ("nchw", "channels_last"):
        alpha, beta = device_sign_fold(bn, y.shape, layout == "channels_last")
        a, be = alpha.cpu().numpy(), beta.cpu().numpy()
        assert (a == 0).any() or Cout < 2
        assert (a < 0).any() and (a > 0).any() or Cout < 4
        neg = P.threshold_bits(y, a, be)
        src = _to(dev, x, layout)
        assert np.array_equal(_run_sign(dev, c, src, x.shape, w, b, a, be, kind), P.pack_sign(neg)), layout
        halo = HALOS[(i + (layout == "nchw")) % 3]
        assert np.array_equal(_run_sign(dev, c, src, x.shape, w, b, a, be, kind, halo=halo), P.pack_nib(neg, halo)), (layout, halo)


def test_numpy_packers_agree_with_the_device_packers(dev):
    x = D.pm1(7, (2, 36, 3, 5))
    planes, _ = ops.sign_pack(_to(dev, x).permute(0, 2, 3, 1).contiguous())
    assert np.array_equal(planes.sign.cpu().numpy(), P.pack_sign(x < 0))
    pixel = ops.BitPlanes(sign=planes.sign, rows=2 * 3 * 5, K=36)
    for halo in HALOS:
        nib = ops.bits_to_nib_pad(pixel, 2, 3, 5, halo, ld=ops.pixel_ld_nib(36))
        assert np.array_equal(nib.words.cpu().numpy(), P.pack_nib(x < 0, halo))


def test_wrappers_check_their_operands(dev):
    x = _to(dev, D.pm1(1, (1, 8, 5, 5)))
    w = _to(dev, D.grid_weights(2, (8, 1, 3, 3)))
    a = torch.ones(8, device=dev)
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_sign(x, w, None, torch.ones(7, device=dev), a, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_sign(x, w, None, a.cpu(), a, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_sign(x, w, None, None, a, 1, 1, 1)
    pl = _planes_of(dev, D.pm1(1, (1, 8, 5, 5)))
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_sign(pl, w, None, a, a, 1, 1, 1)                        # no logical shape
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_sign(pl, w, None, a, a, 1, 1, 1, shape=(1, 8, 5, 6))
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_sign(x, w, None, a, a, 1, 1, 1, out_halo=(-1, 0))
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_from_bits(pl, (1, 8, 5, 5), _to(dev, D.grid_weights(2, (8, 1, 5, 10))), None, 1, 5, 1)      # 50 taps
    # empty batch: planes of zero rows, nothing launched
    before = _lib.call_counts.get(SIGN, 0)
    out, hw = ops.depthwise_conv2d_sign(x[:0], w, None, a, a, 1, 1, 1)
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


def _stack(dev, seed=5):
    """pw 1x1 -> dw 3x3 -> pw 1x1 -> dw 3x3 stride 2 (ternary, m = 2) -> pw 1x1, a BatchNorm -> Hardtanh -> sign run after each but
    the last: the un-modified modules."""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    seq = nn.Sequential(BinConv2d(16, 32, 1), *_run(32, g),
                        BinConv2d(32, 32, 3, padding=1, groups=32), *_run(32, g),
                        BinConv2d(32, 64, 1), *_run(64, g),
                        TerConv2d(64, 128, 3, stride=2, padding=1, groups=64), *_run(128, g),
                        BinConv2d(128, 32, 1))
    return _ready(seq, dev)


def _ready(seq, dev):
    """Weights spread over [-1.5, 1.5] — the default initialisation lies inside the ternary dead zone, a TerConv2d would multiply
    by zeros — then the device and eval mode (which stores the quantised image)."""
    g = torch.Generator().manual_seed(23)
    for m in seq.modules():
        if isinstance(m, (BinConv2d, TerConv2d)):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * 3 - 1.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g))
    return seq.to(dev).eval()


def _value(t):
    return t.value() if isinstance(t, lazy.LazyActivation) else t


def _delta(after, before, name):
    return after.get(name, 0) - before.get(name, 0)


@pytest.fixture(autouse=True)
def _fresh_stats():
    start = lazy.DEFER_DEPTHWISE
    lazy.STATS.clear()
    yield
    assert lazy.DEFER_DEPTHWISE is start


def test_unmodified_block_stack_runs_as_fused_chains(dev):
    seq, x = _stack(dev), _pm1((3, 16, 12, 12), dev)
    with torch.no_grad(), lazy.depthwise_deferred():
        with lazy.eager():
            e = seq(x)
        assert type(e) is torch.Tensor and e.shape == (3, 32, 6, 6)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        y = seq(x)
        stats, after = dict(lazy.STATS), dict(_lib.call_counts)
        assert isinstance(y, lazy.LazyActivation)
        got = y.value()
    assert torch.equal(got, e)
    # five convs deferred, the four chains between them ran fused, no intermediate activation was computed in fp32
    assert stats.get("deferred") == 5 and stats.get("fused") == 4 and stats.get("materialised", 0) == 0, stats
    assert _delta(after, before, "qt_dwconv2d_f32") == 0 and _delta(after, before, SIGN) == 2
    assert not [k for k in after if k.startswith("qt_pool_affine_sign_pack") and _delta(after, before, k)]
    if _fused._cfg("PAD_PLANES"):       # the depthwise launch wrote its pointwise consumer's nibble plane itself
        assert not [k for k in after if k.startswith("qt_bits_to_nib") and _delta(after, before, k)]


def test_switch_off_is_the_module_by_module_depthwise_path(dev):
    seq, x = _stack(dev), _pm1((3, 16, 12, 12), dev)
    with torch.no_grad():
        with lazy.eager():
            e = seq(x)
        with lazy.depthwise_deferred(False):
            before = dict(_lib.call_counts)
            got = _value(seq(x))
            after = dict(_lib.call_counts)
        with lazy.depthwise_deferred():
            on = _value(seq(x))
    assert torch.equal(got, e) and torch.equal(on, e)
    assert _delta(after, before, "qt_dwconv2d_f32") == 2 and _delta(after, before, SIGN) == 0 and _delta(after, before, F32) == 0


@pytest.mark.parametrize("layout", ("nchw", "channels_last"))
def test_depthwise_first_layer_on_a_real_valued_input_defers_and_fuses(dev, layout):
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    seq = _ready(nn.Sequential(BinConv2d(20, 20, 3, padding=1, groups=20), *_run(20, g), BinConv2d(20, 16, 1)), dev)
    x = torch.randn(2, 20, 9, 8, generator=g).to(dev)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), lazy.depthwise_deferred():
        with lazy.eager():
            e = seq(x)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = _value(seq(x))
        after = dict(_lib.call_counts)
    assert torch.equal(got, e)
    assert lazy.STATS["deferred"] == 2 and lazy.STATS["fused"] == 1, lazy.STATS
    assert _delta(after, before, SIGN) == 1 and _delta(after, before, "qt_dwconv2d_f32") == 0


@pytest.mark.parametrize("where", ("before_bn", "after_sign"))
def test_depthwise_chain_with_a_maxpool_equals_eager(dev, where):
    g = torch.Generator().manual_seed(13)
    torch.manual_seed(13)
    run = _run(40, g)
    mods = [BinConv2d(8, 20, 1), *_run(20, g), TerConv2d(20, 40, 3, padding=1, groups=20)]
    mods += [nn.MaxPool2d(2), *run] if where == "before_bn" else [*run, nn.MaxPool2d(2)]
    seq = _ready(nn.Sequential(*mods, BinConv2d(40, 16, 3, padding=1)), dev)
    x = _pm1((2, 8, 10, 10), dev, 3)
    with torch.no_grad(), lazy.depthwise_deferred():
        with lazy.eager():
            e = seq(x)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = _value(seq(x))
        after = dict(_lib.call_counts)
    assert torch.equal(got, e)
    assert lazy.STATS["fused"] == 2 and _delta(after, before, SIGN) == 1 and _delta(after, before, "qt_dwconv2d_f32") == 0, lazy.STATS


def test_deferred_depthwise_conv_materialises_from_planes(dev):
    g = torch.Generator().manual_seed(17)
    torch.manual_seed(17)
    head = _ready(nn.Sequential(BinConv2d(8, 36, 1), *_run(36, g), TerConv2d(36, 72, 3, stride=2, padding=1, groups=36)), dev)
    tail = nn.Sequential(*_run(72, g)).to(dev).eval()
    x = _pm1((3, 8, 9, 8), dev, 4)
    with torch.no_grad(), lazy.depthwise_deferred():
        with lazy.eager():
            e_conv = head(x)
            e_sign = tail(e_conv)
        before = dict(_lib.call_counts)
        y = head(x)
        assert isinstance(y, lazy.LazyActivation) and isinstance(y._qt.input, _fused.packed.PackedActivation)
        got = y * 1.0                                   # not in the grammar: the conv's own fp32 value, computed from the planes
        after = dict(_lib.call_counts)
        assert type(got) is torch.Tensor and got.is_contiguous() and torch.equal(got, e_conv)
        assert _delta(after, before, F32) == 1 and _delta(after, before, "qt_dwconv2d_f32") == 0
        # read after the sign: conv from the planes, the recorded BatchNorm / Hardtanh / sign replayed
        s = tail(head(x))
        assert isinstance(s, lazy.LazyActivation) and s._qt.signed
        assert torch.equal(s.value(), e_sign)


def test_explicit_fused_form_and_hipgraph_replay(dev):
    seq, x = _stack(dev), _pm1((3, 16, 12, 12), dev)
    seq[0].binary_input = True              # the +-1 hint: nothing asks the device about the input while the graph is captured
    with torch.no_grad(), lazy.depthwise_deferred():
        with lazy.eager():
            e = seq(x)
        fused = fuse_sequential(seq, fuse_conv=True, fold="device")
        assert [type(m) for m in fused] == [FusedConvPoolBnSign, FusedDepthwiseBnSign, FusedConvPoolBnSign, FusedDepthwiseBnSign, BinConv2d]
        before = dict(_lib.call_counts)
        assert torch.equal(_value(fused(x)), e)
        assert _delta(dict(_lib.call_counts), before, SIGN) == 2
        graph = utils.graphed(seq, x)
        assert torch.equal(graph(x), e)
        x2 = _pm1((3, 16, 12, 12), dev, 9)
        with lazy.eager():
            e2 = seq(x2)
        assert torch.equal(graph(x2), e2) and not torch.equal(e, e2)


def test_conv_can_defer_admits_depthwise_only(dev):
    """The gate of lazy.py: ``groups == in_channels`` inside ops.depthwise_applicable under the switch, for a tensor and for the
    shape stand-in of an activation that is not forced yet; every other grouped conv stays declined."""
    dwl = _ready(BinConv2d(8, 16, 3, padding=1, groups=8), dev)
    g2 = _ready(BinConv2d(8, 8, 3, padding=1, groups=2), dev)
    taps50 = _ready(TerConv2d(8, 8, (5, 10), padding=5, groups=8), dev)
    x = _pm1((1, 8, 12, 12), dev)
    with torch.no_grad():
        with lazy.depthwise_deferred():
            assert lazy._conv_can_defer(dwl, x) and lazy._conv_can_defer(dwl, lazy._ShapeOnly((1, 8, 12, 12)))
            assert not lazy._conv_can_defer(dwl, lazy._ShapeOnly((1, 8, 0, 12)))
            assert not lazy._conv_can_defer(g2, x) and not lazy._conv_can_defer(g2, lazy._ShapeOnly((1, 8, 12, 12)))
            assert not lazy._conv_can_defer(taps50, x)
            assert isinstance(dwl(x), lazy.LazyActivation) and type(g2(x)) is torch.Tensor
        with lazy.depthwise_deferred(False):
            assert not lazy._conv_can_defer(dwl, x) and not lazy._conv_can_defer(dwl, lazy._ShapeOnly((1, 8, 12, 12)))
            assert type(dwl(x)) is torch.Tensor


def test_fused_depthwise_block_declines_at_run_time(dev):
    g = torch.Generator().manual_seed(19)
    conv = _ready(BinConv2d(8, 8, 3, padding=1, groups=8), dev)
    blk = FusedDepthwiseBnSign(conv, _run(8, g)[0].to(dev).eval(), fold="device")
    x = _pm1((1, 8, 5, 5), dev)
    act = blk(x)
    assert act.planes is not None and act.shape == (1, 8, 5, 5)
    blk.out_nib_halo = (1, 1)
    nib = blk(act)                          # planes in, the consumer's nibble plane out
    assert nib.planes is None and nib.halo == (1, 1) and nib.nib.words.shape == (49, 4)
    with pytest.raises(ValueError):
        blk(nib)                            # a nibble-only activation: in lazy.py the chain then materialises
    conv.weight.data.mul_(0.3)              # off the quantiser's grid
    conv.reset_quant_cache()
    assert not conv._eval_on_grid()
    with pytest.raises(ValueError):
        blk(x)
