"""Grouped convs inside the fused inference chain, the host side: the exactness argument of the design restated with numpy, the plane
entries validating before they launch, what ``FusedGroupedBnSign`` / ``fuse_sequential`` / ``link_nib_planes`` construct and decline,
``ops.grouped_planes_applicable`` and the ``lazy.grouped_deferred`` switch.  The kernel: tests/test_gpu_gconv_chain.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _dw_planes as P
import _gconv_exact as X
from pytorch_quantize_impls_amd import _lib, lazy, ops
from pytorch_quantize_impls_amd.functions import BinaryConnect, _fused
from pytorch_quantize_impls_amd.layers import (BinConv2d, TerConv2d, XNORConv2d, FusedConvPoolBnSign, FusedDepthwiseBnSign,
                                               FusedGroupedBnSign, FusedPoolBnSign, PackedMaxPool, fuse_sequential)
from pytorch_quantize_impls_amd.layers.fused import link_nib_planes

ENTRIES = ("qt_gconv2d_sign", "qt_gconv2d_bits_f32")
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
PTR = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it

# (cin_g, kernel, stride, padding, dilation): every (cin_g, taps) class the GPU file walks
CLASSES = [(ci, k, s, p, d) for ci in (2, 4, 8)
           for k, s, p, d in (((3, 3), (1, 1), (1, 1), (1, 1)), ((3, 3), (2, 2), (1, 1), (1, 1)), ((5, 5), (1, 1), (2, 2), (1, 1)),
                              ((1, 1), (1, 1), (0, 0), (1, 1)), ((7, 7), (1, 1), (3, 3), (1, 1)), ((2, 3), (1, 1), (0, 0), (1, 1)),
                              ((3, 1), (2, 1), (1, 0), (2, 1)))]


# ---- exactness of the design ---------------------------------------------------------------------------------------------------------

def _int_sum(x, w, G, kernel, stride, padding, dilation):
    """The integer S of the contract: per tap popc(nz) - 2 popc((x_field ^ neg) & nz), from boolean arrays, in int64."""
    N, C, H, W = x.shape
    Cout, cin_g = w.shape[:2]
    cout_g = Cout // G
    Ho, Wo = X.out_hw(H, W, kernel, stride, padding, dilation)
    xneg = x < 0
    nz, wneg = (w != 0).reshape(Cout, cin_g, -1), (w < 0).reshape(Cout, cin_g, -1)
    first = (np.arange(Cout) // cout_g) * cin_g
    S = np.zeros((N, Cout, Ho, Wo), dtype=np.int64)
    for t, ho, hi, wo, wi in X._taps(H, W, Ho, Wo, kernel, stride, padding, dilation):
        for ci in range(cin_g):
            field = xneg[:, first + ci][:, :, hi, wi]
            m, ng = nz[None, :, ci, t, None, None], wneg[None, :, ci, t, None, None]
            S[:, :, ho, wo] += m.astype(np.int64) - 2 * ((field ^ ng) & m).astype(np.int64)
    return S


@pytest.mark.parametrize("cin_g,kernel,stride,padding,dilation", CLASSES,
                         ids=[f"i{c[0]}-k{c[1][0]}x{c[1][1]}-s{c[2][0]}{c[2][1]}-d{c[4][0]}" for c in CLASSES])
def test_pinned_fp32_forward_equals_the_integer_sum_plus_bias(cin_g, kernel, stride, padding, dilation):
    """On +-1 images and weights in {-1, 0, +1} the pinned fp32 order of qt_gconv2d_f32 (tests/_gconv_exact.py) gives exactly
    float32(S) + float32(bias), rounded once, with S the XOR / AND / popcount sum of the plane kernel's contract — bias non-integer."""
    G, cout_g, seed = 5, 3, 100 * cin_g + kernel[0] * 10 + kernel[1]
    x = X.pm1(seed, (2, G * cin_g, 9, 8))
    w = X.grid_weights(seed + 1, (G * cout_g, cin_g) + kernel)
    assert (w == 0).any() and (w < 0).any() and (w > 0).any()
    b = (X.small_ints(seed + 2, (G * cout_g,)) + np.float32(0.3)).astype(np.float32) * np.float32(1.7)
    assert not np.array_equal(b, np.rint(b))
    S = _int_sum(x, w, G, kernel, stride, padding, dilation)
    assert np.abs(S).max() <= cin_g * kernel[0] * kernel[1] <= 8 * 49
    y = X.forward(x, w, b, G, kernel, stride, padding, dilation)
    want = S.astype(np.float32) + b[None, :, None, None]
    assert y.dtype == want.dtype == np.float32 and np.array_equal(y, want)
    y0 = X.forward(x, w, None, G, kernel, stride, padding, dilation)
    assert np.array_equal(y0, S.astype(np.float32)) and not np.signbit(y0[y0 == 0]).any()            # a zero sum is +0
    # the extremes: all-(+1) weights on all-(+1) / all-(-1) images count the taps inside the image
    # (9 x 8 holds every kernel of the list whole, so the largest magnitude is cin_g * taps; the border outputs count fewer)
    ones = np.ones_like(w)
    for sgn in (1, -1):
        xe = np.full_like(x, sgn)
        Se = _int_sum(xe, ones, G, kernel, stride, padding, dilation)
        assert (sgn * Se).max() == cin_g * kernel[0] * kernel[1] and (sgn * Se).min() >= cin_g
        assert (padding == (0, 0)) == ((sgn * Se).min() == cin_g * kernel[0] * kernel[1])
        assert np.array_equal(X.forward(xe, ones, None, G, kernel, stride, padding, dilation), Se.astype(np.float32))


def test_threshold_bit_ties_negative_and_zero_alpha():
    """bit = [fl(fl(y alpha) + beta) < 0]: a tie gives 0, a negative alpha turns the comparison, alpha = 0 leaves the sign of beta
    (-0 and NaN included: both give 0)."""
    y = np.array([3.0, -3.0, 0.0, 5.5], dtype=np.float32).reshape(1, 1, 2, 2)
    assert P.threshold_bits(y, [1.0], [-3.0]).ravel().tolist() == [False, True, True, False]            # y == 3: the tie
    assert P.threshold_bits(y, [-1.0], [3.0]).ravel().tolist() == [False, False, False, True]           # y == 3: the tie, turned
    assert P.threshold_bits(y, [0.5], [-2.75]).ravel().tolist() == [True, True, True, False]            # y == 5.5: the tie
    assert not P.threshold_bits(y, [0.0], [0.0]).any() and not P.threshold_bits(y, [0.0], [-0.0]).any()
    assert P.threshold_bits(y, [0.0], [-1.0]).all() and not P.threshold_bits(y, [0.0], [1.0]).any()
    assert not P.threshold_bits(y, [1.0], [np.nan]).any()


# ---- validation through the library, nothing enqueued --------------------------------------------------------------------------------

def test_entries_are_declared_in_the_header_and_bound():
    declared = _lib.header_declared_functions()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def _sign(lib, **kw):
    """G = 10 groups of 4 -> 40 input and (cout_g = 4) 40 output channels: packed_ld = 4, pixel_ld_nib = 8."""
    a = dict(xp=PTR, ldx=4, w=PTR, bias=None, alpha=PTR, beta=PTR, sign=PTR, ldb=4, nib=PTR, ldn=8, hy=1, hx=1, N=2, G=10, ci=4, co=4,
             H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, kind=0)
    a.update(kw)
    return lib.qt_gconv2d_sign(a["xp"], a["ldx"], a["w"], a["bias"], a["alpha"], a["beta"], a["sign"], a["ldb"], a["nib"], a["ldn"],
                               a["hy"], a["hx"], a["N"], a["G"], a["ci"], a["co"], a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"],
                               a["ph"], a["pw"], a["dh"], a["dw"], a["kind"], None)


def _f32(lib, **kw):
    a = dict(xp=PTR, ldx=4, w=PTR, bias=None, y=PTR, N=2, G=10, ci=4, co=4, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1,
             ys=(1000, 25, 5, 1), kind=0)
    a.update(kw)
    return lib.qt_gconv2d_bits_f32(a["xp"], a["ldx"], a["w"], a["bias"], a["y"], a["N"], a["G"], a["ci"], a["co"], a["H"], a["W"],
                                   a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], *a["ys"], a["kind"], None)


def test_sign_entry_validates_before_it_launches():
    lib = _lib.load()
    # 1. the halo's sign, then the grouped entries' first step
    assert _sign(lib, hy=-1) == INVALID and _sign(lib, hx=-1) == INVALID
    assert _sign(lib, N=0, hy=-1) == INVALID                                           # looked at before the empty problem
    assert _sign(lib, N=-1) == INVALID and _sign(lib, ci=0) == INVALID and _sign(lib, co=0) == INVALID and _sign(lib, sh=0) == INVALID
    assert _sign(lib, kh=5, kw=10) == UNSUPPORTED                                      # 50 taps
    assert _sign(lib, ci=3, hy=-1) == INVALID                                          # ... before the channel count
    # 2. the shape limits: 2, 4 or 8 input channels per group, before the pointers and before the empty problem
    for ci in (1, 3, 6, 16):
        assert _sign(lib, ci=ci, ldx=8) == UNSUPPORTED, ci
        assert _sign(lib, ci=ci, ldx=8, w=None, alpha=None) == UNSUPPORTED
        assert _sign(lib, ci=ci, N=0) == UNSUPPORTED
    for ci in (2, 8):
        assert _sign(lib, ci=ci, xp=None) == INVALID                                   # admitted: the next check answers
    assert _sign(lib, kh=7, kw=7, ph=0, pw=0) == INVALID                               # does not fit a 5 x 5 image
    # 3. empty tensors: nothing to do, whatever the pointers are
    assert _sign(lib, N=0, xp=None, w=None, alpha=None, beta=None, sign=None, nib=None) == OK
    assert _sign(lib, G=0, xp=None, w=None, sign=None, nib=None) == OK and _sign(lib, H=0, hy=65) == OK
    # 4. the halo's size
    assert _sign(lib, hy=65) == UNSUPPORTED and _sign(lib, hx=65, w=None) == UNSUPPORTED
    assert _sign(lib, hy=64, w=None) == INVALID
    # 5. invalid arguments, then alignment
    assert _sign(lib, kind=3) == INVALID and _sign(lib, kind=-1) == INVALID
    assert _sign(lib, xp=None) == INVALID and _sign(lib, w=None) == INVALID
    assert _sign(lib, alpha=None) == INVALID and _sign(lib, beta=None) == INVALID
    assert _sign(lib, sign=None, nib=None) == INVALID                                  # no output plane
    assert _sign(lib, ldb=3) == INVALID and _sign(lib, ldn=4) == INVALID               # below packed_ld(40) = 4 / pixel_ld_nib(40) = 8
    assert _sign(lib, ldx=3) == INVALID and _sign(lib, ldx=2) == INVALID               # below packed_ld(40), even where 2 words would hold it
    assert _sign(lib, G=17, ci=8, ldn=12, ldx=4) == INVALID and _sign(lib, G=17, ci=8, ldn=12, ldx=7) == INVALID    # 136 channels: 5 words -> ld 8
    assert _sign(lib, co=12, ldn=12) == INVALID                                        # 120 output channels: 15 nibble words -> ldn 16
    assert _sign(lib, ldx=3, xp=PTR + 2) == INVALID                                    # invalid argument before alignment
    assert _sign(lib, xp=PTR + 2) == ALIGNMENT and _sign(lib, w=PTR + 1) == ALIGNMENT and _sign(lib, bias=PTR + 2) == ALIGNMENT
    assert _sign(lib, alpha=PTR + 2) == ALIGNMENT and _sign(lib, sign=PTR + 1) == ALIGNMENT
    assert _sign(lib, nib=PTR + 4) == ALIGNMENT and _sign(lib, ldn=10) == ALIGNMENT    # 16-byte nibble rows
    # a plane that is not wanted is not validated
    assert _sign(lib, sign=None, ldb=0, ldn=4) == INVALID and _sign(lib, nib=None, ldn=0, ldb=3) == INVALID


def test_f32_entry_validates_before_it_launches():
    lib = _lib.load()
    assert _f32(lib, xp=None) == INVALID and _f32(lib, w=None) == INVALID and _f32(lib, y=None) == INVALID
    assert _f32(lib, xp=PTR + 2) == ALIGNMENT and _f32(lib, y=PTR + 1) == ALIGNMENT and _f32(lib, bias=PTR + 2) == ALIGNMENT
    assert _f32(lib, kh=5, kw=10) == UNSUPPORTED
    for ci in (1, 3, 6, 16):
        assert _f32(lib, ci=ci, ldx=8) == UNSUPPORTED and _f32(lib, ci=ci, y=None) == UNSUPPORTED
    assert _f32(lib, ldx=3) == INVALID
    assert _f32(lib, G=17, ci=8, ldx=4, ys=(17 * 4 * 25, 25, 5, 1)) == INVALID          # 136 channels need ld 8
    assert _f32(lib, ys=(1000, 25, 5, 2)) == INVALID and _f32(lib, ys=(1000, 1, 200, 41)) == INVALID    # neither dense layout
    assert _f32(lib, kind=-1) == INVALID and _f32(lib, sh=0) == INVALID
    assert _f32(lib, kh=7, kw=7, ph=0, pw=0) == INVALID
    assert _f32(lib, N=0, xp=None, w=None, y=None) == OK and _f32(lib, H=0, xp=None, y=None) == OK


# ---- ops -------------------------------------------------------------------------------------------------------------------------------

def test_grouped_planes_applicable_table():
    f = ops.grouped_planes_applicable
    x = (2, 32, 9, 9)
    for cin_g, want in ((1, False), (2, True), (3, False), (4, True), (6, False), (8, True), (16, False), (32, False)):
        G = 96 // cin_g if cin_g in (3, 6) else 32 // cin_g
        xs = (2, G * cin_g, 9, 9)
        assert ops.grouped_applicable(xs, (2 * G, cin_g, 3, 3), 1, 1, 1, G)
        assert f(xs, (2 * G, cin_g, 3, 3), 1, 1, 1, G) is want, cin_g
    assert f(x, (8, 4, 3, 3), 1, 1, 1, 8) and f(x, (40, 4, 7, 7), 1, 3, 1, 8) and f(x, (8, 4, 1, 1), (2, 1), 0, 1, 8)
    assert f(x, (16, 2, 3, 3), 1, 1, 1, 16)                                       # the predicate knows no minimum of groups ...
    assert f((2, 4, 9, 9), (2, 2, 3, 3), 1, 1, 1, 2)                              # ... the routes add GROUPED_MIN_GROUPS
    assert not f(x, (8, 4, 5, 10), 1, 5, 1, 8)                                    # 50 taps
    assert not f(x, (8, 4, 3, 3), 1, "same", 1, 8) and not f(x, (8, 4, 3, 3), 1, 1, 1, 4)      # groups do not match the channels
    assert not f((2, 32, 0, 9), (8, 4, 3, 3), 1, 1, 1, 8) and not f((2, 32, 2, 2), (8, 4, 3, 3), 1, 0, 1, 8)
    assert not f((32, 9, 9), (8, 4, 3, 3), 1, 1, 1, 8) and not f(x, (9, 4, 3, 3), 1, 1, 1, 8)
    assert ops.GC_PLANE_CIN_G == (2, 4, 8)


def test_wrappers_reject_host_tensors_and_fp32_inputs():
    w = torch.randn(8, 4, 3, 3)
    a = torch.ones(8)
    planes = ops.BitPlanes(sign=torch.zeros((25, 4), dtype=torch.int32), rows=25, K=16)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_sign(planes, w, None, a, a, 1, 1, 1, 4, shape=(1, 16, 5, 5))
    with pytest.raises(TypeError):
        ops.grouped_conv2d_from_bits(planes, (1, 16, 5, 5), w, None, 1, 1, 1, 4)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_sign(torch.randn(1, 16, 5, 5), w, None, a, a, 1, 1, 1, 4)          # the fp32 input form is not built


# ---- layers.fused ----------------------------------------------------------------------------------------------------------------------

def _bn(c):
    return nn.BatchNorm2d(c)


def _reflecting(conv):
    conv.padding_mode = "reflect"
    return conv


def test_fused_grouped_block_accepts_and_declines():
    assert _fused.GROUPED_MIN_GROUPS == 4
    ok = FusedGroupedBnSign(BinConv2d(32, 32, 3, padding=1, groups=8), _bn(32))
    assert ok.out_nib_halo is None and ok.fold == "reference" and isinstance(ok._pool, FusedPoolBnSign) and not ok.flatten_hwc
    assert FusedGroupedBnSign(TerConv2d(32, 48, 3, stride=2, padding=1, groups=16), _bn(48), nn.MaxPool2d(2), fold="device").fold == "device"
    assert FusedGroupedBnSign(BinConv2d(32, 4, 1, groups=4), _bn(4), flatten_hwc=True).flatten_hwc                # cin_g 8, cout_g 1
    assert FusedGroupedBnSign(BinConv2d(32, 32, 7, padding=3, groups=4), _bn(32))._pool.pool_k == 1            # 49 taps, K = 392
    for conv, bn in ((BinConv2d(8, 8, 3, padding=1, groups=2), _bn(8)),                                # fewer than GROUPED_MIN_GROUPS
                     (BinConv2d(12, 12, 3, padding=1, groups=3), _bn(12)),
                     (BinConv2d(12, 12, 3, padding=1, groups=4), _bn(12)),                             # cin_g 3
                     (BinConv2d(24, 24, 3, padding=1, groups=4), _bn(24)),                             # cin_g 6
                     (BinConv2d(64, 64, 3, padding=1, groups=4), _bn(64)),                             # cin_g 16
                     (BinConv2d(8, 8, 3, padding=1, groups=8), _bn(8)),                                # depthwise
                     (BinConv2d(8, 8, 3, padding=1), _bn(8)),                                          # ungrouped
                     (XNORConv2d(32, 32, 3, padding=1, groups=8), _bn(32)),
                     (_reflecting(BinConv2d(32, 32, 3, padding=1, groups=8)), _bn(32)),                # a non-zero padding mode
                     (BinConv2d(32, 32, 3, padding="same", groups=8), _bn(32)),
                     (TerConv2d(32, 32, 3, padding=1, groups=8), _bn(16)),
                     (BinConv2d(32, 32, (5, 10), padding=5, groups=8), _bn(32)),                       # 50 taps
                     (nn.Conv2d(32, 32, 3, padding=1, groups=8), _bn(32))):
        with pytest.raises(ValueError):
            FusedGroupedBnSign(conv, bn)
    with pytest.raises(ValueError):
        FusedGroupedBnSign(BinConv2d(32, 32, 3, padding=1, groups=8), nn.BatchNorm1d(32))
    with pytest.raises(ValueError):
        FusedGroupedBnSign(BinConv2d(32, 32, 3, padding=1, groups=8), _bn(32), nn.MaxPool2d((3, 2)))
    with pytest.raises(RuntimeError):
        ok(torch.randn(1, 32, 5, 5))                                                   # training mode
    ok.eval()
    with pytest.raises(TypeError):
        ok(torch.randn(1, 32, 5, 5))                                                   # an fp32 tensor: that form is not built
    ok.refold()


def _host_act(shape, nib=False):
    N, C, H, W = shape
    if nib:
        words = torch.zeros((N * H * W, ops.pixel_ld_nib(C)), dtype=torch.int32)
        return _fused.packed.PackedActivation(None, shape, nib=ops.NibPlanes(words=words, rows=N * H * W, K=C), halo=(0, 0))
    sign = torch.zeros((N * H * W, ops.packed_ld(C)), dtype=torch.int32)
    return _fused.packed.PackedActivation(ops.BitPlanes(sign=sign, rows=N * H * W, K=C), shape)


def test_fused_grouped_block_declines_at_run_time_with_value_errors():
    """What makes a deferred chain materialise: each raises ValueError before anything is launched."""
    conv = BinConv2d(32, 32, 3, padding=1, groups=8)
    blk = FusedGroupedBnSign(conv, _bn(32)).eval()
    with pytest.raises(ValueError, match="bit planes"):
        blk(_host_act((1, 32, 5, 5), nib=True))                                        # a nibble-only input
    with pytest.raises(ValueError, match="input"):
        blk(_host_act((1, 64, 5, 5)))                                                  # a shape outside the limits: the channels
    with pytest.raises(ValueError, match="input"):
        blk(_host_act((1, 32, 0, 5)))
    # (an off-grid eval weight is looked at on the device only: tests/test_gpu_gconv_chain.py)


def test_fuse_sequential_builds_the_grouped_block_behind_a_plane_producer_only():
    def run(c):
        return [_bn(c), nn.Hardtanh(), BinaryConnect()]
    seq = nn.Sequential(BinConv2d(32, 32, 3, padding=1, groups=8), *run(32),                             # 0: at the head: stays
                        BinConv2d(32, 64, 1), *run(64),                                                  # 4
                        BinConv2d(64, 64, 3, padding=1, groups=16), *run(64),                            # 8: behind a fused conv
                        TerConv2d(64, 128, 3, stride=2, padding=1, groups=8), nn.MaxPool2d(2), *run(128),   # 12: behind a grouped block
                        BinConv2d(128, 128, 3, padding=1), *run(128),                                    # 17
                        BinConv2d(128, 128, 3, padding=1, groups=2), *run(128),                          # 21: two groups: stays
                        BinConv2d(128, 128, 3, padding=1, groups=32), *run(128),                         # 25: behind a FusedPoolBnSign: stays
                        BinConv2d(128, 32, 1))
    fused = fuse_sequential(seq, fuse_conv=True, fold="device")
    assert [type(m) for m in fused] == [BinConv2d, FusedPoolBnSign, FusedConvPoolBnSign, FusedGroupedBnSign, FusedGroupedBnSign,
                                        FusedConvPoolBnSign, BinConv2d, FusedPoolBnSign, BinConv2d, FusedPoolBnSign, BinConv2d]
    assert fused[0] is seq[0] and fused[3].conv is seq[8] and fused[3].bn is seq[9] and fused[4].conv is seq[12]
    assert fused[4]._pool.pool_k == 2 and fused[6] is seq[21] and fused[8] is seq[25]
    assert all(m.fold == "device" for m in fused if not isinstance(m, BinConv2d))
    # link_nib_planes: the producer in front of a grouped block stays on bit planes; a grouped block writes the next fused conv's
    # nibble plane with that conv's padding as the halo, and bit planes in front of anything else
    assert fused[2].out_nib_halo is None and fused[3].out_nib_halo is None and fused[4].out_nib_halo == (1, 1)
    assert fused[5].out_nib_halo is None
    # behind a PackedMaxPool and behind a depthwise block
    seq2 = nn.Sequential(BinConv2d(16, 32, 3, padding=1), *run(32), nn.MaxPool2d(2),
                         BinConv2d(32, 32, 3, padding=1, groups=4), *run(32),
                         BinConv2d(32, 32, 3, padding=1, groups=32), *run(32),
                         BinConv2d(32, 32, 1, groups=16), *run(32), BinConv2d(32, 8, 3, padding=2))
    fused2 = fuse_sequential(seq2, fuse_conv=True, packed_pool=True)
    assert [type(m) for m in fused2] == [FusedConvPoolBnSign, PackedMaxPool, FusedGroupedBnSign, FusedDepthwiseBnSign, FusedGroupedBnSign,
                                         BinConv2d]
    assert [m.out_nib_halo for m in fused2[:5]] == [None] * 5
    link_nib_planes([fused2[4], FusedConvPoolBnSign(seq2[17], _bn(8))])
    assert fused2[4].out_nib_halo == (2, 2)
    # without fuse_conv nothing changes for the convs
    plain = fuse_sequential(seq, fuse_conv=False)
    assert plain[4] is seq[8] and type(plain[5]) is FusedPoolBnSign


# ---- lazy ------------------------------------------------------------------------------------------------------------------------------

def test_grouped_deferred_restores_the_previous_setting():
    start = lazy.DEFER_GROUPED
    with lazy.grouped_deferred():
        assert lazy.DEFER_GROUPED is True
        with lazy.grouped_deferred(False):
            assert lazy.DEFER_GROUPED is False
        assert lazy.DEFER_GROUPED is True
    assert lazy.DEFER_GROUPED is start
    with pytest.raises(KeyError):
        with lazy.grouped_deferred(not start):
            assert lazy.DEFER_GROUPED is (not start)
            raise KeyError("x")
    assert lazy.DEFER_GROUPED is start


def test_host_grouped_layers_never_defer():
    """On the host nothing defers, whatever the switch says: the layer keeps the torch expression."""
    gl = BinConv2d(32, 32, 3, padding=1, groups=8).eval()
    x = torch.randn(1, 32, 5, 5)
    for on in (True, False):
        with torch.no_grad(), lazy.grouped_deferred(on):
            assert not lazy._conv_can_defer(gl, x)
            assert not lazy._conv_can_defer(gl, lazy._ShapeOnly((1, 32, 5, 5)))
            y = gl(x)
        assert type(y) is torch.Tensor and torch.equal(y, torch.nn.functional.conv2d(x, gl.weight, gl.bias, 1, 1, 1, 8))
