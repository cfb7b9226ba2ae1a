"""Depthwise convs inside the fused inference chain, the host side: the plane entries exist and validate before they launch, the
numpy plane packers of tests/_dw_planes.py hold the documented layouts, ``FusedDepthwiseBnSign`` / ``fuse_sequential`` construct
(and decline) what they should, and the ``lazy.depthwise_deferred`` switch restores itself.  The kernels:
tests/test_gpu_dwconv_chain.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _dw_planes as P
from pytorch_quantize_impls_amd import _lib, lazy, ops
from pytorch_quantize_impls_amd.functions import BinaryConnect
from pytorch_quantize_impls_amd.layers import (BinConv2d, TerConv2d, XNORConv2d, FusedConvPoolBnSign, FusedDepthwiseBnSign,
                                               FusedPoolBnSign, fuse_sequential)

ENTRIES = ("qt_dwconv2d_sign", "qt_dwconv2d_bits_f32")
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
PTR = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it


def test_entries_are_declared_in_the_header_and_bound():
    declared = _lib.header_declared_functions()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def _sign(lib, **kw):
    """C = 40, m = 1: packed_ld(C) = 4 words cover it exactly with ld 4, pixel_ld_nib(C) = 8."""
    a = dict(x=PTR, xp=None, ldx=0, w=PTR, bias=None, alpha=PTR, beta=PTR, sign=PTR, ldb=4, nib=PTR, ldn=8, hy=1, hx=1, N=2, C=40, m=1,
             H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, xs=(1000, 25, 5, 1), kind=0)
    a.update(kw)
    return lib.qt_dwconv2d_sign(a["x"], a["xp"], a["ldx"], a["w"], a["bias"], a["alpha"], a["beta"], a["sign"], a["ldb"], a["nib"],
                                a["ldn"], a["hy"], a["hx"], a["N"], a["C"], a["m"], a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"],
                                a["ph"], a["pw"], a["dh"], a["dw"], *a["xs"], a["kind"], None)


def _f32(lib, **kw):
    a = dict(xp=PTR, ldx=4, w=PTR, bias=None, y=PTR, N=2, C=40, m=1, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1,
             ys=(1000, 25, 5, 1), kind=0)
    a.update(kw)
    return lib.qt_dwconv2d_bits_f32(a["xp"], a["ldx"], a["w"], a["bias"], a["y"], a["N"], a["C"], a["m"], a["H"], a["W"], a["kh"],
                                    a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], *a["ys"], a["kind"], None)


def test_sign_entry_validates_before_it_launches():
    lib = _lib.load()
    plane = dict(x=None, xp=PTR, ldx=4)
    for src in ({}, plane):
        assert _sign(lib, **src, w=None) == INVALID
        assert _sign(lib, **src, alpha=None) == INVALID and _sign(lib, **src, beta=None) == INVALID
        assert _sign(lib, **src, sign=None, nib=None) == INVALID                     # no output plane
        assert _sign(lib, **src, kh=5, kw=10) == UNSUPPORTED                         # 50 taps
        assert _sign(lib, **src, ldn=4) == INVALID                                   # below pixel_ld_nib(40) = 8
        assert _sign(lib, **src, ldb=3) == INVALID
        assert _sign(lib, **src, hy=-1) == INVALID and _sign(lib, **src, hx=-1) == INVALID
        assert _sign(lib, **src, hy=65) == UNSUPPORTED
        assert _sign(lib, **src, kind=3) == INVALID
        assert _sign(lib, **src, alpha=PTR + 2) == ALIGNMENT and _sign(lib, **src, sign=PTR + 1) == ALIGNMENT
        assert _sign(lib, **src, nib=PTR + 4) == ALIGNMENT and _sign(lib, **src, ldn=10) == ALIGNMENT      # 16-byte nibble rows
        assert _sign(lib, **src, N=-1) == INVALID and _sign(lib, **src, m=0) == INVALID
    assert _sign(lib, x=None) == INVALID                                             # neither input form
    assert _sign(lib, xp=PTR, ldx=4) == INVALID                                      # both
    assert _sign(lib, x=PTR + 2) == ALIGNMENT and _sign(lib, **dict(plane, xp=PTR + 2)) == ALIGNMENT
    assert _sign(lib, xs=(1000, 25, 5, 2)) == INVALID                                # not a dense layout
    assert _sign(lib, **dict(plane, ldx=3)) == INVALID                               # below packed_ld(40) = 4
    assert _sign(lib, **dict(plane, ldx=2)) == INVALID                               # ... even where ceil(C / 32) words would fit
    # a plane that is not wanted is not validated: its stride is only looked at with its pointer (a valid call would launch
    # on the stand-in pointer, so the positive side of this is left to the GPU file)
    assert _sign(lib, sign=None, ldb=0, ldn=4) == INVALID and _sign(lib, nib=None, ldn=0, ldb=3) == INVALID
    # empty tensors: nothing to do, whatever the pointers are
    assert _sign(lib, N=0, x=None, w=None, alpha=None, beta=None, sign=None, nib=None) == OK
    assert _sign(lib, C=0, x=None, w=None, sign=None, nib=None) == OK
    assert _sign(lib, N=0, hy=-1) == INVALID                                         # the halo's sign is looked at first


def test_f32_entry_validates_before_it_launches():
    lib = _lib.load()
    assert _f32(lib, xp=None) == INVALID and _f32(lib, w=None) == INVALID and _f32(lib, y=None) == INVALID
    assert _f32(lib, xp=PTR + 2) == ALIGNMENT and _f32(lib, y=PTR + 1) == ALIGNMENT and _f32(lib, bias=PTR + 2) == ALIGNMENT
    assert _f32(lib, kh=5, kw=10) == UNSUPPORTED
    assert _f32(lib, ldx=3) == INVALID
    assert _f32(lib, ys=(1000, 25, 5, 2)) == INVALID
    assert _f32(lib, kind=-1) == INVALID and _f32(lib, sh=0) == INVALID
    assert _f32(lib, kh=7, kw=7, ph=0, pw=0) == INVALID                              # does not fit a 5 x 5 image
    assert _f32(lib, N=0, xp=None, w=None, y=None) == OK and _f32(lib, H=0, xp=None, y=None) == OK


def test_wrappers_reject_host_tensors():
    x, w = torch.randn(1, 4, 5, 5), torch.randn(4, 1, 3, 3)
    a = torch.ones(4)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_sign(x, w, None, a, a, 1, 1, 1)
    planes = ops.BitPlanes(sign=torch.zeros((25, 4), dtype=torch.int32), rows=25, K=4)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_sign(planes, w, None, a, a, 1, 1, 1, shape=(1, 4, 5, 5))
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_from_bits(planes, (1, 4, 5, 5), w, None, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_sign(object(), w, None, a, a, 1, 1, 1)


def test_numpy_plane_packers_on_hand_written_words():
    """The layouts of ops.sign_pack (bit k & 31 of word k >> 5, 1 = negative, pad zero) and ops.bits_to_nib_pad (nibble k & 7 of
    word k >> 3, +1 = 0x2, -1 = 0xA, channels past C and border pixels zero), word by word."""
    assert [P.packed_ld(k) for k in (1, 32, 128, 129, 257)] == [ops.packed_ld(k) for k in (1, 32, 128, 129, 257)] == [4, 4, 4, 8, 12]
    assert [P.pixel_ld_nib(k) for k in (1, 32, 33, 132)] == [ops.pixel_ld_nib(k) for k in (1, 32, 33, 132)] == [4, 4, 8, 20]
    # one image, 1 x 2 pixels, 3 channels: pixel 0 = (-, +, -), pixel 1 = (+, +, -)
    neg = np.zeros((1, 3, 1, 2), dtype=bool)
    neg[0, :, 0, 0] = (True, False, True)
    neg[0, :, 0, 1] = (False, False, True)
    s = P.pack_sign(neg)
    assert s.dtype == np.int32 and s.tolist() == [[0b101, 0, 0, 0], [0b100, 0, 0, 0]]
    n0 = P.pack_nib(neg)
    assert n0.dtype == np.int32 and n0.tolist() == [[0xA2A, 0, 0, 0], [0xA22, 0, 0, 0]]
    n1 = P.pack_nib(neg, halo=(1, 2))              # [1 + 2][2 + 4] pixels, the image at row 1, columns 2..3
    assert n1.shape == (18, 4) and n1[6 + 2].tolist() == [0xA2A, 0, 0, 0] and n1[6 + 3].tolist() == [0xA22, 0, 0, 0]
    assert int(np.count_nonzero(n1)) == 2
    # channel 33 is bit 1 of word 1 / nibble 1 of word 4; channel 31 the sign bit of word 0 (int32: negative)
    neg = np.zeros((1, 34, 1, 1), dtype=bool)
    neg[0, 33] = neg[0, 31] = True
    assert P.pack_sign(neg).view(np.uint32).tolist() == [[0x80000000, 0b10, 0, 0]]
    nb = P.pack_nib(neg).view(np.uint32)
    assert nb.shape == (1, 8) and nb[0].tolist() == [0x22222222, 0x22222222, 0x22222222, 0xA2222222, 0xA2, 0, 0, 0]
    # the threshold bit: two float32 roundings, a tie is not negative
    y = np.array([1.0, -1.0, 3.0, 0.0], dtype=np.float32).reshape(1, 1, 2, 2)
    assert P.threshold_bits(y, [0.5], [-0.5]).ravel().tolist() == [False, True, False, True]
    assert P.threshold_bits(y, [-1.0], [1.0]).ravel().tolist() == [False, False, True, False]
    big = np.full((1, 1, 1, 1), 16777216.0, dtype=np.float32)                   # 2^24 * 1 - (2^24 + 1 -> 2^24): a tie in float32
    assert not P.threshold_bits(big, [1.0], [-16777217.0]).any()


def _bn(c):
    return nn.BatchNorm2d(c)


def test_fused_depthwise_block_declines_what_it_cannot_run():
    ok = FusedDepthwiseBnSign(BinConv2d(8, 8, 3, padding=1, groups=8), _bn(8))
    assert ok.out_nib_halo is None and ok.fold == "reference" and isinstance(ok._pool, FusedPoolBnSign)
    assert FusedDepthwiseBnSign(TerConv2d(8, 16, 3, stride=2, padding=1, groups=8), _bn(16), nn.MaxPool2d(2), fold="device").fold == "device"
    for conv, bn in ((BinConv2d(8, 8, 3, padding=1, groups=2), _bn(8)),
                     (BinConv2d(8, 8, 3, padding=1), _bn(8)),
                     (BinConv2d(1, 1, 3, padding=1, groups=1), _bn(1)),
                     (XNORConv2d(8, 8, 3, padding=1, groups=8), _bn(8)),
                     (BinConv2d(8, 8, 3, padding="same", groups=8), _bn(8)),
                     (TerConv2d(8, 8, 3, padding=1, groups=8, ), _bn(16)),
                     (BinConv2d(8, 8, (5, 10), padding=5, groups=8), _bn(8)),                      # 50 taps
                     (nn.Conv2d(8, 8, 3, padding=1, groups=8), _bn(8))):
        with pytest.raises(ValueError):
            FusedDepthwiseBnSign(conv, bn)
    with pytest.raises(ValueError):
        FusedDepthwiseBnSign(BinConv2d(8, 8, 3, padding=1, groups=8), nn.BatchNorm1d(8))
    with pytest.raises(ValueError):
        FusedDepthwiseBnSign(BinConv2d(8, 8, 3, padding=1, groups=8), _bn(8), nn.MaxPool2d((3, 2)))
    with pytest.raises(RuntimeError):
        ok(torch.randn(1, 8, 5, 5))                                                  # training mode
    ok.eval()
    with pytest.raises(TypeError):
        ok(torch.randn(1, 8, 5, 5))                                                  # a host tensor
    ok.refold()


def test_fuse_sequential_builds_the_depthwise_block():
    def run(c):
        return [_bn(c), nn.Hardtanh(), BinaryConnect()]
    seq = nn.Sequential(BinConv2d(16, 32, 1), *run(32),
                        BinConv2d(32, 32, 3, padding=1, groups=32), *run(32),
                        BinConv2d(32, 64, 3, padding=1), *run(64),
                        TerConv2d(64, 128, 3, stride=2, padding=1, groups=64), nn.MaxPool2d(2), *run(128),
                        BinConv2d(128, 128, 3, padding=1, groups=2), *run(128),
                        BinConv2d(128, 32, 1))
    fused = fuse_sequential(seq, fuse_conv=True, fold="device")
    kinds = [type(m) for m in fused]
    assert kinds == [FusedConvPoolBnSign, FusedDepthwiseBnSign, FusedConvPoolBnSign, FusedDepthwiseBnSign, BinConv2d, FusedPoolBnSign,
                     BinConv2d]
    assert fused[1].conv is seq[4] and fused[1].bn is seq[5] and fused[3].conv is seq[12] and fused[3]._pool.pool_k == 2
    assert all(m.fold == "device" for m in fused if not isinstance(m, BinConv2d))
    # producers: the block in front of a depthwise block stays on bit planes; a depthwise block writes the next fused conv's
    # nibble plane with that conv's padding as the halo; in front of an un-fused conv it hands over bit planes
    assert fused[0].out_nib_halo is None and fused[1].out_nib_halo == (1, 1) and fused[2].out_nib_halo is None
    assert fused[3].out_nib_halo is None
    # without fuse_conv nothing changes for the convs
    plain = fuse_sequential(seq, fuse_conv=False)
    assert plain[1].__class__ is FusedPoolBnSign and plain[2] is seq[4]


def test_depthwise_deferred_restores_the_previous_setting():
    start = lazy.DEFER_DEPTHWISE
    with lazy.depthwise_deferred():
        assert lazy.DEFER_DEPTHWISE is True
        with lazy.depthwise_deferred(False):
            assert lazy.DEFER_DEPTHWISE is False
        assert lazy.DEFER_DEPTHWISE is True
    assert lazy.DEFER_DEPTHWISE is start
    with pytest.raises(KeyError):
        with lazy.depthwise_deferred(not start):
            assert lazy.DEFER_DEPTHWISE is (not start)
            raise KeyError("x")
    assert lazy.DEFER_DEPTHWISE is start


def test_host_depthwise_layers_never_defer():
    """On the host nothing defers, whatever the switch says: the layer keeps the torch expression."""
    dwl = BinConv2d(8, 8, 3, padding=1, groups=8).eval()
    x = torch.randn(1, 8, 5, 5)
    for on in (True, False):
        with torch.no_grad(), lazy.depthwise_deferred(on):
            assert not lazy._conv_can_defer(dwl, x)
            assert not lazy._conv_can_defer(dwl, lazy._ShapeOnly((1, 8, 5, 5)))
            y = dwl(x)
        assert type(y) is torch.Tensor and torch.equal(y, torch.nn.functional.conv2d(x, dwl.weight, dwl.bias, 1, 1, 1, 8))
