"""Grouped DorefaConv2d inside the fused int8 code chain, the host side: the code-plane entries exist and validate before they launch,
``ops.grouped_codes_applicable`` on its boundary shapes, the wrappers reject host tensors, ``FusedGroupedDorefaBnQuant`` declines what
it cannot run, ``lazy.grouped_deferred`` restores both switches, host layers never defer, and the reference of tests/_gconv_codes.py
is pinned on hand-computed outputs, equals the depthwise reference at one channel per group and holds no sensitive element for any
case of the GPU list.  The kernels: tests/test_gpu_gconv_codes.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _codes_exact as C
import _dw_codes as D
import _gconv_codes as R
from pytorch_quantize_impls_amd import _lib, lazy, ops, packed
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import (BinConv2d, DorefaConv2d, FusedDepthwiseDorefaBnQuant, FusedDorefaConvBnQuant,
                                               FusedGroupedDorefaBnQuant)

ENTRIES = ("qt_gconv2d_codes", "qt_gconv2d_codes_f32")
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
PTR = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it


def test_entries_are_declared_in_the_header_and_bound():
    declared = _lib.header_declared_functions()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the argument lists of the depthwise code entries with (G, cin_g, cout_g) in place of (C, m)
    for name, dw in zip(ENTRIES, ("qt_dwconv2d_codes", "qt_dwconv2d_codes_f32")):
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[dw][1]) + 1


def _codes(lib, **kw):
    """G = 10 groups of 4 -> 40 input and (cout_g = 4) 40 output channels: 48-byte rows on both sides."""
    a = dict(x=PTR, ldx=48, ihy=1, ihx=1, inv_n=1.0 / 15, w=PTR, bias=None, alpha=PTR, beta=PTR, stats=None, relu=1, bits=4, codes=PTR,
             ldc=48, ohy=1, ohx=1, flag=PTR, N=2, G=10, ci=4, co=4, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)
    a.update(kw)
    return lib.qt_gconv2d_codes(a["x"], a["ldx"], a["ihy"], a["ihx"], a["inv_n"], a["w"], a["bias"], a["alpha"], a["beta"], a["stats"],
                                a["relu"], a["bits"], a["codes"], a["ldc"], a["ohy"], a["ohx"], a["flag"], a["N"], a["G"], a["ci"],
                                a["co"], a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], None)


def _f32(lib, **kw):
    a = dict(x=PTR, ldx=48, ihy=0, ihx=0, inv_n=1.0 / 15, w=PTR, bias=None, flag=None, y=PTR, N=2, G=10, ci=4, co=4, H=5, W=5, kh=3,
             kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, ys=(1000, 25, 5, 1))
    a.update(kw)
    return lib.qt_gconv2d_codes_f32(a["x"], a["ldx"], a["ihy"], a["ihx"], a["inv_n"], a["w"], a["bias"], a["flag"], a["y"], a["N"],
                                    a["G"], a["ci"], a["co"], a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"],
                                    a["dh"], a["dw"], *a["ys"], None)


def test_codes_entry_validates_before_it_launches():
    lib = _lib.load()
    # 1. negative halos and sizes, a kernel / stride below 1; too many taps
    assert _codes(lib, ihy=-1) == INVALID and _codes(lib, ihx=-1) == INVALID
    assert _codes(lib, ohy=-1) == INVALID and _codes(lib, ohx=-1) == INVALID
    assert _codes(lib, N=-1) == INVALID and _codes(lib, ci=0) == INVALID and _codes(lib, co=0) == INVALID and _codes(lib, sh=0) == INVALID
    assert _codes(lib, kh=5, kw=10) == UNSUPPORTED                                   # 50 taps
    assert _codes(lib, N=0, ohy=-1) == INVALID                                       # the halo's sign is looked at first
    # 2. empty tensors: nothing to do, whatever the pointers and the other limits are
    assert _codes(lib, N=0, x=None, w=None, alpha=None, beta=None, codes=None, flag=None) == OK
    assert _codes(lib, G=0, x=None, codes=None) == OK and _codes(lib, H=0, ihy=65, ci=33) == OK
    # 3. the other limits, in front of the pointers
    assert _codes(lib, ci=33, x=None) == UNSUPPORTED and _codes(lib, ci=32, kh=5, kw=5, ph=2, pw=2, w=None) == UNSUPPORTED     # K = 800
    assert _codes(lib, ci=32, kh=4, kw=4, ph=2, pw=2, ldx=320, x=None) == INVALID    # K = 512 is inside: the null pointer answers
    assert _codes(lib, ihy=65) == UNSUPPORTED and _codes(lib, ohx=65, w=None) == UNSUPPORTED
    assert _codes(lib, G=1 << 19, ci=1, co=4, N=1, H=3, W=3, ldx=1 << 19, ldc=1 << 21) == UNSUPPORTED     # G cout_g > QT_DW_MAX_CHANNELS
    assert _codes(lib, N=1 << 20, G=1, ci=1, co=1, H=40, W=40, ldx=16, ldc=16, ihy=64, ihx=64) == UNSUPPORTED   # 2^31 pixel rows in the input plane
    assert _codes(lib, N=1 << 20, G=1, ci=1, co=1, H=40, W=40, ldx=16, ldc=16, ohy=64, ohx=64) == UNSUPPORTED   # ... in the output plane
    assert _codes(lib, ldc=1 << 31, codes=None) == UNSUPPORTED
    assert _codes(lib, kh=7, kw=7, ph=0, pw=0) == INVALID                            # does not fit a 5 x 5 image
    # 4. null tensors, the quantiser, the row strides ...
    for name in ("x", "w", "alpha", "beta", "codes", "flag"):
        assert _codes(lib, **{name: None}) == INVALID, name
    assert _codes(lib, bits=1) == INVALID and _codes(lib, bits=9) == INVALID
    assert _codes(lib, relu=2) == INVALID and _codes(lib, relu=-1) == INVALID
    assert _codes(lib, ldx=32) == INVALID and _codes(lib, ldc=32) == INVALID         # below 40 rounded up to 16
    assert _codes(lib, ldx=40) == INVALID and _codes(lib, ldc=47) == INVALID         # ... even where the channels would fit
    assert _codes(lib, co=5, ldc=48) == INVALID                                      # 50 output channels need 64-byte rows
    # ... then the alignments
    for name in ("w", "alpha", "beta", "flag"):
        assert _codes(lib, **{name: PTR + 2}) == ALIGNMENT, name
    assert _codes(lib, bias=PTR + 1) == ALIGNMENT and _codes(lib, stats=PTR + 2) == ALIGNMENT
    assert _codes(lib, ldx=52) == ALIGNMENT and _codes(lib, ldc=56) == ALIGNMENT
    assert _codes(lib, x=PTR + 4) == ALIGNMENT and _codes(lib, codes=PTR + 8) == ALIGNMENT
    # any cin_g within the limits and any cout_g: only the null pointer is refused
    for ci, co in ((1, 2), (3, 3), (5, 1), (16, 8), (32, 17)):
        assert _codes(lib, G=4, ci=ci, co=co, ldx=128, ldc=80, alpha=None) == INVALID, (ci, co)
    assert _codes(lib, bits=1, alpha=PTR + 2) == INVALID                             # INVALID_ARG comes before ALIGNMENT


def test_f32_entry_validates_before_it_launches():
    lib = _lib.load()
    assert _f32(lib, ihy=-1) == INVALID and _f32(lib, N=-1) == INVALID and _f32(lib, kh=5, kw=10) == UNSUPPORTED
    assert _f32(lib, N=0, x=None, w=None, y=None) == OK and _f32(lib, H=0, x=None, y=None) == OK
    assert _f32(lib, ihx=65) == UNSUPPORTED and _f32(lib, ci=33, y=None) == UNSUPPORTED
    assert _f32(lib, x=None) == INVALID and _f32(lib, w=None) == INVALID and _f32(lib, y=None) == INVALID
    assert _f32(lib, ys=(1000, 25, 5, 2)) == INVALID                                 # not a dense layout
    assert _f32(lib, ldx=32) == INVALID
    assert _f32(lib, x=PTR + 4) == ALIGNMENT and _f32(lib, y=PTR + 1) == ALIGNMENT and _f32(lib, bias=PTR + 2) == ALIGNMENT
    assert _f32(lib, flag=PTR + 2) == ALIGNMENT and _f32(lib, ldx=52) == ALIGNMENT
    assert _f32(lib, kh=7, kw=7, ph=0, pw=0) == INVALID


# ---- ops -------------------------------------------------------------------------------------------------------------------------------

def test_grouped_codes_applicable_on_its_boundary_shapes():
    f = ops.grouped_codes_applicable
    x = (2, 32, 9, 9)
    for cin_g in (1, 2, 3, 4, 8, 16, 32):                                            # whatever the fp32 entry takes
        G = 96 // cin_g if cin_g == 3 else 32 // cin_g
        assert f((2, G * cin_g, 9, 9), (2 * G, cin_g, 3, 3), 1, 1, 1, G), cin_g
    assert not f((2, 4 * 33, 9, 9), (4, 33, 1, 1), 1, 0, 1, 4)                       # cin_g = 33
    assert f(x, (8, 4, 7, 7), 1, 3, 1, 8) and not f(x, (8, 4, 5, 10), 1, 5, 1, 8)    # 49 / 50 taps
    assert f((1, 64, 9, 9), (2, 32, 4, 4), 1, 2, 1, 2) and not f((1, 64, 9, 9), (2, 32, 3, 6), 1, 3, 1, 2)      # K = 512 / 576
    assert f(x, (8 * 17, 4, 1, 1), (2, 1), 0, 1, 8) and f((2, 4, 9, 9), (2, 2, 3, 3), 1, 1, 1, 2)              # any cout_g; no minimum of groups
    assert not f(x, (8, 4, 3, 3), 1, "same", 1, 8) and not f(x, (8, 4, 3, 3), 1, 1, 1, 4)      # groups do not match the channels
    assert not f((2, 32, 0, 9), (8, 4, 3, 3), 1, 1, 1, 8) and not f((2, 32, 2, 2), (8, 4, 3, 3), 1, 0, 1, 8)
    assert not f((32, 9, 9), (8, 4, 3, 3), 1, 1, 1, 8) and not f(x, (9, 4, 3, 3), 1, 1, 1, 8)
    # 2^31 elements: the tensors of the fp32 entry bound it (a pixel row holds at least one element)
    assert f((1, 4, 1 << 14, (1 << 15) - 1), (4, 1, 1, 1), 1, 0, 1, 4) and not f((1, 4, 1 << 14, 1 << 15), (4, 1, 1, 1), 1, 0, 1, 4)
    for args in ((x, (8, 4, 3, 3), 1, 1, 1, 8), (x, (8, 4, 5, 10), 1, 5, 1, 8), (x, (16, 2, 3, 3), 2, 1, 1, 16)):
        assert f(*args) == ops.grouped_applicable(*args)


def _host_planes(N=1, Cc=16, H=5, W=5):
    return ops.CodePlanes(codes=torch.zeros((N * H * W, 16), dtype=torch.int8), rows=N * H * W, K=Cc, inv_n=1.0 / 15, bit_width=4)


def test_wrappers_check_their_operands_before_any_launch():
    w, a = torch.randn(16, 4, 3, 3), torch.ones(16)
    epi = ops.CodeEpilogue(a, a, 4)
    shape = (1, 16, 5, 5)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_codes(_host_planes(), shape, w, None, epi, 1, 1, 1, 4)                   # host tensors
    with pytest.raises(TypeError):
        ops.grouped_conv2d_from_codes(_host_planes(), shape, w, None, 1, 1, 1, 4)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_codes(torch.zeros(shape), shape, w, None, epi, 1, 1, 1, 4)               # not CodePlanes
    with pytest.raises(TypeError):
        ops.grouped_conv2d_from_codes(object(), shape, w, groups=4)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(_host_planes(), None, w, None, epi, 1, 1, 1, 4)                    # no logical shape


def _bn(c):
    return nn.BatchNorm2d(c)


def test_fused_grouped_block_declines_what_it_cannot_run():
    ok = FusedGroupedDorefaBnQuant(DorefaConv2d(16, 16, 3, padding=1, groups=4, bit_width=1), _bn(16), 4)
    assert ok.out_halo == (0, 0) and ok.fold == "reference" and ok.relu == 1 and ok.bit_width == 4
    k3 = FusedGroupedDorefaBnQuant(DorefaConv2d(32, 68, 3, stride=2, padding=1, groups=4, bit_width=3), _bn(68), 2, relu=False,
                                   out_halo=(2, 1), fold="device")
    assert k3.fold == "device" and k3.out_halo == (2, 1) and k3.relu == 0          # any weight bit_width, cin_g = 8, cout_g = 17
    assert FusedGroupedDorefaBnQuant(DorefaConv2d(8, 8, 1, groups=4, bit_width=1), _bn(8), 8, out_halo=1).out_halo == (1, 1)
    assert (_fused.GROUPED_MIN_GROUPS, _fused.GROUPED_MAX_CIN_G) == (4, 8)
    for conv, bn in ((DorefaConv2d(8, 8, 3, padding=1, groups=2, bit_width=1), _bn(8)),                 # two groups
                     (DorefaConv2d(24, 24, 3, padding=1, groups=3, bit_width=1), _bn(24)),              # three
                     (DorefaConv2d(64, 64, 3, padding=1, groups=4, bit_width=1), _bn(64)),              # cin_g = 16
                     (DorefaConv2d(8, 8, 3, padding=1, groups=8, bit_width=1), _bn(8)),                 # depthwise
                     (DorefaConv2d(8, 8, 3, padding=1, bit_width=1), _bn(8)),                           # ungrouped
                     (BinConv2d(16, 16, 3, padding=1, groups=4), _bn(16)),
                     (nn.Conv2d(16, 16, 3, padding=1, groups=4), _bn(16)),
                     (DorefaConv2d(16, 16, 3, padding="same", groups=4, bit_width=1), _bn(16)),
                     (DorefaConv2d(16, 16, 3, padding=1, groups=4, bit_width=1, ), _bn(32)),            # the BatchNorm's width
                     (DorefaConv2d(16, 16, (5, 10), padding=5, groups=4, bit_width=1), _bn(16))):       # 50 taps
        with pytest.raises(ValueError):
            FusedGroupedDorefaBnQuant(conv, bn, 4)
    gl = DorefaConv2d(16, 16, 3, padding=1, groups=4, bit_width=1)
    with pytest.raises(ValueError):
        FusedGroupedDorefaBnQuant(gl, nn.BatchNorm1d(16), 4)                         # ... and its rank
    with pytest.raises(ValueError):
        FusedGroupedDorefaBnQuant(gl, _bn(16), 4, relu="pre")
    for bits in (1, 9):
        with pytest.raises(ValueError):
            FusedGroupedDorefaBnQuant(gl, _bn(16), bits)
    # the siblings keep declining a grouped conv
    with pytest.raises(ValueError):
        FusedDorefaConvBnQuant(gl, _bn(16), 4)
    with pytest.raises(ValueError):
        FusedDepthwiseDorefaBnQuant(gl, _bn(16), 4)
    act = packed.CodeActivation(_host_planes(1, 16), (1, 16, 5, 5))
    with pytest.raises(ValueError):
        ok(act)                                                                      # training mode
    ok.conv.eval()
    with pytest.raises(ValueError):
        ok(act)                                                                      # ... of the BatchNorm
    ok.eval()
    with pytest.raises(ValueError):
        ok(act, residual=act)
    with pytest.raises(TypeError):
        ok(torch.randn(1, 16, 5, 5))                                                 # not a CodeActivation
    with pytest.raises(ValueError):
        ok(packed.CodeActivation(_host_planes(1, 8), (1, 8, 5, 5)))                  # another channel count
    with pytest.raises(TypeError):
        ok(act)                                                                      # a host plane
    ok.refold()
    # (an off-grid eval weight is a device-side question: tests/test_gpu_gconv_codes.py)


def test_grouped_deferred_restores_both_switches():
    start = (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES)
    for on in (True, False):
        with lazy.grouped_deferred(on):
            assert (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES) == (on, on)
            with lazy.grouped_deferred(not on):
                assert (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES) == (not on, not on)
            assert (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES) == (on, on)
        assert (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES) == start
    # the two switches are independent outside the block: a mixed setting comes back as it was
    lazy.DEFER_GROUPED_CODES = not start[0]
    try:
        with pytest.raises(KeyError):
            with lazy.grouped_deferred(start[0]):
                raise KeyError("x")
        assert (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES) == (start[0], not start[0])
    finally:
        lazy.DEFER_GROUPED_CODES = start[1]
    # the depthwise pair is another pair
    dw = (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES)
    with lazy.grouped_deferred(not start[1]):
        assert (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES) == dw


def test_host_grouped_dorefa_layers_never_defer():
    """On the host nothing defers, whatever the switches say: the layer keeps the torch expression.  (The admit / decline table of
    ``lazy._dorefa_can_defer`` needs device weights: tests/test_gpu_gconv_codes.py.)"""
    gl = DorefaConv2d(16, 16, 3, padding=1, groups=4, bit_width=1).eval()
    x = torch.randn(1, 16, 5, 5)
    for on in (True, False):
        with torch.no_grad(), lazy.grouped_deferred(on):
            assert not lazy._dorefa_can_defer(gl, x)
            assert not lazy._dorefa_can_defer(gl, lazy._CodeShapeOnly((1, 16, 5, 5)))
            y = gl(x)
        assert type(y) is torch.Tensor and torch.equal(y, torch.nn.functional.conv2d(x, gl.weight, gl.bias, 1, 1, 1, 4))
    with torch.no_grad(), lazy.grouped_deferred(True):
        gl.train()
        assert not lazy._dorefa_can_defer(gl, lazy._CodeShapeOnly((1, 16, 5, 5)))


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_reference_on_hand_computed_outputs():
    """Two groups of two channels, one output channel each, a 2 x 2 image, 1 x 1 taps, inv_n = 1/4, folded alpha = 1, beta = 0, levels
    15, no ReLU.  Channels hold q = 1, 2 | 3, 4 at pixel (0, 0); taps (1/2, 1) | (1, -1/2):
        y[0] = 1/4 * 1/2 + 2/4 * 1 = 0.625 -> 15 y = 9.375: 9;      y[1] = 3/4 - 4/4 * 1/2 = 0.25 -> 3.75: 4.
    With a bias of 0.875 on channel 0: y = 1.5, 15 y = 22.5 — a tie, half to even: 22."""
    q = np.zeros((1, 4, 2, 2), dtype=np.int64)
    q[0, :, 0, 0] = (1, 2, 3, 4)
    q[0, :, 1, 1] = (4, 4, 8, 2)
    w = np.array([[0.5, 1.0], [1.0, -0.5]], dtype=np.float32).reshape(2, 2, 1, 1)
    geom = ((1, 1), (1, 1), (0, 0), (1, 1))
    one, zero = torch.ones(2), torch.zeros(2)
    ref = R.reference(q, 0.25, w, None, 2, geom, C.Epi(alpha=one, beta=zero, levels=15.0, relu=0))
    assert ref["y"][0, :, 0, 0].tolist() == [0.625, 0.25] and ref["codes"][0, 0, 0].tolist() == [9, 4]
    assert ref["y"][0, :, 1, 1].tolist() == [1.5, 1.75] and ref["codes"][0, 1, 1].tolist() == [22, 26]      # 22.5 -> 22, 26.25
    assert int(ref["codes"][0, 0, 1].abs().sum()) == 0 and not ref["flag"] and int(C.sensitive(ref).sum()) == 0
    tie = R.reference(q, 0.25, w, np.array([0.875, 0.0], dtype=np.float32), 2, geom, C.Epi(alpha=one, beta=zero, levels=15.0, relu=0))
    assert tie["y"][0, 0, 0, 0] == 1.5 and int(tie["codes"][0, 0, 0, 0]) == 22
    # a 3 x 3 kernel with padding: the corner output sums the four taps inside the image, input channel by input channel
    q3 = np.arange(1, 19, dtype=np.int64).reshape(1, 2, 3, 3)
    w3 = np.stack([np.full((3, 3), 0.5, np.float32), np.full((3, 3), -0.25, np.float32)])[None]               # [1, 2, 3, 3]
    r3 = R.reference(q3, 0.25, w3, None, 1, ((3, 3), (1, 1), (1, 1), (1, 1)),
                     C.Epi(alpha=torch.ones(1), beta=torch.zeros(1), levels=15.0, relu=1))
    # channel 0 corner: q = 1, 2, 4, 5 -> 12 / 8; channel 1 corner: q = 10, 11, 13, 14 -> -48 / 16
    assert r3["y"][0, 0, 0, 0] == 1.5 - 3.0 and int(r3["codes"][0, 0, 0, 0]) == 0                             # behind the ReLU
    assert r3["y"][0, 0, 1, 1] == (45 / 8) - (126 / 16)
    # the plane: pixel rows of 16 bytes, a zero border
    plane = R.out_plane(ref, (1, 2))
    assert plane.shape == (4 * 6, 16) and plane[1 * 6 + 2, :2].tolist() == [9, 4] and plane[2 * 6 + 3, :2].tolist() == [22, 26]
    assert int(plane.count_nonzero()) == 4
    assert torch.equal(C.decode_plane(plane, 1, 2, 2, 2, (1, 2)), ref["codes"].permute(0, 3, 1, 2))


@pytest.mark.parametrize("i", [i for i, c in enumerate(D.CASES) if c.C * c.m <= 40])
def test_one_channel_per_group_is_the_depthwise_reference(i):
    """cin_g = 1: the grouped reference restates the depthwise one, tensor for tensor."""
    c, r = D.CASES[i], D.build(i)
    ref = R.reference(r.q, r.inv_n, r.w[:, None], r.b, c.C, D.geom(c), r.epi)
    assert np.array_equal(ref["y"], r.ref["y"]) and np.array_equal(np.signbit(ref["y"]), np.signbit(r.ref["y"]))
    for k in ("codes", "t", "lo", "hi"):
        assert torch.equal(ref[k], r.ref[k]), k
    assert ref["flag_head"] == r.ref["flag_head"]


def test_the_case_list_covers_every_axis_value():
    cs = R.CASES
    first = cs[:2 * len(R.SHAPES)]
    assert [(c.G, c.cin_g, c.cout_g) for c in first] == list(R.SHAPES) * 2
    geoms = [(c.kernel, c.stride, c.padding, c.dilation) for c in first]
    assert all(geoms.count(g) >= 2 for g in R.GEOMS)
    assert {(c.H, c.W) for c in cs} == set(R.MAPS) and {c.N for c in cs} == set(R.BATCHES)
    assert {c.in_halo for c in cs} == set(R.HALOS) == {c.out_halo for c in cs}
    assert any(c.in_halo[0] > c.padding[0] and c.in_halo[1] > c.padding[1] for c in cs)         # a halo larger than the padding
    assert any(c.in_halo == (0, 0) and c.padding != (0, 0) for c in cs)                         # ... and a padding without a halo
    assert {c.in_bits for c in cs} == set(R.BITS) == {c.out_bits for c in cs}
    assert {c.relu for c in cs} == {True, False} and {c.form for c in cs} == set(R.FORMS) and {c.taps for c in cs} == set(R.TAPS)
    assert {(c.form, c.bias) for c in cs} == {(f, b) for f in R.FORMS for b in (True, False)}
    assert len({c.id for c in cs}) == len(cs)
    assert all(R.macs(c) <= R.MAC_BUDGET for c in cs)
    assert all(ops.grouped_codes_applicable((c.N, c.G * c.cin_g, c.H, c.W), (c.G * c.cout_g, c.cin_g) + c.kernel, c.stride, c.padding,
                                            c.dilation, c.G) for c in cs)
    # every compile-time form of the kernel: 1 x 1 and 3 x 3 at cin_g 2 / 4 / 8 with cout_g % 4 == 0
    forms = {(c.kernel, c.cin_g) for c in cs if c.cout_g % 4 == 0 and c.kernel in ((1, 1), (3, 3))}
    assert forms >= {(k, ci) for k in ((1, 1), (3, 3)) for ci in (2, 4, 8)}


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[c.id for c in R.CASES])
def test_reference_has_no_sensitive_element_in_any_gpu_case(i):
    """The GPU comparison waives nothing, so the seeds of the list are chosen such that the reference itself is unambiguous
    everywhere."""
    r = R.build(i)
    codes = r.ref["codes"]
    assert C.waiver_cap(codes.numel()) == 0
    assert int(C.sensitive(r.ref).sum()) == 0
    assert int(codes.count_nonzero()) > codes.numel() // 20                          # the case says something
    assert int(codes.abs().max()) <= 127
    if i == 0:
        assert not r.ref["flag"]                                                     # the overflow test starts from a clear flag


def test_overflow_scales_of_the_gpu_test_raise_the_flag_values_they_are_meant_to():
    c, r = R.CASES[0], R.build(0)
    for scale, want in ((200.0, 1), (1e6, 3)):
        epi = C.Epi(alpha=r.alpha * scale, beta=r.beta, levels=r.epi.levels, stats=r.stats, relu=r.epi.relu)
        ref = R.reference(r.q, r.inv_n, r.w, r.b, c.G, R.geom(c), epi)
        assert ref["flag"] and ref["flag_head"] == want, scale


def test_designed_case_sits_on_ties_and_on_the_relu_boundary():
    d = R.designed()
    assert d.cin_g == 4 and d.ties > 0 and d.on_relu > 0 and d.below_relu > 100
    assert int(C.sensitive(d.ref).sum()) == 0 and not d.ref["flag"]
