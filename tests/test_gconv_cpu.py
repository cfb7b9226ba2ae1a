"""Grouped convs with a few channels per group, the host side: the C-ABI entries exist and validate before they launch, the shape
predicate and the route predicate, and the layers on CPU tensors (which keep the torch expression).  The kernels themselves:
tests/test_gpu_gconv.py."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, DorefaConv2d

ENTRIES = ("qt_gconv2d_f32", "qt_gconv2d_grad_input_f32", "qt_gconv2d_grad_weight_f32", "qt_gconv2d_grad_weight_work_floats")
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
P = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it
MAX_CIN_G, MAX_K = _lib.DEFINES["QT_GC_MAX_CIN_G"], _lib.DEFINES["QT_GC_MAX_K"]
MAX_CHANNELS = _lib.DEFINES["QT_DW_MAX_CHANNELS"]


def test_entries_are_declared_in_the_header_and_bound():
    declared = _lib.header_declared_functions()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["qt_gconv2d_grad_weight_work_floats"][0] is ctypes.c_int64
    assert (MAX_CIN_G, MAX_K) == (32, 512) == (ops.GC_MAX_CIN_G, ops.GC_MAX_K)
    assert all(n.startswith("qt_gconv2d") for n in ENTRIES)        # a two-group layer is pinned to run no qt_dwconv2d* entry
    assert issubclass(_fused.GroupedConv2dFn, _fused.QtFunction)
    assert _fused.GROUPED_MIN_GROUPS == 4 and 1 <= _fused.GROUPED_MAX_CIN_G <= 31


def test_grouped_applicable_case_by_case():
    ok = ops.grouped_applicable
    assert ok((2, 12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 4)                       # cin_g 3, cout_g 2
    assert ok((2, 12, 7, 7), (20, 3, 3, 3), (2, 1), (2, 0), (1, 2), 4)       # per-axis geometry
    assert ok((2, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8)                        # cin_g 1: accepted at this level
    assert ok((1, 5, 5, 5), (2, 5, 1, 1), 1, 0, 1, 1)                        # one group
    assert ok((1, 2 * MAX_CIN_G, 9, 9), (2, MAX_CIN_G, 4, 4), 1, 0, 1, 2)    # K exactly 512
    assert MAX_CIN_G * 16 == MAX_K
    assert not ok((1, 2 * (MAX_CIN_G + 1), 9, 9), (2, MAX_CIN_G + 1, 3, 3), 1, 0, 1, 2)       # cin_g 33
    assert not ok((1, 64, 9, 9), (2, 32, 3, 6), 1, 0, 1, 2)                  # K = 576
    assert ok((1, 20, 9, 9), (2, 10, 7, 7), 1, 3, 1, 2)                      # 49 taps, K = 490
    assert not ok((1, 22, 9, 9), (2, 11, 7, 7), 1, 3, 1, 2)                  # 49 taps, K = 539
    assert not ok((2, 8, 12, 12), (8, 2, 5, 10), 1, 5, 1, 4)                 # kh * kw = 50
    assert not ok((2, 12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 2)                   # C != G * cin_g
    assert not ok((2, 12, 7, 7), (10, 3, 3, 3), 1, 1, 1, 4)                  # out_channels no multiple of G
    assert not ok((2, 12, 7, 7), (8, 3, 3, 3), 1, "same", 1, 4)              # string padding
    assert not ok((12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 4)                      # not 4-D
    assert not ok((2, 12, 2, 2), (8, 3, 5, 5), 1, 0, 1, 4)                   # the kernel does not fit
    assert not ok((0, 12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 4)                   # empty
    assert not ok((2, 12, 7, 7), (8, 3, 3, 3), 0, 1, 1, 4)                   # stride 0
    assert not ok((1 << 12, 1 << 10, 1 << 5, 1 << 4), (1 << 10, 2, 3, 3), 1, 1, 1, 1 << 9)          # 2^31 elements
    assert ok((1 << 12, 1 << 10, 1 << 4, 1 << 4), (1 << 10, 2, 3, 3), 1, 1, 1, 1 << 9)
    assert not ok((1 << 12, 1 << 10, 1 << 4, 1 << 4), (1 << 11, 2, 3, 3), 1, 1, 1, 1 << 9)          # ... of the output
    assert not ok((1, 8, 1, 1), (2 * MAX_CHANNELS, 2, 1, 1), 1, 0, 1, 4)     # more output channels than the grid takes
    assert ok((256, 128, 56, 56), (128, 4, 3, 3), 1, 1, 1, 32)               # the 3 x 3 of a ResNeXt-50 block


def _layer(cin, cout, groups, **kw):
    return types.SimpleNamespace(weight=torch.empty(cout, cin // groups, 3, 3), groups=groups, stride=(1, 1), padding=(1, 1),
                                 dilation=(1, 1), padding_mode="zeros", **kw)


def test_grouped_route_case_by_case(monkeypatch):
    x = torch.empty(2, 32, 6, 6)
    # a CPU tensor never takes the route ...
    assert not _fused.grouped_route(_layer(32, 32, 8), x)

    # ... the remaining conditions are looked at on a stand-in that says it lives on the device
    class Dev(torch.Tensor):
        is_cuda = True

    def on(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype).as_subclass(Dev)

    route = _fused.grouped_route
    assert _fused.GROUPED_MAX_CIN_G >= 4, "the window below assumes the shipped constant admits 4 channels per group"
    assert route(_layer(32, 32, 8), on((2, 32, 6, 6)))                                  # 8 groups of 4
    assert route(_layer(32, 64, 8), on((2, 32, 6, 6)))
    assert route(_layer(8, 8, 4), on((2, 8, 6, 6)))                                     # groups == GROUPED_MIN_GROUPS, cin_g 2
    assert not route(_layer(8, 8, 2), on((2, 8, 6, 6)))                                 # two groups
    assert not route(_layer(9, 9, 3), on((2, 9, 6, 6)))                                 # three groups
    assert not route(_layer(8, 8, 8), on((2, 8, 6, 6)))                                 # one channel per group: the depthwise route
    assert not route(_layer(8, 8, 1), on((2, 8, 6, 6)))
    assert not route(_layer(32, 32, 8), on((2, 32, 6, 6), torch.float16))               # half dtypes
    assert not route(_layer(32, 32, 8), on((32, 6, 6)))                                 # not 4-D
    assert not route(_layer(32, 32, 8), on((2, 16, 6, 6)))                              # channels that do not match
    lay = _layer(32, 32, 8)
    lay.padding_mode = "reflect"
    assert not route(lay, on((2, 32, 6, 6)))
    lay = _layer(32, 32, 8)
    lay.padding = "same"
    assert not route(lay, on((2, 32, 6, 6)))
    lay = _layer(32, 32, 8)
    lay.weight = lay.weight.half()
    assert not route(lay, on((2, 32, 6, 6)))
    # the cin_g window: the constant's own value is inside, the next one outside, 32 always outside
    top = _fused.GROUPED_MAX_CIN_G
    assert route(_layer(4 * top, 8, 4), on((1, 4 * top, 6, 6)))
    assert not route(_layer(4 * (top + 1), 8, 4), on((1, 4 * (top + 1), 6, 6)))
    assert not route(_layer(128, 8, 4), on((1, 128, 6, 6)))
    monkeypatch.setattr(_fused, "GROUPED_MAX_CIN_G", 1)                                 # routing off
    assert not route(_layer(32, 32, 8), on((2, 32, 6, 6)))


GEOM = (2, 4, 3, 2, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1)        # N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw
XS, YS = (300, 25, 5, 1), (200, 25, 5, 1)


def _fwd(lib, **kw):
    a = dict(x=P, w=P, bias=None, y=P, N=2, G=4, cin_g=3, cout_g=2, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1,
             xs=XS, ys=YS, kind=0)
    a.update(kw)
    return lib.qt_gconv2d_f32(a["x"], a["w"], a["bias"], a["y"], a["N"], a["G"], a["cin_g"], a["cout_g"], a["H"], a["W"], a["kh"],
                              a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], *a["xs"], *a["ys"], a["kind"], None)


def test_forward_validates_before_it_launches():
    lib = _lib.load()
    assert _fwd(lib, x=None) == INVALID and _fwd(lib, w=None) == INVALID and _fwd(lib, y=None) == INVALID
    # 1. invalid sizes come first: a size below its minimum is INVALID even where a limit is broken too
    assert _fwd(lib, N=-1) == INVALID and _fwd(lib, cin_g=0) == INVALID and _fwd(lib, cout_g=0) == INVALID and _fwd(lib, G=-1) == INVALID
    assert _fwd(lib, sh=0) == INVALID and _fwd(lib, ph=-1) == INVALID and _fwd(lib, dw=0) == INVALID
    assert _fwd(lib, N=-1, cin_g=MAX_CIN_G + 1) == INVALID
    assert _fwd(lib, kh=5, kw=10) == UNSUPPORTED                           # 50 taps > QT_DW_MAX_TAPS
    assert _lib.DEFINES["QT_DW_MAX_TAPS"] == 49
    # 2. empty operands before the limits and before the pointers
    assert _fwd(lib, N=0, x=None, w=None, y=None) == OK and _fwd(lib, G=0, x=None, y=None) == OK
    assert _fwd(lib, H=0, cin_g=MAX_CIN_G + 1, x=None) == OK
    # 3. the limits before kind, pointers and strides
    assert _fwd(lib, cin_g=MAX_CIN_G + 1, kind=7, x=None) == UNSUPPORTED
    assert _fwd(lib, cin_g=MAX_CIN_G, kh=4, kw=4, H=9, W=9, kind=7) == INVALID      # K == 512 is inside: the kind is looked at
    assert _fwd(lib, cin_g=MAX_CIN_G, kh=3, kw=6, H=9, W=9, kind=7) == UNSUPPORTED  # K == 576
    assert _fwd(lib, cin_g=11, kh=7, kw=7, H=9, W=9, x=None) == UNSUPPORTED        # 49 taps, K == 539
    assert _fwd(lib, G=MAX_CHANNELS, cout_g=2, H=1, W=1, ph=1, pw=1, x=None) == UNSUPPORTED
    assert _fwd(lib, N=1 << 20, G=1 << 10, x=None) == UNSUPPORTED           # >= 2^31 elements
    assert _fwd(lib, kh=7, kw=7, ph=0, pw=0, kind=7) == INVALID             # does not fit a 5 x 5 image
    # 4. kind, null tensors, strides, alignment
    assert _fwd(lib, kind=3) == INVALID
    assert _fwd(lib, xs=(300, 25, 5, 2)) == INVALID                         # not a dense layout
    assert _fwd(lib, xs=(200, 25, 5, 1)) == INVALID                         # the strides of another channel count
    assert _fwd(lib, ys=(200, 1, 25, 5)) == INVALID                         # channels-last strides of another shape
    assert _fwd(lib, x=P + 2) == ALIGNMENT and _fwd(lib, bias=P + 1) == ALIGNMENT


def test_gradients_validate_before_they_launch():
    lib = _lib.load()
    gi = lib.qt_gconv2d_grad_input_f32
    assert gi(None, P, P, *GEOM, *YS, *XS, 0, None) == INVALID and gi(P, P, None, *GEOM, *YS, *XS, 0, None) == INVALID
    assert gi(P, P, P + 2, *GEOM, *YS, *XS, 0, None) == ALIGNMENT
    assert gi(P, P, P, *GEOM, *YS, 300, 25, 1, 5, 0, None) == INVALID
    assert gi(P, P, P, *GEOM, *XS, *XS, 0, None) == INVALID                 # go described with the strides of x
    assert gi(P, P, P, *GEOM, *YS, *XS, 5, None) == INVALID
    assert gi(None, None, None, 0, *GEOM[1:], *YS, *XS, 0, None) == OK
    assert gi(None, None, None, 2, 4, MAX_CIN_G + 1, *GEOM[3:], *YS, *XS, 9, None) == UNSUPPORTED
    work = lib.qt_gconv2d_grad_weight_work_floats
    need = work(*GEOM)
    assert need >= 4 * 2 * 3 * (9 + 1) and work(0, *GEOM[1:]) == 0 and work(-1, *GEOM[1:]) == INVALID
    assert work(2, 4, 3, 2, 5, 5, 5, 10, 1, 1, 1, 1, 1, 1) == UNSUPPORTED
    assert work(2, 4, MAX_CIN_G + 1, 2, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1) == UNSUPPORTED
    gw = lib.qt_gconv2d_grad_weight_f32
    # a workspace too small for either layout of go: less than one split's partials (the query is the larger of the two plans)
    assert gw(P, P, P, P, None, P, 4 * 2 * 3 * (9 + 1) - 1, *GEOM, *YS, *XS, 1.001, None) == INVALID
    assert gw(P, P, P, P, None, None, need, *GEOM, *YS, *XS, 1.001, None) == INVALID
    assert gw(P, P, None, P, None, P, need, *GEOM, *YS, *XS, 1.001, None) == INVALID           # the mask needs the weight
    assert gw(P, P, P, P, None, P, need, *GEOM, *YS, *XS, -1.0, None) == INVALID
    assert gw(P, P, P, P, None, P, need, *GEOM, *YS, *XS, float("nan"), None) == INVALID
    assert gw(P, P, P, P, P + 2, P, need, *GEOM, *YS, *XS, 0.0, None) == ALIGNMENT
    assert gw(None, None, None, None, None, None, 0, 0, *GEOM[1:], *YS, *XS, 0.0, None) == OK
    assert gw(None, None, None, None, None, None, 0, 2, 4, MAX_CIN_G + 1, *GEOM[3:], *YS, *XS, -1.0, None) == UNSUPPORTED
    # the work size covers either layout of the gradient: one partial per (split, co, ci, tap) and per (split, co, ci) for the bias
    assert work(256, 32, 4, 4, 56, 56, 3, 3, 1, 1, 1, 1, 1, 1) >= 128 * 4 * 10


def test_wrappers_reject_cpu_tensors():
    x, w = torch.randn(1, 8, 5, 5), torch.randn(8, 2, 3, 3)
    with pytest.raises(TypeError):
        ops.grouped_conv2d(x, w, None, 1, 1, 1, 4)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_grad_input(x.shape, w, torch.randn(1, 8, 5, 5), 1, 1, 1, 4)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_grad_weight(x, torch.randn(1, 8, 5, 5), w, 1, 1, 1, 4)


@pytest.mark.parametrize("cout_g", (3, 6))
def test_grouped_layers_on_cpu_tensors_equal_the_torch_expression(cout_g):
    torch.manual_seed(3)
    G, cin_g = 4, 3
    C, Cout = G * cin_g, G * cout_g
    x = torch.randn(2, C, 9, 8)
    before = dict(_lib.call_counts)
    for make, q in ((lambda: BinConv2d(C, Cout, 3, padding=1, groups=G), lambda w: torch.where(w < 0, -1.0, 1.0)),
                    (lambda: TerConv2d(C, Cout, 3, stride=2, padding=1, groups=G),
                     lambda w: torch.where(w >= 0.5, 1.0, torch.where(w < -0.5, -1.0, 0.0)))):
        layer = make()
        layer.weight.data.uniform_(-1.5, 1.5)
        assert not _fused.grouped_route(layer, x)
        xi = x.clone().requires_grad_(True)
        y = layer(xi)
        want = F.conv2d(x, q(layer.weight.detach()), layer.bias, layer.stride, layer.padding, layer.dilation, G)
        assert torch.equal(y.detach(), want)
        y.sum().backward()
        assert xi.grad is not None and layer.weight.grad is not None
        assert (layer.weight.grad[layer.weight.detach().abs() > 1.001] == 0).all()
        layer.eval()
        with torch.no_grad():
            assert torch.equal(layer(x), want)
    for k in (1, 4, 32):
        layer = DorefaConv2d(C, Cout, 3, padding=1, groups=G, bit_width=k)
        y = layer(x)
        want = F.conv2d(x, layer.weight_op.forward(layer.weight).detach(), layer.bias, 1, 1, 1, G)
        assert torch.equal(y.detach(), want)
        y.sum().backward()
        assert layer.weight.grad is not None
    assert {k: v for k, v in _lib.call_counts.items() if k.startswith("qt_gconv2d")} == \
        {k: v for k, v in before.items() if k.startswith("qt_gconv2d")}
