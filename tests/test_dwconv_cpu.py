"""Depthwise convs, the host side: the C-ABI entries exist and validate before they launch, the shape predicate, and the layers
on CPU tensors (which keep the torch expression).  The kernels themselves: tests/test_gpu_dwconv.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, DorefaConv2d

ENTRIES = ("qt_dwconv2d_f32", "qt_dwconv2d_grad_input_f32", "qt_dwconv2d_grad_weight_f32", "qt_dwconv2d_grad_weight_work_floats")
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
P = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it


def test_entries_are_declared_in_the_header_and_bound():
    declared = _lib.header_declared_functions()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES["qt_dwconv2d_grad_weight_work_floats"][0] is ctypes.c_int64
    assert (_lib.DEFINES["QT_DW_RAW"], _lib.DEFINES["QT_DW_SIGN"], _lib.DEFINES["QT_DW_TERNARY"]) == (0, 1, 2)
    assert _lib.DEFINES["QT_DW_MAX_TAPS"] == 49 == ops.DW_MAX_TAPS
    assert ops.DW_KINDS == {"raw": 0, "binary": 1, "ternary": 2}
    assert issubclass(_fused.DepthwiseConv2dFn, _fused.QtFunction)


def test_depthwise_applicable_case_by_case():
    ok = ops.depthwise_applicable
    assert ok((2, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8)                      # m = 1
    assert ok((2, 8, 7, 7), (24, 1, 3, 3), (2, 1), (2, 0), 2, 8)           # m = 3, per-axis geometry
    assert ok((1, 1, 5, 5), (2, 1, 1, 1), 1, 0, 1, 1)                      # groups == C == 1
    assert ok((2, 8, 9, 9), (8, 1, 7, 7), 1, 3, 1, 8)                      # 49 taps
    assert not ok((2, 8, 7, 7), (8, 2, 3, 3), 1, 1, 1, 4)                  # two channels per group
    assert not ok((2, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 4)                  # groups != C
    assert not ok((2, 8, 12, 12), (8, 1, 5, 10), 1, 5, 1, 8)               # kh * kw = 50
    assert not ok((2, 8, 7, 7), (8, 1, 3, 3), 1, "same", 1, 8)             # string padding
    assert not ok((2, 8, 7, 7), (8, 1, 3, 3), 1, "valid", 1, 8)
    assert not ok((2, 8, 7, 7), (12, 1, 3, 3), 1, 1, 1, 8)                 # out_channels no multiple of C
    assert not ok((8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8)                     # not 4-D
    assert not ok((2, 8, 2, 2), (8, 1, 5, 5), 1, 0, 1, 8)                  # the kernel does not fit
    assert not ok((0, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8)                  # empty
    assert not ok((1 << 12, 1 << 10, 1 << 5, 1 << 4), (1 << 10, 1, 3, 3), 1, 1, 1, 1 << 10)          # 2^31 elements
    assert ok((1 << 12, 1 << 10, 1 << 4, 1 << 4), (1 << 10, 1, 3, 3), 1, 1, 1, 1 << 10)
    assert not ok((1 << 12, 1 << 10, 1 << 4, 1 << 4), (1 << 11, 1, 3, 3), 1, 1, 1, 1 << 10)          # ... of the output
    assert ok((256, 1024, 7, 7), (2048, 1, 3, 3), 1, 1, 1, 1024)


def _fwd(lib, **kw):
    a = dict(x=P, w=P, bias=None, y=P, N=2, C=4, m=1, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1,
             xs=(100, 25, 5, 1), ys=(100, 25, 5, 1), kind=0)
    a.update(kw)
    return lib.qt_dwconv2d_f32(a["x"], a["w"], a["bias"], a["y"], a["N"], a["C"], a["m"], a["H"], a["W"], a["kh"], a["kw"], a["sh"],
                               a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], *a["xs"], *a["ys"], a["kind"], None)


def test_forward_validates_before_it_launches():
    lib = _lib.load()
    assert _fwd(lib, x=None) == INVALID and _fwd(lib, w=None) == INVALID and _fwd(lib, y=None) == INVALID
    assert _fwd(lib, N=-1) == INVALID and _fwd(lib, m=0) == INVALID and _fwd(lib, sh=0) == INVALID and _fwd(lib, ph=-1) == INVALID
    assert _fwd(lib, kind=3) == INVALID
    assert _fwd(lib, kh=5, kw=10) == UNSUPPORTED                           # 50 taps
    assert _fwd(lib, kh=7, kw=7, ph=0, pw=0) == INVALID                    # does not fit a 5 x 5 image
    assert _fwd(lib, xs=(100, 25, 5, 2)) == INVALID                        # not a dense layout
    assert _fwd(lib, ys=(100, 1, 25, 5), xs=(100, 1, 20, 4)) == INVALID    # channels-last strides of another shape
    assert _fwd(lib, x=P + 2) == ALIGNMENT and _fwd(lib, bias=P + 1) == ALIGNMENT
    assert _fwd(lib, N=1 << 20, C=1 << 10, xs=(25 << 10, 25, 5, 1), ys=(25 << 10, 25, 5, 1)) == UNSUPPORTED     # >= 2^31 elements
    # empty tensors: nothing to do, whatever the pointers are
    assert _fwd(lib, N=0, x=None, w=None, y=None) == OK and _fwd(lib, C=0, x=None, y=None) == OK


def test_gradients_validate_before_they_launch():
    lib = _lib.load()
    geom = (2, 4, 1, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1)
    nchw = (100, 25, 5, 1)
    gi = lib.qt_dwconv2d_grad_input_f32
    assert gi(None, P, P, *geom, *nchw, *nchw, 0, None) == INVALID and gi(P, P, None, *geom, *nchw, *nchw, 0, None) == INVALID
    assert gi(P, P, P + 2, *geom, *nchw, *nchw, 0, None) == ALIGNMENT
    assert gi(P, P, P, *geom, *nchw, 100, 25, 1, 5, 0, None) == INVALID
    assert gi(None, None, None, 0, *geom[1:], *nchw, *nchw, 0, None) == OK
    work = lib.qt_dwconv2d_grad_weight_work_floats
    need = work(*geom)
    assert need >= 4 * (9 + 1) and work(0, *geom[1:]) == 0 and work(-1, *geom[1:]) == INVALID
    assert work(2, 4, 1, 5, 5, 5, 10, 1, 1, 1, 1, 1, 1) == UNSUPPORTED
    gw = lib.qt_dwconv2d_grad_weight_f32
    assert gw(P, P, P, P, None, P, need - 1, *geom, *nchw, *nchw, 1.001, None) == INVALID          # workspace too small
    assert gw(P, P, P, P, None, None, need, *geom, *nchw, *nchw, 1.001, None) == INVALID
    assert gw(P, P, None, P, None, P, need, *geom, *nchw, *nchw, 1.001, None) == INVALID           # the mask needs the weight
    assert gw(P, P, P, P, None, P, need, *geom, *nchw, *nchw, -1.0, None) == INVALID
    assert gw(P, P, P, P, None, P, need, *geom, *nchw, *nchw, float("nan"), None) == INVALID
    assert gw(P, P, P, P, P + 2, P, need, *geom, *nchw, *nchw, 0.0, None) == ALIGNMENT
    assert gw(None, None, None, None, None, None, 0, 0, *geom[1:], *nchw, *nchw, 0.0, None) == OK
    # the work size covers either layout of the gradient and grows with the channel count only through the plan
    assert work(256, 1024, 2, 7, 7, 3, 3, 1, 1, 1, 1, 1, 1) >= 2048 * 10


def test_wrappers_reject_cpu_tensors():
    x, w = torch.randn(1, 4, 5, 5), torch.randn(4, 1, 3, 3)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d(x, w, None, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_grad_input(x.shape, w, torch.randn(1, 4, 5, 5), 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_grad_weight(x, torch.randn(1, 4, 5, 5), w, 1, 1, 1)


@pytest.mark.parametrize("m", (1, 2))
def test_depthwise_layers_on_cpu_tensors_equal_the_torch_expression(m):
    torch.manual_seed(3)
    C = 6
    x = torch.randn(2, C, 9, 8)
    before = dict(_lib.call_counts)
    for make, q in ((lambda: BinConv2d(C, C * m, 3, padding=1, groups=C), lambda w: torch.where(w < 0, -1.0, 1.0)),
                    (lambda: TerConv2d(C, C * m, 3, stride=2, padding=1, groups=C),
                     lambda w: torch.where(w >= 0.5, 1.0, torch.where(w < -0.5, -1.0, 0.0)))):
        layer = make()
        layer.weight.data.uniform_(-1.5, 1.5)
        assert not _fused.depthwise_route(layer, x)
        xi = x.clone().requires_grad_(True)
        y = layer(xi)
        want = F.conv2d(x, q(layer.weight.detach()), layer.bias, layer.stride, layer.padding, layer.dilation, C)
        assert torch.equal(y.detach(), want)
        y.sum().backward()
        assert xi.grad is not None and layer.weight.grad is not None
        assert (layer.weight.grad[layer.weight.detach().abs() > 1.001] == 0).all()
        layer.eval()
        with torch.no_grad():
            assert torch.equal(layer(x), want)
    for k in (1, 4, 32):
        layer = DorefaConv2d(C, C * m, 3, padding=1, groups=C, bit_width=k)
        y = layer(x)
        want = F.conv2d(x, layer.weight_op.forward(layer.weight).detach(), layer.bias, 1, 1, 1, C)
        assert torch.equal(y.detach(), want)
        y.sum().backward()
        assert layer.weight.grad is not None
    assert {k: v for k, v in _lib.call_counts.items() if k.startswith("qt_dwconv2d")} == \
        {k: v for k, v in before.items() if k.startswith("qt_dwconv2d")}
