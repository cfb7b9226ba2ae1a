"""Grouped convs with 16 ... 64 channels per group on the reduction-sliced matrix-core kernel, the host side: the shape and route
predicates and the two C-ABI entries, which validate before they launch.  The kernel: tests/test_gpu_gconv_wide.py."""
import types

import pytest
import torch

from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from test_gconv_mfma_cpu import OK, INVALID, ALIGNMENT, UNSUPPORTED, P, XS, _call, _layer


@pytest.mark.parametrize("c,good", [(8, False), (16, True), (20, False), (24, True), (32, True), (40, True), (48, True), (56, False),
                                    (64, True), (72, False)])
def test_grouped_wide_applicable_channel_window(c, good):
    ok = ops.grouped_wide_applicable
    assert ok((2, 8 * c, 7, 7), (8 * 16, c, 3, 3), 1, 1, 1, 8) == ok((2, 128, 7, 7), (8 * c, 16, 3, 3), 1, 1, 1, 8) == good


def test_grouped_wide_applicable_geometry_window():
    ok = lambda k=3, s=1, p=1, d=1, x=(2, 512, 7, 7): ops.grouped_wide_applicable(x, (512, 64, k, k), s, p, d, 8)      # noqa: E731
    assert ok() and ok(k=1, p=0) and ok(s=2, p=(1, 0)) and ok(k=1, s=2, p=0)
    assert not ok(k=5, p=2) and not ok(s=3) and not ok(s=(2, 1)) and not ok(d=2) and not ok(p=2) and not ok(p="same")
    assert not ok(x=(0, 512, 7, 7)) and not ok(p=0, x=(2, 512, 1, 1)) and not ok(x=(1 << 14, 512, 16, 16))


def test_grouped_wide_route_case_by_case(monkeypatch):
    class Dev(torch.Tensor):          # the stand-in of tests/test_gconv_mfma_cpu.py: a tensor that says it lives on the device
        is_cuda = True

    def on(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype).as_subclass(Dev)

    route = _fused.grouped_wide_route
    monkeypatch.setattr(_fused, "GROUPED_WIDE", True)
    monkeypatch.setattr(_fused, "GROUPED_MFMA", True)
    assert route(_layer(512, 512, 8), on((2, 512, 6, 6))) and route(_layer(8 * 40, 8 * 24, 8), on((2, 320, 6, 6)))
    assert route(_layer(128, 8 * 24, 8), on((2, 128, 6, 6)))                           # 16 in, 24 out: the old kernel refuses 24
    for cin, cout in ((128, 128), (8 * 32, 8 * 48)):                                   # what grouped_mfma_route takes stays there
        assert _fused.grouped_mfma_route(_layer(cin, cout, 8), on((2, cin, 6, 6))) and not route(_layer(cin, cout, 8), on((2, cin, 6, 6)))
    assert not route(_layer(256, 256, 4), on((2, 256, 6, 6)))                          # four groups of 64: the per-group loop
    assert not route(_layer(512, 512, 8), torch.empty(2, 512, 6, 6))                   # a CPU tensor never takes the route
    assert not any(route(_layer(512, 512, 8), on((2, 512, 6, 6), dt)) for dt in (torch.float16, torch.bfloat16))
    for attr, value in (("padding_mode", "reflect"), ("padding", "same"), ("dilation", (2, 2)), ("weight", torch.empty(512, 64, 3, 3).half())):
        lay = _layer(512, 512, 8)
        setattr(lay, attr, value)
        assert not route(lay, on((2, 512, 6, 6)))
    monkeypatch.setattr(_fused, "GROUPED_WIDE", False)                                  # the switch off
    assert not route(_layer(512, 512, 8), on((2, 512, 6, 6)))


@pytest.mark.parametrize("entry", ("fwd", "gin"))
def test_entries_validate_before_they_launch(entry):
    lib = _lib.load()    # the new entries share the old ones' argument lists: handed to the sibling's `_call` under the names it calls
    wide = types.SimpleNamespace(qt_gmconv2d_f32=lib.qt_gwconv2d_f32, qt_gmconv2d_grad_input_f32=lib.qt_gwconv2d_grad_input_f32)
    call = lambda **kw: _call(wide, entry, **kw)          # noqa: E731
    assert call(a=None) == INVALID and call(w=None) == INVALID and call(b=None) == INVALID
    # 1. sizes below their minimum are INVALID even where a limit is broken too
    assert call(N=-1) == INVALID and call(cin_g=0) == INVALID and call(cout_g=0) == INVALID and call(sh=0) == INVALID
    assert call(ph=-1) == INVALID and call(dw=0) == INVALID and call(N=-1, cin_g=20) == INVALID
    assert call(kh=5, kw=10) == UNSUPPORTED
    # 2. an empty problem is OK whatever the pointers and the limits are
    assert call(N=0, a=None, w=None, b=None) == OK and call(G=0, a=None) == OK and call(H=0, cin_g=20, a=None) == OK
    # 3. the limits before kind, pointers and strides; 24, 40 and 64 are inside them here
    for bad in (dict(cin_g=8), dict(cin_g=20), dict(cin_g=56), dict(cout_g=8), dict(cout_g=72), dict(kh=5, kw=5, ph=2, pw=2),
                dict(dh=2, dw=2), dict(sh=3, sw=3), dict(sh=2, sw=1), dict(ph=2), dict(kh=1, kw=3), dict(N=1 << 24)):
        assert call(kind=7, a=None, **bad) == UNSUPPORTED, bad
    for good in (dict(cin_g=40), dict(cout_g=24), dict(cout_g=64), dict(cin_g=64, cout_g=64)):
        assert call(kind=7, a=None, **good) == INVALID, good
    assert call(H=1, W=1, ph=0, pw=0, kind=7) == INVALID                    # the kernel does not fit
    # 4. kind, strides, alignment
    assert call(kind=3) == INVALID and call(xs=(3200, 25, 5, 2)) == INVALID and call(ys=XS) == INVALID
    assert call(a=P + 2) == ALIGNMENT and call(b=P + 1) == ALIGNMENT
    if entry == "fwd":
        assert call(bias=P + 2) == ALIGNMENT
