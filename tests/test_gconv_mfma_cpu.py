"""Grouped convs with 16, 24 or 32 channels per group on the matrix cores, the host side: the shape and route predicates and the
two C-ABI entries, which validate before they launch.  The kernels themselves: tests/test_gpu_gconv_mfma.py."""
import types

import pytest
import torch

from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused

OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
P = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it


def test_grouped_mfma_applicable_at_the_edges_of_the_window():
    ok = ops.grouped_mfma_applicable
    assert ops.GM_MAX_COUT_G == _lib.DEFINES["QT_GM_MAX_COUT_G"] == 48 and _fused.GROUPED_MFMA_MIN_GROUPS == 8 == _fused.GROUPED_MAX_CIN_G
    for cin_g, good in ((8, False), (16, True), (20, False), (24, True), (32, True), (40, False)):
        assert ok((2, 8 * cin_g, 7, 7), (8 * 16, cin_g, 3, 3), 1, 1, 1, 8) == good
    for cout_g, good in ((8, False), (16, True), (24, False), (48, True), (64, False)):
        assert ok((2, 128, 7, 7), (8 * cout_g, 16, 3, 3), 1, 1, 1, 8) == good
    assert ok((2, 128, 7, 7), (128, 16, 1, 1), 2, 0, 1, 8) and ok((2, 128, 7, 7), (128, 16, 3, 3), 2, (1, 0), 1, 8)
    assert ok((2, 32, 7, 7), (32, 16, 3, 3), 1, 1, 1, 2)                          # the group minimum is the route's, not the entry's
    assert not ok((2, 128, 7, 7), (128, 16, 5, 5), 1, 1, 1, 8) and not ok((2, 128, 7, 7), (128, 16, 1, 3), 1, 0, 1, 8)
    assert not ok((2, 128, 7, 7), (128, 16, 3, 3), 3, 1, 1, 8) and not ok((2, 128, 7, 7), (128, 16, 3, 3), (2, 1), 1, 1, 8)
    assert not ok((2, 128, 7, 7), (128, 16, 3, 3), 1, 1, 2, 8) and not ok((2, 128, 7, 7), (128, 16, 3, 3), 1, 2, 1, 8)
    assert not ok((2, 128, 7, 7), (128, 16, 3, 3), 1, "same", 1, 8) and not ok((0, 128, 7, 7), (128, 16, 3, 3), 1, 1, 1, 8)
    assert not ok((2, 128, 1, 1), (128, 16, 3, 3), 1, 0, 1, 8)                    # the kernel does not fit
    assert not ok((1 << 12, 1 << 9, 1 << 5, 1 << 5), (1 << 9, 16, 3, 3), 1, 1, 1, 32)          # 2^31 elements
    assert ok((256, 512, 14, 14), (512, 16, 3, 3), 1, 1, 1, 32)                   # the 3 x 3 of ResNeXt-50's third stage


def _layer(cin, cout, groups, **kw):
    return types.SimpleNamespace(weight=torch.empty(cout, cin // groups, 3, 3), groups=groups, stride=(1, 1), padding=(1, 1),
                                 dilation=(1, 1), padding_mode="zeros", **kw)


def test_grouped_mfma_route_case_by_case(monkeypatch):
    class Dev(torch.Tensor):          # the stand-in of tests/test_gconv_cpu.py: a tensor that says it lives on the device
        is_cuda = True

    def on(shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype).as_subclass(Dev)

    route = _fused.grouped_mfma_route
    monkeypatch.setattr(_fused, "GROUPED_MFMA", True)
    assert not route(_layer(128, 128, 8), torch.empty(2, 128, 6, 6))                   # a CPU tensor never takes the route
    assert route(_layer(128, 128, 8), on((2, 128, 6, 6))) and route(_layer(9 * 32, 9 * 48, 9), on((2, 288, 6, 6)))
    assert not _fused.grouped_route(_layer(128, 128, 8), on((2, 128, 6, 6)))           # the streaming window ends at 8 channels
    assert not route(_layer(64, 64, 4), on((2, 64, 6, 6)))                             # four groups of 16: the per-group loop
    assert not route(_layer(64, 64, 8), on((2, 64, 6, 6)))                             # 8 channels per group: grouped_route's
    assert not any(route(_layer(128, 128, 8), on((2, 128, 6, 6), dt)) for dt in (torch.float16, torch.bfloat16))     # half dtypes
    assert not route(_layer(128, 128, 8), on((128, 6, 6))) and not route(_layer(128, 128, 8), on((2, 64, 6, 6)))
    for attr, value in (("padding_mode", "reflect"), ("padding", "same"), ("dilation", (2, 2)), ("weight", torch.empty(128, 16, 3, 3).half())):
        lay = _layer(128, 128, 8)
        setattr(lay, attr, value)
        assert not route(lay, on((2, 128, 6, 6)))
    monkeypatch.setattr(_fused, "GROUPED_MFMA", False)                                  # the switch off
    assert not route(_layer(128, 128, 8), on((2, 128, 6, 6)))


XS, YS = (8 * 16 * 25, 25, 5, 1), (8 * 32 * 25, 25, 5, 1)


def _call(lib, entry, **kw):
    a = dict(a=P, w=P, bias=None, b=P, N=2, G=8, cin_g=16, cout_g=32, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1,
             xs=XS, ys=YS, kind=0)
    a.update(kw)
    geom = tuple(a[k] for k in ("N", "G", "cin_g", "cout_g", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw"))
    if entry == "fwd":
        return lib.qt_gmconv2d_f32(a["a"], a["w"], a["bias"], a["b"], *geom, *a["xs"], *a["ys"], a["kind"], None)
    return lib.qt_gmconv2d_grad_input_f32(a["a"], a["w"], a["b"], *geom, *a["ys"], *a["xs"], a["kind"], None)


@pytest.mark.parametrize("entry", ("fwd", "gin"))
def test_entries_validate_before_they_launch(entry):
    call = lambda **kw: _call(_lib.load(), entry, **kw)          # noqa: E731
    assert call(a=None) == INVALID and call(w=None) == INVALID and call(b=None) == INVALID
    # 1. sizes below their minimum are INVALID even where a limit is broken too
    assert call(N=-1) == INVALID and call(cin_g=0) == INVALID and call(cout_g=0) == INVALID and call(sh=0) == INVALID
    assert call(ph=-1) == INVALID and call(dw=0) == INVALID and call(N=-1, cin_g=20) == INVALID
    assert call(kh=5, kw=10) == UNSUPPORTED
    # 2. an empty problem is OK whatever the pointers and the limits are
    assert call(N=0, a=None, w=None, b=None) == OK and call(G=0, a=None) == OK and call(H=0, cin_g=20, a=None) == OK
    # 3. the limits before kind, pointers and strides
    for bad in (dict(cin_g=8), dict(cin_g=20), dict(cin_g=40), dict(cout_g=24), dict(cout_g=64), dict(kh=5, kw=5, ph=2, pw=2),
                dict(dh=2, dw=2), dict(sh=3, sw=3), dict(sh=2, sw=1), dict(ph=2), dict(kh=1, kw=3), dict(N=1 << 24)):
        assert call(kind=7, a=None, **bad) == UNSUPPORTED, bad
    assert call(H=1, W=1, ph=0, pw=0, kind=7) == INVALID                    # the kernel does not fit
    # 4. kind, strides, alignment
    assert call(kind=3) == INVALID and call(xs=(3200, 25, 5, 2)) == INVALID and call(ys=XS) == INVALID
    assert call(a=P + 2) == ALIGNMENT and call(b=P + 1) == ALIGNMENT
    if entry == "fwd":
        assert call(bias=P + 2) == ALIGNMENT
