"""Grouped convs with 16, 24 or 32 channels per group on bf16 / fp16 activations, the host side: ``_fused.grouped_mfma_half_route``
case by case and the two C-ABI entries of csrc/gconv_mfma_h.hip, which validate before they launch.  The kernels themselves:
tests/test_gpu_gconv_mfma_half.py."""
import contextlib
import types

import pytest
import torch

from pytorch_quantize_impls_amd import _lib
from pytorch_quantize_impls_amd.functions import _fused

OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
P = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it
F32, BF16, F16 = (_lib.DEFINES[n] for n in ("QT_DTYPE_F32", "QT_DTYPE_BF16", "QT_DTYPE_F16"))


class Dev(torch.Tensor):          # the stand-in of tests/test_gconv_cpu.py: a tensor that says it lives on the device
    is_cuda = True


def on(shape, dtype):
    return torch.empty(shape, dtype=dtype).as_subclass(Dev)


def _layer(cin, cout, groups, dtype):
    return types.SimpleNamespace(weight=on((cout, cin // groups, 3, 3), dtype), groups=groups, stride=(1, 1), padding=(1, 1),
                                 dilation=(1, 1), padding_mode="zeros")


@contextlib.contextmanager
def autocast_state(dtype):
    """The thread's CUDA autocast state as ``torch.autocast("cuda", dtype=dtype)`` sets it (that context manager switches itself
    off on a machine without a device; ``_fused.half_route`` reads exactly these two values)."""
    was, was_dt = torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype()
    torch.set_autocast_enabled(True)
    torch.set_autocast_gpu_dtype(dtype)
    try:
        yield
    finally:
        torch.set_autocast_enabled(was)
        torch.set_autocast_gpu_dtype(was_dt)


@pytest.mark.parametrize("dt,other", ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)))
def test_grouped_mfma_half_route_case_by_case(monkeypatch, dt, other):
    route = _fused.grouped_mfma_half_route
    monkeypatch.setattr(_fused, "GROUPED_MFMA_HALF", True)
    x = on((2, 128, 6, 6), dt)
    assert route(_layer(128, 128, 8, dt), x) and route(_layer(9 * 32, 9 * 48, 9, dt), on((2, 288, 6, 6), dt))     # same half dtype
    assert not route(_layer(128, 128, 8, torch.float32), x)                            # an fp32 weight without autocast
    with autocast_state(dt):
        assert route(_layer(128, 128, 8, torch.float32), x)                            # ... only under autocast to that dtype
    with autocast_state(other):
        assert not route(_layer(128, 128, 8, torch.float32), x) and not route(_layer(128, 128, 8, dt), x)
    assert not route(_layer(128, 128, 8, other), x)                                    # the other half dtype
    assert not route(_layer(64, 64, 4, dt), on((2, 64, 6, 6), dt))                     # four groups
    assert not route(_layer(64, 128, 8, dt), on((2, 64, 6, 6), dt))                    # cin_g 8: grouped_half_route's
    assert not route(_layer(160, 128, 8, dt), on((2, 160, 6, 6), dt))                  # cin_g 20
    assert not route(_layer(128, 8 * 24, 8, dt), x)                                    # cout_g 24
    assert not _fused.grouped_mfma_route(_layer(128, 128, 8, dt), x)                   # the fp32 route still declines half
    monkeypatch.setattr(_fused, "GROUPED_MFMA_HALF", False)                             # the switch off
    assert not route(_layer(128, 128, 8, dt), x)


XS, YS = (8 * 16 * 25, 25, 5, 1), (8 * 32 * 25, 25, 5, 1)


@pytest.mark.parametrize("entry", ("fwd", "gin"))
def test_half_entries_validate_before_they_launch(entry):
    def call(**kw):
        a = dict(a=P, dtype=BF16, w=P, w_dtype=BF16, bias=None, b=P, N=2, G=8, cin_g=16, cout_g=32, H=5, W=5, kh=3, kw=3, sh=1, sw=1,
                 ph=1, pw=1, dh=1, dw=1, xs=XS, ys=YS, kind=0)
        a.update(kw)
        geom = tuple(a[k] for k in ("N", "G", "cin_g", "cout_g", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw"))
        if entry == "fwd":
            return _lib.load().qt_gmconv2d_h(a["a"], a["dtype"], a["w"], a["w_dtype"], a["bias"], a["b"], *geom, *a["xs"], *a["ys"],
                                             a["kind"], None)
        return _lib.load().qt_gmconv2d_grad_input_h(a["a"], a["dtype"], a["w"], a["w_dtype"], a["b"], *geom, *a["ys"], *a["xs"],
                                                    a["kind"], None)

    # 0. the dtype checks come before everything, the empty problem included
    assert call(dtype=F32, w_dtype=F32) == INVALID and call(dtype=7) == INVALID and call(dtype=BF16, w_dtype=F16) == INVALID
    assert call(dtype=F16, w_dtype=BF16, N=0) == INVALID and call(dtype=3, kh=5, kw=10) == INVALID
    # 1. sizes below their minimum are INVALID even where a limit is broken too; 2. an empty problem is OK whatever the pointers are
    assert call(N=-1) == INVALID and call(cin_g=0) == INVALID and call(sh=0) == INVALID and call(N=-1, cin_g=20) == INVALID
    assert call(kh=5, kw=10) == UNSUPPORTED
    assert call(N=0, a=None, w=None, b=None) == OK and call(H=0, cin_g=20, a=None) == OK and call(G=0, dtype=F16, w_dtype=F32) == OK
    # 3. the limits before kind, pointers and strides
    for bad in (dict(cin_g=8), dict(cin_g=20), dict(cin_g=40), dict(cout_g=24), dict(cout_g=64), dict(kh=5, kw=5, ph=2, pw=2),
                dict(dh=2, dw=2), dict(sh=3, sw=3), dict(sh=2, sw=1), dict(ph=2), dict(kh=1, kw=3), dict(N=1 << 24)):
        assert call(kind=7, a=None, **bad) == UNSUPPORTED, bad
    assert call(H=1, W=1, ph=0, pw=0, kind=7) == INVALID                    # the kernel does not fit
    # 4. kind, null tensors, strides; then alignment: 2 bytes for the half tensors, 4 for an fp32 weight and the bias
    assert call(kind=3) == INVALID and call(a=None) == INVALID and call(w=None) == INVALID and call(b=None) == INVALID
    assert call(xs=(3200, 25, 5, 2)) == INVALID and call(ys=XS) == INVALID
    assert call(a=P + 1) == ALIGNMENT and call(b=P + 1) == ALIGNMENT and call(w=P + 1) == ALIGNMENT
    assert call(w=P + 2, w_dtype=F32, dtype=F16) == ALIGNMENT and (entry == "gin" or call(bias=P + 2) == ALIGNMENT)
