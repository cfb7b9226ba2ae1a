"""The one-term matrix-core weight gradient of the grouped convs on bf16 / fp16 operands, the host side: qt_gmconv2d_grad_weight_h
(csrc/gconv_mfma_h.hip) validates before it launches, and the route choice of ``GroupedMfmaConv2dFn.backward`` for a half
activation.  The kernel itself: tests/test_gpu_gconv_mfma_wgrad_half.py."""
import pytest

from pytorch_quantize_impls_amd import _lib
from pytorch_quantize_impls_amd.functions import _fused
from test_gconv_mfma_half_cpu import ALIGNMENT, BF16, F16, F32, INVALID, OK, P, UNSUPPORTED, XS, YS

GEOM = ("N", "G", "cin_g", "cout_g", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw")


def call(**kw):
    a = dict(go=P, x=P, dtype=BF16, w=P, gw=P, gbias=P, w_dtype=BF16, work=P, N=2, G=8, cin_g=16, cout_g=32, H=5, W=5, kh=3, kw=3, sh=1,
             sw=1, ph=1, pw=1, dh=1, dw=1, xs=XS, ys=YS, ste=1.001)
    a.update(kw)
    geom = tuple(a[k] for k in GEOM)
    floats = a["floats"] if "floats" in a else max(_lib.load().qt_gmconv2d_grad_weight_work_floats(*geom), 0)
    return _lib.load().qt_gmconv2d_grad_weight_h(a["go"], a["x"], a["dtype"], a["w"], a["gw"], a["gbias"], a["w_dtype"], a["work"],
                                                 floats, *geom, *a["ys"], *a["xs"], a["ste"], None)


def test_entry_validates_before_it_launches():
    # 0. the dtype checks come before everything, the empty problem included
    assert call(dtype=F32, w_dtype=F32) == INVALID and call(dtype=7) == INVALID and call(dtype=BF16, w_dtype=F16) == INVALID
    assert call(dtype=F16, w_dtype=BF16, N=0) == INVALID and call(dtype=3, kh=5, kw=10) == INVALID
    # 1. sizes below their minimum; 2. an empty problem is OK whatever the pointers are
    assert call(N=-1) == INVALID and call(cout_g=0) == INVALID and call(N=-1, cin_g=20) == INVALID and call(kh=5, kw=10) == UNSUPPORTED
    assert call(N=0, go=None, x=None, gw=None, work=None) == OK and call(H=0, cin_g=20, go=None, dtype=F16, w_dtype=F32) == OK
    # 3. the limits before pointers and strides
    for bad in (dict(cin_g=8), dict(cin_g=20), dict(cin_g=40), dict(cout_g=24), dict(cout_g=64), dict(kh=5, kw=5, ph=2, pw=2),
                dict(dh=2, dw=2), dict(sh=3, sw=3), dict(sh=2, sw=1), dict(ph=2), dict(kh=1, kw=3), dict(N=1 << 24)):
        assert call(ste=-1.0, go=None, **bad) == UNSUPPORTED, bad
    assert call(H=1, W=1, ph=0, pw=0, go=None) == INVALID                  # the kernel does not fit
    # 4. pointers (w only because the mask is on), the threshold, strides, the workspace of the ONE query
    for name in ("go", "x", "gw", "work", "w"):
        assert call(**{name: None}) == INVALID, name
    assert call(ste=-1.0) == INVALID and call(ste=float("nan")) == INVALID and call(floats=-1) == INVALID
    assert call(xs=(3200, 25, 5, 2)) == INVALID and call(ys=XS) == INVALID
    need = _lib.load().qt_gmconv2d_grad_weight_work_floats(2, 8, 16, 32, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1)
    assert need == 2 * 8 * (9 * 32 * 16 + 32)
    assert call(floats=need - 1) == INVALID and call(floats=need - 1, work=P + 4) == INVALID
    # 5. alignment: 2 bytes for go / x and a half gw / gbias / w, 4 for their fp32 forms, 16 for work
    for name, off, wdt in (("go", 1, BF16), ("x", 1, BF16), ("gw", 1, BF16), ("gbias", 1, BF16), ("w", 1, BF16), ("gw", 2, F32),
                           ("gbias", 2, F32), ("w", 2, F32), ("work", 4, BF16), ("work", 8, F32)):
        assert call(**{name: P + off}, w_dtype=wdt) == ALIGNMENT, (name, off)
    # with the mask off a null w passes the pointer checks: the call gets as far as the alignment check
    assert call(w=None, ste=0.0, work=P + 4) == ALIGNMENT and call(w=None, ste=0.5, work=P + 4) == INVALID


@pytest.mark.parametrize("switch", (True, False))
def test_half_wgrad_route_is_a_function_of_its_switch_and_the_floor(monkeypatch, switch):
    monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD_HALF", switch)
    monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD", not switch)          # the fp32 switch is not read
    route = _fused.grouped_mfma_wgrad_route
    assert route((2, 128, 23, 23), half=True) == switch and route((256, 512, 14, 14), half=True) == switch
    assert route((2, 128, 23, 23)) == (not switch) and route((2, 128, 23, 23), half=False) == (not switch)
    assert not route((2, 128, 22, 23), half=True) and not route((1023, 4096, 1, 1), half=True)
    monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD_MIN_L", 126)
    assert route((2, 128, 9, 7), half=True) == switch and not route((2, 128, 9, 6), half=True)
