"""The matrix-core weight gradient of the grouped convs with 16, 24 or 32 channels per group, the host side: the C-ABI entry
validates before it launches, its workspace size, and the route choice of ``GroupedMfmaConv2dFn.backward``.  The kernel itself:
tests/test_gpu_gconv_mfma_wgrad.py."""
import pytest

from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused

OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
P = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it
XS, YS = (8 * 16 * 25, 25, 5, 1), (8 * 32 * 25, 25, 5, 1)
GEOM = ("N", "G", "cin_g", "cout_g", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw")


def _args(**kw):
    a = dict(go=P, x=P, w=P, gw=P, gbias=P, work=P, N=2, G=8, cin_g=16, cout_g=32, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1,
             dw=1, xs=XS, ys=YS, ste=1.001)
    a.update(kw)
    return a, tuple(a[k] for k in GEOM)


def _need(**kw):
    return _lib.load().qt_gmconv2d_grad_weight_work_floats(*_args(**kw)[1])


def _call(**kw):
    a, geom = _args(**kw)
    floats = a["floats"] if "floats" in a else max(_need(**kw), 0)
    return _lib.load().qt_gmconv2d_grad_weight_f32(a["go"], a["x"], a["w"], a["gw"], a["gbias"], a["work"], floats, *geom, *a["ys"],
                                                   *a["xs"], a["ste"], None)


def test_entry_validates_before_it_launches():
    call = _call
    for name in ("go", "x", "gw", "work", "w"):                   # w only because the mask is on
        assert call(**{name: None}) == INVALID, name
    assert call(ste=-1.0) == INVALID and call(ste=float("nan")) == INVALID and call(floats=-1) == INVALID
    # 1. sizes below their minimum are INVALID even where a limit is broken too
    assert call(N=-1) == INVALID and call(cin_g=0) == INVALID and call(cout_g=0) == INVALID and call(sh=0) == INVALID
    assert call(ph=-1) == INVALID and call(dw=0) == INVALID and call(N=-1, cin_g=20) == INVALID
    assert call(kh=5, kw=10) == UNSUPPORTED
    # 2. an empty problem is OK whatever the pointers and the limits are, and needs no workspace
    assert call(N=0, go=None, x=None, gw=None, work=None) == OK and call(G=0, go=None) == OK and call(H=0, cin_g=20, go=None) == OK
    assert _need(N=0) == 0 and _need(G=0) == 0 and _need(W=0, cin_g=20) == 0
    # 3. the limits before pointers and strides
    for bad in (dict(cin_g=8), dict(cin_g=20), dict(cin_g=40), dict(cout_g=24), dict(cout_g=64), dict(kh=5, kw=5, ph=2, pw=2),
                dict(dh=2, dw=2), dict(sh=3, sw=3), dict(sh=2, sw=1), dict(ph=2), dict(kh=1, kw=3), dict(N=1 << 24)):
        assert call(ste=-1.0, go=None, **bad) == UNSUPPORTED and _need(**bad) == UNSUPPORTED, bad
    assert call(H=1, W=1, ph=0, pw=0, go=None) == INVALID and _need(H=1, W=1, ph=0, pw=0) == INVALID      # the kernel does not fit
    # 4. strides, the workspace, alignment
    assert call(xs=(3200, 25, 5, 2)) == INVALID and call(ys=XS) == INVALID
    need = _need()
    assert need == 2 * 8 * (9 * 32 * 16 + 32)                     # two one-tile images: two splits
    assert call(floats=need - 1) == INVALID and call(floats=need - 1, work=P + 4) == INVALID
    for name, off in (("go", 2), ("x", 1), ("gw", 2), ("gbias", 1), ("w", 3), ("work", 4)):       # the partials are float4 stores
        assert call(**{name: P + off}) == ALIGNMENT, name

    # the documented cap on splits per group (1024 / G would be more), and 1024 workgroups at 32 groups
    cap, block = _lib.DEFINES["QT_GM_WGRAD_MAX_SPLITS"], 9 * 16 * 16 + 16
    assert cap == ops.GM_WGRAD_MAX_SPLITS == 128 and _need(N=256, G=1, cout_g=16, H=14, W=14) == cap * block
    assert ops.grouped_mfma_grad_weight_work_floats((256, 512, 14, 14), (512, 16, 3, 3), 1, 1, 1, 32) == 32 * 32 * block


@pytest.mark.parametrize("switch", (True, False))
def test_wgrad_route_is_a_function_of_the_switch_and_the_reduction_length(monkeypatch, switch):
    monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD", switch)
    route = _fused.grouped_mfma_wgrad_route
    assert _fused.GROUPED_MFMA_WGRAD_MIN_L == 1024
    assert route((2, 128, 23, 23)) == switch and route((1024, 128, 1, 1)) == switch and route((256, 512, 14, 14)) == switch
    assert not route((2, 128, 22, 23)) and not route((1023, 4096, 1, 1)) and not route((2, 128, 9, 7))
    monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD_MIN_L", 126)
    assert route((2, 128, 9, 7)) == switch and not route((2, 128, 9, 6))
