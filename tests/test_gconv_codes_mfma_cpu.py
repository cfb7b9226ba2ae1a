"""Grouped DorefaConv2d with 16 / 32 input channels per group on code planes, the host side: the two entries of
csrc/gconv_codes_mfma.hip exist and validate in the documented order before they launch, ``ops.grouped_mfma_codes_applicable`` on its
boundary shapes, ``FusedGroupedMfmaDorefaBnQuant`` declines what it cannot run, ``lazy.grouped_mfma_deferred`` sets and restores both
of its switches, and host layers never defer.  The kernel: tests/test_gpu_gconv_codes_mfma.py."""
import pytest
import torch
import torch.nn as nn

from pytorch_quantize_impls_amd import _lib, lazy, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import DorefaConv2d, FusedGroupedDorefaBnQuant, FusedGroupedMfmaDorefaBnQuant

OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
PTR = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it


def _codes(lib, **kw):
    """G = 8 groups of 16 -> 128 input and output channels."""
    a = dict(x=PTR, ldx=128, ihy=1, ihx=1, inv_n=1.0 / 15, w=PTR, bias=None, alpha=PTR, beta=PTR, stats=None, relu=1, bits=4, codes=PTR,
             ldc=128, ohy=1, ohx=1, flag=PTR, N=2, G=8, ci=16, co=16, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1,
             ws=PTR, wb=1)
    a.update(kw)
    return lib.qt_gmconv2d_codes(a["x"], a["ldx"], a["ihy"], a["ihx"], a["inv_n"], a["w"], a["bias"], a["alpha"], a["beta"], a["stats"],
                                 a["relu"], a["bits"], a["codes"], a["ldc"], a["ohy"], a["ohx"], a["flag"], a["N"], a["G"], a["ci"],
                                 a["co"], a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"],
                                 a["ws"], a["wb"], None)


def _f32(lib, **kw):
    a = dict(x=PTR, ldx=128, ihy=0, ihx=0, inv_n=1.0 / 15, w=PTR, bias=None, flag=None, y=PTR, N=2, G=8, ci=16, co=16, H=5, W=5, kh=3,
             kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, ys=(3200, 25, 5, 1), ws=PTR, wb=1)
    a.update(kw)
    return lib.qt_gmconv2d_codes_f32(a["x"], a["ldx"], a["ihy"], a["ihx"], a["inv_n"], a["w"], a["bias"], a["flag"], a["y"], a["N"],
                                     a["G"], a["ci"], a["co"], a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"],
                                     a["dh"], a["dw"], *a["ys"], a["ws"], a["wb"], None)


def test_entries_are_declared_in_the_header_and_bound():
    declared = _lib.header_declared_functions()
    lib = _lib.load()
    for name, sibling in (("qt_gmconv2d_codes", "qt_gconv2d_codes"), ("qt_gmconv2d_codes_f32", "qt_gconv2d_codes_f32")):
        assert name in declared and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        # the sibling's list plus (w_scale, w_bits) in front of the stream
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[sibling][1]) + 2


@pytest.mark.parametrize("fn", (_codes, _f32), ids=("codes", "f32"))
def test_entries_validate_in_the_documented_order_before_they_launch(fn):
    lib = _lib.load()
    # 1. signs come first, whatever else is wrong
    assert fn(lib, ihy=-1, x=None, ci=24) == INVALID and fn(lib, N=-1, ci=24) == INVALID and fn(lib, sh=0, x=None) == INVALID
    assert fn(lib, co=0) == INVALID and fn(lib, ph=-1) == INVALID
    # 2. the empty problem, whatever the pointers and the window
    assert fn(lib, N=0, x=None, w=None, ci=24) == OK and fn(lib, G=0, x=None) == OK and fn(lib, H=0, x=None) == OK
    # 3. the window in front of the pointers
    for kw in (dict(G=4), dict(ci=8), dict(ci=24), dict(ci=64), dict(co=8), dict(co=64), dict(kh=5, kw=5, ph=2, pw=2), dict(kh=3, kw=1),
               dict(sh=3, sw=3), dict(sh=1, sw=2), dict(dh=2, dw=2), dict(ph=2), dict(ihy=65), dict(N=1 << 22, H=1 << 5, W=1 << 5)):
        assert fn(lib, x=None, **kw) == UNSUPPORTED, kw
    assert fn(lib, H=1, W=1, ph=0, pw=0, x=None) == INVALID                    # the kernel does not fit the image
    for kw in (dict(ci=32, co=48), dict(kh=1, kw=1, ph=0, pw=0, sh=2, sw=2), dict(ph=0, pw=1)):
        assert fn(lib, w=None, **kw) == INVALID, kw                           # inside the window: on to the pointers
    # 4. pointers and bounds, then alignment
    assert fn(lib, x=None) == INVALID and fn(lib, w=None) == INVALID and fn(lib, ldx=112) == INVALID
    assert fn(lib, wb=0) == INVALID and fn(lib, wb=8) == INVALID and fn(lib, wb=1, ws=None) == INVALID
    assert fn(lib, w=PTR + 2) == ALIGNMENT and fn(lib, bias=PTR + 1) == ALIGNMENT and fn(lib, ws=PTR + 2) == ALIGNMENT
    assert fn(lib, ldx=136) == ALIGNMENT and fn(lib, x=PTR + 8) == ALIGNMENT


def test_each_entry_checks_its_own_output_form():
    lib = _lib.load()
    assert _codes(lib, ohx=-1) == INVALID and _codes(lib, ohy=65, codes=None) == UNSUPPORTED
    assert _codes(lib, ldc=1 << 31, codes=None) == UNSUPPORTED
    assert _codes(lib, bits=1) == INVALID and _codes(lib, bits=9) == INVALID and _codes(lib, relu=2) == INVALID
    assert _codes(lib, alpha=None) == INVALID and _codes(lib, codes=None) == INVALID and _codes(lib, flag=None) == INVALID
    assert _codes(lib, ldc=112) == INVALID and _codes(lib, ldc=136) == ALIGNMENT and _codes(lib, codes=PTR + 4) == ALIGNMENT
    assert _codes(lib, stats=PTR + 2) == ALIGNMENT and _codes(lib, flag=PTR + 2) == ALIGNMENT
    assert _f32(lib, y=None) == INVALID and _f32(lib, ys=(1, 2, 3, 4)) == INVALID and _f32(lib, y=PTR + 2) == ALIGNMENT
    assert _f32(lib, flag=PTR + 2) == ALIGNMENT


def test_applicable_on_its_boundary_shapes():
    ok = ops.grouped_mfma_codes_applicable
    x, g = (2, 128, 9, 9), 8
    assert ok(x, (128, 16, 3, 3), 1, 1, 1, g) and ok(x, (384, 16, 3, 3), 2, 1, 1, g) and ok(x, (128, 16, 1, 1), 1, 0, 1, g)
    assert ok((2, 256, 9, 9), (256, 32, 3, 3), 1, (0, 1), 1, g)
    assert not ok((2, 192, 9, 9), (192, 24, 3, 3), 1, 1, 1, g)             # 24 channels per group: the fp32 route only
    assert not ok((2, 64, 9, 9), (64, 8, 3, 3), 1, 1, 1, g) and not ok((2, 512, 9, 9), (512, 64, 3, 3), 1, 1, 1, g)
    assert not ok(x, (64, 16, 3, 3), 1, 1, 1, g) and not ok(x, (512, 16, 3, 3), 1, 1, 1, g)      # cout_g 8, 64
    assert not ok(x, (128, 16, 5, 5), 1, 2, 1, g) and not ok(x, (128, 16, 3, 3), 3, 1, 1, g)
    assert not ok(x, (128, 16, 3, 3), (1, 2), 1, 1, g) and not ok(x, (128, 16, 3, 3), 1, 2, 1, g)
    assert not ok(x, (128, 16, 3, 3), 1, 1, 2, g)
    assert ops.GMC_CIN_G == (16, 32) and ops.GMC_COUT_G == (16, 32, 48)


def _conv(groups=8, cin_g=16, bits=1, **kw):
    return DorefaConv2d(groups * cin_g, groups * cin_g, 3, padding=1, groups=groups, bit_width=bits, **kw).eval()


def test_block_declines_what_it_cannot_run():
    bn = nn.BatchNorm2d(128).eval()
    blk = FusedGroupedMfmaDorefaBnQuant(_conv(), bn, 4)
    assert blk.bit_width == 4 and blk.relu == 1
    FusedGroupedMfmaDorefaBnQuant(_conv(bits=7), bn, 4, relu=False)
    with pytest.raises(ValueError):
        FusedGroupedMfmaDorefaBnQuant(_conv(groups=4, cin_g=32), bn, 4)                   # fewer than 8 groups
    with pytest.raises(ValueError):
        FusedGroupedMfmaDorefaBnQuant(_conv(bits=8), bn, 4)
    with pytest.raises(ValueError):
        FusedGroupedMfmaDorefaBnQuant(_conv(groups=8, cin_g=24), nn.BatchNorm2d(192).eval(), 4)
    with pytest.raises(ValueError):
        FusedGroupedMfmaDorefaBnQuant(_conv(), bn, 4, relu="pre")
    with pytest.raises(ValueError):
        FusedGroupedDorefaBnQuant(_conv(), bn, 4)                                         # the sibling keeps declining 16 per group
    with pytest.raises(ValueError):
        blk(object(), residual=torch.zeros(1))


def test_switch_pair_is_set_and_restored_and_host_layers_never_defer():
    start = (lazy.DEFER_GROUPED_MFMA, lazy.DEFER_GROUPED_MFMA_CODES)
    for on in (True, False):
        with lazy.grouped_mfma_deferred(on):
            assert (lazy.DEFER_GROUPED_MFMA, lazy.DEFER_GROUPED_MFMA_CODES) == (on, on)
        assert (lazy.DEFER_GROUPED_MFMA, lazy.DEFER_GROUPED_MFMA_CODES) == start
    conv = _conv()
    assert _fused._grouped_mfma_codes_window(conv, (2, 128, 6, 6)) and not _fused._grouped_mfma_codes_window(_conv(bits=8), (2, 128, 6, 6))
    assert not _fused._grouped_mfma_codes_window(_conv(groups=4, cin_g=16), (2, 64, 6, 6))
    x = torch.randn(2, 128, 6, 6)
    with torch.no_grad(), lazy.grouped_mfma_deferred(True):
        lazy.STATS.clear()
        y = conv(x)
        assert type(y) is torch.Tensor and lazy.STATS.get("deferred", 0) == 0
        assert _fused.dorefa_grouped_mfma_codes_forward(conv, x) is None
        assert torch.equal(y, torch.nn.functional.conv2d(x, conv.weight, conv.bias, 1, 1, 1, 8))
