"""Residual blocks of the sign chain, the host side: qt_bn_add_sign_f32 is declared in the header, bound from it and validates before
it launches; ``lazy.residual_deferred`` restores itself; ``FusedConvBnAddSign`` declines what it cannot run; and on CPU tensors
nothing defers and a Bi-Real block computes what plain torch computes, whatever the switch says.  The kernel and the chains:
tests/test_gpu_resid_sign.py, tests/test_gpu_resid_chain.py."""
from ctypes import c_float, c_int, c_int64, c_void_p

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from pytorch_quantize_impls_amd import _lib, lazy, ops
from pytorch_quantize_impls_amd.functions import BinaryConnect
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, XNORConv2d
from pytorch_quantize_impls_amd.layers.fused import FusedConvBnAddSign

ENTRY = "qt_bn_add_sign_f32"
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
PTR = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it


def test_entry_is_declared_in_the_header_and_bound():
    assert ENTRY in _lib.header_declared_functions() and ENTRY in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    want = ([c_void_p, c_int64] + [c_void_p] * 4 + [c_int64] * 4 + [c_int, c_float, c_float] + [c_void_p] + [c_int64] * 4
            + [c_void_p, c_int64] * 2 + [c_int64] * 6 + [c_void_p])
    assert restype is c_int and argtypes == want and len(argtypes) == 29
    names = [n for n, _ in _lib.HEADER.functions[ENTRY][1]]
    assert names == ["x", "ldx", "weight", "bias", "bn_stats", "r", "rs_n", "rs_c", "rs_h", "rs_w", "hardtanh", "lo", "hi", "sum", "ss_n", "ss_c",
                     "ss_h", "ss_w", "sign_plane", "ldb", "nib_plane", "ldn", "out_halo_h", "out_halo_w", "N", "C", "Ho", "Wo", "stream"]
    assert getattr(_lib.load(), ENTRY).argtypes == argtypes


def _call(lib, **kw):
    a = dict(x=PTR, ldx=40, weight=PTR, bias=PTR, stats=PTR, r=PTR, rs=(1000, 25, 5, 1), ht=1, lo=-1.0, hi=1.0, sum=PTR + 0x100000,
             lds=40, sign=PTR + 0x200000, ldb=4, nib=PTR + 0x300000, ldn=8, hy=1, hx=1, N=2, C=40, H=5, W=5)
    a.update(kw)
    lds = a["lds"]
    ss = a.get("ss") or (a["H"] * a["W"] * lds, 1, a["W"] * lds, lds)          # the sum as rows with a pitch, unless ``ss`` says otherwise
    return getattr(lib, ENTRY)(a["x"], a["ldx"], a["weight"], a["bias"], a["stats"], a["r"], *a["rs"], a["ht"], a["lo"], a["hi"],
                               a["sum"], *ss, a["sign"], a["ldb"], a["nib"], a["ldn"], a["hy"], a["hx"], a["N"], a["C"], a["H"],
                               a["W"], None)


def test_entry_validates_before_it_launches():
    """The header's order: negative sizes, empty problems, limits, arguments, alignment (C = 40: packed_ld 4, pixel_ld_nib 8)."""
    lib = _lib.load()
    for k in ("N", "C", "H", "W", "hy", "hx"):
        assert _call(lib, **{k: -1}) == INVALID
    assert _call(lib, N=0, hy=-1) == INVALID                                            # the halo's sign is looked at first
    for k in ("N", "C", "H", "W"):
        assert _call(lib, **{k: 0}, x=None, r=None, weight=None, sum=None, sign=None, nib=None) == OK
    assert _call(lib, hy=65) == UNSUPPORTED and _call(lib, hx=65) == UNSUPPORTED
    assert _call(lib, hy=65, x=None) == UNSUPPORTED                                     # limits before arguments
    assert _call(lib, N=1 << 20, H=1 << 6, W=1 << 5) == UNSUPPORTED                     # 2^31 pixel rows
    for k in ("x", "weight", "bias", "stats", "r"):
        assert _call(lib, **{k: None}) == INVALID
    assert _call(lib, sum=None, sign=None, nib=None) == INVALID
    assert _call(lib, ht=2) == INVALID and _call(lib, ht=-1) == INVALID
    assert _call(lib, lo=1.0, hi=-1.0) == INVALID and _call(lib, hi=float("nan")) == INVALID
    assert _call(lib, ldx=39) == INVALID and _call(lib, lds=39) == INVALID
    assert _call(lib, rs=(1000, 25, 5, 2)) == INVALID and _call(lib, rs=(975, 1, 195, 39)) == INVALID
    assert _call(lib, ldb=3) == INVALID and _call(lib, ldn=4) == INVALID
    assert _call(lib, sum=PTR + 16) == INVALID and _call(lib, sum=PTR, lds=44) == INVALID          # overlap that is not "in place"
    nchw = (1000, 25, 5, 1)
    assert _call(lib, ss=(1000, 25, 5, 2)) == INVALID and _call(lib, sum=PTR, ss=nchw) == INVALID   # no dense form; NCHW over x
    assert _call(lib, sum=None, ss=(1, 2, 3, 4), x=PTR + 2) == ALIGNMENT                            # strides of an absent sum are not read
    assert _call(lib, sum=PTR + 0x100002, ss=nchw) == ALIGNMENT
    assert _call(lib, x=None, sum=PTR + 2) == INVALID                                   # arguments before alignment
    for k in ("x", "weight", "bias", "stats", "r"):
        assert _call(lib, **{k: PTR + 2}) == ALIGNMENT
    assert _call(lib, sum=PTR + 0x100002) == ALIGNMENT and _call(lib, sign=PTR + 0x200001) == ALIGNMENT
    assert _call(lib, nib=PTR + 0x300004) == ALIGNMENT and _call(lib, ldn=10) == ALIGNMENT
    assert _call(lib, sign=None, ldb=0, ldn=4) == INVALID and _call(lib, nib=None, ldn=0, ldb=3) == INVALID


def test_wrapper_rejects_host_tensors():
    x2, v, r = torch.zeros(50, 8), torch.ones(8), torch.zeros(2, 8, 5, 5)
    with pytest.raises(TypeError):
        ops.bn_add_sign(x2, (2, 8, 5, 5), v, v, torch.ones(16), r)


def test_residual_deferred_restores_the_previous_setting():
    start = lazy.DEFER_RESIDUAL_SIGN
    with lazy.residual_deferred():
        assert lazy.DEFER_RESIDUAL_SIGN is True
        with lazy.residual_deferred(False):
            assert lazy.DEFER_RESIDUAL_SIGN is False
        assert lazy.DEFER_RESIDUAL_SIGN is True
    assert lazy.DEFER_RESIDUAL_SIGN is start
    with pytest.raises(KeyError):
        with lazy.residual_deferred(not start):
            assert lazy.DEFER_RESIDUAL_SIGN is (not start)
            raise KeyError("x")
    assert lazy.DEFER_RESIDUAL_SIGN is start
    assert "DEFER_RESIDUAL_SIGN" in lazy.__doc__ and "residual_deferred" in lazy.__doc__


def test_block_declines_what_it_cannot_run():
    bn = nn.BatchNorm2d(8)
    ok = FusedConvBnAddSign(BinConv2d(8, 8, 3, padding=1), bn, hardtanh=nn.Hardtanh())
    assert ok.hardtanh == (-1.0, 1.0) and ok.fold == "device" and ok.out_nib_halo is None
    assert FusedConvBnAddSign(TerConv2d(8, 8, 3, padding=1, groups=8), bn, (-0.5, 2.0), fold="device").hardtanh == (-0.5, 2.0)
    for conv, b, kw in ((BinConv2d(8, 8, 3, padding=1, deterministic=False), bn, {}),                 # the stochastic forms
                        (TerConv2d(8, 8, 3, padding=1, deterministic=False), bn, {}),
                        (XNORConv2d(8, 8, 3, padding=1), bn, {}),
                        (nn.Conv2d(8, 8, 3, padding=1), bn, {}),
                        (BinConv2d(8, 8, 3, padding="same"), bn, {}),
                        (BinConv2d(8, 8, 3, padding=1), nn.MaxPool2d(2), {}),                         # a pool in front of the BatchNorm
                        (BinConv2d(8, 8, 3, padding=1), nn.BatchNorm2d(4), {}),
                        (BinConv2d(8, 8, 3, padding=1), nn.BatchNorm1d(8), {}),
                        (BinConv2d(8, 8, 3, padding=1).half(), bn, {}),                               # half dtypes
                        (BinConv2d(8, 8, 3, padding=1), bn, {"hardtanh": (0.5, 1.0)}),
                        (BinConv2d(8, 8, 3, padding=1), bn, {"fold": "reference"})):
        with pytest.raises(ValueError):
            FusedConvBnAddSign(conv, b, **kw)
    x = torch.randn(1, 8, 4, 4)
    with pytest.raises(RuntimeError):
        ok(x, x)                                                                         # training mode
    ok.eval()
    with pytest.raises(TypeError):
        ok(x, x)                                                                         # a host tensor
    ok.refold()


@pytest.mark.parametrize("conv_t", (BinConv2d, TerConv2d))
def test_on_cpu_tensors_nothing_defers_and_results_are_unchanged(conv_t):
    torch.manual_seed(0)
    conv, bn = conv_t(8, 8, 3, padding=1).eval(), nn.BatchNorm2d(8).eval()
    bn.running_mean.normal_(), bn.running_var.uniform_(0.5, 2.0)
    sign = BinaryConnect()
    x = torch.randn(2, 8, 6, 6)
    results = []
    for on in (True, False):
        lazy.STATS.clear()
        with torch.no_grad(), lazy.residual_deferred(on):
            c = conv(sign(x))
            assert type(c) is torch.Tensor
            s = bn(c) + x
            s += x
            results.append(F.hardtanh(s))
        assert type(s) is torch.Tensor and not lazy.STATS.get("deferred") and not lazy.STATS.get("residual_sign_fused")
    want = F.hardtanh(F.batch_norm(F.conv2d(torch.where(x < 0, -1.0, 1.0), conv.weight, conv.bias, 1, 1), bn.running_mean, bn.running_var,
                                   bn.weight, bn.bias, False, 0.0, bn.eps) + x + x)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], want)
