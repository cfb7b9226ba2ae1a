"""Depthwise / grouped streaming convs on bf16 / fp16 operands, the part that needs no GPU: the numpy rounding helper of
tests/_half_round.py pinned against torch on the CPU, the two route predicates case by case (on a stand-in "device" tensor, as
tests/test_gconv_cpu.py does), and the argument validation of the six "_h" entries with nothing launched.  The kernels themselves:
tests/test_gpu_half_streaming.py."""
import contextlib
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import _half_round as HR
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
ENTRIES = ("qt_dwconv2d_h", "qt_dwconv2d_grad_input_h", "qt_dwconv2d_grad_weight_h", "qt_gconv2d_h", "qt_gconv2d_grad_input_h",
           "qt_gconv2d_grad_weight_h")
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
P = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it
F32, BF16, F16 = (_lib.DEFINES[k] for k in ("QT_DTYPE_F32", "QT_DTYPE_BF16", "QT_DTYPE_F16"))


# ---- the rounding helper ---------------------------------------------------------------------------------------------------------

def _torch_bits(x32, fmt):
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(DTYPES[fmt]).view(torch.int16).numpy().view(np.uint16)


def _torch_up(bits, fmt):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).view(DTYPES[fmt]).float().numpy()


def _agree(x32, fmt):
    ok, n = HR.same_bits(HR.ROUND[fmt](x32), _torch_bits(x32, fmt), fmt)
    assert ok, (fmt, n)


@pytest.mark.parametrize("fmt", list(DTYPES))
def test_all_patterns_upcast_exactly_and_round_back(fmt):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    up = HR.UPCAST[fmt](bits)
    want = _torch_up(bits, fmt)
    nan = HR.is_nan(bits, fmt)
    assert np.array_equal(np.isnan(up), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(up.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    back = HR.ROUND[fmt](up)
    assert np.array_equal(back[~nan], bits[~nan]) and HR.is_nan(back[nan], fmt).all()
    _agree(up, fmt)


@pytest.mark.parametrize("fmt", list(DTYPES))
def test_every_halfway_point_of_a_few_binades_rounds_to_even(fmt):
    one, mant = HR.FORMATS[fmt]["one"], HR.FORMATS[fmt]["mant"]
    per = 1 << mant
    for first in (one - 3 * per, one, one + 7 * per, 1):          # three normal binades and the smallest (subnormal) patterns
        lo = np.arange(first, first + per, dtype=np.uint32).astype(np.uint16)
        a, b = HR.UPCAST[fmt](lo).astype(np.float64), HR.UPCAST[fmt](lo + np.uint16(1)).astype(np.float64)
        mid = ((a + b) / 2).astype(np.float32)
        assert np.array_equal(mid.astype(np.float64), (a + b) / 2)                     # the midpoints are fp32 values
        for sign in (1.0, -1.0):
            got = HR.ROUND[fmt]((sign * mid).astype(np.float32))
            even = np.where(lo & 1, lo + np.uint16(1), lo) | np.uint16(0x8000 if sign < 0 else 0)
            assert np.array_equal(got, even), fmt                                      # both parities occur: lo runs over a whole binade
            _agree((sign * mid).astype(np.float32), fmt)
            for nudge, want in ((np.float32(1 - 2.0 ** -23), lo), (np.float32(1 + 2.0 ** -23), lo + np.uint16(1))):
                if first > 1:
                    assert np.array_equal(HR.ROUND[fmt]((sign * mid * nudge).astype(np.float32)) & np.uint16(0x7FFF), want)


def test_fp16_overflow_edge_and_subnormal_range():
    r = HR.rne_fp16
    below = np.nextafter(np.float32(65520.0), np.float32(0))          # 65519.996...
    assert list(r(np.array([65504.0, below, 65520.0, -65520.0, 1e30], np.float32))) == [0x7BFF, 0x7BFF, 0x7C00, 0xFC00, 0x7C00]
    assert list(r(np.array([2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25], np.float32))) == \
        [0, 2, 1, 0x8001, 0x0400, 0x0400]
    # every multiple of 2^-26 up to 2^-13 (quarter steps of the subnormal spacing), and the fp32 subnormals
    k = np.arange(0, 1 << 13, dtype=np.float64)
    x = (k * 2.0 ** -26).astype(np.float32)
    for s in (1, -1):
        _agree(s * x, "fp16")
    tiny = np.array([1e-45, 1e-40, -1e-39, 1.17549435e-38], np.float32)
    assert list(r(tiny)) == [0, 0, 0x8000, 0] and list(HR.rne_bf16(tiny)[:1]) == [0]
    _agree(tiny, "bf16")


@pytest.mark.parametrize("fmt", list(DTYPES))
def test_specials_and_random_patterns(fmt):
    inf = HR.FORMATS[fmt]["inf"]
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    got = HR.ROUND[fmt](sp)
    assert list(got[:4]) == [0, 0x8000, inf, 0x8000 | inf] and HR.is_nan(got[4:], fmt).all()
    _agree(sp, fmt)
    rnd = np.random.RandomState(5).randint(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    _agree(rnd, fmt)
    assert float(HR.half_ulp(np.array([1.0]), fmt)[0]) == 2.0 ** -(HR.FORMATS[fmt]["mant"] + 1)


# ---- the route predicates --------------------------------------------------------------------------------------------------------

class Dev(torch.Tensor):
    is_cuda = True


def on(shape, dtype=torch.bfloat16):
    return torch.empty(shape, dtype=dtype).as_subclass(Dev)


def _layer(cin, cout, groups, dtype=torch.bfloat16):
    return types.SimpleNamespace(weight=on((cout, cin // groups, 3, 3), dtype), groups=groups, stride=(1, 1), padding=(1, 1),
                                 dilation=(1, 1), padding_mode="zeros")


@contextlib.contextmanager
def autocast_state(dtype):
    """The thread's CUDA autocast state as ``torch.autocast("cuda", dtype=dtype)`` sets it — that context manager switches
    itself off on a machine without a device, and ``_fused.half_route`` reads exactly these two values."""
    was, was_dt = torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype()
    torch.set_autocast_enabled(True)
    torch.set_autocast_gpu_dtype(dtype)
    try:
        yield
    finally:
        torch.set_autocast_enabled(was)
        torch.set_autocast_gpu_dtype(was_dt)


def _route_cases(route, layer_of, x_shape):
    """What both predicates share; ``layer_of(dtype)`` makes a layer the route takes for an input ``on(x_shape, dtype)``."""
    for dt, other in ((torch.bfloat16, torch.float16), (torch.float16, torch.bfloat16)):
        assert route(layer_of(dt), on(x_shape, dt))                                   # same half dtype
        assert not route(layer_of(torch.float32), on(x_shape, dt))                    # fp32 weight without autocast
        assert not route(layer_of(other), on(x_shape, dt))                            # two half dtypes
        with autocast_state(dt):
            assert route(layer_of(torch.float32), on(x_shape, dt))                    # ... accepted under autocast to the activation's dtype
            assert route(layer_of(dt), on(x_shape, dt))
        with autocast_state(other):
            assert not route(layer_of(torch.float32), on(x_shape, dt))                # autocast to the other half dtype
            assert not route(layer_of(dt), on(x_shape, dt))                           # a bf16 model under fp16 autocast
        assert not route(layer_of(dt), on(x_shape, torch.float32)) and not route(layer_of(dt), on(x_shape, torch.float64))
        assert not route(layer_of(dt), torch.empty(x_shape, dtype=dt))                # a CPU input
        assert not route(layer_of(dt), on(x_shape[1:], dt))                           # not 4-D
        for attr, value in (("padding_mode", "reflect"), ("padding", "same")):
            lay = layer_of(dt)
            setattr(lay, attr, value)
            assert not route(lay, on(x_shape, dt))


def test_depthwise_half_route_case_by_case(monkeypatch):
    monkeypatch.setattr(_fused, "DEPTHWISE_HALF", True)
    route = _fused.depthwise_half_route
    _route_cases(route, lambda dt: _layer(8, 8, 8, dt), (2, 8, 6, 6))
    assert route(_layer(8, 16, 8), on((2, 8, 6, 6)))                                  # multiplier 2
    assert not route(_layer(8, 8, 4), on((2, 8, 6, 6))) and not route(_layer(8, 8, 2), on((2, 8, 6, 6)))
    assert not route(_layer(8, 8, 1), on((2, 8, 6, 6)))
    assert not _fused.depthwise_route(_layer(8, 8, 8), on((2, 8, 6, 6)))              # the fp32 route keeps declining half
    monkeypatch.setattr(_fused, "DEPTHWISE_HALF", False)
    assert not route(_layer(8, 8, 8), on((2, 8, 6, 6)))


def test_grouped_half_route_case_by_case(monkeypatch):
    monkeypatch.setattr(_fused, "GROUPED_HALF_MAX_CIN_G", 4)
    route = _fused.grouped_half_route
    _route_cases(route, lambda dt: _layer(32, 32, 8, dt), (2, 32, 6, 6))
    assert route(_layer(8, 8, 4), on((2, 8, 6, 6)))                                   # groups == GROUPED_MIN_GROUPS, cin_g 2
    assert not route(_layer(8, 8, 2), on((2, 8, 6, 6))) and not route(_layer(9, 9, 3), on((2, 9, 6, 6)))      # 2 and 3 groups
    assert not route(_layer(8, 8, 8), on((2, 8, 6, 6)))                               # one channel per group: the depthwise route
    assert route(_layer(16, 8, 4), on((1, 16, 6, 6))) and not route(_layer(20, 8, 4), on((1, 20, 6, 6)))      # cin_g 4 in, 5 out
    monkeypatch.setattr(_fused, "GROUPED_HALF_MAX_CIN_G", 8)
    assert route(_layer(32, 8, 4), on((1, 32, 6, 6))) and not route(_layer(36, 8, 4), on((1, 36, 6, 6)))      # cin_g 8 in, 9 out
    monkeypatch.setattr(_fused, "GROUPED_HALF_MAX_CIN_G", 31)                          # never above GROUPED_MAX_CIN_G
    top = _fused.GROUPED_MAX_CIN_G
    assert route(_layer(4 * top, 8, 4), on((1, 4 * top, 6, 6))) and not route(_layer(4 * (top + 1), 8, 4), on((1, 4 * (top + 1), 6, 6)))
    assert not _fused.grouped_route(_layer(32, 32, 8), on((2, 32, 6, 6)))             # the fp32 route keeps declining half
    monkeypatch.setattr(_fused, "GROUPED_HALF_MAX_CIN_G", 0)
    assert not route(_layer(32, 32, 8), on((2, 32, 6, 6)))


def test_shipped_switches_are_inside_their_ranges():
    assert isinstance(_fused.DEPTHWISE_HALF, bool)
    assert _fused.GROUPED_HALF_MAX_CIN_G in (0, 4, 8) and _fused.GROUPED_HALF_MAX_CIN_G <= _fused.GROUPED_MAX_CIN_G
    assert isinstance(_fused.STREAMING_HALF_STATS, dict)


# ---- C-ABI -------------------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_with_dtype_arguments_and_bound():
    with open(_lib.HEADER_PATH, encoding="utf-8") as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(qt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    lib = _lib.load()
    for name in ENTRIES:
        assert name in protos and name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        args = [" ".join(a.split()) for a in protos[name].split(",")]
        assert "int dtype" in args and "int w_dtype" in args
        # every element-type argument is called "...dtype"; the only typed pointers left are the fp32 bias and workspace
        assert all(a.startswith(("const void*", "void*")) or a in ("const float* bias", "float* work") for a in args if "*" in a), name
    assert _lib.version() >= 302


DW_GEOM = (2, 6, 2, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1)                 # N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw
DW_XS, DW_YS = (150, 25, 5, 1), (300, 25, 5, 1)
GC_GEOM = (2, 4, 3, 2, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1)              # N, G, cin_g, cout_g, H, W, ...
GC_XS, GC_YS = (300, 25, 5, 1), (200, 25, 5, 1)
FAMILIES = (("qt_dwconv2d", DW_GEOM, DW_XS, DW_YS, "qt_dwconv2d_grad_weight_work_floats"),
            ("qt_gconv2d", GC_GEOM, GC_XS, GC_YS, "qt_gconv2d_grad_weight_work_floats"))


@pytest.mark.parametrize("fam", FAMILIES, ids=["depthwise", "grouped"])
def test_half_entries_validate_before_they_launch(fam):
    stem, geom, xs, ys, work_name = fam
    lib = _lib.load()
    fwd, gin, gwt = (getattr(lib, stem + s) for s in ("_h", "_grad_input_h", "_grad_weight_h"))
    need = getattr(lib, work_name)(*geom)
    empty = (0,) + geom[1:]
    # less than one split's partials: too small for either layout of go (the query is the larger of the two plans)
    one_split = (geom[1] * geom[2] if stem == "qt_dwconv2d" else geom[1] * geom[2] * geom[3]) * (3 * 3 + 1)
    assert need >= one_split

    def f(x=P, dt=BF16, w=P, wdt=BF16, bias=None, y=P, g=geom, xs_=xs, ys_=ys, kind=1):
        return fwd(x, dt, w, wdt, bias, y, *g, *xs_, *ys_, kind, None)

    def gi(go=P, dt=F16, w=P, wdt=F32, gx=P, g=geom, kind=0):
        return gin(go, dt, w, wdt, gx, *g, *ys, *xs, kind, None)

    def gw(go=P, x=P, dt=BF16, w=P, gw_=P, gb=None, wdt=BF16, work=P, n=need, g=geom, gs=ys, thr=1.001):
        return gwt(go, x, dt, w, gw_, gb, wdt, work, n, *g, *gs, *xs, thr, None)

    # (a call with every argument valid is never made here: it would launch)
    # unknown dtype codes come first — fp32 is not an activation dtype, the weight is the activation's type or fp32
    for call in (f, gi, gw):
        assert call(dt=F32) == INVALID and call(dt=3) == INVALID and call(dt=-1) == INVALID
        assert call(dt=BF16, wdt=F16) == INVALID and call(dt=F16, wdt=BF16) == INVALID and call(dt=BF16, wdt=7) == INVALID
        assert call(dt=7, g=empty) == INVALID
    # empty shapes: QT_OK whatever the pointers are
    assert f(x=None, w=None, y=None, g=empty) == OK and gi(go=None, w=None, gx=None, g=empty) == OK
    assert gw(go=None, x=None, w=None, gw_=None, work=None, n=0, g=empty) == OK
    # 2-byte elements need 2-byte alignment only; an odd BYTE address is misaligned, and so is an fp32 pointer off 4 bytes
    assert f(x=P + 1) == ALIGNMENT and f(y=P + 1) == ALIGNMENT and f(w=P + 1) == ALIGNMENT and f(bias=P + 2) == ALIGNMENT
    assert f(w=P + 2, wdt=F32) == ALIGNMENT
    assert gi(go=P + 1) == ALIGNMENT and gi(gx=P + 3) == ALIGNMENT and gi(w=P + 2) == ALIGNMENT          # (its w is fp32)
    assert gw(go=P + 1) == ALIGNMENT and gw(x=P + 1) == ALIGNMENT and gw(gw_=P + 1) == ALIGNMENT and gw(gb=P + 1) == ALIGNMENT
    assert gw(work=P + 2) == ALIGNMENT and gw(gw_=P + 2, wdt=F32) == ALIGNMENT
    # null tensors, kind, ste_threshold, the workspace, strides of neither dense layout
    assert f(x=None) == INVALID and f(w=None) == INVALID and f(y=None) == INVALID and f(kind=3) == INVALID
    assert gi(go=None) == INVALID and gi(kind=5) == INVALID
    assert gw(work=None) == INVALID and gw(n=one_split - 1) == INVALID and gw(thr=-1.0) == INVALID and gw(thr=float("nan")) == INVALID
    assert gw(w=None) == INVALID                                    # the mask needs the weight
    bad = (xs[0], xs[1], xs[2], 2)
    assert f(xs_=bad) == INVALID and f(ys_=(ys[0], 1, ys[2], ys[3])) == INVALID and gw(gs=bad) == INVALID
    # the limits of the fp32 entries hold
    k = 5 if stem == "qt_dwconv2d" else 6                           # where (kh, kw) sit in the geometry
    assert f(g=geom[:k] + (5, 10) + geom[k + 2:]) == UNSUPPORTED    # 50 taps
    assert ctypes.c_int64 is _lib.SIGNATURES[work_name][0]


def test_ops_keep_refusing_host_tensors_and_mixed_dtypes():
    # (constants, not draws: the suite's statistical tests further on read the global generator where the earlier tests left it)
    x, w = torch.ones(1, 4, 5, 5).bfloat16(), torch.ones(4, 1, 3, 3).bfloat16()
    with pytest.raises(TypeError):
        ops.depthwise_conv2d(x, w, None, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.grouped_conv2d(torch.ones(1, 8, 5, 5).half(), torch.ones(8, 2, 3, 3).half(), None, 1, 1, 1, 4)
    with pytest.raises(TypeError):
        ops._dw_half_codes(on((1, 4, 5, 5)), on((4, 1, 3, 3), torch.float16))
    with pytest.raises(TypeError):
        ops._dw_half_codes(on((1, 4, 5, 5), torch.float32), on((4, 1, 3, 3)))
    with pytest.raises(TypeError):
        ops._dw_half_codes(on((1, 4, 5, 5)), on((4, 1, 3, 3)), on((1, 4, 5, 5), torch.float16))
    assert ops._dw_half_codes(on((1, 4, 5, 5), torch.float32), on((4, 1, 3, 3), torch.float32)) is None
    assert ops._dw_half_codes(on((1, 4, 5, 5)), on((4, 1, 3, 3), torch.float32)) == (BF16, F32)
    assert ops._dw_half_codes(on((1, 4, 5, 5), torch.float16), on((4, 1, 3, 3), torch.float16)) == (F16, F16)
