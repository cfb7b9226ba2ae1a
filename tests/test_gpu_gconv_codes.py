"""Grouped DorefaConv2d inside the fused int8 code chain, on the GPU: the code-plane forms of csrc/gconv.hip through
ops.grouped_conv2d_codes / ops.grouped_conv2d_from_codes, layers.fused.FusedGroupedDorefaBnQuant and lazy.py under
``lazy.grouped_deferred()``.  Modelled test for test on tests/test_gpu_dw_codes.py.

The reference (tests/_gconv_codes.py) uses none of the package's packers or kernels: numpy float32 decode, tests/_gconv_exact.py's
float32 forward (the pinned order of qt_gconv2d_f32), tests/_codes_exact.py's epilogue and plane codec.  Every comparison is exact
(``torch.equal`` / ``compare_codes(designed=True)``: nothing is waived — tests/test_gconv_codes_cpu.py shows that the reference has
no sensitive element in any case); every output buffer lies between sentinels; every pad and border byte must be zero.  The input
planes carry NON-zero codes in their halo: the kernels must never read them.  All shapes are small: the file runs in a few seconds."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import _codes_exact as C
import _gconv_codes as R
import _gconv_exact as G
from test_gpu_dw_codes import (_bn, _delta, _dev, _guarded_bytes, _guarded_f32, _in_planes, _input, _intact, _run, _value,  # noqa: F401
                               _epi)
from pytorch_quantize_impls_amd import _lib, lazy, ops, packed, utils
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import DorefaConv2d, FusedDorefaConvBnQuant, FusedGroupedDorefaBnQuant
from pytorch_quantize_impls_amd.utils import implicit

pytestmark = pytest.mark.gpu

CODES, F32, EAGER, EXPAND = "qt_gconv2d_codes", "qt_gconv2d_codes_f32", "qt_gconv2d_f32", "qt_codes_to_f32"
DW_CODES = "qt_dwconv2d_codes"
MISMATCHED = {"bytes": 0, "waived": 0, "planes": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _w(dev, r):
    return _dev(dev, r.w)


def _run_codes(dev, r, shape, groups, geometry, in_halo, out_halo, in_bits, out_bits, relu):
    """One launch into a guarded plane; returns (the plane on the host, the flag value, the CodePlanes)."""
    N, Cc, H, W = shape
    kernel, stride, padding, dilation = geometry
    Cout = r.w.shape[0]
    Ho, Wo = G.out_hw(H, W, kernel, stride, padding, dilation)
    x = _in_planes(dev, r.q, in_halo, r.inv_n, in_bits)
    rows = N * (Ho + 2 * out_halo[0]) * (Wo + 2 * out_halo[1])
    buf, out = _guarded_bytes(dev, rows, C.code_ld(Cout))
    before = _lib.call_counts.get(CODES, 0)
    got = ops.grouped_conv2d_codes(x, shape, _w(dev, r), _dev(dev, r.b), _epi(dev, r, out_bits, relu, out_halo), stride, padding,
                                   dilation, groups, in_halo=in_halo, out=out)
    assert _lib.call_counts[CODES] == before + 1 and _intact(buf)
    assert got.codes is out and (got.rows, got.K, got.bit_width) == (rows, Cout, out_bits) and got.overflow is x.overflow
    assert got.inv_n == ops.inv_levels(out_bits)
    return out.cpu(), int(got.overflow.item()), got


def _check(plane, ref, N, Ho, Wo, Cout, out_halo, what):
    C.check_plane_zeros(plane, N, Ho, Wo, Cout, out_halo, what)
    got = C.decode_plane(plane, N, Ho, Wo, Cout, out_halo, what).permute(0, 2, 3, 1)
    waived, msg = C.compare_codes(got, ref, designed=True, what=what)
    want = R.out_plane(ref, out_halo)
    MISMATCHED["bytes"] += int((plane != want).sum())
    MISMATCHED["waived"] += waived
    MISMATCHED["planes"] += 1
    assert waived == 0 and msg == "", msg
    assert torch.equal(plane, want), what                                        # ... byte for byte


def _shape(c):
    return (c.N, c.G * c.cin_g, c.H, c.W)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[c.id for c in R.CASES])
def test_code_plane_in_code_plane_out(dev, i):
    c, r = R.CASES[i], R.build(i)
    Cout = c.G * c.cout_g
    Ho, Wo = G.out_hw(c.H, c.W, *R.geom(c))
    plane, flag, _ = _run_codes(dev, r, _shape(c), c.G, R.geom(c), c.in_halo, c.out_halo, c.in_bits, c.out_bits, c.relu)
    _check(plane, r.ref, c.N, Ho, Wo, Cout, c.out_halo, c.id)
    assert flag == r.ref["flag_head"]
    # the other halos of the output: the same codes in another frame
    other = R.HALOS[(R.HALOS.index(c.out_halo) + 1) % 3]
    plane, _, _ = _run_codes(dev, r, _shape(c), c.G, R.geom(c), c.in_halo, other, c.in_bits, c.out_bits, c.relu)
    _check(plane, r.ref, c.N, Ho, Wo, Cout, other, c.id + f" out_halo {other}")


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[c.id for c in R.CASES])
def test_code_plane_in_fp32_out_in_both_layouts(dev, i):
    c, r = R.CASES[i], R.build(i)
    shape = _shape(c)
    w, b = _w(dev, r), _dev(dev, r.b)
    x = _in_planes(dev, r.q, c.in_halo, r.inv_n, c.in_bits)
    want = torch.from_numpy(r.ref["y"])
    # inside the package: the fp32 entry on the expanded image
    image = packed.CodeActivation(_in_planes(dev, r.q, (0, 0), r.inv_n, c.in_bits), shape).float()
    assert torch.equal(image.cpu(), torch.from_numpy(R.image(r.q, r.inv_n)))
    eager = ops.grouped_conv2d(image, w, b, c.stride, c.padding, c.dilation, c.G)
    args = (c.stride, c.padding, c.dilation, c.G)
    for layout in ("nchw", "channels_last"):
        buf, out = _guarded_f32(dev, tuple(want.shape), layout)
        before = _lib.call_counts.get(F32, 0)
        y = ops.grouped_conv2d_from_codes(x, shape, w, b, *args, in_halo=c.in_halo, out=out)
        assert y is out and _intact(buf) and _lib.call_counts[F32] == before + 1
        assert torch.equal(y.cpu(), want), layout
        assert torch.equal(y, eager), layout
    y = ops.grouped_conv2d_from_codes(x, shape, w, b, *args, in_halo=c.in_halo)
    assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y.cpu(), want)
    y = ops.grouped_conv2d_from_codes(x, shape, w, b, *args, in_halo=c.in_halo, channels_last=False)
    assert y.is_contiguous() and torch.equal(y.cpu(), want)
    # a raised flag of the chain: every output NaN, decided on the device
    x.overflow.fill_(1)
    for layout in ("nchw", "channels_last"):
        buf, out = _guarded_f32(dev, tuple(want.shape), layout)
        y = ops.grouped_conv2d_from_codes(x, shape, w, b, *args, in_halo=c.in_halo, out=out)
        assert bool(torch.isnan(y).all()) and _intact(buf)
    y = ops.grouped_conv2d_from_codes(x, shape, w, b, *args, in_halo=c.in_halo, flagged=False)
    assert torch.equal(y.cpu(), want)


def test_every_compared_plane_matched_byte_for_byte():
    """The module's own tally, printed for the record: zero mismatching bytes, zero waived elements.  It is informational — it counts
    what the tests above compared in this process (nothing, if it runs alone); each of them asserts ``torch.equal`` itself."""
    print(f"GCONV-CODES planes={MISMATCHED['planes']} mismatching_bytes={MISMATCHED['bytes']} waived={MISMATCHED['waived']}")
    assert MISMATCHED["bytes"] == 0 and MISMATCHED["waived"] == 0


def test_designed_codes_on_rint_ties_and_on_the_relu_boundary(dev):
    d = R.designed()
    assert d.cin_g == 4 and d.ties >= 1 and d.on_relu >= 1
    Ho, Wo = G.out_hw(d.H, d.W, *d.geometry)
    for in_halo, out_halo in (((0, 0), (1, 1)), ((2, 1), (0, 0))):
        plane, flag, _ = _run_codes(dev, d, (d.N, d.G * d.cin_g, d.H, d.W), d.G, d.geometry, in_halo, out_halo, 4, 4, True)
        _check(plane, d.ref, d.N, Ho, Wo, d.G * d.cout_g, out_halo, "designed")
        assert flag == 0


def test_overflow_flag_values(dev):
    """|q| > 127 stores code 0 and raises flag value 1; a huge BatchNorm weight (|q| > 2047) raises 3; a clear flag stays 0."""
    c, r = R.CASES[0], R.build(0)
    shape, Cout = _shape(c), c.G * c.cout_g
    Ho, Wo = G.out_hw(c.H, c.W, *R.geom(c))
    assert not r.ref["flag"]
    plane, flag, _ = _run_codes(dev, r, shape, c.G, R.geom(c), (0, 0), (0, 0), c.in_bits, c.out_bits, c.relu)
    assert flag == 0
    for scale, want_flag in ((200.0, 1), (1e6, 3)):
        alpha = r.alpha * scale
        epi = C.Epi(alpha=alpha, beta=r.beta, levels=r.epi.levels, stats=r.stats, relu=r.epi.relu)
        ref = R.reference(r.q, r.inv_n, r.w, r.b, c.G, R.geom(c), epi)
        assert ref["flag"] and ref["flag_head"] == want_flag, (scale, ref["flag_head"])
        big = R.Case(q=r.q, w=r.w, b=r.b, alpha=alpha, beta=r.beta, stats=r.stats, inv_n=r.inv_n)
        plane, flag, _ = _run_codes(dev, big, shape, c.G, R.geom(c), (1, 1), (1, 1), c.in_bits, c.out_bits, c.relu)
        _check(plane, ref, c.N, Ho, Wo, Cout, (1, 1), f"overflow x{scale}")
        assert flag == want_flag
        out_of_range = ~(C.quantise(ref["t"], r.epi.levels)[1])
        assert bool(out_of_range.any()) and int(ref["codes"][out_of_range].abs().sum()) == 0
    # the flag is shared: a plane produced behind a raised flag keeps it raised
    x = _in_planes(dev, r.q, (0, 0), r.inv_n, c.in_bits, flag=torch.full((1,), 1, dtype=torch.int32, device=dev))
    got = ops.grouped_conv2d_codes(x, shape, _w(dev, r), _dev(dev, r.b), _epi(dev, r, c.out_bits, c.relu, (0, 0)), c.stride, c.padding,
                                   c.dilation, c.G)
    assert got.overflow is x.overflow and int(got.overflow.item()) == 1


@pytest.mark.parametrize("i", [i for i, c in enumerate(R.CASES) if c.cin_g == 1])
def test_one_channel_per_group_gives_the_bytes_of_the_depthwise_entry(dev, i):
    c, r = R.CASES[i], R.build(i)
    shape = _shape(c)
    w, b = _w(dev, r), _dev(dev, r.b)
    for out_halo in R.HALOS:
        x = _in_planes(dev, r.q, c.in_halo, r.inv_n, c.in_bits)
        epi = _epi(dev, r, c.out_bits, c.relu, out_halo)
        b0, b1 = _lib.call_counts.get(CODES, 0), _lib.call_counts.get(DW_CODES, 0)
        g = ops.grouped_conv2d_codes(x, shape, w, b, epi, c.stride, c.padding, c.dilation, c.G, in_halo=c.in_halo)
        d = ops.depthwise_conv2d_codes(x, shape, w, b, epi, c.stride, c.padding, c.dilation, in_halo=c.in_halo)
        assert _lib.call_counts[CODES] == b0 + 1 and _lib.call_counts[DW_CODES] == b1 + 1
        assert g.codes.shape == d.codes.shape and torch.equal(g.codes, d.codes)
    yg = ops.grouped_conv2d_from_codes(x, shape, w, b, c.stride, c.padding, c.dilation, c.G, in_halo=c.in_halo)
    yd = ops.depthwise_conv2d_from_codes(x, shape, w, b, c.stride, c.padding, c.dilation, in_halo=c.in_halo)
    assert torch.equal(yg, yd)


def test_wrappers_check_their_operands(dev):
    c, r = R.CASES[1], R.build(1)
    shape = _shape(c)
    x = _in_planes(dev, r.q, (0, 0), r.inv_n, c.in_bits)
    w = _w(dev, r)
    good = _epi(dev, r, 4, True, (0, 0))
    args = (c.stride, c.padding, c.dilation, c.G)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, None, w, None, good, *args)                                     # no logical shape
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, shape, w, None, good, *args, in_halo=(1, 1))                    # the plane has no halo
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, shape, w, None, _epi(dev, r, 4, "pre", (0, 0)), *args)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, shape, w, None, _epi(dev, r, 9, True, (0, 0)), *args)
    res = _epi(dev, r, 4, True, (0, 0))
    res.res_codes = x
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, shape, w, None, res, *args)                                     # no residual
    with pytest.raises(TypeError):
        ops.grouped_conv2d_codes(x, shape, w, None, (good.alpha, good.beta), *args)
    with pytest.raises(TypeError):
        ops.grouped_conv2d_codes(x, shape, w, None, ops.CodeEpilogue(good.alpha.cpu(), good.beta, 4), *args)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, shape, w, None, ops.CodeEpilogue(good.alpha[:-1], good.beta, 4), *args)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, shape, w, None, good, c.stride, c.padding, c.dilation, 2)       # groups do not fit the weight
    with pytest.raises(ValueError):
        ops.grouped_conv2d_from_codes(x, shape, _dev(dev, np.zeros((16, 4, 5, 10), np.float32)), None, 1, 5, 1, c.G)      # 50 taps
    with pytest.raises(ValueError):
        ops.grouped_conv2d_codes(x, shape, w, None, good, *args, out=torch.empty((3, 16), dtype=torch.int8, device=dev))
    # an empty batch: a plane of zero rows, nothing launched
    before = _lib.call_counts.get(CODES, 0)
    empty = ops.CodePlanes(codes=x.codes[:0], rows=0, K=shape[1], inv_n=x.inv_n, bit_width=4)
    out = ops.grouped_conv2d_codes(empty, (0,) + shape[1:], w, None, good, *args)
    assert out.codes.shape[0] == 0 and _lib.call_counts.get(CODES, 0) == before


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_c_abi_validates_in_the_documented_order_and_takes_the_empty_problem(dev):
    lib = _lib.load()
    OK, INVALID, ALIGN, UNSUPPORTED = 0, -1, -2, -4
    N, Gg, ci, co, H, W = 2, 4, 4, 4, 6, 5
    Cin, Cout = Gg * ci, Gg * co
    x = torch.full((N * H * W * 16 + 64,), 3, dtype=torch.int8, device=dev)
    w = torch.ones((Cout * ci * 9 + 4,), device=dev)
    vec = torch.ones((2 * Cout + 4,), device=dev)
    flag = torch.zeros((4,), dtype=torch.int32, device=dev)
    out = torch.full((N * H * W * 16 + 64,), 0x5A, dtype=torch.int8, device=dev)
    y = torch.full((N * Cout * H * W + 16,), 12345.0, device=dev)
    P = ctypes.c_void_p
    base = dict(x=x.data_ptr(), ldx=16, ihy=0, ihx=0, inv_n=0.25, w=w.data_ptr(), bias=vec.data_ptr(), alpha=vec.data_ptr(),
                beta=vec.data_ptr(), stats=None, relu=1, bits=4, codes=out.data_ptr(), ldc=16, ohy=0, ohx=0, flag=flag.data_ptr(),
                N=N, G=Gg, ci=ci, co=co, H=H, W=W, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, y=y.data_ptr())

    def codes(**kw):
        a = dict(base, **kw)
        return lib.qt_gconv2d_codes(P(a["x"]), a["ldx"], a["ihy"], a["ihx"], ctypes.c_float(a["inv_n"]), P(a["w"]), P(a["bias"]),
                                    P(a["alpha"]), P(a["beta"]), P(a["stats"]), a["relu"], a["bits"], P(a["codes"]), a["ldc"], a["ohy"],
                                    a["ohx"], P(a["flag"]), a["N"], a["G"], a["ci"], a["co"], a["H"], a["W"], a["kh"], a["kw"], a["sh"],
                                    a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], None)

    def f32(**kw):
        a = dict(base, **kw)
        Ho, Wo = a["H"], a["W"]
        s = a.get("ys", (Cout * Ho * Wo, Ho * Wo, Wo, 1))
        return lib.qt_gconv2d_codes_f32(P(a["x"]), a["ldx"], a["ihy"], a["ihx"], ctypes.c_float(a["inv_n"]), P(a["w"]), P(a["bias"]),
                                        P(a["flag"]), P(a["y"]), a["N"], a["G"], a["ci"], a["co"], a["H"], a["W"], a["kh"], a["kw"],
                                        a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], *s, None)

    for fn in (codes, f32):
        # 1. a negative halo and the sizes come first, whatever else is wrong
        assert fn(ihy=-1, x=None, ldx=3) == INVALID and fn(co=0, x=None) == INVALID and fn(sh=0, w=None) == INVALID
        assert fn(kh=5, kw=10, x=None) == UNSUPPORTED                           # 50 taps
        # 2. the empty problem: QT_OK whatever the pointers are
        assert fn(N=0, x=None, w=None, codes=None, y=None, ldx=1) == OK and fn(G=0, x=None) == OK and fn(H=0, w=None) == OK
        # 3. the limits in front of the pointers
        assert fn(ci=33, x=None) == UNSUPPORTED and fn(ci=32, G=1, kh=5, kw=5, ph=2, pw=2, x=None) == UNSUPPORTED     # K = 800
        assert fn(ihy=65, x=None) == UNSUPPORTED and fn(kh=9, kw=1, ph=0, x=None) == INVALID    # the kernel does not fit the image
        # 4. pointers, bounds, then alignment
        assert fn(x=None) == INVALID and fn(w=None) == INVALID and fn(ldx=15) == INVALID and fn(ldx=0, w=w.data_ptr() + 2) == INVALID
        assert fn(w=w.data_ptr() + 2) == ALIGN and fn(bias=vec.data_ptr() + 1) == ALIGN
        assert fn(ldx=24) == ALIGN and fn(x=x.data_ptr() + 8, ldx=16) == ALIGN
        assert fn(bias=None) == OK
    assert codes(ohx=-1) == INVALID and codes(ohy=65, codes=None) == UNSUPPORTED and codes(ldc=1 << 31, codes=None) == UNSUPPORTED
    assert codes(bits=1) == INVALID and codes(bits=9) == INVALID and codes(relu=2) == INVALID and codes(relu=-1) == INVALID
    assert codes(alpha=None) == INVALID and codes(beta=None) == INVALID and codes(codes=None) == INVALID and codes(flag=None) == INVALID
    assert codes(ldc=8) == INVALID and codes(ldc=24) == ALIGN and codes(codes=out.data_ptr() + 4) == ALIGN
    assert codes(flag=flag.data_ptr() + 2) == ALIGN and codes(stats=vec.data_ptr() + 2) == ALIGN
    assert codes(stats=vec.data_ptr()) == OK and codes(ci=1, G=16, co=1) == OK
    assert f32(y=None) == INVALID and f32(ys=(1, 2, 3, 4)) == INVALID and f32(y=y.data_ptr() + 2) == ALIGN
    assert f32(flag=None) == OK and f32(ys=(H * W * Cout, 1, W * Cout, Cout)) == OK
    torch.cuda.synchronize()
    # nothing above wrote past the problem, and the empty problems wrote nothing: the tails still hold their fill
    assert bool((out[N * H * W * 16:] == 0x5A).all()) and bool((y[N * Cout * H * W:] == 12345.0).all())
    fresh = torch.full((64,), 0x5A, dtype=torch.int8, device=dev)
    assert codes(N=0, codes=fresh.data_ptr()) == OK
    torch.cuda.synchronize()
    assert bool((fresh == 0x5A).all())


# ---- module level ----------------------------------------------------------------------------------------------------------------

class _Net(nn.Module):
    """stem fp32 conv -> BN -> ReLU -> quant -> [pw -> run -> grouped 3x3 -> run] x 2 -> pw -> run -> avg_pool -> Linear: un-modified
    modules; the first grouped layer has 8 groups of 4 channels, the second 5 groups of 8 and stride 2."""

    def __init__(self, g, g_bits=1, pool=False):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), *_run(16, g))
        mods = [DorefaConv2d(16, 32, 1, bit_width=1), *_run(32, g),
                DorefaConv2d(32, 32, 3, padding=1, groups=8, bit_width=g_bits), *_run(32, g),
                DorefaConv2d(32, 40, 1, bit_width=1), *_run(40, g)]
        if pool:
            mods.append(nn.MaxPool2d(2))
        mods += [DorefaConv2d(40, 40, 3, stride=2, padding=1, groups=5, bit_width=g_bits), *_run(40, g),
                 DorefaConv2d(40, 48, 1, bit_width=1), *_run(48, g)]
        self.body = nn.Sequential(*mods)
        self.pool = pool
        self.fc = nn.Linear(48, 10)

    def forward(self, x):
        y = self.body(self.stem(x))
        return self.fc(torch.nn.functional.avg_pool2d(y, y.shape[-1]).flatten(1))


def _net(dev, seed=5, **kw):
    torch.manual_seed(seed)
    net = _Net(torch.Generator().manual_seed(seed), **kw)
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, DorefaConv2d):
            m.weight.data.copy_(torch.randn(m.weight.shape, generator=g) * 0.6)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net.to(dev).to(memory_format=torch.channels_last).eval()


@pytest.fixture(autouse=True)
def _fresh_stats():
    start = (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES, lazy.DEFER_CODES)
    lazy.STATS.clear()
    _fused.LIBRARY_PATHS.clear()
    yield
    assert (lazy.DEFER_GROUPED, lazy.DEFER_GROUPED_CODES, lazy.DEFER_CODES) == start


@pytest.mark.parametrize("g_bits", (1, 3))
def test_unmodified_stack_stays_on_code_planes(dev, g_bits):
    net, x = _net(dev, seed=5 + g_bits, g_bits=g_bits), _input(dev)
    assert net.body[4].bit_width == g_bits and net.body[4]._eval_on_grid()
    with torch.no_grad(), lazy.grouped_deferred(True):
        with lazy.eager():
            e = net(x)
        assert type(e) is torch.Tensor and e.shape == (2, 10) and bool(torch.isfinite(e).all())
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = net(x)
        stats, after = dict(lazy.STATS), dict(_lib.call_counts)
    assert torch.equal(got, e)
    # five DoReFa convs deferred, one fused block per conv, nothing materialised between the stem quantiser and the head: the
    # average pool reads the last chain's codes
    assert stats.get("deferred") == 5 and stats.get("fused") == 5 and stats.get("materialised", 0) == 0, stats
    assert stats.get("avg_pool_on_codes") == 1 and not [k for k in stats if k.startswith("fallback")], stats
    assert _delta(after, before, CODES) == 2 and _delta(after, before, EAGER) == 0 and _delta(after, before, F32) == 0
    # no code-to-fp32 launch between the stem quantiser and the head: the one there is is the head's average pool, which reads the
    # last chain's codes
    assert _delta(after, before, EXPAND) == 1
    assert _delta(after, before, "qt_conv2d_implicit_codes") == 3
    assert not _fused.LIBRARY_PATHS, _fused.LIBRARY_PATHS


def test_switch_off_is_the_module_by_module_grouped_path(dev):
    net, x = _net(dev), _input(dev)
    with torch.no_grad():
        with lazy.eager():
            e = net(x)
        with lazy.grouped_deferred(False):
            lazy.STATS.clear()
            before = dict(_lib.call_counts)
            got = net(x)
            stats, after = dict(lazy.STATS), dict(_lib.call_counts)
        with lazy.grouped_deferred(True):
            on = net(x)
        # the new switch alone decides: the sign families' switch may stay on
        with lazy.grouped_deferred(True):
            lazy.DEFER_GROUPED_CODES = False
            before2 = dict(_lib.call_counts)
            got2 = net(x)
            after2 = dict(_lib.call_counts)
            lazy.DEFER_GROUPED_CODES = True
        # ... and it needs DEFER_CODES
        with lazy.grouped_deferred(True), lazy.codes_deferred(False):
            before3 = dict(_lib.call_counts)
            got3 = net(x)
            after3 = dict(_lib.call_counts)
    assert torch.equal(got, e) and torch.equal(on, e) and torch.equal(got2, e) and torch.equal(got3, e)
    # the three pointwise convs still defer; each grouped layer runs qt_gconv2d_f32 on an fp32 image and un-fuses its neighbours
    assert stats.get("deferred") == 3, stats
    for a, b in ((after, before), (after2, before2), (after3, before3)):
        assert _delta(a, b, EAGER) == 2 and _delta(a, b, CODES) == 0 and _delta(a, b, F32) == 0
    # each grouped layer has its producer's codes expanded to an fp32 image; the third expansion is the head's average pool
    for a, b in ((after, before), (after2, before2)):
        assert _delta(a, b, EXPAND) == 3 and _delta(a, b, "qt_conv2d_implicit_codes") == 3
    assert not _fused.LIBRARY_PATHS, _fused.LIBRARY_PATHS


def test_maxpool_behind_the_quantiser_runs_on_codes(dev):
    net, x = _net(dev, seed=7, pool=True), _input(dev, 3)
    with torch.no_grad(), lazy.grouped_deferred(True):
        with lazy.eager():
            e = net(x)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = net(x)
        after = dict(_lib.call_counts)
    assert torch.equal(got, e)
    assert lazy.STATS["fused"] == 5 and lazy.STATS.get("materialised", 0) == 0, lazy.STATS
    assert _delta(after, before, "qt_pool_codes_i8") == 1 and _delta(after, before, CODES) == 2 and _delta(after, before, EAGER) == 0


def test_grouped_root_read_by_another_consumer_materialises_from_codes(dev):
    net = _net(dev, seed=11)
    b = net.body
    x = _input(dev, 5, n=3)
    with torch.no_grad(), lazy.grouped_deferred(True):
        # behind a deferred pointwise chain: the grouped conv's input is a code plane
        head = nn.Sequential(net.stem, *b[:6])                              # ... pw -> run -> g -> BatchNorm
        with lazy.eager():
            e_bn = head(x)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        y = head(x)
        assert isinstance(y, lazy.LazyActivation) and isinstance(y._qt.input, packed.CodeActivation)
        got = torch.sigmoid(y)                                              # not in the grammar: conv from the codes, BatchNorm replayed
        after = dict(_lib.call_counts)
        assert torch.equal(got, torch.sigmoid(e_bn))
        assert _delta(after, before, F32) == 1 and _delta(after, before, EAGER) == 0 and _delta(after, before, CODES) == 0
        assert lazy.STATS["materialised"] >= 1
        # the second grouped layer (stride 2) read directly
        mid = nn.Sequential(net.stem, *b[:13])
        with lazy.eager():
            e_mid = mid(x)
        before = dict(_lib.call_counts)
        got = mid(x) * 1.0
        after = dict(_lib.call_counts)
        assert type(got) is torch.Tensor and torch.equal(got, e_mid)
        assert _delta(after, before, F32) == 1 and _delta(after, before, CODES) == 1 and _delta(after, before, EAGER) == 0
        # on the code TAG of an fp32 tensor: the grouped conv defers on the tag, and its result takes the tensor's layout
        # (CodeActivation.source_channels_last).  nnDorefaQuant tags its channels-last result; the same image in NCHW storage
        # carrying the same codes (packed.attach_codes) is the NCHW arm
        gl = DorefaConv2d(16, 24, 3, padding=1, groups=4, bit_width=1).to(dev).eval()
        tail = nn.Sequential(*_run(24, torch.Generator().manual_seed(3))).to(dev).eval()
        q_cl = net.stem(x)
        tag = packed.lookup_codes(q_cl, packed.NHWC)
        assert tag is not None and ops._dw_channels_last(q_cl)
        q_nchw = packed.attach_codes(q_cl.contiguous(memory_format=torch.contiguous_format), tag, packed.NHWC)
        assert q_nchw.is_contiguous() and not ops._dw_channels_last(q_nchw) and torch.equal(q_nchw, q_cl)
        for q, cl in ((q_cl, True), (q_nchw, False)):
            assert packed.lookup_codes(q, packed.NHWC) is not None
            with lazy.eager():
                e_tag = gl(q)
                e_tail = tail(e_tag)
            assert type(e_tag) is torch.Tensor and ops._dw_channels_last(e_tag) is cl
            before = dict(_lib.call_counts)
            yt = gl(q)
            assert isinstance(yt, lazy.LazyActivation) and yt._qt.input.source_channels_last is cl
            gt = yt * 1.0
            after = dict(_lib.call_counts)
            assert torch.equal(gt, e_tag) and gt.stride() == e_tag.stride() and ops._dw_channels_last(gt) is cl
            assert _delta(after, before, F32) == 1 and _delta(after, before, EAGER) == 0 and _delta(after, before, CODES) == 0
            # ... and the chain behind it runs fused from the tag's codes (the BatchNorm probe has the module graph's layout)
            before = dict(_lib.call_counts)
            got = tail(gl(q)) * 1.0
            after = dict(_lib.call_counts)
            assert torch.equal(got, e_tail)
            assert _delta(after, before, CODES) == 1 and _delta(after, before, EAGER) == 0 and _delta(after, before, F32) == 0


class _Residual(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        b = self.net.body
        q = b[3](b[2](b[1](b[0](self.net.stem(x)))))
        t = b[5](b[4](q)) + q                                             # an add behind a grouped BatchNorm
        return b[11](b[10](b[9](b[8](b[7](b[6](t))))))


def test_add_behind_a_grouped_batchnorm_falls_back_and_equals_eager(dev):
    m, x = _Residual(_net(dev, seed=13)), _input(dev, 6)
    with torch.no_grad(), lazy.grouped_deferred(True):
        with lazy.eager():
            e = m(x)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = _value(m(x))
        after = dict(_lib.call_counts)
    assert torch.equal(got, e)
    assert lazy.STATS["materialised"] >= 1 and _delta(after, before, F32) == 1 and _delta(after, before, CODES) == 0, lazy.STATS


def test_explicit_fused_form_equals_the_deferred_graph_and_replays_in_a_hipgraph(dev):
    net, x = _net(dev, seed=15), _input(dev, 7)
    b = net.body
    with torch.no_grad(), lazy.grouped_deferred(True):
        q = b[3](b[2](b[1](b[0](net.stem(x)))))
        assert isinstance(q, lazy.LazyActivation)
        act = q._qt.force((0, 0))
        assert isinstance(act, packed.CodeActivation)
        tag = act.codes
        # the deferred graph's codes of g -> BN -> ReLU -> quant -> pw -> BN -> ReLU -> quant
        y = b[11](b[10](b[9](b[8](b[7](b[6](b[5](b[4](q))))))))
        assert isinstance(y, lazy.LazyActivation)
        want = y._qt.force((0, 0))
        gc = FusedGroupedDorefaBnQuant(b[4], b[5], 4, relu=True, out_halo=0, fold="device")
        pw = FusedDorefaConvBnQuant(b[8], b[9], 4, relu=True, out_halo=0, fold="device")
        before = dict(_lib.call_counts)
        got = pw(gc(act))
        assert _delta(dict(_lib.call_counts), before, CODES) == 1
        assert got.shape == want.shape and torch.equal(got.codes.codes, want.codes.codes)
        assert int(got.codes.overflow.item()) == 0
        # with a halo for a consumer that pads: the same codes inside a zero border
        gc2 = FusedGroupedDorefaBnQuant(b[4], b[5], 4, relu=True, out_halo=(2, 1), fold="device")
        mid, mid2 = gc(act), gc2(act)
        assert mid2.halo == (2, 1) and torch.equal(mid2.without_halo().codes.codes, mid.codes.codes)
        # one capture and replay of the explicit form (no parallel branches); the folds are cached, nothing asks the host
        static = tag.codes.clone()
        sact = packed.CodeActivation(ops.CodePlanes(codes=static, rows=tag.rows, K=tag.K, inv_n=tag.inv_n, bit_width=tag.bit_width,
                                                    overflow=tag.overflow), tuple(act.shape))
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            pw(gc(sact))
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = pw(gc(sact))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.codes.codes, want.codes.codes)
        act2 = b[3](b[2](b[1](b[0](net.stem(_input(dev, 8))))))._qt.force((0, 0))
        static.copy_(act2.codes.codes)
        graph.replay()
        torch.cuda.synchronize()
        want2 = pw(gc(act2))
        assert torch.equal(out.codes.codes, want2.codes.codes) and not torch.equal(want2.codes.codes, want.codes.codes)


def test_stack_replays_from_the_default_implicit_hipgraph_and_equals_eager(dev, monkeypatch):
    """The same stack the way a user calls it: twice eagerly, captured in the third call, replayed from then on."""
    monkeypatch.setattr(implicit, "KEEP_IF_FASTER", 0.0)              # no test may depend on the clock
    net = _net(dev, seed=19, g_bits=3)
    x, x2 = _input(dev, 9), _input(dev, 10)
    with lazy.grouped_deferred(True), utils.implicit_graphs(True):
        with torch.no_grad(), utils.implicit_graphs(False), lazy.eager():
            want, want2 = net(x).clone(), net(x2).clone()
        assert bool(torch.isfinite(want).all()) and not torch.equal(want, want2)
        counts = []
        with torch.no_grad():
            for i in range(5):
                assert ("forward" in net.__dict__) == (i >= 2), (i, utils.implicit_graph_stats(net))
                before = dict(_lib.call_counts)
                y = net(x)
                after = dict(_lib.call_counts)
                counts.append({k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)})
                assert type(y) is torch.Tensor and torch.equal(y, want), i
            # (the capturing call runs the forward more than once: two launches of the grouped entry each time)
            assert counts[2].get(CODES, 0) >= 2 and counts[2].get(CODES, 0) % 2 == 0 and counts[2].get(EAGER, 0) == 0, counts[2]
            assert counts[3] == {} and counts[4] == {}, ("a replay issued launches from the host", counts[3], counts[4])
            assert torch.equal(net(x2), want2) and torch.equal(net(x), want)          # fresh data through the same graph
        st = utils.implicit_graph_stats(net)
        assert st["wrapped"] and st["graphs"] == 1 and st["value_mismatch"] == 0 and st["capture_failures"] == {}, st


def test_dorefa_can_defer_admits_the_grouped_route_only(dev):
    mk = lambda *a, **k: DorefaConv2d(*a, **k).to(dev).eval()          # noqa: E731
    g8 = mk(32, 32, 3, padding=1, groups=8, bit_width=3)               # cin_g = 4
    g2 = mk(16, 16, 3, padding=1, groups=2, bit_width=1)
    g3 = mk(24, 24, 3, padding=1, groups=3, bit_width=1)
    c16 = mk(64, 64, 3, padding=1, groups=4, bit_width=1)              # cin_g = 16
    c2, c8 = mk(8, 8, 1, groups=4, bit_width=1), mk(32, 68, 3, padding=1, groups=4, bit_width=1)
    k50 = mk(32, 32, (5, 10), padding=5, groups=8, bit_width=1)
    dwl = mk(16, 16, 3, padding=1, groups=16, bit_width=1)
    same = mk(32, 32, 3, padding="same", groups=8, bit_width=1)
    S = lazy._CodeShapeOnly
    with torch.no_grad():
        with lazy.grouped_deferred(True):
            assert lazy._dorefa_can_defer(g8, S((1, 32, 12, 12))) and lazy._dorefa_can_defer(c2, S((1, 8, 5, 5)))
            assert lazy._dorefa_can_defer(c8, S((2, 32, 7, 9)))
            assert not lazy._dorefa_can_defer(g8, S((1, 32, 0, 12))) and not lazy._dorefa_can_defer(g8, S((1, 16, 12, 12)))
            assert not lazy._dorefa_can_defer(g2, S((1, 16, 12, 12))) and not lazy._dorefa_can_defer(g3, S((1, 24, 12, 12)))
            assert not lazy._dorefa_can_defer(c16, S((1, 64, 12, 12))) and not lazy._dorefa_can_defer(k50, S((1, 32, 12, 12)))
            assert not lazy._dorefa_can_defer(same, S((1, 32, 12, 12)))
            with lazy.codes_deferred(False):
                assert not lazy._dorefa_can_defer(g8, S((1, 32, 12, 12)))          # both switches are needed
            with lazy.depthwise_deferred(False):                                    # the depthwise switch is another one
                assert lazy._dorefa_can_defer(g8, S((1, 32, 12, 12))) and not lazy._dorefa_can_defer(dwl, S((1, 16, 12, 12)))
            blk = FusedGroupedDorefaBnQuant(g8, nn.BatchNorm2d(32).to(dev).eval(), 4)
            g8.weight.data.mul_(0.37)                                               # off the quantiser's grid
            g8.reset_quant_cache()
            assert not g8._eval_on_grid() and not lazy._dorefa_can_defer(g8, S((1, 32, 12, 12)))
            planes = ops.CodePlanes(codes=torch.zeros((25, 32), dtype=torch.int8, device=dev), rows=25, K=32, inv_n=1.0 / 15, bit_width=4)
            with pytest.raises(ValueError):
                blk(packed.CodeActivation(planes, (1, 32, 5, 5)))                   # the block declines it as well
        with lazy.grouped_deferred(False):
            assert not lazy._dorefa_can_defer(c8, S((2, 32, 7, 9))) and not lazy._dorefa_can_defer(c2, S((1, 8, 5, 5)))
            with lazy.depthwise_deferred(True):
                assert lazy._dorefa_can_defer(dwl, S((1, 16, 12, 12)))
