"""Depthwise DorefaConv2d inside the fused int8 code chain, on the GPU: the code-plane forms of csrc/dwconv.hip through
ops.depthwise_conv2d_codes / ops.depthwise_conv2d_from_codes, layers.fused.FusedDepthwiseDorefaBnQuant and lazy.py under
``lazy.depthwise_deferred()``.

The reference (tests/_dw_codes.py) uses none of the package's packers or kernels: numpy float32 decode, tests/_dw_exact.py's float32
forward (which reproduces qt_dwconv2d_f32 bit for bit), tests/_codes_exact.py's epilogue and plane codec.  Every comparison is exact
(``torch.equal`` / ``compare_codes(designed=True)``: nothing is waived — tests/test_dw_codes_cpu.py shows that the reference has no
sensitive element in any case); every output buffer lies between sentinels; every pad and border byte must be zero.  The input
planes carry NON-zero codes in their halo: the kernels must never read them.  All shapes are small: the file runs in a few seconds."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _codes_exact as C
import _dw_codes as R
import _dw_exact as D
from pytorch_quantize_impls_amd import _lib, lazy, ops, packed, utils
from pytorch_quantize_impls_amd.functions import _fused, nnDorefaQuant
from pytorch_quantize_impls_amd.layers import DorefaConv2d, FusedDepthwiseDorefaBnQuant, FusedDorefaConvBnQuant

pytestmark = pytest.mark.gpu

SENTINEL_B = 0x5A
SENTINEL_F = 12345.0
PAD = 256                    # elements: the guarded views stay 16-byte aligned
HALO_JUNK = 77               # what the halo pixels of every input plane hold
CODES, F32, EAGER = "qt_dwconv2d_codes", "qt_dwconv2d_codes_f32", "qt_dwconv2d_f32"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _dev(dev, a):
    if a is None:
        return None
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(dev)


def _guarded_bytes(dev, rows, ld):
    buf = torch.full((rows * ld + 2 * PAD,), SENTINEL_B, dtype=torch.int8, device=dev)
    return buf, buf[PAD:PAD + rows * ld].view(rows, ld)


def _guarded_f32(dev, shape, layout):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL_F, dtype=torch.float32, device=dev)
    mid = buf[PAD:PAD + n]
    if layout == "channels_last":
        N, Cc, H, W = shape
        return buf, mid.view(N, H, W, Cc).permute(0, 3, 1, 2)
    return buf, mid.view(*shape)


def _intact(buf):
    v = SENTINEL_B if buf.dtype == torch.int8 else SENTINEL_F
    return bool((buf[:PAD] == v).all() and (buf[-PAD:] == v).all())


def _in_planes(dev, q, halo, inv_n, bits=4, flag=None):
    """ops.CodePlanes of the codes q [N, C, H, W], encoded by the reference's codec, with junk in the halo pixels."""
    N, Cc, H, W = q.shape
    hy, hx = halo
    plane = C.encode_plane(torch.from_numpy(q), halo)
    p4 = plane.view(N, H + 2 * hy, W + 2 * hx, -1)
    keep = p4[:, hy:hy + H, hx:hx + W].clone()
    p4[...] = HALO_JUNK
    p4[:, hy:hy + H, hx:hx + W] = keep
    flag = torch.zeros((1,), dtype=torch.int32, device=dev) if flag is None else flag
    return ops.CodePlanes(codes=plane.to(dev), rows=int(plane.shape[0]), K=Cc, inv_n=float(inv_n), bit_width=bits, overflow=flag)


def _epi(dev, r, bits, relu, out_halo, flag=None):
    stats = None if r.stats is None else torch.cat([r.stats[0], r.stats[1]]).to(dev)
    return ops.CodeEpilogue(_dev(dev, r.alpha), _dev(dev, r.beta), bits, relu, out_halo=out_halo, bn_stats=stats, overflow=flag)


def _run_codes(dev, r, shape, geometry, in_halo, out_halo, in_bits, out_bits, relu):
    """One launch into a guarded plane; returns (the plane on the host, the flag value, the CodePlanes)."""
    N, Cc, H, W = shape
    kernel, stride, padding, dilation = geometry
    Cout = r.w.shape[0]
    Ho, Wo = D.out_hw(H, W, kernel, stride, padding, dilation)
    x = _in_planes(dev, r.q, in_halo, r.inv_n, in_bits)
    rows = N * (Ho + 2 * out_halo[0]) * (Wo + 2 * out_halo[1])
    buf, out = _guarded_bytes(dev, rows, C.code_ld(Cout))
    before = _lib.call_counts.get(CODES, 0)
    got = ops.depthwise_conv2d_codes(x, shape, _dev(dev, r.w).unsqueeze(1), _dev(dev, r.b), _epi(dev, r, out_bits, relu, out_halo),
                                     stride, padding, dilation, in_halo=in_halo, out=out)
    assert _lib.call_counts[CODES] == before + 1 and _intact(buf)
    assert got.codes is out and (got.rows, got.K, got.bit_width) == (rows, Cout, out_bits) and got.overflow is x.overflow
    assert got.inv_n == ops.inv_levels(out_bits)
    return out.cpu(), int(got.overflow.item()), got


def _check(plane, ref, N, Ho, Wo, Cout, out_halo, what):
    C.check_plane_zeros(plane, N, Ho, Wo, Cout, out_halo, what)
    got = C.decode_plane(plane, N, Ho, Wo, Cout, out_halo, what).permute(0, 2, 3, 1)
    waived, msg = C.compare_codes(got, ref, designed=True, what=what)
    assert waived == 0 and msg == "", msg
    assert torch.equal(plane, R.out_plane(ref, out_halo)), what                  # ... byte for byte


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[c.id for c in R.CASES])
def test_code_plane_in_code_plane_out(dev, i):
    c, r = R.CASES[i], R.build(i)
    Cout = c.C * c.m
    Ho, Wo = D.out_hw(c.H, c.W, *R.geom(c))
    plane, flag, _ = _run_codes(dev, r, (c.N, c.C, c.H, c.W), R.geom(c), c.in_halo, c.out_halo, c.in_bits, c.out_bits, c.relu)
    _check(plane, r.ref, c.N, Ho, Wo, Cout, c.out_halo, c.id)
    assert flag == r.ref["flag_head"]
    # the other halos of the output: the same codes in another frame
    other = R.HALOS[(R.HALOS.index(c.out_halo) + 1) % 3]
    plane, _, _ = _run_codes(dev, r, (c.N, c.C, c.H, c.W), R.geom(c), c.in_halo, other, c.in_bits, c.out_bits, c.relu)
    _check(plane, r.ref, c.N, Ho, Wo, Cout, other, c.id + f" out_halo {other}")


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[c.id for c in R.CASES])
def test_code_plane_in_fp32_out_in_both_layouts(dev, i):
    c, r = R.CASES[i], R.build(i)
    shape = (c.N, c.C, c.H, c.W)
    w, b = _dev(dev, r.w).unsqueeze(1), _dev(dev, r.b)
    x = _in_planes(dev, r.q, c.in_halo, r.inv_n, c.in_bits)
    want = torch.from_numpy(r.ref["y"])
    # inside the package: the fp32 entry on the expanded image
    image = packed.CodeActivation(_in_planes(dev, r.q, (0, 0), r.inv_n, c.in_bits), shape).float()
    assert torch.equal(image.cpu(), torch.from_numpy(R.image(r.q, r.inv_n)))
    eager = ops.depthwise_conv2d(image, w, b, c.stride, c.padding, c.dilation)
    for layout in ("nchw", "channels_last"):
        buf, out = _guarded_f32(dev, tuple(want.shape), layout)
        before = _lib.call_counts.get(F32, 0)
        y = ops.depthwise_conv2d_from_codes(x, shape, w, b, c.stride, c.padding, c.dilation, in_halo=c.in_halo, out=out)
        assert y is out and _intact(buf) and _lib.call_counts[F32] == before + 1
        assert torch.equal(y.cpu(), want), layout
        assert torch.equal(y, eager), layout
    y = ops.depthwise_conv2d_from_codes(x, shape, w, b, c.stride, c.padding, c.dilation, in_halo=c.in_halo)
    assert y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y.cpu(), want)
    y = ops.depthwise_conv2d_from_codes(x, shape, w, b, c.stride, c.padding, c.dilation, in_halo=c.in_halo, channels_last=False)
    assert y.is_contiguous() and torch.equal(y.cpu(), want)
    # a raised flag of the chain: every output NaN, decided on the device
    x.overflow.fill_(1)
    for layout in ("nchw", "channels_last"):
        buf, out = _guarded_f32(dev, tuple(want.shape), layout)
        y = ops.depthwise_conv2d_from_codes(x, shape, w, b, c.stride, c.padding, c.dilation, in_halo=c.in_halo, out=out)
        assert bool(torch.isnan(y).all()) and _intact(buf)
    y = ops.depthwise_conv2d_from_codes(x, shape, w, b, c.stride, c.padding, c.dilation, in_halo=c.in_halo, flagged=False)
    assert torch.equal(y.cpu(), want)


def test_designed_codes_on_rint_ties_and_on_the_relu_boundary(dev):
    d = R.designed()
    assert d.ties >= 8 and d.on_relu >= 8
    Ho, Wo = D.out_hw(d.H, d.W, *d.geometry)
    for in_halo, out_halo in (((0, 0), (1, 1)), ((2, 1), (0, 0))):
        plane, flag, _ = _run_codes(dev, d, (d.N, d.C, d.H, d.W), d.geometry, in_halo, out_halo, 4, 4, True)
        _check(plane, d.ref, d.N, Ho, Wo, d.C * d.m, out_halo, "designed")
        assert flag == 0


def test_overflow_flag_values(dev):
    """|q| > 127 stores code 0 and raises flag value 1; a huge BatchNorm weight (|q| > 2047) raises 3; a clear flag stays 0."""
    c, r = R.CASES[0], R.build(0)
    shape, Cout = (c.N, c.C, c.H, c.W), c.C * c.m
    Ho, Wo = D.out_hw(c.H, c.W, *R.geom(c))
    assert not r.ref["flag"]
    plane, flag, _ = _run_codes(dev, r, shape, R.geom(c), (0, 0), (0, 0), c.in_bits, c.out_bits, c.relu)
    assert flag == 0
    for scale, want_flag in ((60.0, 1), (1e6, 3)):
        alpha = r.alpha * scale
        epi = C.Epi(alpha=alpha, beta=r.beta, levels=r.epi.levels, stats=r.stats, relu=r.epi.relu)
        ref = R.reference(r.q, r.inv_n, r.w, r.b, R.geom(c), epi)
        assert ref["flag"] and ref["flag_head"] == want_flag
        big = R.Case(q=r.q, w=r.w, b=r.b, alpha=alpha, beta=r.beta, stats=r.stats, inv_n=r.inv_n)
        plane, flag, _ = _run_codes(dev, big, shape, R.geom(c), (1, 1), (1, 1), c.in_bits, c.out_bits, c.relu)
        _check(plane, ref, c.N, Ho, Wo, Cout, (1, 1), f"overflow x{scale}")
        assert flag == want_flag
        out_of_range = ~(C.quantise(ref["t"], r.epi.levels)[1])
        assert bool(out_of_range.any()) and int(ref["codes"][out_of_range].abs().sum()) == 0
    # the flag is shared: a plane produced behind a raised flag keeps it raised
    x = _in_planes(dev, r.q, (0, 0), r.inv_n, c.in_bits, flag=torch.full((1,), 1, dtype=torch.int32, device=dev))
    got = ops.depthwise_conv2d_codes(x, shape, _dev(dev, r.w).unsqueeze(1), _dev(dev, r.b), _epi(dev, r, c.out_bits, c.relu, (0, 0)),
                                     c.stride, c.padding, c.dilation)
    assert got.overflow is x.overflow and int(got.overflow.item()) == 1


def test_wrappers_check_their_operands(dev):
    c, r = R.CASES[1], R.build(1)
    shape = (c.N, c.C, c.H, c.W)
    x = _in_planes(dev, r.q, (0, 0), r.inv_n, c.in_bits)
    w = _dev(dev, r.w).unsqueeze(1)
    good = _epi(dev, r, 4, True, (0, 0))
    args = (c.stride, c.padding, c.dilation)
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_codes(x, None, w, None, good, *args)                                   # no logical shape
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_codes(x, shape, w, None, good, *args, in_halo=(1, 1))                  # the plane has no halo
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_codes(x, shape, w, None, _epi(dev, r, 4, "pre", (0, 0)), *args)
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_codes(x, shape, w, None, _epi(dev, r, 9, True, (0, 0)), *args)
    res = _epi(dev, r, 4, True, (0, 0))
    res.res_codes = x
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_codes(x, shape, w, None, res, *args)                                   # no residual
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_codes(x, shape, w, None, (good.alpha, good.beta), *args)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_codes(x, shape, w, None, ops.CodeEpilogue(good.alpha.cpu(), good.beta, 4), *args)
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_codes(x, shape, w, None, ops.CodeEpilogue(good.alpha[:-1], good.beta, 4), *args)
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_from_codes(x, shape, _dev(dev, np.zeros((c.C * c.m, 1, 5, 10), np.float32)), None, 1, 5, 1)      # 50 taps
    with pytest.raises(ValueError):
        ops.depthwise_conv2d_codes(x, shape, w, None, good, *args, out=torch.empty((3, 16), dtype=torch.int8, device=dev))
    # an empty batch: a plane of zero rows, nothing launched
    before = _lib.call_counts.get(CODES, 0)
    empty = ops.CodePlanes(codes=x.codes[:0], rows=0, K=c.C, inv_n=x.inv_n, bit_width=4)
    out = ops.depthwise_conv2d_codes(empty, (0,) + shape[1:], w, None, good, *args)
    assert out.codes.shape[0] == 0 and _lib.call_counts.get(CODES, 0) == before


# ---- module level ----------------------------------------------------------------------------------------------------------------

def _bn(c, g):
    bn = nn.BatchNorm2d(c)
    bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
    bn.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 1.0)      # (sized so that 15 t stays far inside int8: no range flag)
    gamma = torch.rand(c, generator=g) * 0.5 + 0.3
    gamma[::5] *= -1
    bn.weight.data.copy_(gamma)
    bn.bias.data.copy_(torch.randn(c, generator=g) * 0.2 + 0.2)
    return bn


def _run(c, g, bits=4):
    return [_bn(c, g), nn.ReLU(), nnDorefaQuant(bits)]


class _Net(nn.Module):
    """stem fp32 conv -> BN -> ReLU -> quant -> [dw -> BN -> ReLU -> quant -> pw -> BN -> ReLU -> quant] x 2 -> avg_pool -> Linear:
    un-modified modules; the second depthwise layer has stride 2."""

    def __init__(self, g, dw_bits=1, pool=False):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), *_run(16, g))
        mods = [DorefaConv2d(16, 16, 3, padding=1, groups=16, bit_width=dw_bits), *_run(16, g),
                DorefaConv2d(16, 36, 1, bit_width=1), *_run(36, g)]
        if pool:
            mods.append(nn.MaxPool2d(2))
        mods += [DorefaConv2d(36, 36, 3, stride=2, padding=1, groups=36, bit_width=dw_bits), *_run(36, g),
                 DorefaConv2d(36, 40, 1, bit_width=1), *_run(40, g)]
        self.body = nn.Sequential(*mods)
        self.pool = pool
        self.fc = nn.Linear(40, 10)

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


def _input(dev, seed=2, n=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 16, 16, generator=g).to(dev).contiguous(memory_format=torch.channels_last)


def _delta(after, before, name):
    return after.get(name, 0) - before.get(name, 0)


def _value(t):
    return t.value() if isinstance(t, lazy.LazyActivation) else t


@pytest.fixture(autouse=True)
def _fresh_stats():
    start = (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES)
    lazy.STATS.clear()
    _fused.LIBRARY_PATHS.clear()
    yield
    assert (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES) == start


def test_unmodified_stack_stays_on_code_planes(dev):
    net, x = _net(dev), _input(dev)
    with torch.no_grad(), lazy.depthwise_deferred(True):
        with lazy.eager():
            e = net(x)
        assert type(e) is torch.Tensor and e.shape == (2, 10) and bool(torch.isfinite(e).all())
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = net(x)
        stats, after = dict(lazy.STATS), dict(_lib.call_counts)
    assert torch.equal(got, e)
    # four DoReFa convs deferred, one fused block per conv, nothing materialised between the stem quantiser and the head: the
    # average pool reads the last chain's codes
    assert stats.get("deferred") == 4 and stats.get("fused") == 4 and stats.get("materialised", 0) == 0, stats
    assert stats.get("avg_pool_on_codes") == 1 and not [k for k in stats if k.startswith("fallback")], stats
    assert _delta(after, before, CODES) == 2 and _delta(after, before, EAGER) == 0 and _delta(after, before, F32) == 0
    assert _delta(after, before, "qt_conv2d_implicit_codes") == 2
    assert not _fused.LIBRARY_PATHS, _fused.LIBRARY_PATHS


def test_switch_off_is_the_module_by_module_depthwise_path(dev):
    net, x = _net(dev), _input(dev)
    with torch.no_grad():
        with lazy.eager():
            e = net(x)
        with lazy.depthwise_deferred(False):
            lazy.STATS.clear()
            before = dict(_lib.call_counts)
            got = net(x)
            stats, after = dict(lazy.STATS), dict(_lib.call_counts)
        with lazy.depthwise_deferred(True):
            on = net(x)
        # the new switch alone decides: the sign families' switch may stay on
        with lazy.depthwise_deferred(True):
            lazy.DEFER_DEPTHWISE_CODES = False
            before2 = dict(_lib.call_counts)
            got2 = net(x)
            after2 = dict(_lib.call_counts)
            lazy.DEFER_DEPTHWISE_CODES = True
    assert torch.equal(got, e) and torch.equal(on, e) and torch.equal(got2, e)
    # the two pointwise convs still defer; each depthwise layer runs qt_dwconv2d_f32 on an fp32 image and un-fuses its neighbours
    assert stats.get("deferred") == 2, stats
    for a, b in ((after, before), (after2, before2)):
        assert _delta(a, b, EAGER) == 2 and _delta(a, b, CODES) == 0 and _delta(a, b, F32) == 0
    assert not _fused.LIBRARY_PATHS, _fused.LIBRARY_PATHS


def test_maxpool_behind_the_quantiser_runs_on_codes(dev):
    net, x = _net(dev, seed=7, pool=True), _input(dev, 3)
    with torch.no_grad(), lazy.depthwise_deferred(True):
        with lazy.eager():
            e = net(x)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = net(x)
        after = dict(_lib.call_counts)
    assert torch.equal(got, e)
    assert lazy.STATS["fused"] == 4 and lazy.STATS.get("materialised", 0) == 0, lazy.STATS
    assert _delta(after, before, "qt_pool_codes_i8") == 1 and _delta(after, before, CODES) == 2 and _delta(after, before, EAGER) == 0


def test_three_bit_depthwise_weights_defer_and_equal_eager(dev):
    net, x = _net(dev, seed=9, dw_bits=3), _input(dev, 4)
    assert net.body[0].bit_width == 3 and net.body[0]._eval_on_grid()
    with torch.no_grad(), lazy.depthwise_deferred(True):
        with lazy.eager():
            e = net(x)
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        got = net(x)
        after = dict(_lib.call_counts)
    assert torch.equal(got, e)
    assert lazy.STATS["deferred"] == 4 and lazy.STATS["fused"] == 4 and lazy.STATS.get("materialised", 0) == 0, lazy.STATS
    assert _delta(after, before, CODES) == 2 and _delta(after, before, EAGER) == 0


def test_depthwise_root_read_by_another_consumer_materialises_from_codes(dev):
    g = torch.Generator().manual_seed(21)
    torch.manual_seed(21)
    net = _net(dev, seed=11)
    head = nn.Sequential(net.stem, net.body[0], net.body[1])            # ... -> quant -> dw -> BatchNorm
    x = _input(dev, 5, n=3)
    with torch.no_grad(), lazy.depthwise_deferred(True):
        with lazy.eager():
            e_bn = head(x)
            e_conv = nn.Sequential(net.stem, net.body[0])(x)
        # the stem quantiser's output is an fp32 tensor with a code tag: the depthwise conv defers on the tag
        lazy.STATS.clear()
        before = dict(_lib.call_counts)
        y = head(x)
        assert isinstance(y, lazy.LazyActivation) and isinstance(y._qt.input, packed.CodeActivation)
        got = torch.sigmoid(y)                                            # not in the grammar: conv from the codes, BatchNorm replayed
        after = dict(_lib.call_counts)
        assert torch.equal(got, torch.sigmoid(e_bn))
        assert _delta(after, before, F32) == 1 and _delta(after, before, EAGER) == 0 and _delta(after, before, CODES) == 0
        assert lazy.STATS["materialised"] >= 1
        # behind a deferred pointwise chain: the depthwise conv's input is a code plane with the producer's halo
        mid = nn.Sequential(net.stem, *net.body[:9])                      # ... pw -> BN -> ReLU -> quant -> dw (stride 2)
        with lazy.eager():
            e_mid = mid(x)
        before = dict(_lib.call_counts)
        got = mid(x) * 1.0
        after = dict(_lib.call_counts)
        assert type(got) is torch.Tensor and torch.equal(got, e_mid)
        assert _delta(after, before, F32) == 1 and _delta(after, before, CODES) == 1 and _delta(after, before, EAGER) == 0
        assert type(e_conv) is torch.Tensor


class _Residual(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        b = self.net.body
        q = self.net.stem(x)
        t = b[1](b[0](q)) + q                                             # an add behind a depthwise BatchNorm
        return b[7](b[6](b[5](b[4](b[3](b[2](t))))))


def test_add_behind_a_depthwise_batchnorm_falls_back_and_equals_eager(dev):
    m, x = _Residual(_net(dev, seed=13)), _input(dev, 6)
    with torch.no_grad(), lazy.depthwise_deferred(True):
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
    with torch.no_grad(), lazy.depthwise_deferred(True):
        q = net.stem(x)
        tag = packed.lookup_codes(q, packed.NHWC)
        assert tag is not None
        act = packed.CodeActivation(tag, tuple(q.shape))
        # the deferred graph's codes of dw -> BN -> ReLU -> quant -> pw -> BN -> ReLU -> quant
        y = b[7](b[6](b[5](b[4](b[3](b[2](b[1](b[0](q))))))))
        assert isinstance(y, lazy.LazyActivation)
        want = y._qt.force((0, 0))
        dw = FusedDepthwiseDorefaBnQuant(b[0], b[1], 4, relu=True, out_halo=0, fold="device")
        pw = FusedDorefaConvBnQuant(b[4], b[5], 4, relu=True, out_halo=0, fold="device")
        before = dict(_lib.call_counts)
        got = pw(dw(act))
        assert _delta(dict(_lib.call_counts), before, CODES) == 1
        assert got.shape == want.shape and torch.equal(got.codes.codes, want.codes.codes)
        assert int(got.codes.overflow.item()) == 0
        # with a halo for a consumer that pads: the same codes inside a zero border
        dw2 = FusedDepthwiseDorefaBnQuant(b[0], b[1], 4, relu=True, out_halo=(2, 1), fold="device")
        mid, mid2 = dw(act), dw2(act)
        assert mid2.halo == (2, 1) and torch.equal(mid2.without_halo().codes.codes, mid.codes.codes)
        # one capture and replay of the explicit form (no parallel branches); the folds are cached, nothing asks the host
        static = act.codes.codes.clone()
        sact = packed.CodeActivation(ops.CodePlanes(codes=static, rows=tag.rows, K=tag.K, inv_n=tag.inv_n, bit_width=tag.bit_width,
                                                    overflow=tag.overflow), tuple(q.shape))
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            pw(dw(sact))
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                out = pw(dw(sact))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.codes.codes, want.codes.codes)
        q2 = net.stem(_input(dev, 8))
        tag2 = packed.lookup_codes(q2, packed.NHWC)
        static.copy_(tag2.codes)
        graph.replay()
        torch.cuda.synchronize()
        want2 = pw(dw(packed.CodeActivation(tag2, tuple(q2.shape))))
        assert torch.equal(out.codes.codes, want2.codes.codes) and not torch.equal(want2.codes.codes, want.codes.codes)


def test_dorefa_can_defer_admits_depthwise_only(dev):
    net = _net(dev, seed=17, dw_bits=3)
    dwl = net.body[0]
    g2 = DorefaConv2d(16, 16, 3, padding=1, groups=2, bit_width=1).to(dev).eval()
    taps50 = DorefaConv2d(16, 16, (5, 10), padding=5, groups=16, bit_width=1).to(dev).eval()
    k3 = DorefaConv2d(16, 16, 3, padding=1, bit_width=3).to(dev).eval()
    shape = lazy._CodeShapeOnly((1, 16, 12, 12))
    with torch.no_grad():
        with lazy.depthwise_deferred(True):
            assert lazy._dorefa_can_defer(dwl, shape) and not lazy._dorefa_can_defer(dwl, lazy._CodeShapeOnly((1, 16, 0, 12)))
            assert not lazy._dorefa_can_defer(g2, shape) and not lazy._dorefa_can_defer(taps50, shape)
            assert not lazy._dorefa_can_defer(k3, shape)                       # un-grouped convs still need 1-bit weights
            with lazy.codes_deferred(False):
                assert not lazy._dorefa_can_defer(dwl, shape)                  # both switches are needed
            dwl.weight.data.mul_(0.37)                                          # off the quantiser's grid
            dwl.reset_quant_cache()
            assert not dwl._eval_on_grid() and not lazy._dorefa_can_defer(dwl, shape)
        with lazy.depthwise_deferred(False):
            assert not lazy._dorefa_can_defer(net.body[8], lazy._CodeShapeOnly((1, 36, 12, 12)))
