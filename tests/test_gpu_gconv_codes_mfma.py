"""Grouped DorefaConv2d with 16 / 32 input channels per group on int8 code planes, on the int8 matrix cores
(csrc/gconv_codes_mfma.hip): the two C entries byte for byte against a numpy reference written here, the fp32 form against the dense
code conv group by group, and an un-modified pw -> grouped -> pw stack under ``lazy.grouped_mfma_deferred()``.

The reference uses none of the package's packers: an int64 conv sum of the codes with the integer weight bytes, then the float32
steps of the header contract (numpy float32 arithmetic is IEEE, one rounding per operation) and of the code epilogue.  The device
form of the BatchNorm is a fused multiply-add: those cases use constants that make every product exact (powers of two), so the
float64 evaluation of the reference is the fused result.  alpha = 2^-m puts 15 t on exact .5 ties and, with ReLU, on the boundary
t = 0.  Nothing is waived; every output lies between sentinels; the input halo and row pad hold non-zero garbage.

Maps and the tile the launch plans for them (gq_plan: of 8 x 8, 16 x 4, 4 x 16 output pixels the fewest tiles, 8 x 8 on a tie):
9 x 19 -> 4 wide x 16 tall, 1 x 5 tiles; 19 x 19 (and 37 x 37 at stride 2) -> 8 x 8, 3 x 3 tiles, ragged both ways; 11 x 31 -> 16 wide
x 4 tall, 3 x 2 tiles, ragged both ways; 5 x 7 -> one ragged tile."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from pytorch_quantize_impls_amd import _lib, lazy, ops, utils
from pytorch_quantize_impls_amd.functions import _fused, nnDorefaQuant
from pytorch_quantize_impls_amd.layers import DorefaConv2d
from pytorch_quantize_impls_amd.utils import implicit

pytestmark = pytest.mark.gpu

CODES, F32 = "qt_gmconv2d_codes", "qt_gmconv2d_codes_f32"
f32 = np.float32
P = ctypes.c_void_p
GUARD = 256                    # sentinel bytes in front of and behind every output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _case(seed, cin_g=16, cout_g=16, k=3, s=1, p=1, hw=(9, 19), ih=1, oh=1, w_bits=1, relu=1, devbn=False, overflow=False, pad=16,
          N=2, G=8):
    """The operands of one launch, on the host: codes over -127 .. 127, weight bytes, exact power-of-two constants."""
    r = np.random.default_rng(seed)
    H, W = hw
    Cin, Cout = G * cin_g, G * cout_g
    q = r.integers(-127, 128, size=(N, H, W, Cin)).astype(np.int8)
    nw = (1 << w_bits) - 1
    if w_bits == 1:
        wb = r.choice([-1, 1], size=(Cout, cin_g, k, k)).astype(np.int64)
        E, inv_n = f32(0.5), f32(0.125)                       # s = 2^-4: y = S / 16 exactly
        w, scale = (wb * E).astype(f32), f32(inv_n * E)
    else:
        wb = (2 * r.integers(0, nw + 1, size=(Cout, cin_g, k, k)) - nw).astype(np.int64)      # the odd levels
        E, inv_n = None, f32(1.0) / f32(15.0)
        w = (wb.astype(f32) / f32(nw)).astype(f32)
        scale = f32(np.float64(inv_n) * np.float64(f32(1.0) / f32(nw)))
    alpha = (r.choice([-1.0, 1.0], size=Cout) * 2.0 ** r.integers(-9, -5, size=Cout)).astype(f32)
    if overflow:
        alpha[3], alpha[Cout - 2] = f32(4.0), f32(1024.0)      # |q| beyond 127, and beyond 2047
    return dict(N=N, G=G, cin_g=cin_g, cout_g=cout_g, k=k, s=s, p=p, H=H, W=W, ih=ih, oh=oh, w_bits=w_bits, relu=relu, devbn=devbn,
                q=q, wb=wb, w=w, E=E, inv_n=inv_n, scale=scale, alpha=alpha, pad=pad, Cin=Cin, Cout=Cout,
                bias=(r.integers(-32, 33, size=Cout) / 16.0).astype(f32), beta=(r.integers(-16, 17, size=Cout) / 32.0).astype(f32),
                mean=(r.integers(-64, 65, size=Cout) / 16.0).astype(f32), rs=(2.0 ** r.integers(-3, 1, size=Cout)).astype(f32),
                Ho=(H + 2 * p - k) // s + 1, Wo=(W + 2 * p - k) // s + 1)


def _ref_y(c):
    """y [N, Ho, Wo, Cout] float32: the exact int64 sum, then fl(fl(S * s) + bias)."""
    N, G, k, s, p, Ho, Wo = c["N"], c["G"], c["k"], c["s"], c["p"], c["Ho"], c["Wo"]
    x = np.pad(c["q"].astype(np.int64), ((0, 0), (p, p), (p, p), (0, 0))).reshape(N, c["H"] + 2 * p, c["W"] + 2 * p, G, c["cin_g"])
    wg = c["wb"].reshape(G, c["cout_g"], c["cin_g"], k, k)
    S = np.zeros((N, Ho, Wo, G, c["cout_g"]), dtype=np.int64)
    for i in range(k):
        for j in range(k):
            S += np.einsum("nhwgc,gjc->nhwgj", x[:, i:i + (Ho - 1) * s + 1:s, j:j + (Wo - 1) * s + 1:s], wg[:, :, :, i, j])
    assert np.abs(S).max() < (1 << 24)
    return (S.reshape(N, Ho, Wo, c["Cout"]).astype(f32) * c["scale"]).astype(f32) + c["bias"]


def _ref_codes(c, y, bits=4):
    """(codes int8 [N, Ho, Wo, Cout], flag, t) of the code epilogue."""
    if c["devbn"]:      # fma(fl(fl(y - mean) * rs), weight, bias): product and sum exact in float64 for these constants
        u = ((y - c["mean"]).astype(f32) * c["rs"]).astype(f32)
        t = (u.astype(np.float64) * c["alpha"].astype(np.float64) + c["beta"].astype(np.float64)).astype(f32)
    else:
        t = ((y * c["alpha"]).astype(f32) + c["beta"]).astype(f32)
    if c["relu"]:
        t = np.where(t < 0, f32(0), t)
    qv = np.rint((f32((1 << bits) - 1) * t).astype(f32))
    out = np.abs(qv) > 127
    flag = 0 if not out.any() else (3 if (np.abs(qv) > 2047).any() else 1)
    return np.where(out, 0, qv).astype(np.int8), flag, t


def _t(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return P(None if t is None else t.data_ptr())


def _launch(dev, c, form, channels_last=True, raised=False, bits=4):
    """One launch of either entry into a guarded buffer.  "codes": (the whole plane [N, Ho + 2 oh, Wo + 2 oh, ldc], the flag);
    "f32": y as [N, Ho, Wo, Cout].  The input plane's halo and row pad are filled with non-zero garbage."""
    lib = _lib.load()
    N, Cout, Ho, Wo, ih, oh = c["N"], c["Cout"], c["Ho"], c["Wo"], c["ih"], c["oh"]
    ldx = c["Cin"] + c["pad"]
    plane = np.full((N, c["H"] + 2 * ih, c["W"] + 2 * ih, ldx), 77, dtype=np.int8)
    plane[:, ih:ih + c["H"], ih:ih + c["W"], :c["Cin"]] = c["q"]
    x, w, bias = _t(dev, plane), _t(dev, c["w"]), _t(dev, c["bias"])
    E = _t(dev, np.array([c["E"]], dtype=f32)) if c["E"] is not None else None
    flag = torch.full((1,), int(raised), dtype=torch.int32, device=dev)
    head = (_ptr(x), ldx, ih, ih, ctypes.c_float(float(c["inv_n"])), _ptr(w), _ptr(bias))
    geom = (N, c["G"], c["cin_g"], c["cout_g"], c["H"], c["W"], c["k"], c["k"], c["s"], c["s"], c["p"], c["p"], 1, 1)
    if form == "codes":
        ldc = Cout + c["pad"]
        shape = (N, Ho + 2 * oh, Wo + 2 * oh, ldc)
        buf = torch.full((int(np.prod(shape)) + 2 * GUARD,), 0x5A, dtype=torch.int8, device=dev)
        al, be = _t(dev, c["alpha"]), _t(dev, c["beta"])
        stats = _t(dev, np.concatenate([c["mean"], c["rs"]])) if c["devbn"] else None
        rc = lib.qt_gmconv2d_codes(*head, _ptr(al), _ptr(be), _ptr(stats), c["relu"], bits, P(buf.data_ptr() + GUARD), ldc, oh, oh,
                                   _ptr(flag), *geom, _ptr(E), c["w_bits"], None)
    else:
        shape = (N, Ho, Wo, Cout) if channels_last else (N, Cout, Ho, Wo)
        buf = torch.full((int(np.prod(shape)) + GUARD // 2,), 12345.0, device=dev)
        ys = (Ho * Wo * Cout, 1, Wo * Cout, Cout) if channels_last else (Cout * Ho * Wo, Ho * Wo, Wo, 1)
        rc = lib.qt_gmconv2d_codes_f32(*head, _ptr(flag), P(buf.data_ptr() + GUARD), *geom, *ys, _ptr(E), c["w_bits"], None)
    assert rc == 0
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    g = GUARD // host.itemsize
    assert (host[:g] == host[0]).all() and (host[-g:] == host[0]).all() and host[0] in (0x5A, 12345.0)
    body = host[g:-g].reshape(shape)
    return (body, int(flag.item())) if form == "codes" else (body if channels_last else body.transpose(0, 2, 3, 1))


def _check_codes(dev, c):
    want, flag, _ = _ref_codes(c, _ref_y(c))
    got, got_flag = _launch(dev, c, "codes")
    oh = c["oh"]
    full = np.zeros_like(got)                      # border, pad bytes: zero
    full[:, oh:oh + c["Ho"], oh:oh + c["Wo"], :c["Cout"]] = want
    assert int((got != full).sum()) == 0 and got_flag == flag


MULTI = [dict(hw=(19, 19)), dict(hw=(37, 37), s=2, N=1), dict(hw=(11, 31), N=1), dict(hw=(19, 19), p=0, cin_g=32, cout_g=48, w_bits=3)]
AXES = [dict(), dict(k=1, p=0), dict(s=2), dict(p=0), dict(k=1, p=0, s=2), dict(hw=(5, 7)), dict(hw=(5, 7), s=2), dict(ih=0, oh=0),
        dict(ih=2), dict(w_bits=3), dict(w_bits=7), dict(relu=0), dict(devbn=True), dict(devbn=True, relu=0, hw=(19, 19)), dict(pad=48),
        dict(hw=(11, 31), s=2, oh=0), dict(hw=(19, 19), k=1, p=0, s=2)]
PAIRS = [dict(k=k, p=k // 2, cin_g=ci, cout_g=co) for k in (3, 1) for ci in (16, 32) for co in (16, 32, 48)][1:]
CASES = list(enumerate(MULTI + AXES + PAIRS))


def test_reference_holds_the_designed_edges():
    """Exact .5 ties of 15 t and values on or below the ReLU boundary are in the base case and the multi-tile cases."""
    for seed, kw in CASES[:5]:
        c = _case(seed, **dict(kw, relu=0))
        if c["w_bits"] == 1:
            nt = (f32(15) * _ref_codes(c, _ref_y(c))[2]).astype(np.float64)
            assert (np.abs(nt - np.floor(nt)) == 0.5).any() and (nt <= 0).any(), kw


@pytest.mark.parametrize("seed,kw", CASES, ids=lambda v: str(v))
def test_code_entry_equals_the_integer_reference_byte_for_byte(dev, seed, kw):
    _check_codes(dev, _case(seed, **kw))


def test_a_quantiser_result_outside_int8_raises_the_flag_and_stores_zero(dev):
    c = _case(3, overflow=True)
    want, flag, _ = _ref_codes(c, _ref_y(c))
    assert flag == 3 and (want[..., 3] == 0).mean() > 0.5
    _check_codes(dev, c)


@pytest.mark.parametrize("channels_last", (False, True))
@pytest.mark.parametrize("seed,kw", list(enumerate(MULTI + [dict(), dict(k=1, p=0, w_bits=7, cout_g=32)], 100)), ids=lambda v: str(v))
def test_f32_entry_equals_the_integer_reference_bit_for_bit(dev, seed, kw, channels_last):
    c = _case(seed, **kw)
    got = _launch(dev, c, "f32", channels_last)
    assert int((got.view(np.uint32) != _ref_y(c).view(np.uint32)).sum()) == 0


@pytest.mark.parametrize("channels_last", (False, True))
def test_f32_entry_is_nan_everywhere_behind_a_raised_flag(dev, channels_last):
    assert np.isnan(_launch(dev, _case(5), "f32", channels_last, raised=True)).all()


@pytest.mark.parametrize("w_bits", (1, 3))
def test_f32_result_is_the_dense_code_conv_group_by_group(dev, w_bits):
    c = _case(21, w_bits=w_bits, hw=(9, 11))
    N, G, ci, co, H, W = c["N"], c["G"], c["cin_g"], c["cout_g"], c["H"], c["W"]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    inv_n, w, bias = float(c["inv_n"]), _t(dev, c["w"]), _t(dev, c["bias"])
    E = _t(dev, np.array(c["E"], dtype=f32)) if w_bits == 1 else None

    def plane(q):
        return ops.CodePlanes(codes=_t(dev, q.reshape(N * H * W, -1)), rows=N * H * W, K=q.shape[-1], inv_n=inv_n, bit_width=4,
                              overflow=flag)

    got = ops.grouped_mfma_conv2d_from_codes(plane(c["q"]), (N, G * ci, H, W), w, bias, 1, 1, 1, G, bit_width_w=w_bits, scale_dev=E)
    parts = []
    for g in range(G):
        xg, wg, bg = plane(c["q"][..., g * ci:(g + 1) * ci]), w[g * co:(g + 1) * co], bias[g * co:(g + 1) * co]
        if w_bits == 1:
            y2 = ops.conv2d_codes(xg, (N, ci, H, W), ops.pack_conv_weight_codes(wg), (3, 3), inv_n, bg, 1, 1, 1, scale_dev=E)
        else:
            y2 = ops.conv2d_codes(xg, (N, ci, H, W), ops.pack_conv_weight_dorefa_codes(wg, w_bits), (3, 3),
                                  inv_n * _fused._inv_levels(w_bits), bg, 1, 1, 1, max_abs_code=127 * 7)
        parts.append(y2.view(N, H, W, co).permute(0, 3, 1, 2))
    assert torch.equal(got, torch.cat(parts, 1))


# ---- module level ----------------------------------------------------------------------------------------------------------------

def _input(dev, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 16, 16, generator=g).to(dev).contiguous(memory_format=torch.channels_last)


def _net(dev, groups, g_bits, seed):
    """stem fp32 conv -> run -> pw 1 x 1 -> run -> grouped 3 x 3 -> run -> pw 1 x 1 -> run, run = BatchNorm -> ReLU -> nnDorefaQuant(4):
    un-modified modules.  The running statistics are those of one batch (momentum 1), so that 15 t stays inside int8 behind the 144-
    and 256-term sums and the chain's range flag stays down."""
    g = torch.Generator().manual_seed(seed)

    def run(c):
        bn = nn.BatchNorm2d(c, momentum=1.0)
        bn.weight.data.copy_((torch.rand(c, generator=g) * 0.5 + 0.3) * torch.where(torch.arange(c) % 5 == 0, -1.0, 1.0))
        bn.bias.data.copy_(torch.randn(c, generator=g) * 0.2 + 0.2)
        return [bn, nn.ReLU(), nnDorefaQuant(4)]

    net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), *run(16), DorefaConv2d(16, 256, 1, bit_width=1), *run(256),
                        DorefaConv2d(256, 256, 3, padding=1, groups=groups, bit_width=g_bits), *run(256),
                        DorefaConv2d(256, 32, 1, bit_width=1), *run(32))
    for m in net.modules():
        if isinstance(m, (nn.Conv2d, DorefaConv2d)):
            m.weight.data.copy_(torch.randn(m.weight.shape, generator=g) * 0.6)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    net = net.to(dev).to(memory_format=torch.channels_last).eval()
    bns = [m for m in net if isinstance(m, nn.BatchNorm2d)]
    for m in bns:
        m.train()
    with torch.no_grad(), lazy.eager():
        net(_input(dev))
    for m in bns:
        m.eval()
    _fused.LIBRARY_PATHS.clear()
    return net


def _counted(net, x):
    """(the fp32 result, launches by entry, lazy.STATS) of one forward."""
    lazy.STATS.clear()
    before = dict(_lib.call_counts)
    y = net(x)
    y = y.value() if isinstance(y, lazy.LazyActivation) else y
    return y, {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if v != before.get(k, 0)}, dict(lazy.STATS)


@pytest.fixture(autouse=True)
def _fresh_stats():
    start = (lazy.DEFER_GROUPED_MFMA, lazy.DEFER_GROUPED_MFMA_CODES)
    _fused.LIBRARY_PATHS.clear()
    yield
    assert (lazy.DEFER_GROUPED_MFMA, lazy.DEFER_GROUPED_MFMA_CODES) == start


@pytest.mark.parametrize("groups,g_bits", ((16, 1), (8, 1), (16, 3)))
def test_unmodified_triple_stays_on_code_planes_and_equals_eager(dev, groups, g_bits):
    net, x = _net(dev, groups, g_bits, seed=30 + groups + g_bits), _input(dev)
    with torch.no_grad():
        with lazy.grouped_mfma_deferred(True):
            routed = _fused.STREAMING_CODES_STATS["grouped_mfma"]
            with lazy.eager():
                e, used, _ = _counted(net, x)
            # module by module: the new kernel on the code tag, counted, no library conv
            assert used.get(F32) == 1 and _fused.STREAMING_CODES_STATS["grouped_mfma"] == routed + 1 and not _fused.LIBRARY_PATHS
            got, used, stats = _counted(net, x)
            assert torch.equal(got, e) and bool(torch.isfinite(e).all())
            # all three DoReFa convs deferred; the grouped one ran the new code entry between two dense code convs
            assert stats.get("deferred") == 3 and used.get(CODES) == 1 and F32 not in used and not _fused.LIBRARY_PATHS, (stats, used)
            assert used.get("qt_conv2d_implicit_codes") == 2
        with lazy.grouped_mfma_deferred(False):
            off, used, _ = _counted(net, x)
        # the previous path: the dense library behind a materialised chain
        assert CODES not in used and F32 not in used and _fused.LIBRARY_PATHS
        # ... the only reference here that does not come from the new kernel.  It sums in fp32 in the library's order, so a value
        # on a rounding tie of a quantiser may land one level (1 / 15) away, once per quantiser behind the grouped conv; never more
        d = (off - e).abs()
        assert float(d.max()) <= 2.0 / 15.0 + 1e-6 and float((d > 0).float().mean()) < 0.01


def test_triple_replays_from_the_default_implicit_hipgraph_and_equals_eager(dev, monkeypatch):
    monkeypatch.setattr(implicit, "KEEP_IF_FASTER", 0.0)              # no test may depend on the clock
    net = nn.Sequential(_net(dev, 16, 1, seed=41), nn.AdaptiveAvgPool2d(1), nn.Flatten()).to(dev).eval()
    x, x2 = _input(dev, 9), _input(dev, 10)
    with lazy.grouped_mfma_deferred(True), utils.implicit_graphs(True):
        with torch.no_grad(), utils.implicit_graphs(False), lazy.eager():
            want, want2 = net(x).clone(), net(x2).clone()
        assert bool(torch.isfinite(want).all()) and not torch.equal(want, want2)
        with torch.no_grad():
            for i in range(5):
                y = net(x)
                assert type(y) is torch.Tensor and torch.equal(y, want), i
            assert torch.equal(net(x2), want2) and torch.equal(net(x), want)          # fresh data through the same graph
        st = utils.implicit_graph_stats(net)
        assert st["wrapped"] and st["graphs"] == 1 and st["value_mismatch"] == 0 and st["capture_failures"] == {}, st


def test_fuse_sequential_builds_the_block_behind_a_code_producer(dev):
    from pytorch_quantize_impls_amd.layers import FusedDorefaConvBnQuant, FusedGroupedMfmaDorefaBnQuant, fuse_sequential
    net = _net(dev, 16, 1, seed=51)
    x = _input(dev)
    with torch.no_grad(), lazy.eager(), lazy.grouped_mfma_deferred(True):
        want = net(x)
        head, tail = net[:4], nn.Sequential(FusedDorefaConvBnQuant(net[4], net[5], 4, fold="device"), *net[8:12])
        fused = fuse_sequential(tail, fuse_conv=True, fold="device")
        assert len(fused) == 2 and isinstance(fused[1], FusedGroupedMfmaDorefaBnQuant)
        # not behind a producer of code planes: the modules stay as they are
        assert not any(isinstance(m, FusedGroupedMfmaDorefaBnQuant) for m in fuse_sequential(net[8:12], fuse_conv=True))
        from pytorch_quantize_impls_amd import packed
        h = head(x)                                  # the stem quantiser's fp32 image, which carries its codes
        act = fused(packed.CodeActivation(packed.lookup_codes(h, packed.NHWC), tuple(h.shape)))
        assert act.shape == (2, 256, 16, 16) and torch.equal(act.float(), net[:12](x))
