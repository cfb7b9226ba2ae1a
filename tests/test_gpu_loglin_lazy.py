"""The deferred level chain of the Lin / Log family on the device (lazy.py kind "levels", layers.fused.FusedLogLinConvBnQuant /
LevelMaxPool / FusedBnLogLinQuant, the level epilogue of the implicit conv): kernels against the two-step forms byte for byte, whole
nets against ``lazy.eager()`` with torch.equal, routes by call counts, materialisation, switches, implicit hipGraphs."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from pytorch_quantize_impls_amd import _lib, lazy, ops, packed, utils
from pytorch_quantize_impls_amd.functions import _fused, log_lin_connect
from pytorch_quantize_impls_amd.layers import (FusedBnLogLinQuant, FusedLogLinConvBnQuant, LevelMaxPool, LinearQuant, QuantConv2d)
from pytorch_quantize_impls_amd.layers import fused as fused_mod
from test_gpu_loglin_act import calls
from test_gpu_loglin_train import _VGGLinLog

CHANNELS = (3, 13, 40, 64, 130)                   # the set tests/test_gpu_loglin_act.py uses
ACT_QUANTS = (("lin", 1, 3, False), ("lin", 1, 8, False), ("log", 1, 3, True), ("lin", 2, 8, True), ("log", 2, 3, False))
GEOMS = ((3, 1, 1), (5, 1, 2), (1, 1, 0), (3, 2, 1), (5, 2, 0))          # (kernel, stride, padding)
MAPS = ((8, 8), (7, 9), (13, 11), (16, 16))                              # incl. sizes that are not powers of two


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    assert _lib.device_info()[0].startswith("gfx950")
    return torch.device("cuda:0")


def _bn(C, dev, seed, one_d=False):
    g = torch.Generator().manual_seed(seed)
    bn = (torch.nn.BatchNorm1d if one_d else torch.nn.BatchNorm2d)(C).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.7)
        bn.running_var.copy_(torch.rand(C, generator=g) * 3 + 0.3)
        bn.weight.copy_((torch.rand(C, generator=g) + 0.4) * torch.where(torch.rand(C, generator=g) < 0.2, -1.0, 1.0))
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    return bn


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                C = m.num_features
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.5)
                m.running_var.copy_(torch.rand(C, generator=g) * 4 + 0.5)
                m.weight.copy_(torch.rand(C, generator=g) + 0.5)
                m.bias.copy_(torch.randn(C, generator=g) * 0.2)


def _interior(plane, N, H, W, halo):
    hy, hx = halo
    return plane.view(N, H + 2 * hy, W + 2 * hx, -1)[:, hy:hy + H, hx:hx + W].reshape(N * H * W, -1)


def _border_is_zero(plane, N, H, W, halo):
    hy, hx = halo
    p = plane.view(N, H + 2 * hy, W + 2 * hx, -1).clone()
    p[:, hy:hy + H, hx:hx + W] = 0
    return not bool(p.any())


def _conv_cases():
    """A third of channels x channels x geometries plus everything at 130 channels.  The other parameters advance with strides of
    their own (j = running case number), so that no two of them are tied: every pair of values of any two of geometry, map,
    quantiser, ReLU, bias, input halo, output halo, BatchNorm memory format and weight kind occurs, and every channel count meets
    every value of each.  Then cases that run whole tiles for certain (Cout = 128, 3 * 16 * 16 = 768 output pixels: a multiple of
    every tile shape), where the epilogue takes its straight-line body, with each quantiser kind, ReLU on and off."""
    cases = []
    for i, ((cin, cout), geom) in enumerate(itertools.product(itertools.product(CHANNELS, CHANNELS), GEOMS)):
        if (i % 3) and not (cin == 130 or cout == 130):
            continue
        j = len(cases)
        cases.append((cin, cout, geom, MAPS[(j // 2 + j // 13) % 4], ACT_QUANTS[(i + i // 5) % 5], bool(j % 2), bool((j // 8) % 2),
                      (j // 5) % 2, (j // 11) % 2, bool((j // 7) % 2), bool((j // 3) % 2), i))
    for n, spec in enumerate(ACT_QUANTS):
        cases.append((64, 128, (3, 1, 1), (16, 16), spec, bool(n % 2), bool((n // 2) % 2), n % 2, (n + 1) % 2, bool(n % 2), bool(n % 2),
                      1000 + n))
        cases.append((64, 128, (3, 1, 1), (16, 16), spec, not n % 2, True, 0, 1, False, not n % 2, 1010 + n))
    return cases


def test_conv_cases_tie_no_two_parameters():
    cases = _conv_cases()[:-2 * len(ACT_QUANTS)]
    for a, b in itertools.combinations(range(2, 11), 2):
        va, vb = {c[a] for c in cases}, {c[b] for c in cases}
        assert len({(c[a], c[b]) for c in cases}) == len(va) * len(vb), (a, b)
    for a in (0, 1):
        for b in range(2, 11):
            assert len({(c[a], c[b]) for c in cases}) == len(CHANNELS) * len({c[b] for c in cases}), (a, b)


@pytest.mark.gpu
def test_level_epilogue_equals_conv_batchnorm_relu_quantiser(dev):
    """qt_conv2d_implicit_levels against qt_conv2d_implicit -> F.batch_norm -> relu -> qt_linlog_quantize_bf16_f32: planes and
    borders byte for byte."""
    in_q = ("lin", 1, 8, False)
    n_cases = 0
    for cin, cout, (k, s, p), (H, W), spec, relu, with_bias, in_halo, out_halo, cl, wlog, idx in _conv_cases():
        if H + 2 * p < k or W + 2 * p < k:
            continue
        N = 3
        g = torch.Generator().manual_seed(idx)
        x = torch.randn((N, cin, H, W), generator=g).to(dev)
        xq, xp, _ = ops.quantize_levels_bf16(x, *in_q)
        w = ((torch.rand((cout, cin, k, k), generator=g) * 2 - 1) * 4).to(dev)
        wdt, wbits = ("log", 3) if wlog else ("lin", 8)
        wt = ops.pack_levels_bf16x3(w, wdt, 2, wbits, grad_x=False, fwd_terms=1)[0]
        bias = (torch.randn(cout, generator=g) * 0.5).to(dev) if with_bias else None
        bn = _bn(cout, dev, 1000 + idx)
        # two steps: the plain conv on the same plane, then the module chain on its fp32 result
        y2 = ops.float_conv2d(None, w, "raw", bias, s, p, 1, weight_triples=wt, pixels=xp, in_shape=(N, cin, H, W))
        Ho, Wo = ops.conv_out_hw(H, W, k, k, s, p, 1)
        y = y2.view(N, Ho, Wo, cout).permute(0, 3, 1, 2)
        if not cl:
            y = y.contiguous()
        t = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        if relu:
            t = torch.relu(t)
        _, want, layout = ops.quantize_levels_bf16(t, *spec)
        assert layout == packed.NHWC
        # one launch: input plane with or without a physical zero border, output plane likewise
        ih = (max(p, 1),) * 2 if in_halo else (0, 0)
        pix = xp
        if in_halo:
            padded = torch.zeros((N, H + 2 * ih[0], W + 2 * ih[1], xp.data.shape[1]), dtype=torch.int16, device=dev)
            padded[:, ih[0]:ih[0] + H, ih[1]:ih[1] + W] = xp.data.view(N, H, W, -1)
            pix = ops.TriplePlanes(data=padded.view(-1, xp.data.shape[1]), rows=N * (H + 2 * ih[0]) * (W + 2 * ih[1]), K=cin, terms=1)
        fw, fb, stats = fused_mod.device_bn_fold(bn, (N, cout, Ho, Wo), cl)
        oh = (out_halo, out_halo)
        with calls() as c:
            got = ops.conv2d_levels(pix, (N, cin, H, W), wt, (k, k), ops.LevelEpilogue(fw, fb, stats, spec, relu, oh), bias, s, p, 1,
                                    in_halo=ih)
        assert c["qt_conv2d_implicit_levels"] == 1 and sum(c.c.values()) == 1, dict(c.c)
        what = (cin, cout, k, s, p, H, W, spec, relu, with_bias, ih, oh, cl)
        assert got.data.shape == (N * (Ho + 2 * out_halo) * (Wo + 2 * out_halo), want.data.shape[1]), what
        assert torch.equal(_interior(got.data, N, Ho, Wo, oh), want.data), what
        assert _border_is_zero(got.data, N, Ho, Wo, oh), what
        n_cases += 1
    assert n_cases >= 40


@pytest.mark.gpu
def test_level_epilogue_on_the_three_term_image_plane(dev):
    """The first layer: a real image as exact bf16 triples against the three-term weight plane (K = terms * channels)."""
    torch.manual_seed(5)
    for cout, (H, W), spec in ((64, (32, 32), ("lin", 1, 8, False)), (13, (9, 7), ("log", 1, 3, True))):
        conv = QuantConv2d(3, cout, 3, padding=1, fsr=2, bit_width=8).to(dev).eval()
        bn = _bn(cout, dev, 77)
        x = torch.randn((4, 3, H, W), device=dev)
        with torch.no_grad(), lazy.eager():
            t = torch.relu(bn(conv(x)))
            _, want, _ = ops.quantize_levels_bf16(t, *spec)
            got = FusedLogLinConvBnQuant(conv, bn, spec, relu=True, out_halo=1)(x)
        assert got.halo == (1, 1) and got.shape == (4, cout, H, W)
        assert torch.equal(_interior(got.planes.data, 4, H, W, (1, 1)), want.data)
        assert _border_is_zero(got.planes.data, 4, H, W, (1, 1))


@pytest.mark.gpu
def test_pool_levels_equals_max_pool_of_the_image(dev):
    for i, (C, (H, W), (k, s), halo, spec) in enumerate(((64, (8, 8), (2, 2), (1, 1), ("lin", 1, 8, False)),
                                                         (13, (7, 9), (3, 2), (0, 0), ("lin", 1, 3, True)),
                                                         (130, (13, 11), (2, 2), (2, 1), ("log", 1, 3, True)),
                                                         (3, (16, 16), (3, 1), (1, 1), ("log", 2, 3, False)),
                                                         (40, (6, 5), (2, 1), (0, 0), ("lin", 2, 8, True)))):
        g = torch.Generator().manual_seed(40 + i)
        x = (torch.randn((3, C, H, W), generator=g) * 1.5)
        x.view(-1)[::97] = float("nan")
        x.view(-1)[5::53] = 0.0
        x.view(-1)[7::59] = -1e-9                               # -0 after a signed quantiser
        xq, xp, _ = ops.quantize_levels_bf16(x.to(dev), *spec)
        pooled = F.max_pool2d(xq, k, s)
        want, flag, _ = ops.pack_bf16_check(pooled)
        Ho, Wo = pooled.shape[2:]
        with calls() as c:
            got = ops.pool_levels(xp, 3, H, W, k, s, halo)
        assert c["qt_pool_levels_bf16"] == 1 and sum(c.c.values()) == 1
        assert torch.equal(_interior(got.data, 3, Ho, Wo, halo), want.data), (C, H, W, k, s, halo, spec)
        assert _border_is_zero(got.data, 3, Ho, Wo, halo)
        act = LevelMaxPool(torch.nn.MaxPool2d(k, s), out_halo=halo)(packed.LevelActivation(xp, (3, C, H, W)))
        assert act.shape == (3, C, Ho, Wo) and torch.equal(act.planes.data, got.data)


@pytest.mark.gpu
def test_bn_relu_quantiser_rows_pass_equals_the_torch_sequence(dev):
    for i, (rows, C, spec, relu) in enumerate(((256, 1024, ("lin", 1, 8, False), True), (37, 13, ("lin", 1, 3, True), False),
                                               (5, 130, ("log", 1, 3, True), True), (64, 40, ("log", 2, 3, False), False),
                                               (9, 3, ("lin", 2, 8, True), True), (130, 64, ("lin", 1, 8, False), False))):
        g = torch.Generator().manual_seed(90 + i)
        x = (torch.randn((rows, C), generator=g) * 3).to(dev)
        bn = _bn(C, dev, 200 + i, one_d=True)
        with torch.no_grad():
            t = bn(x)
            if relu:
                t = torch.relu(t)
            want_y, want, layout = ops.quantize_levels_bf16(t, *spec)
            assert layout == packed.ROWS_LAST
            with calls() as c:
                got = FusedBnLogLinQuant(bn, spec, relu=relu, want_f32=True)(x)
            assert c["qt_bn_relu_linlog_bf16_f32"] == 1 and c["qt_linlog_quantize_bf16_f32"] == 0
        assert got.shape == (rows, C) and torch.equal(got.planes.data, want.data), (rows, C, spec, relu)
        assert torch.equal(got.image.view(torch.int32), want_y.view(torch.int32)), (rows, C, spec, relu)
        assert torch.equal(got.float().view(torch.int32), want_y.view(torch.int32))


# ---- whole nets ------------------------------------------------------------------------------------------------------------------

def _vgg(dev, dtype, bits, width, seed=3):
    torch.manual_seed(seed)
    m = _VGGLinLog(dtype, bits, width).to(dev)
    _randomise_bn(m, seed + 1)
    return m.eval()


def _explicit_forward(m, x):
    """The net written with the explicit fused modules."""
    spec = ("lin", 1, 8, False)
    act = x
    for i, (conv, bn) in enumerate(zip(m.convs, m.bns)):
        pooled = i % 2 == 1
        act = FusedLogLinConvBnQuant(conv, bn, spec, relu=True, out_halo=0 if (pooled or i == 5) else 1)(act)
        if pooled:
            act = LevelMaxPool(torch.nn.MaxPool2d(2), out_halo=1 if i < 5 else 0)(act)
    act = act.flatten_hwc()
    for lin, bn in zip(m.lins[:2], m.bn1d):
        wt = _fused.loglin_linear_weight_plane(lin, hwc=act.hwc)
        y = ops.bf16_gemm(act.planes, wt, lin.bias.detach())
        act = FusedBnLogLinQuant(bn, spec, relu=True)(y)
    y = ops.bf16_gemm(act.planes, _fused.loglin_linear_weight_plane(m.lins[2]), m.lins[2].bias.detach())
    return F.log_softmax(y, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,bits,width,batch", [("lin", 8, 16, 16), ("log", 3, 16, 16), ("lin", 8, 64, 16), ("log", 3, 64, 16),
                                                    ("lin", 8, 64, 256), ("log", 3, 64, 256)],          # 256: the benchmarked batch
                         ids=["lin-8-16", "log-3-16", "lin-8-64", "log-3-64", "lin-8-64-b256", "log-3-64-b256"])
def test_vgg_logits_equal_eager_explicit_and_replayed(dev, dtype, bits, width, batch):
    m = _vgg(dev, dtype, bits, width)
    x = torch.randn((batch, 3, 32, 32), device=dev)
    with torch.no_grad():
        with lazy.eager():
            want = m(x).clone()
        assert bool(torch.isfinite(want).all()) and float(want.std()) > 0
        assert torch.equal(_explicit_forward(m, x), want)
        with utils.implicit_graphs(True), lazy.levels_deferred():
            outs = [m(x).clone() for _ in range(5)]
            stats = utils.implicit_graph_stats(m)
        for i, y in enumerate(outs):
            assert type(y) is torch.Tensor and torch.equal(y, want), i
        assert stats["wrapped"] and stats["value_mismatch"] == 0 and not stats["capture_failures"], stats
        # calls 3 - 5 were replays of one captured graph, not host-issued forwards that a declined capture would leave behind
        assert stats["graphs"] == 1 and stats["replays"] >= 3 and stats["not_faster"] == 0, stats
        # another input through the same (possibly replayed) forward follows the data
        x2 = torch.randn_like(x)
        with lazy.eager():
            want2 = m(x2).clone()
        with utils.implicit_graphs(True), lazy.levels_deferred():
            assert torch.equal(m(x2), want2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,bits", [("lin", 8), ("log", 3)])
def test_vgg_routes_by_call_counts_and_stats(dev, dtype, bits):
    m = _vgg(dev, dtype, bits, 32)
    x = torch.randn((32, 3, 32, 32), device=dev)
    _fused.reset_detection()
    with torch.no_grad(), lazy.levels_deferred():
        y0 = m(x)
        _fused.LIBRARY_PATHS.clear()
        sync = _fused.DETECT_STATS["sync"]
        before = dict(lazy.STATS)
        with calls() as ev:
            y1 = m(x)
    d = {k: lazy.STATS[k] - before.get(k, 0) for k in lazy.STATS if lazy.STATS[k] != before.get(k, 0)}
    assert torch.equal(y0, y1) and type(y1) is torch.Tensor
    for k in ("qt_linlog_quantize_bf16_f32", "qt_bf16_pack_check_f32", "qt_check_bf16_exact_f32", "qt_lin_quantize_f32",
              "qt_log_quantize_f32", "qt_conv2d_implicit", "qt_conv2d_implicit_variant", "qt_conv2d_implicit_halo"):
        assert ev[k] == 0, (k, dict(ev.c))
    assert ev["qt_bf16x3_pack_f32"] == 1, dict(ev.c)                        # one activation split: the image
    assert ev["qt_conv2d_implicit_levels"] == 6 and ev["qt_bf16_gemm"] == 3, dict(ev.c)
    assert ev["qt_pool_levels_bf16"] == 3 and ev["qt_bn_relu_linlog_bf16_f32"] == 2, dict(ev.c)
    assert ev["qt_bf16x1_pack_conv_levels_f32"] == 0 and ev["qt_bf16x1_pack_levels_f32"] == 0, dict(ev.c)   # weight planes cached
    assert _fused.DETECT_STATS["sync"] == sync and not _fused.LIBRARY_PATHS, dict(_fused.LIBRARY_PATHS)
    assert d == {"deferred": 6, "fused": 6, "levels_dense_deferred": 3, "levels_dense_fused": 2}, d


# ---- materialisation and switches ----------------------------------------------------------------------------------------------------

class _Chain(torch.nn.Module):
    def __init__(self, dev, act_bits=8, groups2=1, mid=None):
        super().__init__()
        self.q = log_lin_connect.nnQuant("lin", 1, act_bits, with_sign=False)
        self.c1 = QuantConv2d(8, 16, 3, padding=1, fsr=2, bit_width=8)
        self.c2 = QuantConv2d(16, 16, 3, padding=1, fsr=2, bit_width=8, groups=groups2)
        self.b1, self.b2 = torch.nn.BatchNorm2d(16), torch.nn.BatchNorm2d(16)
        self.lin = LinearQuant(16 * 16, 10, fsr=1, bit_width=8)
        self.mid = mid
        self.to(dev)
        _randomise_bn(self, 11)
        self.eval()

    def forward(self, x):
        x = self.q(torch.relu(self.b1(self.c1(x))))
        if self.mid is not None:
            x = self.mid(x)
        x = F.max_pool2d(self.q(torch.relu(self.b2(self.c2(x)))), 2)
        return self.lin(x.flatten(1))


def _delta(before):
    return {k: lazy.STATS[k] - before.get(k, 0) for k in lazy.STATS if lazy.STATS[k] != before.get(k, 0)}


@pytest.mark.gpu
def test_materialisation_gives_the_eager_value(dev):
    torch.manual_seed(8)
    x = torch.randn((4, 8, 8, 8), device=dev)
    cases = {"op outside the grammar": dict(mid=lambda t: t * 0.5 + 0.25), "12-bit quantiser": dict(act_bits=12),
             "grouped consumer": dict(groups2=2), "in the grammar": dict()}
    for name, kw in cases.items():
        m = _Chain(dev, **kw)
        with torch.no_grad():
            with lazy.eager():
                want = m(x)
            before = dict(lazy.STATS)
            with lazy.levels_deferred():
                got = m(x)
            d = _delta(before)
            assert torch.equal(got, want), name
            if name == "in the grammar":
                assert d.get("materialised", 0) == 0 and not any(k.startswith("fallback") for k in d), d
                assert d["deferred"] == 2 and d["fused"] == 2, d
            else:
                assert d.get("materialised", 0) >= 1 and any(k.startswith("fallback") for k in d), (name, d)
    # .cpu() / printing / arithmetic on a deferred activation hand out the module-by-module value
    m = _Chain(dev)
    with torch.no_grad():
        with lazy.eager():
            a = m.c1(x)
            want_q = m.q(torch.relu(m.b1(a)))
        before = dict(lazy.STATS)
        with lazy.levels_deferred():
            la = m.c1(x)
            assert isinstance(la, lazy.LazyActivation) and la._qt.kind == "levels" and la.shape == a.shape
            lq = m.q(torch.relu(m.b1(la)))
            assert isinstance(lq, lazy.LazyActivation) and lq._qt.quant == ("lin", 1, 8, False)
            got_q = lq.cpu()
            assert "tensor" in repr(la)
        d = _delta(before)
        assert type(got_q) is torch.Tensor and torch.equal(got_q, want_q.cpu())
        assert torch.equal(la.value(), a)
        assert d.get("materialised", 0) >= 1 and d.get("fallback:cpu", 0) == 1, d
        # the fused plane of the same chain is the plane of that value
        with lazy.levels_deferred():
            act = m.q(torch.relu(m.b1(m.c1(x))))._qt.force((1, 1))
        assert act is not None and act.halo == (1, 1)
        assert torch.equal(act.float().contiguous().view(torch.int32), want_q.view(torch.int32))


@pytest.mark.gpu
def test_updates_between_calls_are_picked_up(dev):
    torch.manual_seed(9)
    m = _Chain(dev)
    x = torch.randn((4, 8, 8, 8), device=dev)

    def both():
        with torch.no_grad():
            with lazy.eager():
                want = m(x)
            with lazy.levels_deferred():
                got = m(x)
        assert torch.equal(got, want)
        return want.clone()

    y0 = both()
    with torch.no_grad():
        m.b1.running_mean.add_(0.5)
        m.b2.weight.mul_(-1.5)
    y1 = both()
    assert not torch.equal(y0, y1)
    with torch.no_grad():
        m.c2.weight.copy_(m.c2.weight.roll(1, 0))
        m.lin.weight.mul_(-1.0)
    y2 = both()
    assert not torch.equal(y1, y2)
    # a producer written between the deferral and the use is an error, as for the other kinds
    with torch.no_grad(), lazy.levels_deferred():
        la = m.b1(m.c1(x))
        m.b1.running_var.mul_(2.0)
        with pytest.raises(RuntimeError, match="modified in place"):
            la.value()


@pytest.mark.gpu
def test_in_place_write_on_a_dense_result_leaves_the_recorded_chain_its_value(dev):
    """A LinearQuant result (kind "ldense") written in place, outside the grammar, after BatchNorm1d -> ReLU -> nnQuant was recorded
    on it: the tensor shows the write, the recorded chain reads the private copy of the old value (and version-checks that copy)."""
    torch.manual_seed(12)
    lin = LinearQuant(40, 24, fsr=1, bit_width=8).to(dev).eval()
    bn = _bn(24, dev, 31, one_d=True)
    q = log_lin_connect.nnQuant("lin", 1, 8, with_sign=False)
    x = torch.randn((9, 40), device=dev)
    with torch.no_grad():
        with lazy.eager():
            y = lin(x)
            want = q(torch.relu(bn(y)))
        with lazy.levels_deferred():
            ld = lin(x)
            assert type(ld) is lazy.LazyDense and ld._qt.kind == "ldense"
            chain = q(torch.relu(bn(ld)))
            assert isinstance(chain, lazy.LazyActivation) and chain._qt.value is None
            ld.mul_(2.0)
            assert torch.equal(ld.as_subclass(torch.Tensor), y * 2.0)
            act = chain._qt.force()
            assert act is not None and torch.equal(act.float().view(torch.int32), want.view(torch.int32))
            assert torch.equal(chain.value(), want)


@pytest.mark.gpu
def test_switch_off_shows_no_levels_activity(dev):
    torch.manual_seed(10)
    m = _Chain(dev)
    x = torch.randn((4, 8, 8, 8), device=dev)
    assert lazy.DEFER_LEVELS is False
    before = dict(lazy.STATS)
    with torch.no_grad():
        with calls() as c:
            y = m(x)
        a = m.c1(x)
    assert type(y) is torch.Tensor and type(a) is torch.Tensor and dict(lazy.STATS) == before
    for k in ("qt_conv2d_implicit_levels", "qt_pool_levels_bf16", "qt_bn_relu_linlog_bf16_f32"):
        assert c[k] == 0, dict(c.c)
    # the explicit modules refuse what they cannot fold: a BatchNorm in training mode, levels beyond one bf16 term
    with pytest.raises(RuntimeError):
        FusedLogLinConvBnQuant(m.c1, torch.nn.BatchNorm2d(16).to(dev), ("lin", 1, 8, False))(x)
    with pytest.raises(ValueError):
        FusedLogLinConvBnQuant(m.c1, m.b1, ("lin", 1, 12, False))
