"""One-term bf16 route of the Lin / Log family on the GPU (csrc/loglin_act.hip, the one-term level packs of csrc/loglin_pack.hip,
functions/_fused.py loglin_act_planes / detect_bf16_exact): the quantise-and-pack kernel bit for bit, results that are bit-equal
to fp64 where every partial sum is exact, general inputs against fp64 at the family's 1e-5 bar, routes by call counts, and the
detection of un-tagged activations."""
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import norm_err
from pytorch_quantize_impls_amd import _lib, ops, packed
from pytorch_quantize_impls_amd.functions import _fused, log_lin_connect
from pytorch_quantize_impls_amd.layers import LinearQuant, QuantConv2d
from test_gpu_loglin_train import _VGGLinLog, _ref_grads, _same_nan, _step
from test_loglin_act_cpu import bf16_exact_np

TOL = 1e-5          # the project's normalised bar for this family (tests/test_gpu_loglin_train.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    assert _lib.device_info()[0].startswith("gfx950")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _fresh_detection():
    _fused.reset_detection()
    yield
    _fused.reset_detection()


def n(t):
    return t.detach().cpu().numpy()


class calls:
    """Counts of C-ABI entry points called inside the block."""

    def __enter__(self):
        self.before = Counter(_lib.call_counts)
        self.c = Counter()
        return self

    def __exit__(self, *exc):
        self.c = Counter({k: v - self.before.get(k, 0) for k, v in _lib.call_counts.items() if v != self.before.get(k, 0)})

    def __getitem__(self, k):
        return self.c.get(k, 0)


def _edge_input(shape, fsr, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 2 - 1) * 2.0 ** fsr * 1.3
    flat = x.view(-1)
    edge = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), 2.0 ** fsr * 3, -(2.0 ** fsr) * 5, 1e-30, -1e-38, 1e-45,
            2.0 ** (fsr - 0.5), -(2.0 ** (fsr - 2.5)), 2.0 ** (fsr - 4) * 1.5, -(2.0 ** (fsr - 3)) * 2.5]
    for i, v in enumerate(edge):
        if i * 5 < flat.numel():
            flat[i * 5] = v
    return x.to(dev)


def _plane_checks(y, planes, layout, what):
    """The plane against the fp32 image it came with: high halves, NaN stays NaN, zero pad, granules."""
    if y.dim() == 4:
        assert layout == packed.NHWC
        rows = y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])
        ld = ops.triple_ld_bytes(y.shape[1], 16, 1)
    else:
        assert layout == packed.ROWS_LAST
        rows = y.reshape(-1, y.shape[-1])
        ld = ops.triple_ld_bytes(y.shape[-1], 128, 1)
    R, C = rows.shape
    assert planes.terms == 1 and (planes.rows, planes.K) == (R, C) and tuple(planes.data.shape) == (R, ld // 2), what
    img = n(rows.contiguous()).view(np.uint32)
    pl = n(planes.data).view(np.uint16).astype(np.uint32)
    nan = np.isnan(n(rows.contiguous()))
    assert np.array_equal((pl[:, :C] << 16)[~nan], img[~nan]), what
    assert ((pl[:, :C][nan] & 0x7FFF) > 0x7F80).all(), what
    assert not pl[:, C:].any(), what


QUANT_CONFIGS = [("lin", 1, 8), ("lin", 2, 4), ("lin", 0, 1), ("lin", -2, 3), ("lin", 7, 8),
                 ("log", 1, 2), ("log", 2, 3), ("log", 7, 4), ("log", 0, 6)]


@pytest.mark.gpu
def test_quantise_and_pack_equals_the_quantise_kernels(dev):
    shapes = [(37, 13), (5, 3), (130, 259), (64, 64), (9, 40), (2, 3, 40), (2, 3, 5, 7), (2, 13, 5, 7), (3, 40, 4, 6), (2, 64, 8, 8),
              (1, 130, 3, 5)]
    for ci, (dtype, fsr, bits) in enumerate(QUANT_CONFIGS):
        for sign in (True, False):            # Lin: mode 1 / 0; Log: with / without sign
            for si, shape in enumerate(shapes):
                if (ci + si + sign) % 2 and len(shape) != 4:       # every config on every 4-D shape, half of the row shapes
                    continue
                x = _edge_input(shape, fsr, dev, 100 * ci + si)
                views = [x] if len(shape) != 4 else [x, x.contiguous(memory_format=torch.channels_last)]
                for xv in views:
                    ref = ops.lin_quantize(xv, fsr, bits, 1 if sign else 0) if dtype == "lin" else ops.log_quantize(xv, fsr, bits, sign)
                    with calls() as c:
                        y, planes, layout = ops.quantize_levels_bf16(xv, dtype, fsr, bits, sign)
                    what = (dtype, fsr, bits, sign, shape, xv.stride())
                    assert c["qt_linlog_quantize_bf16_f32"] == 1 and c["qt_bf16x3_pack_f32"] == 0, what
                    assert c["qt_lin_quantize_f32"] == 0 and c["qt_log_quantize_f32"] == 0, what
                    assert y.stride() == xv.stride() and _same_nan(n(y), n(ref)), what
                    _plane_checks(y, planes, layout, what)
    # the module form tags its result; a tensor without a plane geometry (1-D, a strided view) takes the plain kernel, same bits
    q = log_lin_connect.nnQuant("lin", 1, 8, with_sign=False)
    x = _edge_input((2, 13, 5, 7), 1, dev, 7)
    with calls() as c:
        y = q(x)
    assert c["qt_linlog_quantize_bf16_f32"] == 1 and _same_nan(n(y), n(ops.lin_quantize(x, 1, 8, 0)))
    tag = packed.lookup_levels(y, packed.NHWC)
    assert tag is not None and packed.lookup_levels(y, packed.ROWS_LAST) is None
    _plane_checks(y, tag, packed.NHWC, "module")
    with calls() as c:
        y1 = q(x.view(-1))
        y2 = q(x[:, :, ::2])
    assert c["qt_linlog_quantize_bf16_f32"] == 0 and c["qt_lin_quantize_f32"] == 2
    assert _same_nan(n(y1), n(y).reshape(-1)) and _same_nan(n(y2), n(y)[:, :, ::2])
    with _fused.scope(LOGLIN_ONE_TERM=False), calls() as c:
        y3 = q(x)
    assert c["qt_linlog_quantize_bf16_f32"] == 0 and packed.lookup_levels(y3, packed.NHWC) is None and _same_nan(n(y3), n(y))
    # outside the one-term window the entry point refuses (the wrappers never send it there)
    with pytest.raises(ValueError):
        ops.quantize_levels_bf16(x, "lin", 1, 9)
    with pytest.raises(ValueError):
        ops.quantize_levels_bf16(x, "log", 1, 7)


@pytest.mark.gpu
def test_check_and_pack_of_untagged_activations(dev):
    edge = np.array([0.0, -0.0, 1.0, -1.5, 2.0 ** -126, 255.0, 257.0, 1.00390625, 0.1, 2.0 ** -127, 2.0 ** -133, 2.0 ** -149,
                     float("inf"), -float("inf"), float("nan")], np.float32)
    pats = np.array([0x3F808000, 0x7F800001, 0x7FC00000, 0x00010000, 0x00800000, 0x80000000], np.uint32).view(np.float32)
    for v, want in zip(np.concatenate([edge, pats]), bf16_exact_np(np.concatenate([edge, pats]))):
        host = np.ones((3, 50), np.float32)
        host.view(np.uint32)[1, 17] = np.array(v, np.float32).view(np.uint32)      # the bit pattern, NaN payloads included
        x = torch.from_numpy(host).to(dev)
        assert np.array_equal(n(x).view(np.uint32), host.view(np.uint32))
        assert ops.is_bf16_exact(x) == bool(want), v
        assert (int(ops.check_bf16_exact(x).item()) == 0) == bool(want), v
        planes, flag, layout = ops.pack_bf16_check(x)
        assert (int(flag.item()) == 0) == bool(want) and layout == packed.ROWS_LAST, v
    # an exact activation: the plane is the quantiser's own, in every layout
    for shape in [(37, 13), (130, 259), (2, 13, 5, 7), (3, 64, 4, 4), (2, 3, 6, 5)]:
        x = torch.randn(shape, device=dev) * 2
        views = [x] if len(shape) != 4 else [x, x.contiguous(memory_format=torch.channels_last)]
        for xv in views:
            y, want, layout = ops.quantize_levels_bf16(xv, "lin", 1, 8, True)
            with calls() as c:
                planes, flag, lay2 = ops.pack_bf16_check(y.clone(memory_format=torch.preserve_format))
            assert c["qt_bf16_pack_check_f32"] == 1 and lay2 == layout and int(flag.item()) == 0
            assert torch.equal(planes.data, want.data) and (planes.rows, planes.K, planes.terms) == (want.rows, want.K, 1)
            assert ops.is_bf16_exact(y) and not ops.is_bf16_exact(xv)
            bad = y.clone(memory_format=torch.preserve_format)
            bad[(-1,) * bad.dim()] = 0.3
            assert int(ops.pack_bf16_check(bad)[1].item()) != 0


def _levels_of(plane3, Cout, taps, Cin):
    """[Cout, taps, Cin] first slots of a three-term tap-major plane."""
    cb = ops.triple_ld_bytes(Cin, 16, 3) // 2
    return plane3.data[:, :taps * cb].view(Cout, taps, cb)[:, :, 0:3 * Cin:3]


@pytest.mark.gpu
def test_one_term_weight_planes(dev):
    from test_gpu_loglin_train import _bf16_nan_canon, _edge_weight
    for i, (dtype, fsr, bits, shape) in enumerate([("lin", 2, 8, (64, 3, 3, 3)), ("log", 2, 3, (13, 7, 1, 1)), ("lin", 1, 4, (20, 70, 5, 5)),
                                                   ("log", 1, 2, (128, 64, 3, 3)), ("lin", 0, 3, (7, 130, 3, 3)), ("lin", 1, 8, (10, 4096)),
                                                   ("log", 2, 3, (37, 13)), ("lin", 2, 4, (130, 259)), ("log", 1, 4, (5, 3))]):
        w = _edge_weight(shape, fsr, bits, dev, 40 + i)
        views = [w, w.contiguous(memory_format=torch.channels_last)] if len(shape) == 4 else [w, w.t().contiguous().t()]
        for wv in views:
            f3, g3, q3 = ops.pack_levels_bf16x3(wv, dtype, fsr, bits, image=True)
            with calls() as c:
                f1, g1, q1 = ops.pack_levels_bf16x3(wv, dtype, fsr, bits, image=True, fwd_terms=1)
            entry = "qt_bf16x1_pack_conv_levels_f32" if len(shape) == 4 else "qt_bf16x1_pack_levels_f32"
            assert c[entry] == 1 and sum(c.c.values()) == 1, dict(c.c)
            assert _same_nan(n(q1), n(q3)) and torch.equal(_bf16_nan_canon(g1.data), _bf16_nan_canon(g3.data))
            Cout, Cin = shape[0], shape[1]
            taps = shape[2] * shape[3] if len(shape) == 4 else 1
            cb1 = ops.triple_ld_bytes(Cin, 16, 1) // 2
            ld = max(128, (taps * cb1 * 2 + 127) // 128 * 128)
            assert f1.terms == 1 and f1.rows == Cout and tuple(f1.data.shape) == (Cout, ld // 2)
            assert f1.K == (taps * cb1 if len(shape) == 4 else Cin)
            got = f1.data[:, :taps * cb1].view(Cout, taps, cb1)
            assert torch.equal(_bf16_nan_canon(got[:, :, :Cin]), _bf16_nan_canon(_levels_of(f3, Cout, taps, Cin))), (dtype, shape)
            assert not got[:, :, Cin:].any() and not f1.data[:, taps * cb1:].any(), (dtype, shape)


# ---- bit-exact results where every partial sum is exact ----------------------------------------------------------------------------
# Activations Lin(fsr=1, bit_width=4, unsigned): multiples of 2^-3 up to 2 (<= 16 units); weights Lin(fsr=2, bit_width=4): multiples of
# 2^-2 up to 4 (<= 16 units): products <= 2^8 units of 2^-5, K <= 64 * 9 = 576 -> every partial sum is an integer below 2^18 units:
# exact in fp32 in any order.  Log activations (fsr=1, bit_width=2): +-2^e, e in [-3, 1]; Log weights (fsr=2, bit_width=2): +-2^e,
# e in [-2, 2]: the same units and bound.  Gradients: g = integers in [-8, 8] times 2^-4; grad_x sums <= 64 * 25 products of <= 128
# units of 2^-6, grad_W sums N Ho Wo <= 2048 products of <= 128 units of 2^-7: below 2^24 units too.  Hence torch.equal to the
# fp64 evaluation rounded once.

EXACT = {"lin": dict(act=("lin", 1, 4, False), w=(2, 4)), "log": dict(act=("log", 1, 2, True), w=(2, 2))}


def _exact_layer(kind, build, dev, seed, bias):
    torch.manual_seed(seed)
    fsr, bits = EXACT[kind]["w"]
    layer = build(fsr, bits, kind).to(dev)
    with torch.no_grad():
        if layer.bias is not None:
            layer.bias.copy_(torch.randint(-40, 41, layer.bias.shape).float() * 2.0 ** -5)
    return layer


def _exact_case(kind, layer, x_shape, dev, seed, conv):
    """Train (autograd), no-grad (train mode) and eval forwards of ``layer`` on a tagged quantised activation, against fp64."""
    torch.manual_seed(seed)
    q = log_lin_connect.nnQuant(*EXACT[kind]["act"][:3], with_sign=EXACT[kind]["act"][3])
    r = (torch.randn(x_shape, device=dev) * 1.5).requires_grad_(True)
    pack = "qt_bf16x1_pack_conv_levels_f32" if conv is not None else "qt_bf16x1_pack_levels_f32"
    layer.train(True)
    layer.zero_grad()
    with calls() as c:
        x = q(r)
        y = layer(x)
    assert c[pack] == 1 and c["qt_bf16x3_pack_f32"] == 0 and c["qt_bf16x6_pack_f32"] == 0, dict(c.c)
    gout = torch.randint(-8, 9, y.shape, device=dev).float() * 2.0 ** -4
    y.backward(gout)
    wq = layer.weight_op.forward(layer.weight.detach())
    b = layer.bias if layer.bias is not None else torch.zeros(layer.weight.shape[0], device=dev)
    ry, rgx, rgw, rgb = _ref_grads(x, wq, b, gout, conv)
    assert torch.equal(y.detach().cpu(), ry.float()), ("y", kind, x_shape)
    assert torch.equal(r.grad.cpu(), rgx.float()), ("grad_x", kind, x_shape)
    assert torch.equal(layer.weight.grad.cpu(), rgw.float()), ("grad_W", kind, x_shape)
    if layer.bias is not None:
        assert torch.equal(layer.bias.grad.cpu(), rgb.float()), ("grad_b", kind, x_shape)
    with torch.no_grad():
        with calls() as c:
            y1 = layer(q(r))
        assert c[pack] == 1 and c["qt_bf16x3_pack_f32"] == 0, dict(c.c)
        assert torch.equal(y1.cpu(), ry.float()), ("no-grad", kind, x_shape)
        layer.eval()
        with calls() as c:
            y2 = layer(q(r))
            y3 = layer(q(r))          # the one-term weight plane is cached
        assert c[pack] == 1 and c["qt_bf16x3_pack_f32"] == 0, dict(c.c)
        assert torch.equal(y2.cpu(), ry.float()) and torch.equal(y3.cpu(), ry.float()), ("eval", kind, x_shape)
    layer.train(True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lin", "log"])
def test_linear_bit_exact_where_sums_are_exact(dev, kind):
    for i, (x_shape, N, bias) in enumerate([((64, 576), 128, True), ((7, 37), 13, False), ((2, 3, 40), 24, True), ((33, 512), 10, True)]):
        layer = _exact_layer(kind, lambda f, b, d: LinearQuant(x_shape[-1], N, bias, dtype=d, fsr=f, bit_width=b), dev, i, bias)
        _exact_case(kind, layer, x_shape, dev, 10 + i, None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lin", "log"])
def test_conv_bit_exact_where_sums_are_exact(dev, kind):
    cases = [  # N, Cin, Cout, H, k, stride, padding, bias
        (2, 64, 32, 16, 3, 1, 1, True),          # 3 x 3 padded, K = 576: pixel-major grad_W
        (2, 64, 32, 16, 3, 1, 1, False),
        (2, 20, 40, 13, 5, 1, 2, True),          # 5 x 5 (Cin < 32: grad_W keeps the real-valued route)
        (2, 32, 40, 11, 5, 1, 2, True),          # 5 x 5 on the pixel-major kernel
        (3, 13, 7, 9, 1, 1, 0, True),            # 1 x 1
        (2, 128, 128, 8, 1, 1, 0, True),         # 1 x 1 on the K-major grad_W GEMMs
        (2, 16, 24, 17, 3, 2, 1, True),          # stride 2
        (2, 24, 16, 12, 1, 2, 0, True),          # 1 x 1, stride 2: the strided grad_W form
        (4, 3, 16, 10, 3, 1, 1, True),           # three channels
    ]
    for i, (N, Cin, Cout, H, k, s, p, bias) in enumerate(cases):
        layer = _exact_layer(kind, lambda f, b, d: QuantConv2d(Cin, Cout, k, stride=s, padding=p, bias=bias, fsr=f, bit_width=b, dtype=d),
                             dev, 20 + i, bias)
        before = dict(_fused.LIBRARY_PATHS)
        _exact_case(kind, layer, (N, Cin, H, H), dev, 30 + i, (s, p, 1))
        assert dict(_fused.LIBRARY_PATHS) == before, cases[i]
    # a channels-last activation
    layer = _exact_layer(kind, lambda f, b, d: QuantConv2d(64, 32, 3, padding=1, fsr=f, bit_width=b, dtype=d), dev, 60, True)
    torch.manual_seed(61)
    q = log_lin_connect.nnQuant(*EXACT[kind]["act"][:3], with_sign=EXACT[kind]["act"][3])
    r = (torch.randn((2, 64, 9, 9), device=dev) * 1.5).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    x = q(r)
    assert packed.lookup_levels(x, packed.NHWC) is not None
    y = layer(x)
    gout = torch.randint(-8, 9, y.shape, device=dev).float() * 2.0 ** -4
    y.backward(gout)
    ry, rgx, rgw, rgb = _ref_grads(x, layer.weight_op.forward(layer.weight.detach()), layer.bias, gout, (1, 1, 1))
    assert torch.equal(y.detach().cpu(), ry.float()) and torch.equal(r.grad.cpu(), rgx.float())
    assert torch.equal(layer.weight.grad.cpu(), rgw.float()) and torch.equal(layer.bias.grad.cpu(), rgb.float())


# ---- general inputs against fp64 ------------------------------------------------------------------------------------------------

def _check_quantised(layer, r, act, tagged, seed):
    torch.manual_seed(seed)
    q = log_lin_connect.nnQuant(*act[:3], with_sign=act[3])
    ri = r.clone(memory_format=torch.preserve_format).requires_grad_(True)
    x = q(ri)
    if not tagged:
        x = x * 1.0                       # the same values without the tag: the detection decides
        assert packed.lookup_levels(x, packed.NHWC) is None and packed.lookup_levels(x, packed.ROWS_LAST) is None
    layer.zero_grad()
    conv = None if isinstance(layer, LinearQuant) else (layer.stride, layer.padding, layer.dilation)
    with calls() as c:
        y = layer(x)
    assert c["qt_bf16x1_pack_levels_f32"] + c["qt_bf16x1_pack_conv_levels_f32"] == 1, dict(c.c)
    assert c["qt_bf16_pack_check_f32"] == (0 if tagged else 1) and c["qt_bf16x3_pack_f32"] == 0, dict(c.c)
    gout = torch.randn_like(y)
    y.backward(gout)
    wq = layer.weight_op.forward(layer.weight.detach())
    ry, rgx, rgw, rgb = _ref_grads(x, wq, layer.bias, gout, conv)
    for got, want, what in ((y, ry, "y"), (ri.grad, rgx, "grad_x"), (layer.weight.grad, rgw, "grad_W"), (layer.bias.grad, rgb, "grad_b")):
        assert got.shape == want.shape, what
        err = norm_err(n(got), want.numpy())
        assert err <= TOL, (what, err, tagged)


ACTS = [("lin", 1, 8, False), ("log", 1, 3, True)]


@pytest.mark.gpu
def test_linear_gradients_vs_fp64_on_quantised_activations(dev):
    from test_gpu_loglin_train import _init
    for i, (dtype, fsr, bits, M, K, N) in enumerate([("lin", 1, 8, 64, 4096, 1024), ("lin", 2, 3, 7, 37, 13), ("log", 1, 3, 32, 1024, 10),
                                                     ("log", 0, 4, 5, 300, 77)]):
        layer = _init(LinearQuant(K, N, True, dtype=dtype, fsr=fsr, bit_width=bits), dev, i)
        r = torch.randn((M, K), device=dev)
        for act in ACTS:
            for tagged in (True, False):
                _check_quantised(layer, r, act, tagged, 10 + i)
    layer = _init(LinearQuant(40, 24, True, dtype="lin", fsr=0, bit_width=5), dev, 9)
    _check_quantised(layer, torch.randn((2, 3, 40), device=dev), ACTS[0], True, 19)          # a 3-D input
    _check_quantised(layer, torch.randn((2, 3, 40), device=dev), ACTS[1], False, 19)


@pytest.mark.gpu
def test_conv_gradients_vs_fp64_on_quantised_activations(dev):
    from test_gpu_loglin_train import _init
    cases = [  # dtype, fsr, bits, N, Cin, Cout, H, k, stride, padding, dilation  (tests/test_gpu_loglin_train.py)
        ("lin", 2, 8, 4, 3, 64, 32, 3, 1, 1, 1),
        ("log", 2, 3, 2, 3, 96, 67, 11, 4, 2, 1),
        ("lin", 2, 8, 2, 64, 128, 16, 3, 1, 1, 1),
        ("log", 1, 3, 2, 40, 20, 15, 5, 2, 2, 1),
        ("lin", 1, 4, 3, 13, 7, 9, 1, 1, 0, 1),
        ("log", 2, 2, 2, 16, 24, 17, 3, 2, 0, 1),
        ("lin", 0, 6, 2, 24, 16, 19, 3, 4, 1, 1),
    ]
    for i, (dtype, fsr, bits, N, Cin, Cout, H, k, s, p, d) in enumerate(cases):
        layer = _init(QuantConv2d(Cin, Cout, k, stride=s, padding=p, dilation=d, fsr=fsr, bit_width=bits, dtype=dtype), dev, i)
        r = torch.randn((N, Cin, H, H), device=dev)
        for rv in (r, r.contiguous(memory_format=torch.channels_last)):
            for act in ACTS:
                for tagged in (True, False):
                    before = dict(_fused.LIBRARY_PATHS)
                    _check_quantised(layer, rv, act, tagged, 20 + i)
                    assert dict(_fused.LIBRARY_PATHS) == before, (cases[i], dict(_fused.LIBRARY_PATHS))


# ---- routes -------------------------------------------------------------------------------------------------------------------

def _vgg_counts(dev, dtype, bits, one_term):
    torch.manual_seed(3)
    model = _VGGLinLog(dtype, bits).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    x, t = torch.randn((32, 3, 32, 32), device=dev), torch.randint(0, 10, (32,), device=dev)
    with _fused.scope(LOGLIN_ONE_TERM=one_term):
        _fused.reset_detection()
        _step(model, opt, x, t)
        _fused.LIBRARY_PATHS.clear()
        with calls() as step:
            loss = _step(model, opt, x, t)
        assert not _fused.LIBRARY_PATHS, dict(_fused.LIBRARY_PATHS)
        assert bool(torch.isfinite(loss))
        model.eval()
        with torch.no_grad():
            y0 = model(x)
            with calls() as ev:
                y1 = model(x)
        assert torch.equal(y0, y1) and not _fused.LIBRARY_PATHS
    return step, ev, y1


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,bits", [("lin", 8), ("log", 3)])
def test_vgg_routes_by_call_counts(dev, dtype, bits):
    step, ev, y_on = _vgg_counts(dev, dtype, bits, True)
    # training step: five convs and three linears behind a quantiser (or its pooled / flattened output) on one-term planes, the
    # first conv (a real image) on the three-term route
    assert step["qt_bf16x1_pack_conv_levels_f32"] == 5 and step["qt_bf16x3_pack_conv_levels_f32"] == 1, dict(step.c)
    assert step["qt_bf16x1_pack_levels_f32"] == 3 and step["qt_bf16x3_pack_levels_f32"] == 0, dict(step.c)
    assert step["qt_linlog_quantize_bf16_f32"] == 8 and step["qt_lin_quantize_f32"] == 0, dict(step.c)
    assert step["qt_bf16_pack_check_f32"] == 3, dict(step.c)                  # two pooled conv inputs, the flattened one
    assert step["qt_bf16x6_pack_f32"] == 0, dict(step.c)                      # no six-term split: grad_W of the linears
    assert step["qt_wgrad_pm_pack_act_f32"] == 5, dict(step.c)                # conv grad_W: the activation as it is, bf16
    first_conv_splits = step["qt_wgrad_pm_pack_act_s2d_f32"] + step["qt_wgrad_pm_pack_act_s2d_f16x2"]
    assert first_conv_splits == 1, dict(step.c)                               # only the first conv splits its (real) image
    # eval forward, second call: weight planes cached, one activation split (the image), eight one-term contractions
    assert ev["qt_bf16x3_pack_f32"] == 1 and ev["qt_bf16x1_pack_conv_levels_f32"] == 0 and ev["qt_bf16x1_pack_levels_f32"] == 0, dict(ev.c)
    assert ev["qt_linlog_quantize_bf16_f32"] == 8 and ev["qt_bf16_pack_check_f32"] == 3, dict(ev.c)
    assert ev["qt_conv2d_implicit"] + ev["qt_conv2d_implicit_variant"] == 6 and ev["qt_bf16_gemm"] == 3, dict(ev.c)
    # switched off: the counts of the three-term route, as before this route existed
    step0, ev0, y_off = _vgg_counts(dev, dtype, bits, False)
    for k in ("qt_bf16x1_pack_conv_levels_f32", "qt_bf16x1_pack_levels_f32", "qt_linlog_quantize_bf16_f32", "qt_bf16_pack_check_f32",
              "qt_check_bf16_exact_f32", "qt_wgrad_pm_pack_act_f32"):
        assert step0[k] == 0 and ev0[k] == 0, (k, dict(step0.c), dict(ev0.c))
    assert step0["qt_bf16x3_pack_conv_levels_f32"] == 6 and step0["qt_bf16x3_pack_levels_f32"] == 3, dict(step0.c)
    assert step0["qt_lin_quantize_f32"] == 8 and step0["qt_bf16x6_pack_f32"] == 6, dict(step0.c)
    assert step0["qt_wgrad_pm_pack_act_s2d_f32"] + step0["qt_wgrad_pm_pack_act_s2d_f16x2"] == 6, dict(step0.c)
    # (in eval mode LinearQuant re-applies its weight quantiser, like upstream: three more Lin launches for the Lin net)
    assert ev0["qt_bf16x3_pack_f32"] == 9 and ev0["qt_lin_quantize_f32"] == 8 + (3 if dtype == "lin" else 0), dict(ev0.c)
    assert ev["qt_lin_quantize_f32"] == 0, dict(ev.c)
    assert bool(torch.isfinite(y_on).all()) and bool(torch.isfinite(y_off).all())


# ---- detection ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_untagged_exact_activations_take_the_one_term_route(dev):
    torch.manual_seed(4)
    q = log_lin_connect.nnQuant("lin", 1, 8, with_sign=False)
    conv = QuantConv2d(32, 48, 3, padding=1, fsr=2, bit_width=8).to(dev)
    lin = LinearQuant(32 * 16, 20, fsr=1, bit_width=8).to(dev)
    with torch.no_grad():
        a = q(torch.randn((4, 32, 8, 8), device=dev))
        pooled = F.max_pool2d(a, 2)
        assert packed.lookup_levels(pooled, packed.NHWC) is None
        for layer, x in ((conv, pooled), (lin, pooled.flatten(1)), (lin, pooled.reshape(2, 2, -1))):
            with calls() as c:
                y = layer(x)
            assert c["qt_bf16_pack_check_f32"] == 1 and c["qt_bf16x3_pack_f32"] == 0, dict(c.c)
            assert c["qt_bf16x1_pack_conv_levels_f32"] + c["qt_bf16x1_pack_levels_f32"] == 1, dict(c.c)
            with _fused.scope(LOGLIN_ONE_TERM=False):
                want = layer(x)
            assert norm_err(n(y), n(want)) <= TOL
        # a real-valued activation does not; the second call takes the negative verdict from the cache, without a check
        xr = torch.randn((4, 32, 4, 4), device=dev)
        with calls() as c:
            y = conv(xr)
        assert c["qt_bf16_pack_check_f32"] == 1 and c["qt_bf16x3_pack_f32"] >= 1 and c["qt_bf16x1_pack_conv_levels_f32"] == 0, dict(c.c)
        cached, sync = _fused.DETECT_STATS["cached"], _fused.DETECT_STATS["sync"]
        with calls() as c:
            y2 = conv(xr)
        assert c["qt_bf16_pack_check_f32"] == 0 and c["qt_bf16x3_pack_f32"] >= 1, dict(c.c)
        assert _fused.DETECT_STATS["cached"] == cached + 1 and _fused.DETECT_STATS["sync"] == sync
        with _fused.scope(LOGLIN_ONE_TERM=False):
            assert torch.equal(y, conv(xr)) and torch.equal(y2, y)


@pytest.mark.gpu
def test_remembered_verdicts_do_not_sync_and_poison_when_broken(dev):
    torch.manual_seed(6)
    model = _VGGLinLog("lin", 8, width=16).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    x, t = torch.randn((8, 3, 32, 32), device=dev), torch.randint(0, 10, (8,), device=dev)
    with _fused.detect_scope("remember"):
        _step(model, opt, x, t)
        sync = _fused.DETECT_STATS["sync"]
        with calls() as c:
            _step(model, opt, x, t)
        assert _fused.DETECT_STATS["sync"] == sync
        assert c["qt_bf16_pack_check_f32"] == 3 and c["qt_bf16x1_pack_conv_levels_f32"] == 5, dict(c.c)
        # a remembered "exact" verdict and an activation of the same shape that is not: NaN, never numbers
        q = log_lin_connect.nnQuant("lin", 1, 8, with_sign=False)
        conv = QuantConv2d(16, 24, 3, padding=1, fsr=2, bit_width=8).to(dev)
        lin = LinearQuant(40, 12, fsr=1, bit_width=8).to(dev)
        with torch.no_grad():
            good4, good2 = q(torch.randn((2, 16, 6, 6), device=dev)) * 1.0, q(torch.randn((5, 40), device=dev)) * 1.0
            for layer, good in ((conv, good4), (lin, good2)):
                y = layer(good)                                       # asked and remembered
                assert bool(torch.isfinite(y).all())
                y = layer(good)                                       # trusted: the flag rides in the bias
                assert bool(torch.isfinite(y).all())
                y = layer(torch.randn_like(good))
                assert bool(torch.isnan(y).all())
        xi = torch.randn_like(good4).requires_grad_(True)             # and under autograd
        assert bool(torch.isnan(conv(xi)).all())


@pytest.mark.gpu
def test_graph_captured_step_on_the_one_term_route_matches_eager(dev):
    from pytorch_quantize_impls_amd.utils import GraphedTrainStep
    for dtype, bits in (("lin", 8), ("log", 3)):
        torch.manual_seed(5)
        a = _VGGLinLog(dtype, bits, width=16).to(dev)
        b = _VGGLinLog(dtype, bits, width=16).to(dev)
        b.load_state_dict(a.state_dict())
        oa, ob = torch.optim.SGD(a.parameters(), lr=0.05), torch.optim.SGD(b.parameters(), lr=0.05)
        xs = [torch.randn((16, 3, 32, 32), device=dev) for _ in range(3)]
        ts = [torch.randint(0, 10, (16,), device=dev) for _ in range(3)]
        with calls() as c:
            step = GraphedTrainStep(b, lambda out, t: F.nll_loss(out, t), xs[0], ts[0])
        assert c["qt_bf16x1_pack_conv_levels_f32"] >= 5 and c["qt_bf16x1_pack_levels_f32"] >= 3, dict(c.c)
        assert c["qt_linlog_quantize_bf16_f32"] >= 8 and c["qt_bf16_pack_check_f32"] >= 3 and c["qt_bf16x6_pack_f32"] == 0, dict(c.c)
        for x, t in zip(xs, ts):
            _step(a, oa, x, t)
            step(x, t)
            ob.step()
            b.clamp()
        torch.cuda.synchronize()
        for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
            assert norm_err(n(pb), n(pa)) <= TOL, (dtype, name)
