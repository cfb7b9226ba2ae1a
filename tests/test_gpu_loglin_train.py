"""Lin / Log fixed-point layers in training mode on the matrix cores (functions/_fused.py LogLinLinearFn / LogLinConv2dFn, the
quantise-and-pack kernel csrc/loglin_pack.hip): operand planes bit for bit, gradients against an fp64 evaluation of the reference
expression F.linear / F.conv2d(x, Q(W), b), no dense library in a training step, graph capture, unchanged no-grad / eval routes."""
import glob
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import norm_err
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused, log_lin_connect
from pytorch_quantize_impls_amd.layers import LinearQuant, QuantConv2d

TOL = 1e-5
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    assert _lib.device_info()[0].startswith("gfx950")
    return torch.device("cuda:0")


def n(t):
    return t.detach().cpu().numpy()


def _quant(w, dtype, fsr, bits):
    """The existing quantise kernels' image (what the layers' weight_op computes on the device)."""
    return ops.lin_quantize(w, fsr, bits, 1) if dtype == "lin" else ops.log_quantize(w, fsr, bits, True)


def _bf16_nan_canon(p: torch.Tensor) -> torch.Tensor:
    """int16 plane with every bf16 NaN pattern replaced by one quiet NaN (payloads are not part of the contract)."""
    v = p.to(torch.int32) & 0xFFFF
    return torch.where((v & 0x7FFF) > 0x7F80, torch.full_like(v, 0x7FC0), v)


def _same_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])


def _edge_weight(shape, fsr, bits, dev, seed):
    """Random weight of roughly the level range with edge values planted: +-0, +-inf, NaN, exact round-half ties, |w| above 2^fsr,
    tiny |w|."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(shape, generator=g) * 2 - 1) * 2.0 ** fsr * 1.3
    flat = w.view(-1)
    step = 2.0 ** (fsr - bits)
    edge = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), 2.0 ** fsr * 3, -(2.0 ** fsr) * 5, 1e-30, -1e-38, 1e-45,
            step * 0.5, -step * 1.5, step * 2.5, 2.0 ** (fsr - 0.5), -(2.0 ** (fsr - 2.5))]
    for i, v in enumerate(edge):
        if i * 7 < flat.numel():
            flat[i * 7] = v
    return w.to(dev)


def _configs():
    for bits in (1, 3, 8):
        for fsr in (-2, 0, 1, 2, 7):
            yield "lin", fsr, bits
    for bits in (2, 3, 4):
        for fsr in (-2, 1, 7):
            yield "log", fsr, bits


@pytest.mark.gpu
def test_linear_planes_equal_existing_packs(dev):
    shapes = [(10, 4096), (37, 13), (1024, 1024), (5, 3), (130, 259), (9, 21)]      # K = 21: 126 of 128 bytes
    for ci, (dtype, fsr, bits) in enumerate(_configs()):
        for si, (N, K) in enumerate(shapes):
            w = _edge_weight((N, K), fsr, bits, dev, 100 * ci + si)
            for wv in (w, w.t().contiguous().t()):            # contiguous and column-major
                fwd, gx, wq = ops.pack_levels_bf16x3(wv, dtype, fsr, bits, image=True)
                ref = _quant(w, dtype, fsr, bits)
                assert _same_nan(n(wq), n(ref)), (dtype, fsr, bits, N, K)
                assert wq.stride() == wv.stride()
                want_f = ops.weight_bf16x3(ref, "raw", terms=3)
                want_g = ops.weight_bf16x3(ref.t().contiguous(), "raw", terms=3)
                assert fwd.data.shape == want_f.data.shape and gx.data.shape == want_g.data.shape
                assert torch.equal(_bf16_nan_canon(fwd.data), _bf16_nan_canon(want_f.data)), (dtype, fsr, bits, N, K)
                assert torch.equal(_bf16_nan_canon(gx.data), _bf16_nan_canon(want_g.data)), (dtype, fsr, bits, N, K)
                assert (fwd.rows, fwd.K, gx.rows, gx.K) == (N, K, K, N)


@pytest.mark.gpu
def test_conv_planes_equal_existing_packs(dev):
    shapes = [(64, 3, 3), (13, 7, 1), (96, 3, 11), (20, 70, 5), (128, 64, 3), (7, 130, 3), (200, 9, 1)]
    for ci, (dtype, fsr, bits) in enumerate(_configs()):
        for si, (Cout, Cin, k) in enumerate(shapes):
            if (ci + si) % 3:                                  # a third of the product, every shape and config still covered
                continue
            w = _edge_weight((Cout, Cin, k, k), fsr, bits, dev, 1000 * ci + si)
            ref = _quant(w, dtype, fsr, bits)
            want_f = ops.pack_conv_weight_bf16x3(ref, "raw", terms=3)
            want_g = ops.pack_conv_weight_bf16x3(ref, "raw", terms=3, transpose_flip=True)
            for wv in (w, w.contiguous(memory_format=torch.channels_last)):
                fwd, gx, wq = ops.pack_levels_bf16x3(wv, dtype, fsr, bits, image=True)
                assert _same_nan(n(wq), n(ref)) and wq.stride() == wv.stride(), (dtype, fsr, bits, Cout, Cin, k)
                assert torch.equal(_bf16_nan_canon(fwd.data), _bf16_nan_canon(want_f.data)), (dtype, fsr, bits, Cout, Cin, k)
                assert torch.equal(_bf16_nan_canon(gx.data), _bf16_nan_canon(want_g.data)), (dtype, fsr, bits, Cout, Cin, k)
    # one plane alone, and the image alone
    w = _edge_weight((24, 40, 3, 3), 1, 3, dev, 7)
    fwd, gx, wq = ops.pack_levels_bf16x3(w, "log", 1, 3, grad_x=False)
    assert gx is None and wq is None
    assert torch.equal(_bf16_nan_canon(fwd.data), _bf16_nan_canon(ops.pack_conv_weight_bf16x3(_quant(w, "log", 1, 3), "raw", terms=3).data))
    _, _, wq = ops.pack_levels_bf16x3(w, "lin", 2, 8, forward=False, grad_x=False, image=True)
    assert _same_nan(n(wq), n(_quant(w, "lin", 2, 8)))


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


def _ref_grads(x, wq, b, gout, conv_args=None):
    """fp64 evaluation of F.linear / F.conv2d(x, Q(W), b) and its gradients wrt x, Q(W) (= grad_W, identity backward) and b."""
    xd = x.detach().cpu().double().requires_grad_(True)
    wd = wq.detach().cpu().double().requires_grad_(True)
    bd = b.detach().cpu().double().requires_grad_(True)
    y = F.linear(xd, wd, bd) if conv_args is None else F.conv2d(xd, wd, bd, *conv_args)
    y.backward(gout.detach().cpu().double())
    return y.detach(), xd.grad, wd.grad, bd.grad


def _check_layer(layer, x, seed):
    torch.manual_seed(seed)
    xi = x.clone().requires_grad_(True)
    y = layer(xi)
    gout = torch.randn_like(y)
    y.backward(gout)
    wq = layer.weight_op.forward(layer.weight.detach())
    conv = None if isinstance(layer, LinearQuant) else (layer.stride, layer.padding, layer.dilation)
    ry, rgx, rgw, rgb = _ref_grads(x, wq, layer.bias, gout, conv)
    for got, want, what in ((y, ry, "y"), (xi.grad, rgx, "grad_x"), (layer.weight.grad, rgw, "grad_W"), (layer.bias.grad, rgb, "grad_b")):
        assert got.shape == want.shape, what
        assert norm_err(n(got), want.numpy()) <= TOL, (what, norm_err(n(got), want.numpy()))


def _init(layer, dev, seed):
    torch.manual_seed(seed)
    layer = layer.to(dev)
    with torch.no_grad():
        layer.bias.uniform_(-0.5, 0.5)
    return layer


@pytest.mark.gpu
def test_linear_gradients_vs_fp64(dev):
    for i, (dtype, fsr, bits, M, K, N) in enumerate([("lin", 1, 8, 64, 4096, 1024), ("lin", 2, 3, 7, 37, 13), ("log", 1, 3, 32, 1024, 10),
                                                     ("log", 0, 4, 5, 300, 77)]):
        layer = _init(LinearQuant(K, N, True, dtype=dtype, fsr=fsr, bit_width=bits), dev, i)
        x = torch.randn((M, K), device=dev)
        names = _kernels(lambda: _check_layer(layer, x, 10 + i))
        assert any("level_pack_kernel" in k for k in names), names
    x3 = torch.randn((2, 3, 40), device=dev)                                 # a 3-D input
    _check_layer(_init(LinearQuant(40, 24, True, dtype="lin", fsr=0, bit_width=5), dev, 9), x3, 19)


@pytest.mark.gpu
def test_conv_gradients_vs_fp64(dev):
    cases = [  # dtype, fsr, bits, N, Cin, Cout, H, k, stride, padding, dilation
        ("lin", 2, 8, 4, 3, 64, 32, 3, 1, 1, 1),       # 3-channel first layer
        ("log", 2, 3, 2, 3, 96, 67, 11, 4, 2, 1),      # Cin = 3, 11 x 11, stride 4
        ("lin", 2, 8, 2, 64, 128, 16, 3, 1, 1, 1),
        ("log", 1, 3, 2, 40, 20, 15, 5, 2, 2, 1),
        ("lin", 1, 4, 3, 13, 7, 9, 1, 1, 0, 1),
        ("log", 2, 2, 2, 16, 24, 17, 3, 2, 0, 1),
        ("lin", 0, 6, 2, 24, 16, 19, 3, 4, 1, 1),
    ]
    for i, (dtype, fsr, bits, N, Cin, Cout, H, k, s, p, d) in enumerate(cases):
        layer = _init(QuantConv2d(Cin, Cout, k, stride=s, padding=p, dilation=d, fsr=fsr, bit_width=bits, dtype=dtype), dev, i)
        x = torch.randn((N, Cin, H, H), device=dev)
        for xv in (x, x.contiguous(memory_format=torch.channels_last)):
            layer.zero_grad()
            before = dict(_fused.LIBRARY_PATHS)
            names = _kernels(lambda: _check_layer(layer, xv, 20 + i))
            assert dict(_fused.LIBRARY_PATHS) == before, (cases[i], dict(_fused.LIBRARY_PATHS))
            assert any("level_pack_kernel" in k for k in names), names
    # dilation 2: grad_x takes the counted library helper on the packed fp32 image, the rest stays on the kernels
    layer = _init(QuantConv2d(8, 16, 3, padding=2, dilation=2, fsr=1, bit_width=3, dtype="log"), dev, 50)
    x = torch.randn((2, 8, 14, 14), device=dev)
    before = _fused.LIBRARY_PATHS["conv grad_input outside the matrix-core route"]
    _check_layer(layer, x, 51)
    assert _fused.LIBRARY_PATHS["conv grad_input outside the matrix-core route"] == before + 1


@pytest.mark.gpu
def test_levels_beyond_bf16_take_the_six_term_routes(dev):
    for i, (dtype, fsr, bits) in enumerate([("lin", 2, 12), ("lin", 1, 32), ("log", 0, 7)]):
        assert not ops.levels_exact_in_bf16(dtype, fsr, bits)
        lin = _init(LinearQuant(96, 40, True, dtype=dtype, fsr=fsr, bit_width=bits), dev, i)
        conv = _init(QuantConv2d(8, 16, 3, padding=1, fsr=fsr, bit_width=bits, dtype=dtype), dev, 10 + i)
        before = dict(_fused.LIBRARY_PATHS)
        for layer, x in ((lin, torch.randn((9, 96), device=dev)), (conv, torch.randn((2, 8, 10, 10), device=dev))):
            names = _kernels(lambda: _check_layer(layer, x, 30 + i))
            assert any("sext_kernel" in k for k in names), names             # six-term planes of Q(W) (forward, grad_x)
            assert not any("level_pack_kernel" in k for k in names), names
        assert dict(_fused.LIBRARY_PATHS) == before


class _VGGLinLog(torch.nn.Module):
    """Shaped like the reference's models/samples/VGG16_LinLogQuant.py (CIFAR-10): six 3 x 3 QuantConv2d with BatchNorm, ReLU and the
    nnQuant(fsr=1, bit_width=8, with_sign=False) activation quantiser, three LinearQuant; ``width`` scales the channels."""

    def __init__(self, dtype="lin", bits=8, width=64):
        super().__init__()
        c1, c2, c3 = width, 2 * width, 4 * width
        self.quant_act = log_lin_connect.nnQuant(fsr=1, bit_width=8, with_sign=False)
        chans = [(3, c1), (c1, c1), (c1, c2), (c2, c2), (c2, c3), (c3, c3)]
        self.convs = torch.nn.ModuleList(QuantConv2d(a, b, 3, padding=1, fsr=2, bit_width=bits, dtype=dtype) for a, b in chans)
        self.bns = torch.nn.ModuleList(torch.nn.BatchNorm2d(b) for _, b in chans)
        self.lins = torch.nn.ModuleList([LinearQuant(c3 * 16, 4 * c3, fsr=1, bit_width=bits, dtype=dtype),
                                         LinearQuant(4 * c3, 4 * c3, fsr=1, bit_width=bits, dtype=dtype),
                                         LinearQuant(4 * c3, 10, fsr=1, bit_width=bits, dtype=dtype)])
        self.bn1d = torch.nn.ModuleList([torch.nn.BatchNorm1d(4 * c3), torch.nn.BatchNorm1d(4 * c3)])

    def clamp(self):
        for m in list(self.convs) + list(self.lins):
            m.clamp()

    def forward(self, x):
        for i, (conv, bn) in enumerate(zip(self.convs, self.bns)):
            x = self.quant_act(torch.relu(bn(conv(x))))
            if i % 2 == 1:
                x = F.max_pool2d(x, 2)
        x = x.flatten(1)
        for lin, bn in zip(self.lins[:2], self.bn1d):
            x = self.quant_act(torch.relu(bn(lin(x))))
        return F.log_softmax(self.lins[2](x), 1)


def _our_kernel_names():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "pytorch_quantize_impls_amd", "csrc", "*.h*")):
        with open(path) as fh:
            names.update(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", fh.read()))
    return names


def _step(model, opt, x, t):
    opt.zero_grad()
    loss = F.nll_loss(model(x), t)
    loss.backward()
    opt.step()
    model.clamp()
    return loss


@pytest.mark.gpu
def test_training_step_uses_no_dense_library(dev):
    ours = _our_kernel_names()
    assert "level_pack_kernel" in ours
    for dtype, bits in (("lin", 8), ("log", 3)):
        torch.manual_seed(3)
        model = _VGGLinLog(dtype, bits).to(dev)
        opt = torch.optim.SGD(model.parameters(), lr=0.01)
        x, t = torch.randn((32, 3, 32, 32), device=dev), torch.randint(0, 10, (32,), device=dev)
        _step(model, opt, x, t)
        _fused.LIBRARY_PATHS.clear()
        names = _kernels(lambda: _step(model, opt, x, t))
        assert not _fused.LIBRARY_PATHS, dict(_fused.LIBRARY_PATHS)
        foreign = [k for k in names if not any(o in k for o in ours)]
        lib = [k for k in foreign if any(tok in k.lower() for tok in ("gemm", "conv", "cijk", "blas", "winograd"))]
        assert not lib, lib
        assert any("level_pack_kernel" in k for k in names), names


@pytest.mark.gpu
def test_graph_captured_step_matches_eager(dev):
    from pytorch_quantize_impls_amd.utils import GraphedTrainStep
    for dtype, bits in (("lin", 8), ("log", 3)):
        torch.manual_seed(5)
        a = _VGGLinLog(dtype, bits, width=16).to(dev)
        b = _VGGLinLog(dtype, bits, width=16).to(dev)
        b.load_state_dict(a.state_dict())
        oa, ob = torch.optim.SGD(a.parameters(), lr=0.05), torch.optim.SGD(b.parameters(), lr=0.05)
        xs = [torch.randn((16, 3, 32, 32), device=dev) for _ in range(3)]
        ts = [torch.randint(0, 10, (16,), device=dev) for _ in range(3)]
        # (the warm-up calls of GraphedTrainStep advance BatchNorm's running statistics only; training-mode outputs use batch ones)
        step = GraphedTrainStep(b, lambda out, t: F.nll_loss(out, t), xs[0], ts[0])
        for x, t in zip(xs, ts):
            _step(a, oa, x, t)
            step(x, t)
            ob.step()
            b.clamp()
        torch.cuda.synchronize()
        for (name, pa), pb in zip(a.named_parameters(), b.parameters()):
            assert norm_err(n(pb), n(pa)) <= TOL, (dtype, name)


@pytest.mark.gpu
def test_no_grad_and_eval_forwards_unchanged(dev):
    torch.manual_seed(8)
    for dtype, fsr, bits in (("lin", 1, 8), ("log", 2, 3)):
        lin = LinearQuant(200, 48, True, dtype=dtype, fsr=fsr, bit_width=bits).to(dev)
        conv = QuantConv2d(16, 32, 3, padding=1, fsr=fsr, bit_width=bits, dtype=dtype).to(dev)
        x2, x4 = torch.randn((12, 200), device=dev), torch.randn((3, 16, 11, 11), device=dev)
        for mode in (True, False):
            lin.train(mode)
            conv.train(mode)
            with torch.no_grad():
                wq = lin.weight_op.forward(lin.weight)
                want = ops.float_linear(x2, wq, "raw", lin.bias, terms=3)
                assert torch.equal(lin(x2), want)
                cw = conv.weight_op.forward(conv.weight) if mode else conv.weight
                y2 = ops.float_conv2d(x4, cw, "raw", conv.bias, 1, 1, 1, terms=3)
                assert torch.equal(conv(x4), y2.view(3, 11, 11, 32).permute(0, 3, 1, 2).contiguous())
        # eval mode with autograd: the swapped weight, on the new Functions, same values as the no-grad eval forward
        xi = x4.clone().requires_grad_(True)
        y = conv(xi)
        with torch.no_grad():
            ye = conv(x4)
        assert norm_err(n(y), n(ye)) <= TOL
        conv.train(True)
        lin.train(True)
