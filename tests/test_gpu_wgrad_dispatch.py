"""One case per rung of the weight-gradient ladder and per layer family, through the layers' public entry points.

Each case runs one training-mode forward / backward on an activation that carries its quantiser's tag and asserts (a) from the
C-ABI call counters which weight-gradient entries ran and which did not, (b) that no dense-library path was counted, (c) grad_W
(and the bias gradient, where the route produces it on the way) against torch.nn.grad.conv2d_weight in float64 with the family's
mask or scale, at the bar tests/test_gpu_r2.py holds these routes to.  The shapes are those of tests/test_wgrad_dispatch_cpu.py:
the smallest for which each rung's predicate holds and no earlier one's does.  Nothing here names a helper of the dispatch, so
the file is independent of how the routes are walked."""
import pytest
import torch

from conftest import norm_err
from test_gpu_r2 import TOL

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib, lazy_train, ops  # noqa: E402
from pytorch_quantize_impls_amd.functions import BinaryConnectDeterministic, nnDorefaQuant  # noqa: E402
from pytorch_quantize_impls_amd.functions import _fused, log_lin_connect, xnor_connect  # noqa: E402
from pytorch_quantize_impls_amd.layers import BinConv2d, DorefaConv2d, QuantConv2d  # noqa: E402

# (N, Cin, Cout, H, k, stride, padding)
PM3, GEMM1, GEMM7 = (3, 32, 32, 8, 3, 1, 1), (2, 128, 128, 6, 1, 1, 0), (2, 128, 128, 8, 7, 1, 3)
STRIDED3, STRIDED1, SWAPPED, IMG3, PM3_S2 = (3, 8, 32, 8, 3, 2, 1), (3, 16, 24, 8, 1, 2, 0), (4, 32, 64, 8, 7, 1, 3), (2, 3, 32, 8, 3, 1, 1), (3, 32, 32, 8, 3, 2, 1)

PM_F16, PM_F32, PM_REDUCE, PM_BIAS = "qt_wgrad_pm_f16", "qt_wgrad_pm_f32", "qt_wgrad_pm_reduce_f32", "qt_wgrad_pm_bias_reduce_f32"
PM_ACT, PM_ACT_S2D = "qt_wgrad_pm_pack_act_f16", "qt_wgrad_pm_pack_act_s2d_f16x2"
GEMM_TAPS, GEMM_ACT, GEMM_REDUCE = "qt_bf16_gemm_taps", "qt_wgrad_pack_act_f32", "qt_wgrad_reduce_f32"
#: the entries of each rung under the default two-term split: (ran, did not run)
RUNG = {"pm": ((PM_F16, PM_ACT, PM_REDUCE), (GEMM_TAPS, GEMM_REDUCE, PM_F32, PM_ACT_S2D)),
        "gemm": ((GEMM_TAPS, GEMM_ACT, GEMM_REDUCE), (PM_F16, PM_F32, PM_REDUCE)),
        "strided k x k": ((PM_F16, PM_ACT, PM_REDUCE), (GEMM_TAPS, GEMM_REDUCE, PM_F32, PM_ACT_S2D)),
        "strided 1 x 1": ((GEMM_TAPS, GEMM_ACT, GEMM_REDUCE), (PM_F16, PM_F32, PM_REDUCE)),
        "s2d": ((PM_F16, PM_ACT_S2D, PM_REDUCE), (GEMM_TAPS, GEMM_REDUCE, PM_F32, PM_ACT))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def counted(fn):
    """(fn(), C-ABI call-count deltas, dense-library path deltas)."""
    calls, lib = dict(_lib.call_counts), dict(_fused.LIBRARY_PATHS)
    out = fn()
    torch.cuda.synchronize()
    dcalls = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
    dlib = {k: v - lib.get(k, 0) for k, v in _fused.LIBRARY_PATHS.items() if v != lib.get(k, 0)}
    return out, dcalls, dlib


def assert_route(calls, lib, ran, absent, what):
    print(f"{what}: entries {sorted(calls)}; library {lib}")
    assert not lib, f"{what}: dense-library paths taken: {lib}"
    missing = [e for e in ran if not calls.get(e)]
    assert not missing, f"{what}: route entries {missing} did not run; ran {sorted(calls)}"
    extra = [e for e in absent if calls.get(e)]
    assert not extra, f"{what}: entries {extra} ran"


def assert_close(got, want64, what):
    err = norm_err(got.detach().cpu().numpy(), want64.cpu().numpy())
    print(f"{what}: error {err:.3g}")
    assert err <= TOL, f"{what}: {err:.3g} > {TOL}"


def operands(shape, dev, seed, pm1=True):
    N, Cin, Cout, H, k, s, p = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.where(torch.rand((N, Cin, H, H), generator=gen) < 0.5, -1.0, 1.0) if pm1 else torch.randn((N, Cin, H, H), generator=gen)
    Ho = (H + 2 * p - k) // s + 1
    g = torch.randn((N, Cout, Ho, Ho), generator=gen)
    w = torch.rand((Cout, Cin, k, k), generator=gen) * 3.0 - 1.5                   # a third of the latent weights beyond the STE bound
    cl = torch.channels_last
    return x.to(dev).contiguous(memory_format=cl), g.to(dev).contiguous(memory_format=cl), w.to(dev)


def grad_w64(x, g, w_shape, s, p, groups=1):
    return torch.nn.grad.conv2d_weight(x.detach().double().cpu(), tuple(w_shape), g.double().cpu(), stride=s, padding=p, groups=groups)


def ste64(gw, w):
    return torch.where(w.detach().double().cpu().abs() > ops.STE_THRESHOLD, 0.0, gw)


# ---- BinConv2d (QuantConv2dFn: masked, bias by-product) -----------------------------------------------------------------------------

def _bin_layer(shape, dev, w, groups=1):
    N, Cin, Cout, H, k, s, p = shape
    layer = BinConv2d(Cin, Cout, k, stride=s, padding=p, bias=True, groups=groups).to(dev).to(memory_format=torch.channels_last)
    layer.weight.data.copy_(w)
    return layer


@pytest.mark.parametrize("shape,rung", [(PM3, "pm"), (GEMM1, "gemm"), (STRIDED3, "strided k x k"), (STRIDED1, "strided 1 x 1"),
                                        (SWAPPED, "swapped"), (IMG3, "s2d")], ids=lambda v: v if isinstance(v, str) else None)
def test_binconv2d(dev, shape, rung):
    N, Cin, Cout, H, k, s, p = shape
    what = f"BinConv2d {shape}, {rung}"
    image = rung == "s2d"
    x0, g, w = operands(shape, dev, 11, pm1=not image)
    layer = _bin_layer(shape, dev, w)
    if image:
        layer.binary_input = False
    with lazy_train.eager():
        x = x0 if image else BinaryConnectDeterministic.apply(x0)        # (no gradient into x: the backward is grad_W and bias)
        y = layer(x)
        _, calls, lib = counted(lambda: y.backward(g))
    if rung == "swapped":
        # the swapped conv is the forward's implicit-GEMM conv on the transposed operands: no weight-gradient entry at all
        wgrad = [e for e in calls if "wgrad" in e or e == GEMM_TAPS]
        assert_route(calls, lib, ("qt_conv2d_implicit",), wgrad, what)
    else:
        assert_route(calls, lib, *RUNG[rung], what)
    by_product = rung in ("pm", "s2d")               # only these two hand the bias list to the gradient pack
    assert bool(calls.get(PM_BIAS)) == by_product, f"{what}: bias by-product {calls.get(PM_BIAS)}"
    assert_close(layer.weight.grad, ste64(grad_w64(x, g, w.shape, s, p), w), what + " grad_W")
    assert_close(layer.bias.grad, g.double().sum((0, 2, 3)), what + " bias")


def test_binconv2d_gemm_7x7_also_in_the_swapped_gate(dev):
    """7 x 7 with 128 channels: the K-major rung and the swapped conv both take it; the K-major one is first."""
    N, Cin, Cout, H, k, s, p = GEMM7
    x0, g, w = operands(GEMM7, dev, 12)
    layer = _bin_layer(GEMM7, dev, w)
    with lazy_train.eager():
        y = layer(BinaryConnectDeterministic.apply(x0))
        _, calls, lib = counted(lambda: y.backward(g))
    assert_route(calls, lib, *RUNG["gemm"], "BinConv2d 7x7")
    assert not calls.get("qt_conv2d_implicit"), calls
    assert_close(layer.weight.grad, ste64(grad_w64(x0, g, w.shape, s, p), w), "BinConv2d 7x7 grad_W")


def test_binconv2d_groups_2_counts_the_library(dev):
    """Two groups of 16 -> 16 channels: no rung takes 16 channels of a +-1 activation, each group's weight gradient is the
    library's and is counted under the one existing reason; nothing else is."""
    N, Cin, Cout, H, k, s, p = PM3
    x0, g, _ = operands(PM3, dev, 13)
    w = torch.rand((Cout, Cin // 2, k, k), generator=torch.Generator().manual_seed(14)).to(dev) * 3.0 - 1.5
    layer = _bin_layer(PM3, dev, w, groups=2)
    with lazy_train.eager():
        y = layer(BinaryConnectDeterministic.apply(x0))
        _, calls, lib = counted(lambda: y.backward(g))
    print("groups=2:", sorted(calls), lib)
    assert lib == {"conv grad_weight outside the matrix-core route": 2}
    assert not [e for e in calls if "wgrad" in e]
    assert_close(layer.weight.grad, ste64(grad_w64(x0, g, w.shape, s, p, groups=2), w), "BinConv2d groups=2 grad_W")


# ---- DorefaConv2d(bit_width=1) behind nnDorefaQuant(4): codes, un-masked, un-scaled --------------------------------------------------

@pytest.mark.parametrize("shape,rung", [(PM3, "pm"), (GEMM1, "gemm"), (STRIDED1, "strided 1 x 1")], ids=lambda v: v if isinstance(v, str) else None)
def test_dorefa_w1a4(dev, shape, rung):
    N, Cin, Cout, H, k, s, p = shape
    what = f"DorefaConv2d W1A4 {shape}, {rung}"
    _, g, w = operands(shape, dev, 21)
    gen = torch.Generator().manual_seed(22)
    x0 = (torch.randint(0, 16, (N, Cin, H, H), generator=gen).float() / 15.0).to(dev).contiguous(memory_format=torch.channels_last)
    layer = DorefaConv2d(Cin, Cout, k, stride=s, padding=p, bias=False, bit_width=1).to(dev).to(memory_format=torch.channels_last)
    layer.weight.data.copy_(w / 1.5)
    with lazy_train.eager():
        x = nnDorefaQuant(4)(x0)
        y = layer(x)
        _, calls, lib = counted(lambda: y.backward(g))
    ran, absent = RUNG[rung]
    ran = tuple(e for e in ran if e != PM_ACT) if rung == "pm" else ran
    assert_route(calls, lib, ran, absent + ("qt_digit_combine_f32",), what)
    assert_close(layer.weight.grad, grad_w64(x, g, w.shape, s, p), what + " grad_W")


# ---- Lin-quantised QuantConv2d on a level-tagged activation: three exact bf16 terms, never the fp16 planes -------------------------

@pytest.mark.parametrize("shape", [PM3, PM3_S2], ids=["pm", "stride 2: per-tap real route"])
def test_lin_levels(dev, shape):
    N, Cin, Cout, H, k, s, p = shape
    what = f"QuantConv2d lin {shape}"
    x0, g, w = operands(shape, dev, 31, pm1=False)
    conv = QuantConv2d(Cin, Cout, k, stride=s, padding=p, fsr=2, bit_width=4, dtype="lin").to(dev)
    conv.weight.data.copy_(w)
    q = log_lin_connect.nnQuant("lin", 1, 4, with_sign=False)
    with lazy_train.eager(), ops.float_split("f16x2"):
        x = q(x0)
        y = conv(x)
        _, calls, lib = counted(lambda: y.backward(g))
    if s == 1:
        assert_route(calls, lib, (PM_F32, PM_REDUCE), (PM_F16, GEMM_TAPS, PM_ACT_S2D), what)
    else:
        assert_route(calls, lib, (), [e for e in calls if e.startswith("qt_wgrad_pm")] + [GEMM_TAPS], what)
    assert_close(conv.weight.grad, grad_w64(x, g, w.shape, s, p), what + " grad_W")


# ---- XNORConv2d: un-masked route result + the XNOR-Net combination ---------------------------------------------------------------------

@pytest.mark.parametrize("quant_input", [False, True], ids=["pm1 input", "quant_input"])
def test_xnor_conv2d(dev, quant_input):
    N, Cin, Cout, H, k, s, p = PM3
    what = f"XNORConv2d {PM3}, quant_input={quant_input}"
    x0, g, w = operands(PM3, dev, 41, pm1=not quant_input)
    w = (w / 30.0).requires_grad_()
    b = torch.zeros(Cout, device=dev, requires_grad=True)
    op = xnor_connect.XNORConv2d([0, 1], quant_input, s, p, 1, 1)
    with lazy_train.eager():
        x = x0 if quant_input else BinaryConnectDeterministic.apply(x0)
        y = op.apply(x, w, b)
        _, calls, lib = counted(lambda: y.backward(g))
    assert_route(calls, lib, *RUNG["s2d" if quant_input else "pm"], what)
    assert calls.get(PM_BIAS), f"{what}: no bias by-product"
    xs = x.detach().double().cpu()
    if quant_input:           # the backward sees the quantised image sign(x) * mean(|x|, 1)
        xs = torch.sign(xs) * xs.abs().mean(1, keepdim=True)
    wd = w.detach().double().cpu()
    gw, sgn, alpha = grad_w64(xs, g, w.shape, s, p), torch.sign(wd), wd.abs().mean((0, 1), keepdim=True)
    assert_close(w.grad, alpha * gw + sgn * (gw * sgn).mean(xnor_connect.DIM, keepdim=True), what + " grad_W")
    assert_close(b.grad, g.double().sum((0, 2, 3)), what + " bias")
