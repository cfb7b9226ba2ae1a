"""Round-5 GPU tests, part a: the ADVICE r4 items.

  * every package autograd.Function keeps the graph to a deferred training-mode BatchNorm chain (Function.apply bypasses
    __torch_function__; lazy_train.resolve_args in functions.common.QtFunction.apply), a foreign Function fails loudly;
  * the computed result of an eval-mode quantised Linear layer (DEFER_DENSE) is real memory (lazy.LazyDense);
  * ONE alpha per XNORConv2d weight: qt_xnor_weight_f32 (eval image / real-input route) and qt_xnor_tap_prep_f32 (+-1 routes)
    sum the columns in the same order (csrc/xnor_alpha.h)."""
import copy
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import lazy, lazy_train, ops  # noqa: E402
from pytorch_quantize_impls_amd.functions import BinaryConnect, binary_connect, terner_connect, xnor_connect, log_lin_connect  # noqa: E402
from pytorch_quantize_impls_amd.layers import BinConv2d, LinearBin, XNORConv2d  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _grads(consume, dev, eager, seed=5):
    torch.manual_seed(seed)
    conv = BinConv2d(16, 32, 3, padding=1).to(dev).train()
    bn = torch.nn.BatchNorm2d(32).to(dev).train()
    x = torch.randn(4, 16, 8, 8, device=dev).sign().requires_grad_(True)
    torch.manual_seed(seed + 1)
    if eager:
        with lazy_train.eager():
            y = consume(bn(conv(x)))
    else:
        h = bn(conv(x))
        assert type(h) is lazy_train.TrainChain
        y = consume(h)
    assert y.grad_fn is not None
    g = torch.arange(y.numel(), dtype=torch.float32, device=dev).reshape(y.shape) / y.numel()
    (y * g).sum().backward()
    return y.detach(), conv.weight.grad, bn.weight.grad, bn.bias.grad, x.grad


@pytest.mark.parametrize("name", ["bin_stochastic", "ter_det", "quant_xnor", "lin_quant", "binary_dense"])
def test_package_functions_keep_the_graph_to_a_deferred_training_chain(dev, name):
    w = torch.randn(6, 32 * 8 * 8, device=dev)
    consume = {
        "bin_stochastic": lambda h: binary_connect.BinaryConnectStochastic.apply(h),
        "ter_det": lambda h: terner_connect.TernaryConnectDeterministic.apply(h),
        "quant_xnor": lambda h: xnor_connect.QuantXnor(h.reshape(4, -1), 1),
        "lin_quant": lambda h: log_lin_connect.Quant(h, "lin", bit_width=4),
        "binary_dense": lambda h: binary_connect.BinaryDense.apply(h.reshape(4, -1), w, None),
    }[name]
    a = _grads(consume, dev, eager=False)
    b = _grads(consume, dev, eager=True)
    if name != "bin_stochastic":          # (rand_like follows the memory layout of its argument: different draws; the gradients
        #                                    do not depend on the draw — backward is the STE mask of the saved input)
        # the replayed BatchNorm is this backend's statistics kernel, the eager one MIOpen's: last-bit differences
        assert float((a[0] - b[0]).abs().max()) <= 1e-5 * max(1.0, float(b[0].abs().max())), name
    for u, v in zip(a[1:], b[1:]):
        assert u is not None and v is not None
        assert float((u - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), name


def test_a_foreign_function_on_a_deferred_training_chain_fails_loudly(dev):
    class Sq(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            ctx.save_for_backward(t)
            return t * t

        @staticmethod
        def backward(ctx, g):
            return 2 * ctx.saved_tensors[0] * g

    with pytest.raises(RuntimeError, match="lazy_train.resolve"):
        _grads(lambda h: Sq.apply(h), dev, eager=False)
    a = _grads(lambda h: Sq.apply(lazy_train.resolve(h)), dev, eager=False)
    b = _grads(lambda h: Sq.apply(h), dev, eager=True)
    for u, v in zip(a, b):
        assert float((u - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max()))


def test_dense_deferred_result_is_real_memory(dev):
    torch.manual_seed(0)
    lin = LinearBin(256, 64).to(dev).eval()
    bn = torch.nn.BatchNorm1d(64).to(dev).eval()
    bn.running_mean.normal_()
    x = torch.randn(32, 256, device=dev).sign()
    with torch.no_grad():
        with lazy.eager():
            want = lin(x)
            want_bits = BinaryConnect()(torch.nn.functional.hardtanh(bn(want)))
        y = lin(BinaryConnect()(x))
        assert type(y) is lazy.LazyDense and isinstance(y, lazy.LazyActivation)
        # an ordinary tensor to everything that bypasses __torch_function__
        with torch._C.DisableTorchFunctionSubclass():
            plain = y.as_subclass(torch.Tensor)
        assert plain.data_ptr() != 0 and torch.equal(plain, want)
        buf = io.BytesIO()
        torch.save(y, buf)
        buf.seek(0)
        assert torch.equal(torch.load(buf, weights_only=False).to(dev), want)
        # still records BatchNorm1d -> Hardtanh -> BinaryConnect
        got = BinaryConnect()(torch.nn.functional.hardtanh(bn(y)))
        assert torch.equal(lazy.resolve(got), want_bits)
        # chain recorded first, then an in-place op on the result: the chain reads the un-mutated value, the tensor's own
        # memory holds the mutated one
        y = lin(BinaryConnect()(x))
        rec = bn(y)
        y.mul_(2.0)
        with torch._C.DisableTorchFunctionSubclass():
            plain = y.as_subclass(torch.Tensor)
        assert torch.equal(plain, want * 2.0) and torch.equal(y + 0, want * 2.0)
        assert torch.equal(lazy.resolve(BinaryConnect()(torch.nn.functional.hardtanh(rec))), want_bits)


@pytest.mark.parametrize("shape", [(576, 192, 5, 5), (192, 3, 11, 11), (24, 8, 3, 3), (5, 3, 1, 1), (7, 5, 3, 2)])
def test_one_alpha_per_xnor_conv_weight(dev, shape):
    torch.manual_seed(sum(shape))
    w = torch.randn(shape, device=dev) * 0.05
    wq, alpha = ops.xnor_weight(w, 2)
    taps = ops.xnor_tap_prep(w)
    assert torch.equal(alpha.reshape(-1), taps.alpha)                      # the same bits on every route
    ref = w.double().abs().mean((0, 1)).reshape(-1)
    assert float((alpha.reshape(-1).double() - ref).abs().max() / ref.abs().max()) <= 1e-6
    assert torch.equal(wq, torch.sign(w) * alpha)
    # the layer: eval image and TapScales agree too
    Cout, Cin, kh, kw = shape
    layer = XNORConv2d(Cin, Cout, (kh, kw), padding=kh // 2).to(dev)
    layer.weight.data.copy_(w)
    layer.eval()
    img_alpha = layer.weight.detach().abs().amax((0, 1)).reshape(-1)
    assert torch.equal(img_alpha, taps.alpha)


# ---- eval-mode forward with autograd enabled (model.eval(); model(x) without no_grad) ---------------------------

@pytest.mark.parametrize("family", ["binary", "ternary"])
def test_eval_mode_forward_under_autograd_runs_on_the_own_kernels(dev, family):
    from pytorch_quantize_impls_amd import _lib
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import LinearTer, TerConv2d
    Lin, Conv = (LinearBin, BinConv2d) if family == "binary" else (LinearTer, TerConv2d)
    torch.manual_seed(11)
    conv = Conv(32, 64, 3, padding=1).to(dev)
    lin = Lin(64 * 6 * 6, 24).to(dev)
    if family == "ternary":
        conv.weight.data.uniform_(-1, 1)
        lin.weight.data.uniform_(-1, 1)
    conv.eval(), lin.eval()
    x = torch.randn(8, 32, 6, 6, device=dev).sign().requires_grad_(True)
    before_lib = dict(_fused.LIBRARY_PATHS)
    before = dict(_lib.call_counts)
    y = lin(conv(x).flatten(1))                                   # autograd enabled: the parameters require grad
    assert type(y) is torch.Tensor and y.grad_fn is not None
    g = torch.randn_like(y)
    y.backward(g)
    moved = {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if v != before.get(k, 0)}
    assert any(k.startswith(("qt_conv2d_implicit", "qt_nib_gemm", "qt_xnor_gemm", "qt_tern_gemm")) for k in moved), moved
    assert {k: v - before_lib.get(k, 0) for k, v in _fused.LIBRARY_PATHS.items() if v != before_lib.get(k, 0)} == {}
    # the reference expression in fp64 on the stored images
    wc, wl = conv.weight.detach().double().cpu(), lin.weight.detach().double().cpu()
    wc.requires_grad_(True), wl.requires_grad_(True)
    xr = x.detach().double().cpu().requires_grad_(True)
    yr = torch.nn.functional.linear(torch.nn.functional.conv2d(xr, wc, conv.bias.detach().double().cpu(), padding=1).flatten(1), wl,
                                    lin.bias.detach().double().cpu())
    yr.backward(g.double().cpu())
    for got, want in ((y, yr), (x.grad, xr.grad), (conv.weight.grad, wc.grad), (lin.weight.grad, wl.grad)):
        assert float((got.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max()) <= 1e-5
    # an off-grid weight (a float checkpoint loaded after .eval()) under autograd: the dense expression, counted
    lin.weight.data.normal_()
    lin.reset_quant_cache()
    before_lib = dict(_fused.LIBRARY_PATHS)
    lin(torch.randn(4, 64 * 6 * 6, device=dev).sign().requires_grad_(True))
    assert sum(_fused.LIBRARY_PATHS.values()) == sum(before_lib.values()) + 1


# ---- XNORConv2d(quant_input=True): VERDICT r4 missing #1 / row a20 (functions/xnor_connect.py:135-169) ---------------------------------

import hashlib  # noqa: E402
import json  # noqa: E402
import os  # noqa: E402

import numpy as np  # noqa: E402

from conftest import GOLDEN_DIR  # noqa: E402
from test_oracle_golden_r5 import G21, G22, g21_operands, g22_operands, sampled  # noqa: E402


@pytest.fixture(scope="module")
def g5():
    return np.load(os.path.join(GOLDEN_DIR, "golden_r5_v1.npz"), allow_pickle=False)


def _lib_delta(before):
    from pytorch_quantize_impls_amd.functions import _fused
    return {k: v - before.get(k, 0) for k, v in _fused.LIBRARY_PATHS.items() if v != before.get(k, 0)}


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_xnor_input_quantiser_vs_oracle(dev, oracle, layout):
    from pytorch_quantize_impls_amd import _lib, synth
    for seed, shape in ((1, (2, 192, 27, 27)), (2, (3, 8, 7, 5)), (3, (2, 3, 19, 19)), (4, (1, 100, 4, 4)), (5, (2, 576, 13, 13))):
        x = synth.normal(seed, shape)
        x.reshape(-1)[::53] = 0.0
        xt = torch.from_numpy(x).to(dev)
        if layout == "channels_last":
            xt = xt.contiguous(memory_format=torch.channels_last)
        before = _lib.call_counts["qt_xnor_input_quant_f32"]
        q = ops.xnor_input_quant(xt)
        assert _lib.call_counts["qt_xnor_input_quant_f32"] == before + 1
        assert q.shape == xt.shape and q.is_contiguous(memory_format=torch.channels_last)
        want = oracle.xnor_input_quant(x)
        got = q.cpu().numpy()
        assert np.array_equal(got == 0, want == 0) and np.array_equal(np.sign(got), np.sign(want))
        assert float(np.abs(got - want).max()) <= 2e-6 * float(np.abs(want).max())        # summation order of the per-pixel mean (fp32, up to 576 terms)
    # exactly representable means: bit-exact
    sg = synth.pm1(9, (2, 64, 5, 5))
    a = np.exp2(np.floor(synth.uniform(10, (2, 1, 5, 5), -3, 3))).astype(np.float32)
    xt = torch.from_numpy(sg * a).to(dev)
    assert np.array_equal(ops.xnor_input_quant(xt).cpu().numpy(), oracle.xnor_input_quant(sg * a))


@pytest.mark.parametrize("name", G22)
def test_xnor_conv_quant_input_reference_digest(dev, name):
    """G22: power-of-two per-pixel magnitudes and per-tap weights — every sum exact in any order: the reference's SHA-256."""
    from pytorch_quantize_impls_amd import _lib
    from pytorch_quantize_impls_amd.functions import _fused
    with open(os.path.join(GOLDEN_DIR, "golden_hashes_r5.json")) as fh:
        c = json.load(fh)["cases"][name]
    x, w = g22_operands(c)
    op = xnor_connect.XNORConv2d([0, 1], True, c["stride"], c["pad"], 1, 1)
    before, calls = dict(_fused.LIBRARY_PATHS), dict(_lib.call_counts)
    for fmt in (torch.contiguous_format, torch.channels_last):
        with torch.no_grad():
            y = op.apply(torch.from_numpy(x).to(dev).contiguous(memory_format=fmt), torch.from_numpy(w).to(dev))
        got = np.ascontiguousarray(y.cpu().numpy(), dtype=np.float32)
        assert hashlib.sha256(got.tobytes()).hexdigest() == c["sha256_f32"], fmt
    assert _lib_delta(before) == {}
    assert _lib.call_counts["qt_conv2d_implicit_taps_rows"] == calls.get("qt_conv2d_implicit_taps_rows", 0) + 2     # the fp4-rate route
    assert _lib.call_counts["qt_xnor_input_quant_f32"] == calls.get("qt_xnor_input_quant_f32", 0) + 2


@pytest.mark.parametrize("name", G21)
def test_xnor_conv_quant_input_vs_reference_fp64(dev, g5, name):
    """G21: forward and all gradients of the reference function in fp64, <= 1e-5 normalised."""
    from pytorch_quantize_impls_amd.functions import _fused
    x, w, b, go, s, p = g21_operands(g5, name)
    op = xnor_connect.XNORConv2d([0, 1], True, s, p, 1, 1)
    xt = torch.from_numpy(x).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    wt = torch.from_numpy(w).to(dev).requires_grad_(True)
    bt = torch.from_numpy(b).to(dev).requires_grad_(True) if b is not None else None
    before = dict(_fused.LIBRARY_PATHS)
    old = _fused.BWD_MFMA_MIN_MACS
    _fused.BWD_MFMA_MIN_MACS = 0
    try:
        y = op.apply(xt, wt, bt) if bt is not None else op.apply(xt, wt)
        y.backward(torch.from_numpy(go).to(dev))
    finally:
        _fused.BWD_MFMA_MIN_MACS = old
    assert sampled(g5, name, "y", y.detach().cpu().numpy()) <= 1e-5
    assert sampled(g5, name, "gx", xt.grad.cpu().numpy()) <= 1e-5
    assert sampled(g5, name, "gw", wt.grad.cpu().numpy()) <= 1e-5
    if bt is not None:
        assert sampled(g5, name, "gb", bt.grad.cpu().numpy()) <= 1e-5
    lib = _lib_delta(before)
    if name != "c3_first_layer":          # Cin % 8 == 0: every contraction on the own kernels (the 3-channel case: grad_input of a first layer on the library, counted)
        assert lib == {}, lib


def test_xnor_conv_quant_input_vs_oracle_seeded(dev, oracle):
    from pytorch_quantize_impls_amd import synth
    for seed, (B, Cin, Cout, H, k, s, p) in enumerate(((3, 64, 40, 12, 3, 1, 1), (2, 32, 48, 9, 5, 1, 2), (2, 16, 24, 11, 3, 2, 0),
                                                       (1, 8, 8, 5, 1, 1, 0), (2, 3, 32, 19, 5, 2, 2), (2, 20, 130, 10, 3, 1, 2),
                                                       (5, 96, 200, 7, 3, 1, 1), (1, 7, 9, 6, 6, 1, 3))):
        x = synth.normal(900 + seed, (B, Cin, H, H))
        x.reshape(-1)[::41] = 0.0
        x[:, :, 1::4, 2::3] = 0.0                      # whole pixels of zeros: their scale is 0 (the row factor inherits)
        x[0, :, :2, :] = 0.0                           # ... and whole windows of them
        w = synth.normal(950 + seed, (Cout, Cin, k, k), 0.1)
        b = synth.normal(980 + seed, (Cout,))
        for dil in ((1, 2) if seed in (0, 5) else (1,)):
            want = oracle.xnor_conv2d_forward(x, w, b, s, p, dil, quant_input=True)
            op = xnor_connect.XNORConv2d([0, 1], True, s, p, dil, 1)
            with torch.no_grad():
                got = op.apply(torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)).cpu().numpy()
            assert got.shape == want.shape
            assert float(np.abs(got - want).max() / np.abs(want).max()) <= 1e-5, (B, Cin, Cout, H, k, s, p, dil)


# ---- DoReFa layers at 8 < bit_width < 32 (VERDICT r4 missing #3; G23) ------------------------------------------------------------------

from test_oracle_golden_r5 import G23  # noqa: E402


@pytest.mark.parametrize("mode", ["train", "eval", "eval_autograd"])
@pytest.mark.parametrize("name", G23)
def test_dorefa_9_to_16_bit_layers_vs_reference_fp64_vectors(dev, name, mode):
    """Forward (+ all gradients in training mode) of LinearDorefa / DorefaConv2d at bit_width 9 / 12 / 16 against the reference's own
    layers in double precision: <= 1e-5 normalised (2e-5 for the weight gradient through tanh / max|tanh|); no dense-library call."""
    from conftest import norm_err
    from pytorch_quantize_impls_amd.functions import _fused, nnDorefaQuant
    from pytorch_quantize_impls_amd.layers import DorefaConv2d, LinearDorefa
    g20 = np.load(os.path.join(GOLDEN_DIR, "golden_r5b_v1.npz"), allow_pickle=False)
    g = {k: g20[f"g23_{name}_{k}"] for k in ("x", "w", "b", "go", "y", "gx", "gw", "gb", "geom")}
    geom = [int(v) for v in g["geom"]]
    bits, coded = geom[-2], bool(geom[-1])
    if name.startswith("conv"):
        B, Cin, Cout, H, k, s, p = geom[:7]
        layer = DorefaConv2d(Cin, Cout, k, stride=s, padding=p, bias=True, bit_width=bits)
    else:
        B, K, N = geom[:3]
        layer = LinearDorefa(K, N, bias=True, bit_width=bits)
    layer = layer.to(dev).train()
    layer.weight.data.copy_(torch.from_numpy(g["w"]))
    layer.bias.data.copy_(torch.from_numpy(g["b"]))
    raw = torch.from_numpy(g["x"]).to(dev)
    if raw.dim() == 4:
        raw = raw.contiguous(memory_format=torch.channels_last)
    old = _fused.BWD_MFMA_MIN_MACS
    _fused.BWD_MFMA_MIN_MACS = 0
    lib_before = dict(_fused.LIBRARY_PATHS)
    try:
        if mode == "train":
            raw.requires_grad_(True)
            x = nnDorefaQuant(4)(raw) if coded else raw * 1.0
            x.retain_grad()
            y = layer(x)
            y.backward(torch.from_numpy(g["go"]).to(dev))
            assert norm_err(y.detach().cpu().numpy(), g["y"]) <= 1e-5
            assert norm_err(x.grad.cpu().numpy(), g["gx"]) <= 1e-5
            assert norm_err(layer.weight.grad.cpu().numpy(), g["gw"]) <= 2e-5
            assert norm_err(layer.bias.grad.cpu().numpy(), g["gb"]) <= 1e-5
        else:
            layer.eval()                                     # the weight now holds the quantised image
            x = raw.requires_grad_(True) if mode == "eval_autograd" else raw
            if mode == "eval":
                with torch.no_grad():
                    y = layer(x)
            else:
                y = layer(x)
                y.backward(torch.from_numpy(g["go"]).to(dev))
                assert norm_err(x.grad.cpu().numpy(), g["gx"]) <= 1e-5      # d/dx is the same expression in both modes
            assert norm_err(torch.as_tensor(y).detach().cpu().numpy(), g["y"]) <= 1e-5
    finally:
        _fused.BWD_MFMA_MIN_MACS = old
    assert _lib_delta(lib_before) == {}


# ---- the persistent direct 3 x 3 code conv (csrc/code_conv3x3.hip) == the implicit-GEMM route, bit for bit ---------------------------

def test_direct_code_conv3x3_equals_the_implicit_gemm_route(dev):
    """The fused DoReFa ResNet-18 forward (stage-1 / stage-2 stride-1 convs on the persistent direct kernel) gives the same logits,
    bit for bit, as with the kernel switched off (ops.CONV_NO_DIRECT_CODES: every conv on the implicit-GEMM kernel) and as the
    module-by-module graph; batches 8 / 24 / 256 (whole 128-pixel tiles, ragged tile counts per workgroup).  Both sides run in
    this process: the flag is an argument of every launch, each scope holds the forward and the read-back of its result, and
    implicit hipGraphs are off, since a replay would keep the flags of its capture."""
    import bench_models
    from pytorch_quantize_impls_amd import _lib, utils
    count = _lib.load().qt_code_conv3x3_launch_count
    torch.manual_seed(4)
    m4 = bench_models.DorefaResNet18(w_bits=1, a_bits=4)
    bench_models.randomize_bn(m4, seed=3)
    for m in m4.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.mul_(4.0)
    m4 = m4.to(dev).to(memory_format=torch.channels_last).eval()
    f4 = bench_models.FusedDorefaResNet18(m4, fold="device")
    res, direct = {}, {}
    with utils.implicit_graphs(False):
        for off in (False, True):
            out, c0 = [], int(count())
            with ops.scope(CONV_FLAGS=ops.CONV_NO_DIRECT_CODES if off else 0):
                for B in (8, 24, 256):
                    x = torch.randn((B, 3, 32, 32), device=dev,
                                    generator=torch.Generator(device=dev).manual_seed(B)).contiguous(memory_format=torch.channels_last)
                    with torch.no_grad():
                        y = f4(x)
                        with lazy.eager():
                            ye = m4(x)
                        out.append(hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest() + ":" + str(bool(torch.equal(y, ye))))
            res[off], direct[off] = out, int(count()) - c0
    assert res[False] == res[True], res
    assert all(r.endswith(":True") for r in res[False]), res
    assert direct[False] > 0 and direct[True] == 0, direct          # the two sides did take different routes


# ---- thread-local switches: float_split / lazy_train.eager do not leak between threads; backward keeps the forward's mode

def test_float_split_is_thread_local_and_follows_the_graph_into_backward(dev):
    import threading
    from pytorch_quantize_impls_amd import _lib
    torch.manual_seed(0)
    x = torch.randn(64, 200, device=dev)
    w = torch.randn(48, 200, device=dev)
    with ops.float_split("bf16x3"):
        ref3 = ops.float_linear(x, w, "binary")
    ref2 = ops.float_linear(x, w, "binary")
    assert ops.current_float_split() == "f16x2"
    want = torch.nn.functional.linear(x.double(), torch.where(w < 0, -1.0, 1.0).double()).float()
    assert float((ref3 - want).abs().max() / want.abs().max()) <= 1e-6      # exact products, fp32 accumulation
    assert float((ref2 - want).abs().max() / want.abs().max()) <= 1e-5
    errs = []

    def worker(mode, ref, n=200):
        try:
            for _ in range(n):
                if mode is None:
                    assert ops.current_float_split() == "f16x2"
                    y = ops.float_linear(x, w, "binary")
                else:
                    with ops.float_split(mode):
                        assert ops.current_float_split() == mode
                        y = ops.float_linear(x, w, "binary")
                if not torch.equal(y, ref):
                    errs.append(mode)
                    return
        except Exception as exc:  # noqa: BLE001
            errs.append(repr(exc))
    ts = [threading.Thread(target=worker, args=("bf16x3", ref3)), threading.Thread(target=worker, args=(None, ref2)),
          threading.Thread(target=worker, args=("bf16x3", ref3)), threading.Thread(target=worker, args=(None, ref2))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    # backward runs on the autograd engine's thread: it re-opens the mode the forward was recorded under
    lin = LinearBin(200, 48).to(dev).train()
    xin = (x * 3.0).requires_grad_(True)                  # real-valued input: the float routes
    with ops.float_split("bf16x3"):
        y = lin(xin)
    before = dict(_lib.call_counts)
    y.sum().backward()                                    # outside the scope
    moved = {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if v != before.get(k, 0)}
    assert not any(k.startswith("qt_f16x2") for k in moved), moved
    assert any(k.startswith(("qt_bf16x3", "qt_bf16x6", "qt_bf16_gemm")) for k in moved), moved
    # and lazy_train.eager() of one thread does not switch another thread's recording off
    flags = {}

    def probe():
        flags["other"] = lazy_train.enabled()
    with lazy_train.eager():
        t = threading.Thread(target=probe)
        t.start()
        t.join()
        flags["mine"] = lazy_train.enabled()
    assert flags == {"other": True, "mine": False}


def test_direct_code_conv3x3_geometry_fuzz(dev):
    """Seeded geometries of FusedBnDorefaQuant -> FusedDorefaConvBnQuant (fold="device"): channels 64 / 128, Cout 64 / 128 / 192,
    power-of-two maps 4 .. 64 (tiles inside an image, whole images per tile, ragged tile counts per workgroup), halos 0 / 1 on
    the output, with / without a code residual and ReLU, bit widths 2 .. 4: the code planes of the persistent direct kernel equal
    those of the implicit-GEMM kernel byte for byte (ops.CONV_NO_DIRECT_CODES, an argument of the launch)."""
    from pytorch_quantize_impls_amd.layers import DorefaConv2d, FusedBnDorefaQuant, FusedDorefaConvBnQuant
    from pytorch_quantize_impls_amd import _lib
    count = _lib.load().qt_code_conv3x3_launch_count
    rng = np.random.default_rng(20260930)
    done = 0
    for it in range(24):
        Cin = int(rng.choice([64, 128])); Cout = int(rng.choice([64, 128, 192]))
        H = int(rng.choice([4, 8, 16, 32])); W = int(rng.choice([4, 8, 16, 32, 64])); N = int(rng.choice([1, 2, 3, 8, 16, 33]))
        if (N * H * W) % 128:
            N = int(np.ceil(N * H * W / 128) * 128 // (H * W)) or 1
            if (N * H * W) % 128:
                continue
        bits = int(rng.choice([2, 3, 4])); relu = bool(rng.integers(0, 2)); use_res = bool(rng.integers(0, 2)) and Cin == Cout
        oh = int(rng.integers(0, 2))
        torch.manual_seed(1000 + it)
        bn0 = torch.nn.BatchNorm2d(Cin).to(dev).eval()
        bn0.running_mean.normal_(); bn0.running_var.uniform_(0.5, 2.0); bn0.weight.data.normal_(); bn0.bias.data.normal_()
        conv = DorefaConv2d(Cin, Cout, 3, padding=1, bias=False, bit_width=1).to(dev)
        conv.weight.data.normal_(0, 0.05)
        conv.eval()
        bn = torch.nn.BatchNorm2d(Cout).to(dev).eval()
        bn.running_mean.normal_(0, 0.5); bn.running_var.uniform_(0.5, 2.0); bn.weight.data.normal_(); bn.bias.data.normal_(0, 0.3)
        x = torch.rand(N, Cin, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        head = FusedBnDorefaQuant(bn0, bits, relu=True, out_halo=1, fold="device")
        blk = FusedDorefaConvBnQuant(conv, bn, bits, relu=relu, out_halo=oh, fold="device")
        outs = []
        with torch.no_grad():
            for off in (False, True):
                with ops.scope(CONV_FLAGS=ops.CONV_NO_DIRECT_CODES if off else 0):
                    act = head(x)
                    c0 = int(count())
                    y = blk(act, residual=act if use_res else None)
                    assert int(count()) - c0 == (0 if off else 1), "route"
                    outs.append((y.without_halo().codes.codes.clone(), y.codes.codes.clone(), int(y.codes.overflow.item())))
        assert torch.equal(outs[0][0], outs[1][0]), (Cin, Cout, H, W, N, bits, relu, use_res, oh)
        assert torch.equal(outs[0][1], outs[1][1]), "halo border differs"
        assert outs[0][2] == outs[1][2]
        done += 1
    assert done >= 16


def test_conv_flags_are_thread_local(dev):
    """ops.CONV_FLAGS set by ``ops.scope`` holds for the calling thread only: while the main thread keeps its 64 -> 64 block (8 x 8
    map, batch 2: one whole 128-pixel tile) off the direct kernel, a worker thread's call of the same block takes it, with the same
    codes byte for byte; after the scope the main thread takes it again."""
    import threading
    from pytorch_quantize_impls_amd.layers import DorefaConv2d, FusedBnDorefaQuant, FusedDorefaConvBnQuant
    from pytorch_quantize_impls_amd import _lib
    count = _lib.load().qt_code_conv3x3_launch_count
    torch.manual_seed(77)
    bn0 = torch.nn.BatchNorm2d(64).to(dev).eval()
    bn0.running_mean.normal_(); bn0.running_var.uniform_(0.5, 2.0); bn0.weight.data.normal_(); bn0.bias.data.normal_()
    conv = DorefaConv2d(64, 64, 3, padding=1, bias=False, bit_width=1).to(dev)
    conv.weight.data.normal_(0, 0.05)
    conv.eval()
    bn = torch.nn.BatchNorm2d(64).to(dev).eval()
    bn.running_mean.normal_(0, 0.5); bn.running_var.uniform_(0.5, 2.0); bn.weight.data.normal_(); bn.bias.data.normal_(0, 0.3)
    x = torch.rand(2, 64, 8, 8, device=dev).contiguous(memory_format=torch.channels_last)
    head = FusedBnDorefaQuant(bn0, 4, relu=True, out_halo=1, fold="device")
    blk = FusedDorefaConvBnQuant(conv, bn, 4, relu=True, out_halo=1, fold="device")

    def run():
        with torch.no_grad():
            act = head(x)
            c0 = int(count())
            y = blk(act)
            codes = y.codes.codes.clone()
            torch.cuda.synchronize()
            return int(count()) - c0, codes

    worker = {}

    def work():
        try:
            worker["flags"] = ops._cfg("CONV_FLAGS")
            worker["moved"], worker["codes"] = run()
        except Exception as exc:  # noqa: BLE001
            worker["error"] = repr(exc)

    with ops.scope(CONV_FLAGS=ops.CONV_NO_DIRECT_CODES):
        moved, codes = run()
        assert moved == 0
        t = threading.Thread(target=work)
        t.start()
        t.join()
        assert ops._cfg("CONV_FLAGS") == ops.CONV_NO_DIRECT_CODES
    assert "error" not in worker, worker
    assert worker["flags"] == 0 and worker["moved"] == 1
    assert torch.equal(worker["codes"], codes)
    moved, after = run()
    assert moved == 1 and torch.equal(after, codes)


@pytest.mark.parametrize("bits", [1, 3, 8])
def test_dorefa_eval_mode_forward_under_autograd(dev, bits):
    """DoReFa layers in eval mode with autograd on (parameters require grad): F.linear / F.conv2d on the stored image is the reference
    expression (layers/dorefa_layers.py:45,81); forward + input / weight gradients vs fp64, no dense-library call."""
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import DorefaConv2d, LinearDorefa
    torch.manual_seed(20 + bits)
    conv = DorefaConv2d(16, 24, 3, padding=1, bit_width=bits).to(dev)
    lin = LinearDorefa(24 * 5 * 5, 10, bit_width=bits).to(dev)
    conv.eval(), lin.eval()
    x = torch.rand(6, 16, 5, 5, device=dev).requires_grad_(True)
    old = _fused.BWD_MFMA_MIN_MACS
    _fused.BWD_MFMA_MIN_MACS = 0
    before = dict(_fused.LIBRARY_PATHS)
    try:
        y = lin(conv(x).flatten(1))
        g = torch.randn_like(y)
        y.backward(g)
    finally:
        _fused.BWD_MFMA_MIN_MACS = old
    assert _lib_delta(before) == {}
    wc, wl = conv.weight.detach().double().cpu().requires_grad_(True), lin.weight.detach().double().cpu().requires_grad_(True)
    xr = x.detach().double().cpu().requires_grad_(True)
    yr = torch.nn.functional.linear(torch.nn.functional.conv2d(xr, wc, conv.bias.detach().double().cpu(), padding=1).flatten(1), wl,
                                    lin.bias.detach().double().cpu())
    yr.backward(g.double().cpu())
    for got, want in ((y, yr), (x.grad, xr.grad), (conv.weight.grad, wc.grad), (lin.weight.grad, wl.grad)):
        assert float((got.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max()) <= 1e-5
