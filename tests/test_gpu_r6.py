"""Round-6 GPU tests.

  * batch-256 reference digests of the remaining AlexNet conv layers of config 3 (tests/golden/make_golden_r6.py, G24): conv2
    (K = 4800, the 384 x 192 tiles), conv4, conv5 — with `c3_binconv3_b256` (round 4) every binarised conv of
    models/Alexnet/Alexnet_Bin.py:12-39 is now digest-pinned at the config's own batch."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import lazy, synth  # noqa: E402
from pytorch_quantize_impls_amd.layers import BinConv2d  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def t32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


@pytest.mark.parametrize("name", ["c3_binconv2_b256", "c3_binconv4_b256", "c3_binconv5_b256"])
@pytest.mark.parametrize("mode", ["eval_deferred", "eval_eager", "train"])
def test_alexnet_conv_layers_reproduce_the_reference_digest_at_batch_256(dev, name, mode):
    """BinConv2d at AlexNet's conv2 / conv4 / conv5 (layers/binary_layers.py:103-106), batch 256, +-1 inputs: the SHA-256 of the
    fp32 result is the reference layer's (exact integer sums) through the deferred inference graph (materialised), the
    module-by-module eval path and the training-mode forward, channels-last storage."""
    with open(os.path.join(GOLDEN_DIR, "golden_hashes_r6.json")) as fh:
        c = json.load(fh)["cases"][name]
    B, Cin, Cout, H, k = c["B"], c["Cin"], c["Cout"], c["H"], c["k"]
    conv = BinConv2d(Cin, Cout, k, stride=c["stride"], padding=c["pad"]).to(dev)
    conv.weight.data.copy_(t32(synth.uniform(c["w_seed"], (Cout, Cin, k, k), -1.0, 1.0), dev))
    conv.bias.data.copy_(t32(np.round(synth.normal(c["b_seed"], (Cout,)) * 4), dev))
    x = t32(synth.pm1(c["x_seed"], (B, Cin, H, H)), dev).contiguous(memory_format=torch.channels_last)
    conv.train(mode == "train")
    with torch.no_grad():
        if mode == "eval_deferred":
            y = conv(x)
            assert isinstance(y, lazy.LazyActivation)
            y = y.value()
        else:
            with lazy.eager():
                y = conv(x)
    a = np.ascontiguousarray(y.detach().float().contiguous().cpu().numpy(), dtype=np.float32)
    assert a.shape == (B, Cout, H, H)
    assert hashlib.sha256(a.tobytes()).hexdigest() == c["sha256_f32_nchw"], (float(a.astype(np.float64).sum()), c["sum"])


# ---- implicit hipGraphs (utils/implicit.py): the un-modified eval-mode model replays by itself after the second identical call --------

def _c4_model(dev, seed=4):
    import bench_models
    torch.manual_seed(seed)
    m = bench_models.DorefaResNet18(w_bits=1, a_bits=4)
    bench_models.randomize_bn(m, seed=3)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_var.mul_(4.0)
    return m.to(dev).to(memory_format=torch.channels_last).eval()


def test_implicit_graph_replays_the_unmodified_c4_model_after_the_second_call(dev):
    """No wrapper: model(x) under no_grad, three times — calls 1 and 2 are eager, the root then carries an instance-level forward and
    call 3 onwards are hipGraph replays with the eager logits bit for bit; weight updates, a new input shape, training mode and
    autograd all do what the eager model does."""
    from pytorch_quantize_impls_amd import utils
    with utils.implicit_graphs(True):
        m = _c4_model(dev)
        x = torch.randn(32, 3, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
        with torch.no_grad(), utils.implicit_graphs(False):
            want = m(x).clone()
        assert "forward" not in m.__dict__
        with torch.no_grad():
            y1 = m(x)
            assert "forward" not in m.__dict__
            y2 = m(x)
            assert utils.implicit_graph_stats(m)["wrapped"], utils.implicit_graph_stats(m)
            y3 = m(x)
            y4 = m(x)
        st = utils.implicit_graph_stats(m)
        assert st["replays"] >= 2 and st["value_mismatch"] == 0 and not st["capture_failures"], st
        for y in (y1, y2, y3, y4):
            assert torch.equal(y, want)
        assert y3.data_ptr() != y4.data_ptr()                                 # results are copies, not the captured buffer
        # another input, same signature: the replay follows the data
        x2 = torch.randn_like(x)
        with torch.no_grad():
            got2 = m(x2)
            with utils.implicit_graphs(False):
                want2 = m(x2)
        assert torch.equal(got2, want2) and not torch.equal(got2, want)
        # a weight update drops the graphs (version counters); the next calls are eager on the new weights, then captured again
        with torch.no_grad():
            m.blocks[0].conv1.weight.mul_(-1.0)
            before = utils.implicit_graph_stats(m)["replays"]
            got3 = m(x)
            with utils.implicit_graphs(False):
                want3 = m(x)
            assert torch.equal(got3, want3) and not torch.equal(got3, want)
            for _ in range(3):
                assert torch.equal(m(x), want3)
        assert utils.implicit_graph_stats(m)["replays"] > before
        # a new shape is a new signature; training mode / autograd are never replayed
        xs = x[:8].contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            with utils.implicit_graphs(False):
                want_s = m(xs)
            for _ in range(3):
                assert torch.equal(m(xs), want_s)
        r = utils.implicit_graph_stats(m)["replays"]
        y = m(x)                                                             # autograd on: eager, with a graph to differentiate
        assert y.requires_grad and utils.implicit_graph_stats(m)["replays"] == r
        m.train()
        with torch.no_grad():
            m(x)
        assert utils.implicit_graph_stats(m)["replays"] == r
        # module by module on request
        m.eval()
        from pytorch_quantize_impls_amd import lazy, _lib
        with torch.no_grad(), lazy.eager():
            c0 = _lib.call_counts["qt_conv2d_implicit"]
            m(x)
            assert _lib.call_counts["qt_conv2d_implicit"] > c0 and utils.implicit_graph_stats(m)["replays"] == r


def test_implicit_graph_leaves_instrumented_and_opted_out_models_alone(dev):
    import copy
    from pytorch_quantize_impls_amd import utils
    with utils.implicit_graphs(True):
        m = _c4_model(dev)
        x = torch.randn(8, 3, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
        seen = []
        h = m.blocks[3].register_forward_hook(lambda mod, i, o: seen.append(1))
        with torch.no_grad():
            for _ in range(4):
                m(x)
        assert len(seen) == 4 and "forward" not in m.__dict__              # the hook saw every call
        h.remove()
        with torch.no_grad():
            for _ in range(6):
                y = m(x)
        assert utils.implicit_graph_stats(m)["wrapped"] and utils.implicit_graph_stats(m)["replays"] >= 1
        # a deep copy carries an empty wrapper bound to the COPY: its own weights decide its result
        m2 = copy.deepcopy(m)
        with torch.no_grad():
            m2.linear.weight.mul_(2.0)
            m2.linear.bias.zero_()
            m.linear.bias.zero_()
            a, b = m(x), m2(x)
        assert torch.allclose(b, 2.0 * a)
        utils.implicit_graphs_off(m)
        assert "forward" not in m.__dict__
        with torch.no_grad():
            for _ in range(4):
                m(x)
        assert "forward" not in m.__dict__ and utils.implicit_graph_stats(m)["opted_out"]


def test_implicit_graph_keeps_a_device_bound_forward_eager(dev):
    """BinaryNet-AlexNet at batch 256 is device-bound (0.8 ms of kernels in 16 launches): the replay is timed against the eager
    forward at capture time and not kept."""
    import bench_models
    from pytorch_quantize_impls_amd import utils
    with utils.implicit_graphs(True):
        torch.manual_seed(1)
        m = bench_models.AlexNetBin()
        bench_models.randomize_bn(m)
        m = m.to(dev).to(memory_format=torch.channels_last).eval()
        x = torch.randn(256, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            ys = [m(x) for _ in range(5)]
        st = utils.implicit_graph_stats(m)
        assert st["wrapped"] and st["value_mismatch"] == 0, st
        assert all(torch.equal(ys[0], y) for y in ys)
        # either verdict is legitimate on a given box; what must hold: a kept graph was measurably faster, a dropped one costs nothing
        assert st["graphs"] + st["not_faster"] >= 1, st


# ---- round-6 launch diet of the training step: the fused kernels against the launches they replace ----------------------------------

def test_abs_mean_one_launch_is_the_mean_of_abs_and_leaves_its_ticket_zero(dev):
    """qt_abs_mean_f32 (E = mean|W| of DoReFa's 1-bit weights, functions/dorefa_connect.py:100): fp64 reference to 2^-22 relative,
    identical bits on repeated calls (order-fixed fold), any dense layout, sizes around the block boundaries; the work buffer is
    zero again after every call."""
    from pytorch_quantize_impls_amd import ops, _lib
    torch.manual_seed(0)
    for n in (1, 3, 4, 5, 255, 1024, 4097, 64 * 64 * 9, 512 * 512 * 9 + 3):
        x = torch.randn(n, device=dev) * 3.0
        c0 = _lib.call_counts["qt_abs_mean_f32"]
        a, b = ops.abs_mean(x), ops.abs_mean(x)
        assert _lib.call_counts["qt_abs_mean_f32"] == c0 + 2
        ref = x.double().abs().mean()
        assert a.dim() == 0 and torch.equal(a, b)
        assert abs(float(a) - float(ref)) <= 2.0 ** -22 * float(ref), (n, float(a), float(ref))
    w = torch.randn(64, 32, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
    assert abs(float(ops.abs_mean(w)) - float(w.double().abs().mean())) <= 1e-7
    for work in ops._ABS_MEAN_WORK.values():
        assert int(work[0]) == 0
    # a CPU tensor takes torch's expression
    xc = torch.randn(100)
    assert torch.equal(ops.abs_mean(xc), xc.abs().mean())


def test_fused_absmax_split_equals_the_three_launch_form(dev):
    """qt_f16x2_absmax_pack_f32 (partials + fold-and-split) writes the plane and the scale of qt_f16x2_absmax_scale_f32 +
    qt_f16x2_pack_f32 bit for bit, and scale3[2] = s * E for the consumer."""
    from pytorch_quantize_impls_amd import ops, _lib
    torch.manual_seed(1)
    for rows, K in ((1, 4), (7, 36), (513, 200), (4096, 576)):
        x = torch.randn(rows, K, device=dev) * (10.0 ** float(torch.randint(-6, 6, (1,))))
        E = torch.rand((), device=dev) + 0.5
        with ops.float_split("f16x2"):
            c0 = _lib.call_counts["qt_f16x2_absmax_pack_f32"]
            new = ops.split_bf16x3(x, mul_dev=E)
            assert _lib.call_counts["qt_f16x2_absmax_pack_f32"] == c0 + 1
            scale = ops.pow2_scale(x)
            old = ops._triple_pack(x, 0, None, None, 2, scale=scale)
        assert torch.equal(new.scale, old.scale) and torch.equal(new.data, old.data)
        assert torch.equal(new.scale_dev_with(E), old.scale[0:1] * E) and new.scale_dev_with(E).data_ptr() == new.scale_mul[1].data_ptr()
        assert torch.equal(new.scale_dev_with(None), old.scale[0:1])
        other = torch.ones((), device=dev) * 3
        assert torch.equal(new.scale_dev_with(other), old.scale[0:1] * 3)            # another scalar: the multiply is launched


def test_code_digits_and_their_recombination(dev):
    from pytorch_quantize_impls_amd import ops
    torch.manual_seed(2)
    x = (torch.randint(0, 3000, (4, 64, 8, 8), device=dev).float() / 15.0).contiguous(memory_format=torch.channels_last)
    hi, lo, flag = ops.code_digits(x, 15.0)
    q = torch.round(x * 15.0)
    assert hi.stride() == x.stride() and torch.equal(hi, torch.floor(q / 256.0)) and torch.equal(lo, q - hi * 256.0)
    assert int(flag) == 0
    a, b = torch.randn(64, 64, device=dev), torch.randn(64, 64, device=dev)
    inv = ops._inv_f32(15.0)
    assert torch.equal(ops.digit_combine(a, b, inv, flag), (a * 256.0 + b) * inv)
    big = torch.full((8,), 2.0 ** 16 / 15.0 * 1.01, device=dev)
    _, _, f2 = ops.code_digits(big, 15.0)
    assert int(f2) & ops.CODE_DIGIT_FLAG_BIT
    assert torch.isnan(ops.digit_combine(a, b, inv, f2)).all()


def test_linear_grad_input_operand_from_one_pack_kernel(dev):
    """grad_x = g . Q(W) of LinearBin / LinearTer: the LDS-tiled transposing pack (qt_f16x2_pack_conv_weight_f32, 1 x 1 transposed) gives
    the plane of quantise -> transpose -> pack, and the layer's gradient is unchanged bit for bit."""
    from pytorch_quantize_impls_amd import ops
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import LinearBin, LinearTer
    torch.manual_seed(3)
    for N, K in ((256, 512), (300, 260), (4096, 1024)):
        w = torch.randn(N, K, device=dev)
        for kind in ("binary", "ternary"):
            one = ops.pack_conv_weight_bf16x3(w.reshape(N, K, 1, 1), kind, terms=2, transpose_flip=True)
            ref = ops.weight_bf16x3(_fused.quantize_weight_f32(w, kind).t().contiguous(), "raw", terms=2)
            n4 = (N + 3) // 4 * 4
            assert torch.equal(one.data[:, :2 * N], ref.data[:, :2 * N]) and not one.data[:, 2 * N:].any() and one.rows == K
    for cls in (LinearBin, LinearTer):
        layer = cls(1024, 512).to(dev).train()
        x = torch.randn(64, 1024, device=dev).sign().requires_grad_(True)
        g = torch.randn(64, 512, device=dev)
        grads = []
        for flag in (True, False):
            _fused.LINEAR_GRAD_X_ONE_PACK = flag
            try:
                x.grad = None
                layer(x).backward(g)
                grads.append(x.grad.clone())
            finally:
                _fused.LINEAR_GRAD_X_ONE_PACK = True
        assert torch.equal(grads[0], grads[1])


# ---- the one-pass 3 x 3 first-layer kernel (csrc/conv_first3x3.hip: VGG-16's conv1_1) -----------------------------------------------

@pytest.mark.parametrize("N,C,H,W", [(2, 3, 32, 32), (3, 3, 45, 70), (1, 1, 7, 5), (2, 4, 64, 33), (4, 3, 224, 224)])
@pytest.mark.parametrize("cl", [True, False])
def test_first3x3_kernel_all_three_epilogues(dev, N, C, H, W, cl):
    """fp32 result within 1e-5 of the fp64 conv (normalised; two fp16 terms per tile), and the threshold bits / the nibble halo plane
    are EXACTLY the float predicate ((y_kernel + 0) * alpha < -beta on the kernel's own fp32 result) for slopes of both signs,
    zero and NaN — one accumulation serves all three; the halo of the nibble plane is zero; any image layout."""
    from pytorch_quantize_impls_amd import ops
    torch.manual_seed(N * 1000 + C * 100 + H + W)
    x = torch.randn(N, C, H, W, device=dev) * 2.5
    x[0, 0, : min(H, 6), : min(W, 6)] *= 300.0                                        # tiles with very different scales
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    wq = torch.randint(-1, 2, (64, C, 3, 3), device=dev).float()
    bias = torch.randn(64, device=dev)
    frag = ops.pack_first3x3_weight(wq)
    y = ops.conv_first3x3(x, frag, 64, bias)
    assert y is not None and tuple(y.shape) == (N * H * W, 64)
    ref = torch.nn.functional.conv2d(x.double(), wq.double(), bias.double(), 1, 1).permute(0, 2, 3, 1).reshape(N * H * W, 64)
    err = float((y.double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err
    alpha = torch.randn(64, device=dev)
    alpha[3], alpha[10], alpha[20] = 0.0, float("nan"), -0.0
    beta = torch.randn(64, device=dev) * 3
    beta[3], beta[4] = -1.0, float("inf")
    y0 = ops.conv_first3x3(x, frag, 64, None)                                         # the accumulation without the bias
    want = ((y0 + bias) * alpha < -beta)                                              # [N*H*W, 64] bool: the epilogue's float predicate
    bits = ops.conv_first3x3(x, frag, 64, bias, epi=(alpha, beta))
    got = ((bits.sign.view(N * H * W, 4)[:, :2].unsqueeze(-1) >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).bool().reshape(N * H * W, 64)
    assert torch.equal(got, want), int((got != want).sum())
    assert not bits.sign.view(N * H * W, 4)[:, 2:].any()
    nib = ops.conv_first3x3(x, frag, 64, bias, epi=ops.NibEpilogue(alpha, beta, (1, 1)))
    plane = nib.words.view(N, H + 2, W + 2, 8)
    inner = plane[:, 1:-1, 1:-1, :].reshape(N * H * W, 8)
    nibbles = ((inner.unsqueeze(-1) >> (4 * torch.arange(8, device=dev, dtype=torch.int32))) & 0xF).reshape(N * H * W, 64)
    assert torch.equal(nibbles == 0xA, want) and torch.equal(nibbles == 0x2, ~want)
    border = plane.clone()
    border[:, 1:-1, 1:-1, :] = 0
    assert not border.any()


def test_vgg_first_layer_module_and_fused_routes_share_the_first3x3_kernel(dev):
    """TerConv2d(3, 64, 3, padding=1) on a real-valued image: the module-by-module fp32 result, the deferred chain and the explicit
    fused block all run qt_conv3x3_first_f32; the chain's signs are the signs BatchNorm of the fp32 result has."""
    from pytorch_quantize_impls_amd import _lib, lazy
    from pytorch_quantize_impls_amd.functions import BinaryConnect
    from pytorch_quantize_impls_amd.layers import TerConv2d
    torch.manual_seed(9)
    conv = TerConv2d(3, 64, 3, padding=1).to(dev)
    conv.weight.data.uniform_(-1.2, 1.2)
    conv.binary_input = False
    conv2 = TerConv2d(64, 64, 3, padding=1).to(dev)
    conv2.weight.data.uniform_(-1.2, 1.2)
    bn = torch.nn.BatchNorm2d(64).to(dev)
    bn.running_mean.normal_()
    bn.running_var.uniform_(0.5, 2.0)
    bn.weight.data.normal_()
    bn.bias.data.normal_()
    seq = torch.nn.Sequential(conv, bn, torch.nn.Hardtanh(), BinaryConnect(), conv2).eval()
    x = torch.randn(3, 3, 40, 56, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        c0 = _lib.call_counts["qt_conv3x3_first_f32"]
        with lazy.eager():
            want = seq(x)
        assert _lib.call_counts["qt_conv3x3_first_f32"] == c0 + 1
        got = seq(x)
        if isinstance(got, lazy.LazyActivation):
            got = got.value()
        assert _lib.call_counts["qt_conv3x3_first_f32"] == c0 + 2
    assert torch.equal(got, want)


def _threshold_conv_case(dev, Cin, Cout, k, N, H, W, kind):
    """Operands of one fp4 conv with integer thresholds: negative / zero slopes and constant predicates among the channels."""
    from pytorch_quantize_impls_amd import ops
    pd = k // 2
    x = t32(synth.pm1(71, (N, Cin, H, W)), dev).contiguous(memory_format=torch.channels_last)
    bits = ops.sign_pack(x.permute(0, 2, 3, 1).contiguous())[0]
    px = ops.bits_to_nib_pad(bits, N, H, W, (pd, pd), ld=ops.pixel_ld_nib(Cin))
    wp = ops.pack_conv_weight_nib(t32(synth.uniform(72, (Cout, Cin, k, k), -1, 1), dev), kind)
    b = t32(synth.uniform(73, (Cout,), -4, 4), dev)
    alpha = t32(synth.uniform(74, (Cout,), -0.2, 0.2), dev)
    beta = t32(synth.uniform(75, (Cout,), -8, 8), dev)
    alpha[0] = 0.0
    alpha[1], beta[1] = 0.0, -1.0
    beta[2], beta[3] = 1e6, -1e6
    alpha[5], beta[5] = -0.0, 1.0
    thr = ops.integer_thresholds(b, alpha, beta, Cin * k * k)
    args = (px, (N, Cin, H + 2 * pd, W + 2 * pd), wp, (k, k), b, 1, 0, 1)
    return args, alpha, beta, thr


@pytest.mark.parametrize("Cin,Cout,k,N,H,W,kind", [
    # AlexNet conv2 - conv5 at batch <= 8 (M <= 4096) take the small-M tiles (ConvV128x64D, ConvVSkinny), which have no sign-bit
    # form; their batch-256 tiles (384 x 192 / 256 x 192 / 256 x 256 ping-pong) are pinned in tests/test_gpu_exact_b256.py
    (192, 576, 5, 4, 27, 27, "binary"),      # AlexNet conv2
    (576, 1152, 3, 8, 13, 13, "binary"),     # conv3
    (1152, 768, 3, 8, 13, 13, "ternary"),    # conv4
    (768, 256, 3, 3, 13, 13, "binary"),      # conv5
    (128, 128, 3, 2, 56, 56, "ternary"),     # VGG conv2_2: 256 x 128 tiles, two workgroups per CU
    (256, 256, 3, 2, 28, 28, "ternary"),     # conv3_2
    (512, 512, 3, 3, 14, 9, "binary"),       # conv4_2 / conv5 (ragged last row tile)
    (64, 64, 3, 1, 5, 7, "ternary"),         # one partial tile
])
def test_sign_bit_threshold_epilogue_equals_the_compare_form(dev, Cin, Cout, k, N, H, W, kind):
    """fp4 convs with integer thresholds: the weights-as-rows kernels (ElemFp4T: start values -(T - 1/2), bit = the accumulator's
    sign, csrc/mfma_gemm_kernel.h) against the compare form (ops.CONV_COMPARE_THRESHOLDS) and the float epilogue — bit planes and
    the next conv's nibble halo planes, bit for bit, with negative / zero slopes and constant predicates among the channels."""
    from pytorch_quantize_impls_amd import ops
    args, alpha, beta, thr = _threshold_conv_case(dev, Cin, Cout, k, N, H, W, kind)
    want_bits = ops.conv2d_nib(*args, epi=(alpha, beta))
    want_nib = ops.conv2d_nib(*args, epi=ops.NibEpilogue(alpha, beta, (1, 1)))
    assert 0.02 < float((want_bits.sign != 0).float().mean())
    with ops.scope(CONV_FLAGS=ops.CONV_COMPARE_THRESHOLDS):
        cmp_bits = ops.conv2d_nib(*args, epi=(alpha, beta, thr))
        cmp_nib = ops.conv2d_nib(*args, epi=ops.NibEpilogue(alpha, beta, (1, 1), thr=thr))
    for shape in (want_bits.sign.shape, want_nib.words.shape):          # poison what torch.empty will hand out
        junk = torch.full(tuple(shape), 0x55555555, dtype=torch.int32, device=dev)
        del junk
    got_bits = ops.conv2d_nib(*args, epi=(alpha, beta, thr))
    got_nib = ops.conv2d_nib(*args, epi=ops.NibEpilogue(alpha, beta, (1, 1), thr=thr))
    assert torch.equal(cmp_bits.sign, want_bits.sign) and torch.equal(cmp_nib.words, want_nib.words)
    assert torch.equal(got_bits.sign, want_bits.sign)
    assert torch.equal(got_nib.words, want_nib.words)


def test_unknown_conv_flag_bits_are_refused(dev, monkeypatch):
    """A bit outside the three QT_CONV_* flags: ``ops.scope`` raises, and past the scope (the module default set directly) the
    library answers QT_ERR_INVALID_ARG before anything is launched — bits and nibble-plane entries; flags 0 run."""
    from pytorch_quantize_impls_amd import _lib, ops
    args, alpha, beta, thr = _threshold_conv_case(dev, 64, 64, 3, 1, 5, 7, "ternary")
    unknown = 0x80
    assert unknown & ~ops.CONV_FLAGS_MASK and not unknown & 0xf
    with pytest.raises(ValueError):
        with ops.scope(CONV_FLAGS=unknown):
            pass
    with pytest.raises(ValueError):
        with ops.scope(CONV_FLAGS=ops.CONV_COMPARE_THRESHOLDS | unknown):
            pass
    monkeypatch.setattr(ops, "CONV_FLAGS", unknown)
    for epi in ((alpha, beta, thr), ops.NibEpilogue(alpha, beta, (1, 1), thr=thr)):
        with pytest.raises(_lib.QtStatusError) as err:
            ops.conv2d_nib(*args, epi=epi)
        assert "(qt_status -1)" in str(err.value), err.value            # QT_ERR_INVALID_ARG
    monkeypatch.setattr(ops, "CONV_FLAGS", 0)
    want = ops.conv2d_nib(*args, epi=(alpha, beta))
    assert torch.equal(ops.conv2d_nib(*args, epi=(alpha, beta, thr)).sign, want.sign)


def test_graft_entry_smoke_runs_on_the_device():
    """__graft_entry__.smoke() — the driver's round-end check — passes on this tree (it asserts the HIP entry points it expects were
    executed: a route renamed by a later round must be renamed there too)."""
    import importlib
    ge = importlib.import_module("__graft_entry__")
    ge.smoke()
