"""Training gradients at the benchmark's batch (256), layer by layer, against the float64 references of tests/_grad_exact.py.

Each layer is built as the benchmark models build it (channels_last, train mode) and fed an input that carries the tag its
quantiser leaves in the step (BinaryConnect's +-1 planes, nnDorefaQuant's codes), so the dispatcher takes the step's route.
Every backward runs under torch.profiler: the case asserts the C-ABI entries of its route ran, that no dense-library path was
taken (_fused.LIBRARY_PATHS), and records the kernel instances it compared.

  (a) designed gradients, bit for bit: every contraction is exact in fp32 (``proves_exact`` checks it for the actual tensors
      first); grad_x, grad_W (masked / scaled as the route does, batch chunks from the route's own plan) and the bias gradient
      must equal the reference exactly, under both float splits, with one exponent per tensor (2^-40 or 2^30: the per-tensor
      scale of grad_x) and one per output channel over 2^-20 .. 2^20 (the per-channel scales of the two-plane weight gradient).
      BinaryNet-AlexNet conv1 (real image, space-to-depth), conv2 (5x5), conv3 - conv5 (3x3), LinearBin 9216 -> 4096,
      4096 -> 4096, 4096 -> 10; DoReFa ResNet-18 W1A4 3x3 at 64 / 128 / 512 channels, 3x3 stride 2, the 1x1 stride-2
      shortcuts, a W4 layer;
  (b) edges: ragged batch chunks on the pixel-major, K-major and space-to-depth routes, channels off the tile grid, odd K, a
      gradient that is not channels-last, the forwards that carry an output scale under the exact split;
  (c) Gaussian data spanning six decades per channel (non-zero lo / mid planes) against float64 with stated bars;
  (e) one batch-256 training step of each benchmark model: every backward kernel instance it launches was compared here, is
      torch's own (allow-list with reasons) or is named in KNOWN_UNCOVERED with where it is checked instead.

Not here: the training chains at batch 256 (d: tests/test_gpu_train_chain_b256.py), the plane past 2^31 bytes, the DoReFa
digit route, the channels-last parameter (layout_like) and AlexNet conv4 (conv3 and conv5 share its kernels).  The Lin / Log layers at batch 256
(level chain and gradients) are in tests/test_gpu_loglin_b256.py, XNOR-Net at batch 256 (tap convs, grad_x) in
tests/test_gpu_xnor_b256.py.
Run the whole module: the coverage test reads what the cases before it recorded; it prints the module's peak device memory
(59 cases; 12.2 GiB and 21 s measured on an MI355X)."""
import re

import pytest
import torch

import _grad_exact as G

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib, lazy_train, ops  # noqa: E402
from pytorch_quantize_impls_amd.functions import BinaryConnectDeterministic, nnDorefaQuant  # noqa: E402
from pytorch_quantize_impls_amd.functions import _fused  # noqa: E402
from pytorch_quantize_impls_amd.layers import BinConv2d, DorefaConv2d, LinearBin  # noqa: E402

BATCH = 256
SPLITS = ("f16x2", "bf16x3")
PEAK = {}                   # test id -> peak device memory (bytes); reported by the coverage test
COVERED = {}                # kernel instance -> cases that compared its output here


def kernel_label(name: str) -> str:
    """Profiler kernel name -> 'wgrad_pm_kernel<64, 32, 5, 5, 2>': no namespace, no return type, no parameter list."""
    k = name.replace("(anonymous namespace)::", "")
    k = k[5:] if k.startswith("void ") else k
    depth = 0
    for i, ch in enumerate(k):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and i > 0:
            return k[:i]
    return k


def profiled(fn):
    """(fn(), kernel labels it launched, C-ABI call-count deltas, dense-library path deltas)."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    calls, lib = dict(_lib.call_counts), dict(_fused.LIBRARY_PATHS)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    kernels = {kernel_label(e.key) for e in prof.key_averages() if e.device_type == DeviceType.CUDA}
    dcalls = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
    dlib = {k: v - lib.get(k, 0) for k, v in _fused.LIBRARY_PATHS.items() if v != lib.get(k, 0)}
    return out, kernels, dcalls, dlib


def backward_traced(y, g, case, expect=(), absent=()):
    """y.backward(g) under the profiler: the C-ABI entries ``expect`` ran, ``absent`` did not, no dense-library path; the
    kernels are recorded as compared by ``case`` (call this only where the case then compares every output it produced)."""
    _, kernels, calls, lib = profiled(lambda: y.backward(g, retain_graph=True))
    assert not lib, f"{case}: dense-library paths taken: {lib}"
    missing = [e for e in expect if not calls.get(e)]
    assert not missing, f"{case}: route entries {missing} did not run; ran {sorted(calls)}"
    extra = [e for e in absent if calls.get(e)]
    assert not extra, f"{case}: entries {extra} ran"
    for k in kernels:
        COVERED.setdefault(k, []).append(case)
    return kernels


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    PEAK[request.node.name] = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()


def _check(got, want, what, names=("co", "ci", "ky", "kx")):
    rep = G.mismatch_report(got, want, names, what=what)
    assert not rep, rep


def _prove(a, b, contract, split, what, per_channel=False, out_dim=0, split_b=None, a_dim=1,
           b_exact_in=(torch.float16, torch.bfloat16)):
    ok, why = G.proves_exact(a, b, contract, split, a_channel_dim=a_dim if per_channel else None, split_b=split_b,
                             out_channel_dim=out_dim if per_channel else None, b_exact_in=b_exact_in)
    assert ok, f"{what}: the designed operands are not exact ({why})"


def _designs(Cout, exp, seed):
    """(name, exponent kwargs): one exponent per tensor, then one per output channel."""
    return (("per-tensor", dict(exp=exp)), ("per-channel", dict(ch_exps=G.spread_exps(Cout, -20, 20, seed))))


def _split_batch(N, nc):
    return [min(nc, N - n0) for n0 in range(0, N, nc)]


def _pm_chunks(N, Cout, Cin, H, W, k, p):
    """Image counts of the pixel-major route's batch chunks: the route's own search (ops.wgrad_chunk_images) over its plan."""
    Ho = H + 2 * p - k + 1
    return _split_batch(N, ops.wgrad_chunk_images(
        N, lambda n: ops.wgrad_pm_plan(n, Cout, Cin, H, W, Ho, k, k, p, p, ops.WGRAD_PM_WORKGROUPS)[0]))


def _gemm_chunks(N, Cout, Cin, H, W, k, p):
    """The same for the K-major route (ops.wgrad_gemm_plan)."""
    return _split_batch(N, ops.wgrad_chunk_images(N, lambda n: ops.wgrad_gemm_plan(n, Cout, Cin, H, W, k, k, p, p)[0]))


# ---- BinaryNet: BinConv2d / LinearBin with BinaryConnect-tagged +-1 input ---------------------------------------------------------

def _bin_conv_case(dev, Cin, Cout, H, k, s, p, split, seed, amp, exp, real_image=False, bias=True, cl_grad=True, N=BATCH):
    layer = BinConv2d(Cin, Cout, k, stride=s, padding=p, bias=bias).to(dev).to(memory_format=torch.channels_last)
    layer.weight.data.copy_(G.latent_weight(layer.weight.shape, seed, dev))
    if real_image:
        layer.binary_input = False
        x = G.int_uniform((N, Cin, H, H), -4, 4, seed + 1, dev)
    else:
        x0 = (G.pm1((N, Cin, H, H), seed + 1, dev) * 0.5).requires_grad_()
    Ho = (H + 2 * p - k) // s + 1
    wq = G.safe_sign(layer.weight)
    with lazy_train.eager(), ops.float_split(split):
        if not real_image:
            x = BinaryConnectDeterministic.apply(x0)
            x.retain_grad()
        y = layer(x)
        for name, ek in _designs(Cout, exp, seed):
            g = G.grad_ints((N, Cout, Ho, Ho), amp, seed + 2, dev, channels_last=cl_grad, **ek)
            per = name == "per-channel"
            what = f"BinConv2d {Cin}->{Cout} k{k}/s{s} at {H}, {split}, {name}"
            layer.weight.grad = None
            if bias:
                layer.bias.grad = None
            if not real_image:
                x.grad = None
            two = split == "f16x2"
            expect = ["qt_wgrad_pm_f16" if two else "qt_wgrad_pm_f32", "qt_wgrad_pm_reduce_f32"]
            if real_image:
                expect.append("qt_wgrad_pm_pack_act_s2d_f16x2" if two else "qt_wgrad_pm_pack_act_s2d_f32")
            else:
                expect.append("qt_conv2d_implicit")
            absent = []
            if bias:
                (expect if cl_grad else absent).append("qt_wgrad_pm_bias_reduce_f32")
            backward_traced(y, g, what, expect, absent)
            xv = x.detach()
            _prove(g, xv, lambda a, b: G.conv_grad_weight64(b, a, k, s, p), split, what + " grad_W", per_channel=per,
                   split_b=split if real_image else None)
            if real_image:      # the space-to-depth image of the stride-s conv on the pixel-major kernel
                k2, Cs8 = -(-k // s), -(-Cin * s * s // 8) * 8
                chunks = _pm_chunks(N, Cout, (2 if two else 3) * Cs8, Ho + k2 - 1, Ho + k2 - 1, k2, 0)
            else:
                chunks = _pm_chunks(N, Cout, Cin, H, H, k, p)
            dW = G.ste_mask(G.chunked_sum(G.conv_grad_weight64(xv, g, k, s, p, chunks=chunks)), layer.weight)
            _check(layer.weight.grad, dW, what + " grad_W")
            if bias:
                _check(layer.bias.grad, G.to_f32_exact(G.bias_grad64(g)), what + " bias", ("c",))
            if not real_image and not per:
                _prove(g, wq, lambda a, b: G.conv_grad_input64(a, b, (H, H), s, p), split, what + " grad_x")
                _check(x.grad, G.to_f32_exact(G.conv_grad_input64(g, wq, (H, H), s, p)), what + " grad_x",
                       ("n", "c", "y", "x"))


@pytest.mark.parametrize("split", SPLITS)
def test_alexnet_bin_conv1_real_image_s2d_weight_gradient_and_bias(dev, split):
    _bin_conv_case(dev, 3, 192, 224, 11, 4, 2, split, 11, 2, -40, real_image=True)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("Cin,Cout,H,k,p,exp", [
    (192, 576, 27, 5, 2, -40),      # conv2: pixel-major <64,32,5,5>, bias by-product
    (576, 1152, 13, 3, 1, 30),      # conv3: Cout % 128 == 0, the full kernel
    (768, 256, 13, 3, 1, -40),      # conv5
])
def test_alexnet_bin_convs_at_batch_256(dev, split, Cin, Cout, H, k, p, exp):
    _bin_conv_case(dev, Cin, Cout, H, k, 1, p, split, Cin + Cout, 8, exp)


def _bin_linear_case(dev, K, Nf, split, seed, exp, N=BATCH):
    layer = LinearBin(K, Nf).to(dev)
    layer.weight.data.copy_(G.latent_weight(layer.weight.shape, seed, dev))
    x0 = (G.pm1((N, K), seed + 1, dev) * 0.5).requires_grad_()
    wq = G.safe_sign(layer.weight)
    with lazy_train.eager(), ops.float_split(split):
        x = BinaryConnectDeterministic.apply(x0)
        x.retain_grad()
        y = layer(x)
        for name, ek in _designs(Nf, exp, seed):
            g = G.grad_ints((N, Nf), 8, seed + 2, dev, **ek)
            per = name == "per-channel"
            what = f"LinearBin {K}->{Nf}, {split}, {name}"
            layer.weight.grad = layer.bias.grad = x.grad = None
            one_pack = split == "f16x2" and Nf % 4 == 0          # _fused.LINEAR_GRAD_X_ONE_PACK; else pm1_matmul
            backward_traced(y, g, what, ["qt_f16x2_pack_conv_weight_f32"] if one_pack else [],
                            [] if one_pack else ["qt_f16x2_pack_conv_weight_f32"])
            # grad_W: rows of g^T are output features, three exact bf16 terms
            _prove(g.t(), x.detach(), lambda a, b: a @ b, "bf16x3", what + " grad_W", per_channel=per, a_dim=0)
            _check(layer.weight.grad, G.ste_mask(G.to_f32_exact(G.linear_grad_w64(g, x.detach())), layer.weight), what + " grad_W",
                   ("o", "i"))
            _check(layer.bias.grad, G.to_f32_exact(G.bias_grad64(g)), what + " bias", ("o",))
            if not per:
                _prove(g, wq, lambda a, b: a @ b, split, what + " grad_x")
                _check(x.grad, G.to_f32_exact(G.linear_grad_x64(g, wq)), what + " grad_x", ("n", "i"))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("K,Nf,exp", [(9216, 4096, -40), (4096, 4096, 30), (4096, 10, -40), (21, 16, 30), (21, 13, -40)])
def test_alexnet_bin_linears_at_batch_256(dev, split, K, Nf, exp):
    # 4096 -> 10: N % 4 != 0 takes pm1_matmul; 21 -> 16 / 13: odd K (the pack tail of a row) on both grad_x forms
    _bin_linear_case(dev, K, Nf, split, K + Nf, exp)


# ---- DoReFa W1A4 (ResNet-18): DorefaConv2d(bit_width=1) on nnDorefaQuant(4) codes ----------------------------------------------

def _dorefa_case(dev, Cin, Cout, H, k, s, p, split, seed, amp, exp, w_bits=1, N=BATCH, big_codes=False):
    n_a = 15.0
    codes = G.int_uniform((N, Cin, H, H), 0, 15, seed + 1, dev)
    if big_codes:       # 1 % of the codes beyond int8 (the un-clamped quantiser): the digit route / the fp16 plane with poison
        gen = G._gen(seed + 3, dev)
        big = torch.randint(200, 301, codes.shape, generator=gen, device=dev).float()
        codes = torch.where(torch.rand(codes.shape, generator=gen, device=dev) < 0.01, big, codes)
        codes = codes.contiguous(memory_format=torch.channels_last)
    # codes beyond int8: the pixel-major fp16 plane keeps them (one pass, chunked scale); otherwise 256-digits, (256 GW(hi) +
    # GW(lo)) * fl(1 / n) once (_fused.dorefa_conv_grad_weight)
    digits = big_codes and (split == "bf16x3" or k == 1)
    x0 = (codes / n_a).contiguous(memory_format=torch.channels_last).requires_grad_()
    Ho = (H + 2 * p - k) // s + 1
    if w_bits == 1:
        layer = DorefaConv2d(Cin, Cout, k, stride=s, padding=p, bias=False, bit_width=1).to(dev).to(memory_format=torch.channels_last)
        layer.weight.data.copy_(G.latent_weight(layer.weight.shape, seed, dev, -1.0, 1.0))
        wparam = layer.weight
        E = ops.abs_mean(layer.weight.detach())
        assert abs(float(E) - float(layer.weight.detach().double().abs().mean())) <= 1e-6 * float(E)
        wimg = G.safe_sign(layer.weight)
        gx_scale = E
    else:
        n_w = float((1 << w_bits) - 1)
        lv = (2 * torch.randint(-(1 << (w_bits - 1)), 1 << (w_bits - 1), (Cout, Cin, k, k), device=dev) + 1).float()  # odd levels
        wparam = (lv / n_w).requires_grad_()
        wimg = lv
        gx_scale = _fused._inv_levels(w_bits)
    with lazy_train.eager(), ops.float_split(split):
        x = nnDorefaQuant(4)(x0)
        x.retain_grad()
        if w_bits == 1:
            y = layer(x)
        else:
            y = _fused.DorefaWkConv2dFn.apply(x, wparam, None, w_bits, (s, p, 1, 1))
        for name, ek in _designs(Cout, exp, seed):
            g = G.grad_ints((N, Cout, Ho, Ho), amp, seed + 2, dev, **ek)
            per = name == "per-channel"
            what = f"DoReFa W{w_bits}A4 {Cin}->{Cout} k{k}/s{s} at {H}, {split}, {name}"
            wparam.grad = x.grad = None
            if k == 1:
                expect = ["qt_bf16_gemm_taps", "qt_wgrad_reduce_f32"]           # K-sliced GEMM over the sub-sampled positions
            else:
                expect = ["qt_wgrad_pm_reduce_f32"]
            if digits:
                expect.append("qt_digit_combine_f32")
            backward_traced(y, g, what, expect + ["qt_conv2d_implicit"], [] if digits else ["qt_digit_combine_f32"])
            q = torch.round(x.detach() * n_a)
            assert torch.equal(q, codes), "the quantiser's codes are not the designed ones"
            # codes beyond int8: the fp16 plane reads q (exact to 2048), the digit route its 256-digits (exact in bf16, and each
            # digit's sum is bounded by that of q)
            _prove(g, q, lambda a, b: G.conv_grad_weight64(b, a, k, s, p), split, what + " grad_W", per_channel=per,
                   b_exact_in=(torch.float16,) if big_codes else (torch.float16, torch.bfloat16))
            if k == 1:
                chunks = _gemm_chunks(N, Cout, Cin, Ho, Ho, 1, 0)
            elif s > 1:          # the pixel-major kernel on the space-to-depth image (ops.conv2d_grad_weight_strided)
                chunks = _pm_chunks(N, Cout, Cin * s * s, H // s, H // s, 3, 1)
            else:
                chunks = _pm_chunks(N, Cout, Cin, H, H, k, p)
            parts = G.conv_grad_weight64(q, g, k, s, p, chunks=chunks)
            if digits:
                dW = G.scaled(G.to_f32_exact(sum(parts) if isinstance(parts, list) else parts), ops._inv_f32(n_a))
            else:
                dW = G.chunked_sum(parts, ops._inv_f32(n_a))
            _check(wparam.grad, dW, what + " grad_W")
            if not per:
                _prove(g, wimg, lambda a, b: G.conv_grad_input64(a, b, (H, H), s, p), split, what + " grad_x")
                S = G.to_f32_exact(G.conv_grad_input64(g, wimg, (H, H), s, p))
                _check(x.grad, G.scaled(S, gx_scale), what + " grad_x", ("n", "c", "y", "x"))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("Cin,Cout,H,k,s,p,w_bits", [
    (64, 64, 32, 3, 1, 1, 1),       # layer1: Cout % 128 != 0, the 64-row pixel-major kernel
    (128, 128, 16, 3, 1, 1, 1),     # layer2: the full kernel
    (64, 128, 32, 3, 2, 1, 1),      # stride 2: zero-dilated grad_x, space-to-depth weight gradient and its tap gather
    (64, 128, 32, 1, 2, 0, 1),      # 1x1 stride-2 shortcut: the K-sliced GEMM
    (256, 512, 8, 1, 2, 0, 1),      # the last shortcut
    (128, 256, 16, 3, 2, 1, 1),     # layer3's stride-2 conv
    (128, 256, 16, 1, 2, 0, 1),     # layer3's shortcut
    (256, 512, 8, 3, 2, 1, 1),      # layer4's stride-2 conv
    (256, 256, 8, 3, 1, 1, 1),      # layer3
    (512, 512, 4, 3, 1, 1, 1),      # the 4x4 maps of the last stage
    (64, 64, 32, 3, 1, 1, 4),       # W4: level grad_x with fl(1 / n_w)
])
def test_dorefa_resnet18_convs_at_batch_256(dev, split, Cin, Cout, H, k, s, p, w_bits):
    # caught: under the exact three-term split ("bf16x3") the implicit conv's bf16 epilogue dropped its output scale, so grad_x
    # of these layers came out without E = mean|W| (W1) or fl(1 / n_w) (W4) — about 2x too large (csrc/mfma_gemm_kernel.h)
    _dorefa_case(dev, Cin, Cout, H, k, s, p, split, Cin + Cout + k + s, 3, -40 if s == 1 else 30, w_bits=w_bits)


# ---- edges --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("Cin,Cout,H,k,s,p", [(64, 64, 32, 3, 1, 1), (64, 128, 32, 1, 2, 0), (64, 128, 32, 3, 2, 1)])
def test_dorefa_codes_beyond_int8_at_batch_256(dev, split, Cin, Cout, H, k, s, p):
    _dorefa_case(dev, Cin, Cout, H, k, s, p, split, Cin + Cout + 7 * k + s, 1, -40 if s == 1 else 30, big_codes=True)


@pytest.fixture()
def small_wgrad_budget():
    prev = ops.WGRAD_GEMM_BYTES
    try:
        yield
    finally:
        ops.WGRAD_GEMM_BYTES = prev


# Chunks halve from the batch, so a batch of 256 is always cut into equal powers of two: the ragged tails take a batch of 249.
RAGGED = 249


def test_ragged_chunks_pixel_major(dev, small_wgrad_budget):
    # 64 -> 64 3x3 at 32^2: chunks of 63 images plan 238 K slices, the 60-image tail 255 (ops._wgrad_pm_run sizes its buffers
    # for both); the 4-bit activation's fl(1 / 15) is applied per chunk, so the chunk boundaries are visible in the result
    N, C, H = RAGGED, 64, 32
    ops.WGRAD_GEMM_BYTES = 100 << 20
    chunks = _pm_chunks(N, C, C, H, H, 3, 1)
    slices = [ops.wgrad_pm_plan(c, C, C, H, H, H, 3, 3, 1, 1, ops.WGRAD_PM_WORKGROUPS)[1] for c in (chunks[0], chunks[-1])]
    assert len(set(chunks)) > 1 and slices[1] > slices[0], (chunks, slices)
    for split in SPLITS:
        _dorefa_case(dev, C, C, H, 3, 1, 1, split, 77, 3, -40, N=N)


def test_ragged_chunks_k_major_shortcut(dev, small_wgrad_budget):
    N, Cin, Cout, H = RAGGED, 64, 128, 32
    ops.WGRAD_GEMM_BYTES = 30 << 20
    chunks = _gemm_chunks(N, Cout, Cin, H // 2, H // 2, 1, 0)
    assert len(set(chunks)) > 1, chunks
    for split in SPLITS:
        _dorefa_case(dev, Cin, Cout, H, 1, 2, 0, split, 78, 3, 30, N=N)


def test_ragged_chunks_space_to_depth_first_layer(dev, small_wgrad_budget):
    ops.WGRAD_GEMM_BYTES = 300 << 20
    for split in SPLITS:
        nt = 2 if split == "f16x2" else 3
        chunks = _pm_chunks(RAGGED, 192, nt * 48, 57, 57, 3, 0)
        assert len(set(chunks)) > 1, chunks
        _bin_conv_case(dev, 3, 192, 224, 11, 4, 2, split, 79, 2, -40, real_image=True, N=RAGGED)


@pytest.mark.parametrize("Cin,Cout", [(33, 65), (65, 130), (100, 200)])
def test_channels_off_the_tile_grid(dev, Cin, Cout):
    for split in SPLITS:
        _bin_conv_case(dev, Cin, Cout, 13, 3, 1, 1, split, Cin * Cout, 8, -40)
        _dorefa_case(dev, Cin, Cout, 16, 3, 1, 1, split, Cin * Cout + 1, 3, 30)


def test_gradient_not_channels_last_bias_reduced_by_the_caller(dev):
    for split in SPLITS:
        _bin_conv_case(dev, 192, 576, 27, 5, 1, 2, split, 81, 8, -40, cl_grad=False)


def test_dorefa_forwards_with_an_output_scale_under_the_exact_split(dev):
    # the bf16 element of the implicit conv once ignored its output scale: under "bf16x3" these forwards (and the DoReFa grad_x
    # above) came out without E = mean|W| / fl(1 / n_w)
    N, C, Co, H = 32, 64, 96, 16
    x = G.int_uniform((N, C, H, H), -8, 8, 5, dev) * 2.0 ** -3               # real-valued, untagged: the split route
    w = G.latent_weight((Co, C, 3, 3), 6, dev, -1.0, 1.0)
    S = G.to_f32_exact(_exact_conv64(x, G.safe_sign(w)))
    with lazy_train.eager(), ops.float_split("bf16x3"):
        layer = DorefaConv2d(C, Co, 3, padding=1, bias=False, bit_width=1).to(dev).to(memory_format=torch.channels_last)
        layer.weight.data.copy_(w)
        (y, _, calls, lib) = profiled(lambda: layer(x))
        assert not lib and calls.get("qt_conv2d_implicit"), (calls, lib)
        _check(y, G.scaled(S, ops.abs_mean(w)), "DoReFa W1 forward, bf16x3", ("n", "c", "y", "x"))
        lv = (2 * torch.randint(-8, 8, (Co, C, 3, 3), device=dev) + 1).float()
        wq = lv / 15.0
        y4 = _fused.dorefa_levels_conv_forward(x, wq, None, (1, 1, 1, 1), 4)
        S4 = G.to_f32_exact(_exact_conv64(x, lv))
        _check(y4, G.scaled(S4, _fused._inv_levels(4)), "DoReFa W4 level forward, bf16x3", ("n", "c", "y", "x"))


def _exact_conv64(x, w):
    Cout = int(w.shape[0])
    cols = torch.nn.functional.unfold(x.to(torch.float64), 3, padding=1)
    return torch.matmul(w.to(torch.float64).reshape(Cout, -1), cols).reshape(x.shape[0], Cout, x.shape[2], x.shape[3])


# ---- (c) Gaussian data --------------------------------------------------------------------------------------------------------

def _gauss(shape, seed, dev, decades=6.0, channels_last=True):
    """randn with channel c (dim 1) scaled by 10^(u_c), u over ``decades`` decades: the lo / mid planes of every split carry data."""
    gen = G._gen(seed, dev)
    v = torch.randn(tuple(shape), generator=gen, device=dev)
    u = torch.linspace(-decades / 2, decades / 2, int(shape[1]), device=dev)[torch.randperm(int(shape[1]), generator=gen, device=dev)]
    v = v * torch.pow(10.0, u).reshape((1, -1) + (1,) * (len(shape) - 2))
    return v.contiguous(memory_format=torch.channels_last) if channels_last and len(shape) == 4 else v


def _rows_err(got, want, dim):
    """normwise error per slice along ``dim``: max|got - want| / max|want| of each slice."""
    d = (got.double() - want).abs().movedim(dim, 0).reshape(got.shape[dim], -1).amax(1)
    m = want.abs().movedim(dim, 0).reshape(got.shape[dim], -1).amax(1)
    return d / torch.where(m > 0, m, torch.ones_like(m))


# Bars.  grad_W: 1e-5 normwise per output channel (a row of dW sees one gradient channel; the two-plane split scales per
# channel, test_weight_gradient_pixel_major_both_splits_vs_fp64).  grad_x: 1e-5 normwise per image — under the per-tensor scale
# a channel 10^6 below the largest keeps ~2^-39 of max|g| absolute, far under 1e-5 of the image's largest sum, which the large
# channels dominate; per channel of grad_x no bar is claimed.  Bias: |err| <= 1e-5 * sum|g| of the channel (a Gaussian
# channel's sum can cancel).
BAR = 1e-5


@pytest.mark.parametrize("split", SPLITS)
def test_gaussian_alexnet_conv2_and_conv1_at_batch_256(dev, split):
    with lazy_train.eager(), ops.float_split(split):
        layer = BinConv2d(192, 576, 5, padding=2).to(dev).to(memory_format=torch.channels_last)
        layer.weight.data.copy_(G.latent_weight(layer.weight.shape, 21, dev))
        x0 = (G.pm1((BATCH, 192, 27, 27), 22, dev) * 0.5).requires_grad_()
        x = BinaryConnectDeterministic.apply(x0)
        x.retain_grad()
        y = layer(x)
        g = _gauss((BATCH, 576, 27, 27), 23, dev)
        case = f"Gaussian conv2, {split}"
        backward_traced(y, g, case, ["qt_wgrad_pm_reduce_f32", "qt_wgrad_pm_bias_reduce_f32", "qt_conv2d_implicit"])
        ref = G.conv_grad_weight64(x.detach(), g, 5, 1, 2)
        ref = torch.where(layer.weight.detach().abs() <= torch.tensor(G.STE_THRESHOLD, dtype=torch.float32), ref, 0.0)
        e = _rows_err(layer.weight.grad, ref, 0)
        assert float(e.max()) <= BAR, (case, "grad_W per channel", float(e.max()))
        gx = G.conv_grad_input64(g, G.safe_sign(layer.weight), (27, 27), 1, 2)
        e = _rows_err(x.grad, gx, 0)
        assert float(e.max()) <= BAR, (case, "grad_x per image", float(e.max()))
        db = (layer.bias.grad.double() - G.bias_grad64(g)).abs()
        assert bool((db <= BAR * G.bias_grad64(g.abs())).all()), (case, "bias", float(db.max()))

        c1 = BinConv2d(3, 192, 11, stride=4, padding=2).to(dev).to(memory_format=torch.channels_last)
        c1.binary_input = False
        c1.weight.data.copy_(G.latent_weight(c1.weight.shape, 24, dev))
        img = torch.randn((BATCH, 3, 224, 224), generator=G._gen(25, dev), device=dev).contiguous(memory_format=torch.channels_last)
        y1 = c1(img)
        g1 = _gauss((BATCH, 192, 55, 55), 26, dev)
        case = f"Gaussian conv1 (real image), {split}"
        backward_traced(y1, g1, case, ["qt_wgrad_pm_reduce_f32", "qt_wgrad_pm_bias_reduce_f32"])
        ref = G.conv_grad_weight64(img, g1, 11, 4, 2)
        ref = torch.where(c1.weight.detach().abs() <= torch.tensor(G.STE_THRESHOLD, dtype=torch.float32), ref, 0.0)
        e = _rows_err(c1.weight.grad, ref, 0)
        assert float(e.max()) <= BAR, (case, "grad_W per channel", float(e.max()))
        db = (c1.bias.grad.double() - G.bias_grad64(g1)).abs()
        assert bool((db <= BAR * G.bias_grad64(g1.abs())).all()), (case, "bias", float(db.max()))


@pytest.mark.parametrize("split", SPLITS)
def test_gaussian_dorefa_and_linear_at_batch_256(dev, split):
    with lazy_train.eager(), ops.float_split(split):
        for Cin, Cout, H, s in ((64, 64, 32, 1), (64, 128, 32, 2)):
            layer = DorefaConv2d(Cin, Cout, 3, stride=s, padding=1, bias=False, bit_width=1).to(dev).to(memory_format=torch.channels_last)
            layer.weight.data.copy_(G.latent_weight(layer.weight.shape, Cin + s, dev, -1.0, 1.0))
            codes = G.int_uniform((BATCH, Cin, H, H), 0, 15, Cout + s, dev)
            x0 = (codes / 15.0).contiguous(memory_format=torch.channels_last).requires_grad_()
            x = nnDorefaQuant(4)(x0)
            x.retain_grad()
            y = layer(x)
            g = _gauss((BATCH, Cout, H // s, H // s), Cin * s, dev)
            case = f"Gaussian DoReFa {Cin}->{Cout}/s{s}, {split}"
            backward_traced(y, g, case, ["qt_wgrad_pm_reduce_f32", "qt_conv2d_implicit"])
            ref = G.conv_grad_weight64(codes, g, 3, s, 1) / 15.0
            e = _rows_err(layer.weight.grad, ref, 0)
            assert float(e.max()) <= BAR, (case, "grad_W per channel", float(e.max()))
            gx = G.conv_grad_input64(g, G.safe_sign(layer.weight), (H, H), s, 1) * float(ops.abs_mean(layer.weight.detach()))
            e = _rows_err(x.grad, gx, 0)
            assert float(e.max()) <= BAR, (case, "grad_x per image", float(e.max()))
        lin = LinearBin(4096, 4096).to(dev)
        lin.weight.data.copy_(G.latent_weight(lin.weight.shape, 31, dev))
        x0 = (G.pm1((BATCH, 4096), 32, dev) * 0.5).requires_grad_()
        x = BinaryConnectDeterministic.apply(x0)
        x.retain_grad()
        y = lin(x)
        g = _gauss((BATCH, 4096), 33, dev)
        case = f"Gaussian LinearBin 4096->4096, {split}"
        backward_traced(y, g, case)
        ref = torch.where(lin.weight.detach().abs() <= torch.tensor(G.STE_THRESHOLD, dtype=torch.float32),
                          G.linear_grad_w64(g, x.detach()), 0.0)
        e = _rows_err(lin.weight.grad, ref, 0)
        assert float(e.max()) <= BAR, (case, "grad_W per feature", float(e.max()))
        e = _rows_err(x.grad, G.linear_grad_x64(g, G.safe_sign(lin.weight)), 0)
        assert float(e.max()) <= BAR, (case, "grad_x per row", float(e.max()))


# ---- (e) route coverage -------------------------------------------------------------------------------------------------------

# torch's own kernels in a training step's backward (loss, log-softmax, elementwise, reductions, copies): not this project's code
ALLOW = [
    (r"^at::", "torch's own kernels: loss backward, elementwise ops, reductions, fills and copies"),
    (r"^softmax_warp_backward<", "torch's log-softmax backward"),
    (r"^Memset", "runtime memsets of torch's gradient buffers"),
    (r"^Cijk_", "hipBLASLt GEMMs of a plain torch nn.Linear (DoReFa ResNet-18's fp32 classifier, not a quantised layer)"),
    (r"^(igemm_wrw_|naive_conv_|_ZN2ck|SubTensorOp)", "MIOpen backward of a plain torch nn.Conv2d (DoReFa ResNet-18's fp32 stem)"),
    (r"^MIOpenBatchNormBwd", "torch's nn.BatchNorm2d backward (DoReFa ResNet-18 BatchNorms outside the fused chains)"),
]
# backward kernels of the steps that this module does not compare, each with where it is checked instead
KNOWN_UNCOVERED = [
    (r"^(bwd_dx_kernel|bwd_sum_kernel|fold2_kernel|pool_bwd_kernel)$",
     "training chains of train_chain.hip ([MaxPool,] BatchNorm, Hardtanh, sign / the DoReFa form): exact on designed operands "
     "and vs fp64 at the batch-256 row counts, tests/test_gpu_train_chain_b256.py"),
    (r"^(act_bwd_dx_kernel|act_bwd_sum_kernel)$",
     "DoReFa chain BatchNorm [+ residual] -> ReLU -> quantiser: exact on designed operands and vs fp64 at the batch-256 row "
     "counts, tests/test_gpu_train_chain_b256.py"),
    (r"ElemF16Taps",
     "XNOR-Net per-tap grad_x: bit-exact vs float64 on every configuration and at batch 256, "
     "tests/test_gpu_xnor_b256.py::test_grad_input_is_bit_exact_on_designed_operands"),
]


def _step_backward_kernels(name, dev):
    import bench_models
    import torch.nn.functional as F
    torch.manual_seed(0)
    if name == "alexnet_bin":
        model = bench_models.AlexNetBin()
        x = torch.randn(BATCH, 3, 224, 224, device=dev)
    elif name == "alexnet_xnor":
        from pytorch_quantize_impls_amd.layers import LinearXNOR, XNORConv2d
        model = bench_models.alexnet_xnor()
        for mod in model.modules():
            if isinstance(mod, (XNORConv2d, LinearXNOR)):
                mod.weight.data.normal_(0, 0.05)
                mod.bias.data.zero_()
        x = torch.randn(BATCH, 3, 224, 224, device=dev)
    else:
        model = bench_models.DorefaResNet18(w_bits=1, a_bits=4)
        x = torch.randn(BATCH, 3, 32, 32, device=dev)
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    x = x.contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 10, (BATCH,), device=dev)
    out = model(x)
    if name == "dorefa_resnet18":
        out = F.log_softmax(out, 1)
    loss = F.nll_loss(out, t)
    _, kernels, _, lib = profiled(loss.backward)
    return kernels, lib


def test_every_backward_kernel_of_the_training_steps_was_compared(dev):
    allow = [re.compile(p) for p, _ in ALLOW]
    known = {k: why for k, why in KNOWN_UNCOVERED}
    report, missing = [], {}
    for name in ("alexnet_bin", "alexnet_xnor", "dorefa_resnet18"):
        kernels, lib = _step_backward_kernels(name, dev)
        assert not lib, f"{name} step: dense-library paths in the backward: {lib}"
        for k in sorted(kernels):
            if k in COVERED:
                report.append(f"  {name}: {k} <- {COVERED[k][0]}")
            elif any(a.search(k) for a in allow):
                continue
            elif any(re.search(p, k) for p in known):
                report.append(f"  {name}: {k} NOT compared here ({next(w for p, w in known.items() if re.search(p, k))})")
            else:
                missing.setdefault(k, []).append(name)
    worst = max(PEAK.items(), key=lambda kv: kv[1]) if PEAK else ("-", 0)
    print("\nbackward kernels of the batch-256 training steps:\n" + "\n".join(report)
          + f"\npeak device memory of the module: {worst[1] / 2**30:.2f} GiB ({worst[0]})")
    assert not missing, "backward kernels of the training steps that no case compared:\n" + "\n".join(
        f"  {k}  ({', '.join(v)})" for k, v in sorted(missing.items()))
