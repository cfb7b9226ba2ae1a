"""Threshold-bit convs at the configs' own batch and at the size edges of the direct 3x3 kernel, every output bit against the
exact reference of tests/_exact.py (float64 integer sums on the device, the fused blocks' fp32 predicate).

  * the layer shapes of C3 (AlexNet-Bin conv2-conv5) and C5 (VGG-16 conv1_2-conv5_x) at batch 256 through the entry points the
    fused blocks call (ops.conv2d_nib, ops.conv3x3_direct_nib): bit planes and nibble halo planes, binary and ternary weights,
    the sign-bit (ElemFp4T), compare (ops.CONV_COMPARE_THRESHOLDS) and float (no thresholds) epilogues, pooled bits where AlexNet pools,
    edge channels (zero / NaN slopes, huge and infinite offsets, exact ties);
  * the real-valued first layers (VGG conv1_1: first3x3, AlexNet conv1: first_direct) at batch 256 against float64;
  * both fused networks block by block at batch 256, each block fed with the exact reference chain's activation;
  * the direct kernel at tiny maps, at padded widths / heights around 256, over its lean and general epilogue instances, with an
    input plane past 2 GiB (the pointer path) and an output plane past 4 GiB;
  * the kernel configuration every case ran (torch.profiler), and one test that every fp4 threshold-epilogue configuration the
    dispatcher selects with default switches ran against the exact reference in this module.

Run the whole module: the coverage test reads what the cases before it recorded."""
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _routes as R

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import ops  # noqa: E402

BATCH = 256
BUDGET = 1 << 30            # bytes of float64 temporaries per reference chunk

# the configurations with a sign-bit (ElemFp4T) instance: mfma_gemm.hip launches them through launch_cfg_t
SWAPT = {"ConvV128x128D", "ConvV128x2", "ConvVPP192", "ConvVPP256", "ConvVPP256x192"}
COVERED = {}                # route label -> case ids that compared it with the exact reference


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


PEAK = {}                   # test id -> peak device memory (bytes)


@pytest.fixture(autouse=True)
def _free_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    PEAK[request.node.name] = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()


def routes(names):
    """Profiler kernel names -> labels 'ConvVPP256<ElemFp4T>', 'direct3x3<4,2,2,2,lean>', ..."""
    names = [k.replace("(anonymous namespace)::", "") for k in names]
    out = R.mfma_routes(names, elem="ElemFp4T?")
    for k in names:
        m = re.search(r"direct3x3_kernel<(\d+), (\d+), (\d+), (\d+), 0(?:, (true|false))?>", k)
        if m:
            out.add(f"direct3x3<{m.group(1)},{m.group(2)},{m.group(3)},{m.group(4)},{'lean' if m.group(5) == 'true' else 'general'}>")
        for first in ("first3x3_kernel", "conv_first_direct_kernel"):
            if first in k:
                out.add(first)
    return out


def traced(fn, expect, case, described=None):
    """Run fn under torch.profiler and assert that the kernel ``expect`` (a label of routes()) ran — and, where the case has a
    describe entry point (``described``: its answer), that it names that kernel."""
    R.assert_described(described, expect, case)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    seen = routes(e.key for e in prof.key_averages())
    assert expect in seen, (case, expect, sorted(map(str, seen)))
    return out


def record(expect, case):
    COVERED.setdefault(expect, []).append(case)


def _affine(Cout, K, seed, dev, edges=True):
    """bias, alpha, beta with thresholds spread over the populated range of a K-term +-1 sum; with ``edges`` the channels of
    test_gpu_r6's edge set (zero / negative-zero / NaN slopes, +-1e6 and +-inf offsets) and three exact ties at acc = 2."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    bias = torch.randn(Cout, generator=g, device=dev) * 3
    alpha = (torch.rand(Cout, generator=g, device=dev) - 0.5) * 0.6
    beta = -alpha * torch.randn(Cout, generator=g, device=dev) * (0.5 * K ** 0.5)
    if edges:
        alpha[0], beta[0] = 0.0, 0.5
        alpha[1], beta[1] = 0.0, -1.0
        beta[2], beta[3] = 1e6, -1e6
        alpha[4], beta[4] = -0.0, 1.0
        alpha[5] = float("nan")
        beta[6], beta[7] = float("inf"), float("-inf")
        alpha[8], beta[8], bias[8] = 1.0, -2.0, 0.0              # bit <=> acc < 2
        alpha[9], beta[9], bias[9] = -1.0, 2.0, 0.0              # bit <=> acc > 2
        alpha[10], beta[10], bias[10] = 0.5, -1.25, 0.5          # bit <=> acc < 2, through two roundings
    return bias, alpha, beta


def _weights(Cout, Cin, k, kind, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if kind == "binary":
        return (torch.randint(0, 2, (Cout, Cin, k, k), generator=g, device=dev) * 2 - 1).float()
    return torch.randint(-1, 2, (Cout, Cin, k, k), generator=g, device=dev).float()


class Out:
    """A kernel output to compare: bit plane ([N*Ho*Wo, ld]) or nibble halo plane, optionally of the max-pooled conv."""

    def __init__(self, name, planes, Ho, Wo, halo=None, pool=None):
        self.name, self.Ho, self.Wo, self.halo, self.pool = name, Ho, Wo, halo, pool
        self.words = planes.sign if isinstance(planes, ops.BitPlanes) else planes.words

    def bits(self, idx, C):
        n = int(idx.numel())
        if self.halo is None:
            w = self.words.view(-1, self.Ho * self.Wo, self.words.shape[1])[idx]
            X.check_pad_bits(w, C, self.name)
            return X.bits_of_words(w, C).view(n, self.Ho, self.Wo, C)
        hy, hx = self.halo
        w = self.words.view(-1, (self.Ho + 2 * hy) * (self.Wo + 2 * hx), self.words.shape[1])[idx]
        return X.nib_to_bits(X.decode_nib(w.reshape(-1, w.shape[-1]), n, self.Ho, self.Wo, C, self.halo))


def compare(words, N, H, W, Cin, wq, stride, pad, affine, outs, images=None, case=""):
    """Every listed image of every output against the exact reference (chunks of images, one float64 conv per chunk)."""
    bias, alpha, beta = affine
    Cout, k = int(wq.shape[0]), int(wq.shape[2])
    dev = words.device
    idx_all = torch.arange(N, device=dev) if images is None else torch.as_tensor(sorted(set(images)), device=dev)
    step = X.image_chunk(X.conv_bytes_per_image(Cin, H, W, Cout, k, stride, pad), BUDGET)
    w3 = words.view(N, H * W, words.shape[1])
    for i in range(0, int(idx_all.numel()), step):
        idx = idx_all[i:i + step]
        n = int(idx.numel())
        acc = X.exact_conv(X.pm1_nchw(w3[idx].reshape(n * H * W, -1), n, H, W, Cin), wq, stride, pad)
        for o in outs:
            a = F.max_pool2d(acc, *o.pool) if o.pool else acc
            want, v = X.predicate(a, bias, alpha, beta)
            msg = X.mismatch_report(o.bits(idx, Cout), want.permute(0, 2, 3, 1), a.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1),
                                    images=idx.tolist(), what=f"{case} {o.name}")
            assert not msg, msg
        del acc


def pm1_input(N, H, W, Cin, pad, seed, dev):
    words = X.random_bit_words(N * H * W, Cin, seed, dev)
    px = ops.bits_to_nib_pad(ops.BitPlanes(sign=words, rows=N * H * W, K=Cin), N, H, W, (pad, pad), ld=ops.pixel_ld_nib(Cin))
    return words, px


def run_implicit(dev, case, N, Cin, Cout, H, k, kind, cfg, pool=None, forms=("swapt", "compare", "float"),
                 nib_halo=(1, 1), seed=1):
    """ops.conv2d_nib (the implicit-GEMM conv on the physically padded nibble plane, as the fused blocks call it) with the
    threshold epilogue in the listed forms, bit planes and nibble halo planes, against the exact reference."""
    W, pad = H, k // 2
    words, px = pm1_input(N, H, W, Cin, pad, seed, dev)
    wq = _weights(Cout, Cin, k, kind, seed + 1, dev)
    wp = ops.pack_conv_weight_nib(wq, kind)
    K = Cin * k * k
    bias, alpha, beta = _affine(Cout, K, seed + 2, dev)
    thr = ops.integer_thresholds(bias, alpha, beta, K)
    args = (px, (N, Cin, H + 2 * pad, W + 2 * pad), wp, (k, k), bias, 1, 0, 1)
    outs = []
    for form in forms:
        t = None if form == "float" else thr
        elem = "ElemFp4T" if (form == "swapt" and cfg in SWAPT) else "ElemFp4"
        label = f"{cfg}<{elem}>"
        flags = ops.CONV_COMPARE_THRESHOLDS if form == "compare" else 0
        named = [ops.conv_kernel_name(0, N, H + 2 * pad, W + 2 * pad, px.ld, (k, k), (1, 1), (0, 0), (1, 1), wp.ld, Cout, epilogue=e,
                                      has_thr=t is not None, variant=flags) for e in (ops.EPI_BITS, ops.EPI_NIB)]
        with ops.scope(CONV_FLAGS=flags):
            bits = traced(lambda: ops.conv2d_nib(*args, epi=(alpha, beta, t)), label, f"{case} {form} bits", named[0])
            nib = traced(lambda: ops.conv2d_nib(*args, epi=ops.NibEpilogue(alpha, beta, nib_halo, thr=t)), label, f"{case} {form} nib",
                         named[1])
        outs += [Out(f"{form}/bits", bits, H, W), Out(f"{form}/nib", nib, H, W, halo=nib_halo)]
        if pool:
            Hp = (H - pool[0]) // pool[1] + 1
            neg = ops.neg_alpha_words(alpha)
            pb, _ = ops.pool_bits(bits, N, H, W, pool[0], pool[1], neg)
            pn, _ = ops.pool_bits_nib(bits, N, H, W, pool[0], pool[1], neg, (1, 1))
            outs += [Out(f"{form}/pooled bits", pb, Hp, Hp, pool=pool), Out(f"{form}/pooled nib", pn, Hp, Hp, halo=(1, 1), pool=pool)]
        record(label, case)
    compare(words, N, H, W, Cin, wq, 1, pad, (bias, alpha, beta), outs, case=case)


def direct_label(Cin, Cout, out_bits, N, H, W):
    """The direct3x3_kernel instance qt_conv3x3_direct_nib launches (csrc/direct_conv3x3.hip, host side)."""
    cw = ops.pixel_ld_nib(Cin)
    ldo = ops.packed_ld(Cout) if out_bits else ops.pixel_ld_nib(Cout)
    out_bytes = N * H * W * ldo * 4 if out_bits else N * (H + 2) * (W + 2) * ldo * 4
    bits_ok = ldo == 4 if Cout == 128 else (cw == 8 and ldo in (2, 4))
    lean = Cout in (64, 128) and out_bytes < (1 << 32) and (not out_bits or bits_ok)
    inst = {(8, True): "2,2,1,3", (8, False): "2,4,1,2", (16, True): "4,1,2,2", (16, False): "4,2,2,2"}[(cw, Cout <= 64)]
    return f"direct3x3<{inst},{'lean' if lean else 'general'}>"


def run_direct(dev, case, N, Cin, Cout, H, W, kind, outs_wanted=("bits", "nib"), images=None, seed=1):
    """ops.conv3x3_direct_nib (the direct kernel on the halo-1 nibble plane) with bit-plane and nibble-plane output against the exact
    reference; ``images``: the batch indices to check (default: all)."""
    words, px = pm1_input(N, H, W, Cin, 1, seed, dev)
    wq = _weights(Cout, Cin, 3, kind, seed + 1, dev)
    wp = ops.pack_conv_weight_nib(wq, kind)
    bias, alpha, beta = _affine(Cout, Cin * 9, seed + 2, dev)
    outs = []
    for form in outs_wanted:
        bits_out = form == "bits"
        label = direct_label(Cin, Cout, bits_out, N, H, W)
        epi = (alpha, beta) if bits_out else ops.NibEpilogue(alpha, beta, (1, 1))
        o = traced(lambda: ops.conv3x3_direct_nib(px, N, Cin, H, W, wp, bias, epi), label, f"{case} {form}")
        outs.append(Out(form, o, H, W) if bits_out else Out(form, o, H, W, halo=(1, 1)))
        record(label, case)
    compare(words, N, H, W, Cin, wq, 1, 1, (bias, alpha, beta), outs, images=images, case=case)


# ---- the C3 / C5 layer shapes at batch 256 ----------------------------------------------------------------------------------

# (case, Cin, Cout, H, k, kind, configuration the dispatcher picks at batch 256, pooling of the fused block)
IMPLICIT_LAYERS = [
    ("alexnet.conv2", 192, 576, 27, 5, "binary", "ConvVPP192", (3, 2)),
    ("alexnet.conv3", 576, 1152, 13, 3, "binary", "ConvVPP256x192", None),
    ("alexnet.conv3/ternary", 576, 1152, 13, 3, "ternary", "ConvVPP256x192", None),
    ("alexnet.conv4", 1152, 768, 13, 3, "binary", "ConvVPP256", None),
    ("alexnet.conv5", 768, 256, 13, 3, "binary", "ConvVPP256", (3, 2)),
    ("vgg.conv3_1", 128, 256, 56, 3, "ternary", "ConvV128x2", None),
    ("vgg.conv3_1/binary", 128, 256, 56, 3, "binary", "ConvV128x2", None),
    ("vgg.conv3_2", 256, 256, 56, 3, "ternary", "ConvVPP256", None),
    ("vgg.conv4_1", 256, 512, 28, 3, "ternary", "ConvVPP256", None),
    ("vgg.conv4_2", 512, 512, 28, 3, "ternary", "ConvVPP256", None),
    ("vgg.conv5_1", 512, 512, 14, 3, "ternary", "ConvVPP256", None),
]


@pytest.mark.parametrize("case,Cin,Cout,H,k,kind,cfg,pool", IMPLICIT_LAYERS, ids=[c[0] for c in IMPLICIT_LAYERS])
def test_implicit_threshold_conv_at_batch_256(dev, case, Cin, Cout, H, k, kind, cfg, pool):
    run_implicit(dev, case, BATCH, Cin, Cout, H, k, kind, cfg, pool, seed=zlib.crc32(case.encode()) % 10007)


DIRECT_LAYERS = [
    ("vgg.conv1_2", 64, 64, 224, "ternary"),
    ("vgg.conv2_1", 64, 128, 112, "ternary"),
    ("vgg.conv2_1/binary", 64, 128, 112, "binary"),
    ("vgg.conv2_2", 128, 128, 112, "ternary"),
]


@pytest.mark.parametrize("case,Cin,Cout,H,kind", DIRECT_LAYERS, ids=[c[0] for c in DIRECT_LAYERS])
def test_direct_threshold_conv_at_batch_256(dev, case, Cin, Cout, H, kind):
    run_direct(dev, case, BATCH, Cin, Cout, H, H, kind, seed=Cin + Cout + H)


# ---- configurations the model layers do not reach at batch 256: small synthetic shapes --------------------------------------

SYNTHETIC = [
    # (case, N, Cin, Cout, H, kind, cfg, why the dispatcher picks it; M = N * H * H, K = bytes of an im2col row)
    ("skinny", 4, 512, 256, 13, "binary", "ConvVSkinny", "M = 676 <= 4096, K >= 2 KiB"),
    ("alexnet.conv3@8", 8, 576, 1152, 13, "ternary", "ConvVSkinny", "AlexNet conv3 at batch 8: M = 1352, 198 tiles of 128 x 64"),
    ("128x64D", 256, 512, 512, 4, "binary", "ConvV128x64D", "M = 4096, 256 tiles of 128 x 64"),
    ("128x128D.skinny", 256, 512, 512, 7, "ternary", "ConvV128x128D", "M = 12544: 98 tiles of 256 rows, 392 of 128 x 128"),
    ("128x128D.small_grid", 64, 256, 256, 16, "binary", "ConvV128x128D", "K = 1152 B, 64 tiles of 256 rows, 256 of 128 x 128"),
    ("64x2", 16, 128, 64, 32, "ternary", "ConvV64x2", "64 columns, K = 576 B"),
    ("128x2.tn128", 16, 128, 128, 32, "binary", "ConvV128x2", "128 columns, K = 576 B"),
    ("v64", 16, 256, 64, 32, "ternary", "ConvV64", "64 columns, K = 1152 B"),
    ("v128", 16, 256, 128, 32, "binary", "ConvV128", "128 columns, K = 1152 B"),
    ("v192", 50, 256, 192, 32, "ternary", "ConvV192", "192 columns, K = 1152 B, 200 tiles of 256 rows: the 384-row tile does not pay"),
]


@pytest.mark.parametrize("case,N,Cin,Cout,H,kind,cfg,why", SYNTHETIC, ids=[c[0] for c in SYNTHETIC])
def test_implicit_threshold_conv_synthetic_configs(dev, case, N, Cin, Cout, H, kind, cfg, why):
    run_implicit(dev, case, N, Cin, Cout, H, 3, kind, cfg, seed=N + Cin + Cout + H)


# ---- size edges of the direct 3x3 kernel ------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(1, 1), (1, 3), (2, 2), (3, 1), (3, 3)])
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (128, 128), (64, 96)])
def test_direct_tiny_maps_many_images_per_tile(dev, H, W, Cin, Cout):
    """Positions tiles of 256 over planes of 9 .. 25 positions: one tile holds up to 28 images (the lean epilogue's row / image
    carries of up to 85 rows per lane)."""
    run_direct(dev, f"tiny {H}x{W} {Cin}->{Cout}", 700, Cin, Cout, H, W, "ternary", seed=H * 10 + W + Cin)


@pytest.mark.parametrize("H,W", [(5, 253), (5, 254), (5, 255), (253, 5), (254, 5), (255, 5), (254, 254)])
@pytest.mark.parametrize("Cin,Cout", [(64, 64), (128, 128)])
def test_direct_padded_sides_around_256(dev, H, W, Cin, Cout):
    """W + 2 and H + 2 at 255 / 256 / 257: the `wide` / `tall` switch of the lean epilogue's carries."""
    run_direct(dev, f"edge {H}x{W} {Cin}->{Cout}", 6, Cin, Cout, H, W, "binary", seed=H + W + Cin)


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("Cout", [32, 64, 96, 128])
def test_direct_lean_and_general_epilogues(dev, Cin, Cout):
    """Every direct3x3_kernel instance (lean and general epilogue, one and two column waves), both output forms."""
    run_direct(dev, f"grid {Cin}->{Cout}", 12, Cin, Cout, 40, 37, "ternary", seed=Cin * 7 + Cout)


def _need_free(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"needs {nbytes / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")


def test_direct_input_plane_past_2gib(dev):
    """Cin = 128, batch 2600 at 112^2: the halo input plane is 2.16 GB, past what the kernel's buffer path addresses, so the
    pointer path loads it.  Checked: every image with bytes past 2^31, the first 4, a seeded sample of 16."""
    N, C, H = 2600, 128, 112
    plane_img = (H + 2) * (H + 2) * ops.pixel_ld_nib(C) * 4
    assert N * plane_img >= 1 << 31
    _need_free(6 << 30)
    g = torch.Generator().manual_seed(26)
    images = list(range((1 << 31) // plane_img, N)) + list(range(4)) + torch.randint(0, N, (16,), generator=g).tolist()
    run_direct(dev, "2GiB input", N, C, 128, H, H, "binary", images=images, seed=2600)


def test_direct_output_plane_past_4gib(dev):
    """A nibble output plane of 4.3 GB (128 channels, batch 5200 at 112^2): past the lean epilogue's 32-bit offsets, so the
    general epilogue writes it; the 2.2 GB input takes the pointer path as well."""
    N, C, Cout, H = 5200, 64, 128, 112
    assert N * (H + 2) ** 2 * ops.pixel_ld_nib(Cout) * 4 >= 1 << 32
    _need_free(10 << 30)
    per = (1 << 32) // ((H + 2) ** 2 * ops.pixel_ld_nib(Cout) * 4)
    g = torch.Generator().manual_seed(52)
    images = list(range(per - 2, per + 3)) + [N - 2, N - 1] + list(range(4)) + torch.randint(0, N, (16,), generator=g).tolist()
    run_direct(dev, "4GiB output", N, C, Cout, H, H, "ternary", outs_wanted=("nib",), images=images, seed=5200)


# ---- real-valued first layers at batch 256 ----------------------------------------------------------------------------------

def _first_layer_check(y0, x, wq, stride, pad, affine, planes, Ho, Wo, case):
    """fp32 result within 1e-5 (normalised) of float64; bits = the float64 predicate except at ties; bits = the float predicate on
    the kernel's own fp32 result, exactly."""
    bias, alpha, beta = affine
    N, Cout = int(x.shape[0]), int(wq.shape[0])
    y0 = y0.view(N, Ho, Wo, Cout)
    step = X.image_chunk(X.conv_bytes_per_image(int(x.shape[1]), int(x.shape[2]), int(x.shape[3]), Cout, int(wq.shape[2]), stride, pad))
    err = ref_max = 0.0
    flips = worst = 0
    total = 0
    for n0 in range(0, N, step):
        ref = X.conv64(x[n0:n0 + step], wq, stride, pad).permute(0, 2, 3, 1)
        err = max(err, float((y0[n0:n0 + step].double() - ref).abs().max()))
        ref_max = max(ref_max, float(ref.abs().max()))
        v64 = (ref + bias.double()) * alpha.double() + beta.double()
        want_f = ((y0[n0:n0 + step] + bias) * alpha < -beta)
        for o in planes:
            got = o.bits(torch.arange(n0, min(N, n0 + step), device=x.device), Cout)
            msg = X.mismatch_report(got, want_f, images=list(range(n0, n0 + int(got.shape[0]))), what=f"{case} {o.name} vs own fp32")
            assert not msg, msg
            f, wr = X.tie_flips(got, v64)
            flips, worst, total = flips + f, max(worst, wr), total + got.numel()
    assert err <= 1e-5 * ref_max, (case, err / ref_max)
    assert flips <= 1e-4 * total and worst <= 1e-5, (case, flips, total, worst)


def test_first3x3_vgg_conv1_1_at_batch_256(dev):
    torch.manual_seed(11)
    N, C, H = BATCH, 3, 224
    x = (torch.randn(N, C, H, H, device=dev) * 2.5).contiguous(memory_format=torch.channels_last)
    wq = _weights(64, C, 3, "ternary", 12, dev)
    bias, alpha, beta = _affine(64, 27, 13, dev, edges=False)
    alpha[3], alpha[10], alpha[20] = 0.0, float("nan"), -0.0
    beta[3], beta[4] = -1.0, float("inf")
    frag = ops.pack_first3x3_weight(wq)
    y0 = traced(lambda: ops.conv_first3x3(x, frag, 64, None), "first3x3_kernel", "conv1_1 fp32")
    bits = traced(lambda: ops.conv_first3x3(x, frag, 64, bias, epi=(alpha, beta)), "first3x3_kernel", "conv1_1 bits")
    nib = traced(lambda: ops.conv_first3x3(x, frag, 64, bias, epi=ops.NibEpilogue(alpha, beta, (1, 1))), "first3x3_kernel", "conv1_1 nib")
    _first_layer_check(y0, x, wq, 1, 1, (bias, alpha, beta), [Out("bits", bits, H, H), Out("nib", nib, H, H, halo=(1, 1))], H, H,
                       "vgg.conv1_1")


def test_first_direct_alexnet_conv1_at_batch_256(dev):
    torch.manual_seed(21)
    N, C, H, Cout = BATCH, 3, 224, 192
    x = torch.randn(N, C, H, H, device=dev).contiguous(memory_format=torch.channels_last)
    wq = _weights(Cout, C, 11, "binary", 22, dev)
    bias, alpha, beta = _affine(Cout, C * 121, 23, dev, edges=False)
    alpha[3], alpha[10], alpha[20] = 0.0, float("nan"), -0.0
    beta[3], beta[4] = -1.0, float("inf")
    fw = ops.pack_first_layer_weight(wq, 4)
    Ho = (H + 4 - 11) // 4 + 1
    y0 = traced(lambda: ops.conv_first_direct(x, fw, None, 4, 2), "conv_first_direct_kernel", "conv1 fp32")
    bits = traced(lambda: ops.conv_first_direct(x, fw, bias, 4, 2, epi=(alpha, beta)), "conv_first_direct_kernel", "conv1 bits")
    _first_layer_check(y0, x, wq, 4, 2, (bias, alpha, beta), [Out("bits", bits, Ho, Ho)], Ho, Ho, "alexnet.conv1")


# ---- the fused networks block by block at batch 256 -------------------------------------------------------------------------

def _as_input(words, shape, producer):
    """The reference chain's activation (bit-plane words) in the form the producing fused block hands over."""
    from pytorch_quantize_impls_amd import packed
    N, C, H, W = shape
    bits = ops.BitPlanes(sign=words, rows=N * H * W, K=C)
    halo = getattr(producer, "out_nib_halo", None) if producer is not None else None
    if halo is None:
        return packed.PackedActivation(bits, shape)
    return packed.PackedActivation(None, shape, nib=ops.bits_to_nib_pad(bits, N, H, W, tuple(halo), ld=ops.pixel_ld_nib(C)),
                                   halo=tuple(halo))


def _act_out(act):
    """Out of a block's PackedActivation: bit planes, nibble halo plane, or the (h, w, c) rows of the classifier input."""
    if act.nib is not None:
        return Out("block nib", act.nib, act.shape[2], act.shape[3], halo=act.halo)
    if len(act.shape) == 2:
        C, H, W = act.hwc
        N = act.shape[0]
        return Out("block flat bits", ops.BitPlanes(sign=act.planes.sign.view(N * H * W, C // 32), rows=N * H * W, K=C), H, W)
    return Out("block bits", act.planes, act.shape[2], act.shape[3])


def _chain(dev, blocks, convs, x, case, kernels):
    """Feed every block the exact reference chain's activation and compare its output: exact for +-1 inputs, ties-only for the
    real-valued first layer.  The chain carries the reference's bits.  ``kernels``: the kernel each conv block must run."""
    from pytorch_quantize_impls_amd.layers import FusedConvPoolBnSign, PackedMaxPool, fold_batchnorm
    N = int(x.shape[0])
    cur, shape, prev, ci = None, tuple(x.shape), None, 0
    for bi, blk in enumerate(blocks):
        C, H, W = shape[1:]
        if isinstance(blk, PackedMaxPool):
            out = blk(_as_input(cur, shape, prev))
            Ho, Wo = (H - blk.pool_k) // blk.pool_s + 1, (W - blk.pool_k) // blk.pool_s + 1
            o = _act_out(out)
            nxt = []
            step = X.image_chunk(8 * C * H * W * 2)
            for n0 in range(0, N, step):
                n = min(N, n0 + step) - n0
                xm = X.pm1_nchw(cur.view(N, H * W, -1)[n0:n0 + n].reshape(n * H * W, -1), n, H, W, C, torch.float32)
                want = (F.max_pool2d(xm, blk.pool_k, blk.pool_s) < 0).permute(0, 2, 3, 1)
                msg = X.mismatch_report(o.bits(torch.arange(n0, n0 + n, device=dev), C), want, images=list(range(n0, n0 + n)),
                                        what=f"{case} pool block {bi}")
                assert not msg, msg
                nxt.append(X.words_of_bits(want).reshape(n * Ho * Wo, -1))
            cur, shape, prev = torch.cat(nxt), (N, C, Ho, Wo), blk
            continue
        assert isinstance(blk, FusedConvPoolBnSign), type(blk)
        conv = convs[ci]
        Cout = conv.out_channels
        kh = conv.kernel_size[0]
        (s, _), (p, _) = conv.stride, conv.padding
        pk, ps = blk._pool.pool_k, blk._pool.pool_s
        alpha, beta = fold_batchnorm(blk.bn)
        with torch.no_grad():
            out = traced(lambda: blk(x if ci == 0 else _as_input(cur, shape, prev)), kernels[ci], f"{case} block {bi}")
        record(kernels[ci], f"{case} block {bi}")
        Ho = (H + 2 * p - kh) // s + 1
        Hq = (Ho - pk) // ps + 1
        o = _act_out(out)
        wq = conv.weight.detach()
        nxt, flips, worst, total = [], 0, 0.0, 0
        step = X.image_chunk(X.conv_bytes_per_image(C, H, W, Cout, kh, s, p))
        for n0 in range(0, N, step):
            n = min(N, n0 + step) - n0
            idx = torch.arange(n0, n0 + n, device=dev)
            got = o.bits(idx, Cout)
            if ci == 0:
                y = X.conv64(x[n0:n0 + n], wq, s, p) + conv.bias.detach().double().view(1, -1, 1, 1)
                if pk != 1 or ps != 1:
                    y = F.max_pool2d(y, pk, ps)
                v64 = (y * alpha.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
                f, wr = X.tie_flips(got, v64)
                flips, worst, total = flips + f, max(worst, wr), total + got.numel()
                want = v64 < 0
            else:
                acc = X.exact_conv(X.pm1_nchw(cur.view(N, H * W, -1)[n0:n0 + n].reshape(n * H * W, -1), n, H, W, C), wq, s, p)
                if pk != 1 or ps != 1:
                    acc = F.max_pool2d(acc, pk, ps)
                want, v = X.predicate(acc, conv.bias.detach(), alpha, beta)
                want, v, acc = want.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1), acc.permute(0, 2, 3, 1)
                msg = X.mismatch_report(got, want, acc, v, images=list(range(n0, n0 + n)),
                                        what=f"{case} block {bi} ({C}->{Cout} @ {H})")
                assert not msg, msg
            nxt.append(X.words_of_bits(want).reshape(-1, X.packed_ld(Cout)))
        if ci == 0:
            assert flips <= 1e-4 * total and worst <= 1e-5, (case, "first layer", flips, total, worst)
        cur, shape, prev, ci = torch.cat(nxt), (N, Cout, Hq, Hq), blk, ci + 1
    assert ci == len(convs)


def test_c5_fused_vgg16_layerwise_at_batch_256(dev):
    """Config C5's features at 3 x 224 x 224, 256 images: every fused block (first3x3, the direct 3x3 kernels, the implicit
    threshold convs, the pools on bits, nibble hand-overs) against the exact reference chain."""
    import bench_models
    from pytorch_quantize_impls_amd import _lib
    from pytorch_quantize_impls_amd.layers import FusedFeatureClassifier, TerConv2d
    torch.manual_seed(5)
    model = bench_models.TernaryVGG16(num_classes=10, image=224, fc=64)
    gen = torch.Generator().manual_seed(8)
    for m in model.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            m.weight.data.copy_(torch.empty_like(m.weight).uniform_(-1.2, 1.2, generator=gen))
            if m.bias is not None:
                m.bias.data.copy_(torch.randn(m.bias.shape, generator=gen))
    bench_models.randomize_bn(model, seed=5)
    model = model.to(dev).to(memory_format=torch.channels_last).eval()
    model.features[0].binary_input = False
    fused = FusedFeatureClassifier(model.features, model.classifier, (512, 7, 7))
    blocks = list(fused.features.children())
    convs = [m for m in model.features if isinstance(m, TerConv2d)]
    x = torch.randn(BATCH, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    before = dict(_lib.call_counts)
    kernels = (["first3x3_kernel", "direct3x3<2,2,1,3,lean>", "direct3x3<2,4,1,2,lean>", "direct3x3<4,2,2,2,lean>",
                "ConvV128x2<ElemFp4T>"] + ["ConvVPP256<ElemFp4T>"] * 8)
    _chain(dev, blocks, convs, x, "vgg16", kernels)
    used = {k: v - before.get(k, 0) for k, v in _lib.call_counts.items() if v - before.get(k, 0)}
    # conv1_1: the one-pass first-layer kernel; conv1_2 .. conv2_2: the direct 3 x 3 kernel; conv3_1 .. conv5_3: the implicit GEMM
    assert used.get("qt_conv3x3_first_f32", 0) >= 1 and used.get("qt_conv3x3_direct_nib", 0) >= 3, used
    assert used.get("qt_conv2d_implicit_bits", 0) + used.get("qt_conv2d_implicit_nib", 0) >= 9, used


def test_c3_fused_alexnet_layerwise_at_batch_256(dev):
    """Config C3's features (AlexNet-Bin, 256 images of 3 x 224 x 224): conv -> MaxPool -> BatchNorm -> sign blocks as threshold
    bits + pooling on bits, one by one against the exact reference chain."""
    import bench_models
    from pytorch_quantize_impls_amd.layers import BinConv2d
    torch.manual_seed(6)
    model = bench_models.AlexNetBin()
    bench_models.randomize_bn(model, seed=6)
    model = model.to(dev).to(memory_format=torch.channels_last).eval()
    fusedm = bench_models.FusedAlexNetBin(model)
    blocks = list(fusedm.net.features.children())
    convs = [m for m in model.features if isinstance(m, BinConv2d)]
    x = torch.randn(BATCH, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    kernels = ["conv_first_direct_kernel", "ConvVPP192<ElemFp4T>", "ConvVPP256x192<ElemFp4T>", "ConvVPP256<ElemFp4T>",
               "ConvVPP256<ElemFp4T>"]
    _chain(dev, blocks, convs, x, "alexnet", kernels)


# ---- coverage: every threshold-epilogue configuration ran against the exact reference ---------------------------------------

# configurations the dispatcher (csrc/tile_select.h select_conv, default switches, fp4 threshold epilogue on an un-padded or
# physically padded plane) can select, and the direct kernel's instances
EXPECTED = sorted(
    [f"{c}<ElemFp4>" for c in ("ConvVSkinny", "ConvV128x128D", "ConvV128x64D", "ConvV128x2", "ConvVPP192", "ConvVPP256",
                               "ConvVPP256x192", "ConvV64x2", "ConvV192", "ConvV128", "ConvV64")]
    + [f"{c}<ElemFp4T>" for c in sorted(SWAPT)]
    + [f"direct3x3<{i},{e}>" for i in ("2,2,1,3", "2,4,1,2", "4,1,2,2", "4,2,2,2") for e in ("lean", "general")])
# not selectable with default switches (documented rather than listed):
#   ConvV256      tn == 256 always takes ConvVPP256 first (the `g_conv_force != 1` ping-pong branch; only variant 1 reaches it)
#   ConvV128x128 / ConvV128x64   only with ops.CONV_NO_DEEP_RING (the round-4 double-buffered A/B configurations)


def test_every_threshold_conv_configuration_ran_against_the_exact_reference():
    if not COVERED:
        pytest.skip("run the whole module: the cases above record the configurations they compared")
    missing = [c for c in EXPECTED if c not in COVERED]
    lines = [f"{c}: {', '.join(COVERED.get(c, ['-'])[:4])}" for c in EXPECTED]
    print("\n".join(["threshold-epilogue configurations exercised:"] + lines))
    print(f"peak device memory of a case: {max(PEAK.values()) / 2**30:.2f} GiB ({max(PEAK, key=PEAK.get)})")
    assert not missing, missing
