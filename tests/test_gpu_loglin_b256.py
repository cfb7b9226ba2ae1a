"""The Lin / Log level chain and the family's gradients at the shapes of the batch-256 VGG16-style net, against references that
share no code with the kernels: tests/_levels_exact.py (quantisers restated from the reference's formulas, float64 conv on
operands whose sums are exact in fp32, torch's own BatchNorm / ReLU) and the float64 contractions of tests/_grad_exact.py.
Every comparison is bit equality; the one tolerance is the log-tie rule of _levels_exact (an element whose log2 sits within
2^-18 of a half-integer may take either adjacent level; at most 1e-4 of a case's elements may be such ties).  Each case prints
its tie count.

  (a) qt_conv2d_implicit_levels on every tile configuration conv_implicit_impl can choose for the level element, one case of
      whole tiles and one ragged in M and N each, on an output plane pre-filled with a bf16 NaN pattern: interior, pad channels
      and halo are compared.  Each case asserts the kernel instance the profiler saw.  Output halo, ReLU, bias, BatchNorm
      memory format, quantiser and operand kind vary over the cases so that each value occurs on both dispatch sides
      (test_level_cases_vary_every_parameter_on_both_sides).  The input halo cannot vary on the bounds-checked side: a plane
      with a halo is either taken by the un-padded kernels or refused (conv_prepare), so there it is always 0; on the halo /
      un-padded side it is 0 (a conv without padding), the padding, or more.  Configurations the level element cannot reach:
      ConvV256 (ConvVPP256 takes every 256-wide un-padded case first), ConvV128x128 / ConvV128x64 (only with the deep ring
      switched off by an environment variable), ConvPP128 / ConvPP64 and the Stamps tiles (variant arguments the level entry
      point does not have).  The ragged large-M cases run 13 x 11 maps with an output halo: the magic-number division of the
      halo row index beyond m = 2^15; two cases have stride 2; the three-term image plane runs on Conv64, as the first layer of
      the batch-256 net does.
  (b) QuantConv2d / LinearQuant on tagged quantised activations, y, grad_x, grad_W and the bias gradient against float64, for
      the six conv and three linear shapes of _VGGLinLog(width=64), Lin and Log.  At the default byte budget a batch of 256
      is one chunk of the weight-gradient plan for every layer, so no batch shows the chunked accumulation there: the cases
      run 249 images under a budget lowered until the plan cuts them into 125 + 124 (two chunks, a ragged last one), which is
      also a batch at which the dispatcher picks the tiles of batch 256 — the coverage test asserts that by kernel label.  The
      first conv runs once more on a real-valued image (nine significant bits, 52 images: its three-term route in the step).
  (c) qt_pool_levels_bf16 and qt_bn_relu_linlog_bf16_f32 on more than 2048 * 256 sixteen-byte words (their grid-stride loops
      take a second pass), channel counts off the 8-channel word, the scalar load path of the rows pass.
  (d) layers.fused.device_bn_fold / device_bn_fold_rows: the restated fma with the fold's values against F.batch_norm on
      tensors of the full activation shapes of the batch-256 net, both memory formats.
  (e) one eval forward under lazy.levels_deferred() and one training step of _VGGLinLog(width=64) at batch 256, Lin and Log:
      every kernel instance of the project's own kernels was compared by a case above, or is named in KNOWN_UNCOVERED with
      the test that checks it.

Run the whole module: the coverage test reads what the cases before it recorded and prints the module's peak device memory
(89 cases; 2.1 GiB and 9 s measured on an MI355X, the slowest case 0.2 s after the first one's warm-up)."""
import re

import pytest
import torch
import torch.nn.functional as F

import _grad_exact as G
import _levels_exact as L

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib, lazy, ops  # noqa: E402
from pytorch_quantize_impls_amd.functions import _fused, log_lin_connect  # noqa: E402
from pytorch_quantize_impls_amd.layers import FusedBnLogLinQuant, LinearQuant, QuantConv2d  # noqa: E402
from pytorch_quantize_impls_amd.layers import fused as fused_mod  # noqa: E402
from test_gpu_grad_b256 import kernel_label, profiled  # noqa: E402,F401
import _routes as R  # noqa: E402
from test_gpu_loglin_train import _VGGLinLog, _our_kernel_names  # noqa: E402

BATCH = 256
ACT_QUANTS = (("lin", 1, 3, False), ("lin", 1, 8, False), ("log", 1, 3, True), ("lin", 2, 8, True), ("log", 2, 3, False))
PEAK = {}                   # test id -> peak device memory (bytes); reported by the coverage test
COVERED = {}                # kernel instance -> cases that compared its output here


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    assert _lib.device_info()[0].startswith("gfx950")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_memory(request):
    if not torch.cuda.is_available():
        yield
        return
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    PEAK[request.node.name] = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()


def _record(kernels, case):
    for k in kernels:
        COVERED.setdefault(k, []).append(case)


# ---- (a) the level epilogue, tile configuration by tile configuration --------------------------------------------------------------

# the configurations the level epilogue is walked over (tuple <-> name: tests/_routes.py)
CFG = {c: R.CFG_ARGS[c] for c in (
    "ConvVSkinny", "ConvV128x64D", "ConvV128x128D", "ConvV128x2", "ConvV64x2", "ConvVPP256", "ConvVPP256x192", "ConvVPP192", "ConvV192",
    "ConvV128", "ConvV64", "ConvSkinny", "Conv128x128", "ConvPP192", "ConvPP256", "ConvPP256x192", "Conv256", "Conv192", "Conv128", "Conv64")}
_tile = R.tile_of


def _instance(cfg):
    return f"mfma_gemm_kernel<GemmCfg<ElemBf16L, {CFG[cfg]}>, false>"


# (configuration, Cin, Cout, images, output map, stride); 3 x 3 kernels.  "whole": Cout a multiple of the tile width (and of 4),
# M = images x map a multiple of the tile height; "ragged": neither.  The batch is the smallest that reaches the configuration
# with these channels (the dispatcher's thresholds are in M = images x map, Cout, the K bytes per im2col row and the weight row
# stride, a multiple of 512 bytes for Cin = 256 only).
HALO_SIDE = [
    ("ConvVSkinny", 256, 64, 3, (16, 16), 1), ("ConvVSkinny", 256, 58, 3, (13, 11), 1),
    ("ConvV128x64D", 256, 512, 16, (16, 16), 1),            # 32 x 8 tiles: also the super-tile order
    ("ConvV128x64D", 256, 506, 22, (13, 11), 1),
    ("ConvV128x128D", 128, 256, 50, (16, 16), 1),           # through the small-grid rule (weight rows not a multiple of 512 bytes)
    ("ConvV128x128D", 256, 256, 50, (16, 16), 1),           # through the long-K rule
    ("ConvV128x128D", 128, 250, 89, (13, 11), 1), ("ConvV128x128D", 256, 250, 89, (13, 11), 1),
    ("ConvV128x2", 32, 128, 3, (16, 16), 1), ("ConvV128x2", 32, 256, 3, (16, 16), 1), ("ConvV128x2", 32, 250, 3, (13, 11), 1),
    ("ConvV64x2", 32, 64, 3, (16, 16), 1), ("ConvV64x2", 32, 58, 3, (13, 11), 1),
    ("ConvVPP256", 64, 256, 3, (16, 16), 1), ("ConvVPP256", 64, 250, 3, (13, 11), 1),
    ("ConvVPP256x192", 128, 192, 3, (16, 16), 1), ("ConvVPP256x192", 128, 186, 3, (13, 11), 1),
    ("ConvVPP192", 64, 384, 129, (16, 16), 1), ("ConvVPP192", 64, 378, 230, (13, 11), 1),
    ("ConvV192", 64, 192, 3, (16, 16), 1), ("ConvV192", 64, 186, 3, (13, 11), 1),
    ("ConvV128", 64, 128, 3, (16, 16), 1), ("ConvV128", 64, 122, 5, (8, 7), 2),            # stride 2: 15 x 13 -> 8 x 7
    ("ConvV64", 64, 64, 3, (16, 16), 1), ("ConvV64", 64, 58, 3, (13, 11), 1),
]
PADDED_SIDE = [
    ("ConvSkinny", 256, 64, 3, (16, 16), 1), ("ConvSkinny", 256, 58, 3, (13, 11), 1),
    ("Conv128x128", 64, 128, 3, (16, 16), 1), ("Conv128x128", 64, 122, 3, (8, 7), 2),
    ("ConvPP192", 64, 384, 129, (16, 16), 1), ("ConvPP192", 64, 378, 230, (13, 11), 1),
    ("ConvPP256", 128, 512, 100, (16, 16), 1), ("ConvPP256", 128, 506, 178, (13, 11), 1),
    ("ConvPP256x192", 128, 576, 67, (16, 16), 1), ("ConvPP256x192", 128, 570, 119, (13, 11), 1),
    ("Conv256", 64, 512, 100, (16, 16), 1), ("Conv256", 64, 506, 178, (13, 11), 1),
    ("Conv192", 64, 576, 67, (16, 16), 1), ("Conv192", 64, 570, 119, (13, 11), 1),
    ("Conv128", 64, 640, 40, (16, 16), 1), ("Conv128", 64, 634, 70, (13, 11), 1),
    ("Conv64", 64, 320, 40, (16, 16), 1), ("Conv64", 64, 314, 70, (13, 11), 1),
    ("Conv64", 3, 320, 40, (16, 16), 1), ("Conv64", 3, 314, 70, (13, 11), 1),           # the three-term image plane
]


def _level_cases():
    """(id, configuration, side, Cin, Cout, images, output map, stride, operand kind, quantiser, relu, bias, channels-last BatchNorm,
    input halo or None = a conv without padding, output halo).  The parameters advance with strides of their own over the running
    number of each side; the large-M 13 x 11 cases always carry an output halo."""
    cases = []
    for side, table in (("halo", HALO_SIDE), ("padded", PADDED_SIDE)):
        for i, (cfg, cin, cout, n, hw, s) in enumerate(table):
            kind = "image" if cin == 3 else ("lin", "log")[(i // 2 + i // 5) % 2]
            spec = ACT_QUANTS[(i + i // 5) % 5]
            relu, bias, cl = bool((i // 2 + i // 3) % 2), bool((i + i // 4) % 2), bool((i // 3) % 2)
            out_halo = 1 if (n * hw[0] * hw[1] > (1 << 15) and hw == (13, 11)) else (i + i // 2) % 2
            in_halo = 0
            if side == "halo":
                in_halo = (None, 1, 2)[i % 3] if s == 1 else 1
            cid = f"{cfg}-{cin}x{cout}-n{n}-{hw[0]}x{hw[1]}" + ("-s2" if s == 2 else "")
            cases.append((cid, cfg, side, cin, cout, n, hw, s, kind, spec, relu, bias, cl, in_halo, out_halo))
    return cases


LEVEL_CASES = _level_cases()


def test_level_cases_vary_every_parameter_on_both_sides():
    assert {c[1] for c in LEVEL_CASES} == set(CFG)
    for cfg in CFG:
        kinds = set()
        for c in LEVEL_CASES:
            if c[1] == cfg:
                tm, tn = _tile(cfg)
                m = c[5] * c[6][0] * c[6][1]
                whole = m % tm == 0 and c[4] % tn == 0 and c[4] % 4 == 0
                ragged = m % tm != 0 and c[4] % tn != 0 and m > tm
                assert whole or ragged, c[0]
                kinds.add(whole)
        assert kinds == {True, False}, cfg
    for side in ("halo", "padded"):
        mine = [c for c in LEVEL_CASES if c[2] == side]
        assert {c[8] for c in mine} >= {"lin", "log"}
        assert {c[9] for c in mine} == set(ACT_QUANTS)
        for col in (10, 11, 12):
            assert {c[col] for c in mine} == {True, False}, (side, col)
        assert {c[14] for c in mine} == {0, 1}
        assert {c[13] for c in mine} == ({None, 1, 2} if side == "halo" else {0})
    assert any(c[7] == 2 for c in LEVEL_CASES if c[2] == "halo") and any(c[7] == 2 for c in LEVEL_CASES if c[2] == "padded")
    big = [c for c in LEVEL_CASES if c[5] * c[6][0] * c[6][1] > (1 << 15) and c[6] == (13, 11)]
    assert {c[2] for c in big} == {"halo", "padded"} and all(c[14] == 1 for c in big)
    assert ("lin", 1, 8, False) in ACT_QUANTS


def _designed_bn(y, seed):
    """An eval BatchNorm2d whose output for the conv result ``y`` spreads over the quantisers' ranges (a few units around zero)."""
    C, dev = int(y.shape[1]), y.device
    g = torch.Generator().manual_seed(seed)
    sd = float(y.std())
    bn = torch.nn.BatchNorm2d(C).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.5 * sd)
        bn.running_var.copy_((torch.rand(C, generator=g) * 1.5 + 0.25) * sd * sd)
        bn.weight.copy_((torch.rand(C, generator=g) + 0.4) * torch.where(torch.rand(C, generator=g) < 0.2, -1.0, 1.0))
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    return bn


@pytest.mark.parametrize("case", LEVEL_CASES, ids=[c[0] for c in LEVEL_CASES])
def test_level_epilogue_on_its_tile_configuration(dev, case):
    cid, cfg, side, cin, cout, N, (Ho, Wo), s, kind, spec, relu, with_bias, cl, in_halo, out_halo = case
    seed = sum(ord(ch) for ch in cid)
    p = 0 if in_halo is None else 1
    H, W = ((Ho - 1) * s + 3 - 2 * p, (Wo - 1) * s + 3 - 2 * p) if s == 1 else (2 * Ho - 1, 2 * Wo - 1)
    assert ops.conv_out_hw(H, W, 3, 3, s, p, 1) == (Ho, Wo)
    x = L.designed_activation(kind, (N, cin, H, W), seed, dev)
    w = L.designed_weight("log" if kind == "log" else "lin", (cout, cin, 3, 3), seed + 1, dev)
    bias = L.designed_bias(cout, seed + 2, dev) if with_bias else None
    # reference: exact conv, then torch's BatchNorm / ReLU on the device, in the memory format the case names
    y = L.exact_conv_f32(x, w, bias, s, p)
    bn = _designed_bn(y, seed + 3)
    y = y.contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
    with torch.no_grad():
        t = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        if relu:
            t = torch.relu(t)
    # operands of the launch
    ih = (in_halo or 0,) * 2
    if kind == "image":
        pix = ops.split_bf16x3(x.permute(0, 2, 3, 1).contiguous().view(N * H * W, cin), ld_bytes=ops.triple_ld_bytes(cin, 16, 3),
                               terms=3).data
        wt = ops.pack_conv_weight_bf16x3(w, "raw", terms=3)
    else:
        pix = L.encode_plane(x, ih)
        wt = ops.pack_levels_bf16x3(w, "lin", 0, 32, True, grad_x=False, fwd_terms=1)[0]      # the levels as they are
    fw, fb, stats = fused_mod.device_bn_fold(bn, (N, cout, Ho, Wo), cl)
    ld = L.plane_ld(cout)
    plane = L.nan_filled(N * (Ho + 2 * out_halo) * (Wo + 2 * out_halo), ld, dev)
    q = ops._level_quant_args(spec)
    I = int

    def launch():
        with ops._on(dev):
            _lib.call("qt_conv2d_implicit_levels", pix.data_ptr(), I(N), I(H), I(W), I(pix.shape[1] // 2), I(ih[0]), I(ih[1]), 3, 3,
                      I(s), I(s), I(p), I(p), 1, 1, wt.data.data_ptr(), I(wt.ld_words), ops._p(bias), fw.data_ptr(), fb.data_ptr(),
                      stats.data_ptr(), int(relu), *q, plane.data_ptr(), I(2 * ld), I(cout), I(out_halo), I(out_halo),
                      ops._stream(dev))

    R.assert_described(ops.conv_kernel_name(2, N, H, W, pix.shape[1] // 2, (3, 3), (s, s), (p, p), (1, 1), wt.ld_words, cout, in_halo=ih,
                                            epilogue=ops.EPI_LEVELS), f"{cfg}<ElemBf16L>", cid)
    _, kernels, calls, lib = profiled(launch)
    assert not lib and calls == {"qt_conv2d_implicit_levels": 1}, (calls, lib)
    ours = sorted(k for k in kernels if k.startswith("mfma_gemm_kernel"))
    assert ours == [_instance(cfg)], f"{cid}: written for {cfg} = {_instance(cfg)}, the dispatcher launched {ours}"
    got = L.decode_plane(plane, (N, cout, Ho, Wo), (out_halo, out_halo), what=cid)       # pad channels and halo are zero
    ties, moved, rep = L.compare_levels(got, t.permute(0, 2, 3, 1), spec, what=cid)
    print(f"\n{cid}: {kind} operands, {spec}, relu={relu} bias={with_bias} channels_last={cl} in_halo={in_halo} out_halo={out_halo}: "
          f"{ties} log ties of {got.numel()} ({moved} on the other level)")
    assert not rep, rep
    _record(kernels, cid)


# ---- (c) the elementwise passes beyond one grid pass -----------------------------------------------------------------------------

@pytest.mark.parametrize("N,C,hw,k,s,halo,spec", [
    (64, 256, (32, 32), 2, 2, (1, 1), ("lin", 1, 8, False)),       # 64 * 18 * 18 * 32 words > 2048 * 256: a second grid pass
    (100, 130, (33, 31), 3, 2, (2, 1), ("log", 1, 3, True)),       # 100 * 20 * 17 * 17 words; 130 channels: a word with 2 of 8 used
    (3, 13, (7, 9), 2, 1, (0, 0), ("lin", 2, 8, True)),
])
def test_pool_levels_beyond_one_grid_pass(dev, N, C, hw, k, s, halo, spec):
    H, W = hw
    g = torch.Generator(device=dev).manual_seed(N + C)
    x = L.quantise(torch.randn((N, C, H, W), generator=g, device=dev) * 1.5, spec)
    x.view(-1)[5::53] = 0.0
    if spec[3]:
        x.view(-1)[7::59] = -0.0
    plane_in = L.encode_plane(x)
    want = F.max_pool2d(x, k, s)
    Ho, Wo = (int(v) for v in want.shape[2:])
    out = L.nan_filled(N * (Ho + 2 * halo[0]) * (Wo + 2 * halo[1]), plane_in.shape[1], dev)
    words = out.numel() // 8
    assert (N < 10) != (words > 2048 * 256)

    def launch():
        with ops._on(dev):
            _lib.call("qt_pool_levels_bf16", plane_in.data_ptr(), int(N), int(H), int(W), int(plane_in.shape[1] * 2), int(k), int(s),
                      out.data_ptr(), int(halo[0]), int(halo[1]), ops._stream(dev))

    _, kernels, calls, _ = profiled(launch)
    assert calls == {"qt_pool_levels_bf16": 1} and "pool_levels_kernel" in kernels, (calls, kernels)
    got = L.decode_plane(out, (N, C, Ho, Wo), halo, what="pooled plane")
    rep = G.mismatch_report(got.view(torch.int32), want.permute(0, 2, 3, 1).contiguous().view(torch.int32), ("n", "y", "x", "c"),
                            what=f"pool {N}x{C}x{H}x{W} k{k}/s{s} (fp32 patterns)")
    assert not rep, rep
    # the wrapper allocates its own plane: the same bytes
    assert torch.equal(ops.pool_levels(ops.TriplePlanes(data=plane_in, rows=N * H * W, K=C, terms=1), N, H, W, k, s, halo).data, out)
    _record(kernels, f"pool {N}x{C}x{H}x{W}")


@pytest.mark.parametrize("rows,C,view,spec,relu", [
    (2100, 2048, False, ("lin", 1, 8, False), True),        # 2100 * 256 words > 2048 * 256
    (2100, 2048, True, ("log", 1, 3, True), False),         # a column view: row stride 2049, base 4 bytes off: the scalar loads
    (2100, 2044, False, ("lin", 2, 8, True), True),         # C % 8 == 4: vector loads and a scalar tail word
    (4200, 1021, False, ("log", 2, 3, False), True),        # C % 4 != 0: scalar loads throughout
    (37, 13, False, ("lin", 1, 3, False), False),
])
def test_bn_relu_quantiser_rows_pass_beyond_one_grid_pass(dev, rows, C, view, spec, relu):
    g = torch.Generator(device=dev).manual_seed(rows + C)
    base = torch.randn((rows, C + (1 if view else 0)), generator=g, device=dev) * 3
    x = base[:, 1:] if view else base
    assert x.stride(1) == 1 and (x.stride(0) % 4 != 0 and x.data_ptr() % 16 != 0) == view
    gc = torch.Generator().manual_seed(C)
    bn = torch.nn.BatchNorm1d(C).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=gc) * 0.7)
        bn.running_var.copy_(torch.rand(C, generator=gc) * 3 + 0.3)
        bn.weight.copy_((torch.rand(C, generator=gc) + 0.4) * torch.where(torch.rand(C, generator=gc) < 0.2, -1.0, 1.0))
        bn.bias.copy_(torch.randn(C, generator=gc) * 0.3)
        t = bn(x)
        if relu:
            t = torch.relu(t)
    w, b, stats, form = fused_mod.device_bn_fold_rows(bn)
    ld = L.plane_ld(C, 128)
    plane = L.nan_filled(rows, ld, dev)
    y = torch.full((rows, C), float("nan"), device=dev)
    assert (rows < 100) != (rows * ld // 8 > 2048 * 256)
    q = ops._level_quant_args(spec)

    def launch():
        with ops._on(dev):
            _lib.call("qt_bn_relu_linlog_bf16_f32", x.data_ptr(), int(x.stride(0)), w.data_ptr(), b.data_ptr(), stats.data_ptr(), int(form),
                      int(relu), *q, y.data_ptr(), int(C), plane.data_ptr(), int(2 * ld), int(rows), int(C), ops._stream(dev))

    _, kernels, calls, _ = profiled(launch)
    assert calls == {"qt_bn_relu_linlog_bf16_f32": 1} and "bn_relu_quant_rows_kernel" in kernels, (calls, kernels)
    got = L.decode_plane(plane, (rows, C), granule=128, what="row plane")
    what = f"rows pass {rows}x{C} view={view} {spec}"
    ties, moved, rep = L.compare_levels(got, t, spec, names=("row", "c"), what=what)
    print(f"\n{what}: {ties} log ties of {got.numel()} ({moved} on the other level)")
    assert not rep, rep
    # the fp32 image holds the same levels (NaN nowhere: every element was written)
    assert torch.equal(y.view(torch.int32) >> 16, got.view(torch.int32) >> 16) and L.bf16_exact(y)
    # the module form on the same input: the same plane
    with torch.no_grad():
        act = FusedBnLogLinQuant(bn, spec, relu=relu)(x)
    assert torch.equal(act.planes.data, plane)
    _record(kernels, what)


# ---- (d) the BatchNorm emulation at the size of the real activation -------------------------------------------------------------

VGG_ACTS = [(64, 32), (64, 32), (128, 16), (128, 16), (256, 8), (256, 8)]          # (channels, map) behind each conv of the net


def _random_bn(bn, seed):
    g = torch.Generator().manual_seed(seed)
    C = bn.num_features
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g) * 4 + 0.5)
        bn.weight.copy_((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.2, -1.0, 1.0))
        bn.bias.copy_(torch.randn(C, generator=g) * 0.2)
    return bn


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("layer", range(6))
def test_bn_fold_equals_batch_norm_at_the_full_activation_shape(dev, layer, channels_last):
    C, hw = VGG_ACTS[layer]
    bn = _random_bn(torch.nn.BatchNorm2d(C).to(dev).eval(), 300 + layer)
    w, b, stats = fused_mod.device_bn_fold(bn, (BATCH, C, hw, hw), channels_last)
    g = torch.Generator(device=dev).manual_seed(400 + layer)
    x = torch.randn((BATCH, C, hw, hw), generator=g, device=dev) * 4
    x[:, :, ::3] *= 23.0
    x = x.contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    with torch.no_grad():
        want = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    mean, rs = stats[:C].view(1, C, 1, 1), stats[C:].view(1, C, 1, 1)
    t32 = torch.mul(torch.sub(x, mean), rs)                       # two fp32 roundings
    got = (t32.double() * w.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1)).float()      # the fma: one rounding
    rep = G.mismatch_report(got, want, ("n", "c", "y", "x"), what=f"BatchNorm2d fold at {tuple(x.shape)}, channels_last={channels_last}")
    assert not rep, rep


@pytest.mark.parametrize("seed", [0, 1])
def test_bn_rows_fold_equals_batch_norm_at_256_rows(dev, seed):
    C = 1024
    bn = _random_bn(torch.nn.BatchNorm1d(C).to(dev).eval(), 500 + seed)
    w, b, stats, form = fused_mod.device_bn_fold_rows(bn)
    g = torch.Generator(device=dev).manual_seed(600 + seed)
    x = torch.randn((BATCH, C), generator=g, device=dev) * 4
    x[::3] *= 23.0
    with torch.no_grad():
        want = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    d = torch.sub(x, stats[:C].view(1, C))
    rs = stats[C:].view(1, C)
    if form == 0:
        got = (torch.mul(d, rs).double() * w.double().view(1, C) + b.double().view(1, C)).float()
    else:
        got = (torch.mul(w.view(1, C), d).double() * rs.double() + b.double().view(1, C)).float()
    rep = G.mismatch_report(got, want, ("row", "c"), what=f"BatchNorm1d fold (form {form}) at {tuple(x.shape)}")
    assert not rep, rep


# ---- (b) the plain one-term conv, LinearQuant and their gradients at the route of batch 256 ------------------------------------------

# activations / weights whose products are integers of 2^-5 (tests/test_gpu_loglin_act.py EXACT): the forward sums stay below
# 256 * 9 * 256 (convs) and 4096 * 256 (linears) units, under 2^24; the gradients are -1 / 0 / +1 times a power of two, and
# proves_exact checks the actual tensors of every backward contraction first.
EXACT = {"lin": dict(act=("lin", 1, 4, False), w=(2, 4)), "log": dict(act=("log", 1, 2, True), w=(2, 2))}
RAGGED = 249                                                     # 125 + 124 under the lowered budget
# the real image of the first layer: its weight gradient sums |x| < 4 in units of 2^-7 over every pixel of the batch, which stays
# below 2^24 units up to about 90 images (proves_exact decides); from 50 images on the forward runs the tile of batch 256
IMAGE_BATCH = 52
VGG_CONVS = [(3, 64, 32), (64, 64, 32), (64, 128, 16), (128, 128, 16), (128, 256, 8), (256, 256, 8)]
VGG_LINS = [(4096, 1024), (1024, 1024), (1024, 10)]
ONE_TERM_PACKS = ("qt_bf16x1_pack_conv_levels_f32", "qt_bf16x1_pack_levels_f32")
THREE_TERM_SPLITS = ("qt_bf16x3_pack_f32", "qt_bf16x6_pack_f32")


def _check(got, want, what, names):
    rep = G.mismatch_report(got, want, names, what=what)
    assert not rep, rep


def _prove(a, b, contract, what, split="bf16x3", split_b=None):
    ok, why = G.proves_exact(a, b, contract, split, split_b=split_b)
    assert ok, f"{what}: the designed operands are not exact ({why})"


@pytest.fixture()
def two_ragged_chunks():
    prev = ops.WGRAD_GEMM_BYTES
    try:
        yield
    finally:
        ops.WGRAD_GEMM_BYTES = prev


def _budget_for_two_chunks(N, Cout, Cin, H):
    """The largest budget (in steps of 1/8) under which the pixel-major plan cuts N images into ceil(N / 2) + the rest."""
    half = (N + 1) // 2
    budget = 1 << 20
    while True:
        ops.WGRAD_GEMM_BYTES = budget
        if ops.wgrad_pm_plan(half, Cout, Cin, H, H, H, 3, 3, 1, 1, ops.WGRAD_PM_WORKGROUPS)[0]:
            break
        budget += budget // 8
    nc = ops.wgrad_chunk_images(N, lambda n: ops.wgrad_pm_plan(n, Cout, Cin, H, H, H, 3, 3, 1, 1, ops.WGRAD_PM_WORKGROUPS)[0])
    assert nc == half and N % nc, (N, nc, budget)
    return budget


def _conv_case(dev, layer, kind, image=False):
    Cin, Cout, H = VGG_CONVS[layer]
    N = IMAGE_BATCH if image else RAGGED
    what = f"QuantConv2d {Cin}->{Cout} at {H}x{H}, {kind}, batch {N}" + (", real image" if image else "")
    torch.manual_seed(700 + layer)
    fsr, bits = EXACT[kind]["w"]
    conv = QuantConv2d(Cin, Cout, 3, padding=1, fsr=fsr, bit_width=bits, dtype=kind).to(dev)
    with torch.no_grad():
        conv.bias.copy_(L.designed_bias(Cout, 710 + layer, dev))
    q = log_lin_connect.nnQuant(*EXACT[kind]["act"][:3], with_sign=EXACT[kind]["act"][3])
    if image:       # k 2^-7, |k| < 512: nine significant bits, not a bf16 value -> the three-term route of the step's first conv
        r = (G.int_uniform((N, Cin, H, H), -511, 511, 730 + layer, dev, channels_last=False) * 2.0 ** -7).requires_grad_(True)
        assert not G.exact_in(r, torch.bfloat16)
    else:
        r = (torch.randn((N, Cin, H, H), device=dev) * 1.5).requires_grad_(True)
    gout = G.grad_ints((N, Cout, H, H), 1, 720 + layer, dev, exp=-4, channels_last=False)
    pm = ops.wgrad_pm_applicable((N, Cin, H, H), (N, Cout, H, H), (3, 3), 1, 1)
    if pm:
        _budget_for_two_chunks(N, Cout, Cin, H)

    def run():
        x = r if image else q(r)
        y = conv(x)
        fwd.update(_lib.call_counts)
        y.backward(gout)
        return x.detach(), y.detach()

    before, fwd = dict(_lib.call_counts), {}
    (x, y), kernels, calls, lib = profiled(run)
    assert not lib, f"{what}: dense-library paths taken: {lib}"
    if image:
        assert calls.get("qt_bf16x3_pack_conv_levels_f32") == 1 and not calls.get("qt_bf16x1_pack_conv_levels_f32"), calls
    else:
        assert calls.get("qt_bf16x1_pack_conv_levels_f32") == 1, calls
        # no split of the activation: not in the forward at all (the backward splits the gradient)
        assert not any(fwd.get(e, 0) - before.get(e, 0) for e in THREE_TERM_SPLITS), (calls, fwd)
    assert not calls.get("qt_bf16x6_pack_f32"), calls                  # no six-term operand anywhere
    if pm:
        assert calls.get("qt_wgrad_pm_f32") == 2 and calls.get("qt_wgrad_pm_reduce_f32") == 2, calls       # two chunks
        assert calls.get("qt_wgrad_pm_pack_act_f32") == 2, calls
    wq = conv.weight_op.forward(conv.weight.detach())
    L.assert_exact_bound(x, wq, conv.bias.detach(), what)
    _check(y, L.exact_conv_f32(x, wq, conv.bias.detach(), 1, 1), what + " y", ("n", "c", "y", "x"))
    _prove(gout, wq, lambda a, b: G.conv_grad_input64(a, b, (H, H), 1, 1), what + " grad_x")
    _check(r.grad, G.to_f32_exact(G.conv_grad_input64(gout, wq, (H, H), 1, 1)), what + " grad_x", ("n", "c", "y", "x"))
    split = None if pm else ops.current_float_split()       # the three-channel layer: the space-to-depth form splits both operands
    _prove(gout, x, lambda a, b: G.conv_grad_weight64(b, a, 3, 1, 1), what + " grad_W", split=split or "bf16x3", split_b=split)
    # exact partial sums: the chunked fp32 accumulation adds exact values whose total is exact too
    _check(conv.weight.grad, G.to_f32_exact(G.conv_grad_weight64(x, gout, 3, 1, 1)), what + " grad_W", ("co", "ci", "ky", "kx"))
    _check(conv.bias.grad, G.to_f32_exact(G.bias_grad64(gout)), what + " bias", ("c",))
    _record(kernels, what)


@pytest.mark.parametrize("kind", ["lin", "log"])
@pytest.mark.parametrize("layer", range(6))
def test_conv_and_gradients_at_the_batch_256_route(dev, two_ragged_chunks, layer, kind):
    _conv_case(dev, layer, kind)


@pytest.mark.parametrize("kind", ["lin", "log"])
def test_first_conv_on_a_real_image_at_the_batch_256_route(dev, two_ragged_chunks, kind):
    """The first layer as the training step runs it: the image is real-valued, so weight and activation enter as three terms."""
    _conv_case(dev, 0, kind, image=True)


@pytest.mark.parametrize("kind", ["lin", "log"])
@pytest.mark.parametrize("layer", range(3))
def test_linear_and_gradients_at_the_batch_256_route(dev, layer, kind):
    K, Nf = VGG_LINS[layer]
    N = BATCH
    what = f"LinearQuant {K}->{Nf}, {kind}, batch {N}"
    torch.manual_seed(800 + layer)
    fsr, bits = EXACT[kind]["w"]
    lin = LinearQuant(K, Nf, True, dtype=kind, fsr=fsr, bit_width=bits).to(dev)
    with torch.no_grad():
        lin.bias.copy_(L.designed_bias(Nf, 810 + layer, dev))
    q = log_lin_connect.nnQuant(*EXACT[kind]["act"][:3], with_sign=EXACT[kind]["act"][3])
    r = (torch.randn((N, K), device=dev) * 1.5).requires_grad_(True)
    gout = G.grad_ints((N, Nf), 2, 820 + layer, dev, exp=-4)

    def run():
        x = q(r)
        y = lin(x)
        fwd.update(_lib.call_counts)
        y.backward(gout)
        return x.detach(), y.detach()

    before, fwd = dict(_lib.call_counts), {}
    (x, y), kernels, calls, lib = profiled(run)
    assert not lib, f"{what}: dense-library paths taken: {lib}"
    assert calls.get("qt_bf16x1_pack_levels_f32") == 1, calls
    assert not any(fwd.get(e, 0) - before.get(e, 0) for e in THREE_TERM_SPLITS) and not calls.get("qt_bf16x6_pack_f32"), (calls, fwd)
    wq = lin.weight_op.forward(lin.weight.detach())
    L.assert_exact_bound(x.view(N, K, 1, 1), wq.view(Nf, K, 1, 1), lin.bias.detach(), what)
    y64 = x.double() @ wq.double().t() + lin.bias.detach().double()
    _check(y, G.to_f32_exact(y64), what + " y", ("n", "o"))
    _prove(gout, wq, lambda a, b: a @ b, what + " grad_x")
    _check(r.grad, G.to_f32_exact(G.linear_grad_x64(gout, wq)), what + " grad_x", ("n", "i"))
    _prove(gout.t(), x, lambda a, b: a @ b, what + " grad_W")
    _check(lin.weight.grad, G.to_f32_exact(G.linear_grad_w64(gout, x)), what + " grad_W", ("o", "i"))
    _check(lin.bias.grad, G.to_f32_exact(G.bias_grad64(gout)), what + " bias", ("o",))
    _record(kernels, what)


# ---- (e) coverage -----------------------------------------------------------------------------------------------------------------

# kernels of the forward / the step that this module does not compare, each with where it is checked instead
KNOWN_UNCOVERED = []


def _vgg_kernels(dev, dtype, bits):
    torch.manual_seed(3)
    model = _VGGLinLog(dtype, bits, 64).to(dev)
    x, t = torch.randn((BATCH, 3, 32, 32), device=dev), torch.randint(0, 10, (BATCH,), device=dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)

    def step():
        opt.zero_grad()
        F.nll_loss(model(x), t).backward()
        opt.step()
        model.clamp()

    step()                                                     # warm-up: plans, detection verdicts
    _, k_step, _, lib_step = profiled(step)
    model.eval()
    with torch.no_grad(), lazy.levels_deferred():
        model(x)
        _, k_fwd, calls, lib_fwd = profiled(lambda: model(x))
    assert calls.get("qt_conv2d_implicit_levels") == 6, calls
    return k_fwd, k_step, {**lib_step, **lib_fwd}


def test_every_kernel_of_the_forward_and_the_step_was_compared(dev):
    ours = _our_kernel_names()
    known = {k: why for k, why in KNOWN_UNCOVERED}
    report, missing = [], {}
    for dtype, bits in (("lin", 8), ("log", 3)):
        k_fwd, k_step, lib = _vgg_kernels(dev, dtype, bits)
        assert not lib, f"{dtype}: dense-library paths: {lib}"
        for name, kernels in ((f"{dtype} eval forward", k_fwd), (f"{dtype} training step", k_step)):
            for k in sorted(kernels):
                if re.match(r"(?:\w+::)*(\w+)", k).group(1) not in ours:
                    continue                                   # torch's own kernels
                if k in COVERED:
                    report.append(f"  {name}: {k} <- {COVERED[k][0]}")
                elif any(re.search(p, k) for p in known):
                    report.append(f"  {name}: {k} NOT compared here ({next(w for p, w in known.items() if re.search(p, k))})")
                else:
                    missing.setdefault(k, []).append(name)
    worst = max(PEAK.items(), key=lambda kv: kv[1]) if PEAK else ("-", 0)
    print("\nkernels of the batch-256 Lin / Log forward and training step:\n" + "\n".join(report)
          + f"\npeak device memory of the module: {worst[1] / 2**30:.2f} GiB ({worst[0]})")
    assert not missing, "kernels of the batch-256 forward / step that no case compared:\n" + "\n".join(
        f"  {k}  ({', '.join(v)})" for k, v in sorted(missing.items()))
