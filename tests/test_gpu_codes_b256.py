"""The DoReFa int8 code chain (config C4: ResNet-18 W1A4) kernel by kernel against the exact reference of tests/_codes_exact.py:
float64 integer sums and the code epilogue with one correctly rounded fp32 result per kernel operation.  Every output byte is
compared — codes, halo border, pad bytes — and the int8 range flag.

  (a) qt_conv2d_implicit_codes (mode 2 of csrc/mfma_gemm_kernel.h) on the C4 net's own launches, one case per tile route, under
      ops.CONV_NO_DIRECT_CODES and, where that changes the configuration, ops.CONV_NO_DEEP_RING; the 1 x 1 stride-2 shortcut convs
      (BatchNorm epilogue, fp32 out) hand their result to the main conv as res_f32;
  (b) the epilogue's forms at one shape per tile family: fast / general branch, device / folded BatchNorm, residual kinds, halos,
      ReLU placements, bit widths, conv bias, scale_dev, Cout % 32 != 0 and Cout % 4 != 0, the edge channels (NaN, inf, huge);
  (c) the persistent direct 3 x 3 kernel (csrc/code_conv3x3.hip): both loader modes, the whole walk (>= 3 tiles per workgroup,
      ragged tile counts), W = 4 .. 128, RT < H / == H / > H, halos;
  (d) the chain's other kernels (csrc/codes_i8.hip): head, code pool, decode;
  (e) the fused C4 net block by block at batch 256, each block fed the reference chain's code plane;
  (f) every configuration the dispatcher describes for the launches of (e), with and without the two switches, and both direct
      kernel instances, ran against the reference in this module.

"Designed" cases use operands for which every step is exact (tests/test_codes_exact_cpu.py pins that and their share of exact
ties): zero differing bytes.  "Realistic" cases use BatchNorm statistics like bench_models.randomize_bn: a differing element passes
only if the kernel's code is one the reference itself cannot rule out (an fma whose float64 sum is an fp32 midpoint), at most one
per million elements of a case.

Run the whole module: the coverage test reads what the cases before it recorded."""
import time

import pytest
import torch
import torch.nn.functional as F

import _codes_exact as CX
import _exact as X
import _routes as R

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import ops  # noqa: E402

BATCH = 256
BUDGET = 1 << 30            # bytes of float64 temporaries per reference chunk
COVERED = {}                # route label -> case ids that compared it with the exact reference
PEAK = {}                   # test id -> peak device memory (bytes)
TOTALS = {"cases": 0, "designed_bytes_differing": 0, "waived": 0, "elements": 0, "t0": None}
NO_DIRECT, NO_RING = ops.CONV_NO_DIRECT_CODES, ops.CONV_NO_DEEP_RING


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    if TOTALS["t0"] is None:
        TOTALS["t0"] = time.time()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    PEAK[request.node.name] = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()


def routes(names):
    """Profiler kernel names -> labels 'ConvV128x64D<ElemI8>', 'code_conv3x3<64,0>'."""
    names = [k.replace("(anonymous namespace)::", "") for k in names]
    return R.mfma_routes(names, elem="ElemI8") | R.code_conv3x3_routes(names)


def traced(fn, expect, case, described=None):
    """Run fn under torch.profiler; the kernel ``expect`` (a label of routes()) ran, and the describe entry point names it."""
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


def launch_count():
    from pytorch_quantize_impls_amd import _lib
    return int(_lib.load().qt_code_conv3x3_launch_count())


# ---- operands and the comparison ---------------------------------------------------------------------------------------------

def planes(q, halo, inv_n, bits):
    """Integer codes [N, C, H, W] -> ops.CodePlanes of the halo plane."""
    N, C, H, W = (int(v) for v in q.shape)
    codes = CX.encode_plane(q, halo, CX.code_ld(C))
    return ops.CodePlanes(codes=codes, rows=int(codes.shape[0]), K=C, inv_n=float(inv_n), bit_width=int(bits))


def input_codes(N, C, H, W, designed, seed, dev, image_rows=False):
    """Codes uniform in 0..3 (designed) or 0..15; ``image_rows``: the top and bottom row of image n hold the constant 1 + n % 3, so a
    row taken from a neighbouring image changes the sum."""
    q = CX.random_codes((N, C, H, W), 0, 3 if designed else 15, seed, dev)
    if image_rows:
        c = (1 + torch.arange(N, device=dev) % 3).view(N, 1, 1)
        q[:, :, 0, :] = c
        q[:, :, H - 1, :] = c
    return q


class Params:
    """The operands of one conv case, for the kernel and for the reference."""

    def __init__(self, dev, Cin, Cout, k, designed, form="device", bits=4, seed=1, use_scale_dev=None, conv_bias=False, edges=False):
        self.designed, self.form, self.bits, self.levels = designed, form, bits, float((1 << bits) - 1)
        self.w_int = CX.pm1_weights(Cout, Cin, k, seed + 1, dev)
        K = Cin * k * k
        if designed:
            self.shift = CX.designed_shift(K, self.levels)
            scale, self.alpha, self.beta, self.stats = CX.designed_params(Cout, self.shift, seed + 2, dev, form)
            # scale_dev given instead of scale: 1/4 = 1 * 1/4 (exact either way)
            self.scale, self.scale_dev = (1.0, torch.tensor(scale, device=dev)) if use_scale_dev else (scale, None)
            self.weight = self.w_int
            self.bias = (torch.randint(-8, 9, (Cout,), device=dev, generator=CX._gen(seed + 3, dev)).float() / 4) if conv_bias else None
        else:
            if form == "offset":        # device form with a cancelling offset: the fma's single rounding decides codes
                inv, E, self.alpha, self.beta, self.stats = CX.cancelling_params(Cout, K, seed + 2, dev)
            else:
                inv, E, self.alpha, self.beta, self.stats = CX.realistic_params(Cout, K, seed + 2, dev, form)
            self.scale, self.scale_dev = (inv, E) if use_scale_dev in (None, True) else (float(CX.kernel_scale(inv, E)), None)
            self.weight = self.w_int * E
            self.bias = (torch.randn(Cout, device=dev, generator=CX._gen(seed + 3, dev)) * 0.5) if conv_bias else None
        if edges:
            CX.edge_channels(self.alpha, self.beta, self.stats, self.levels)
        self.kscale = CX.kernel_scale(self.scale, self.scale_dev, dev)
        self.bn_stats = torch.cat([self.stats[0], self.stats[1]]).contiguous() if self.stats is not None else None

    def residual_f32(self, shape, seed, dev):
        g = CX._gen(seed, dev)
        if self.designed:
            return torch.randint(-12, 13, shape, device=dev, generator=g).float() / 4
        return torch.randn(shape, device=dev, generator=g)

    def residual_affine(self, Cout, seed, dev, device_form):
        g = CX._gen(seed, dev)
        if self.designed:
            ra = (torch.randint(0, 2, (Cout,), device=dev, generator=g) * 2 - 1).float() * 2
            rb = torch.randint(-4, 5, (Cout,), device=dev, generator=g).float() / 4
            return (ra, rb, (torch.randint(-4, 5, (Cout,), device=dev, generator=g).float() / 4, torch.full((Cout,), 0.5, device=dev))) \
                if device_form else (ra, rb)
        ra, rb = torch.rand(Cout, device=dev, generator=g) + 0.5, torch.randn(Cout, device=dev, generator=g) * 0.1
        return (ra, rb, (torch.randn(Cout, device=dev, generator=g), torch.rand(Cout, device=dev, generator=g) * 0.5 + 0.25)) \
            if device_form else (ra, rb)


RELU = {False: 0, True: 1, "pre": 2}


def check_plane(got_plane, flag, q_in, P, Epi_of, N, Cout, Ho, Wo, k, stride, out_halo, case, want_flag=None):
    """Every byte of the kernel's plane against the reference, images in chunks under BUDGET; the waiver rule; the range flag.
    ``Epi_of(idx)``: the reference epilogue arguments for the images ``idx`` (residuals sliced)."""
    Cin, H, W = (int(v) for v in q_in.shape[1:])
    got = CX.decode_plane(got_plane, N, Ho, Wo, Cout, out_halo, case).permute(0, 2, 3, 1)       # asserts zero border and pad bytes
    assert got_plane.shape[1] == CX.code_ld(Cout)
    step = X.image_chunk(X.conv_bytes_per_image(Cin, H, W, Cout, k, stride, k // 2), BUDGET)
    waived, ref_flag = 0, False
    for n0 in range(0, N, step):
        idx = slice(n0, min(N, n0 + step))
        acc = CX.exact_acc(q_in[idx], P.w_int, stride, k // 2).permute(0, 2, 3, 1)
        ref = CX.epilogue(CX.conv_value(acc, P.kscale, P.bias), Epi_of(idx))
        w, msg = CX.compare_codes(got[idx], ref, P.designed, acc, images=list(range(n0, n0 + acc.shape[0])), what=case)
        if msg:
            print(msg)
            if P.designed:
                TOTALS["designed_bytes_differing"] += int((got[idx] != ref["codes"]).sum())
        assert not msg, msg
        waived += w
        ref_flag |= ref["flag"]
        del acc, ref
    n = got.numel()
    print(f"{case}: {n} codes compared, {waived} waived (cap {CX.waiver_cap(n)}), flag {int(flag.item())}")
    assert waived <= CX.waiver_cap(n), (case, waived, n)
    assert int(flag.item()) == (1 if ref_flag else 0), (case, "range flag", int(flag.item()), ref_flag)
    if want_flag is not None:
        assert ref_flag == want_flag, (case, "the reference's flag", ref_flag)
    TOTALS["cases"] += 1
    TOTALS["waived"] += waived
    TOTALS["elements"] += n


def conv_case(dev, case, N, Cin, Cout, H, W=None, k=3, stride=1, designed=True, form="device", relu=True, bits=4, in_halo=(1, 1),
              out_halo=(1, 1), res=None, res_halo=(0, 0), conv_bias=False, use_scale_dev=None, flags=NO_DIRECT, expect=None,
              direct=None, edges=False, want_flag=None, seed=1, image_rows=False, res_f32_given=None):
    """One launch of ops.conv2d_codes with a CodeEpilogue against the reference.  ``res``: None, "codes", "f32", "f32_affine" (folded
    residual BatchNorm) or "f32_bn" (device form: the residual is normalised by ops.bn_eval_device first, as the fused layer does).
    ``expect``: the implicit-GEMM configuration that must run (and be described); ``direct``: 'code_conv3x3<CB,MODE>' instead."""
    W = H if W is None else W
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    P = Params(dev, Cin, Cout, k, designed, form, bits, seed, use_scale_dev, conv_bias, edges)
    q_in = input_codes(N, Cin, H, W, designed, seed, dev, image_rows)
    px = planes(q_in, in_halo, 1.0, bits)
    wc = ops.pack_conv_weight_codes(P.weight)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    epi = ops.CodeEpilogue(P.alpha, P.beta, bits, relu, out_halo=out_halo, bn_stats=P.bn_stats, overflow=flag)
    M = N * Ho * Wo
    r_codes = r_f32 = r_aff = None
    rscale = 0.25 if designed else ops.inv_levels(bits)
    if res == "codes":
        r_codes = CX.random_codes((N, Cout, Ho, Wo), 0, 15, seed + 5, dev)
        epi.res_codes, epi.res_halo = planes(r_codes, res_halo, rscale, bits), res_halo
    elif res is not None:
        r_f32 = P.residual_f32((M, Cout), seed + 6, dev) if res_f32_given is None else res_f32_given
        epi.res_f32 = r_f32
        if res == "f32_affine":
            r_aff = P.residual_affine(Cout, seed + 7, dev, False)
            epi.res_affine = r_aff
        elif res == "f32_bn":
            r_aff = P.residual_affine(Cout, seed + 7, dev, True)
            epi.res_f32 = ops.bn_eval_device(r_f32, r_aff[0], r_aff[1], torch.cat(list(r_aff[2])).contiguous())

    def run():
        return ops.conv2d_codes(px, (N, Cin, H, W), wc, (k, k), P.scale, P.bias, stride, pad, 1, scale_dev=P.scale_dev, epi=epi,
                                in_halo=in_halo)

    label = direct or f"{expect}<ElemI8>"
    described = None
    if direct is None:
        described = ops.conv_kernel_name(1, N, H, W, px.ld_words, (k, k), (stride, stride), (pad, pad), (1, 1), wc.ld_words, Cout,
                                         in_halo=in_halo, epilogue=ops.EPI_CODES, variant=flags)
    c0 = launch_count()
    with ops.scope(CONV_FLAGS=flags):
        out = traced(run, label, case, described)
    assert launch_count() - c0 == (1 if direct else 0), (case, "launches of the direct kernel", launch_count() - c0)
    assert out.overflow is flag and out.rows == N * (Ho + 2 * out_halo[0]) * (Wo + 2 * out_halo[1])

    def epi_of(idx):
        n = len(range(*idx.indices(N)))
        rf = r_f32.view(N, Ho, Wo, Cout)[idx] if r_f32 is not None else None
        rc = r_codes[idx].permute(0, 2, 3, 1) if r_codes is not None else None
        assert n > 0
        return CX.Epi(P.alpha, P.beta, P.levels, P.stats, RELU[relu], rf, r_aff, rc, rscale)

    check_plane(out.codes, flag, q_in, P, epi_of, N, Cout, Ho, Wo, k, stride, out_halo, case, want_flag)
    record(label, case)
    return P


# ---- (a) the implicit-GEMM code epilogue on the C4 net's launches, one case per route -----------------------------------------

# (case, batch, Cin, Cout, H, k, stride, flags next to CONV_NO_DIRECT_CODES, configuration).  A route is (M, Cout, bytes of an
# im2col row), not the batch: where the dispatcher describes the same configuration at a smaller batch the case runs the smallest
# power-of-two batch that still has four 256-row tiles (the test asserts that the description is the batch-256 one); the small-M
# rungs of the 8 x 8 and 4 x 4 stages exist at batch 256 only and run there.
C4_LAUNCHES = [
    ("s1 64->64 @32 (batch 1 = 4 tiles)", 1, 64, 64, 32, 3, 1, 0, "ConvV64x2"),
    ("s2.down 64->128 /2 @32 (batch 4)", 4, 64, 128, 32, 3, 2, 0, "ConvV128x2"),
    ("s2 128->128 @16 (batch 4)", 4, 128, 128, 16, 3, 1, 0, "ConvV128"),
    ("s3.down 128->256 /2 @16", BATCH, 128, 256, 16, 3, 2, 0, "ConvV128x128D"),
    ("s3.down 128->256 /2 @16, no deep ring (batch 16)", 16, 128, 256, 16, 3, 2, NO_RING, "ConvVPP256"),
    ("s3 256->256 @8", BATCH, 256, 256, 8, 3, 1, 0, "ConvV128x128D"),
    ("s3 256->256 @8, no deep ring", BATCH, 256, 256, 8, 3, 1, NO_RING, "ConvV128x128"),
    ("s4.down 256->512 /2 @8", BATCH, 256, 512, 8, 3, 2, 0, "ConvV128x64D"),
    ("s4.down 256->512 /2 @8, no deep ring", BATCH, 256, 512, 8, 3, 2, NO_RING, "ConvV128x64"),
    ("s4 512->512 @4", BATCH, 512, 512, 4, 3, 1, 0, "ConvV128x64D"),
    ("s4 512->512 @4, no deep ring", BATCH, 512, 512, 4, 3, 1, NO_RING, "ConvV128x64"),
    ("s4 512->512 @4 at batch 16 (M = 256: the skinny rung)", 16, 512, 512, 4, 3, 1, 0, "ConvVSkinny"),
]


def _describe_c4(N, Cin, Cout, H, k, stride, flags, epilogue=None):
    kb = k * k * ops.code_ld_bytes(Cin, 16)
    ldw = ops.code_ld_bytes(kb, 512 if kb >= 2048 else 128) // 4
    return ops.conv_kernel_name(1, N, H, H, ops.code_ld_bytes(Cin, 16) // 4, (k, k), (stride, stride), (k // 2, k // 2), (1, 1), ldw, Cout,
                                in_halo=(1, 1), epilogue=ops.EPI_CODES if epilogue is None else epilogue, variant=flags)


@pytest.mark.parametrize("designed", [True, False], ids=["designed", "realistic"])
@pytest.mark.parametrize("case,N,Cin,Cout,H,k,stride,extra,cfg", C4_LAUNCHES, ids=[c[0] for c in C4_LAUNCHES])
def test_implicit_code_conv_on_the_c4_launches(dev, case, N, Cin, Cout, H, k, stride, extra, cfg, designed):
    flags = NO_DIRECT | extra
    if "skinny" not in case:
        assert _describe_c4(N, Cin, Cout, H, k, stride, flags) == _describe_c4(BATCH, Cin, Cout, H, k, stride, flags) == f"{cfg}<ElemI8>"
    # stride-1 layers carry the identity shortcut as a code residual (halo 1), as the fused blocks launch them
    res = "codes" if (stride == 1 and Cin == Cout) else None
    conv_case(dev, f"{case} {'designed' if designed else 'realistic'}", N, Cin, Cout, H, k=k, stride=stride, designed=designed,
              res=res, res_halo=(1, 1), flags=flags, expect=cfg, seed=Cin + Cout + H + (0 if designed else 50))


SHORTCUTS = [("s2.sc 64->128", 4, 64, 128, 32), ("s3.sc 128->256", 16, 128, 256, 16), ("s4.sc 256->512", 64, 256, 512, 8)]


@pytest.mark.parametrize("designed", [True, False], ids=["designed", "realistic"])
@pytest.mark.parametrize("case,N,Cin,Cout,H", SHORTCUTS, ids=[c[0] for c in SHORTCUTS])
def test_shortcut_conv_feeds_the_main_conv_as_res_f32(dev, case, N, Cin, Cout, H, designed):
    """The 1 x 1 stride-2 shortcut conv with the device BatchNorm in its epilogue (fp32 out) against the reference's
    fma(fl(fl(v - mean) * rs), weight, bias); its result is then the fp32 residual of the stage's second conv (Cout -> Cout at H / 2,
    the straight-line epilogue with an fp32 residual).  Batches: the smallest with four 256-row tiles of the main conv."""
    seed = Cin + H + (0 if designed else 50)
    P = Params(dev, Cin, Cout, 1, designed, "device", 4, seed)
    q_in = input_codes(N, Cin, H, H, designed, seed, dev)
    px = planes(q_in, (1, 1), 1.0, 4)
    wc = ops.pack_conv_weight_codes(P.weight)
    label = _describe_c4(N, Cin, Cout, H, 1, 2, 0, ops.EPI_HALO_BN)
    y = traced(lambda: ops.conv2d_codes(px, (N, Cin, H, H), wc, (1, 1), P.scale, None, 2, 0, 1, scale_dev=P.scale_dev,
                                        epi=ops.BnEpilogue(P.alpha, P.beta, P.bn_stats), in_halo=(1, 1)), label, case, label)
    acc = CX.exact_acc(q_in, P.w_int, 2, 0).permute(0, 2, 3, 1)
    v = CX.conv_value(acc, P.kscale)
    want, alt = CX.f_fma(CX.f_mul(CX.f_sub(v, P.stats[0]), P.stats[1]), P.alpha, P.beta)
    got = y.view(want.shape)
    diff = (got != want)
    undecided = diff & (got == alt)
    assert int((diff & ~undecided).sum()) == 0, (case, int(diff.sum()), got[diff][:4], want[diff][:4])
    assert int(undecided.sum()) <= (0 if designed else CX.waiver_cap(want.numel()))
    record(f"{label} BatchNorm epilogue", case)
    Ho = H // 2
    cfg = _describe_c4(N, Cout, Cout, Ho, 3, 1, NO_DIRECT)
    conv_case(dev, f"{case} -> main conv", N, Cout, Cout, Ho, designed=designed, res="f32", res_f32_given=y, flags=NO_DIRECT,
              expect=cfg[:-len("<ElemI8>")], seed=seed + 1)


# ---- (b) the epilogue's forms at one shape per tile family --------------------------------------------------------------------

FULL = (4, 64, 64, 8, 8)         # M = 256, one whole 256 x 64 tile: the straight-line (fast) branch where the form allows it
RAGGED = (3, 40, 52, 9, 11)      # M = 297, Cout % 32 != 0: partial row and column tiles, the general branch
ODD = (3, 40, 50, 9, 11)         # Cout % 4 != 0
FORMS = [
    # (id, shape, keyword arguments of conv_case)
    ("device/fast", FULL, {}),
    ("device/fast no relu", FULL, {"relu": False}),
    ("device/general by conv bias", FULL, {"conv_bias": True}),
    ("device/general by pre-relu", FULL, {"relu": "pre"}),
    ("device/general by ragged tiles", RAGGED, {}),
    ("device/ragged, bounds-checked taps", RAGGED, {"in_halo": (0, 0), "expect": "Conv64"}),
    ("device/Cout % 4 != 0", ODD, {}),
    ("device/Cout % 4 != 0 pre-relu bias", ODD, {"relu": "pre", "conv_bias": True}),
    ("folded", FULL, {"form": "folded"}),
    ("folded ragged", RAGGED, {"form": "folded", "relu": False}),
    ("folded pre-relu bias", RAGGED, {"form": "folded", "relu": "pre", "conv_bias": True}),
    ("res_f32 device fast", FULL, {"res": "f32"}),
    ("res_f32 device ragged", RAGGED, {"res": "f32"}),
    ("res_f32 folded", FULL, {"form": "folded", "res": "f32"}),
    ("res_f32 folded res_affine", FULL, {"form": "folded", "res": "f32_affine"}),
    ("res_f32 folded res_affine ragged", RAGGED, {"form": "folded", "res": "f32_affine"}),
    ("res_f32 device BatchNorm of the residual", FULL, {"res": "f32_bn"}),
    ("res_codes halo (0,0)", FULL, {"res": "codes", "res_halo": (0, 0)}),
    ("res_codes halo (1,1)", FULL, {"res": "codes", "res_halo": (1, 1)}),
    ("res_codes halo (2,1)", FULL, {"res": "codes", "res_halo": (2, 1)}),
    ("res_codes halo (2,1) ragged no relu", RAGGED, {"res": "codes", "res_halo": (2, 1), "relu": False}),
    ("res_codes halo (1,1) folded", RAGGED, {"res": "codes", "res_halo": (1, 1), "form": "folded"}),
    ("out_halo (0,0)", FULL, {"out_halo": (0, 0)}),
    ("out_halo (3,0)", FULL, {"out_halo": (3, 0)}),
    ("out_halo (0,0) ragged", RAGGED, {"out_halo": (0, 0)}),
    ("out_halo (3,0) ragged", ODD, {"out_halo": (3, 0)}),
    ("in_halo (2,1)", FULL, {"in_halo": (2, 1)}),
    ("in_halo (2,1) ragged", RAGGED, {"in_halo": (2, 1)}),
    ("2 bit", FULL, {"bits": 2}),
    ("8 bit", FULL, {"bits": 8}),
    ("2 bit ragged", RAGGED, {"bits": 2, "res": "codes"}),
    ("8 bit ragged folded", RAGGED, {"bits": 8, "form": "folded"}),
    ("scale_dev", FULL, {"use_scale_dev": True}),
    ("scale_dev ragged", RAGGED, {"use_scale_dev": True}),
]


@pytest.mark.parametrize("designed", [True, False], ids=["designed", "realistic"])
@pytest.mark.parametrize("name,shape,kw", FORMS, ids=[f[0] for f in FORMS])
def test_code_epilogue_forms(dev, name, shape, kw, designed):
    N, Cin, Cout, H, W = shape
    kw = dict(kw)
    if not designed and "use_scale_dev" in kw:
        kw["use_scale_dev"] = False          # realistic cases pass scale_dev by default: here the product as ONE host scale
    kw.setdefault("expect", "ConvV64x2")
    conv_case(dev, f"{name} {'designed' if designed else 'realistic'}", N, Cin, Cout, H, W, designed=designed, flags=NO_DIRECT,
              seed=[f[0] for f in FORMS].index(name) + 3, **kw)


@pytest.mark.parametrize("shape", [FULL, RAGGED], ids=["full", "ragged"])
@pytest.mark.parametrize("form", ["device", "folded"])
def test_edge_channels_give_code_zero_and_the_flag(dev, shape, form):
    """Zero, negative-zero and NaN weight, +-1e6 and +-inf bias, a huge rs: code 0 for exactly the reference's out-of-range and NaN
    elements and the range flag raised; the same shape without those channels leaves it at 0."""
    N, Cin, Cout, H, W = shape
    conv_case(dev, f"edges {form}", N, Cin, Cout, H, W, designed=False, form=form, edges=True, want_flag=True, flags=NO_DIRECT,
              expect="ConvV64x2", seed=77)
    conv_case(dev, f"no edges {form}", N, Cin, Cout, H, W, designed=False, form=form, edges=False, want_flag=False, flags=NO_DIRECT,
              expect="ConvV64x2", seed=77)


OFFSET = [
    # (id, N, Cin, Cout, H, W, keyword arguments): every form of the device BatchNorm fma
    ("implicit straight-line", 4, 64, 64, 8, 8, {"expect": "ConvV64x2", "flags": NO_DIRECT}),
    ("implicit straight-line code residual", 4, 64, 64, 8, 8, {"expect": "ConvV64x2", "flags": NO_DIRECT, "res": "codes", "res_halo": (1, 1)}),
    ("implicit straight-line fp32 residual", 4, 64, 64, 8, 8, {"expect": "ConvV64x2", "flags": NO_DIRECT, "res": "f32"}),
    ("implicit general", 3, 40, 52, 9, 11, {"expect": "ConvV64x2", "flags": NO_DIRECT}),
    ("direct 64", 2, 64, 64, 16, 16, {"direct": "code_conv3x3<64,0>", "flags": 0}),
    ("direct 64 code residual", 2, 64, 64, 16, 16, {"direct": "code_conv3x3<64,0>", "flags": 0, "res": "codes", "res_halo": (1, 1)}),
    ("direct 128", 4, 128, 128, 8, 8, {"direct": "code_conv3x3<128,2>", "flags": 0}),
    ("direct 128 code residual no relu", 4, 128, 128, 8, 8, {"direct": "code_conv3x3<128,2>", "flags": 0, "res": "codes", "res_halo": (1, 1),
                                                           "relu": False}),
]


@pytest.mark.parametrize("name,N,Cin,Cout,H,W,kw", OFFSET, ids=[c[0] for c in OFFSET])
def test_fma_single_rounding_decides_codes(dev, name, N, Cin, Cout, H, W, kw):
    """BatchNorm statistics with a common offset of 2^16 that the bias takes out again (CX.cancelling_params): the product inside
    the fma is ~7000 while t is ~1, so a kernel that rounds the product before adding the bias gives other codes for a few elements
    in a thousand (tests/test_codes_exact_cpu.py counts them at these shapes).  The integer sums of a layer take only a few thousand
    values per channel: with plain statistics the single rounding decides a code about once in a million distinct values."""
    conv_case(dev, f"offset {name}", N, Cin, Cout, H, W, designed=False, form="offset", seed=len(name), **kw)


def test_fma_single_rounding_decides_codes_in_the_head(dev):
    C, rows = 40, 297
    P = Params(dev, C, C, 1, False, "offset", 4, 5)
    x = torch.randn((rows, C), device=dev, generator=CX._gen(9, dev)) * 5
    out, _ = ops.affine_dorefa_codes(x, P.alpha, P.beta, 4, True, ld_bytes=ops.code_ld_bytes(C, 16), bn_stats=P.bn_stats)
    ref = CX.epilogue(x, CX.Epi(P.alpha, P.beta, 15.0, P.stats, 1))
    got = CX.decode_plane(out.codes, 1, 1, rows, C).permute(0, 2, 3, 1)
    w, msg = CX.compare_codes(got, {k: (v.view(1, 1, rows, C) if torch.is_tensor(v) else v) for k, v in ref.items()}, False, what="head offset")
    assert not msg and w == 0, msg
    assert int(out.overflow.item()) == ref["flag_head"] == 0


# ---- (c) the persistent direct 3 x 3 kernel ----------------------------------------------------------------------------------

def c3_plan(N, Cin, Cout, H, W, in_halo=(1, 1)):
    """qt_code_conv3x3_try's launch numbers (csrc/code_conv3x3.hip, restated): rows per tile, LDS bytes, workgroups per CU, grid,
    and the tiles the busiest and the idlest workgroup walk."""
    CB = CX.code_ld(Cin)
    RT = 128 // W
    Hp, Wp = H + 2 * in_halo[0], W + 2 * in_halo[1]
    tiles_m, tiles_n = (N * H + RT - 1) // RT, Cout // 64
    patch_rows = RT + 2 if RT <= H else (RT // H) * Hp
    patch_bytes = (patch_rows * Wp * CB + 255) // 256 * 256
    lds = 64 * 9 * CB + 2 * patch_bytes + 4 * 4096
    assert lds <= 160 * 1024, "outside the direct kernel's LDS envelope: the launch would take the implicit-GEMM route"
    per_cu = max(1, min(4, (160 * 1024) // lds))
    grid = min(tiles_m * tiles_n, 256 * per_cu)
    grid = max(tiles_n, grid // tiles_n * tiles_n)
    mstep = grid // tiles_n
    return {"RT": RT, "lds": lds, "per_cu": per_cu, "grid": grid, "tiles": tiles_m * tiles_n,
            "most": (tiles_m + mstep - 1) // mstep, "least": tiles_m // mstep}


def direct_label(Cin):
    return "code_conv3x3<64,0>" if CX.code_ld(Cin) == 64 else "code_conv3x3<128,2>"


# The walk, by the formulas above.  64 channels at 32 x 32: lds = 79360 B, 2 workgroups per CU, grid 512, 8 row tiles per image; batch
# 192 is the smallest with 3 tiles for every workgroup (1536 tiles), batch 200 (1600 tiles) leaves 64 workgroups with 4 tiles and 448
# with 3.  128 -> 128 channels at 16 x 16: lds = 136192 B, 1 workgroup per CU, grid 256 = 128 row walkers x 2 column tiles, 2 row
# tiles per image; batch 192 gives every workgroup 3 tiles (768), batch 200 gives 16 row walkers 4 and 112 of them 3.  The test
# asserts these numbers against c3_plan.
WALK = [
    ("64ch @32 batch 192: 3 tiles per workgroup", 192, 64, 64, 32, {"grid": 512, "per_cu": 2, "most": 3, "least": 3}),
    ("64ch @32 batch 200: ragged 4 / 3", 200, 64, 64, 32, {"grid": 512, "per_cu": 2, "most": 4, "least": 3}),
    ("64ch @32 batch 256: the net's launch", 256, 64, 64, 32, {"grid": 512, "per_cu": 2, "most": 4, "least": 4}),
    ("128ch @16 batch 192: 3 tiles per workgroup", 192, 128, 128, 16, {"grid": 256, "per_cu": 1, "most": 3, "least": 3}),
    ("128ch @16 batch 200: ragged 4 / 3", 200, 128, 128, 16, {"grid": 256, "per_cu": 1, "most": 4, "least": 3}),
    ("128ch @16 batch 256: the net's launch", 256, 128, 128, 16, {"grid": 256, "per_cu": 1, "most": 4, "least": 4}),
]


@pytest.mark.parametrize("designed", [True, False], ids=["designed", "realistic"])
@pytest.mark.parametrize("case,N,Cin,Cout,H,want", WALK, ids=[c[0] for c in WALK])
def test_direct_kernel_persistent_walk(dev, case, N, Cin, Cout, H, want, designed):
    plan = c3_plan(N, Cin, Cout, H, H)
    assert {k: plan[k] for k in want} == want, plan
    assert plan["tiles"] >= 3 * plan["grid"]             # both LDS patch buffers are refilled by every workgroup
    if N == 192:                                         # ... and no smaller batch does
        assert c3_plan(N - 1, Cin, Cout, H, H)["least"] < 3
    conv_case(dev, f"walk {case} {'designed' if designed else 'realistic'}", N, Cin, Cout, H, designed=designed, res="codes",
              res_halo=(1, 1), flags=0, direct=direct_label(Cin), seed=N + Cin)


GEOMETRY = [
    # (N, Cin, Cout, H, W, in_halo, out_halo, res, relu): RT = 128 / W rows per tile
    (2, 64, 64, 2, 128, (1, 1), (1, 1), None, True),          # W = 128: RT = 1 < H
    (3, 64, 128, 4, 128, (2, 2), (0, 0), None, False),
    (2, 64, 64, 4, 64, (1, 1), (1, 1), "codes", True),        # RT = 2 < H
    (2, 128, 128, 8, 64, (1, 1), (0, 0), None, True),
    (5, 64, 192, 4, 32, (1, 1), (1, 1), None, True),          # RT = 4 == H, ragged: 5 row tiles x 3 column tiles
    (4, 128, 64, 4, 32, (2, 2), (1, 1), None, False),
    (3, 128, 192, 16, 16, (1, 1), (1, 1), None, True),        # RT = 8 < H
    (2, 64, 64, 8, 16, (2, 2), (0, 0), None, True),           # RT = 8 == H
    (6, 64, 128, 8, 8, (1, 1), (1, 1), None, True),           # RT = 16 > H: 2 images per tile
    (6, 128, 128, 8, 8, (1, 1), (1, 1), "codes21", True),     # (residual plane with halo (2, 1): rows and columns differ)
    (4, 64, 64, 8, 8, (2, 2), (0, 0), "codes21", False),
    (24, 64, 64, 4, 4, (1, 1), (1, 1), None, True),           # RT = 32 > H: 8 images per tile
    (16, 128, 128, 4, 4, (1, 1), (1, 1), "codes", True),      # (lds = 160 KiB exactly: the envelope's edge)
    (8, 64, 192, 4, 4, (2, 2), (0, 0), None, False),
    (8, 64, 64, 8, 4, (1, 1), (1, 1), None, True),            # W = 4, H = 8: 4 images per tile
    (8, 128, 128, 64, 4, (1, 1), (1, 1), None, True),         # W = 4, RT = 32 < H
]


@pytest.mark.parametrize("designed", [True, False], ids=["designed", "realistic"])
@pytest.mark.parametrize("N,Cin,Cout,H,W,ih,oh,res,relu", GEOMETRY, ids=[f"{g[1]}->{g[2]} {g[0]}x{g[3]}x{g[4]} in{g[5][0]} out{g[6][0]}" for g in GEOMETRY])
def test_direct_kernel_geometry(dev, N, Cin, Cout, H, W, ih, oh, res, relu, designed):
    """Tiles inside an image, one image per tile, several images per tile (the input's top and bottom rows hold a per-image
    constant: a halo row taken from the neighbouring image changes the sum), both loader modes, Cout 64 / 128 / 192."""
    assert (N * H * W) % 128 == 0
    c3_plan(N, Cin, Cout, H, W, ih)
    conv_case(dev, f"direct {Cin}->{Cout} {N}x{H}x{W} in{ih} out{oh} {'designed' if designed else 'realistic'}", N, Cin, Cout, H, W,
              designed=designed, relu=relu, in_halo=ih, out_halo=oh, res="codes" if res else None,
              res_halo=(2, 1) if res == "codes21" else (1, 1), flags=0, direct=direct_label(Cin), seed=N + H + W + Cin, image_rows=True)


@pytest.mark.parametrize("Cin,Cout,N,H", [(64, 64, 2, 16), (128, 128, 4, 8)])
def test_direct_kernel_edge_channels(dev, Cin, Cout, N, H):
    """The edge channels through the direct kernel's packed-fp32 epilogue: code 0 and the flag for exactly the reference's
    out-of-range and NaN elements (q = 127 stays, q = 128 goes); without them the flag stays 0."""
    for edges in (True, False):
        conv_case(dev, f"direct edges={edges} {Cin}->{Cout}", N, Cin, Cout, H, designed=False, edges=edges, want_flag=edges, flags=0,
                  direct=direct_label(Cin), seed=31)


# ---- (d) the chain's other kernels --------------------------------------------------------------------------------------------

# One thread of affine_codes_kernel (csrc/codes_i8.hip) takes 4 consecutive channels and loads them as one float4 when the row
# stride is a multiple of 4 floats: C = 64 and 40 are multiples of that width, C = 3 is not (scalar loads, 1 valid channel of 4).
HEAD = [(c, f, r, res) for c in (3, 40, 64) for f in ("device", "folded") for r in (False, True, "pre")
        for res in (None, "f32", "f32_affine", "codes")]


@pytest.mark.parametrize("designed", [True, False], ids=["designed", "realistic"])
@pytest.mark.parametrize("C,form,relu,res", HEAD, ids=[f"C{h[0]} {h[1]} relu={h[2]} res={h[3]}" for h in HEAD])
def test_head_kernel(dev, C, form, relu, res, designed):
    """ops.affine_dorefa_codes: [rows, C] fp32 -> codes, flat (rows = 33: the general walk for C = 40; 297: the fixed-slot walk) and
    into a halo plane; with an fp32 residual also through the residual's own BatchNorm in the form of the main one."""
    seed = C + len(form) + RELU[relu] * 7 + (0 if designed else 50)
    for N, H, W, halo in ((3, 9, 11, (0, 0)), (1, 3, 11, (0, 0)), (3, 9, 11, (1, 1)), (4, 8, 8, (2, 1))):
        rows = N * H * W
        P = Params(dev, C, C, 1, designed, form, 4, seed)
        g = CX._gen(seed + rows, dev)
        x = (torch.randint(-120, 121, (rows, C), device=dev, generator=g).float() / 4) if designed else \
            (torch.randn((rows, C), device=dev, generator=g) * 5)
        if designed:      # x = acc / 4 with the conv cases' scale folded in: the same exact chain
            P.stats = (P.stats[0], torch.full_like(P.stats[1], 0.25)) if P.stats is not None else None
            P.alpha = P.alpha if P.stats is not None else torch.sign(P.alpha) * 0.5
            P.bn_stats = torch.cat(list(P.stats)).contiguous() if P.stats is not None else None
        rf = ra = rc = None
        rscale = 0.25 if designed else ops.inv_levels(4)
        kw = {}
        if res == "codes":
            rc = CX.random_codes((rows, C), 0, 15, seed + 5, dev)
            pl = CX.encode_plane(rc.view(rows, C, 1, 1), (0, 0), CX.code_ld(C))
            kw["res_codes"] = ops.CodePlanes(codes=pl, rows=rows, K=C, inv_n=rscale, bit_width=4)
        elif res is not None:
            rf = P.residual_f32((rows, C), seed + 6, dev)
            kw["res_f32"] = rf
            if res == "f32_affine":
                ra = P.residual_affine(C, seed + 7, dev, form == "device")
                kw["res_affine"] = ra if len(ra) == 2 else (ra[0], ra[1], torch.cat(list(ra[2])).contiguous())
        out, _ = ops.affine_dorefa_codes(x, P.alpha, P.beta, 4, relu, ld_bytes=ops.code_ld_bytes(C, 16), bn_stats=P.bn_stats,
                                         halo_nhw=(N, H, W) if any(halo) else None, out_halo=halo, **kw)
        ref = CX.epilogue(x, CX.Epi(P.alpha, P.beta, 15.0, P.stats, RELU[relu], rf, ra, rc, rscale))
        got = CX.decode_plane(out.codes, N, H, W, C, halo, "head").permute(0, 2, 3, 1).reshape(rows, C)
        case = f"head C={C} {form} relu={relu} res={res} {N}x{H}x{W} halo {halo}"
        w, msg = CX.compare_codes(got.view(1, 1, rows, C), {k: (v.view(1, 1, rows, C) if torch.is_tensor(v) else v) for k, v in ref.items()},
                                  designed, what=case)
        assert not msg, msg
        assert w <= CX.waiver_cap(got.numel())
        assert int(out.overflow.item()) == ref["flag_head"], (case, int(out.overflow.item()), ref["flag_head"])
        TOTALS["cases"] += 1
        TOTALS["waived"] += w
        TOTALS["elements"] += got.numel()


def test_head_kernel_edge_channels(dev):
    """NaN / inf / huge parameters in the head: code 0 and flag 3 (some |q| > 2047 or NaN), as the kernel documents."""
    C, rows = 40, 297
    P = Params(dev, C, C, 1, False, "device", 4, 5, edges=True)
    x = torch.randn((rows, C), device=dev, generator=CX._gen(9, dev)) * 5
    out, _ = ops.affine_dorefa_codes(x, P.alpha, P.beta, 4, True, ld_bytes=ops.code_ld_bytes(C, 16), bn_stats=P.bn_stats)
    ref = CX.epilogue(x, CX.Epi(P.alpha, P.beta, 15.0, P.stats, 1))
    got = CX.decode_plane(out.codes, 1, 1, rows, C).permute(0, 2, 3, 1)
    w, msg = CX.compare_codes(got, {k: (v.view(1, 1, rows, C) if torch.is_tensor(v) else v) for k, v in ref.items()}, False, what="head edges")
    assert not msg and w == 0, msg
    assert ref["flag_head"] == 3 and int(out.overflow.item()) == 3


@pytest.mark.parametrize("N,C,H,W,k,s,halo", [(3, 40, 9, 11, 2, 2, (0, 0)), (3, 40, 9, 11, 3, 2, (1, 1)), (2, 64, 8, 8, 2, 2, (1, 1)),
                                              (2, 3, 7, 5, 3, 2, (0, 0)), (4, 64, 32, 32, 3, 2, (2, 1))])
def test_pool_codes_against_integer_max(dev, N, C, H, W, k, s, halo):
    """ops.pool_codes (MaxPool2d(k, s), un-padded, floor mode: what layers.CodeMaxPool accepts) = the max of the decoded integers."""
    q = CX.random_codes((N, C, H, W), -128, 127, N + C + k, dev)
    out = ops.pool_codes(planes(q, (0, 0), 1 / 15, 4), N, H, W, k, s, halo)
    Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
    want = F.max_pool2d(q.double(), k, s).to(torch.int64)
    assert torch.equal(CX.decode_plane(out.codes, N, Ho, Wo, C, halo, "pooled plane"), want)


@pytest.mark.parametrize("N,C,H,W,halo", [(3, 40, 9, 11, (0, 0)), (2, 3, 5, 4, (1, 1)), (2, 64, 8, 8, (2, 1)), (1, 50, 3, 3, (1, 1))])
def test_codes_to_f32_against_code_times_inv_n(dev, N, C, H, W, halo):
    """ops.codes_to_f32 = fl(code * inv_n); with the chain's range flag raised every value is NaN (``nan_all`` in the kernel)."""
    q = CX.random_codes((N, C, H, W), -128, 127, N + C, dev)
    inv = ops.inv_levels(4)
    cp = planes(q, halo, inv, 4)
    cp.overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
    y = ops.codes_to_f32(cp, N, H, W, halo)
    want = CX.f_mul(q.permute(0, 2, 3, 1).float(), CX.f32_scalar(inv, dev))
    assert y.shape == want.shape and torch.equal(y, want)
    cp.overflow.fill_(1)
    assert bool(torch.isnan(ops.codes_to_f32(cp, N, H, W, halo)).all())
    assert torch.equal(ops.codes_to_f32(cp, N, H, W, halo, flagged=False), want)


# ---- (e) the fused C4 net block by block at batch 256 -------------------------------------------------------------------------

def _c4_model(dev):
    import bench_models
    torch.manual_seed(4)
    m4 = bench_models.DorefaResNet18(w_bits=1, a_bits=4)
    bench_models.randomize_bn(m4, seed=3)
    for m in m4.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_var.mul_(4.0)
    m4 = m4.to(dev).to(memory_format=torch.channels_last).eval()
    return m4, bench_models.FusedDorefaResNet18(m4, fold="device")


class _NetParams:
    """Reference operands of one fused conv of the net: sign weights, the kernel's scale, the device BatchNorm's numbers."""
    designed, bias = False, None

    def __init__(self, fconv, shape):
        from pytorch_quantize_impls_amd.layers.fused import device_bn_fold
        conv = fconv.conv if hasattr(fconv, "conv") else fconv
        w = conv.weight.detach()
        self.w_int = torch.where(w < 0, -1.0, 1.0)
        E = conv._eval_planes(lambda w2: w2.abs().amax(), key="E")
        self.kscale = CX.kernel_scale(ops.inv_levels(4), E, w.device)
        bn = fconv.bn if hasattr(fconv, "bn") else None
        if bn is not None:
            self.alpha, self.beta, st = device_bn_fold(bn, shape, True)
            self.stats = (st[:len(st) // 2], st[len(st) // 2:])


def _act(q, dev):
    from pytorch_quantize_impls_amd import packed
    cp = planes(q, (1, 1), ops.inv_levels(4), 4)
    cp.overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
    return packed.CodeActivation(cp, tuple(q.shape), halo=(1, 1))


def test_c4_fused_resnet18_blockwise_at_batch_256(dev):
    """bench_models.FusedDorefaResNet18(fold="device"), 256 images of 3 x 32 x 32, default switches (the direct kernel on): the head
    and every fused conv of every block against the reference, each fed the REFERENCE chain's code plane, under the waiver rule."""
    from pytorch_quantize_impls_amd import utils
    m4, f4 = _c4_model(dev)
    x = torch.randn((BATCH, 3, 32, 32), device=dev, generator=CX._gen(256, dev)).contiguous(memory_format=torch.channels_last)
    N = BATCH
    with torch.no_grad(), utils.implicit_graphs(False):
        x0 = f4.stem(x)
        head = f4.q0(x0)
        from pytorch_quantize_impls_amd.layers.fused import device_bn_fold
        hw, hb, hst = device_bn_fold(m4.bn, tuple(x0.shape), True)
        ref = CX.epilogue(x0.permute(0, 2, 3, 1), CX.Epi(hw, hb, 15.0, (hst[:64], hst[64:]), 1))
        got = CX.decode_plane(head.codes.codes, N, 32, 32, 64, (1, 1), "head").permute(0, 2, 3, 1)
        w, msg = CX.compare_codes(got, ref, False, what="c4 head")
        assert not msg and w <= CX.waiver_cap(got.numel()), msg
        assert int(head.codes.overflow.item()) == ref["flag_head"] == 0
        cur = ref["codes"].permute(0, 3, 1, 2).contiguous()
        for bi, blk in enumerate(f4.blocks):
            _, Cin, H, _ = cur.shape
            c1, c2 = blk.c1, blk.c2
            Cout, stride = c1.conv.out_channels, c1.conv.stride[0]
            Ho = H // stride
            kernels = {(64, 1): "code_conv3x3<64,0>", (128, 1): "code_conv3x3<128,2>"}
            k1 = kernels.get((Cout, stride)) or _describe_c4(N, Cin, Cout, H, 3, stride, 0)
            # (a conv with an fp32 residual — the blocks with a shortcut conv — is not the direct kernel's case)
            k2 = (kernels.get((Cout, 1)) if blk.sc_conv is None else None) or _describe_c4(N, Cout, Cout, Ho, 3, 1, 0)
            # conv1 -> bn1 -> relu -> quant
            a_in = _act(cur, dev)
            o1 = traced(lambda: c1(a_in), k1, f"c4 block {bi} conv1")
            P1 = _NetParams(c1, (N, Cout, Ho, Ho))
            check_plane(o1.codes.codes, o1.codes.overflow, cur, P1, lambda idx: CX.Epi(P1.alpha, P1.beta, 15.0, P1.stats, 1),
                        N, Cout, Ho, Ho, 3, stride, (1, 1), f"c4 block {bi} conv1 ({k1})", want_flag=False)
            record(k1, f"c4 block {bi} conv1")
            step = X.image_chunk(X.conv_bytes_per_image(Cin, H, H, Cout, 3, stride, 1), BUDGET)
            mid = torch.cat([CX.epilogue(CX.conv_value(CX.exact_acc(cur[n0:n0 + step], P1.w_int, stride, 1).permute(0, 2, 3, 1), P1.kscale),
                                         CX.Epi(P1.alpha, P1.beta, 15.0, P1.stats, 1))["codes"] for n0 in range(0, N, step)]).permute(0, 3, 1, 2).contiguous()
            # conv2 -> bn2 -> + shortcut -> relu -> quant
            a_mid = _act(mid, dev)
            P2 = _NetParams(c2, (N, Cout, Ho, Ho))
            if blk.sc_conv is None:
                a_res = _act(cur, dev)
                o2 = traced(lambda: c2(a_mid, residual=a_res), k2, f"c4 block {bi} conv2")
                res_codes, res_f32 = cur.permute(0, 2, 3, 1), None
            else:
                # the shortcut branch (1 x 1 / 2 conv -> BatchNorm, one launch) against the reference, then as the fp32 residual
                ksc = _describe_c4(N, Cin, Cout, H, 1, stride, 0, ops.EPI_HALO_BN)
                y2, none = traced(lambda: c2._shortcut(blk.sc_conv, _act(cur, dev), blk.sc_bn), ksc, f"c4 block {bi} shortcut")
                assert none is None, "the shortcut branch did not run as one launch"
                Ps = _NetParams(blk.sc_conv, None)
                sw, sb, sst = device_bn_fold(blk.sc_bn, (N, Cout, Ho, Ho), True)
                v = CX.conv_value(CX.exact_acc(cur, Ps.w_int, stride, 0).permute(0, 2, 3, 1), Ps.kscale)
                want, alt = CX.f_fma(CX.f_mul(CX.f_sub(v, sst[:Cout]), sst[Cout:]), sw, sb)
                gy = y2.view(want.shape)
                bad = (gy != want) & (gy != alt)
                assert int(bad.sum()) == 0 and int((gy != want).sum()) <= CX.waiver_cap(want.numel()), (bi, int(bad.sum()))
                record(f"{ksc} BatchNorm epilogue", f"c4 block {bi} shortcut")
                o2 = traced(lambda: c2(a_mid, residual=y2), k2, f"c4 block {bi} conv2")
                res_codes, res_f32 = None, gy          # what the conv was fed (verified above)

            def epi2(idx, res_codes=res_codes, res_f32=res_f32, P2=P2):
                return CX.Epi(P2.alpha, P2.beta, 15.0, P2.stats, 1, res_f32[idx] if res_f32 is not None else None, None,
                              res_codes[idx] if res_codes is not None else None, ops.inv_levels(4))
            check_plane(o2.codes.codes, o2.codes.overflow, mid, P2, epi2, N, Cout, Ho, Ho, 3, 1, (1, 1), f"c4 block {bi} conv2 ({k2})",
                        want_flag=False)
            record(k2, f"c4 block {bi} conv2")
            step = X.image_chunk(X.conv_bytes_per_image(Cout, Ho, Ho, Cout, 3, 1, 1), BUDGET)
            cur = torch.cat([CX.epilogue(CX.conv_value(CX.exact_acc(mid[n0:n0 + step], P2.w_int, 1, 1).permute(0, 2, 3, 1), P2.kscale),
                                         epi2(slice(n0, min(N, n0 + step))))["codes"] for n0 in range(0, N, step)]).permute(0, 3, 1, 2).contiguous()
        assert cur.shape == (N, 512, 4, 4)


# ---- (f) coverage -------------------------------------------------------------------------------------------------------------

def test_every_described_code_conv_configuration_ran_against_the_exact_reference():
    if not COVERED:
        pytest.skip("run the whole module: the cases above record the configurations they compared")
    expected = {"code_conv3x3<64,0>", "code_conv3x3<128,2>"}
    cin = 64
    for cout, stride, H in ((64, 1, 32), (64, 1, 32), (128, 2, 32), (128, 1, 16), (256, 2, 16), (256, 1, 8), (512, 2, 8), (512, 1, 4)):
        for a, b, h, s in ((cin, cout, H, stride), (cout, cout, H // stride, 1)):
            for flags in (0, NO_DIRECT, NO_RING, NO_DIRECT | NO_RING):
                expected.add(_describe_c4(BATCH, a, b, h, 3, s, flags))
        cin = cout
    missing = sorted(c for c in expected if c not in COVERED)
    print("\n".join(["code-conv configurations exercised:"] + [f"{c}: {', '.join(COVERED.get(c, ['-'])[:3])}" for c in sorted(expected)]))
    wall = time.time() - TOTALS["t0"] if TOTALS["t0"] else float("nan")
    print(f"cases {TOTALS['cases']}, codes compared {TOTALS['elements']}, designed bytes differing {TOTALS['designed_bytes_differing']}, "
          f"waived {TOTALS['waived']}, wall {wall:.0f} s, peak device memory {max(PEAK.values()) / 2**30:.2f} GiB "
          f"({max(PEAK, key=PEAK.get)})")
    assert not missing, missing
