"""The XNOR-Net tap convs (csrc/conv_taps.hip, the E::TAPS paths of csrc/mfma_gemm_kernel.h) route by route against the
independent float64 reference of tests/_xnor_exact.py.

  (a) exact, every bit: +-1 activations, weights +-2^{e_t} (power-of-two tap alphas over the widest span the exactness proof
      allows, ramp up then drop; an all-zero tap in the middle, a leading one, a lone zero weight), ops.conv2d_nib_taps on packed
      planes with bias == the float64 reference converted to fp32, for every configuration select_conv_taps (csrc/tile_select.h) can select, odd
      k-steps per tap (Cin = 192, 576; 3 x 3 and 5 x 5), 1 x 1, stride 2, anisotropic padding, dilation 2, ragged M and Cout,
      and bench_models.alexnet_xnor's conv2 .. conv5 at batch 256;
  (b) the threshold-bit and nibble-halo-plane epilogues on the same inputs, every word against tests/_exact.predicate on the
      exact y: edge channels (zero / negative-zero / NaN slopes, +-1e6 and +-inf offsets), exact ties placed on values the
      exact result takes, pad bits, zero halo — no bit excluded;
  (c) quant_input=True, Conv128<ElemFp4TapsRows>: ops.conv2d_nib_taps_rows with a power-of-two per-pixel scale plane (all-zero
      pixels at the left edge, in the middle and as a whole image row), bit-exact against xnor_rows64;
  (d) grad_x, ElemF16Taps: ops.conv2d_grad_input_taps on integer gradients x 2^exp (exp -40 and 30), bit-exact against
      xnor_grad_input64, on every configuration the transposed conv selects and at AlexNet-XNOR conv2 .. conv5, batch 256
      (the route always takes the two-term fp16 split: ops.FLOAT_SPLIT is not consulted);
  (e) Gaussian weights (nearly equal alphas; a second set with per-tap scales over six decades and one tap at 2^-60 of the
      others) through (a), (c), (d), per output ELEMENT:  |got - ref64| <= (S + 2 T + 16) 2^-23 B  (S MFMA k-steps along K, T
      taps, B the element's magnitude bound; derivation at _xnor_exact.horner_bound);
  (f) closure: every Config<Elem> select_conv_taps can return was compared above, and every kernel instance with `Taps` in its name
      that a batch-256 training step of bench_models.alexnet_xnor, its eval-mode deferred forward and an
      XNORConv2d(quant_input=True) training step launch is among them.

Every case asserts the kernel configuration it names (torch.profiler) before it records it.
Run the whole module: the closure tests read what the cases before them recorded.

Measured on an MI355X (whole module, 118 cases): 9 s, peak device memory 7.75 GiB (grad_x of alexnet.conv2 at batch 256);
the exact cases with zero mismatching elements / words; worst err / bound of the Gaussian cases 0.115 (forward 1 x 1, nearly
equal alphas: S = 1, so the bound is at its tightest), at most 0.038 elsewhere — MEASURED_RATIOS below, printed again by the
closure test."""
import time

import pytest
import torch

import _exact as X
import _grad_exact as G
import _routes as R
import _xnor_exact as XE

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import ops  # noqa: E402

F64, F32 = torch.float64, torch.float32

ROWS_ROUTE = "Conv128<ElemFp4TapsRows>"
COVERED = {}                # "Config<Elem>/form" -> case ids that compared it
RATIOS = {}                 # Gaussian case -> worst err / bound
PEAK = {}                   # test id -> peak device memory (bytes)
T0 = time.perf_counter()

# worst err / bound of the Gaussian cases as measured on an MI355X, (equal, decades) per case (a record; the bound is derived,
# not tuned: _xnor_exact.horner_bound)
MEASURED_RATIOS = {
    "fwd c256/valid": (0.007, 0.014), "fwd c200/padded": (0.008, 0.015), "fwd rows384/padded": (0.010, 0.020),
    "fwd odd3/5x5/padded": (0.001, 0.006), "fwd odd9/valid": (0.002, 0.006), "fwd stride2": (0.007, 0.019),
    "fwd dil2/padded": (0.011, 0.021), "fwd 1x1": (0.115, 0.030),
    "rows tiny": (0.010, 0.019), "rows stride2": (0.011, 0.038), "rows 5x5": (0.005, 0.013), "rows ragged": (0.010, 0.017),
    "grad c128x128": (0.008, 0.016), "grad skinny": (0.007, 0.011), "grad vpp256": (0.010, 0.014),
    "grad vpp256x192": (0.012, 0.011), "grad cout72": (0.009, 0.018), "grad stride2": (0.007, 0.013),
}


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


def routes(names):
    """Profiler kernel names -> labels 'ConvVPP256<ElemFp4Taps>', ..."""
    return R.mfma_routes(names)


def profiled(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, routes(e.key for e in prof.key_averages())


def traced(fn, expect, case, described=None):
    """Run fn under torch.profiler and assert that the kernel ``expect`` (a label of routes()) ran — and, where the case has a
    describe entry point (``described``: its answer), that it names that kernel."""
    R.assert_described(described, expect, case)
    out, seen = profiled(fn)
    assert expect in seen, (case, expect, sorted(map(str, seen)))
    return out


def record(label, form, case):
    COVERED.setdefault(f"{label}/{form}", []).append(case)


# ---- operands -----------------------------------------------------------------------------------------------------------------

def _tap_scales(w, alpha64, lone, dev, case):
    """TapScales of a designed weight: from the weight itself (the training-mode entry; its fp32 column means must be the
    designed powers of two), or — a lone zero weight makes mean|w| of its tap a non-power of two — from the designed alphas
    (the eval-mode entry)."""
    a32 = alpha64.to(F32).to(dev)
    if lone is None:
        ts = ops.xnor_tap_prep(w)
        assert torch.equal(ts.alpha, a32), (case, ts.alpha.tolist(), a32.tolist())
        return ts
    return ops.xnor_tap_prep(alpha=a32)


class Fwd:
    """Operands of a forward case: +-1 activation, designed (or Gaussian) weight, packed planes, tap tables."""

    def __init__(self, dev, case, weights="pow2"):
        (self.name, self.B, self.Cin, self.Cout, self.H, self.k, self.s, self.p, self.d, variant, self.float_route,
         self.thr_route) = case
        seed = XE.case_seed(self.name)
        k, T = self.k, self.k * self.k
        self.shape = (self.B, self.Cin, self.H, self.H)
        self.x = G.pm1(self.shape, seed, dev)
        self.px = ops.pack_pixels_nib(self.x, ld=ops.pixel_ld_nib_taps(self.Cin))
        self.ksteps = T * self.px.ld // 8
        if weights == "pow2":
            exps, zero_taps, lone = XE.tap_design(T, self.Cin, variant, Cout=self.Cout)
            self.w = XE.pow2_tap_weight((self.Cout, self.Cin, k, k), exps, seed + 1, dev, zero_taps, lone)
            self.alpha64 = XE.designed_alpha(exps, zero_taps, dev)
            self.bias = XE.exact_bias(self.Cout, exps, seed + 2, dev)
            self.ts = _tap_scales(self.w, self.alpha64, lone, dev, self.name)
            ok, why = XE.proves_exact_taps(self.ts.alpha, self.Cin, self.bias)
            assert ok, (self.name, why)
        else:
            self.w = XE.gauss_tap_weight((self.Cout, self.Cin, k, k), seed + 1, dev, **weights)
            self.w[self.Cout // 2, self.Cin // 3, k // 2, k // 2] = 0.0
            self.alpha64 = XE.tap_alpha64(self.w)
            self.bias = torch.randn((self.Cout,), generator=G._gen(seed + 2, dev), device=dev) * float(self.alpha64.max()) * 3
            self.ts = ops.xnor_tap_prep(self.w)
        self.ws = ops.pack_conv_weight_nib(self.w, "sign", cw=self.px.ld)
        self.Ho, self.Wo = XE.out_hw(self.H, self.H, k, k, self.s, self.p, self.d)
        self.args = (self.px, self.shape, self.ws, (k, k), self.ts.fwd, self.bias, self.s, self.p, self.d)

    def run(self, epi=None):
        return ops.conv2d_nib_taps(*self.args, epi=epi)

    def named(self, epilogue=ops.EPI_PLAIN):
        """The kernel the describe entry point names for run() with this epilogue."""
        return ops.conv_taps_kernel_name(0, self.B, self.H, self.H, self.px.ld, ops._pairs(self.k), ops._pairs(self.s), ops._pairs(self.p), ops._pairs(self.d),
                                         self.ws.ld, self.Cout, epilogue)

    def nhwc(self, t):
        return t.permute(0, 2, 3, 1).reshape(self.B * self.Ho * self.Wo, self.Cout)


def _affine_taps(y64, bias, seed, dev):
    """alpha, beta of the threshold epilogue with thresholds spread over the populated range of the exact result y64
    [N, Cout, Ho, Wo] (no bias), the edge channels of test_gpu_exact_b256._affine (zero / negative-zero / NaN slopes, +-1e6 and
    +-inf offsets) and three exact ties: channels 8 .. 10 tie at a value t0 = v0 + bias that the exact result takes (v0 = the
    channel's median, an element of it), so bit <=> y < v0, y > v0, and y < v0 through two roundings."""
    Cout = int(y64.shape[1])
    g = G._gen(seed, dev)
    sig = float(y64.std())
    alpha = (torch.rand(Cout, generator=g, device=dev) - 0.5) * 0.6
    beta = -alpha * torch.randn(Cout, generator=g, device=dev) * sig
    alpha[0], beta[0] = 0.0, 0.5
    alpha[1], beta[1] = 0.0, -1.0
    beta[2], beta[3] = 1e6 * sig, -1e6 * sig
    alpha[4], beta[4] = -0.0, 1.0
    alpha[5] = float("nan")
    beta[6], beta[7] = float("inf"), float("-inf")
    ties = 0
    for c, (a, sgn) in zip((8, 9, 10), ((1.0, -1.0), (-1.0, 1.0), (0.5, -0.5))):
        v0 = y64[:, c].reshape(-1).median()
        t0 = XE.to_f32_exact((v0 + bias[c].to(F64)).reshape(1), "tie")[0]
        alpha[c], beta[c] = a, sgn * t0
        ties += int((y64[:, c] == v0).sum())
    assert ties >= 3
    return alpha, beta


def _check_bits(words, Cout, want, y, v, what):
    Xw = words.view(want.shape[0], want.shape[1] * want.shape[2], -1)
    X.check_pad_bits(Xw, Cout, what)
    got = X.bits_of_words(Xw, Cout).view(want.shape)
    msg = X.mismatch_report(got, want, y, v, what=what)
    assert not msg, msg


def _check_nib(words, f, halo, want, y, v, what):
    got = X.nib_to_bits(X.decode_nib(words, f.B, f.Ho, f.Wo, f.Cout, halo))
    msg = X.mismatch_report(got, want, y, v, what=what)
    assert not msg, msg


# ---- (a) + (b): exact forward, every configuration ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", XE.FWD_CASES, ids=[c[0] for c in XE.FWD_CASES])
def test_forward_is_bit_exact_on_designed_operands(dev, case):
    f = Fwd(dev, case)
    y64 = XE.tap_sums64(f.x, torch.sign(f.w), f.s, f.p, f.d, alpha=f.alpha64)
    want = XE.to_f32_exact(y64 + f.bias.to(F64).view(1, -1, 1, 1), f.name)
    label = f"{f.float_route}<ElemFp4Taps>"
    y = traced(f.run, label, f.name, f.named())
    msg = XE.value_report(y.view(f.B, f.Ho, f.Wo, f.Cout).permute(0, 3, 1, 2), want, what=f"{f.name} fp32 result")
    assert not msg, msg
    record(label, "float", f.name)
    del y, want
    if f.thr_route is None:
        return
    # (b) the threshold epilogues: the fused blocks' fp32 predicate on the exact y
    alpha, beta = _affine_taps(y64, f.bias, XE.case_seed(f.name) + 3, dev)
    bit, v = X.predicate(y64, f.bias, alpha, beta)
    bit, v, ynhwc = bit.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1), y64.permute(0, 2, 3, 1)
    frac = float(bit[..., 11:].float().mean())
    assert 0.2 < frac < 0.8, (f.name, frac)                                  # real thresholds, not all-0 / all-1 planes
    label = f"{f.thr_route}<ElemFp4Taps>"
    bits = traced(lambda: f.run(epi=(alpha, beta)), label, f"{f.name} bits", f.named(ops.EPI_BITS))
    _check_bits(bits.sign, f.Cout, bit, ynhwc, v, f"{f.name} bits")
    record(label, "bits", f.name)
    halo = (2, 1) if f.name == "aniso" else (1, 1)
    nib = traced(lambda: f.run(epi=ops.NibEpilogue(alpha, beta, halo)), label, f"{f.name} nib", f.named(ops.EPI_NIB))
    _check_nib(nib.words, f, halo, bit, ynhwc, v, f"{f.name} nib")
    record(label, "nib", f.name)


# ---- (c) quant_input=True: per-row, per-tap factors -----------------------------------------------------------------------------

class Rows:
    def __init__(self, dev, case, weights="pow2"):
        self.name, self.B, self.Cin, self.Cout, self.H, self.k, self.s, self.p = case
        seed = XE.case_seed("rows " + self.name)
        k, T, H = self.k, self.k * self.k, self.H
        lo, hi = XE.A_EXPS
        if weights == "pow2":
            self.A = XE.pow2_plane((self.B, H, H), lo, hi, 0.1, seed, dev)
        else:
            self.A = torch.rand((self.B, H, H), generator=G._gen(seed, dev), device=dev) + 0.05
            self.A = torch.where(torch.rand((self.B, H, H), generator=G._gen(seed + 5, dev), device=dev) < 0.1, 0.0, self.A)
        # all-zero pixels: the left edge of the first windows, a whole row of the image, the middle of a window
        self.A[:, :, 0] = 0.0
        self.A[:, H // 2, :] = 0.0
        self.A[:, 1, 2] = 0.0
        self.xs = G.pm1((self.B, self.Cin, H, H), seed + 1, dev) * (self.A != 0).unsqueeze(1)
        self.x = (self.xs * self.A.unsqueeze(1)).contiguous(memory_format=torch.channels_last)
        Cw = ops.pixel_ld_nib_taps(self.Cin)
        self.ksteps = T * Cw // 8
        if weights == "pow2":
            exps, zero_taps, _ = XE.tap_design(T, self.Cin, "mid", x_absmax=2.0 ** (hi - lo), Cout=self.Cout)
            self.w = XE.pow2_tap_weight((self.Cout, self.Cin, k, k), exps, seed + 2, dev, zero_taps)
            self.alpha64 = XE.designed_alpha(exps, zero_taps, dev)
            self.bias = XE.exact_bias(self.Cout, [e + lo for e in exps], seed + 3, dev)
            self.ts = _tap_scales(self.w, self.alpha64, None, dev, self.name)
            nz = self.A[self.A != 0]
            ok, why = XE.proves_exact_taps(self.ts.alpha, self.Cin, self.bias, x_absmax=float(nz.max()), x_quantum=G.quantum_exp(nz))
            assert ok, (self.name, why)
        else:
            self.w = XE.gauss_tap_weight((self.Cout, self.Cin, k, k), seed + 2, dev, **weights)
            self.alpha64 = XE.tap_alpha64(self.w)
            self.bias = torch.randn((self.Cout,), generator=G._gen(seed + 3, dev), device=dev) * float(self.alpha64.max())
            self.ts = ops.xnor_tap_prep(self.w)
        self.wp = ops.pack_conv_weight_nib(self.w, "sign", cw=Cw)
        self.Ho, self.Wo = XE.out_hw(H, H, k, k, self.s, self.p, 1)

    def run(self):
        y = ops.conv2d_nib_taps_rows(self.x, self.A, self.wp, (self.k, self.k), self.ts.fwd, self.bias, self.s, self.p, 1)
        assert y is not None
        return y.view(self.B, self.Ho, self.Wo, self.Cout).permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", XE.ROWS_CASES, ids=[c[0] for c in XE.ROWS_CASES])
def test_row_scaled_forward_is_bit_exact_on_designed_operands(dev, case):
    r = Rows(dev, case)
    y64 = XE.tap_sums64(r.xs, torch.sign(r.w), r.s, r.p, 1, alpha=r.alpha64, a_plane=r.A)
    want = XE.to_f32_exact(y64 + r.bias.to(F64).view(1, -1, 1, 1), r.name)
    y = traced(r.run, ROWS_ROUTE, f"rows {r.name}")
    msg = XE.value_report(y, want, what=f"rows {r.name}")
    assert not msg, msg
    record(ROWS_ROUTE, "float", f"rows {r.name}")


# ---- (d) grad_x -----------------------------------------------------------------------------------------------------------------

class Grad:
    def __init__(self, dev, case, exp=None, weights="pow2"):
        self.name, self.B, self.Cin, self.Cout, self.H, self.k, self.s, self.p, self.route = case
        seed = XE.case_seed("grad " + self.name)
        k, T = self.k, self.k * self.k
        self.Ho, _ = XE.out_hw(self.H, self.H, k, k, self.s, self.p, 1)
        gshape = (self.B, self.Cout, self.Ho, self.Ho)
        self.ksteps = T * (ops.triple_ld_bytes(self.Cout, 16, 2) // 4) // 8
        if weights == "pow2":
            self.g = G.grad_ints(gshape, XE.GRAD_AMP, seed, dev, exp=exp)
            exps, zero_taps, _ = XE.tap_design(T, self.Cout, "mid", x_absmax=float(XE.GRAD_AMP), bias_quanta=0, Cout=self.Cout)
            self.w = XE.pow2_tap_weight((self.Cout, self.Cin, k, k), exps, seed + 1, dev, zero_taps)
            self.alpha64 = XE.designed_alpha(exps, zero_taps, dev)
            self.ts = _tap_scales(self.w, self.alpha64, None, dev, self.name)
            ok, why = XE.proves_exact_taps(self.ts.alpha, self.Cout, grad=self.g, reverse=True)
            assert ok, (self.name, why)
        else:
            self.g = torch.randn(gshape, generator=G._gen(seed, dev), device=dev).contiguous(memory_format=torch.channels_last)
            self.w = XE.gauss_tap_weight((self.Cout, self.Cin, k, k), seed + 1, dev, **weights)
            self.w[self.Cout // 2, self.Cin // 3, k // 2, k // 2] = 0.0
            self.alpha64 = XE.tap_alpha64(self.w)
            self.ts = ops.xnor_tap_prep(self.w)

    def run(self):
        gx = ops.conv2d_grad_input_taps((self.B, self.Cin, self.H, self.H), self.w, self.g, self.ts.bwd, self.s, self.p, 1)
        assert gx is not None
        return gx


def _grad_exps(name):
    """Both exponents at the small shapes; one each at the batch-256 layer shapes."""
    if not name.startswith("alexnet"):
        return XE.GRAD_EXPS
    return (XE.GRAD_EXPS[0],) if name in ("alexnet.conv2", "alexnet.conv4") else (XE.GRAD_EXPS[1],)


GRAD_PARAMS = [(c, e) for c in XE.GRAD_CASES for e in _grad_exps(c[0])]


@pytest.mark.parametrize("case,exp", GRAD_PARAMS, ids=[f"{c[0]}-e{e}" for c, e in GRAD_PARAMS])
def test_grad_input_is_bit_exact_on_designed_operands(dev, case, exp):
    gd = Grad(dev, case, exp)
    ref, _ = XE.xnor_grad_input64(gd.g, gd.w, (gd.H, gd.H), gd.s, gd.p, alpha=gd.alpha64, bound=False)
    want = XE.to_f32_exact(ref, gd.name)
    label = f"{gd.route}<ElemF16Taps>"
    gx = traced(gd.run, label, f"grad {gd.name}")
    msg = XE.value_report(gx, want, what=f"grad_x {gd.name} 2^{exp}")
    assert not msg, msg
    record(label, "float", f"grad {gd.name} 2^{exp}")


# ---- (e) Gaussian data, per element ---------------------------------------------------------------------------------------------

# "equal": N(0, 0.05), alphas agree to about 0.5 %; "decades": one scale per tap over six decades and one tap (the middle one, or
# the last) at 2^-60 of the others
WEIGHT_SETS = ("equal", "decades")


def _weights_kw(kind, T, last=False):
    if kind == "equal":
        return {}
    return {"decades": 6, "tiny_tap": (T - 1 if last else T // 2) if T > 1 else None}


def _ratio(case, got, ref, B, ksteps, taps):
    r = XE.worst_ratio(got, ref, XE.horner_bound(B, ksteps, taps))
    RATIOS[case] = r
    print(f"{case}: worst err / bound = {r:.4f} (S = {ksteps} k-steps, T = {taps} taps)")
    return r


GAUSS_FWD = ["c256/valid", "c200/padded", "rows384/padded", "odd3/5x5/padded", "odd9/valid", "stride2", "dil2/padded", "1x1"]


@pytest.mark.parametrize("kind", list(WEIGHT_SETS))
@pytest.mark.parametrize("name", GAUSS_FWD)
def test_forward_gaussian_within_the_per_element_bound(dev, name, kind):
    case = next(c for c in XE.FWD_CASES if c[0] == name)
    T = case[5] ** 2
    f = Fwd(dev, case, weights=_weights_kw(kind, T, last=name in ("odd9/valid", "stride2")))
    ref, B = XE.xnor_conv64(f.x, f.w, f.bias, f.s, f.p, f.d)
    label = f"{f.float_route}<ElemFp4Taps>"
    y = traced(f.run, label, f"gauss {name}", f.named())
    y = y.view(f.B, f.Ho, f.Wo, f.Cout).permute(0, 3, 1, 2)
    assert _ratio(f"fwd {name} {kind}", y, ref, B, f.ksteps, T) <= 1.0


@pytest.mark.parametrize("kind", list(WEIGHT_SETS))
@pytest.mark.parametrize("name", ["tiny", "stride2", "5x5", "ragged"])
def test_row_scaled_gaussian_within_the_per_element_bound(dev, name, kind):
    case = next(c for c in XE.ROWS_CASES if c[0] == name)
    T = case[5] ** 2
    r = Rows(dev, case, weights=_weights_kw(kind, T, last=name == "ragged"))
    ref, B = XE.xnor_rows64(r.xs, r.A, r.w, r.bias, r.s, r.p, 1)
    y = traced(r.run, ROWS_ROUTE, f"gauss rows {name}")
    assert _ratio(f"rows {name} {kind}", y, ref, B, r.ksteps, T) <= 1.0


@pytest.mark.parametrize("kind", list(WEIGHT_SETS))
@pytest.mark.parametrize("name", ["c128x128", "skinny", "vpp256", "vpp256x192", "cout72", "stride2"])
def test_grad_input_gaussian_within_the_per_element_bound(dev, name, kind):
    case = next(c for c in XE.GRAD_CASES if c[0] == name)
    T = case[5] ** 2
    gd = Grad(dev, case, weights=_weights_kw(kind, T, last=name in ("skinny", "cout72")))
    ref, B = XE.xnor_grad_input64(gd.g, gd.w, (gd.H, gd.H), gd.s, gd.p)
    gx = traced(gd.run, f"{gd.route}<ElemF16Taps>", f"gauss grad {name}")
    assert _ratio(f"grad {name} {kind}", gx, ref, B, gd.ksteps, T) <= 1.0


# ---- (f) closure ----------------------------------------------------------------------------------------------------------------

# what select_conv_taps (csrc/tile_select.h) can return.  Un-padded planes (`valid`): the three small-M tiles, then by column tile
# width; every one of them carries the float and both threshold epilogues.  Bounds-checked taps: the float result of a grid
# under 200 tiles takes ConvSkinny / Conv128x128 (`!epi.alpha && epi.mode == 0`), everything else the ping-pong tiles / Conv64.
_VALID = ("ConvV128x128", "ConvV128x64", "ConvVSkinny", "ConvVPP256", "ConvVPP192", "ConvVPP256x192", "ConvVPP128", "ConvV64")
_PADDED_ANY = ("ConvPP256", "ConvPP192", "ConvPP256x192", "ConvPP128", "Conv64")
_PADDED_FLOAT = ("ConvSkinny", "Conv128x128")
EXPECTED = sorted(
    [f"{c}<ElemFp4Taps>/{form}" for c in _VALID + _PADDED_ANY for form in ("float", "bits", "nib")]
    + [f"{c}<ElemFp4Taps>/float" for c in _PADDED_FLOAT]
    + [f"{c}<ElemF16Taps>/float" for c in _VALID + _PADDED_ANY + _PADDED_FLOAT]
    + [f"{ROWS_ROUTE}/float"])


def test_every_tap_configuration_was_compared():
    if not COVERED:
        pytest.skip("run the whole module: the cases above record the configurations they compared")
    print("\n".join(["tap-conv configurations compared with the float64 reference:"]
                    + [f"  {c}: {', '.join(COVERED.get(c, ['-'])[:4])}" for c in EXPECTED]))
    missing = [c for c in EXPECTED if c not in COVERED]
    assert not missing, missing


def _tap_instances(fn):
    _, seen = profiled(fn)
    return {k for k in seen if "Taps" in k}


def test_every_tap_kernel_of_the_batch_256_model_passes_was_compared(dev):
    if not COVERED:
        pytest.skip("run the whole module: the cases above record the configurations they compared")
    import bench_models
    import torch.nn.functional as F
    from pytorch_quantize_impls_amd.functions import _fused
    from pytorch_quantize_impls_amd.layers import LinearXNOR, XNORConv2d
    covered = {k.rsplit("/", 1)[0] for k in COVERED}
    B = 256
    torch.manual_seed(0)
    model = bench_models.alexnet_xnor()
    for mod in model.modules():
        if isinstance(mod, (XNORConv2d, LinearXNOR)):
            mod.weight.data.normal_(0, 0.05)
            mod.bias.data.zero_()
    bench_models.randomize_bn(model, 0)
    model = model.to(dev).to(memory_format=torch.channels_last).train()
    x = torch.randn(B, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 10, (B,), device=dev)
    _fused.LIBRARY_PATHS.clear()

    def step():
        F.nll_loss(model(x), t).backward()

    seen = {"training step": _tap_instances(step)}
    assert not _fused.LIBRARY_PATHS, dict(_fused.LIBRARY_PATHS)
    model.zero_grad(set_to_none=True)
    model.eval()

    def deferred():
        with torch.no_grad():
            return model(x).sum().item()

    seen["eval deferred forward"] = _tap_instances(deferred)
    del model
    torch.cuda.empty_cache()
    # (the layer class forces quant_input=False like upstream: the function is called directly, at conv3's shape)
    from pytorch_quantize_impls_amd.functions import xnor_connect
    op = xnor_connect.XNORConv2d([0, 1], True, 1, 1, 1, 1)
    wq = (torch.randn(1152, 576, 3, 3, device=dev) * 0.05).requires_grad_()
    bq = torch.zeros(1152, device=dev, requires_grad=True)
    xq = torch.randn(B, 576, 13, 13, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_()

    def qstep():
        op.apply(xq, wq, bq).square().mean().backward()

    seen["quant_input step"] = _tap_instances(qstep)
    lines, missing = [], []
    for what, ks in seen.items():
        assert ks, f"{what}: no tap kernel ran"
        for k in sorted(ks):
            cases = [c for key, cs in COVERED.items() if key.rsplit("/", 1)[0] == k for c in cs]
            lines.append(f"  {what}: {k} <- {', '.join(cases[:3]) if cases else 'NOT COMPARED'}")
            if k not in covered:
                missing.append((what, k))
    worst = max(PEAK.items(), key=lambda kv: kv[1]) if PEAK else ("-", 0)
    print("\n".join(["tap kernels of the batch-256 passes:"] + lines))
    print(f"peak device memory of a case: {worst[1] / 2**30:.2f} GiB ({worst[0]}); module time so far {time.perf_counter() - T0:.0f} s")
    if RATIOS:
        print("worst err / bound of the Gaussian cases: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))
    assert not missing, missing
