"""bf16 / fp16 activations of the sign layers on the packed HIP routes (run with -m gpu on an MI355X).

Everything goes through the public layers / quantiser modules and the C-ABI.  The references are the fixtures of
tests/golden/make_golden_half.py (the reference's layers on CPU half tensors; tests/test_half_cpu.py shows they are
round-to-nearest-even of fl32(exact sum + bias)) and fp64 values computed here from the same inputs.

Gradient bars (one correct rounding on top of the fp32 routes' normalised 1e-5 bar):
    bf16: |ours - exact| <= 2^-8  |exact| + 1e-5 max|exact|              (8 significant bits: half an ulp is at most 2^-8 |x|)
    fp16: |ours - exact| <= 2^-11 |exact| + 2^-25 + 1e-5 max|exact|      (11 bits; 2^-25 is half a subnormal step)
and against the reference's own half gradients no element differs by more than one ulp (both are one rounding from exact).
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _half_cases as HC
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib, ops  # noqa: E402
from pytorch_quantize_impls_amd.functions import BinaryConnect, TernaryConnect, _fused  # noqa: E402
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, LinearBin, LinearTer  # noqa: E402

LIN = {"binary": LinearBin, "ternary": LinearTer}
CONV = {"binary": BinConv2d, "ternary": TerConv2d}
PACKERS_H = ("qt_sign_pack_h", "qt_sign_pack_nib_h", "qt_pack_pair_nib_h", "qt_ternary_pack_h", "qt_ternary_pack_nib_h")
CONTRACTIONS = ("qt_xnor_gemm", "qt_tern_gemm", "qt_nib_gemm_h", "qt_conv2d_implicit_h")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "golden_half_v1.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def gold_hashes():
    with open(os.path.join(GOLDEN_DIR, "golden_half_hashes.json")) as fh:
        return json.load(fh)["sha256_of_uint16_bits"]


def lib_paths():
    return sum(_fused.LIBRARY_PATHS.values())


def counts():
    return dict(_lib.call_counts)


def ran(before, names):
    return sum(_lib.call_counts[n] - before.get(n, 0) for n in names)


def make_linear(case, kind, name, dev):
    x, w, b = HC.linear_inputs(case, kind, name)
    lay = LIN[kind](case["K"], case["N"], bias=b is not None).to(dev).to(HC.DTYPES[name])
    lay.weight.data.copy_(w.to(dev))
    if b is not None:
        lay.bias.data.copy_(b.to(dev))
    return lay, x, w, b


def make_conv(case, kind, name, dev):
    x, w, b = HC.conv_inputs(case, kind, name)
    lay = CONV[kind](case["Cin"], case["Cout"], case["k"], stride=case["stride"], padding=case["pad"],
                     bias=b is not None).to(dev).to(HC.DTYPES[name])
    lay.weight.data.copy_(w.to(dev))
    if b is not None:
        lay.bias.data.copy_(b.to(dev))
    return lay, x, w, b


def forward_modes(lay, xd):
    """(mode, train?, result) for tagged / hinted / detected activations in training and eval mode, without autograd."""
    for mode in ("tagged", "hinted", "detected"):
        lay.binary_input = True if mode == "hinted" else None
        for train in (True, False):
            lay.train(train)
            xin = BinaryConnect()(xd * 0.75) if mode == "tagged" else xd      # 0.75 x: real-valued, same signs
            with torch.no_grad():
                yield mode, train, lay(xin)
    lay.train(True)
    lay.binary_input = None


# ---- case 1: quantiser edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_quantiser_edges(dev, gold, name):
    dt = HC.DTYPES[name]
    e = gold[f"edge_{name}_in"]
    for shape in ((-1,), (2, -1), (-1, 8)):            # 1-D (no tag), ragged rows and whole 16-byte vectors
        for q, mod in (("bin", BinaryConnect()), ("ter", TernaryConnect())):
            x = HC.from_bits(e, dt).reshape(shape).to(dev).requires_grad_(True)
            before = counts()
            y = mod(x)
            assert y.dtype == dt
            assert np.array_equal(HC.bits(y).ravel() & (0xFFFF if q == "bin" else 0x7FFF),
                                  gold[f"edge_{name}_{q}_out"] & (0xFFFF if q == "bin" else 0x7FFF)), (q, shape)
            nz = (gold[f"edge_{name}_{q}_out"] & 0x7FFF) != 0
            assert np.array_equal(HC.bits(y).ravel()[nz], gold[f"edge_{name}_{q}_out"][nz])       # (the sign of a zero is free)
            y.backward(torch.ones_like(y))
            assert x.grad.dtype == dt and np.array_equal(HC.bits(x.grad).ravel(), gold[f"edge_{name}_{q}_mask"]), (q, shape)
            if q == "bin" and len(shape) == 2:
                assert ran(before, ("qt_sign_pack_h",)) == 1, "the half quantiser did not run the half packer"
    # the C-ABI +-1 check and the packers on the edge vector itself
    x = HC.from_bits(e, dt).to(dev)
    assert not ops.is_pm1(x)
    _, one, half, inf, _ = HC.FORMAT[name]
    pm = HC.from_bits(np.array([one, one | 0x8000] * 36 + [one], dtype=np.uint16), dt).to(dev)
    assert ops.is_pm1(pm) and ops.is_pm1(pm[1:])                    # (the second view is not 16-byte aligned)
    bad = pm.clone()
    bad[-1] = 0.5
    assert not ops.is_pm1(bad)
    ei = e.astype(np.int64)
    mag, neg = ei & 0x7FFF, (ei >> 15) == 1
    is_neg = neg & (mag != 0) & (mag <= inf)
    planes, _ = ops.sign_pack(x.reshape(1, -1))
    word = planes.sign.cpu().numpy().view(np.uint32)[0]
    got = np.array([(int(word[i // 32]) >> (i % 32)) & 1 for i in range(len(e))], dtype=bool)
    assert np.array_equal(got, is_neg)
    nib = ops.ternary_pack_nib(x.reshape(1, -1)).words.cpu().numpy().view(np.uint32)[0]
    gotn = np.array([(int(nib[i // 8]) >> (4 * (i % 8))) & 0xF for i in range(len(e))])
    pos = (mag > inf) | (~neg & (mag >= half))
    tneg = neg & (mag > half) & (mag <= inf)
    assert np.array_equal(gotn, np.where(pos, 0x2, np.where(tneg, 0xA, 0x0)))


# ---- case 2: Linear forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_linear_forward_bits(dev, gold_hashes, name, kind):
    dt = HC.DTYPES[name]
    for case in HC.linear_cases():
        lay, x, w, b = make_linear(case, kind, name, dev)
        key = f"{case['name']}_{kind}_{name}_y"
        before_lib, before = lib_paths(), counts()
        for mode, train, y in forward_modes(lay, x.to(dev)):
            assert y.dtype == dt and tuple(y.shape) == (case["B"], case["N"])
            assert HC.digest(y) == gold_hashes[key], (key, mode, train)
        assert lib_paths() == before_lib, f"{key}: a dense-library path was taken"
        assert ran(before, PACKERS_H) > 0 and ran(before, CONTRACTIONS) > 0, key


def test_c2_shape_bits_and_route(dev, gold_hashes):
    """4096^3 in bf16: both operands from ONE half pack launch, the matrix-core GEMM stores bf16 itself."""
    x, w = HC.c2_inputs()
    lay = LinearBin(4096, 4096, bias=False).to(dev).to(torch.bfloat16)
    lay.weight.data.copy_(w.to(dev))
    lay.binary_input = True
    before_lib, before = lib_paths(), counts()
    with torch.no_grad():
        y = lay(x.to(dev))
    assert y.dtype == torch.bfloat16 and HC.digest(y) == gold_hashes["c2_4096_bf16_y"]
    assert lib_paths() == before_lib
    assert ran(before, ("qt_pack_pair_nib_h",)) == 1 and ran(before, ("qt_nib_gemm_h",)) == 1
    assert ran(before, ("qt_nib_gemm", "qt_pack_pair_nib_f32")) == 0


# ---- case 3: Conv2d forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_conv_forward_bits(dev, gold_hashes, name, kind):
    dt = HC.DTYPES[name]
    for case in HC.conv_cases():
        lay, x, w, b = make_conv(case, kind, name, dev)
        key = f"{case['name']}_{kind}_{name}_y"
        for cl in (False, True):
            xd = x.to(dev).contiguous(memory_format=torch.channels_last) if cl else x.to(dev)
            before_lib, before = lib_paths(), counts()
            for mode, train, y in forward_modes(lay, xd):
                assert y.dtype == dt
                assert HC.digest(y) == gold_hashes[key], (key, mode, train, cl)
            assert lib_paths() == before_lib, f"{key}: a dense-library path was taken"
            assert ran(before, ("qt_sign_pack_nib_h", "qt_sign_pack_h")) > 0 and ran(before, ("qt_conv2d_implicit_h",)) > 0, key


# ---- activations that are not +-1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_real_valued_half_activation_keeps_the_counted_torch_expression(dev, name):
    dt = HC.DTYPES[name]
    torch.manual_seed(3)
    lin = LinearBin(64, 16).to(dev).to(dt)
    x = torch.randn(8, 64, device=dev).to(dt)
    before = lib_paths()
    with torch.no_grad():
        y = lin(x)
    assert lib_paths() > before
    wq = torch.where(lin.weight.data < 0, -1.0, 1.0).to(dt)
    assert torch.equal(y, F.linear(x, wq, lin.bias))
    conv = BinConv2d(32, 16, 3, padding=1).to(dev).to(dt)
    xc = torch.randn(2, 32, 6, 6, device=dev).to(dt)
    before = lib_paths()
    with torch.no_grad():
        yc = conv(xc)
    assert lib_paths() > before
    wq = torch.where(conv.weight.data < 0, -1.0, 1.0).to(dt)
    assert torch.equal(yc, F.conv2d(xc, wq, conv.bias, 1, 1))


@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_broken_pm1_assumption_poisons_the_half_result(dev, name):
    """DETECT_MODE = "remember": a remembered "+-1" verdict and then a real-valued tensor — the device flag rides in through the
    bias and the whole result is NaN, as on the fp32 route; reset_detection() recovers."""
    dt = HC.DTYPES[name]
    lin = LinearBin(96, 24).to(dev).to(dt).eval()
    lin32 = LinearBin(96, 24).to(dev).eval()
    x = torch.from_numpy(HC.synth.pm1(77, (16, 96))).to(dev)
    _fused.reset_detection()
    prev = _fused.DETECT_MODE
    _fused.DETECT_MODE = "remember"
    try:
        with torch.no_grad():
            good = lin(x.to(dt))
            good32 = lin32(x)
            assert not torch.isnan(good).any()
            broken = x.clone()
            broken[3, 5] = 0.25
            nan_h, nan_32 = lin(broken.to(dt)), lin32(broken)
            assert nan_h.dtype == dt and torch.equal(torch.isnan(nan_h), torch.isnan(nan_32)) and torch.isnan(nan_h).all()
            _fused.reset_detection(lin.weight)
            before = lib_paths()
            ok = lin(broken.to(dt))                      # asked again: not +-1 -> the counted torch expression
            assert lib_paths() > before and not torch.isnan(ok).any()
    finally:
        _fused.DETECT_MODE = prev
        _fused.reset_detection()


# ---- case 5: gradients -----------------------------------------------------------------------------------------------------
def grad_bar(name, exact):
    a = exact.abs()
    if name == "bf16":
        return 2.0 ** -8 * a + 1e-5 * a.max()
    return 2.0 ** -11 * a + 2.0 ** -25 + 1e-5 * a.max()


def check_grad(label, name, ours, exact, ref_bits, report, ref_digest=None):
    """The fp64 bar; with the reference's bit patterns also the one-ulp comparison (report: label, differing elements, elements);
    with only its digest, whether the whole tensor is bit-identical (report: label, None if identical else -1, elements)."""
    dt = HC.DTYPES[name]
    assert ours.dtype == dt, label
    o = ours.detach().cpu().double()
    err = (o - exact).abs()
    bar = grad_bar(name, exact)
    worst = float((err - bar).max())
    print(f"{label}: max|ours - exact| = {float(err.max()):.3e}, worst margin to the bar = {worst:.3e}")
    assert worst <= 0, label
    if ref_bits is not None:
        r = HC.from_bits(ref_bits, dt).reshape(o.shape).double()
        d = (o - r).abs()
        n = int((d != 0).sum())
        report.append((label, n, o.numel()))
        assert bool((d <= HC.ulp_of(torch.maximum(o.abs(), r.abs()), name)).all()), f"{label}: more than one ulp from the reference's half gradient"
    elif ref_digest is not None:
        report.append((label, None if HC.digest(ours) == ref_digest else -1, o.numel()))


def summarise(report):
    """Prints how the gradients compare with the reference's own half gradients; at least one tensor must have been compared."""
    by_bits = [r for r in report if r[1] is not None and r[1] >= 0]
    by_digest = [r for r in report if r[1] is None or r[1] < 0]
    print(f"compared element by element with the reference's half gradient (one-ulp bar): {len(by_bits)} tensors, "
          f"{sum(t for _, _, t in by_bits)} elements, {sum(n for _, n, _ in by_bits)} differ: {[(l, n) for l, n, _ in by_bits if n]}")
    print(f"compared by digest only (too large to store): {len(by_digest)} tensors, bit-identical: "
          f"{sum(1 for r in by_digest if r[1] is None)}; not identical: {[l for l, n, _ in by_digest if n is not None]}")
    assert by_bits, "no gradient was compared with the reference's"


@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_linear_gradients(dev, gold, gold_hashes, name, kind):
    dt = HC.DTYPES[name]
    report = []
    for case in HC.linear_cases():
        assert case["grads"]
        for mode in ("hinted", "tagged"):
            lay, x, w, b = make_linear(case, kind, name, dev)
            lay.binary_input = True if mode == "hinted" else None
            g = HC.grad_out(case["seed"], (case["B"], case["N"]), name)
            xd = x.to(dev).requires_grad_(True)
            before_lib = lib_paths()
            xin = BinaryConnect()(xd) if mode == "tagged" else xd          # (x is +-1: the quantiser's STE passes g unchanged)
            y = lay(xin)
            y.backward(g.to(dev))
            assert lib_paths() == before_lib, f"{case['name']}: a dense-library path was taken"
            wq = HC.quantise(w, kind).double()
            gx = g.double() @ wq
            keep = (w.double().abs() <= 1.001)
            gw_unmasked = g.double().t() @ x.double()
            key = f"{case['name']}_{kind}_{name}"
            ref = (lambda s: gold[f"{key}_{s}"] if f"{key}_{s}" in gold.files else None) if mode == "hinted" else (lambda s: None)
            dig = (lambda s: gold_hashes.get(f"{key}_{s}")) if mode == "hinted" else (lambda s: None)
            check_grad(f"{key} {mode} grad_input", name, xd.grad, gx, ref("gx"), report, dig("gx"))
            check_grad(f"{key} {mode} grad_weight", name, lay.weight.grad, gw_unmasked * keep, ref("gw"), report, dig("gw"))
            masked = (~keep) & (gw_unmasked != 0)
            assert bool((lay.weight.grad.cpu()[masked] == 0).all()) and bool((lay.weight.grad.cpu()[keep & (gw_unmasked.abs() > 1e-3)] != 0).all())
            if b is not None:
                check_grad(f"{key} {mode} grad_bias", name, lay.bias.grad, g.double().sum(0), ref("gb"), report, dig("gb"))
            else:
                assert lay.bias is None
    summarise(report)


@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_conv_gradients(dev, gold, gold_hashes, name, kind):
    """hinted (binary_input=True), tagged (BinaryConnect in front of a channels-last activation: NHWC planes, its STE backward in
    half) and detected (the forward's device check tells the backward that the activation is +-1)."""
    report = []
    for case in HC.conv_cases():
        if not case["grads"]:
            continue
        Ho = (case["H"] + 2 * case["pad"] - case["k"]) // case["stride"] + 1
        g = HC.grad_out(case["seed"], (case["B"], case["Cout"], Ho, Ho), name)
        x, w, b = HC.conv_inputs(case, kind, name)
        x64 = x.double().requires_grad_(True)
        wq64 = HC.quantise(w, kind).double().requires_grad_(True)
        F.conv2d(x64, wq64, None, case["stride"], case["pad"]).backward(g.double())
        keep = (w.double().abs() <= 1.001)
        key = f"{case['name']}_{kind}_{name}"
        for mode in ("hinted", "tagged", "detected"):
            lay, _, _, _ = make_conv(case, kind, name, dev)
            lay.binary_input = True if mode == "hinted" else None
            xd = x.to(dev)
            if mode == "tagged":
                xd = xd.contiguous(memory_format=torch.channels_last)
            xd.requires_grad_(True)
            before_lib, before = lib_paths(), counts()
            xin = BinaryConnect()(xd) if mode == "tagged" else xd          # (x is +-1: the quantiser's STE passes g unchanged)
            lay(xin).backward(g.to(dev))
            assert lib_paths() == before_lib, f"{case['name']} {mode}: a dense-library path was taken"
            if mode == "tagged":
                assert ran(before, ("qt_sign_pack_nib_h",)) == (1 if kind == "binary" else 0), \
                    "the quantiser's NHWC planes were not used (only the binary weight goes through qt_sign_pack_nib_h)"
            first = mode == "hinted"
            ref = (lambda s: gold[f"{key}_{s}"] if f"{key}_{s}" in gold.files else None) if first else (lambda s: None)
            dig = (lambda s: gold_hashes.get(f"{key}_{s}")) if first else (lambda s: None)
            check_grad(f"{key} {mode} grad_input", name, xd.grad, x64.grad, ref("gx"), report, dig("gx"))
            check_grad(f"{key} {mode} grad_weight", name, lay.weight.grad, wq64.grad * keep, ref("gw"), report, dig("gw"))
            masked = (~keep) & (wq64.grad != 0)
            assert bool((lay.weight.grad.cpu()[masked] == 0).all())
            if b is not None:
                check_grad(f"{key} {mode} grad_bias", name, lay.bias.grad, g.double().sum((0, 2, 3)), ref("gb"), report, dig("gb"))
    summarise(report)


# ---- stochastic weight quantisers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_stochastic_layers_pack_their_explicit_image(dev, name, kind):
    """deterministic=False: the quantiser keeps its torch expression, its explicit image (weight_q) goes through the half
    packers; forward = RNE(exact sum with that image + bias), backward on the saved draw, no library path."""
    dt = HC.DTYPES[name]
    from pytorch_quantize_impls_amd.functions.binary_connect import stochastic_binarize
    from pytorch_quantize_impls_amd.functions.terner_connect import stochastic_ternarize
    draw = stochastic_binarize if kind == "binary" else stochastic_ternarize
    lcase = [c for c in HC.linear_cases() if c["name"] == "lin_K96_B128_N96"][0]
    ccase = HC.conv_cases()[0]
    for which, case in (("lin", lcase), ("conv", ccase)):
        if which == "lin":
            x, w, b = HC.linear_inputs(case, kind, name)
            lay = LIN[kind](case["K"], case["N"], bias=b is not None, deterministic=False)
        else:
            x, w, b = HC.conv_inputs(case, kind, name)
            lay = CONV[kind](case["Cin"], case["Cout"], case["k"], stride=case["stride"], padding=case["pad"], bias=b is not None,
                             deterministic=False)
        lay = lay.to(dev).to(dt)
        lay.weight.data.copy_((w * 0.6).to(dev))                       # inside (-1, 1): the draws are not all forced
        if b is not None:
            lay.bias.data.copy_(b.to(dev))
        lay.binary_input = True
        xd = x.to(dev).requires_grad_(True)
        before_lib, before = lib_paths(), counts()
        torch.manual_seed(1234)
        y = lay(xd)
        torch.manual_seed(1234)
        wq = draw(lay.weight.detach(), torch.rand_like(lay.weight.detach())).cpu()
        assert 0 < float((wq != HC.quantise(lay.weight.detach().cpu(), kind)).double().mean()), "the draw equals the deterministic image"
        exact = HC.exact_linear(x, wq, b) if which == "lin" else HC.exact_conv(x, wq, b, case["stride"], case["pad"])
        assert y.dtype == dt and HC.digest(y) == HC.digest(HC.rne_of_fl32(exact, dt)), (which, kind)
        g = HC.grad_out(case["seed"], tuple(y.shape), name)
        y.backward(g.to(dev))
        assert lib_paths() == before_lib and ran(before, PACKERS_H) > 0 and ran(before, CONTRACTIONS) == 1
        if which == "lin":
            gx = g.double() @ wq.double()
        else:
            x64 = x.double().requires_grad_(True)
            F.conv2d(x64, wq.double(), None, case["stride"], case["pad"]).backward(g.double())
            gx = x64.grad
        check_grad(f"stochastic {which} {kind} {name} grad_input", name, xd.grad, gx, None, [])
        assert lay.weight.grad.dtype == dt


# ---- autocast --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_autocast_fp32_layers_behind_a_half_quantiser(dev, gold_hashes, name):
    dt = HC.DTYPES[name]
    lcase = [c for c in HC.linear_cases() if c["name"] == "lin_K96_B128_N96"][0]
    ccase = HC.conv_cases()[0]
    for case, make, cls_key in ((lcase, HC.linear_inputs, "lin"), (ccase, HC.conv_inputs, "conv")):
        x, w, b = make(case, "binary", name)
        if cls_key == "lin":
            lay = LinearBin(case["K"], case["N"], bias=b is not None).to(dev)
        else:
            lay = BinConv2d(case["Cin"], case["Cout"], case["k"], stride=case["stride"], padding=case["pad"], bias=b is not None).to(dev)
        lay.weight.data.copy_(w.float().to(dev))                # an fp32 model holding the same (half-representable) values
        if b is not None:
            lay.bias.data.copy_(b.float().to(dev))
        xd = (x.to(dev) * 0.75)
        before_lib, before = lib_paths(), counts()
        with torch.autocast("cuda", dtype=dt):
            y = lay(BinaryConnect()(xd))
        assert y.dtype == dt and HC.digest(y) == gold_hashes[f"{case['name']}_binary_{name}_y"]
        assert lib_paths() == before_lib and ran(before, CONTRACTIONS) == 1
        y.float().sum().backward()
        assert lay.weight.grad.dtype == torch.float32 and (lay.bias is None or lay.bias.grad.dtype == torch.float32)
        assert lib_paths() == before_lib
        with pytest.raises(RuntimeError):
            lay(BinaryConnect()(xd))                            # the same mixed-dtype call outside autocast raises, as F.linear does


def test_autocast_to_another_half_dtype_keeps_the_reference_expression(dev):
    """A bf16 model under fp16 autocast: the reference expression casts both operands to the autocast dtype, so the packed
    route declines and the counted torch expression returns fp16 (as before this route existed)."""
    lin = LinearBin(96, 24).to(dev).bfloat16()
    x = torch.from_numpy(HC.synth.pm1(0x9100, (16, 96))).to(dev).bfloat16()
    lin.binary_input = True
    before = lib_paths()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        y = lin(x)
    wq = torch.where(lin.weight.data < 0, -1.0, 1.0)
    assert y.dtype == torch.float16 and lib_paths() > before
    assert torch.equal(y, F.linear(x.half(), wq.half(), lin.bias.data.half()))


# ---- eval swap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_eval_swap_round_trip_and_replanning(dev, gold_hashes, name):
    dt = HC.DTYPES[name]
    case = [c for c in HC.linear_cases() if c["name"] == "lin_K96_B128_N96"][0]
    for kind in HC.KINDS:
        lay, x, w, b = make_linear(case, kind, name, dev)
        key = f"{case['name']}_{kind}_{name}_y"
        lay.binary_input = True
        lay.eval()
        assert lay.weight.dtype == dt and torch.equal(lay.weight.data.cpu(), HC.quantise(w, kind))
        with torch.no_grad():
            assert HC.digest(lay(x.to(dev))) == gold_hashes[key]
            before = counts()
            assert HC.digest(lay(x.to(dev))) == gold_hashes[key]
        assert ran(before, ("qt_sign_pack_h", "qt_ternary_pack_h")) == 1, "the eval-mode weight planes were not cached"
        lay.train()
        assert lay.weight.dtype == dt and np.array_equal(HC.bits(lay.weight.data), HC.bits(w)), "the half weight did not come back bit for bit"
        # a weight update, then eval again: the planes are re-packed from the new image
        with torch.no_grad():
            lay.weight.neg_()
        lay.eval()
        with torch.no_grad():
            y2 = lay(x.to(dev))
        want = HC.rne_of_fl32(HC.exact_linear(x, HC.quantise(-w, kind), b), dt)
        assert HC.digest(y2) == HC.digest(want)


# ---- a two-block BinaryNet-style network -----------------------------------------------------------------------------------
def _binary_net(dev, dt):
    torch.manual_seed(11)
    net = torch.nn.Sequential(
        BinConv2d(32, 64, 3, padding=1), torch.nn.MaxPool2d(2), torch.nn.BatchNorm2d(64), torch.nn.Hardtanh(), BinaryConnect(),
        BinConv2d(64, 64, 3, padding=1), torch.nn.MaxPool2d(2), torch.nn.BatchNorm2d(64), torch.nn.Hardtanh(), BinaryConnect(),
        torch.nn.Flatten(), LinearBin(64 * 4 * 4, 10))
    for m in net:
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.normal_(1.0, 0.3)
            m.bias.data.normal_(0.0, 0.3)
            m.running_mean.normal_(0.0, 8.0)
            m.running_var.uniform_(20.0, 60.0)
    return net.to(dev).to(dt)


def _run_by_expression(net, x, record=None):
    """The same graph, module by module, the sign layers by their torch expression on the device (the dense library)."""
    for m in net:
        if isinstance(m, (BinConv2d, LinearBin)):
            wq = torch.where(m.weight.detach() < 0, -1.0, 1.0).to(x.dtype) if m.training else m.weight.detach()
            x = F.linear(x, wq, m.bias) if isinstance(m, LinearBin) else F.conv2d(x, wq, m.bias, m.stride, m.padding)
        else:
            x = m(x)
    return x


def test_two_block_binary_net_bf16(dev):
    dt = torch.bfloat16
    net = _binary_net(dev, dt)
    x = torch.from_numpy(HC.synth.pm1(0x9001, (8, 32, 16, 16))).to(dev).to(dt)
    # eval
    net.eval()
    before_lib = lib_paths()
    with torch.no_grad():
        y = net(x)
    assert lib_paths() == before_lib and y.dtype == dt
    with torch.no_grad():
        assert torch.equal(y, _run_by_expression(net, x)), "eval forward differs from the device's torch expression"
    # train: forward against the expression graph (same BatchNorm statistics: both start from the same buffers)
    net.train()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    acts, xi = [], x.clone().requires_grad_(True)
    h = xi
    before_lib = lib_paths()
    for m in net:
        if isinstance(m, (BinConv2d, LinearBin)):
            hin = h
            hin.retain_grad()
            h = m(hin)
            h.retain_grad()
            acts.append((m, hin, h))
        else:
            h = m(h)
    y = h
    g = torch.from_numpy(HC.synth.normal(0x9002, tuple(y.shape))).to(dev).to(dt)
    y.backward(g)
    assert lib_paths() == before_lib, "a dense-library path was taken in training mode"
    net.load_state_dict(state)
    with torch.no_grad():
        assert torch.equal(y, _run_by_expression(net, x)), "train forward differs from the device's torch expression"
    # backward, module by module: every sign layer's gradients against fp64 from ITS inputs and ITS incoming gradient
    for m, hin, hout in acts:
        gi, xi64 = hout.grad.cpu().double(), hin.detach().cpu().double().requires_grad_(True)
        w = m.weight.detach().cpu()
        wq64 = HC.quantise(w, "binary").double().requires_grad_(True)
        out = F.linear(xi64, wq64) if isinstance(m, LinearBin) else F.conv2d(xi64, wq64, None, m.stride, m.padding)
        out.backward(gi)
        keep = w.double().abs() <= 1.001
        lbl = type(m).__name__ + str(tuple(w.shape))
        check_grad(lbl + " grad_input", "bf16", hin.grad, xi64.grad, None, [])
        check_grad(lbl + " grad_weight", "bf16", m.weight.grad, wq64.grad * keep, None, [])
        check_grad(lbl + " grad_bias", "bf16", m.bias.grad, gi.sum(0) if gi.dim() == 2 else gi.sum((0, 2, 3)), None, [])


# ---- steady state ----------------------------------------------------------------------------------------------------------
def test_steady_state_half_forwards_do_not_synchronise(dev):
    """The method of test_gpu_r2.py::test_steady_state_forwards_do_not_synchronise on a half model: tagged activations never ask
    the device; with DETECT_MODE = "remember" an un-tagged +-1 input does not either from the third identical call on."""
    dt = torch.bfloat16
    net = _binary_net(dev, dt).eval()
    x = torch.from_numpy(HC.synth.pm1(0x9003, (8, 32, 16, 16))).to(dev).to(dt)      # un-tagged: the first conv detects
    prev = _fused.DETECT_MODE
    _fused.DETECT_MODE = "remember"
    _fused.reset_detection()
    try:
        with torch.no_grad():
            first = net(x)
            second = net(x)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                third = net(x)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(first, second) and torch.equal(first, third)
    finally:
        _fused.DETECT_MODE = prev
        _fused.reset_detection()
