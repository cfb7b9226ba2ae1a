"""Grouped convs with 16, 24 or 32 channels per group on bf16 / fp16 tensors on the GPU: qt_gmconv2d_h / qt_gmconv2d_grad_input_h
(csrc/gconv_mfma_h.hip) through ops.grouped_mfma_conv2d*, and BinConv2d / TerConv2d on ``_fused.grouped_mfma_half_route``.  The
contract (include/qt_hip.h "Grouped convolution on the matrix cores, half precision"): result = RNE(fp32 sum + bias), the fp32
sum exact below 2^24 units.  References: tests/_gconv_exact.py in float64, the integer rounding of tests/_half_round.py.  Results
are written into sentinel-guarded views; 16-bit patterns are compared with NaN as a class; nothing is waived."""
import copy
import itertools

import numpy as np
import pytest
import torch

import _gconv_exact as G
import _half_round as HR
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d
from pytorch_quantize_impls_amd.utils.graphs import _no_collection_inside

pytestmark = pytest.mark.gpu

FMTS = {"bf16": torch.bfloat16, "fp16": torch.float16}
MAXINT = {"bf16": 255, "fp16": 2047}                      # integers of this magnitude are exact in the dtype
SENTINEL, PAD = 0x5A5A, 67
LAYOUTS = ("nchw", "channels_last")
GEOMS = [(ch, ksp, m) for ch in ((16, 16), (24, 48), (32, 32)) for ksp in ((1, 1, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0))
         for m in ((1, 1), (9, 7), (9, 37)) if m[0] + 2 * ksp[2] >= ksp[0]]          # a 3 x 3 without padding needs a 3 x 3 map
STATS = dict(compared=0, differing=0, worst=0.0)
NEW = ("qt_gmconv2d_h", "qt_gmconv2d_grad_input_h", "qt_gconv2d_grad_weight_h")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    yield torch.device("cuda:0")
    print(f"\n[gconv mfma half] designed elements compared {STATS['compared']}, differing bit patterns {STATS['differing']}, "
          f"worst err / bound on real-valued data {STATS['worst']:.3f}")


def half_of(a, fmt):
    bits = HR.ROUND[fmt](np.asarray(a, dtype=np.float32))
    return bits, HR.UPCAST[fmt](bits)


def to_dev(dev, bits, fmt, layout="nchw", odd=False):
    """The patterns as a device tensor of the dtype; ``odd``: a view one element into its storage (2-byte, not 4-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(FMTS[fmt]).to(dev)
    if layout == "channels_last" and t.dim() == 4:
        t = t.contiguous(memory_format=torch.channels_last)
    if odd:
        flat, (N, C, H, W) = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev), t.shape
        v = flat[1:].view(N, H, W, C).permute(0, 3, 1, 2) if layout == "channels_last" else flat[1:].view(t.shape)
        assert v.data_ptr() % 4 == 2
        return v.copy_(t)
    return t


def bits_of(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def case_of(ch, ksp, m, groups):
    k, s, p = ksp
    return G.Case(cin_g=ch[0], cout_g=ch[1], G=groups, N=2, kernel=(k, k), stride=(s, s), padding=(p, p), dilation=(1, 1), H=m[0], W=m[1])


def run(dev, fmt, c, xb, wdev, b32, gob, kind, lx="nchw", ly="nchw", odd=False):
    """(y bits, gx bits) of the two entries for case ``c``, each written into a sentinel-guarded view."""
    xs, _, ys = c.shapes
    bias = None if b32 is None else torch.from_numpy(b32).to(dev)
    calls = ((ys, ly, lambda o: ops.grouped_mfma_conv2d(to_dev(dev, xb, fmt, lx, odd), wdev, bias, c.stride, c.padding, 1, c.G, kind=kind, out=o)),
             (xs, lx, lambda o: ops.grouped_mfma_conv2d_grad_input(xs, wdev, to_dev(dev, gob, fmt, ly, odd), c.stride, c.padding, 1, c.G, kind=kind, out=o)))
    out = []
    for (N, C, H, W), lay, call in calls:
        buf = torch.full((N * C * H * W + 2 * PAD,), SENTINEL, dtype=torch.int16, device=dev)
        mid = buf.view(FMTS[fmt])[PAD:-PAD]
        view = mid.view(N, H, W, C).permute(0, 3, 1, 2) if lay == "channels_last" else mid.view(N, C, H, W)
        assert call(view) is view and (buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all()
        out.append(bits_of(view))
    return out


def refs64(c, x32, wq, b32, go32):
    with np.errstate(all="ignore"):
        return G.forward(x32, wq, b32, c.G, *c.geom, dtype=np.float64), G.grad_input(go32, wq, c.shapes[0], c.G, *c.geom, dtype=np.float64)


def check(got, want64, fmt, what):
    want = HR.ROUND[fmt](want64.astype(np.float32))                        # exact where the sums are integers below 2^24
    ok, n = HR.same_bits(got, want, fmt)
    STATS["compared"] += want.size
    STATS["differing"] += n
    assert ok, (what, fmt, n, want.size)
    return want


@pytest.mark.parametrize("i", range(len(GEOMS)), ids=lambda i: "i{0[0]}o{0[1]}-k{1[0]}s{1[1]}p{1[2]}-{2[0]}x{2[1]}".format(*GEOMS[i]))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_designed_integers_are_rne_of_the_exact_sum(dev, fmt, i):
    """Layouts, the weight's dtype and G rotate with the case; "ternary" / "raw" on one case each, one on odd-offset views."""
    c, fi, big = case_of(*GEOMS[i], 8 + i % 2), list(FMTS).index(fmt), MAXINT[fmt]
    xs, ws, ys = c.shapes
    kind = "ternary" if i == 4 else ("raw" if i == 7 else "binary")
    xb, x32 = half_of(G._rng(10 * i + fi).randint(-big, big + 1, size=xs), fmt)
    gob, go32 = half_of(G._rng(10 * i + fi + 1).randint(-big, big + 1, size=ys), fmt)
    wb, w32 = half_of(G.small_ints(10 * i + 2, ws) if kind == "raw" else G.weights(10 * i + 2, ws), fmt)
    wq = G.quantize(w32, kind)
    b32 = G.small_ints(10 * i + 3, (ws[0],)) if i % 3 else None
    K = max(c.cin_g, c.cout_g) * c.kernel[0] ** 2
    assert K * big * np.abs(wq).max() + 3 < 2 ** 24                                      # every fp32 sum is exact
    wdev = torch.from_numpy(w32).to(dev) if (i + fi) % 3 == 0 else to_dev(dev, wb, fmt)
    y, gx = run(dev, fmt, c, xb, wdev, b32, gob, kind, LAYOUTS[(i + fi) % 2], LAYOUTS[(i // 2) % 2], odd=i == 10)
    y64, gx64 = refs64(c, x32, wq, b32, go32)
    check(y, y64, fmt, "forward")
    check(gx, gx64, fmt, "grad_input")


@pytest.mark.parametrize("fmt", list(FMTS))
def test_ties_overflow_and_non_finite_inputs(dev, fmt):
    c = case_of((16, 16), (3, 1, 1), (9, 7), 8)
    xs, ws, ys = c.shapes
    ones = half_of(np.ones(ys), fmt)[0]
    # all-ones input and weights: an interior sum is 144; the integer bias moves every channel onto a chosen value
    base = 256 if fmt == "bf16" else 2048
    targets = [base + 1, base + 3, base + 5, base + 7] + ([65519, 65520, -65520, 70000] if fmt == "fp16" else [383, 385, -257, -259])
    b32 = np.array([targets[j % 8] - 144.0 for j in range(ws[0])], dtype=np.float32)
    y, _ = run(dev, fmt, c, half_of(np.ones(xs), fmt)[0], to_dev(dev, half_of(np.ones(ws), fmt)[0], fmt), b32, ones, "raw")
    y64, _ = refs64(c, np.ones(xs), np.ones(ws), b32, np.ones(ys))
    assert np.abs(y64).max() + 144 < 2 ** 24
    back = HR.UPCAST[fmt](check(y, y64, fmt, "ties")).astype(np.float64)
    tie = np.isfinite(back) & (np.abs(back - y64) == HR.half_ulp(y64, fmt))             # the classes the reference alone shows
    assert (tie & (np.abs(back) > np.abs(y64))).any() and (tie & (np.abs(back) < np.abs(y64))).any()
    assert fmt == "bf16" or (np.isinf(back) & (np.abs(y64) == 65520)).any()             # fp16: the first value that overflows
    # a NaN and an inf in the source: every output whose window holds one is non-finite — NaN for the NaN, and for the inf NaN
    # through a zero weight (0 * inf) but +-inf through a +-1 weight (one term: the product is exact) — the others are exact
    xb, _ = half_of(G._rng(5).randint(-MAXINT[fmt], MAXINT[fmt] + 1, size=xs), fmt)
    inf = HR.FORMATS[fmt]["inf"]
    xb[0, 3, 4, 2], xb[1, 20, 0, 6] = inf | 1, inf
    wb, w32 = half_of(G.weights(6, ws), fmt)
    wq = G.quantize(w32, "ternary")
    y, _ = run(dev, fmt, c, xb, to_dev(dev, wb, fmt), None, ones, "ternary", "channels_last")
    hit = []
    for at in ((0, 3, 4, 2), (1, 20, 0, 6)):
        bad = np.zeros(xs)
        bad[at] = 1.0
        hit.append(G.forward(bad, np.ones(ws), None, c.G, *c.geom, dtype=np.float64) > 0)
    want = check(y, refs64(c, HR.UPCAST[fmt](xb), wq, None, np.ones(ys))[0], fmt, "non-finite")
    assert HR.is_nan(y, fmt)[hit[0]].all() and ((y & 0x7FFF) >= inf)[hit[1]].all() and ((y & 0x7FFF) < inf)[~(hit[0] | hit[1])].all()
    assert HR.is_nan(want, fmt)[hit[1]].any() and not HR.is_nan(want, fmt)[hit[1]].all()          # through a zero weight, and not


@pytest.mark.parametrize("i", (4, 15, 30))           # 16 -> 16 3 x 3; 24 -> 48 3 x 3; 32 -> 32 3 x 3 at stride 2 on several tiles
@pytest.mark.parametrize("fmt", list(FMTS))
def test_real_valued_data_within_the_accumulation_bound(dev, fmt, i):
    c = case_of(*GEOMS[i], 8)
    xs, ws, ys = c.shapes
    (xb, x32), (gob, go32) = half_of(G.gauss6(i, xs) / 16, fmt), half_of(G.gauss6(i + 1, ys) / 16, fmt)
    w32, b32 = G.weights(i + 2, ws), (G.gauss6(i + 3, (ws[0],)) / 8).astype(np.float32)
    wq = G.quantize(w32, "binary")
    y, gx = run(dev, fmt, c, xb, torch.from_numpy(w32).to(dev), b32, gob, "binary", LAYOUTS[i % 2])
    y64, gx64 = refs64(c, x32, wq, b32, go32)
    ya, gxa = refs64(c, np.abs(x32), np.abs(wq), np.abs(b32), np.abs(go32))
    for got, want, mag, K in ((y, y64, ya, c.cin_g), (gx, gx64, gxa, c.cout_g)):
        Kp = (K * c.kernel[0] ** 2 + 31) // 32 * 32
        bound = 1.01 * (Kp + 1) * 2.0 ** -23 * mag + HR.half_ulp(want, fmt)
        ratio = float((np.abs(HR.UPCAST[fmt](got).astype(np.float64) - want) / bound).max())
        STATS["worst"] = max(STATS["worst"], ratio)
        print(f"[gconv mfma half] {fmt} case {i}: worst err / bound {ratio:.3f}")
        assert ratio <= 1.0


def test_fp16_subnormal_inputs_are_kept_by_the_matrix_cores(dev):
    """Weight 1 on one tap: the sum is the subnormal input itself.  Pinned to what an MI355X gives: the inputs are NOT flushed."""
    c = case_of((16, 16), (1, 1, 0), (9, 7), 8)
    xs, ws, ys = c.shapes
    xb = G._rng(1).randint(1, 1024, size=xs).astype(np.uint16) | (G._rng(2).randint(0, 2, size=xs) << 15).astype(np.uint16)
    w32 = np.zeros(ws, np.float32)
    w32[np.arange(ws[0]), np.arange(ws[0]) % 16] = 1.0
    y, _ = run(dev, "fp16", c, xb, to_dev(dev, half_of(w32, "fp16")[0], "fp16"), None, half_of(np.ones(ys), "fp16")[0], "raw")
    kept = HR.ROUND["fp16"](refs64(c, HR.UPCAST["fp16"](xb), w32, None, np.ones(ys))[0].astype(np.float32))
    flushed = np.zeros(ys, np.uint16)
    print(f"[gconv mfma half] fp16 subnormal inputs: kept {HR.same_bits(y, kept, 'fp16')}, flushed {HR.same_bits(y, flushed, 'fp16')}")
    assert (kept & 0x7FFF).min() > 0 and HR.same_bits(y, kept, "fp16")[0]


def _layer(cls, dev, seed, stochastic=False):
    layer = cls(128, 256, 3, stride=1, padding=1, groups=8, bias=True, deterministic=not stochastic).to(dev)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(G.weights(seed, tuple(layer.weight.shape))))
        layer.bias.copy_(torch.from_numpy(G.small_ints(seed + 1, (256,))))
    return layer


@pytest.mark.parametrize("cls", (BinConv2d, TerConv2d), ids=("bin", "ter"))
def test_layers_take_the_route_with_the_reference_bits(dev, monkeypatch, cls):
    """{.bfloat16(), .half(), fp32 under autocast} x {train deterministic, train stochastic, eval} x the switch on / off."""
    c = case_of((16, 32), (3, 1, 1), (5, 6), 8)
    for n, (fmt, autocast, mode, on) in enumerate(itertools.product(FMTS, (False, True), ("det", "stoch", "eval"), (True, False))):
        monkeypatch.setattr(_fused, "GROUPED_MFMA_HALF", on)
        tdt, wdt = FMTS[fmt], torch.float32 if autocast else FMTS[fmt]
        layer = _layer(cls, dev, 40 + n, stochastic=mode == "stoch")
        layer = (layer if autocast else layer.to(tdt)).train(mode != "eval")
        xb, x32 = half_of(G.pm1(900 + n, c.shapes[0]), fmt)
        xd = to_dev(dev, xb, fmt, LAYOUTS[n % 2]).requires_grad_(mode != "eval")
        lib, took, calls = sum(_fused.LIBRARY_PATHS.values()), _fused.STREAMING_HALF_STATS["grouped_mfma"], dict(_lib.call_counts)
        torch.manual_seed(77 + n)
        with torch.autocast("cuda", dtype=tdt, enabled=autocast), torch.set_grad_enabled(mode != "eval"):
            y = layer(xd)
        if mode != "eval":
            y.backward(torch.ones_like(y))
            assert xd.grad.dtype == tdt and layer.weight.grad.dtype == wdt and layer.bias.grad.dtype == wdt
        used = {k: _lib.call_counts[k] - calls.get(k, 0) for k in NEW}
        assert y.dtype == tdt
        if not on:                                                         # the switch off: the counted library expression
            assert sum(_fused.LIBRARY_PATHS.values()) > lib and not any(used.values())
            continue
        assert sum(_fused.LIBRARY_PATHS.values()) == lib and _fused.STREAMING_HALF_STATS["grouped_mfma"] == took + 1
        assert used == dict(zip(NEW, (1, 1, 1) if mode != "eval" else (1, 0, 0))), used
        wq = layer.weight.detach().float().cpu().numpy()
        if mode == "stoch":
            torch.manual_seed(77 + n)
            wq = layer._op.apply(layer.weight.detach()).float().cpu().numpy()
        elif mode == "det":
            wq = G.quantize(wq, cls.kind)
        assert set(np.unique(wq)) <= {-1.0, 0.0, 1.0}
        b32 = layer.bias.detach().to(tdt).float().cpu().numpy()
        check(bits_of(y), G.forward(x32, wq, b32, 8, *c.geom, dtype=np.float64), fmt, ("layer", fmt, autocast, mode))


@pytest.mark.parametrize("fmt", list(FMTS))
def test_forward_and_backward_replay_from_a_captured_graph(dev, monkeypatch, fmt):
    monkeypatch.setattr(_fused, "GROUPED_MFMA_HALF", True)
    layer = _layer(BinConv2d, dev, 60).to(FMTS[fmt])
    data = lambda seed, shape: to_dev(dev, half_of(G.gauss6(seed, shape) / 16, fmt)[0], fmt)          # noqa: E731
    xs, gs = data(61, (2, 128, 5, 6)).requires_grad_(True), data(62, (2, 256, 5, 6))

    def step(lay, x, g):
        lay.zero_grad(set_to_none=False)
        x.grad = None if x.grad is None else x.grad.zero_()
        y = lay(x)
        y.backward(g)
        return y.detach(), x.grad, lay.weight.grad, lay.bias.grad

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for _ in range(2):
            step(layer, xs, gs)
        torch.cuda.synchronize(dev)
        with _no_collection_inside(), torch.cuda.graph(graph, stream=stream):
            static = step(layer, xs, gs)
    torch.cuda.synchronize(dev)
    for rep in range(2):                                                  # replayed twice, on new data each time
        x2, g2 = data(63 + rep, xs.shape), data(65 + rep, gs.shape)
        with torch.no_grad():
            xs.copy_(x2)
            gs.copy_(g2)
        calls = _lib.call_counts["qt_gmconv2d_h"]
        graph.replay()
        torch.cuda.synchronize(dev)
        assert _lib.call_counts["qt_gmconv2d_h"] == calls                  # a replay, not a call
        got = [t.clone() for t in static]
        eager = step(copy.deepcopy(layer), x2.clone().requires_grad_(True), g2)
        for a, b in zip(got, eager):
            assert a.dtype == FMTS[fmt] and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_module_totals(dev):
    """Runs last in the file: zero differing bit patterns over every designed comparison above (each also asserted on its own)."""
    assert STATS["compared"] > 0 and STATS["differing"] == 0
