"""The weight gradient of the grouped convs with 16, 24 or 32 channels per group on one-term MFMAs (qt_gmconv2d_grad_weight_h,
csrc/gconv_mfma_h.hip) through ops.grouped_mfma_conv2d_grad_weight and the layers, against the float64 reference of
tests/_gconv_exact.py.  The contract (include/qt_hip.h): fp32 sums that are exact below 2^24 units, one rounding to nearest even
into the weight's dtype.  Results are written into sentinel-guarded views.  The host side: tests/test_gconv_mfma_wgrad_half_cpu.py."""
import numpy as np
import pytest
import torch

import _gconv_exact as G
import _half_round as HR
from test_gpu_gconv_mfma_half import FMTS, LAYOUTS, MAXINT, PAD, SENTINEL, bits_of, half_of, to_dev
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d

pytestmark = pytest.mark.gpu

GWH, STREAM = "qt_gmconv2d_grad_weight_h", "qt_gconv2d_grad_weight_h"
# (channels, groups, (k, s, p), map, batch): 1 x 1 maps (one live k position of 32), 9 x 7 (a partial chunk), 9 x 37 (several column
# tiles and tile tails); then 33 one-tile images over the 32 splits of 32 groups: workgroup 0 carries its accumulators over two units
CASES = [(ch, 8, ksp, m, 2) for ch in ((16, 16), (16, 32), (24, 48), (32, 32)) for ksp in ((1, 1, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0))
         for m in ((1, 1), (9, 7), (9, 37)) if m[0] + 2 * ksp[2] >= ksp[0]] + [((16, 16), 32, (3, 1, 1), (9, 7), 33)]
IDS = ["i{0[0]}o{0[1]}g{1}-k{2[0]}s{2[1]}p{2[2]}-{3[0]}x{3[1]}-N{4}".format(*c) for c in CASES]
REAL = [IDS.index(n) for n in ("i16o16g8-k3s1p1-9x7-N2", "i24o48g8-k3s1p1-9x7-N2", "i32o32g8-k3s2p1-9x37-N2")]
S_MAX = ops.GM_WGRAD_MAX_SPLITS
STATS = dict(compared=0, differing=0, worst=0.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    yield torch.device("cuda:0")
    print(f"\n[gconv mfma wgrad half] designed elements compared {STATS['compared']}, differing bit patterns {STATS['differing']}, "
          f"worst err / bound on real-valued data {STATS['worst']:.3f}")


def _shapes(c):
    (ci, co), Gn, (k, s, p), (H, W), N = c
    Ho, Wo = G.out_hw(H, W, k, s, p, 1)
    return (N, Gn * ci, H, W), (Gn * co, ci, k, k), (N, Gn * co, Ho, Wo)


def _ints(seed, shape, spike, L):
    """Integers in [-3, 3]; with ``spike`` a share min(1/4, 2 / L) of the positions holds +-(an odd integer up to ``spike``)."""
    g = G._rng(seed)
    small = g.randint(-3, 4, size=shape)
    big = (2 * g.randint(spike // 4, (spike + 1) // 2 + 1, size=shape) - 1) * np.where(g.rand(*shape) < 0.5, -1, 1)
    return np.where((g.rand(*shape) < min(0.25, 2.0 / L)) & (spike > 0), big, small)


def _run(dev, fmt, c, xb, gob, w, ste, i=0, workspace=None):
    """(gw, gbias) of ``ops`` for the patterns xb / gob and the device weight ``w``, each in a sentinel-guarded buffer."""
    _k, s, p = c[2]
    bufs = [torch.full((m + 2 * PAD,), SENTINEL, dtype=torch.float32 if w.dtype == torch.float32 else torch.int16, device=dev)
            for m in (w.numel(), w.shape[0])]
    outs = [b.view(w.dtype)[PAD:-PAD] for b in bufs]
    gw, gb = ops.grouped_mfma_conv2d_grad_weight(to_dev(dev, xb, fmt, LAYOUTS[i % 2], odd=i % 4 == 3),
                                                 to_dev(dev, gob, fmt, LAYOUTS[i // 2 % 2], odd=i % 4 == 3), w, s, p, 1, c[1], ste,
                                                 out=outs[0].view(w.shape), out_bias=outs[1], workspace=workspace)
    for b in bufs:
        assert bool((b[:PAD] == SENTINEL).all() and (b[-PAD:] == SENTINEL).all())
    return gw, gb


def _same(got, want64, fmt, wide):
    """fp32 results equal the float64 values; half results are RNE(exact) bit for bit."""
    n = (int((got.cpu().numpy().astype(np.float64) != want64).sum()) if wide
         else HR.same_bits(bits_of(got), HR.ROUND[fmt](want64.astype(np.float32)), fmt)[1])
    STATS["compared"] += want64.size
    STATS["differing"] += n
    return n == 0


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_designed_integers_are_rne_of_the_exact_sum(dev, fmt, i):
    """The spikes sit in x on even cases and in go on odd ones; layouts, odd-offset views and the mask rotate with the case."""
    c = CASES[i]
    xs, ws, ys = _shapes(c)
    L = ys[0] * ys[2] * ys[3]
    (xb, x32), (gob, go32) = (half_of(_ints(7 * i + j, sh, MAXINT[fmt] * (i % 2 == j), L), fmt) for j, sh in enumerate((xs, ys)))
    gw64, ab, gb64 = G.grad_weight(x32, go32, c[1], c[0][0], *c[2], 1)
    assert ab.max() < 2 ** 24 and np.abs(go32).sum((0, 2, 3)).max() < 2 ** 24         # from the reference alone: every fp32 sum is exact
    wb, w16 = half_of(G.weights(7 * i + 2, ws), fmt)
    for wide in (False, True):
        w32 = G.weights(7 * i + 3, ws) if wide else w16
        w = torch.from_numpy(w32).to(dev) if wide else to_dev(dev, wb, fmt)
        ste = G.STE if (i + wide) % 2 else 0.0
        gw, gb = _run(dev, fmt, c, xb, gob, w, ste, i)
        assert gw.dtype == gb.dtype == w.dtype
        assert _same(gw, G.ste_mask(gw64, w32) if ste else gw64, fmt, wide) and _same(gb, gb64, fmt, wide), (wide, ste)


def test_fp16_subnormal_gradients_are_kept(dev):
    """go holds fp16 subnormals, x small integers: every sum is an integer below 2^24 in units of 2^-24, read back through fp32."""
    c = CASES[REAL[0]]
    xs, ws, ys = _shapes(c)
    gob = G._rng(1).randint(1, 1024, size=ys).astype(np.uint16) | (G._rng(2).randint(0, 2, size=ys) << 15).astype(np.uint16)
    xb, x32 = half_of(_ints(3, xs, 0, 1), "fp16")
    gw64, ab, gb64 = G.grad_weight(x32, HR.UPCAST["fp16"](gob), c[1], c[0][0], *c[2], 1)
    assert ab.max() < 1.0 and np.abs(gw64).max() > 0                                  # 2^24 units of 2^-24
    gw, gb = _run(dev, "fp16", c, xb, gob, torch.zeros(ws, device=dev), 0.0)
    assert _same(gw, gw64, "fp16", True) and _same(gb, gb64, "fp16", True)


@pytest.mark.parametrize("i", REAL, ids=[IDS[i] for i in REAL])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_real_valued_data_within_the_accumulation_bound(dev, fmt, i):
    """The header's bound (L + S_max + 2 fp32 roundings of relative error 2^-23; bias: + 1), times 1.02 for the reference's own
    float64 sums, plus half an ulp of the output type where the result is rounded into a half weight dtype."""
    c = CASES[i]
    xs, ws, ys = _shapes(c)
    L = ys[0] * ys[2] * ys[3]
    (xb, x32), (gob, go32) = half_of(G.gauss6(i, xs) / 16, fmt), half_of(G.gauss6(i + 1, ys) / 16, fmt)
    gw64, ab, gb64 = G.grad_weight(x32, go32, c[1], c[0][0], *c[2], 1)
    gabs = np.abs(go32).astype(np.float64).sum((0, 2, 3))
    for wide, wdt in ((True, torch.float32), (False, FMTS[fmt])):
        gw, gb = _run(dev, fmt, c, xb, gob, torch.zeros(ws, dtype=wdt, device=dev), 0.0, i)
        for got, want, mag, extra in ((gw, gw64, ab, 2), (gb, gb64, gabs, 1)):
            got = got.cpu().numpy().astype(np.float64) if wide else HR.UPCAST[fmt](bits_of(got)).astype(np.float64)
            bound = 1.02 * (L + S_MAX + extra) * 2.0 ** -23 * mag + (0 if wide else HR.half_ulp(want, fmt))
            ratio = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
            STATS["worst"] = max(STATS["worst"], ratio)
            print(f"[gconv mfma wgrad half] {fmt} {IDS[i]} w fp32 {wide}: worst err / bound {ratio:.3f}")
            assert ratio <= 1.0


@pytest.mark.parametrize("fmt", list(FMTS))
def test_equal_inputs_give_equal_bits_whatever_the_workspace_holds(dev, fmt):
    c = CASES[REAL[2]]
    xs, ws, ys = _shapes(c)
    xb, gob, (wb, _) = half_of(G.gauss6(5, xs) / 16, fmt)[0], half_of(G.gauss6(6, ys) / 16, fmt)[0], half_of(G.weights(7, ws), fmt)
    need = ops.grouped_mfma_grad_weight_work_floats(xs, ws, c[2][1], c[2][2], 1, c[1])
    runs = [_run(dev, fmt, c, xb, gob, to_dev(dev, wb, fmt), G.STE, 1, torch.full((need,), float("nan"), device=dev)) for _ in range(2)]
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16)) and bool(torch.isfinite(runs[0][0].float()).all())
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16)) and bool(torch.isfinite(runs[0][1].float()).all())


@pytest.mark.parametrize("mode", ("bf16", "fp16", "autocast"))
@pytest.mark.parametrize("cls", (BinConv2d, TerConv2d), ids=("bin", "ter"))
def test_layers_take_the_route_from_the_floor_up_and_under_the_switch(dev, monkeypatch, cls, mode):
    """8 groups of 16 -> 16 on +-1 activations and integer gradients: (23 x 23, on) takes the new entry once, (22 x 23, on) and
    (23 x 23, off) the streaming one once; gradients in the weight's dtype with the reference's bits."""
    fmt, wide = ("bf16" if mode == "autocast" else mode), mode == "autocast"
    monkeypatch.setattr(_fused, "GROUPED_MFMA_HALF", True)
    layer = cls(128, 128, 3, stride=1, padding=1, groups=8, bias=True, deterministic=True).to(dev)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(G.weights(40, tuple(layer.weight.shape))))
    layer = layer if wide else layer.to(FMTS[fmt])
    w32 = layer.weight.detach().float().cpu().numpy()
    for n, (hw, switch) in enumerate((((23, 23), True), ((22, 23), True), ((23, 23), False))):
        monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD_HALF", switch)
        (xb, x32), (gob, go32) = half_of(G.pm1(50 + n, (2, 128) + hw), fmt), half_of(_ints(60 + n, (2, 128) + hw, 0, 1), fmt)
        layer.zero_grad(set_to_none=True)
        calls = dict(_lib.call_counts)
        with torch.autocast("cuda", dtype=FMTS[fmt], enabled=wide):
            y = layer(to_dev(dev, xb, fmt, LAYOUTS[n % 2]).requires_grad_(True))
        y.backward(to_dev(dev, gob, fmt))
        used = tuple(_lib.call_counts[k] - calls.get(k, 0) for k in (GWH, STREAM))
        assert used == ((1, 0) if n == 0 else (0, 1)), (hw, switch, used)
        gw64, ab, gb64 = G.grad_weight(x32, go32, 8, 16, 3, 1, 1, 1)
        assert ab.max() < 2 ** 24 and layer.weight.grad.dtype == layer.bias.grad.dtype == layer.weight.dtype
        assert _same(layer.weight.grad, G.ste_mask(gw64, w32), fmt, wide) and _same(layer.bias.grad, gb64, fmt, wide)
