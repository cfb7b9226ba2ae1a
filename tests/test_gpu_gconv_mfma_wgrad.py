"""The weight gradient of the grouped convs with 16, 24 or 32 channels per group on the matrix cores (qt_gmconv2d_grad_weight_f32,
csrc/gconv_mfma.hip) against the float64 reference of tests/_gconv_exact.py, on the case grid of tests/test_gpu_gconv_mfma.py:
exact on designed integers, inside the accumulation bound on Gaussian data, the same bits twice, through the layers and replayed
from a captured graph.  The host side: tests/test_gconv_mfma_wgrad_cpu.py."""
import copy
import functools

import numpy as np
import pytest
import torch

import _gconv_exact as R
import test_gpu_gconv_mfma as F
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d
from pytorch_quantize_impls_amd.utils.graphs import _no_collection_inside

pytestmark = pytest.mark.gpu

GWT, STREAM = "qt_gmconv2d_grad_weight_f32", "qt_gconv2d_grad_weight_f32"
# (channels, groups, geometry, map, layouts, batch): the forward module's grid at batch 2, and 33 images of one tile each over the
# 32 splits that 32 groups get: workgroup 0 of every group accumulates two tiles, the others one
CASES = [c[:5] + (2,) for c in F.CASES if c[5] == "binary"] + [((16, 16), 32, (3, 1, 1), (9, 7), F.LAYOUTS[1], 33)]
IDS = [i for i, c in zip(F.IDS, F.CASES) if c[5] == "binary"] + ["i16o16g32-k3s1p1-9x7-N33"]
DESIGNS = {"x_wide": (17, 0), "go_wide": (0, 17), "both_medium": (10, 10)}       # spike bits of (x, go); 0: small integers only
S_MAX = ops.GM_WGRAD_MAX_SPLITS


dev = F.dev                                                              # the forward module's device fixture


def _shapes(c):
    (ci, co), G, (k, s, p), (H, W), _lay, N = c
    Ho, Wo = R.out_hw(H, W, k, s, p, 1)
    return (N, G * ci, H, W), (G * co, ci, k, k), (N, G * co, Ho, Wo)


def _spiked(seed, shape, bits, L):
    """Integers in [-3, 3]; a share min(1/4, 2 / L) of the positions (about two per channel, so that sum |go x| stays far below
    2^24) holds +-(2^(bits - 1) + odd r): three non-zero bf16 terms at 17 bits, two at 10."""
    g = R._rng(seed)
    small = g.randint(-3, 4, size=shape)
    if not bits:
        return small.astype(np.float32)
    big = (2 ** (bits - 1) + 2 * g.randint(0, 2 ** (bits - 2), size=shape) + 1) * np.where(g.rand(*shape) < 0.5, -1, 1)
    return np.where(g.rand(*shape) < min(0.25, 2.0 / L), big, small).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(i, design):
    """Inputs of case i and the float64 results, made once: (x, go, w, gw, sum |go x|, gbias).  design None: Gaussian data."""
    c = CASES[i]
    xs, ws, ys = _shapes(c)
    L = ys[0] * ys[2] * ys[3]
    if design is None:
        x, go = R.gauss6(10 + i, xs), R.gauss6(20 + i, ys)
    else:
        x, go = _spiked(10 + i, xs, DESIGNS[design][0], L), _spiked(20 + i, ys, DESIGNS[design][1], L)
    (k, s, p), G = c[2], c[1]
    return (x, go, R.weights(30 + i, ws)) + R.grad_weight(x, go, G, c[0][0], k, s, p, 1)


def _run(dev, c, x, go, w, ste, workspace=None):
    """(gw, gbias) through ``ops`` into sentinel-guarded buffers, in the case's layouts."""
    (k, s, p), lay = c[2], c[4]
    bw, ow = F._guarded(dev, w.shape, "nchw")
    bb = torch.full((w.shape[0] + 2 * F.PAD,), F.SENTINEL, dtype=torch.float32, device=dev)
    gw, gb = ops.grouped_mfma_conv2d_grad_weight(F._to(dev, x, lay[0]), F._to(dev, go, lay[1]), F._to(dev, w), s, p, 1, c[1], ste,
                                                 out=ow, out_bias=bb[F.PAD:-F.PAD], workspace=workspace)
    for buf in (bw, bb):
        assert bool((buf[:F.PAD] == F.SENTINEL).all() and (buf[-F.PAD:] == F.SENTINEL).all())
    return gw, gb


@pytest.mark.parametrize("design", DESIGNS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_designed_integers_are_exact(dev, i, design):
    x, go, w, gw64, ab, gb64 = _reference(i, design)
    assert ab.max() < 2 ** 24 and np.abs(go).sum((0, 2, 3)).max() < 2 ** 24      # from the reference alone: every sum is an exact integer
    for ste, want in ((R.STE, R.ste_mask(gw64, w)), (0.0, gw64)):
        gw, gb = _run(dev, CASES[i], x, go, w, ste)
        bad = int((gw.cpu().numpy() != want).sum()), int((gb.cpu().numpy() != gb64).sum())
        assert bad == (0, 0), (ste, bad)


def _bounds(L, ab, gabs):
    """The bounds of include/qt_hip.h: exact splits and products, the dropped products below 2^-23 |go x|, then at most 6 L + S_max
    (bias: 3 L + S_max) fp32 additions of relative error below 2^-23 each, whatever the hardware's internal order."""
    return 1.02 * (6 * L + S_MAX + 2) * 2.0 ** -23 * ab, 1.02 * (3 * L + S_MAX + 1) * 2.0 ** -23 * gabs


@pytest.mark.parametrize("i", F.REAL, ids=[IDS[i] for i in F.REAL])
def test_gaussian_data_stays_inside_the_accumulation_bound(dev, i):
    x, go, w, gw64, ab, gb64 = _reference(i, None)
    gw, gb = _run(dev, CASES[i], x, go, w, 0.0)
    bw, bb = _bounds(go.shape[0] * go.shape[2] * go.shape[3], ab, np.abs(go).astype(np.float64).sum((0, 2, 3)))
    rw = float((np.abs(gw.cpu().numpy() - gw64) / np.maximum(bw, 1e-300)).max())
    rb = float((np.abs(gb.cpu().numpy() - gb64) / np.maximum(bb, 1e-300)).max())
    print(IDS[i], "worst err / bound: grad_weight", rw, "grad_bias", rb)
    assert rw <= 1.0 and rb <= 1.0, (rw, rb)


def test_equal_inputs_give_equal_bits_whatever_the_workspace_holds(dev):
    i = F.REAL[1]
    x, go, w = _reference(i, None)[:3]
    (_k, s, p), G = CASES[i][2], CASES[i][1]
    need = ops.grouped_mfma_grad_weight_work_floats(x.shape, w.shape, s, p, 1, G)
    runs = [_run(dev, CASES[i], x, go, w, R.STE, torch.full((need,), float("nan"), device=dev)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and bool(torch.isfinite(runs[0][0]).all())


def _step(dev, layer, hw, seed):
    x, go = R.gauss6(seed, (2, F.G * F.CG) + hw), R.gauss6(seed + 1, (2, F.G * F.CG) + hw)
    layer.zero_grad(set_to_none=True)
    calls = dict(_lib.call_counts)
    layer(F._to(dev, x).requires_grad_(True)).backward(F._to(dev, go))
    return x, go, F._used(calls), layer.weight.grad.cpu().numpy(), layer.bias.grad.cpu().numpy()


@pytest.mark.parametrize("cls", (BinConv2d, TerConv2d))
def test_layers_take_the_route_from_the_floor_up_and_under_the_switch(dev, cls, monkeypatch):
    monkeypatch.setattr(_fused, "GROUPED_MFMA", True)
    monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD", True)
    layer = F._layer(cls, dev)
    w = layer.weight.detach().cpu().numpy()
    assert _fused.GROUPED_MFMA_WGRAD_MIN_L == 1024
    x, go, used, gw, gb = _step(dev, layer, (23, 23), 70)                       # L = 1058
    assert (used.get(F.FWD), used.get(F.GIN), used.get(GWT), used.get(STREAM)) == (1, 1, 1, None), used
    gw64, ab, gb64 = R.grad_weight(x, go, F.G, F.CG, *F.GEOM)
    bw, bb = _bounds(2 * 23 * 23, ab, np.abs(go).astype(np.float64).sum((0, 2, 3)))
    assert (np.abs(gw - R.ste_mask(gw64, w)) <= bw).all() and (gw[np.abs(w) > R.STE] == 0).all() and (np.abs(gb - gb64) <= bb).all()
    for hw, switch in (((22, 23), True), ((23, 23), False)):                    # below the floor (L = 1012); the switch off
        monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD", switch)
        x, go, used, gw, gb = _step(dev, layer, hw, 72)
        assert (used.get(F.FWD), used.get(F.GIN), used.get(GWT), used.get(STREAM)) == (1, 1, None, 1), used
        gw64, ab, gb64 = R.grad_weight(x, go, F.G, F.CG, *F.GEOM)
        L = 2 * hw[0] * hw[1]
        assert (np.abs(gw - R.ste_mask(gw64, w)) <= R.grad_weight_bound(ab, L)).all()
        assert (np.abs(gb - gb64) <= R.grad_weight_bound(np.abs(go).sum((0, 2, 3)), L)).all()


def test_backward_replays_from_a_captured_graph(dev, monkeypatch):
    monkeypatch.setattr(_fused, "GROUPED_MFMA", True)
    monkeypatch.setattr(_fused, "GROUPED_MFMA_WGRAD", True)
    layer = F._layer(TerConv2d, dev)
    shape = (2, F.G * F.CG, 23, 23)
    xs, gs = F._to(dev, R.gauss6(80, shape)).requires_grad_(True), F._to(dev, R.gauss6(81, shape))

    def step():
        layer.zero_grad(set_to_none=False)
        layer(xs).backward(gs)

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        torch.cuda.synchronize(dev)
        with _no_collection_inside(), torch.cuda.graph(graph, stream=stream):
            step()
    torch.cuda.synchronize(dev)
    x2, g2 = F._to(dev, R.gauss6(82, shape)), F._to(dev, R.gauss6(83, shape))
    with torch.no_grad():
        xs.copy_(x2)
        gs.copy_(g2)
    for _ in range(3):                                                    # several replays against the one eager step
        graph.replay()
    torch.cuda.synchronize(dev)
    twin = copy.deepcopy(layer)
    twin.zero_grad(set_to_none=True)
    calls = dict(_lib.call_counts)
    twin(x2.clone().requires_grad_(True)).backward(g2)
    assert F._used(calls).get(GWT) == 1
    assert torch.equal(layer.weight.grad, twin.weight.grad) and torch.equal(layer.bias.grad, twin.bias.grad)
