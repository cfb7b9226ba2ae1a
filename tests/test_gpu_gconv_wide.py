"""Grouped convs with 16 ... 64 channels per group (csrc/gconv_wide_mfma.hip) against the float64 reference of tests/_gconv_exact.py:
exact on integers, inside the header's bound on Gaussian data, through the layers, replayed from a captured graph."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _gconv_exact as R
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d
from pytorch_quantize_impls_amd.utils.graphs import _no_collection_inside
from test_gpu_gconv_mfma import SENTINEL, PAD, dev, _guarded, _spiked          # noqa: F401 (dev: the fixture)

pytestmark = pytest.mark.gpu

G, CG, GEOM = 8, 64, (3, 1, 1, 1)                      # CG, GEOM: the layer tests' channels per group and conv arguments
FWD, GIN = "qt_gwconv2d_f32", "qt_gwconv2d_grad_input_f32"
CHANS = ((64, 64), (24, 24), (40, 24), (48, 64), (64, 40), (16, 64))    # (cin_g, cout_g)
GEOMS = ((3, 1, (1, 1)), (3, 2, (1, 0)), (1, 1, (0, 0)), (1, 2, (0, 0)))   # (kernel, stride, padding)
MAPS = ((5, 5), (13, 11), (17, 17))   # one ragged tile; two tiles, ragged last, both halo sides; 3 x 3 stride 2 at 64: the budget shrinks the tile
LAYOUTS = (("nchw", "nchw"), ("nchw", "channels_last"), ("channels_last", "nchw"), ("channels_last", "channels_last"))   # (x, y)
# i % 4 is the geometry; layouts and data (+-1, |v| <= 3, the sibling's 20-bit spiked integers: all three terms) rotate with i + i // 4
CASES = [dict(ch=ch, hw=hw, geom=gm, lay=LAYOUTS[(i + i // 4) % 4], kind=("binary", "ternary")[i // 4 % 2], bias=i % 3 != 1,
              data=(R.pm1, R.small_ints, _spiked)[(i + i // 4) % 3], odd=i % 5 == 0)
         for i, (ch, hw, gm) in enumerate(itertools.product(CHANS, MAPS, GEOMS))]
IDS = ["i{ch[0]}o{ch[1]}-{hw[0]}x{hw[1]}-k{geom[0]}s{geom[1]}p{geom[2][0]}{geom[2][1]}-{lay[0]}-{lay[1]}-{kind}".format(**c) for c in CASES]


def _to(dev, a, layout="nchw", odd=False):
    """``odd``: the same values as a view one element into a buffer — 4-byte aligned only, so no 16-byte loads."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if t.dim() != 4:
        return t
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)[int(odd):]
    v = buf[:t.numel()].view(N, H, W, C).permute(0, 3, 1, 2) if layout == "channels_last" else buf[:t.numel()].view(N, C, H, W)
    return v.copy_(t)


def _shapes(c):
    (ci, co), (H, W), (k, s, p) = c["ch"], c["hw"], c["geom"]
    Ho, Wo = R.out_hw(H, W, k, s, p, 1)
    return (2, G * ci, H, W), (G * co, ci, k, k), (2, G * co, Ho, Wo)


def _run(dev, c, x, go, w, b):
    (k, s, p), lay = c["geom"], c["lay"]
    xs, _ws, ys = _shapes(c)
    by, oy = _guarded(dev, ys, lay[1])
    bx, ox = _guarded(dev, xs, lay[0])
    wd = _to(dev, w)
    y = ops.grouped_wide_conv2d(_to(dev, x, lay[0], c["odd"]), wd, None if b is None else _to(dev, b), s, p, 1, G, kind=c["kind"], out=oy)
    gx = ops.grouped_wide_conv2d_grad_input(xs, wd, _to(dev, go, lay[1], c["odd"]), s, p, 1, G, kind=c["kind"], out=ox)
    for buf in (by, bx):
        assert bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())
    return y, gx


@functools.lru_cache(maxsize=None)
def _reference(i, real):
    """Inputs of case i and the float64 results with their sums of magnitudes, made once: (x, go, w, b, y, |y|, gx, |gx|)."""
    c = CASES[i]
    xs, ws, ys = _shapes(c)
    gen = R.gauss6 if real else c["data"]
    x, go, w = gen(10 + i, xs), gen(20 + i, ys), R.weights(30 + i, ws)
    b = None if not c["bias"] else (R.gauss6 if real else R.small_ints)(40 + i, (ws[0],))
    wq, (k, s, p) = R.quantize(w, c["kind"]), c["geom"]
    ab = None if b is None else np.abs(b)
    fwd = lambda xx, ww, bb: R.forward(xx, ww, bb, G, k, s, p, 1, dtype=np.float64)             # noqa: E731
    gin = lambda gg, ww: R.grad_input(gg, ww, xs, G, k, s, p, 1, dtype=np.float64)              # noqa: E731
    return x, go, w, b, fwd(x, wq, b), fwd(np.abs(x), np.abs(wq), ab), gin(go, wq), gin(np.abs(go), np.abs(wq))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_integers_are_exact_forward_and_grad_input(dev, i):
    c = CASES[i]
    x, go, w, b, y64, ya, g64, ga = _reference(i, False)
    assert ya.max() < 2 ** 24 and ga.max() < 2 ** 24            # from the reference alone: every partial sum is an exact integer
    if c["ch"] == (64, 64) and c["hw"] == (17, 17) and c["geom"][:2] == (3, 2):    # the budget loop took rows off this tile
        xs, ws, _ys = _shapes(c)
        assert ops.grouped_wide_plan("forward", xs, ws, 2, c["geom"][2], 1, G)["tr_shrunk"] > 0
    y, gx = _run(dev, c, x, go, w, b)
    assert torch.equal(y.cpu(), torch.from_numpy(y64.astype(np.float32)))
    assert torch.equal(gx.cpu(), torch.from_numpy(g64.astype(np.float32)))
    y2, gx2 = _run(dev, c, x, go, w, b)                                             # two runs of one call: equal bits
    assert torch.equal(y, y2) and torch.equal(gx, gx2)


def _bound(c, abs_sum, backward):
    """The header's bound (3 Kp + 1) 2^-23 (sum |x q| + |bias|), Kp the reduction length rounded up to a multiple of 32."""
    K = c["ch"][1 if backward else 0] * c["geom"][0] ** 2
    return (3 * (-(-K // 32) * 32) + 1) * 2.0 ** -23 * abs_sum


REAL = [i for i, c in enumerate(CASES) if c["ch"] in ((64, 64), (40, 24)) and c["hw"] == (13, 11) and c["geom"][0] == 3]


@pytest.mark.parametrize("i", REAL, ids=[IDS[i] for i in REAL])
def test_gaussian_data_stays_inside_the_headers_bound(dev, i):
    x, go, w, b, y64, ya, g64, ga = _reference(i, True)
    y, gx = (t.cpu().numpy().astype(np.float64) for t in _run(dev, CASES[i], x, go, w, b))
    ry = float((np.abs(y - y64) / np.maximum(_bound(CASES[i], ya, False), 1e-300)).max())
    rg = float((np.abs(gx - g64) / np.maximum(_bound(CASES[i], ga, True), 1e-300)).max())
    print(IDS[i], "worst err / bound: forward", ry, "grad_input", rg)
    assert ry <= 1.0 and rg <= 1.0, (ry, rg)


def _layer(cls, dev):
    layer = cls(G * CG, G * CG, 3, padding=1, groups=G)
    layer.weight.data.copy_(torch.from_numpy(R.weights(50, tuple(layer.weight.shape))))
    layer.bias.data.copy_(torch.from_numpy(R.small_ints(51, (G * CG,))))
    return layer.to(dev)


def _node(y):          # the name of the conv's autograd node behind the layer's output (the layers return an alias of it)
    fn = y.grad_fn
    while fn is not None and "Conv2dFn" not in type(fn).__name__:
        fn = fn.next_functions[0][0] if fn.next_functions else None
    return type(fn).__name__


def _step(layer, x, go):
    layer.zero_grad(set_to_none=True)
    xd = x.clone().requires_grad_(True)
    y = layer(xd)
    y.backward(go)
    return y, xd.grad, layer.weight.grad, layer.bias.grad


@pytest.mark.parametrize("cls", (BinConv2d, TerConv2d))
def test_layers_reach_the_node_and_match_the_per_group_loop(dev, cls, monkeypatch):
    layer = _layer(cls, dev)
    x, go = R.pm1(52, (2, G * CG, 9, 7)), R.small_ints(53, (2, G * CG, 9, 7))
    xd, gd = _to(dev, x), _to(dev, go)
    monkeypatch.setattr(_fused, "GROUPED_WIDE", True)
    assert _fused.grouped_wide_route(layer, xd) and not _fused.grouped_mfma_route(layer, xd)
    calls = dict(_lib.call_counts)
    y, gx, gw, gb = _step(layer, xd, gd)
    assert _node(y) == "GroupedWideConv2dFnBackward"
    assert (_lib.call_counts[FWD] - calls.get(FWD, 0), _lib.call_counts[GIN] - calls.get(GIN, 0)) == (1, 1)
    layer.eval()                                                          # the stored image, the same launch, the same bits
    with torch.no_grad():
        assert torch.equal(layer(xd), y.detach())
    layer.train()
    monkeypatch.setattr(_fused, "GROUPED_WIDE", False)                    # the per-group loop: the same integers
    yl, gxl, _gwl, _gbl = _step(layer, xd, gd)
    assert _node(yl) != "GroupedWideConv2dFnBackward"
    assert torch.equal(y, yl) and torch.equal(gx, gxl)
    w = layer.weight.detach().cpu().numpy()
    gw64, _ab, gb64 = R.grad_weight(x, go, G, CG, *GEOM)
    gw64 = R.ste_mask(gw64, w)
    assert np.abs(gw.cpu().numpy() - gw64).max() <= 1e-5 * np.abs(gw64).max() and (gw.cpu().numpy()[np.abs(w) > R.STE] == 0).all()
    assert np.abs(gb.cpu().numpy() - gb64).max() <= 1e-5 * np.abs(gb64).max()


def test_forward_and_grad_input_replay_from_a_captured_graph(dev, monkeypatch):
    monkeypatch.setattr(_fused, "GROUPED_WIDE", True)
    layer = _layer(TerConv2d, dev).requires_grad_(False)
    shape = (2, G * CG, 9, 7)
    xs, gs = _to(dev, R.gauss6(60, shape)).requires_grad_(True), _to(dev, R.gauss6(61, shape))

    def step():
        y = layer(xs)
        return y.detach(), torch.autograd.grad(y, xs, gs)[0]

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        torch.cuda.synchronize(dev)
        with _no_collection_inside(), torch.cuda.graph(graph, stream=stream):
            y_static, gx_static = step()
    torch.cuda.synchronize(dev)
    x2, g2 = _to(dev, R.gauss6(62, shape)), _to(dev, R.gauss6(63, shape))
    with torch.no_grad():
        xs.copy_(x2)
        gs.copy_(g2)
    calls = dict(_lib.call_counts)
    for _ in range(3):                                                    # several replays against the one eager step
        graph.replay()
    torch.cuda.synchronize(dev)
    assert _lib.call_counts[FWD] == calls[FWD]                            # replays, not calls
    xe = x2.clone().requires_grad_(True)
    ye = layer(xe)
    assert torch.equal(y_static, ye.detach()) and torch.equal(gx_static, torch.autograd.grad(ye, xe, g2)[0])
