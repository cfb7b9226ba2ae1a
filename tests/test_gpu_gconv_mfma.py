"""Grouped convs with 16, 24 or 32 channels per group on the matrix cores (csrc/gconv_mfma.hip) against the float64 reference of
tests/_gconv_exact.py: exact on designed integers, inside the fp32 accumulation bound on Gaussian data, through the layers, and
replayed from a captured graph.  The host side: tests/test_gconv_mfma_cpu.py."""
import copy
import functools

import numpy as np
import pytest
import torch

import _gconv_exact as R
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, DorefaConv2d
from pytorch_quantize_impls_amd.utils.graphs import _no_collection_inside

pytestmark = pytest.mark.gpu

SENTINEL, PAD = 12345.0, 67
FWD, GIN, GWT = "qt_gmconv2d_f32", "qt_gmconv2d_grad_input_f32", "qt_gconv2d_grad_weight_f32"
CHANS = ((16, 16), (24, 48), (32, 32))                                   # (cin_g, cout_g)
GEOMS = ((1, 1, 0), (3, 1, 1), (3, 2, 1), (3, 1, 0))                     # (kernel, stride, padding)
MAPS = ((1, 1), (9, 7), (5, 37))      # smaller than any tile; no multiple of a tile, odd under stride 2; wider than a tile row
LAYOUTS = (("nchw", "nchw"), ("nchw", "channels_last"), ("channels_last", "nchw"), ("channels_last", "channels_last"))   # (x, y)


def _cases():
    """Every geometry on every map it fits, each with all three channel pairs; groups and layouts rotate.  The kind varies on one."""
    out = []
    for k, s, p in GEOMS:
        for hw in MAPS:
            if min(hw) + 2 * p < k:
                continue
            for ch in CHANS:
                out.append((ch, 8 + len(out) % 2, (k, s, p), hw, LAYOUTS[len(out) % 4], "binary"))
    return out + [((16, 16), 8, (3, 1, 1), (9, 7), LAYOUTS[1], kind) for kind in ("ternary", "raw")]


CASES = _cases()
IDS = ["i{0[0]}o{0[1]}g{1}-k{2[0]}s{2[1]}p{2[2]}-{3[0]}x{3[1]}-{4[0]}-{4[1]}-{5}".format(*c) for c in CASES]
REAL = [i for i, c in enumerate(CASES) if c[3] == (9, 7) and c[2] != (3, 1, 0)][::4][:3]        # three geometries, Gaussian data


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _to(dev, a, layout="nchw"):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" and t.dim() == 4 else t


def _guarded(dev, shape, layout):
    """(buffer, view): ``view`` is a dense tensor of ``shape`` in ``layout`` with PAD sentinel elements on either side."""
    N, C, H, W = shape
    buf = torch.full((N * C * H * W + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    mid = buf[PAD:-PAD]
    return buf, (mid.view(N, H, W, C).permute(0, 3, 1, 2) if layout == "channels_last" else mid.view(*shape))


def _spiked(seed, shape):
    """Integers in [-3, 3]; 1/128 of the positions hold +-(2^19 + odd r), r < 2^19: 20 significant bits, three non-zero bf16 terms."""
    g = R._rng(seed)
    big = (2 ** 19 + 2 * g.randint(0, 2 ** 18, size=shape) + 1) * np.where(g.rand(*shape) < 0.5, -1, 1)
    return np.where(g.rand(*shape) < 1 / 128, big, g.randint(-3, 4, size=shape)).astype(np.float32)


def _shapes(c):
    (ci, co), G, (k, s, p), (H, W) = c[:4]
    Ho, Wo = R.out_hw(H, W, k, s, p, 1)
    return (2, G * ci, H, W), (G * co, ci, k, k), (2, G * co, Ho, Wo)


def _run(dev, c, x, go, w, b):
    """(y, gx) through ``ops`` into sentinel-guarded buffers of the case's layouts."""
    (k, s, p), lay, kind = c[2], c[4], c[5]
    xs, _ws, ys = _shapes(c)
    by, oy = _guarded(dev, ys, lay[1])
    bx, ox = _guarded(dev, xs, lay[0])
    wd = _to(dev, w)
    y = ops.grouped_mfma_conv2d(_to(dev, x, lay[0]), wd, _to(dev, b), s, p, 1, c[1], kind=kind, out=oy)
    gx = ops.grouped_mfma_conv2d_grad_input(xs, wd, _to(dev, go, lay[1]), s, p, 1, c[1], kind=kind, out=ox)
    for buf in (by, bx):
        assert bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())
    return y.cpu().numpy().astype(np.float64), gx.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _reference(i, real):
    """Inputs of case i and the float64 results with their sums of magnitudes, made once: (x, go, w, b, y, |y|, gx, |gx|)."""
    c = CASES[i]
    xs, ws, ys = _shapes(c)
    gen = R.gauss6 if real else _spiked
    x, go = gen(10 + i, xs), gen(20 + i, ys)
    w = R.grid_weights(30 + i, ws) if c[5] == "raw" else R.weights(30 + i, ws)
    b = R.gauss6(40 + i, (ws[0],)) if real else R.small_ints(40 + i, (ws[0],))
    wq = R.quantize(w, c[5])
    (k, s, p), G = c[2], c[1]
    fwd = lambda xx, ww, bb: R.forward(xx, ww, bb, G, k, s, p, 1, dtype=np.float64)             # noqa: E731
    gin = lambda gg, ww: R.grad_input(gg, ww, xs, G, k, s, p, 1, dtype=np.float64)              # noqa: E731
    return x, go, w, b, fwd(x, wq, b), fwd(np.abs(x), np.abs(wq), np.abs(b)), gin(go, wq), gin(np.abs(go), np.abs(wq))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_designed_integers_are_exact_forward_and_grad_input(dev, i):
    x, go, w, b, y64, ya, g64, ga = _reference(i, False)
    assert ya.max() < 2 ** 24 and ga.max() < 2 ** 24            # from the reference alone: every partial sum is an exact integer
    y, gx = _run(dev, CASES[i], x, go, w, b)
    assert int((y != y64).sum()) == 0 and int((gx != g64).sum()) == 0, (int((y != y64).sum()), int((gx != g64).sum()))


def _bound(c, abs_sum, backward):
    """1.01 (3 Kp + 1) 2^-23 sum |terms|: the split and the products are exact; at most 3 Kp + 1 fp32 additions remain (Kp: K
    padded to the MFMA chunk of 32), each with relative error below 2^-23 whatever the hardware's rounding of its accumulations."""
    K = (c[0][1] if backward else c[0][0]) * c[2][0] ** 2
    return 1.01 * (3 * (-(-K // 32) * 32) + 1) * 2.0 ** -23 * abs_sum


@pytest.mark.parametrize("i", REAL, ids=[IDS[i] for i in REAL])
def test_gaussian_data_stays_inside_the_accumulation_bound(dev, i):
    x, go, w, b, y64, ya, g64, ga = _reference(i, True)
    y, gx = _run(dev, CASES[i], x, go, w, b)
    ry = float((np.abs(y - y64) / np.maximum(_bound(CASES[i], ya, False), 1e-300)).max())
    rg = float((np.abs(gx - g64) / np.maximum(_bound(CASES[i], ga, True), 1e-300)).max())
    print(IDS[i], "worst err / bound: forward", ry, "grad_input", rg)
    assert ry <= 1.0 and rg <= 1.0, (ry, rg)


G, CG, GEOM = 8, 16, (3, 1, 1, 1)


def _layer(cls, dev):
    layer = cls(G * CG, G * CG, 3, padding=1, groups=G)
    layer.weight.data.copy_(torch.from_numpy(R.weights(50, tuple(layer.weight.shape))))
    layer.bias.data.copy_(torch.from_numpy(R.gauss6(51, (G * CG,))))
    return layer.to(dev)


def _used(calls):
    return {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}


@pytest.mark.parametrize("cls", (BinConv2d, TerConv2d))
def test_layers_train_step_eval_and_the_switch(dev, cls, monkeypatch):
    monkeypatch.setattr(_fused, "GROUPED_MFMA", True)
    layer = _layer(cls, dev)
    x, go = R.gauss6(52, (2, G * CG, 9, 7)), R.gauss6(53, (2, G * CG, 9, 7))
    w, b = layer.weight.detach().cpu().numpy(), layer.bias.detach().cpu().numpy()
    wq = R.quantize(w, layer.kind)
    xd = _to(dev, x).requires_grad_(True)
    assert _fused.grouped_mfma_route(layer, xd) and not _fused.grouped_route(layer, xd)
    calls = dict(_lib.call_counts)
    y = layer(xd)
    y.backward(_to(dev, go))
    used = _used(calls)
    assert (used.get(FWD), used.get(GIN), used.get(GWT)) == (1, 1, 1) and not [k for k in used if k.startswith("qt_conv2d_implicit")], used
    c = ((CG, CG), G, (3, 1, 1))
    y64, ya = (R.forward(a, q, bb, G, *GEOM, dtype=np.float64) for a, q, bb in ((x, wq, b), (np.abs(x), np.abs(wq), np.abs(b))))
    g64, ga = (R.grad_input(a, q, x.shape, G, *GEOM, dtype=np.float64) for a, q in ((go, wq), (np.abs(go), np.abs(wq))))
    assert (np.abs(y.detach().cpu().numpy() - y64) <= _bound(c, ya, False)).all()
    assert (np.abs(xd.grad.cpu().numpy() - g64) <= _bound(c, ga, True)).all()
    gw64, ab, gb64 = R.grad_weight(x, go, G, CG, *GEOM)
    L = 2 * 9 * 7
    gw = layer.weight.grad.cpu().numpy()
    assert (np.abs(gw - R.ste_mask(gw64, w)) <= R.grad_weight_bound(ab, L)).all() and (gw[np.abs(w) > R.STE] == 0).all()
    assert (np.abs(layer.bias.grad.cpu().numpy() - gb64) <= R.grad_weight_bound(np.abs(go).sum((0, 2, 3)), L)).all()
    # eval: the stored image, the same launch, the same bits — without autograd and with it
    layer.eval()
    with torch.no_grad():
        assert torch.equal(layer(_to(dev, x)), y.detach())
    assert torch.equal(layer(_to(dev, x).requires_grad_(True)).detach(), y.detach())
    # +-1 data: the per-group loop gives the same integers
    xp = _to(dev, R.pm1(54, x.shape))
    with torch.no_grad():
        calls = dict(_lib.call_counts)
        yp = layer(xp)
        assert _used(calls).get(FWD) == 1
        monkeypatch.setattr(_fused, "GROUPED_MFMA", False)
        calls = dict(_lib.call_counts)
        assert not _fused.grouped_mfma_route(layer, xp) and torch.equal(layer(xp), yp) and FWD not in _used(calls)
        # four groups of 16, and DorefaConv2d, stay off the route
        monkeypatch.setattr(_fused, "GROUPED_MFMA", True)
        calls = dict(_lib.call_counts)
        for other in (cls(64, 64, 3, padding=1, groups=4), DorefaConv2d(G * CG, G * CG, 3, padding=1, groups=G, bit_width=4)):
            other.to(dev)(_to(dev, R.pm1(55, (2, other.in_channels, 6, 6))))
        assert not [k for k in _used(calls) if k.startswith("qt_gmconv2d")]


def test_forward_and_backward_replay_from_a_captured_graph(dev, monkeypatch):
    monkeypatch.setattr(_fused, "GROUPED_MFMA", True)
    layer = _layer(TerConv2d, dev)
    shape = (2, G * CG, 9, 7)
    xs, gs = _to(dev, R.gauss6(60, shape)).requires_grad_(True), _to(dev, R.gauss6(61, shape))

    def step():
        layer.zero_grad(set_to_none=False)
        if xs.grad is not None:
            xs.grad.zero_()
        y = layer(xs)
        y.backward(gs)
        return y.detach()

    stream, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        torch.cuda.synchronize(dev)
        with _no_collection_inside(), torch.cuda.graph(graph, stream=stream):
            y_static = step()
    torch.cuda.synchronize(dev)
    x2, g2 = _to(dev, R.gauss6(62, shape)), _to(dev, R.gauss6(63, shape))
    with torch.no_grad():
        xs.copy_(x2)
        gs.copy_(g2)
    calls = dict(_lib.call_counts)
    for _ in range(3):                                                    # several replays against the one eager step
        graph.replay()
    torch.cuda.synchronize(dev)
    assert FWD not in _used(calls)                                        # replays, not calls
    got = (y_static.clone(), xs.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone())
    twin, xe = copy.deepcopy(layer), x2.clone().requires_grad_(True)
    twin.zero_grad(set_to_none=True)
    ye = twin(xe)
    ye.backward(g2)
    assert _used(calls).get(FWD) == 1
    for a, b in zip(got, (ye.detach(), xe.grad, twin.weight.grad, twin.bias.grad)):
        assert torch.equal(a, b)
