"""Grouped sign convs with 16 or 32 channels per group inside the fused inference chain, on the GPU (csrc/gconv_planes_mfma.hip,
its ops, layers.FusedGroupedMfmaBnSign, ``lazy.grouped_mfma_deferred()``), bit for bit against tests/_gconv_exact.py's float32 forward
on the decoded image (integer sums: exact) and tests/_dw_planes.py's threshold bit and packers; every output lies between sentinels."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _dw_planes as P
import _gconv_exact as X
from test_gpu_gconv_chain import (dev, _to, _guarded_words, _guarded_f32, _intact, _planes_of, _pm1, _run, _ready, _triple, _value,  # noqa: F401
                                  _delta, HALOS, KINDS)
from pytorch_quantize_impls_amd import _lib, lazy, ops, utils
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, FusedConvPoolBnSign, FusedGroupedMfmaBnSign, fuse_sequential

pytestmark = pytest.mark.gpu

SIGN, F32, EAGER = "qt_gmconv2d_sign", "qt_gmconv2d_bits_f32", "qt_gmconv2d_f32"
# (G, cin_g, cout_g, N, H, W, k, stride, padding): odd groups in the upper half-word, output groups that straddle words, a partial
# last plane word, ld padding, G % 4 != 0; a partial last 16-pixel tile, tiles across rows and images; every kernel, stride, padding
CASES = ((8, 16, 16, 1, 7, 7, 3, 1, (1, 1)), (9, 16, 48, 3, 5, 17, 3, 2, (1, 0)), (8, 32, 32, 3, 14, 14, 3, 1, (1, 1)),
         (3, 32, 48, 1, 7, 7, 1, 1, (0, 0)), (10, 16, 32, 3, 5, 17, 1, 2, (0, 0)), (3, 32, 48, 3, 14, 14, 3, 2, (0, 0)),
         (10, 16, 32, 1, 14, 14, 3, 1, (1, 0)), (9, 16, 48, 1, 7, 7, 3, 1, (0, 0)))


def _counted(fn):
    before = dict(_lib.call_counts)
    out = fn()
    return out, _delta(dict(_lib.call_counts), before)


def _shapes(c):
    G, ci, co, N, H, W, k, s, p = c
    Ho, Wo = X.out_hw(H, W, (k, k), (s, s), p, (1, 1))
    return (N, G * ci, H, W), (G * co, ci, k, k), (N, G * co, Ho, Wo)


_ref = lambda c, x, wq, b: X.forward(x, wq, b, c[0], (c[6],) * 2, (c[7],) * 2, c[8], (1, 1))  # noqa: E731


def _sign(dev, c, x, w, b, alpha, beta, kind, halo=None, with_bits=False):
    _, _, (N, Cout, Ho, Wo) = _shapes(c)
    kw, bufs = {}, [None, None]
    if halo is None or with_bits:
        bufs[0], kw["out_sign"] = _guarded_words(dev, N * Ho * Wo, P.packed_ld(Cout))
    if halo is not None:
        bufs[1], kw["out_nib"] = _guarded_words(dev, N * (Ho + 2 * halo[0]) * (Wo + 2 * halo[1]), P.pixel_ld_nib(Cout))
    before = _lib.call_counts.get(SIGN, 0)
    out, hw = ops.grouped_mfma_conv2d_sign(_planes_of(dev, x), _to(dev, w), None if b is None else _to(dev, b), _to(dev, alpha),
                                           _to(dev, beta), c[7], c[8], 1, c[0], kind=kind, shape=x.shape, out_halo=halo,
                                           with_bits=with_bits, **kw)
    assert _lib.call_counts[SIGN] == before + 1 and hw == (Ho, Wo) and all(_intact(b_) for b_ in bufs if b_ is not None)
    planes = out if isinstance(out, tuple) else (out,)
    got = [pl.sign.cpu().numpy() if isinstance(pl, ops.BitPlanes) else pl.words.cpu().numpy() for pl in planes]
    return got if with_bits else got[0]


def _f32(dev, c, x, w, b, kind, layout):
    buf, out = _guarded_f32(dev, _shapes(c)[2], layout)
    before = _lib.call_counts.get(F32, 0)
    y = ops.grouped_mfma_conv2d_from_bits(_planes_of(dev, x), x.shape, _to(dev, w), None if b is None else _to(dev, b), c[7], c[8], 1,
                                          c[0], kind=kind, out=out)
    assert y is out and _intact(buf) and _lib.call_counts[F32] == before + 1
    return y.cpu().numpy()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_every_output_form_with_real_valued_weights_of_every_kind(dev, i):
    c, kind = CASES[i], KINDS[i % 3]
    xs, ws, ys = _shapes(c)
    x, w = X.pm1(100 + i, xs), X.weights(200 + i, ws)
    wq = X.quantize(w, "ternary" if kind == "raw" else kind)
    assert kind == "binary" or ((wq == 0).any() and (wq > 0).any() and (wq < 0).any())
    w_in = wq if kind == "raw" else w
    b = X.gauss6(300 + i, (ys[1],)) if i % 2 == 0 else None
    y = _ref(c, x, wq, b)
    r = np.random.RandomState(400 + i)
    alpha = r.randn(ys[1]).astype(np.float32)
    alpha[1::5] = 0
    beta = (r.randn(ys[1]) * 3).astype(np.float32)
    neg = P.threshold_bits(y, alpha, beta)
    args = (dev, c, x, w_in, b, alpha, beta, kind)
    assert np.array_equal(_sign(*args), P.pack_sign(neg))
    for halo in HALOS:
        assert np.array_equal(_sign(*args, halo=halo), P.pack_nib(neg, halo)), halo
    both = _sign(*args, halo=HALOS[i % 3], with_bits=True)
    assert np.array_equal(both[0], P.pack_sign(neg)) and np.array_equal(both[1], P.pack_nib(neg, HALOS[i % 3]))
    for layout in ("nchw", "channels_last"):
        assert np.array_equal(_f32(dev, c, x, w_in, b, kind, layout), y), layout


@pytest.mark.parametrize("i", (0, 2, 5))
def test_all_ones_extreme_sums_border_counts_and_exact_ties_give_bit_0(dev, i):
    c = CASES[i]
    xs, ws, ys = _shapes(c)
    x, w = np.ones(xs, dtype=np.float32), np.ones(ws, dtype=np.float32)
    b = ((X.small_ints(500 + i, (ys[1],)) + np.float32(0.25)) * np.float32(1.3)).astype(np.float32)
    y, y0 = _ref(c, x, w, b), _ref(c, x, w, None)
    assert np.abs(y0).max() == c[1] * c[6] * c[6] and len(np.unique(y0)) > (c[8] != (0, 0))
    assert np.array_equal(_f32(dev, c, x, w, b, "binary", "nchw"), y)
    t = y[0, np.arange(ys[1]), ys[2] // 2, (np.arange(ys[1]) * 3) % ys[3]]           # outputs the channels really take, border columns among them
    alpha, beta = np.ones(ys[1], dtype=np.float32), (-t).astype(np.float32)
    neg = P.threshold_bits(y, alpha, beta)
    assert ((y + beta[None, :, None, None]) == 0).any() and not neg[(y + beta[None, :, None, None]) == 0].any()
    assert np.array_equal(_sign(dev, c, x, w, b, alpha, beta, "raw"), P.pack_sign(neg))
    assert np.array_equal(_sign(dev, c, -x, w, b, alpha, beta, "raw", halo=(1, 1)), P.pack_nib(P.threshold_bits(_ref(c, -x, w, b), alpha, beta), (1, 1)))


def test_wrappers_check_their_operands_and_launch_nothing(dev):
    before = dict(_lib.call_counts)
    for ci, co, k, d in ((8, 16, 3, 1), (24, 16, 3, 1), (16, 24, 3, 1), (16, 16, 5, 1), (16, 16, 3, 2)):       # outside the window
        x = X.pm1(1, (1, 8 * ci, 9, 9))
        w, a = _to(dev, X.grid_weights(2, (8 * co, ci, k, k))), torch.ones(8 * co, device=dev)
        with pytest.raises(ValueError):
            ops.grouped_mfma_conv2d_sign(_planes_of(dev, x), w, None, a, a, 1, 1, d, 8, shape=x.shape)
    x = X.pm1(1, (1, 128, 5, 5))
    pl, w, a = _planes_of(dev, x), _to(dev, X.grid_weights(2, (128, 16, 3, 3))), torch.ones(128, device=dev)
    with pytest.raises(TypeError):
        ops.grouped_mfma_conv2d_sign(_to(dev, x), w, None, a, a, 1, 1, 1, 8)                  # an fp32 tensor: that form is not built
    with pytest.raises(ValueError):
        ops.grouped_mfma_conv2d_sign(pl, w, None, a, a, 1, 1, 1, 8)                           # no logical shape
    with pytest.raises(ValueError):
        ops.grouped_mfma_conv2d_sign(pl, w, None, torch.ones(127, device=dev), a, 1, 1, 1, 8, shape=x.shape)
    empty = ops.BitPlanes(sign=pl.sign[:0], rows=0, K=128)
    out, hw = ops.grouped_mfma_conv2d_sign(empty, w, None, a, a, 1, 1, 1, 8, shape=(0, 128, 5, 5))
    assert out.sign.shape == (0, 4) and hw == (5, 5) and _delta(dict(_lib.call_counts), before) == {}


@pytest.mark.parametrize("family,pool,cg", (("binary", None, 16), ("ternary", "before_bn", 32), ("binary", "after_sign", 32), ("ternary", None, 16)))
def test_unmodified_triple_runs_as_fused_chains(dev, family, pool, cg):
    seq = _triple(dev, (BinConv2d if family == "binary" else TerConv2d)(8 * cg, 8 * cg, 3, padding=1, groups=8), pool)
    x = _pm1((3, 16, 10, 10), dev)
    with torch.no_grad(), lazy.grouped_mfma_deferred(True):
        with lazy.eager():
            e = seq(x)
        lazy.STATS.clear()
        y, d = _counted(lambda: seq(x))
        stats = dict(lazy.STATS)
        assert isinstance(y, lazy.LazyActivation) and torch.equal(y.value(), e)
    assert stats.get("deferred") == 3 and stats.get("fused") == 2 and stats.get("materialised", 0) == 0, stats
    assert d.get(SIGN) == 1 and EAGER not in d and F32 not in d, d


def test_a_tensor_op_behind_the_grouped_conv_materialises_from_planes(dev):
    head = _ready(nn.Sequential(BinConv2d(8, 144, 1), *_run(144, torch.Generator().manual_seed(17)),
                                TerConv2d(144, 288, 3, stride=2, padding=1, groups=9)), dev)
    x = _pm1((3, 8, 9, 8), dev, 4)
    with torch.no_grad(), lazy.grouped_mfma_deferred(True):
        with lazy.eager():
            e = head(x)
        got, d = _counted(lambda: head(x) * 1.0)
    assert type(got) is torch.Tensor and torch.equal(got, e) and d.get(F32) == 1 and EAGER not in d and SIGN not in d, d


def test_explicit_fused_form_and_hipgraph_replay(dev):
    seq = _triple(dev, BinConv2d(128, 256, 3, padding=1, groups=8))
    x, x2 = _pm1((3, 16, 10, 10), dev), _pm1((3, 16, 10, 10), dev, 9)
    seq[0].binary_input = True              # the +-1 hint: nothing asks the device about the input while the graph is captured
    with torch.no_grad(), lazy.grouped_mfma_deferred(True):
        with lazy.eager():
            e, e2 = seq(x), seq(x2)
        fused = fuse_sequential(seq, fuse_conv=True, fold="device")
        assert [type(m) for m in fused] == [FusedConvPoolBnSign, FusedGroupedMfmaBnSign, FusedConvPoolBnSign]
        out, d = _counted(lambda: fused(x))
        assert d.get(SIGN) == 1 and EAGER not in d
        assert np.array_equal(out.planes.sign.cpu().numpy(), P.pack_sign((e < 0).cpu().numpy()))
        graph = utils.graphed(seq, x)
        assert torch.equal(_value(graph(x)), e) and torch.equal(_value(graph(x2)), e2) and not torch.equal(e, e2)


@pytest.mark.parametrize("name", ("taken", "cin_g24", "groups4", "off_grid", "training", "fp32_head"))
def test_switch_off_and_declined_layers_run_the_launches_of_the_parent(dev, name):
    """Off: the parent's launches (qt_gmconv2d_f32), no new entry.  Declined layers: the same launches on and off ("taken": control)."""
    layer = (BinConv2d(192, 128, 3, padding=1, groups=8) if name == "cin_g24" else
             TerConv2d(64, 64, 3, padding=1, groups=4) if name == "groups4" else BinConv2d(128, 128, 3, padding=1, groups=8))
    if name == "fp32_head":
        seq = _ready(nn.Sequential(layer, *_run(128, torch.Generator().manual_seed(3)), BinConv2d(128, 16, 1)), dev)
        x = _pm1((2, 128, 9, 9), dev, 2)
    else:
        seq, x = _triple(dev, layer, tail_run=False), _pm1((2, 16, 9, 9), dev, 2)
    if name == "off_grid":
        seq[4].weight.data.mul_(0.3)
        seq[4].reset_quant_cache()
    elif name == "training":
        seq[4].train()
    runs = {}
    with torch.no_grad():
        with lazy.eager():
            e = seq(x)
        for on in (False, True, False, True):             # the first pair warms the layers' caches
            with lazy.grouped_mfma_deferred(on):
                got, runs[on] = _counted(lambda: _value(seq(x)))
            assert torch.equal(got, e), on
    assert SIGN not in runs[False] and F32 not in runs[False] and (name not in ("taken", "cin_g24", "fp32_head") or runs[False].get(EAGER) == 1), runs
    assert (runs[True].get(SIGN) == 1 and EAGER not in runs[True]) if name == "taken" else runs[True] == runs[False], runs
