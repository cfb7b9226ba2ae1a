"""Depthwise convs (groups == in_channels) on the GPU: csrc/dwconv.hip through ops.depthwise_conv2d*, DepthwiseConv2dFn and the
BinConv2d / TerConv2d / DorefaConv2d layers, against the independent reference of tests/_dw_exact.py (pinned on the CPU by
tests/test_dw_exact_cpu.py).

Forward and grad_input have a pinned summation order: they are compared for BIT equality with the ordered float32 restatement,
and with float64 exactly on integer operands.  grad_weight is an fp32 reduction in a fixed but unstated order: within
1.01 (L + 1) 2^-24 sum |go x| of float64, exact on integer operands, bit-identical when run twice.  Every output lies between
sentinels.  All shapes are small: the whole file runs in a few seconds."""
import copy
import functools

import numpy as np
import pytest
import torch

import _dw_exact as D
from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, DorefaConv2d
from pytorch_quantize_impls_amd.utils.graphs import _no_collection_inside

pytestmark = pytest.mark.gpu

TOL = 1e-5
SENTINEL = 12345.0
PAD = 67
CASES = D.cases()
FWD, GIN, GWT = "qt_dwconv2d_f32", "qt_dwconv2d_grad_input_f32", "qt_dwconv2d_grad_weight_f32"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def nerr(got, want):
    """File-local normalised error: max |got - want| over max |want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _to(dev, a, layout="nchw"):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" and t.dim() == 4 else t


def _guarded(dev, shape, layout="nchw"):
    """(buffer, view): ``view`` is a dense tensor of ``shape`` in ``layout`` with PAD sentinel elements on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)
    mid = buf[PAD:PAD + n]
    if layout == "channels_last" and len(shape) == 4:
        N, C, H, W = shape
        return buf, mid.view(N, H, W, C).permute(0, 3, 1, 2)
    return buf, mid.view(*shape)


def _intact(buf):
    return bool((buf[:PAD] == SENTINEL).all() and (buf[-PAD:] == SENTINEL).all())


def _geom(c):
    return c.kernel, c.stride, c.padding, c.dilation


def _shapes(c):
    Ho, Wo = D.out_hw(c.H, c.W, *_geom(c))
    return (c.N, c.C, c.H, c.W), (c.C * c.m,) + tuple(c.kernel), (c.N, c.C * c.m, Ho, Wo)


def _run_forward(dev, c, x, w, b, kind):
    buf, out = _guarded(dev, _shapes(c)[2], c.layout)
    y = ops.depthwise_conv2d(_to(dev, x, c.layout), _to(dev, w).unsqueeze(1), None if b is None else _to(dev, b), c.stride, c.padding,
                             c.dilation, kind=kind, out=out)
    assert y is out and _intact(buf)
    return y.cpu().numpy()


def _run_grad_input(dev, c, go, w, kind):
    xs = _shapes(c)[0]
    buf, out = _guarded(dev, xs, c.layout)
    gx = ops.depthwise_conv2d_grad_input(xs, _to(dev, w).unsqueeze(1), _to(dev, go, c.layout), c.stride, c.padding, c.dilation, kind=kind,
                                         out=out)
    assert gx is out and _intact(buf)
    return gx.cpu().numpy()


def _run_grad_weight(dev, c, x, go, w, thr, go_layout=None):
    ws = _shapes(c)[1]
    bw, ow = _guarded(dev, (ws[0], 1) + ws[1:])
    bb, ob = _guarded(dev, (ws[0],))
    need = ops.depthwise_grad_weight_work_floats(x.shape, (ws[0], 1) + ws[1:], c.stride, c.padding, c.dilation)
    bk, work = _guarded(dev, (need,))
    gw, gb = ops.depthwise_conv2d_grad_weight(_to(dev, x, c.layout), _to(dev, go, go_layout or c.layout), _to(dev, w).unsqueeze(1), c.stride,
                                              c.padding, c.dilation, ste_threshold=thr, out=ow, out_bias=ob, workspace=work)
    assert gw is ow and gb is ob and _intact(bw) and _intact(bb) and _intact(bk)
    return gw.cpu().numpy().reshape(ws), gb.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(i):
    """Inputs and references of case i, computed once: per data class the ordered-float32 forward and grad_input, and for the
    Gaussian class the float64 grad_weight with its bound."""
    c = CASES[i]
    xs, ws, ys = _shapes(c)
    kind = D.KINDS[i % 3]
    w = D.weights(100 + i, ws)
    wq = D.quantize(w, kind)
    b = D.gauss6(200 + i, (ws[0],)) if i % 2 == 0 else None
    out = {"kind": kind, "w": w, "b": b}
    for name, gen in (("pm1", D.pm1), ("gauss", D.gauss6)):
        x, go = gen(300 + i, xs), gen(400 + i, ys)
        out[name] = dict(x=x, go=go, y=D.forward(x, wq, b, *_geom(c)), gx=D.grad_input(go, wq, xs, *_geom(c)))
    g = out["gauss"]
    g["gw"], g["ab"], g["gb"] = D.grad_weight(g["x"], g["go"], *_geom(c))
    # designed integer operands: +-1 activations, +-1 / 0 weights, small integer bias and gradient
    wi, bi = D.grid_weights(500 + i, ws), D.small_ints(600 + i, (ws[0],))
    xi, gi = D.pm1(700 + i, xs), D.small_ints(800 + i, ys)
    out["int"] = dict(x=xi, go=gi, w=wi, b=bi, y=D.forward(xi, wi, bi, *_geom(c), dtype=np.float64),
                      gx=D.grad_input(gi, wi, xs, *_geom(c), dtype=np.float64))
    out["int"]["gw"], _, out["int"]["gb"] = D.grad_weight(xi, gi, *_geom(c))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_ops_forward_and_grad_input_bit_for_bit(dev, i):
    c, r = CASES[i], _reference(i)
    for name in ("pm1", "gauss"):
        d = r[name]
        y = _run_forward(dev, c, d["x"], r["w"], r["b"], r["kind"])
        assert y.dtype == np.float32 and np.array_equal(y, d["y"]), (name, nerr(y, d["y"]))
        gx = _run_grad_input(dev, c, d["go"], r["w"], r["kind"])
        assert np.array_equal(gx, d["gx"]), (name, nerr(gx, d["gx"]))
    d = r["int"]
    for kind in ("raw", "ternary"):          # the weights are fixed points of the ternary quantiser
        assert np.array_equal(_run_forward(dev, c, d["x"], d["w"], d["b"], kind).astype(np.float64), d["y"])
        assert np.array_equal(_run_grad_input(dev, c, d["go"], d["w"], kind).astype(np.float64), d["gx"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_ops_grad_weight_bound_exact_integers_and_repeatable(dev, i):
    c, r = CASES[i], _reference(i)
    d = r["gauss"]
    thr = 0.0 if r["kind"] == "raw" else float(D.STE)
    L = c.N * d["go"].shape[2] * d["go"].shape[3]
    gw, gb = _run_grad_weight(dev, c, d["x"], d["go"], r["w"], thr)
    want = D.ste_mask(d["gw"], r["w"], thr)
    err, bound = np.abs(gw.astype(np.float64) - want), D.grad_weight_bound(d["ab"], L)
    assert (err <= bound).all(), (float((err - bound).max()), nerr(gw, want))
    if thr > 0:
        assert (gw[np.abs(r["w"]) > D.STE] == 0).all()
    gb_bound = D.grad_weight_bound(np.abs(d["go"].astype(np.float64)).sum((0, 2, 3)), L)
    assert (np.abs(gb.astype(np.float64) - d["gb"]) <= gb_bound).all()
    gw2, gb2 = _run_grad_weight(dev, c, d["x"], d["go"], r["w"], thr)
    assert np.array_equal(gw, gw2) and np.array_equal(gb, gb2)
    # the gradient in the other layout: another walk, the same bound
    other = "nchw" if c.layout == "channels_last" else "channels_last"
    gw3, _ = _run_grad_weight(dev, c, d["x"], d["go"], r["w"], thr, go_layout=other)
    assert (np.abs(gw3.astype(np.float64) - want) <= bound).all()
    d = r["int"]
    gwi, gbi = _run_grad_weight(dev, c, d["x"], d["go"], d["w"], 0.0)
    assert np.array_equal(gwi.astype(np.float64), d["gw"]) and np.array_equal(gbi.astype(np.float64), d["gb"])


def test_allocating_wrappers_keep_the_layout_and_count_their_calls(dev):
    before = dict(_lib.call_counts)
    for layout in D.LAYOUTS:
        x = _to(dev, D.gauss6(1, (2, 6, 9, 8)), layout)
        w = _to(dev, D.weights(2, (12, 1, 3, 3)))
        y = ops.depthwise_conv2d(x, w, None, 2, 1, 1, kind="binary")
        assert y.shape == (2, 12, 5, 4) and y.is_contiguous(memory_format=torch.channels_last) == (layout == "channels_last")
        gx = ops.depthwise_conv2d_grad_input(x.shape, w, y, 2, 1, 1, kind="binary")
        assert gx.shape == x.shape and gx.stride() == x.stride()
        gw, gb = ops.depthwise_conv2d_grad_weight(x, y, w, 2, 1, 1, want_bias=True)
        assert gw.shape == w.shape and gb.shape == (12,)
        assert ops.depthwise_conv2d_grad_weight(x, y, w, 2, 1, 1)[1] is None
    used = {k: _lib.call_counts[k] - before.get(k, 0) for k in (FWD, GIN, GWT)}
    assert used == {FWD: 2, GIN: 2, GWT: 4}
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, _to(dev, D.weights(3, (12, 2, 3, 3))), None, 1, 1, 1)
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, w, None, 1, 1, 1, out=torch.empty(2, 12, 9, 9, device=dev))
    e = torch.empty(0, 6, 9, 8, device=dev)
    assert ops.depthwise_conv2d(e, w, None, 2, 1, 1).shape == (0, 12, 5, 4)
    gw0, gb0 = ops.depthwise_conv2d_grad_weight(e, torch.empty(0, 12, 5, 4, device=dev), w, 2, 1, 1, want_bias=True)
    assert not gw0.any() and not gb0.any()


# ---- the quantisers inside the kernels -------------------------------------------------------------------------------------------

def _edge_case():
    return D.Case(C=3, m=2, N=2, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), H=6, W=7, layout="nchw")


@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_quantiser_edges_inside_the_kernels(dev, layout):
    c = _edge_case()
    c["layout"] = layout
    xs, ws, ys = _shapes(c)
    x, go = D.small_ints(1, xs), D.small_ints(2, ys)
    w = D.weights(3, ws)
    tiny = np.float32(1e-45)
    assert tiny > 0 and tiny == np.nextafter(np.float32(0), np.float32(1))
    w.reshape(-1)[:10] = [-0.0, 0.0, np.nan, tiny, -tiny, 0.5, -0.5, np.nextafter(np.float32(0.5), np.float32(0)),
                          np.nextafter(np.float32(-0.5), np.float32(-1)), -0.25]
    wb = D.quantize(w, "binary")
    assert wb.reshape(-1)[:5].tolist() == [1, 1, 1, 1, -1]                      # -0.0, NaN -> +1; the subnormals keep their sign
    assert np.array_equal(_run_forward(dev, c, x, w, None, "binary"), D.forward(x, wb, None, *_geom(c)))
    assert np.array_equal(_run_grad_input(dev, c, go, w, "binary"), D.grad_input(go, wb, xs, *_geom(c)))
    wt = np.where(np.isnan(w), np.float32(0.75), w)                            # ternary: thresholds +-0.5 exactly
    wq = D.quantize(wt, "ternary")
    assert wq.reshape(-1)[5:9].tolist() == [1, 0, 0, -1]
    assert np.array_equal(_run_forward(dev, c, x, wt, None, "ternary"), D.forward(x, wq, None, *_geom(c)))
    assert np.array_equal(_run_grad_input(dev, c, go, wt, "ternary"), D.grad_input(go, wq, xs, *_geom(c)))
    # the STE mask: |w| == 1.001 passes, the next float above it does not; NaN passes (|NaN| > thr is false)
    above = np.nextafter(D.STE, np.float32(2))
    wm = D.weights(4, ws)
    wm.reshape(-1)[:5] = [D.STE, -D.STE, above, -above, np.nan]
    gw, _ = _run_grad_weight(dev, c, x, go, wm, float(D.STE))
    ref = D.grad_weight(x, go, *_geom(c))[0]
    want = D.ste_mask(ref, wm)
    assert np.array_equal(gw.astype(np.float64), want)                          # integer operands: exact
    assert want.reshape(-1)[2] == 0 and want.reshape(-1)[3] == 0
    assert np.array_equal(want.reshape(-1)[[0, 1, 4]], ref.reshape(-1)[[0, 1, 4]])
    gw0, _ = _run_grad_weight(dev, c, x, go, wm, 0.0)
    assert np.array_equal(gw0.astype(np.float64), ref)


@pytest.mark.parametrize("layout", D.LAYOUTS)
def test_nan_and_inf_reach_exactly_the_windows_that_hold_them(dev, layout):
    c = D.Case(C=2, m=2, N=1, kernel=(3, 3), stride=(2, 1), padding=(1, 1), dilation=(1, 1), H=9, W=11, layout=layout)
    xs, ws, ys = _shapes(c)
    x = D.gauss6(1, xs)
    x[0, 0, 0, 0], x[0, 0, 7, 9], x[0, 1, 4, 5] = np.nan, np.inf, -np.inf
    w = D.weights(2, ws)
    y = _run_forward(dev, c, x, w, None, "binary")
    want = D.forward(x, D.quantize(w, "binary"), None, *_geom(c))
    assert np.array_equal(y, want, equal_nan=True)
    touched = D.forward((~np.isfinite(x)).astype(np.float64), np.ones(ws), None, *_geom(c), dtype=np.float64) > 0
    assert np.array_equal(~np.isfinite(y), touched) and 0 < touched.sum() < touched.size
    go = D.gauss6(3, ys)
    go[0, 1, 2, 3], go[0, 2, 0, 10] = np.nan, np.inf
    gx = _run_grad_input(dev, c, go, w, "binary")
    assert np.array_equal(gx, D.grad_input(go, D.quantize(w, "binary"), xs, *_geom(c)), equal_nan=True)
    hit = D.grad_input((~np.isfinite(go)).astype(np.float64), np.ones(ws), xs, *_geom(c), dtype=np.float64) > 0
    assert np.array_equal(~np.isfinite(gx), hit) and 0 < hit.sum() < hit.size


# ---- the layers ------------------------------------------------------------------------------------------------------------------

def _make(kind, C, m, dev):
    kw = dict(stride=2, padding=1, groups=C, bias=True)
    g = np.random.RandomState(len(kind) * 7 + m)
    if kind == "bin":
        layer = BinConv2d(C, C * m, 3, **kw)
    elif kind == "ter":
        layer = TerConv2d(C, C * m, 3, **kw)
    elif kind == "ter_stochastic":
        layer = TerConv2d(C, C * m, 3, deterministic=False, **kw)
    elif kind == "bin_stochastic":
        layer = BinConv2d(C, C * m, 3, deterministic=False, **kw)
    else:
        layer = DorefaConv2d(C, C * m, 3, bit_width=int(kind[1:]), **kw)
    if kind.endswith("stochastic"):
        # |w| >= 1: the draw is certain; half of the magnitudes lie above the STE bound 1.001
        w = np.where(g.rand(C * m, 1, 3, 3) < 0.5, 1.0, 1.25) * np.where(g.rand(C * m, 1, 3, 3) < 0.5, -1.0, 1.0)
    else:
        w = g.uniform(-1.4, 1.4, size=(C * m, 1, 3, 3))
    layer.weight.data.copy_(torch.from_numpy(w.astype(np.float32)))
    layer.bias.data.copy_(torch.from_numpy(g.uniform(-1, 1, size=(C * m,)).astype(np.float32)))
    return layer.to(dev)


LAYER_KINDS = ("bin", "ter", "bin_stochastic", "ter_stochastic", "k1", "k4", "k32")


@pytest.mark.parametrize("m", (1, 2))
@pytest.mark.parametrize("kind", LAYER_KINDS)
def test_layers_train_step_and_eval_on_the_depthwise_route(dev, kind, m):
    C = 10
    layer = _make(kind, C, m, dev)
    ref = copy.deepcopy(layer).cpu().double()               # host tensors: F.conv2d(x, Q(W), b, groups = C) with the quantiser's own backward
    x = D.gauss6(5, (3, C, 9, 7))
    Ho, Wo = D.out_hw(9, 7, 3, 2, 1, 1)
    go = D.gauss6(6, (3, C * m, Ho, Wo)) * 1e-2
    xr = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    yr = ref(xr)
    yr.backward(torch.from_numpy(go.astype(np.float64)))
    xd = _to(dev, x).requires_grad_(True)
    calls, reasons = dict(_lib.call_counts), dict(_fused.LIBRARY_PATHS)
    y = layer(xd)
    y.backward(_to(dev, go))
    torch.cuda.synchronize()
    used = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
    assert (used.get(FWD), used.get(GIN), used.get(GWT)) == (1, 1, 1), used
    assert not [k for k in used if k.startswith("qt_conv2d_implicit")], used
    assert dict(_fused.LIBRARY_PATHS) == reasons
    errs = dict(y=nerr(y.detach().cpu(), yr.detach()), gx=nerr(xd.grad.cpu(), xr.grad),
                gw=nerr(layer.weight.grad.cpu(), ref.weight.grad), gb=nerr(layer.bias.grad.cpu(), ref.bias.grad))
    print(kind, m, errs)
    assert max(errs.values()) <= TOL, errs
    if not kind.startswith("k"):
        assert (layer.weight.grad[layer.weight.detach().abs() > 1.001] == 0).all()
    # eval: the stored image, the same launch, the same bits — without autograd and with it
    layer.eval()
    calls = dict(_lib.call_counts)
    with torch.no_grad():
        ye = layer(_to(dev, x))
    assert isinstance(ye, torch.Tensor) and ye.dtype == torch.float32 and torch.equal(ye, y.detach())
    xe = _to(dev, x).requires_grad_(True)
    ya = layer(xe)
    assert torch.equal(ya.detach(), y.detach())
    ya.backward(_to(dev, go))
    assert nerr(xe.grad.cpu(), xr.grad) <= TOL
    used = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
    assert used.get(FWD) == 2 and used.get(GIN) == 1 and not [k for k in used if k.startswith("qt_conv2d_implicit")], used
    assert dict(_fused.LIBRARY_PATHS) == reasons


@pytest.mark.parametrize("kind", ("binary", "ternary"))
def test_pm1_data_equals_the_per_group_loop(dev, kind):
    C = 4
    layer = (BinConv2d if kind == "binary" else TerConv2d)(C, 2 * C, 3, padding=1, groups=C).to(dev)
    layer.weight.data.copy_(_to(dev, D.weights(9, (2 * C, 1, 3, 3))))
    x = _to(dev, D.pm1(10, (2, C, 8, 8)))
    calls = dict(_lib.call_counts)
    with torch.no_grad():
        y = layer(x)
        assert _lib.call_counts[FWD] - calls.get(FWD, 0) == 1
        old = _fused.grouped_quant_conv(layer, x, kind, layer._op)
    assert old is not None and torch.equal(y, old)


def test_two_channel_groups_stay_off_the_depthwise_route(dev):
    layer = BinConv2d(4, 4, 3, padding=1, groups=2).to(dev)
    assert not _fused.depthwise_route(layer, torch.empty(2, 4, 8, 8, device=dev))
    x = _to(dev, D.pm1(11, (2, 4, 8, 8))).requires_grad_(True)
    calls = dict(_lib.call_counts)
    layer(x).sum().backward()
    d = DorefaConv2d(4, 4, 3, padding=1, groups=2, bit_width=4).to(dev)
    d(x.detach()).sum().backward()
    assert not [k for k in _lib.call_counts if k.startswith("qt_dwconv2d") and _lib.call_counts[k] != calls.get(k, 0)]
    # an off-grid eval weight of a depthwise layer keeps the library expression and its reason
    dw = BinConv2d(4, 4, 3, padding=1, groups=4).to(dev).eval()
    dw.weight.data.copy_(_to(dev, D.weights(12, (4, 1, 3, 3))))
    dw.reset_quant_cache()
    reasons = dict(_fused.LIBRARY_PATHS)
    with torch.no_grad():
        y = dw(x.detach())
    assert _lib.call_counts[FWD] == calls.get(FWD, 0)
    assert sum(_fused.LIBRARY_PATHS.values()) == sum(reasons.values()) + 1
    assert _fused.LIBRARY_PATHS["eval-mode weight off the quantiser's grid"] == reasons.get("eval-mode weight off the quantiser's grid", 0) + 1
    assert nerr(y.cpu(), torch.nn.functional.conv2d(x.detach().cpu(), dw.weight.detach().cpu(), dw.bias.detach().cpu(), 1, 1, 1, 4)) <= TOL


def test_forward_and_backward_replay_from_a_captured_graph(dev):
    C = 6
    layer = _make("ter", C, 2, dev)
    xs = _to(dev, D.gauss6(20, (2, C, 9, 7))).requires_grad_(True)
    gs = _to(dev, D.gauss6(21, (2, 2 * C, 5, 4)))

    def step():
        layer.zero_grad(set_to_none=False)
        if xs.grad is not None:
            xs.grad.zero_()
        y = layer(xs)
        y.backward(gs)
        return y.detach()

    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        torch.cuda.synchronize(dev)
        with _no_collection_inside(), torch.cuda.graph(graph, stream=stream):
            y_static = step()
    torch.cuda.synchronize(dev)
    x2, g2 = _to(dev, D.gauss6(22, (2, C, 9, 7))), _to(dev, D.gauss6(23, (2, 2 * C, 5, 4)))
    with torch.no_grad():
        xs.copy_(x2)
        gs.copy_(g2)
    calls = dict(_lib.call_counts)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert _lib.call_counts[FWD] == calls.get(FWD, 0)                     # a replay, not a call
    got = (y_static.clone(), xs.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone())
    twin = copy.deepcopy(layer)
    twin.zero_grad(set_to_none=True)
    xe = x2.clone().requires_grad_(True)
    ye = twin(xe)
    ye.backward(g2)
    for a, b in zip(got, (ye.detach(), xe.grad, twin.weight.grad, twin.bias.grad)):
        assert torch.equal(a, b)
