"""Grouped convs with a few channels per group on the GPU: csrc/gconv.hip through ops.grouped_conv2d*, GroupedConv2dFn and the
BinConv2d / TerConv2d / DorefaConv2d layers, against the independent reference of tests/_gconv_exact.py (pinned on the CPU by
tests/test_gconv_exact_cpu.py).

Forward and grad_input have a pinned summation order: they are compared for BIT equality with the ordered float32 restatement,
and with float64 exactly on integer operands.  grad_weight is an fp32 reduction in a fixed but unstated order: within
1.01 (L + 1) 2^-24 sum |go x| of float64, exact on integer operands, bit-identical when run twice.  Every output lies between
sentinels.  All shapes are small: a case takes well under a second."""
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

TOL = 1e-5
SENTINEL = 12345.0
PAD = 67
CASES = R.cases()
FWD, GIN, GWT = "qt_gconv2d_f32", "qt_gconv2d_grad_input_f32", "qt_gconv2d_grad_weight_f32"


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


def _conv(c):
    return c.stride, c.padding, c.dilation, c.G


def _run_forward(dev, c, x, w, b, kind):
    buf, out = _guarded(dev, c.shapes[2], c.layout[1])
    y = ops.grouped_conv2d(_to(dev, x, c.layout[0]), _to(dev, w), None if b is None else _to(dev, b), *_conv(c), kind=kind, out=out)
    assert y is out and _intact(buf)
    return y.cpu().numpy()


def _run_grad_input(dev, c, go, w, kind):
    xs = c.shapes[0]
    buf, out = _guarded(dev, xs, c.layout[0])
    gx = ops.grouped_conv2d_grad_input(xs, _to(dev, w), _to(dev, go, c.layout[1]), *_conv(c), kind=kind, out=out)
    assert gx is out and _intact(buf)
    return gx.cpu().numpy()


def _run_grad_weight(dev, c, x, go, w, thr, go_layout=None):
    ws = c.shapes[1]
    bw, ow = _guarded(dev, ws)
    bb, ob = _guarded(dev, (ws[0],))
    need = ops.grouped_grad_weight_work_floats(x.shape, ws, *_conv(c))
    bk, work = _guarded(dev, (need,))
    gw, gb = ops.grouped_conv2d_grad_weight(_to(dev, x, c.layout[0]), _to(dev, go, go_layout or c.layout[1]), _to(dev, w), *_conv(c),
                                            ste_threshold=thr, out=ow, out_bias=ob, workspace=work)
    assert gw is ow and gb is ob and _intact(bw) and _intact(bb) and _intact(bk)
    return gw.cpu().numpy(), gb.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _data(i):
    """Inputs of case i, made once and left unchanged: Gaussian operands over six decades, and designed integer operands (+-1
    activations, +-1 / 0 weights, small integer bias and gradient)."""
    c = CASES[i]
    xs, ws, ys = c.shapes
    return dict(w=R.weights(100 + i, ws), b=R.gauss6(200 + i, (ws[0],)) if i % 2 == 0 else None,
                x=R.gauss6(300 + i, xs), go=R.gauss6(400 + i, ys),
                wi=R.grid_weights(500 + i, ws), bi=R.small_ints(600 + i, (ws[0],)), xi=R.pm1(700 + i, xs),
                gi=R.small_ints(800 + i, ys, -2, 2))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_ops_forward_and_grad_input_bit_for_bit(dev, i):
    c, d = CASES[i], _data(i)
    xs = c.shapes[0]
    for kind in R.KINDS:
        wq = R.quantize(d["w"], kind)
        y = _run_forward(dev, c, d["x"], d["w"], d["b"], kind)
        want = R.forward(d["x"], wq, d["b"], c.G, *c.geom)
        assert y.dtype == np.float32 and np.array_equal(y, want), (kind, nerr(y, want))
        gx = _run_grad_input(dev, c, d["go"], d["w"], kind)
        want = R.grad_input(d["go"], wq, xs, c.G, *c.geom)
        assert np.array_equal(gx, want), (kind, nerr(gx, want))
    y64 = R.forward(d["xi"], d["wi"], d["bi"], c.G, *c.geom, dtype=np.float64)
    g64 = R.grad_input(d["gi"], d["wi"], xs, c.G, *c.geom, dtype=np.float64)
    for kind in ("raw", "ternary"):          # the weights are fixed points of the ternary quantiser
        assert np.array_equal(_run_forward(dev, c, d["xi"], d["wi"], d["bi"], kind).astype(np.float64), y64)
        assert np.array_equal(_run_grad_input(dev, c, d["gi"], d["wi"], kind).astype(np.float64), g64)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.id for c in CASES])
def test_ops_grad_weight_bound_exact_integers_and_repeatable(dev, i):
    c, d = CASES[i], _data(i)
    kind = R.KINDS[i % 3]
    thr = 0.0 if kind == "raw" else float(R.STE)
    ys = c.shapes[2]
    L = c.N * ys[2] * ys[3]
    ref, ab, ref_b = R.grad_weight(d["x"], d["go"], c.G, c.cin_g, *c.geom)
    gw, gb = _run_grad_weight(dev, c, d["x"], d["go"], d["w"], thr)
    want = R.ste_mask(ref, d["w"], thr)
    err, bound = np.abs(gw.astype(np.float64) - want), R.grad_weight_bound(ab, L)
    assert (err <= bound).all(), (float((err - bound).max()), nerr(gw, want))
    if thr > 0:
        assert (gw[np.abs(d["w"]) > R.STE] == 0).all()
    gb_bound = R.grad_weight_bound(np.abs(d["go"].astype(np.float64)).sum((0, 2, 3)), L)
    assert (np.abs(gb.astype(np.float64) - ref_b) <= gb_bound).all()
    gw2, gb2 = _run_grad_weight(dev, c, d["x"], d["go"], d["w"], thr)
    assert np.array_equal(gw, gw2) and np.array_equal(gb, gb2)
    # the gradient in the other layout: another walk, the same bound
    other = "nchw" if c.layout[1] == "channels_last" else "channels_last"
    gw3, gb3 = _run_grad_weight(dev, c, d["x"], d["go"], d["w"], thr, go_layout=other)
    assert (np.abs(gw3.astype(np.float64) - want) <= bound).all() and (np.abs(gb3.astype(np.float64) - ref_b) <= gb_bound).all()
    # designed integer operands: +-1 x, go in {-2 ... 2}, every sum below 2^24 — exact in any order
    refi, abi, refi_b = R.grad_weight(d["xi"], d["gi"], c.G, c.cin_g, *c.geom)
    assert abi.max() < 2 ** 24
    gwi, gbi = _run_grad_weight(dev, c, d["xi"], d["gi"], d["wi"], 0.0)
    assert np.array_equal(gwi.astype(np.float64), refi) and np.array_equal(gbi.astype(np.float64), refi_b)


ONE = [i for i, c in enumerate(CASES) if c.cin_g == 1]


@pytest.mark.parametrize("i", ONE, ids=[CASES[i].id for i in ONE])
def test_one_channel_per_group_gives_the_bits_of_the_depthwise_entries(dev, i):
    c, d = CASES[i], _data(i)
    assert len(ONE) >= 6
    x, go, w = _to(dev, d["x"], c.layout[0]), _to(dev, d["go"], c.layout[1]), _to(dev, d["w"])
    b = None if d["b"] is None else _to(dev, d["b"])
    calls = dict(_lib.call_counts)
    for kind in R.KINDS:
        y = ops.grouped_conv2d(x, w, b, *_conv(c), kind=kind)
        assert torch.equal(y, ops.depthwise_conv2d(x, w, b, c.stride, c.padding, c.dilation, kind=kind))
        gx = ops.grouped_conv2d_grad_input(x.shape, w, go, *_conv(c), kind=kind)
        assert torch.equal(gx, ops.depthwise_conv2d_grad_input(x.shape, w, go, c.stride, c.padding, c.dilation, kind=kind))
    for k in (FWD, GIN, "qt_dwconv2d_f32", "qt_dwconv2d_grad_input_f32"):
        assert _lib.call_counts[k] - calls.get(k, 0) == 3


def test_allocating_wrappers_keep_the_layout_and_count_their_calls(dev):
    before = dict(_lib.call_counts)
    for layout in ("nchw", "channels_last"):
        x = _to(dev, R.gauss6(1, (2, 12, 9, 8)), layout)
        w = _to(dev, R.weights(2, (8, 3, 3, 3)))
        y = ops.grouped_conv2d(x, w, None, 2, 1, 1, 4, kind="binary")
        assert y.shape == (2, 8, 5, 4) and y.is_contiguous(memory_format=torch.channels_last) == (layout == "channels_last")
        gx = ops.grouped_conv2d_grad_input(x.shape, w, y, 2, 1, 1, 4, kind="binary")
        assert gx.shape == x.shape and gx.stride() == x.stride()
        gw, gb = ops.grouped_conv2d_grad_weight(x, y, w, 2, 1, 1, 4, want_bias=True)
        assert gw.shape == w.shape and gb.shape == (8,)
        assert ops.grouped_conv2d_grad_weight(x, y, w, 2, 1, 1, 4)[1] is None
    used = {k: _lib.call_counts[k] - before.get(k, 0) for k in (FWD, GIN, GWT)}
    assert used == {FWD: 2, GIN: 2, GWT: 4}
    with pytest.raises(ValueError):
        ops.grouped_conv2d(x, _to(dev, R.weights(3, (8, 2, 3, 3))), None, 1, 1, 1, 4)
    with pytest.raises(ValueError):
        ops.grouped_conv2d(x, w, None, 1, 1, 1, 4, out=torch.empty(2, 8, 9, 9, device=dev))
    with pytest.raises(ValueError):
        ops.grouped_conv2d(_to(dev, R.gauss6(4, (1, 66, 5, 5))), _to(dev, R.weights(5, (2, 33, 3, 3))), None, 1, 1, 1, 2)   # cin_g 33
    e = torch.empty(0, 12, 9, 8, device=dev)
    assert ops.grouped_conv2d(e, w, None, 2, 1, 1, 4).shape == (0, 8, 5, 4)
    gw0, gb0 = ops.grouped_conv2d_grad_weight(e, torch.empty(0, 8, 5, 4, device=dev), w, 2, 1, 1, 4, want_bias=True)
    assert not gw0.any() and not gb0.any()
    assert {k: _lib.call_counts[k] - before.get(k, 0) for k in (FWD, GIN, GWT)} == used


# ---- the quantisers inside the kernels -------------------------------------------------------------------------------------------

def _edge_case(layout):
    return R.Case(cin_g=3, cout_g=5, G=2, N=2, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), H=6, W=7,
                  layout=(layout, layout))


@pytest.mark.parametrize("layout", ("nchw", "channels_last"))
def test_quantiser_edges_inside_the_kernels(dev, layout):
    c = _edge_case(layout)
    xs, ws, ys = c.shapes
    x, go = R.small_ints(1, xs), R.small_ints(2, ys)
    w = R.weights(3, ws)
    tiny = np.float32(1e-45)
    assert tiny > 0 and tiny == np.nextafter(np.float32(0), np.float32(1))
    w.reshape(-1)[:10] = [-0.0, 0.0, np.nan, tiny, -tiny, 0.5, -0.5, np.nextafter(np.float32(0.5), np.float32(0)),
                          np.nextafter(np.float32(-0.5), np.float32(-1)), -0.25]
    wb = R.quantize(w, "binary")
    assert wb.reshape(-1)[:5].tolist() == [1, 1, 1, 1, -1]                      # -0.0, NaN -> +1; the subnormals keep their sign
    assert np.array_equal(_run_forward(dev, c, x, w, None, "binary"), R.forward(x, wb, None, c.G, *c.geom))
    assert np.array_equal(_run_grad_input(dev, c, go, w, "binary"), R.grad_input(go, wb, xs, c.G, *c.geom))
    wt = np.where(np.isnan(w), np.float32(0.75), w)                            # ternary: thresholds +-0.5 exactly
    wq = R.quantize(wt, "ternary")
    assert wq.reshape(-1)[5:9].tolist() == [1, 0, 0, -1]
    assert np.array_equal(_run_forward(dev, c, x, wt, None, "ternary"), R.forward(x, wq, None, c.G, *c.geom))
    assert np.array_equal(_run_grad_input(dev, c, go, wt, "ternary"), R.grad_input(go, wq, xs, c.G, *c.geom))
    # a NaN weight run "raw" reaches every output of its channel whose window holds the tap, and no other channel
    y = _run_forward(dev, c, x, w, None, "raw")
    assert np.array_equal(y, R.forward(x, w, None, c.G, *c.geom), equal_nan=True)
    assert np.isnan(y[:, 0]).any() and not np.isnan(y[:, 1:]).any()
    # the STE mask: |w| == 1.001 passes, the next float above it does not; NaN passes (|NaN| > thr is false)
    above = np.nextafter(R.STE, np.float32(2))
    wm = R.weights(4, ws)
    wm.reshape(-1)[:5] = [R.STE, -R.STE, above, -above, np.nan]
    gw, _ = _run_grad_weight(dev, c, x, go, wm, float(R.STE))
    ref = R.grad_weight(x, go, c.G, c.cin_g, *c.geom)[0]
    want = R.ste_mask(ref, wm)
    assert np.array_equal(gw.astype(np.float64), want)                          # integer operands: exact
    assert want.reshape(-1)[2] == 0 and want.reshape(-1)[3] == 0
    assert np.array_equal(want.reshape(-1)[[0, 1, 4]], ref.reshape(-1)[[0, 1, 4]])
    gw0, _ = _run_grad_weight(dev, c, x, go, wm, 0.0)
    assert np.array_equal(gw0.astype(np.float64), ref)


@pytest.mark.parametrize("layout", ("nchw", "channels_last"))
def test_nan_and_inf_reach_exactly_the_windows_that_hold_them(dev, layout):
    c = R.Case(cin_g=2, cout_g=3, G=2, N=1, kernel=(3, 3), stride=(2, 1), padding=(1, 1), dilation=(1, 1), H=9, W=11,
               layout=(layout, layout))
    xs, ws, ys = c.shapes
    x = R.gauss6(1, xs)
    x[0, 0, 0, 0], x[0, 1, 7, 9], x[0, 2, 4, 5] = np.nan, np.inf, -np.inf        # two channels of group 0, one of group 1
    w = R.weights(2, ws)
    y = _run_forward(dev, c, x, w, None, "binary")
    want = R.forward(x, R.quantize(w, "binary"), None, c.G, *c.geom)
    assert np.array_equal(y, want, equal_nan=True)
    touched = R.forward((~np.isfinite(x)).astype(np.float64), np.ones(ws), None, c.G, *c.geom, dtype=np.float64) > 0
    assert np.array_equal(~np.isfinite(y), touched) and 0 < touched.sum() < touched.size
    assert touched[:, :3].sum() > touched[:, 3:].sum() > 0                      # the groups do not mix
    go = R.gauss6(3, ys)
    go[0, 1, 2, 3], go[0, 4, 0, 10] = np.nan, np.inf
    gx = _run_grad_input(dev, c, go, w, "binary")
    assert np.array_equal(gx, R.grad_input(go, R.quantize(w, "binary"), xs, c.G, *c.geom), equal_nan=True)
    hit = R.grad_input((~np.isfinite(go)).astype(np.float64), np.ones(ws), xs, c.G, *c.geom, dtype=np.float64) > 0
    assert np.array_equal(~np.isfinite(gx), hit) and 0 < hit.sum() < hit.size


# ---- the layers ------------------------------------------------------------------------------------------------------------------

G, CIN_G = 4, 3


def _make(kind, cout_g, dev, groups=G, cin_g=CIN_G):
    C, Cout = groups * cin_g, groups * cout_g
    kw = dict(stride=2, padding=1, groups=groups, bias=True)
    g = np.random.RandomState(len(kind) * 7 + cout_g)
    if kind == "bin":
        layer = BinConv2d(C, Cout, 3, **kw)
    elif kind == "ter":
        layer = TerConv2d(C, Cout, 3, **kw)
    elif kind == "ter_stochastic":
        layer = TerConv2d(C, Cout, 3, deterministic=False, **kw)
    elif kind == "bin_stochastic":
        layer = BinConv2d(C, Cout, 3, deterministic=False, **kw)
    else:
        layer = DorefaConv2d(C, Cout, 3, bit_width=int(kind[1:]), **kw)
    shape = (Cout, cin_g, 3, 3)
    if kind.endswith("stochastic"):
        # |w| >= 1: the draw is certain; half of the magnitudes lie above the STE bound 1.001
        w = np.where(g.rand(*shape) < 0.5, 1.0, 1.25) * np.where(g.rand(*shape) < 0.5, -1.0, 1.0)
    else:
        w = g.uniform(-1.4, 1.4, size=shape)
    layer.weight.data.copy_(torch.from_numpy(w.astype(np.float32)))
    layer.bias.data.copy_(torch.from_numpy(g.uniform(-1, 1, size=(Cout,)).astype(np.float32)))
    return layer.to(dev)


LAYER_KINDS = ("bin", "ter", "bin_stochastic", "ter_stochastic", "k1", "k4", "k32")


@functools.lru_cache(maxsize=None)
def _layer_reference(kind, cout_g):
    """The float64 module on the CPU — F.conv2d(x, Q(W), b, groups = 4) with the quantiser's own backward — and its training
    step, computed once per (kind, cout_g) and shared by both layouts."""
    ref = copy.deepcopy(_make(kind, cout_g, "cpu")).double()
    x = R.gauss6(5, (3, G * CIN_G, 9, 7))
    Ho, Wo = R.out_hw(9, 7, 3, 2, 1, 1)
    go = R.gauss6(6, (3, G * cout_g, Ho, Wo)) * 1e-2
    xr = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    yr = ref(xr)
    yr.backward(torch.from_numpy(go.astype(np.float64)))
    return x, go, yr.detach(), xr.grad, ref.weight.grad, ref.bias.grad


@pytest.mark.parametrize("layout", ("nchw", "channels_last"))
@pytest.mark.parametrize("cout_g", (3, 6))
@pytest.mark.parametrize("kind", LAYER_KINDS)
def test_layers_train_step_and_eval_on_the_grouped_route(dev, kind, cout_g, layout):
    layer = _make(kind, cout_g, dev)
    x, go, yr, gxr, gwr, gbr = _layer_reference(kind, cout_g)
    assert _fused.grouped_route(layer, _to(dev, x, layout)) and not _fused.depthwise_route(layer, _to(dev, x, layout))
    xd = _to(dev, x, layout).requires_grad_(True)
    calls, reasons = dict(_lib.call_counts), dict(_fused.LIBRARY_PATHS)
    y = layer(xd)
    y.backward(_to(dev, go, layout))
    torch.cuda.synchronize()
    used = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
    assert (used.get(FWD), used.get(GIN), used.get(GWT)) == (1, 1, 1), used
    assert not [k for k in used if k.startswith("qt_conv2d_implicit") or k.startswith("qt_dwconv2d")], used
    assert dict(_fused.LIBRARY_PATHS) == reasons
    assert y.is_contiguous(memory_format=torch.channels_last) == (layout == "channels_last")
    errs = dict(y=nerr(y.detach().cpu(), yr), gx=nerr(xd.grad.cpu(), gxr), gw=nerr(layer.weight.grad.cpu(), gwr),
                gb=nerr(layer.bias.grad.cpu(), gbr))
    print(kind, cout_g, layout, errs)
    assert max(errs.values()) <= TOL, errs
    if not kind.startswith("k"):
        masked = layer.weight.detach().abs() > 1.001
        assert masked.any() and (layer.weight.grad[masked] == 0).all()
    # eval: the stored image, the same launch, the same bits — without autograd and with it
    layer.eval()
    calls = dict(_lib.call_counts)
    with torch.no_grad():
        ye = layer(_to(dev, x, layout))
    assert isinstance(ye, torch.Tensor) and ye.dtype == torch.float32 and torch.equal(ye, y.detach())
    xe = _to(dev, x, layout).requires_grad_(True)
    ya = layer(xe)
    assert torch.equal(ya.detach(), y.detach())
    ya.backward(_to(dev, go, layout))
    assert nerr(xe.grad.cpu(), gxr) <= TOL
    used = {k: v - calls.get(k, 0) for k, v in _lib.call_counts.items() if v != calls.get(k, 0)}
    assert used.get(FWD) == 2 and used.get(GIN) == 1 and not [k for k in used if k.startswith("qt_conv2d_implicit")], used
    assert dict(_fused.LIBRARY_PATHS) == reasons


@pytest.mark.parametrize("kind", ("binary", "ternary"))
def test_pm1_data_equals_the_per_group_loop(dev, kind):
    C, Cout = G * CIN_G, G * 6
    layer = (BinConv2d if kind == "binary" else TerConv2d)(C, Cout, 3, padding=1, groups=G).to(dev)
    layer.weight.data.copy_(_to(dev, R.weights(9, (Cout, CIN_G, 3, 3))))
    x = _to(dev, R.pm1(10, (2, C, 8, 8)))
    calls = dict(_lib.call_counts)
    with torch.no_grad():
        y = layer(x)
        assert _lib.call_counts[FWD] - calls.get(FWD, 0) == 1
        old = _fused.grouped_quant_conv(layer, x, kind, layer._op)          # integer sums: exact in any order
    assert old is not None and torch.equal(y, old)


def test_two_or_three_groups_and_32_channels_per_group_stay_off_the_grouped_route(dev):
    calls = dict(_lib.call_counts)
    for groups, cin_g in ((2, 3), (3, 3), (4, 32), (4, _fused.GROUPED_MAX_CIN_G + 1)):
        C = groups * cin_g
        x = _to(dev, R.pm1(11, (2, C, 8, 8))).requires_grad_(True)
        for layer in (BinConv2d(C, C, 3, padding=1, groups=groups), TerConv2d(C, 2 * C, 3, padding=1, groups=groups),
                      DorefaConv2d(C, C, 3, padding=1, groups=groups, bit_width=4)):
            layer = layer.to(dev)
            assert not _fused.grouped_route(layer, x)
            y = layer(x)
            y.sum().backward()
            want = torch.nn.functional.conv2d(x.detach().cpu().double(), _quantised(layer).cpu().double(), layer.bias.detach().cpu().double(),
                                              1, 1, 1, groups)
            assert nerr(y.detach().cpu(), want) <= TOL
    assert not [k for k in _lib.call_counts if k.startswith("qt_gconv2d") and _lib.call_counts[k] != calls.get(k, 0)]
    # an off-grid eval weight of a grouped layer keeps the library expression and its reason
    layer = BinConv2d(12, 12, 3, padding=1, groups=4).to(dev).eval()
    layer.weight.data.copy_(_to(dev, R.weights(12, (12, 3, 3, 3))))
    layer.reset_quant_cache()
    x = _to(dev, R.pm1(13, (2, 12, 8, 8)))
    reasons = dict(_fused.LIBRARY_PATHS)
    with torch.no_grad():
        y = layer(x)
    assert _lib.call_counts[FWD] == calls.get(FWD, 0)
    assert sum(_fused.LIBRARY_PATHS.values()) == sum(reasons.values()) + 1
    assert _fused.LIBRARY_PATHS["eval-mode weight off the quantiser's grid"] == reasons.get("eval-mode weight off the quantiser's grid", 0) + 1
    assert nerr(y.cpu(), torch.nn.functional.conv2d(x.cpu(), layer.weight.detach().cpu(), layer.bias.detach().cpu(), 1, 1, 1, 4)) <= TOL


def _quantised(layer):
    w = layer.weight.detach()
    if isinstance(layer, DorefaConv2d):
        return layer.weight_op.forward(w).detach()
    return torch.from_numpy(R.quantize(w.cpu().numpy(), layer.kind)).to(w.device)


def test_forward_and_backward_replay_from_a_captured_graph(dev):
    layer = _make("ter", 6, dev)
    C, Cout = G * CIN_G, G * 6
    xs = _to(dev, R.gauss6(20, (2, C, 9, 7))).requires_grad_(True)
    gs = _to(dev, R.gauss6(21, (2, Cout, 5, 4)))

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
    x2, g2 = _to(dev, R.gauss6(22, (2, C, 9, 7))), _to(dev, R.gauss6(23, (2, Cout, 5, 4)))
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
    assert _lib.call_counts[FWD] == calls.get(FWD, 0) + 1
    for a, b in zip(got, (ye.detach(), xe.grad, twin.weight.grad, twin.bias.grad)):
        assert torch.equal(a, b)
