"""Pins tests/_gconv_exact.py, the reference of the grouped-conv GPU tests, on the CPU: its float64 side against torch's own
grouped conv and autograd, its ordered float32 side against tests/_dw_exact.py at one channel per group (bit for bit) and against
float64 (exactly on integer operands, within the summation bound on Gaussian data), and the case grid."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _dw_exact as D
import _gconv_exact as R

CASES = [
    dict(N=2, G=4, cin_g=3, cout_g=2, H=7, W=7, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1)),
    dict(N=1, G=2, cin_g=5, cout_g=3, H=9, W=14, kernel=(3, 5), stride=(2, 1), padding=(2, 0), dilation=(1, 1)),
    dict(N=3, G=5, cin_g=2, cout_g=4, H=11, W=8, kernel=(3, 3), stride=(2, 2), padding=(3, 3), dilation=(2, 2)),
    dict(N=1, G=1, cin_g=4, cout_g=1, H=8, W=8, kernel=(7, 7), stride=(1, 1), padding=(3, 3), dilation=(1, 2)),
    dict(N=2, G=3, cin_g=16, cout_g=17, H=1, W=1, kernel=(1, 1), stride=(2, 2), padding=(0, 0), dilation=(1, 1)),
    dict(N=1, G=2, cin_g=32, cout_g=2, H=6, W=5, kernel=(4, 4), stride=(1, 1), padding=(1, 1), dilation=(1, 1)),
]
IDS = [f"c{i}" for i in range(len(CASES))]


def _geom(c):
    return c["kernel"], c["stride"], c["padding"], c["dilation"]


def _shapes(c):
    Ho, Wo = R.out_hw(c["H"], c["W"], *_geom(c))
    return ((c["N"], c["G"] * c["cin_g"], c["H"], c["W"]), (c["G"] * c["cout_g"], c["cin_g"]) + c["kernel"],
            (c["N"], c["G"] * c["cout_g"], Ho, Wo))


def _torch64(x, wq, b, go, c):
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    wt = torch.from_numpy(wq.astype(np.float64)).requires_grad_(True)
    bt = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
    y = F.conv2d(xt, wt, bt, c["stride"], c["padding"], c["dilation"], groups=c["G"])
    y.backward(torch.from_numpy(go.astype(np.float64)))
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("c", CASES, ids=IDS)
@pytest.mark.parametrize("kind", R.KINDS)
def test_float64_side_equals_torch_grouped_conv_and_autograd(c, kind):
    xs, ws, ys = _shapes(c)
    x, w, b, go = R.gauss6(1, xs), R.weights(2, ws), R.small_ints(3, (ws[0],)), R.gauss6(4, ys)
    wq = R.quantize(w, kind)
    y, gx, gw, gb = _torch64(x, wq, b, go, c)
    mine = R.forward(x, wq, b, c["G"], *_geom(c), dtype=np.float64)
    assert mine.shape == y.shape and np.abs(mine - y).max() <= 1e-12 * max(np.abs(y).max(), 1e-300)
    mine_gx = R.grad_input(go, wq, xs, c["G"], *_geom(c), dtype=np.float64)
    assert mine_gx.shape == gx.shape and np.abs(mine_gx - gx).max() <= 1e-12 * max(np.abs(gx).max(), 1e-300)
    mine_gw, ab, mine_gb = R.grad_weight(x, go, c["G"], c["cin_g"], *_geom(c))
    assert mine_gw.shape == gw.shape and np.abs(mine_gw - gw).max() <= 1e-12 * max(ab.max(), 1e-300)
    assert np.abs(mine_gb - gb).max() <= 1e-12 * max(np.abs(go).sum(), 1e-300)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("m", (1, 3))
def test_one_channel_per_group_equals_the_depthwise_reference_bit_for_bit(kind, m):
    C, geom = 5, ((3, 3), (2, 1), (1, 1), (1, 2))
    xs = (2, C, 9, 8)
    Ho, Wo = R.out_hw(9, 8, *geom)
    x, go = R.gauss6(1, xs), R.gauss6(2, (2, C * m, Ho, Wo))
    w, b = R.weights(3, (C * m, 1, 3, 3)), R.gauss6(4, (C * m,))
    wq = R.quantize(w, kind)
    assert np.array_equal(R.forward(x, wq, b, C, *geom), D.forward(x, wq[:, 0], b, *geom))
    assert np.array_equal(R.grad_input(go, wq, xs, C, *geom), D.grad_input(go, wq[:, 0], xs, *geom))
    gw, ab, gb = R.grad_weight(x, go, C, 1, *geom)
    dgw, dab, dgb = D.grad_weight(x, go, *geom)
    assert np.array_equal(gw[:, 0], dgw) and np.array_equal(ab[:, 0], dab) and np.array_equal(gb, dgb)


@pytest.mark.parametrize("c", CASES, ids=IDS)
@pytest.mark.parametrize("kind", ("binary", "ternary"))
def test_integer_operands_float32_equals_float64_exactly(c, kind):
    xs, ws, ys = _shapes(c)
    x, go, b = R.pm1(5, xs), R.small_ints(6, ys), R.small_ints(7, (ws[0],))
    wq = R.quantize(R.weights(8, ws), kind)
    assert set(np.unique(wq)) <= {-1.0, 0.0, 1.0}
    y32, y64 = R.forward(x, wq, b, c["G"], *_geom(c)), R.forward(x, wq, b, c["G"], *_geom(c), dtype=np.float64)
    assert y32.dtype == np.float32 and np.array_equal(y32.astype(np.float64), y64)
    g32, g64 = R.grad_input(go, wq, xs, c["G"], *_geom(c)), R.grad_input(go, wq, xs, c["G"], *_geom(c), dtype=np.float64)
    assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), g64)
    gw, _ab, _gb = R.grad_weight(x, go, c["G"], c["cin_g"], *_geom(c))
    assert np.array_equal(gw, np.rint(gw)) and np.abs(gw).max() < 2 ** 24        # exact in float32 in any order


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gaussian_ordered_float32_is_within_the_bound_of_float64(c):
    xs, ws, ys = _shapes(c)
    x, w, go = R.gauss6(9, xs), R.weights(10, ws), R.gauss6(11, ys)
    taps = c["kernel"][0] * c["kernel"][1]
    for kind in R.KINDS:
        wq = R.quantize(w, kind)
        y32 = R.forward(x, wq, None, c["G"], *_geom(c)).astype(np.float64)
        y64 = R.forward(x, wq, None, c["G"], *_geom(c), dtype=np.float64)
        yab = R.forward(np.abs(x), np.abs(wq), None, c["G"], *_geom(c), dtype=np.float64)
        assert (np.abs(y32 - y64) <= R.grad_weight_bound(yab, taps * c["cin_g"])).all()
        g32 = R.grad_input(go, wq, xs, c["G"], *_geom(c)).astype(np.float64)
        g64 = R.grad_input(go, wq, xs, c["G"], *_geom(c), dtype=np.float64)
        gab = R.grad_input(np.abs(go), np.abs(wq), xs, c["G"], *_geom(c), dtype=np.float64)
        assert (np.abs(g32 - g64) <= R.grad_weight_bound(gab, taps * c["cout_g"])).all()


def test_case_grid_covers_every_feasible_pair_and_is_stable():
    cs = R.cases()
    assert 60 <= len(cs) <= 200
    assert R.all_pairs_covered(cs)
    assert [c.id for c in cs] == [c.id for c in R.cases()] and len({c.id for c in cs}) == len(cs)
    for c in cs:
        Ho, Wo = R.out_hw(c.H, c.W, *c.geom)
        taps = c.kernel[0] * c.kernel[1]
        assert Ho >= 1 and Wo >= 1 and taps <= R.MAX_TAPS and c.cin_g <= R.MAX_CIN_G and c.cin_g * taps <= R.MAX_K
    for name, values in (("cin_g", R.CIN_G), ("cout_g", R.COUT_G), ("G", R.GROUPS), ("N", R.BATCHES), ("kernel", R.KERNELS),
                         ("stride", R.STRIDES), ("padding", R.PADDINGS), ("dilation", R.DILATIONS), ("layout", R.LAYOUTS)):
        assert {c[name] for c in cs} >= set(values), name
    assert {(c.H, c.W) for c in cs} >= set(R.MAPS)
    assert sum(c.cin_g * c.kernel[0] * c.kernel[1] == R.MAX_K for c in cs) == 2
    assert any(c.kernel == (7, 7) and c.cin_g == 5 for c in cs)
    for c in cs:
        w = R.weights(c.cin_g * 131 + c.cout_g, c.shapes[1])
        assert R.tie_share(w) == 0.0
