"""Pins tests/_dw_exact.py, the reference of the depthwise GPU tests, on the CPU: its float64 side against torch's own grouped
conv and autograd, its ordered float32 side against float64 (exactly on integer operands, within the summation bound on Gaussian
data), and the generated weights against accidental ties at the quantisers' decision points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _dw_exact as D

CASES = [
    dict(N=2, C=3, m=1, H=7, W=7, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1)),
    dict(N=1, C=4, m=2, H=9, W=14, kernel=(3, 5), stride=(2, 1), padding=(2, 0), dilation=(1, 1)),
    dict(N=3, C=2, m=3, H=11, W=8, kernel=(3, 3), stride=(2, 2), padding=(3, 3), dilation=(2, 2)),
    dict(N=1, C=5, m=1, H=8, W=8, kernel=(7, 7), stride=(1, 1), padding=(3, 3), dilation=(1, 1)),
    dict(N=2, C=1, m=2, H=1, W=1, kernel=(1, 1), stride=(2, 2), padding=(0, 0), dilation=(1, 1)),
    dict(N=1, C=3, m=1, H=13, W=6, kernel=(5, 5), stride=(1, 1), padding=(1, 1), dilation=(1, 1)),
]
IDS = [f"c{i}" for i in range(len(CASES))]


def _geom(c):
    return c["kernel"], c["stride"], c["padding"], c["dilation"]


def _shapes(c):
    Ho, Wo = D.out_hw(c["H"], c["W"], *_geom(c))
    return (c["N"], c["C"], c["H"], c["W"]), (c["C"] * c["m"],) + c["kernel"], (c["N"], c["C"] * c["m"], Ho, Wo)


def _torch64(x, wq, b, go, c):
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    wt = torch.from_numpy(wq.astype(np.float64)).unsqueeze(1).requires_grad_(True)
    bt = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
    y = F.conv2d(xt, wt, bt, c["stride"], c["padding"], c["dilation"], groups=c["C"])
    y.backward(torch.from_numpy(go.astype(np.float64)))
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.squeeze(1).numpy(), bt.grad.numpy()


@pytest.mark.parametrize("c", CASES, ids=IDS)
@pytest.mark.parametrize("kind", D.KINDS)
def test_float64_side_equals_torch_grouped_conv_and_autograd(c, kind):
    xs, ws, ys = _shapes(c)
    x, w, b, go = D.gauss6(1, xs), D.weights(2, ws), D.small_ints(3, (ws[0],)), D.gauss6(4, ys)
    wq = D.quantize(w, kind)
    y, gx, gw, gb = _torch64(x, wq, b, go, c)
    mine = D.forward(x, wq, b, *_geom(c), dtype=np.float64)
    scale = max(np.abs(y).max(), 1e-300)
    assert mine.shape == y.shape and np.abs(mine - y).max() <= 1e-12 * scale
    mine_gx = D.grad_input(go, wq, xs, *_geom(c), dtype=np.float64)
    assert np.abs(mine_gx - gx).max() <= 1e-12 * max(np.abs(gx).max(), 1e-300)
    mine_gw, ab, mine_gb = D.grad_weight(x, go, *_geom(c))
    assert np.abs(mine_gw - gw).max() <= 1e-12 * max(ab.max(), 1e-300)
    assert np.abs(mine_gb - gb).max() <= 1e-12 * max(np.abs(go).sum(), 1e-300)


@pytest.mark.parametrize("c", CASES, ids=IDS)
@pytest.mark.parametrize("kind", ("binary", "ternary"))
def test_integer_operands_float32_equals_float64_exactly(c, kind):
    xs, ws, ys = _shapes(c)
    x, go, b = D.pm1(5, xs), D.small_ints(6, ys), D.small_ints(7, (ws[0],))
    wq = D.quantize(D.weights(8, ws), kind)
    assert set(np.unique(wq)) <= {-1.0, 0.0, 1.0}
    y32, y64 = D.forward(x, wq, b, *_geom(c)), D.forward(x, wq, b, *_geom(c), dtype=np.float64)
    assert y32.dtype == np.float32 and np.array_equal(y32.astype(np.float64), y64)
    g32, g64 = D.grad_input(go, wq, xs, *_geom(c)), D.grad_input(go, wq, xs, *_geom(c), dtype=np.float64)
    assert g32.dtype == np.float32 and np.array_equal(g32.astype(np.float64), g64)
    gw, ab, gb = D.grad_weight(x, go, *_geom(c))
    assert np.array_equal(gw, np.rint(gw)) and np.abs(gw).max() < 2 ** 24        # exact in float32 in any order


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gaussian_ordered_float32_is_within_the_bound_of_float64(c):
    xs, ws, ys = _shapes(c)
    x, w, go = D.gauss6(9, xs), D.weights(10, ws), D.gauss6(11, ys)
    for kind in D.KINDS:
        wq = D.quantize(w, kind)
        taps = c["kernel"][0] * c["kernel"][1]
        y32 = D.forward(x, wq, None, *_geom(c)).astype(np.float64)
        y64 = D.forward(x, wq, None, *_geom(c), dtype=np.float64)
        yab = D.forward(np.abs(x), np.abs(wq), None, *_geom(c), dtype=np.float64)
        assert (np.abs(y32 - y64) <= D.grad_weight_bound(yab, taps)).all()
        g32 = D.grad_input(go, wq, xs, *_geom(c)).astype(np.float64)
        g64 = D.grad_input(go, wq, xs, *_geom(c), dtype=np.float64)
        gab = D.grad_input(np.abs(go), np.abs(wq), xs, *_geom(c), dtype=np.float64)
        assert (np.abs(g32 - g64) <= D.grad_weight_bound(gab, taps * c["m"])).all()


def test_quantisers_at_their_decision_points():
    w = np.array([-0.0, 0.0, np.nan, 1e-45, -1e-45, 0.5, -0.5, np.nextafter(np.float32(0.5), np.float32(0)),
                  np.nextafter(np.float32(-0.5), np.float32(-1)), 2.0, -2.0], dtype=np.float32)
    assert D.quantize(w, "binary").tolist() == [1, 1, 1, 1, -1, 1, -1, 1, -1, 1, -1]
    assert D.quantize(w, "ternary").tolist() == [0, 0, 1, 0, 0, 1, 0, 0, -1, 1, -1]
    assert np.array_equal(D.quantize(w, "raw"), w, equal_nan=True)
    above = np.nextafter(D.STE, np.float32(2))
    wm = np.array([D.STE, -D.STE, above, -above, np.nan], dtype=np.float32)
    assert D.ste_mask(np.ones(5), wm).tolist() == [1, 1, 0, 0, 1]
    assert D.ste_mask(np.ones(5), wm, 0.0).tolist() == [1] * 5


def test_generated_weights_hold_no_accidental_ties():
    """No generated weight sits exactly on +-0.5 or +-1.001 (a case that wants such a value writes it in on purpose), and every
    decision region is populated."""
    for case in D.cases():
        w = D.weights(case.C * 131 + case.m, (case.C * case.m,) + case.kernel)
        assert D.tie_share(w) == 0.0
    w = D.weights(1, (64, 7, 7))
    assert D.tie_share(w) == 0.0
    a = np.abs(w)
    assert (a < 0.5).any() and ((a > 0.5) & (a < 1.001)).any() and (a > 1.001).any() and (w < 0).any() and (w > 0).any()
    assert D.tie_share(np.array([0.5, 1.0, -1.001, 0.25], dtype=np.float32)) == 0.5


def test_case_grid_covers_every_feasible_pair_and_is_stable():
    cs = D.cases()
    assert 80 <= len(cs) <= 120
    assert D.all_pairs_covered(cs)
    assert [c.id for c in cs] == [c.id for c in D.cases()]
    for c in cs:
        Ho, Wo = D.out_hw(c.H, c.W, c.kernel, c.stride, c.padding, c.dilation)
        assert Ho >= 1 and Wo >= 1 and c.kernel[0] * c.kernel[1] <= 49
    assert any(c.padding == (3, 3) and c.kernel == (3, 3) for c in cs)
