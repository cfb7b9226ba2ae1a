"""tests/_xnor_exact.py (the float64 reference of the XNOR-Net tap convs) pinned against torch's own float64 convolutions and
autograd at tiny shapes, and the exactness proofs of every designed operand of tests/test_gpu_xnor_b256.py — the arithmetic
condition at that module's shapes, no large tensors — so that the bit-equality claims hold before a GPU is involved."""
import pytest
import torch
import torch.nn.functional as F

import _grad_exact as G
import _xnor_exact as XE

F64 = torch.float64
CPU = torch.device("cpu")

# N, Cin, Cout, H, W, k, stride, padding, dilation
GEOMS = [
    (2, 3, 4, 6, 7, 3, 1, 0, 1),
    (2, 5, 3, 6, 5, 3, 1, 1, 1),
    (1, 4, 6, 9, 8, 3, 2, 1, 1),
    (2, 3, 2, 9, 9, 3, 1, 2, 2),
    (1, 6, 5, 7, 7, 5, 1, 2, 1),
    (2, 4, 4, 5, 6, 1, 1, 0, 1),
    (1, 3, 4, 7, 6, 3, 1, (2, 1), 1),
    (1, 2, 3, 8, 8, 3, (2, 1), (0, 1), (1, 2)),
]


def _weight(Cout, Cin, k, seed, zero_tap=True, lone_zero=True):
    w = torch.randn((Cout, Cin, k, k), generator=torch.Generator().manual_seed(seed), dtype=F64)
    if zero_tap and k > 1:
        w[:, :, k // 2, k // 2] = 0.0                     # an all-zero tap: alpha_t = 0
    if lone_zero:
        w[0, 0, 0, 0] = 0.0                               # torch.sign semantics: the weight image holds 0 there
    return w


@pytest.mark.parametrize("geom", GEOMS, ids=[str(g) for g in GEOMS])
def test_tap_sums_and_xnor_conv_equal_torch_conv2d(geom):
    N, Cin, Cout, H, W, k, s, p, d = geom
    x = G.pm1((N, Cin, H, W), 3, CPU, zero_frac=0.1, channels_last=False).to(F64)
    w = _weight(Cout, Cin, k, 4)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(5), dtype=F64)
    alpha = w.abs().mean(dim=(0, 1), keepdim=True)
    assert torch.equal(XE.tap_alpha64(w), alpha.reshape(-1))
    if k > 1:
        assert float(alpha[0, 0, k // 2, k // 2]) == 0.0
    want = F.conv2d(x, torch.sign(w) * alpha, bias, s, p, d)
    y, B = XE.xnor_conv64(x, w, bias, s, p, d)
    assert y.shape == want.shape
    assert torch.allclose(y, want, rtol=0, atol=1e-12 * float(want.abs().max()))
    wantB = F.conv2d(x.abs(), torch.sign(w).abs() * alpha, None, s, p, d) + bias.abs().view(1, -1, 1, 1)
    assert torch.allclose(B, wantB, rtol=0, atol=1e-12 * float(wantB.abs().max()))
    assert bool((y.abs() <= B * (1 + 1e-12)).all())
    # the per-tap contractions themselves: exact integers, one conv per tap
    D = XE.tap_sums64(x, torch.sign(w), s, p, d)
    assert D.shape == (N, k * k, Cout) + tuple(want.shape[2:])
    assert torch.equal(D, D.round())
    for t in range(k * k):
        wt = torch.zeros_like(w)
        wt[:, :, t // k, t % k] = torch.sign(w)[:, :, t // k, t % k]
        assert torch.equal(D[:, t], F.conv2d(x, wt, None, s, p, d).round())
    # a tiny byte budget (one image per chunk) changes nothing
    assert torch.equal(XE.xnor_conv64(x, w, bias, s, p, d, budget=1)[0], y)


@pytest.mark.parametrize("geom", GEOMS, ids=[str(g) for g in GEOMS])
def test_xnor_rows_equal_the_conv_of_the_quantised_image(geom):
    N, Cin, Cout, H, W, k, s, p, d = geom
    xr = torch.randn((N, Cin, H, W), generator=torch.Generator().manual_seed(6), dtype=F64)
    xr[:, :, 0, :] = 0.0                                   # all-zero pixels: a whole row, and a lone one
    xr[:, :, H // 2, W // 2] = 0.0
    A = xr.abs().mean(1)
    w = _weight(Cout, Cin, k, 7)
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(8), dtype=F64)
    alpha = w.abs().mean(dim=(0, 1), keepdim=True)
    want = F.conv2d(torch.sign(xr) * A.unsqueeze(1), torch.sign(w) * alpha, bias, s, p, d)
    y, B = XE.xnor_rows64(torch.sign(xr), A, w, bias, s, p, d)
    assert torch.allclose(y, want, rtol=0, atol=1e-12 * float(want.abs().max()))
    assert bool((y.abs() <= B * (1 + 1e-12)).all())
    assert torch.equal(XE.xnor_rows64(torch.sign(xr), A, w, bias, s, p, d, budget=1)[0], y)


@pytest.mark.parametrize("geom", [g for g in GEOMS if g[8] == 1 and isinstance(g[6], int)], ids=str)
def test_xnor_grad_input_equals_torch_and_autograd(geom):
    N, Cin, Cout, H, W, k, s, p, _ = geom
    w = _weight(Cout, Cin, k, 9)
    alpha = w.abs().mean(dim=(0, 1), keepdim=True)
    wq = torch.sign(w) * alpha
    x = torch.randn((N, Cin, H, W), generator=torch.Generator().manual_seed(10), dtype=F64, requires_grad=True)
    y = F.conv2d(x, wq, None, s, p)
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(11), dtype=F64)
    gx, B = XE.xnor_grad_input64(g, w, (H, W), s, p)
    want = torch.nn.grad.conv2d_input(x.shape, wq, g, s, p)
    assert torch.allclose(gx, want, rtol=0, atol=1e-12 * float(want.abs().max()))
    y.backward(g)
    assert torch.allclose(gx, x.grad, rtol=0, atol=1e-12 * float(want.abs().max()))
    assert bool((gx.abs() <= B * (1 + 1e-12)).all())


# ---- designed operands --------------------------------------------------------------------------------------------------------

def test_ramp_exponents_are_non_monotone_and_span_the_range():
    for T in (1, 2, 3, 4, 9, 25, 49):
        for span in (1, 5, 14):
            e = XE.ramp_exps(T, span)
            assert len(e) == T and min(e) == 0
            if T > 1:
                assert max(e) == span
            if T >= 3 and span > 1:
                top = e.index(max(e))
                assert 0 < top < T - 1 and e[-1] < max(e), e          # up, then down


def test_pow2_tap_weight_has_power_of_two_alphas():
    exps = XE.ramp_exps(9, 12)
    w = XE.pow2_tap_weight((8, 6, 3, 3), exps, 1, CPU, zero_taps=(4,))
    assert torch.equal(XE.tap_alpha64(w), XE.designed_alpha(exps, (4,)))
    assert set(torch.sign(w).unique().tolist()) == {-1.0, 0.0, 1.0}
    w = XE.pow2_tap_weight((8, 6, 3, 3), exps, 1, CPU, lone_zero=(4, 2, 4))
    assert float(w[4, 2, 1, 1]) == 0.0 and int((w == 0).sum()) == 1
    # the lone zero makes mean|w| of its tap a non-power of two: such cases hand the designed alphas to the kernels
    with pytest.raises(AssertionError):
        XE.proves_exact_taps(XE.tap_alpha64(w), 6)


def test_proves_exact_taps_accepts_and_rejects():
    a = XE.designed_alpha([0, 3, 6, 2])
    assert XE.proves_exact_taps(a, 64)[0]                                # (1 + 8 + 64 + 4) * 64 quanta
    assert not XE.proves_exact_taps(XE.designed_alpha([0, 19]), 64)[0]   # 2^19 * 64 = 2^25 quanta
    assert XE.proves_exact_taps(XE.designed_alpha([0, 17]), 64)[0]
    # an intermediate S_t can fail where the order matters: the reversed table is checked in its own order
    assert XE.proves_exact_taps(XE.designed_alpha([0, 17]), 64, reverse=True)[0]
    # a bias with a finer quantum than the smallest tap counts
    assert not XE.proves_exact_taps(XE.designed_alpha([0, 17]), 64, bias=torch.tensor([2.0 ** -2]))[0]
    assert XE.proves_exact_taps(XE.designed_alpha([0, 17]), 64, bias=torch.tensor([3.0, -8.0]))[0]
    # zero taps do not count; an all-zero table is trivially exact
    assert XE.proves_exact_taps(XE.designed_alpha([0, 30, 17], zero_taps=(1,)), 64)[0]
    assert XE.proves_exact_taps(torch.zeros(4), 64)[0]
    # a wider operand (the A plane, a gradient) costs its own bits
    assert not XE.proves_exact_taps(XE.designed_alpha([0, 17]), 64, x_absmax=4.0, x_quantum=-2)[0]
    # the fp32 range
    assert not XE.proves_exact_taps(XE.designed_alpha([-130, -128]), 4)[0]
    # grad_x: the gradient must survive the two-term fp16 split
    g = G.grad_ints((2, 8, 3, 3), XE.GRAD_AMP, 1, CPU, exp=-40)
    assert XE.proves_exact_taps(XE.designed_alpha([0, 5, 2]), 8, grad=g, reverse=True)[0]
    bad = g.clone()
    bad[0, 0, 0, 0] = 2.0 ** -40 * (4 + 2.0 ** -10 + 2.0 ** -21)            # bits 2^2 and 2^-21 apart: more than two fp16 terms hold
    assert not XE.proves_exact_taps(XE.designed_alpha([0, 5, 2]), 8, grad=bad, reverse=True)[0]


def test_max_span_is_the_widest_proved_span():
    for T, count in ((9, 64), (9, 576), (25, 192), (9, 1152), (1, 64)):
        s = XE.max_span(T, count, 1.0, XE.BIAS_QUANTA)
        b = torch.tensor([float(XE.BIAS_QUANTA)], dtype=F64)
        assert XE.proves_exact_taps(XE.designed_alpha(XE.ramp_exps(T, s)), count, b)[0]
        if T > 1:
            assert not XE.proves_exact_taps(XE.designed_alpha(XE.ramp_exps(T, s + 1)), count, b)[0]
    assert XE.max_span(9, 64, 1.0, XE.BIAS_QUANTA) >= 14             # Cin = 64, nine taps: about 14 binades


@pytest.mark.parametrize("case", XE.FWD_CASES, ids=[c[0] for c in XE.FWD_CASES])
def test_forward_designs_are_provably_exact(case):
    name, B, Cin, Cout, H, k, s, p, d, variant, _, _ = case
    exps, zero_taps, lone = XE.tap_design(k * k, Cin, variant, Cout=Cout)
    alpha = XE.designed_alpha(exps, zero_taps)
    bias = XE.exact_bias(Cout, exps, XE.case_seed(name), CPU)
    ok, why = XE.proves_exact_taps(alpha, Cin, bias)
    assert ok, (name, why)
    assert max(exps) - min(exps) >= (1 if k > 1 else 0)
    if lone is not None:
        assert lone[0] < Cout and lone[1] < Cin and lone[2] < k * k


@pytest.mark.parametrize("case", XE.ROWS_CASES, ids=[c[0] for c in XE.ROWS_CASES])
def test_row_scaled_designs_are_provably_exact(case):
    name, B, Cin, Cout, H, k, s, p = case
    lo, hi = XE.A_EXPS
    exps, zero_taps, _ = XE.tap_design(k * k, Cin, "mid", x_absmax=2.0 ** (hi - lo), Cout=Cout)
    A = XE.pow2_plane((2, 5, 5), lo, hi, 0.2, XE.case_seed(name), CPU)
    assert float(A.max()) == 2.0 ** hi and G.quantum_exp(A) == lo and bool((A == 0).any())
    bias = XE.exact_bias(Cout, [e + lo for e in exps], XE.case_seed(name), CPU)
    ok, why = XE.proves_exact_taps(XE.designed_alpha(exps, zero_taps), Cin, bias, x_absmax=2.0 ** hi, x_quantum=lo)
    assert ok, (name, why)


@pytest.mark.parametrize("exp", XE.GRAD_EXPS)
@pytest.mark.parametrize("case", XE.GRAD_CASES, ids=[c[0] for c in XE.GRAD_CASES])
def test_gradient_designs_are_provably_exact(case, exp):
    name, B, Cin, Cout, H, k, s, p, _ = case
    exps, zero_taps, _ = XE.tap_design(k * k, Cout, "mid", x_absmax=float(XE.GRAD_AMP), bias_quanta=0, Cout=Cout)
    g = G.grad_ints((2, 8, 3, 3), XE.GRAD_AMP, XE.case_seed(name), CPU, exp=exp)
    assert float(g.abs().max()) == XE.GRAD_AMP * 2.0 ** exp
    ok, why = XE.proves_exact_taps(XE.designed_alpha(exps, zero_taps), Cout, grad=g, reverse=True)
    assert ok, (name, exp, why)
