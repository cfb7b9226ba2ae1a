"""The float64 backward references and the exactness proof of tests/_grad_exact.py, on the host: the references against
torch.nn.grad in float64 at the geometries the GPU tests use, and the proof on cases that hold and cases that must not."""
import pytest
import torch

import _grad_exact as G

F64 = torch.float64


@pytest.mark.parametrize("N,Cin,Cout,H,W,k,s,p", [
    (2, 3, 4, 7, 7, 3, 1, 1),        # 3x3, padding
    (3, 4, 5, 9, 9, 3, 2, 1),        # stride 2 on an odd map
    (2, 5, 3, 9, 8, 1, 2, 0),        # 1x1 stride 2 (odd map: the last row / column is never read)
    (2, 3, 4, 8, 8, 5, 1, 2),        # 5x5
    (2, 3, 6, 31, 31, 11, 4, 2),     # 11x11 stride 4, padding 2 (AlexNet conv1)
])
def test_conv_references_match_torch_nn_grad_float64(N, Cin, Cout, H, W, k, s, p):
    gen = torch.Generator().manual_seed(N * 1000 + H * 10 + k)
    x = torch.randn((N, Cin, H, W), generator=gen, dtype=F64)
    w = torch.randn((Cout, Cin, k, k), generator=gen, dtype=F64)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.randn((N, Cout, Ho, Wo), generator=gen, dtype=F64)
    gx = G.conv_grad_input64(g, w, (H, W), s, p, budget=1 << 12)          # tiny budget: one image per chunk
    gw = G.conv_grad_weight64(x, g, (k, k), s, p, budget=1 << 12)
    assert torch.allclose(gx, torch.nn.grad.conv2d_input(x.shape, w, g, stride=s, padding=p), rtol=1e-12, atol=1e-12)
    assert torch.allclose(gw, torch.nn.grad.conv2d_weight(x, w.shape, g, stride=s, padding=p), rtol=1e-12, atol=1e-12)
    assert torch.allclose(G.bias_grad64(g), g.sum((0, 2, 3)), rtol=1e-12, atol=1e-12)
    parts = G.conv_grad_weight64(x, g, (k, k), s, p, chunks=[1] * (N - 1) + [1])
    assert len(parts) == N and torch.allclose(sum(parts), gw, rtol=1e-12, atol=1e-12)


def test_linear_references():
    gen = torch.Generator().manual_seed(3)
    x, w, g = (torch.randn(s, generator=gen, dtype=F64) for s in ((5, 21), (13, 21), (5, 13)))
    xr = x.clone().requires_grad_()
    wr = w.clone().requires_grad_()
    (xr @ wr.t()).backward(g)
    assert torch.allclose(G.linear_grad_x64(g, w), xr.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(G.linear_grad_w64(g, x), wr.grad, rtol=1e-12, atol=1e-12)


def test_ste_mask_is_the_reduce_kernels_predicate():
    w = torch.tensor([0.0, -1.0, 1.001, -1.002, 1.5, float("nan"), float("inf"), -0.5])
    d = torch.arange(1.0, 9.0)
    want = torch.tensor([1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 8.0])       # fl32(1.001) <= fl32(1.001); NaN is masked
    assert torch.equal(G.ste_mask(d, w), want)


def test_chunked_sum_rounds_every_chunk():
    f32 = torch.float32
    c = float(torch.tensor(1.0, dtype=f32) / torch.tensor(15.0, dtype=f32))          # fl(1 / 15), the 4-bit codes' factor
    parts = [torch.tensor([1.0], dtype=F64), torch.tensor([5.0], dtype=F64)]
    got = G.chunked_sum(parts, c)
    cf = torch.tensor(c, dtype=f32)
    want = torch.tensor([1.0], dtype=f32) * cf + torch.tensor([5.0], dtype=f32) * cf     # fl(fl(1 c) + fl(5 c))
    once = torch.tensor([6.0], dtype=f32) * cf                                           # fl(6 c): one scale of the total
    assert torch.equal(got, want)
    assert not torch.equal(want, once)              # so a reference that scaled the total once would fail the GPU tests
    with pytest.raises(AssertionError):
        G.chunked_sum([torch.tensor([2.0 ** 24 + 1], dtype=F64)])


def test_moving_one_term_changes_the_references():
    x = G.pm1((2, 3, 6, 6), 1, "cpu", channels_last=False).to(F64)
    g = G.grad_ints((2, 4, 6, 6), 3, 2, "cpu", channels_last=False, zeros=False).to(F64)
    w = G.pm1((4, 3, 3, 3), 3, "cpu", channels_last=False).to(F64)
    gw = G.conv_grad_weight64(x, g, 3, 1, 1)
    gx = G.conv_grad_input64(g, w, (6, 6), 1, 1)
    g2 = g.clone()
    g2[1, 2, 5, 5], g2[1, 2, 5, 4] = g[1, 2, 5, 4], g[1, 2, 5, 5]          # swap two positions of one channel
    if torch.equal(g2, g):
        g2[1, 2, 5, 5] += 1
    assert not torch.equal(G.conv_grad_weight64(x, g2, 3, 1, 1), gw)
    assert not torch.equal(G.conv_grad_input64(g2, w, (6, 6), 1, 1), gx)
    x2 = x.clone()
    x2[0, 1, 0, 0] = -x2[0, 1, 0, 0]
    assert not torch.equal(G.conv_grad_weight64(x2, g, 3, 1, 1), gw)


def _wgrad(p, q):
    return G.conv_grad_weight64(q, p, 3, 1, 1)


def test_proves_exact_holds_on_designed_operands():
    g = G.grad_ints((4, 8, 6, 6), 8, 1, "cpu", exp=-40, channels_last=False)
    x = G.pm1((4, 5, 6, 6), 2, "cpu", channels_last=False)
    for split in ("f16x2", "bf16x3"):
        ok, why = G.proves_exact(g, x, _wgrad, split)
        assert ok, why
    # per-channel exponents 2^-20 .. 2^20 are exact under the per-channel scale, not under the per-tensor one
    gc = G.grad_ints((4, 8, 6, 6), 8, 3, "cpu", ch_exps=G.spread_exps(8, -20, 20, 4), channels_last=False)
    ok, why = G.proves_exact(gc, x, _wgrad, "f16x2", a_channel_dim=1, out_channel_dim=0)
    assert ok, why
    ok, why = G.proves_exact(gc, x, _wgrad, "f16x2", a_channel_dim=1)
    assert not ok and "2^24" in why, why                  # one bound for all rows: 2^40 spread of units
    ok, why = G.proves_exact(gc, x, _wgrad, "f16x2")
    assert not ok and "split" in why, why
    # codes of a 4-bit activation and a real image under its own per-tensor scale
    q = G.int_uniform((4, 5, 6, 6), 0, 15, 5, "cpu", channels_last=False)
    assert G.proves_exact(g, q, _wgrad, "f16x2", a_channel_dim=1, out_channel_dim=0)[0]
    img = G.int_uniform((4, 5, 6, 6), -4, 4, 6, "cpu", channels_last=False) * 2.0 ** -7
    assert G.proves_exact(g, img, _wgrad, "f16x2", split_b="f16x2")[0]


def test_proves_exact_fails_where_it_must():
    x = torch.ones((1, 1, 70, 70), dtype=torch.float32)
    big = torch.full((1, 1, 70, 70), 2047.0) * 2.0 ** -3
    ok, why = G.proves_exact(big, x, lambda p, q: G.conv_grad_weight64(q, p, 1), "bf16x3")
    assert ok, why                                       # 4900 * 2047 < 2^24
    big = torch.full((1, 1, 100, 100), 2047.0) * 2.0 ** -3
    ok, why = G.proves_exact(big, torch.ones_like(big), lambda p, q: G.conv_grad_weight64(q, p, 1), "bf16x3")
    assert not ok and "2^24" in why, why                 # 10^4 * 2047 > 2^24
    # 2049 = 2^11 + 1 next to 2^14: under the per-tensor scale it needs the lo term; 2^-30 next to 2^10 is lost
    g = torch.tensor([[2.0 ** 10, 2.0 ** -30]])
    ok, why = G.proves_exact(g, torch.ones((1, 1)), lambda p, q: p @ q, "f16x2")
    assert not ok and "split" in why, why
    ok, why = G.proves_exact(torch.tensor([[1.0 + 2.0 ** -20]]), torch.ones((1, 1)), lambda p, q: p @ q, "f16x2")
    assert ok, why                                       # 21 significant bits: exact as hi + lo
    ok, why = G.proves_exact(torch.tensor([[0.1]]), torch.ones((1, 1)), lambda p, q: p @ q, "f16x2")
    assert not ok and "split" in why, why                # fl32(0.1) has 24 significant bits, hi + lo 22
    ok, why = G.proves_exact(torch.tensor([[1.0]]), torch.tensor([[1.0 / 3.0]]), lambda p, q: p @ q, "f16x2")
    assert not ok and "exact operand" in why, why


def test_quantum_exp():
    assert G.quantum_exp(torch.tensor([3.0, 5.0, 6.0])) == 0
    assert G.quantum_exp(torch.tensor([0.0, 3.0 * 2.0 ** -40, 2.0 ** -30])) == -40
    assert G.quantum_exp(torch.tensor([0.0])) is None
    assert G.quantum_exp(torch.tensor([12.0, 2.0 ** 30])) == 2
