"""tests/_exact.py (the exact reference of the threshold-bit GPU tests) against the C oracle on small shapes, on the CPU:
the exact conv against oracle.conv2d, the threshold bits (pooled or not, binary / ternary weights, edge channels) against
oracle.bin_conv_pool_bn_sign_planes, and the plane codecs against each other."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _exact as X
from pytorch_quantize_impls_amd import synth


def _edge_affine(Cout, seed):
    bias = synth.normal(seed, (Cout,)) * 3
    alpha = synth.uniform(seed + 1, (Cout,), -0.3, 0.3)
    beta = synth.uniform(seed + 2, (Cout,), -4, 4)
    alpha[0], beta[0] = 0.0, 0.5
    alpha[1], beta[1] = 0.0, -1.0
    beta[2], beta[3] = 1e6, -1e6
    alpha[4], beta[4] = -0.0, 1.0
    alpha[5] = np.nan
    beta[6], beta[7] = np.inf, -np.inf
    alpha[8], beta[8], bias[8] = 1.0, -2.0, 0.0          # bit <=> acc < 2: acc = 2 is the tie
    alpha[9], beta[9], bias[9] = -1.0, 2.0, 0.0          # bit <=> acc > 2
    return bias.astype(np.float32), alpha.astype(np.float32), beta.astype(np.float32)


@pytest.mark.parametrize("N,C,Cout,H,W,k,stride,pad,pool,kind", [
    (2, 40, 36, 9, 7, 3, 1, 1, (1, 1), "binary"),
    (3, 32, 33, 11, 11, 3, 1, 1, (3, 2), "ternary"),
    (2, 17, 64, 13, 12, 5, 1, 2, (3, 2), "binary"),
    (1, 70, 40, 15, 15, 3, 2, 1, (1, 1), "ternary"),
    (2, 64, 12, 6, 6, 3, 1, 1, (2, 2), "binary"),
])
def test_exact_reference_matches_the_oracle(oracle, N, C, Cout, H, W, k, stride, pad, pool, kind):
    seed = N * 1000 + C * 10 + Cout
    rows = N * H * W
    words = X.random_bit_words(rows, C, seed, "cpu")
    X.check_pad_bits(words, C)
    x = X.pm1_nchw(words, N, H, W, C)
    assert set(torch.unique(x).tolist()) == {-1.0, 1.0}
    # the codec round trip
    assert torch.equal(X.words_of_bits(X.bits_of_words(words, C)), words)
    w = synth.uniform(seed + 1, (Cout, C, k, k), -1.4, 1.4)
    wq = oracle.safe_sign(w) if kind == "binary" else oracle.ternarize(w)
    bias, alpha, beta = _edge_affine(Cout, seed + 2)
    acc = X.exact_conv(x, torch.from_numpy(wq), stride, pad)
    ref = oracle.conv2d(x.numpy().astype(np.float32), wq, None, stride, pad)
    assert np.array_equal(acc.numpy(), ref.astype(np.float64))
    pk, ps = pool
    pacc = F.max_pool2d(acc, pk, ps) if pool != (1, 1) else acc
    bits, v = X.predicate(pacc, torch.from_numpy(bias), torch.from_numpy(alpha), torch.from_numpy(beta))
    plane, (Ho, Wo) = oracle.bin_conv_pool_bn_sign_planes(x.numpy().astype(np.float32), wq, bias, stride, pad, 1, alpha, beta, pk, ps)
    want = X.bits_of_words(torch.from_numpy(plane.view(np.int32)).reshape(N, Ho, Wo, -1), Cout)
    got = bits.permute(0, 2, 3, 1)
    msg = X.mismatch_report(got, want, pacc.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1), what="reference vs oracle")
    assert not msg, msg
    # both bit values occur in the ordinary channels, and the edge channels are the constants they must be
    assert bool(got[..., 10:].any()) and not bool(got[..., 10:].all())
    assert not bool(got[..., 0].any()) and bool(got[..., 1].all())          # alpha 0: beta >= 0 never, beta < 0 always
    assert not bool(got[..., 2].any()) and bool(got[..., 3].all())          # |beta| 1e6 dominates every sum
    assert not bool(got[..., 5].any()) and not bool(got[..., 6].any()) and bool(got[..., 7].all())   # NaN slope, +-inf beta
    # the report names the first mismatch with its exact sum
    flipped = got.clone()
    flipped[0, 0, 0, 11] ^= True
    rep = X.mismatch_report(flipped, want, pacc.permute(0, 2, 3, 1), v.permute(0, 2, 3, 1), what="probe")
    assert rep.startswith("probe: 1 of") and "(n=0, y=0, x=0, c=11)" in rep and "acc=" in rep


def test_exact_conv_rejects_operands_that_are_not_pm1():
    x = torch.ones(1, 4, 3, 3, dtype=torch.float64)
    w = torch.full((2, 4, 3, 3), 1.0)
    assert float(X.exact_conv(x, w, 1, 1).max()) == 36.0
    with pytest.raises(AssertionError, match="not \\+-1"):
        X.exact_conv(x * 2, w, 1, 1)


def _encode_nib(bits, halo, ld):
    """bool [N, H, W, C] (True = -1) -> a nibble halo plane, the layout ops.bits_to_nib_pad writes."""
    N, H, W, C = bits.shape
    hy, hx = halo
    nib = torch.zeros((N, H + 2 * hy, W + 2 * hx, ld * 8), dtype=torch.int64)
    nib[:, hy:hy + H, hx:hx + W, :C] = torch.where(bits, X.NIB_NEG, X.NIB_POS)
    w = (nib.reshape(N, H + 2 * hy, W + 2 * hx, ld, 8) << (4 * torch.arange(8))).sum(-1)
    return torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32).reshape(-1, ld)


@pytest.mark.parametrize("C,halo", [(64, (1, 1)), (40, (2, 2)), (192, (1, 2))])
def test_nibble_decoder_round_trip_and_checks(C, halo):
    N, H, W = 2, 5, 4
    ld = max(4, ((C + 7) // 8 + 3) // 4 * 4)
    bits = X.bits_of_words(X.random_bit_words(N * H * W, C, C, "cpu"), C).reshape(N, H, W, C)
    plane = _encode_nib(bits, halo, ld)
    assert torch.equal(X.nib_to_bits(X.decode_nib(plane, N, H, W, C, halo)), bits)
    hy, hx = halo
    bad = plane.clone().reshape(N, H + 2 * hy, W + 2 * hx, ld)
    bad[1, 0, 0, 0] = 0x2                                  # a halo pixel with a value
    with pytest.raises(AssertionError, match="halo"):
        X.decode_nib(bad.reshape(-1, ld), N, H, W, C, halo)
    if C % 32:
        bad = plane.clone().reshape(N, H + 2 * hy, W + 2 * hx, ld)
        bad[0, hy, hx, ld - 1] = 0x2 << 28                 # the last pad channel
        with pytest.raises(AssertionError, match="pad channels"):
            X.decode_nib(bad.reshape(-1, ld), N, H, W, C, halo)
    bad = plane.clone().reshape(N, H + 2 * hy, W + 2 * hx, ld)
    bad[0, hy, hx, 0] = (bad[0, hy, hx, 0] & ~0xF) | 0x3   # not an fp4 +-1 / 0
    with pytest.raises(AssertionError, match="outside"):
        X.decode_nib(bad.reshape(-1, ld), N, H, W, C, halo)
