"""tests/_levels_exact.py itself: its quantisers against the reference's own vectors, the plane codecs, the exactness bound of the
designed operands, and the share of log ties of the inputs the GPU cases use."""
import os

import numpy as np
import pytest
import torch

import _levels_exact as L

HERE = os.path.dirname(os.path.abspath(__file__))
ACT_QUANTS = (("lin", 1, 3, False), ("lin", 1, 8, False), ("log", 1, 3, True), ("lin", 2, 8, True), ("log", 2, 3, False))


@pytest.fixture(scope="module")
def g9():
    return np.load(os.path.join(HERE, "golden", "golden_loglin_v1.npz"))


def test_quantisers_equal_the_reference_vectors(g9):
    """Lin bit for bit (sign of zero, NaN, infinities included); Log bit for bit up to the tie rule — the vectors were made with
    fp32 log2, the helper uses float64."""
    moved_total = 0
    for fsr, bits in g9["g9_cfgs"].tolist():
        for sign in (True, False):
            for nm in ("edge", "rand"):
                x = torch.from_numpy(g9[f"g9_{nm}"])
                tag = f"f{fsr}_b{bits}_s{int(sign)}_{nm}"
                for kind in ("lin", "log"):
                    want = torch.from_numpy(g9[f"g9_{kind}_{tag}"])
                    # the reference's vector plays the part of the device result
                    ties, moved, rep = L.compare_levels(want, x, (kind, fsr, bits, sign), names=("i",), what=f"{kind} {tag}")
                    assert not rep, rep
                    assert kind == "log" or (ties, moved) == (0, 0)
                    moved_total += moved
    assert moved_total <= 2         # fp32 against float64 rounding of log2 differs in about 1 of 2e7 Gaussian samples


def test_lin_is_one_rounding_per_operation():
    """Against exact rational arithmetic on a grid that crosses every rounding boundary of Lin(fsr=1, bits=3)."""
    from fractions import Fraction
    xs = torch.arange(-40, 200, dtype=torch.float32) / 64.0
    got = L.lin_quant(xs, 1, 3, False)
    step = Fraction(1, 4)
    for x, g in zip(xs.tolist(), got.tolist()):
        r = round(Fraction(x) / step)                                # Python rounds a Fraction half to even
        assert Fraction(g) == min(max(r * step, 0), 2), (x, g)
    sg = L.lin_quant(xs, 1, 3, True)
    assert torch.equal(sg, torch.sign(xs) * L.lin_quant(xs.abs(), 1, 3, False))


def test_log_ties_are_found_and_either_neighbour_passes():
    t = torch.tensor([2.0 ** 0.5, 2.0 ** -1.5, 3.0, 2.0 ** 2.5, 0.0, float("inf"), 2.0 ** -9.5, 2.0 ** 1.5], dtype=torch.float32)
    spec = ("log", 1, 3, True)                                      # levels 2^-7 .. 2^1
    tie, other = L.log_ties(t, 1, 3)
    assert tie.tolist() == [True, True, False, False, False, False, False, True]       # 2^2.5: beyond hi + 1; 2^-9.5: below lo - 1
    want = L.quantise(t, spec)
    for flip in (False, True):
        got = torch.where(tie & flip, other, want)
        ties, moved, rep = L.compare_levels(got, t, spec, names=("i",), cap=1.0)
        assert not rep and ties == 3 and moved == (2 if flip else 0)
    # 2^1.5 rounds to 2 or to 1, both clamp to hi = 1: the other level is the same level
    assert float(other[7]) == 2.0 and float(want[7]) == 2.0
    # a tie on a level that is not adjacent, and a non-tie on the adjacent level, both fail
    bad = want.clone()
    bad[0] = 4.0
    assert L.compare_levels(bad, t, spec, names=("i",), cap=1.0)[2]
    bad = want.clone()
    bad[2] = 1.0                                                     # t = 3 is 2^1 (4 clamped), and no tie
    assert L.compare_levels(bad, t, spec, names=("i",), cap=1.0)[2]
    with pytest.raises(AssertionError, match="over the cap"):
        L.compare_levels(want[:2], t[:2], spec, names=("i",))


def test_plane_codecs_round_trip():
    g = torch.Generator().manual_seed(3)
    for C, (H, W), halo in ((3, (5, 4), (0, 0)), (13, (7, 9), (1, 1)), (64, (4, 4), (2, 1)), (130, (3, 2), (0, 3))):
        y = L.quantise(torch.randn((2, C, H, W), generator=g) * 2, ("lin", 2, 8, True))
        y[0, 0, 0, 0] = -0.0
        for v in (y, y.contiguous(memory_format=torch.channels_last)):
            p = L.encode_plane(v, halo)
            assert p.shape == (2 * (H + 2 * halo[0]) * (W + 2 * halo[1]), (C + 7) // 8 * 8)
            back = L.decode_plane(p, (2, C, H, W), halo)
            assert torch.equal(back.view(torch.int32), v.permute(0, 2, 3, 1).contiguous().view(torch.int32))
    r = L.quantise(torch.randn((9, 70), generator=g), ("log", 1, 3, True))
    p = L.encode_plane(r, granule=128)
    assert p.shape == (9, 128) and torch.equal(L.decode_plane(p, (9, 70), granule=128), r)
    with pytest.raises(AssertionError, match="not single bf16 terms"):
        L.encode_plane(torch.full((1, 3), 0.1))
    # what a launch did not write shows up: pad channel, halo, interior
    p = L.encode_plane(y, (1, 1))
    C, H, W = 130, 3, 2
    for row, col, msg in ((0, 0, "halo"), (1 * (W + 2) + 1, C, "pad-channel")):
        q = p.clone()
        q[row, col] = L.NAN_FILL
        with pytest.raises(AssertionError, match=msg):
            L.decode_plane(q, (2, C, H, W), (1, 1))
    q = L.nan_filled(p.shape[0], p.shape[1], "cpu")
    with pytest.raises(AssertionError):
        L.decode_plane(q, (2, C, H, W), (1, 1))


@pytest.mark.parametrize("kind", ["lin", "log", "image"])
def test_designed_sums_are_exact_in_fp32_in_any_order(kind):
    Cin = 3 if kind == "image" else 64
    x = L.designed_activation(kind, (1, Cin, 3, 3), 5, "cpu")
    w = L.designed_weight("log" if kind == "log" else "lin", (4, Cin, 3, 3), 6, "cpu")
    b = L.designed_bias(4, 7, "cpu")
    units = L.assert_exact_bound(x, w, b, kind)
    assert units < 2 ** 24
    # the worst case of the largest layer the GPU cases run (256 channels, 3 x 3) stays under the bound too
    assert 256 * 9 * 256 + 40 < 2 ** 24
    prods = (x.reshape(1, -1) * w.reshape(4, -1))                  # the products of the centre output pixel, fp32 (exact)
    assert torch.equal(prods.double(), x.reshape(1, -1).double() * w.reshape(4, -1).double())
    want = prods.double().sum(1) + b.double()
    g = torch.Generator().manual_seed(8)
    for _ in range(6):
        order = torch.randperm(prods.shape[1] + 1, generator=g)
        terms = torch.cat([prods, b.view(4, 1)], 1)[:, order]
        acc = torch.zeros(4)
        for j in range(terms.shape[1]):
            acc = acc + terms[:, j]                                  # one fp32 addition at a time
        assert torch.equal(acc.double(), want)
    y = L.exact_conv_f32(x, w, b, 1, 0)
    assert torch.equal(y.view(-1).double(), want)
    with pytest.raises(AssertionError):
        L.assert_exact_bound(x * 1.0001, w, b)
    with pytest.raises(AssertionError):
        L.assert_exact_bound(x, w, b + 2.0 ** -30)                 # a bias off the grid shrinks the unit: no longer below 2^24


def test_tie_share_of_the_stated_inputs_is_far_below_the_cap():
    """The pre-quantiser values of the GPU cases are BatchNorm outputs of sums of designed products: affine images of integers.
    A stand-in with the same make (integer sums in units of 2^-5 through a random affine map per channel) and plain Gaussians
    both stay under a quarter of the cap."""
    g = torch.Generator().manual_seed(11)
    sums = torch.randint(-60000, 60001, (256, 4096), generator=g).float() * 2.0 ** -5
    a, b = torch.rand((256, 1), generator=g) * 0.02 + 0.001, torch.randn((256, 1), generator=g)
    for t in (sums * a + b, torch.randn((256, 4096), generator=g) * 3):
        for spec in ACT_QUANTS:
            if spec[0] == "log":
                tie, _ = L.log_ties(t, spec[1], spec[2])
                share = float(tie.double().mean())
                assert share < L.TIE_CAP / 4, (spec, share)
