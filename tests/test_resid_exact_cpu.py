"""tests/_resid_exact.py, the reference of the residual pass of the sign chain, pinned without a GPU: against torch's own
F.batch_norm + add + F.hardtanh and the package's CPU BinaryConnect on the designed operands, its plane packers on hand-written words,
its ambiguity reporting on a constructed fp32 midpoint, and — on exactly the realistic inputs tests/test_gpu_resid_sign.py uses — that
its own ambiguous share stays within the project's cap (the seeds of ``seed_of`` are chosen so that it does)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resid_exact as R
from pytorch_quantize_impls_amd.functions import BinaryConnect


EPS = 2.0 ** -60


def _torch_chain(d, hardtanh):
    """The module graph on the CPU: eval BatchNorm (var = 1 / rs^2 a power of 4 and an eps that var absorbs: the reciprocal square
    root is exact), add, Hardtanh, BinaryConnect."""
    var = d["var"].float()
    t = F.batch_norm(d["x"], d["mean"], var, d["weight"], d["bias"], False, 0.0, EPS)
    s = t + d["r"]
    v = s if hardtanh is None else F.hardtanh(s, *hardtanh)
    return v, BinaryConnect()(v)


@pytest.mark.parametrize("hardtanh", R.HARDTANHS, ids=str)
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 4, 3, 5), (3, 33, 7, 7)], ids=str)
def test_reference_equals_torch_on_the_designed_class(shape, hardtanh):
    d = R.designed(shape, 17, hardtanh, fma_case=False)                # (torch's BatchNorm folds its constants: no fma to compare)
    ref = R.reference(d["x"], d["mean"], d["rs"], d["weight"], d["bias"], d["r"], hardtanh)
    assert int(ref["ambiguous"].sum()) == 0
    v, sign = _torch_chain(d, hardtanh)
    nan = torch.isnan(v)
    assert torch.equal(nan, torch.isnan(ref["v"])) and int(nan.sum()) == (1 if d["placed"] > 6 else 0)
    assert torch.equal(v[~nan], ref["v"][~nan])                         # every step is exact: any evaluation order gives these values
    assert torch.equal(sign < 0, ref["neg"])                            # ... and BinaryConnect's -1 is the reference's bit
    assert torch.equal(sign, torch.where(ref["neg"], -torch.ones_like(v), torch.ones_like(v)))


def test_designed_class_places_the_edge_sums():
    ht = (-0.5, 2.0)
    d = R.designed((2, 4, 3, 5), 3, ht)
    ref = R.reference(d["x"], d["mean"], d["rs"], d["weight"], d["bias"], d["r"], ht)
    got = ref["s"][0, 0].flatten()[:9]
    bits = got.view(torch.int32).tolist()
    assert bits[0] == 0 and bits[1] == -(1 << 31) and bits[2] == 1 and bits[3] == -(1 << 31) + 1          # 0, -0.0, +-2^-149
    assert got[4] == -0.5 and got[5] == 2.0 and torch.isnan(got[6]) and got[7] == float("inf") and got[8] == float("-inf")
    assert ref["neg"][0, 0].flatten()[:9].tolist() == [False, False, False, True, True, False, False, False, True]
    v = ref["v"][0, 0].flatten()[:9]
    assert v[7] == 2.0 and v[8] == -0.5 and torch.isnan(v[6])                                               # the clamp; NaN stays
    # the fused multiply-add case of channel 1: 2^-25 with the fma, -2^-25 with a separately rounded product
    assert d["fma_case"] and float(ref["s"][0, 1, 0, 0]) == 2.0 ** -25 and not bool(ref["neg"][0, 1, 0, 0])
    m = R.f_mul(R.f_sub(d["x"][0, 1, 0, 0], d["mean"][1]), d["rs"][1])
    unfused = R.f_add(R.f_add(R.f_mul(m, d["weight"][1]), d["bias"][1]), d["r"][0, 1, 0, 0])
    assert float(unfused) == -(2.0 ** -25)
    assert int(ref["ambiguous"].sum()) == 0


def test_plane_encodings_on_hand_written_words():
    assert [R.packed_ld(k) for k in (1, 32, 128, 129, 257)] == [4, 4, 4, 8, 12]
    assert [R.pixel_ld_nib(k) for k in (1, 32, 33, 132)] == [4, 4, 8, 20]
    neg = torch.zeros((1, 3, 1, 2), dtype=torch.bool)                   # pixel 0 = (-, +, -), pixel 1 = (+, +, -)
    neg[0, :, 0, 0] = torch.tensor([True, False, True])
    neg[0, :, 0, 1] = torch.tensor([False, False, True])
    assert R.sign_plane(neg).tolist() == [[0b101, 0, 0, 0], [0b100, 0, 0, 0]]
    assert R.nib_plane(neg).tolist() == [[0xA2A, 0, 0, 0], [0xA22, 0, 0, 0]]
    n1 = R.nib_plane(neg, halo=(1, 2))                                  # [1 + 2][2 + 4] pixels, the image at row 1, columns 2 .. 3
    assert n1.shape == (18, 4) and n1[6 + 2].tolist() == [0xA2A, 0, 0, 0] and n1[6 + 3].tolist() == [0xA22, 0, 0, 0]
    assert int(np.count_nonzero(n1)) == 2
    neg = torch.zeros((1, 34, 1, 1), dtype=torch.bool)                  # channel 31: top bit of word 0; channel 33: bit 1 of word 1
    neg[0, 33] = neg[0, 31] = True
    assert R.sign_plane(neg).tolist() == [[0x80000000, 0b10, 0, 0]]
    assert R.nib_plane(neg)[0].tolist() == [0x22222222, 0x22222222, 0x22222222, 0xA2222222, 0xA2, 0, 0, 0]


def test_ambiguity_is_reported_where_float64_cannot_decide():
    """m = 1 + 2^-23, weight = 2^-18 (1 - 2^-23), bias = 64: the exact value 64 + 2^-18 - 2^-64 lies just BELOW the midpoint of 64 and
    its upper fp32 neighbour 64 + 2^-17, but float64 (ulp 2^-46 here) rounds it ONTO the midpoint.  The reference cannot know on which
    side the exact sum was: it reports the element, with both candidates followed to v."""
    m = torch.full((1, 1, 1, 1), 1.0 + 2.0 ** -23)
    w, b = torch.tensor([2.0 ** -18 * (1.0 - 2.0 ** -23)]), torch.tensor([64.0])
    zero, one, r0 = torch.zeros(1), torch.ones(1), torch.zeros((1, 1, 1, 1))
    t, alt = R.f_fma(m.flatten(), w, b)
    assert float(t) == 64.0 and float(alt) == 64.0 + 2.0 ** -17
    ref = R.reference(m, zero, one, w, b, r0)
    assert bool(ref["ambiguous"].all()) and float(ref["v"]) == 64.0
    # ambiguity is about v, not about t: behind a clamp, or a residual that absorbs the last bit, both candidates give one value
    assert not bool(R.reference(m, zero, one, w, b, r0, (-1.0, 1.0))["ambiguous"].any())
    assert not bool(R.reference(m, zero, one, w, b, torch.full((1, 1, 1, 1), 2.0 ** 20))["ambiguous"].any())
    # an exact midpoint is reported too (the float64 sum cannot be told from a rounded one): weight = 2^-18, the tie goes to even
    ref = R.reference(torch.ones((1, 1, 1, 1)), zero, one, torch.tensor([2.0 ** -18]), b, r0)
    assert bool(ref["ambiguous"].all()) and float(ref["v"]) == 64.0
    # ... and a sum float64 holds exactly OFF the midpoint is not
    assert not bool(R.reference(m, zero, one, torch.tensor([2.0 ** -18]), b, r0)["ambiguous"].any())


def test_ambiguous_share_of_the_gpu_tests_inputs_is_within_the_cap():
    total = ambiguous = 0
    for C in R.CHANNELS:
        for shape3 in R.SHAPES:
            shape = (shape3[0], C, shape3[1], shape3[2])
            for i, (_, _, _, _, hardtanh) in enumerate(R.combos(C, shape3)):
                d = R.realistic(shape, R.seed_of(C, shape3, i))
                ref = R.reference(d["x"], d["mean"], d["rs"], d["weight"], d["bias"], d["r"], hardtanh)
                n = int(ref["ambiguous"].sum())
                assert n <= R.waiver_cap(ref["v"].numel()), (C, shape3, i, n)
                total, ambiguous = total + ref["v"].numel(), ambiguous + n
                dd = R.designed(shape, R.seed_of(C, shape3, i), hardtanh)
                assert int(R.reference(dd["x"], dd["mean"], dd["rs"], dd["weight"], dd["bias"], dd["r"], hardtanh)["ambiguous"].sum()) == 0
    assert ambiguous * 1_000_000 <= R.WAIVER_PER_MILLION * total, (ambiguous, total)


def test_case_matrix_covers_every_option_value():
    for C in R.CHANNELS:
        for shape3 in R.SHAPES:
            cs = R.combos(C, shape3)
            assert {c[0] for c in cs} == set(R.RESIDUALS) and {c[3] for c in cs} == set(R.HALOS) and {c[4] for c in cs} == set(R.HARDTANHS)
            assert {(c[1], c[2]) for c in cs if c[1] != "nchw"} == {(s, p) for s in R.SUMS for p in R.PLANES}
            assert {c[0] == "nchw" for c in cs if c[1] == "nchw"} == {True, False}
