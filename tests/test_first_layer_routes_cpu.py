"""``_fused.first_layer_rungs``: the pure selector of the forward route ladder for real-valued first-layer convs, against a table
written out by hand from the predicates (ops.first3x3_applicable, direct_first_layer_applicable, d2s_first_layer_applicable,
first_direct_applicable, s2d_applicable) and the route switches.  Nothing is launched: the selector runs without a device."""
import pytest

from pytorch_quantize_impls_amd import ops
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import fused as fused_mod

NIB11, NIB22, BITS, F32 = (1, 1), (2, 2), "bits", None

VGG = (3, 64, 3, 1, 1, 1, 5, 7)
C3 = (3, 32, 3, 1, 1, 1, 6, 6)
C6 = (6, 32, 3, 1, 1, 1, 6, 6)
ALEX = (3, 24, 11, 4, 2, 1, 33, 35)


def rungs(case, kind="binary", out=NIB11, pooled=False, allowed=None):
    C, Cout, k, stride, padding, dilation, H, W = case
    kw = {} if allowed is None else {"allowed": allowed}
    return _fused.first_layer_rungs(C, Cout, (k, k), stride, padding, dilation, H, W, kind, out=out, pooled=pooled, **kw)


@pytest.mark.parametrize("case,want", [
    (VGG, ("first3x3", "direct3x3", "s2d", "plain")),
    (C3, ("direct3x3", "d2s", "s2d", "plain")),
    ((5, 32, 3, 1, 1, 1, 6, 6), ("direct3x3", "d2s", "s2d", "plain")),
    (C6, ("d2s", "s2d", "plain")),
    ((17, 24, 3, 1, 1, 1, 6, 6), ("s2d", "plain")),
    (ALEX, ("first_direct", "s2d", "plain")),
    ((4, 24, 4, 2, 1, 1, 10, 10), ("first_direct", "s2d", "plain")),
    ((3, 24, 5, 1, 2, 1, 9, 6), ("s2d", "plain")),
    ((3, 24, 3, 1, 0, 1, 6, 7), ("plain",)),
    ((3, 24, 3, 1, 1, 2, 6, 7), ("plain",)),
])
def test_default_switches_unpooled_nibble_halo_1(case, want):
    assert rungs(case) == want
    assert rungs(case, kind="ternary") == want


@pytest.mark.parametrize("case,out,pooled,want", [
    # fp32 output: the direct 3x3 kernel and the output-blocked form write planes only
    (VGG, F32, False, ("first3x3", "s2d", "plain")),
    (C3, F32, False, ("s2d", "plain")),
    (ALEX, F32, False, ("first_direct", "s2d", "plain")),
    # threshold bits: the direct kernel stays, the output-blocked form (depth-to-space in the NIBBLE epilogue) goes
    (C3, BITS, False, ("direct3x3", "s2d", "plain")),
    (C6, BITS, False, ("s2d", "plain")),
    # a pool follows: the conv writes bits whatever the block hands on
    (C3, BITS, True, ("direct3x3", "s2d", "plain")),
    (C3, NIB11, True, ("direct3x3", "s2d", "plain")),
    (C3, NIB22, True, ("direct3x3", "s2d", "plain")),
    (VGG, NIB22, True, ("first3x3", "direct3x3", "s2d", "plain")),
    # halo (2, 2): the direct kernel writes the halo-1 plane only; the other rungs expand or write any halo
    (C3, NIB22, False, ("d2s", "s2d", "plain")),
    (VGG, NIB22, False, ("first3x3", "s2d", "plain")),
    # odd H or odd W: no 2x2 output blocks
    ((3, 32, 3, 1, 1, 1, 7, 6), NIB11, False, ("direct3x3", "s2d", "plain")),
    ((3, 32, 3, 1, 1, 1, 6, 7), NIB11, False, ("direct3x3", "s2d", "plain")),
    ((6, 32, 3, 1, 1, 1, 6, 7), NIB11, False, ("s2d", "plain")),
])
def test_output_form(case, out, pooled, want):
    assert rungs(case, out=out, pooled=pooled) == want


def test_switches_are_read_at_call_time(monkeypatch):
    with ops.scope(FIRST_3X3=False):
        assert rungs(VGG) == ("direct3x3", "s2d", "plain")
    with ops.scope(FIRST_DIRECT=False):
        assert rungs(ALEX) == ("s2d", "plain")
        assert rungs(ALEX, kind="xnor") == ("bf16x6",)
    with ops.float_split("bf16x3"):
        assert rungs(VGG) == ("direct3x3", "s2d", "plain")
    assert rungs(VGG) == ("first3x3", "direct3x3", "s2d", "plain")
    monkeypatch.setattr(ops, "FIRST_3X3", False)
    assert rungs(VGG) == ("direct3x3", "s2d", "plain")
    monkeypatch.setattr(fused_mod, "DIRECT_FIRST_LAYER", False)
    assert rungs(VGG) == ("s2d", "plain")
    assert rungs(C3) == ("d2s", "s2d", "plain")
    monkeypatch.setattr(fused_mod, "D2S_FIRST_LAYER", False)
    assert rungs(C3) == ("s2d", "plain") and rungs(C6) == ("s2d", "plain")
    monkeypatch.setattr(_fused, "USE_S2D", False)
    assert rungs(C3) == ("plain",) and rungs(ALEX) == ("first_direct", "plain")
    monkeypatch.setattr(ops, "FIRST_DIRECT", False)
    assert rungs(ALEX) == ("plain",)


def test_allowed_rungs_keep_the_ladder_order():
    assert rungs(VGG, allowed=("plain", "s2d", "first_direct", "first3x3")) == ("first3x3", "s2d", "plain")
    assert rungs(C3, allowed=("first3x3", "direct3x3", "d2s")) == ("direct3x3", "d2s")
    assert rungs(ALEX, allowed=("first3x3", "direct3x3", "d2s")) == ()


def test_xnor_real_weight_pair():
    for out in (F32, BITS, NIB11, NIB22):
        assert rungs(ALEX, kind="xnor", out=out) == ("first_direct_real", "bf16x6")
        assert rungs((3, 24, 3, 1, 1, 1, 6, 7), kind="xnor", out=out) == ("bf16x6",)
    assert rungs(ALEX, kind="xnor", allowed=("bf16x6",)) == ("bf16x6",)
