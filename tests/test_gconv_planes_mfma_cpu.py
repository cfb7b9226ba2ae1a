"""Grouped sign convs of 16 / 32 channels per group on bit planes, without a GPU: the window, the constructor, the header."""
import pytest
import torch.nn as nn

from pytorch_quantize_impls_amd import _lib, ops
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d, XNORConv2d, FusedGroupedMfmaBnSign

# (cin_g, cout_g, kernel, stride, padding, dilation, G, H) -> inside the window
WINDOW = (((16, 16, 3, 1, 1, 1, 8, 7), True), ((32, 48, 3, 2, (1, 0), 1, 1, 7), True), ((32, 32, 1, 1, 0, 1, 32, 7), True),
          ((16, 32, 1, 2, 0, 1, 9, 14), True), ((24, 16, 3, 1, 1, 1, 8, 7), False), ((8, 16, 3, 1, 1, 1, 8, 7), False),
          ((16, 24, 3, 1, 1, 1, 8, 7), False), ((16, 64, 3, 1, 1, 1, 8, 7), False), ((16, 16, 5, 1, 1, 1, 8, 7), False),
          ((16, 16, 3, 1, 1, 2, 8, 7), False), ((16, 16, 3, 3, 1, 1, 8, 7), False), ((16, 16, 3, (1, 2), 1, 1, 8, 7), False),
          ((16, 16, 3, 1, 2, 1, 8, 7), False), ((16, 16, 3, 1, "same", 1, 8, 7), False), ((32, 32, 3, 1, 0, 1, 8, 2), False))


@pytest.mark.parametrize("case,inside", WINDOW, ids=[str(c) for c, _ in WINDOW])
def test_the_window_is_a_pure_function_of_the_shapes(case, inside):
    ci, co, k, s, p, d, G, H = case
    args = ((2, G * ci, H, H), (G * co, ci, k, k), s, p, d, G)
    assert ops.grouped_mfma_planes_applicable(*args) is inside
    assert not (inside and ops.grouped_planes_applicable(*args))                 # disjoint from the popcount plane kernel's window


@pytest.mark.parametrize("conv", (BinConv2d(192, 128, 3, padding=1, groups=8), TerConv2d(64, 64, 3, padding=1, groups=4),
                                  BinConv2d(128, 192, 3, padding=1, groups=8), BinConv2d(128, 128, 5, padding=2, groups=8),
                                  BinConv2d(128, 128, 3, padding=2, dilation=2, groups=8), XNORConv2d(128, 128, 3, padding=1, groups=8),
                                  BinConv2d(128, 128, 3, padding="same", groups=8), nn.Conv2d(128, 128, 3, groups=8)),
                         ids=("cin_g24", "groups4", "cout_g24", "k5", "dilation2", "xnor", "same", "plain"))
def test_the_constructor_refuses_declined_layers(conv):
    with pytest.raises(ValueError):
        FusedGroupedMfmaBnSign(conv, nn.BatchNorm2d(conv.out_channels))


def test_the_entries_are_declared_next_to_their_siblings():
    for new, old in (("qt_gmconv2d_sign", "qt_gconv2d_sign"), ("qt_gmconv2d_bits_f32", "qt_gconv2d_bits_f32")):
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old]
