"""One-term bf16 route of the Lin / Log family, the parts that need no GPU: the C-ABI surface, the tag side channel of the
quantisers' planes, the exactness predicate on bit patterns, plane geometry, and unchanged CPU behaviour."""
import numpy as np
import torch
import torch.nn.functional as F

from pytorch_quantize_impls_amd import _lib, ops, packed
from pytorch_quantize_impls_amd.functions import _fused, log_lin_connect
from pytorch_quantize_impls_amd.layers import LinearQuant, QuantConv2d

NEW_ENTRY_POINTS = ("qt_linlog_quantize_bf16_f32", "qt_bf16_pack_check_f32", "qt_check_bf16_exact_f32",
                    "qt_bf16x1_pack_levels_f32", "qt_bf16x1_pack_conv_levels_f32")


def bf16_exact_np(x) -> np.ndarray:
    """The predicate of qt_check_bf16_exact_f32 / qt_bf16_pack_check_f32 on fp32 bit patterns: finite, low 16 bits zero, and
    zero or a normal number."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    e = (u >> 23) & 0xFF
    return ((u & 0xFFFF) == 0) & (e != 0xFF) & ((e != 0) | ((u & 0x7FFFFFFF) == 0))


def test_new_entry_points_are_declared_and_bound():
    declared = _lib.header_declared_functions()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    # the one-term level packs take the arguments of the three-term ones
    assert _lib.SIGNATURES["qt_bf16x1_pack_levels_f32"] == _lib.SIGNATURES["qt_bf16x3_pack_levels_f32"]
    assert _lib.SIGNATURES["qt_bf16x1_pack_conv_levels_f32"] == _lib.SIGNATURES["qt_bf16x3_pack_conv_levels_f32"]
    assert _lib.SIGNATURES["qt_check_bf16_exact_f32"] == _lib.SIGNATURES["qt_check_pm1_f32"]


def test_exactness_predicate_on_edge_values():
    f = np.float32
    cases = [
        (0.0, True), (-0.0, True), (1.0, True), (-1.5, True), (2.0 ** -126, True), (-(2.0 ** -126), True), (2.0 ** 127, True),
        (255.0, True), (256.0, True), (1.9921875, True),              # 8 significant bits: 255 / 128
        (257.0, False), (1.00390625, False),                            # 9 significant bits (bit 15 of the pattern)
        (0.1, False), (1.0 + 2.0 ** -23, False),
        (2.0 ** -127, False), (2.0 ** -133, False), (2.0 ** -149, False), (-(2.0 ** -130), False),   # denormals, bf16-"exact" or not
        (float("inf"), False), (-float("inf"), False), (float("nan"), False),
    ]
    x = np.array([c[0] for c in cases], f)
    assert bf16_exact_np(x).tolist() == [c[1] for c in cases]
    # patterns: bit 15 set alone, a NaN with only low payload bits, a NaN with a high payload bit
    pat = np.array([0x3F808000, 0x7F800001, 0x7FC00000, 0x00010000, 0x00800000, 0x80000000], np.uint32).view(f)
    assert bf16_exact_np(pat).tolist() == [False, False, False, False, True, True]


def test_every_level_of_an_exact_configuration_passes_the_predicate():
    g = torch.Generator().manual_seed(1)
    for dtype, fsr, bits in [("lin", 1, 8), ("lin", 2, 4), ("lin", -60, 8), ("lin", 60, 1), ("lin", 7, 3), ("log", 1, 2),
                             ("log", 2, 3), ("log", 7, 4), ("log", 2, 7), ("log", 0, 6), ("log", 60, 5)]:
        assert ops.levels_exact_in_bf16(dtype, fsr, bits)
        x = (torch.rand(4096, generator=g) * 2 - 1) * 2.0 ** fsr * 1.5
        x[:8] = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-38, -1e-45, 2.0 ** fsr, 3e38])
        for sign in (True, False):
            y = log_lin_connect.Quant(x, dtype, fsr, bits, with_sign=sign).numpy()
            assert bf16_exact_np(y).all(), (dtype, fsr, bits, sign)
    assert not ops.levels_exact_in_bf16("lin", 1, 9) and not ops.levels_exact_in_bf16("log", 1, 7)
    y = log_lin_connect.Quant(torch.linspace(-2, 2, 4097), "lin", 1, 9).numpy()
    assert not bf16_exact_np(y).all()


class _Planes:
    terms, rows, K = 1, 6, 4


def test_level_tags_follow_the_version_counter_and_the_shape():
    t = torch.zeros(6, 4)
    assert packed.lookup_levels(t, packed.ROWS_LAST) is None
    p = _Planes()
    assert packed.attach_levels(t, p, packed.ROWS_LAST) is t
    assert packed.lookup_levels(t, packed.ROWS_LAST) is p
    assert packed.lookup_levels(t, packed.NHWC) is None                 # another layout
    assert packed.lookup(t, packed.ROWS_LAST) is None and packed.lookup_codes(t, packed.ROWS_LAST) is None   # separate channels
    assert packed.lookup_levels(t.view(4, 6), packed.ROWS_LAST) is None  # a view is another tensor object
    t.add_(1.0)                                                         # in-place write
    assert packed.lookup_levels(t, packed.ROWS_LAST) is None
    t2 = packed.attach_levels(torch.zeros(6, 4), p, packed.ROWS_LAST)
    t2.resize_(3, 8)                                                    # shape change (resize_ does not bump the version)
    assert packed.lookup_levels(t2, packed.ROWS_LAST) is None
    with torch.inference_mode():
        ti = torch.zeros(6, 4)
    packed.attach_levels(ti, p, packed.ROWS_LAST)                       # no version counter: never tagged
    assert packed.lookup_levels(ti, packed.ROWS_LAST) is None


def test_plane_geometry_and_one_term_planes():
    assert ops.triple_ld_bytes(13, 128, 1) == 128 and ops.triple_ld_bytes(64, 128, 1) == 128 and ops.triple_ld_bytes(65, 128, 1) == 256
    assert ops.triple_ld_bytes(3, 16, 1) == 16 and ops.triple_ld_bytes(13, 16, 1) == 32 and ops.triple_ld_bytes(40, 16, 1) == 80
    assert ops.triple_ld_bytes(13, 16, 3) == 80                           # the three-term granules are what they were
    one = ops.TriplePlanes(data=torch.zeros((2, 64), dtype=torch.int16), rows=2, K=13, terms=1)
    assert one.elem == 2 and ops.TriplePlanes(data=one.data, rows=2, K=13).elem == 2
    assert ops.TriplePlanes(data=one.data, rows=2, K=13, terms=2).elem == 3
    geo = ops._act_plane_geometry
    assert geo(torch.zeros(2, 13, 5, 7)) == ("nhwc", (2, 13, 5, 7), (455, 35, 7, 1), 32)
    cl = torch.zeros(2, 13, 5, 7).contiguous(memory_format=torch.channels_last)
    assert geo(cl) == ("nhwc", (2, 13, 5, 7), (455, 1, 91, 13), 32)
    assert geo(torch.zeros(2, 3, 40)) == ("rows_last", (6, 40, 1, 1), (40, 1, 0, 0), 128)
    assert geo(torch.zeros(8, 6).t()) is None and geo(torch.zeros(7)) is None and geo(torch.zeros(2, 4, 6, 6)[:, :, ::2]) is None


def test_route_switch_is_scoped():
    assert _fused.LOGLIN_ONE_TERM is True and "LOGLIN_ONE_TERM" in _fused._SCOPED
    with _fused.scope(LOGLIN_ONE_TERM=False):
        assert _fused._cfg("LOGLIN_ONE_TERM") is False
        with _fused.scope(LOGLIN_ONE_TERM=True):
            assert _fused._cfg("LOGLIN_ONE_TERM") is True
        assert _fused.loglin_act_planes(torch.zeros(2, 4), None, packed.ROWS_LAST) == (None, None)
    assert _fused._cfg("LOGLIN_ONE_TERM") is True
    assert _fused.loglin_act_planes(torch.zeros(2, 4), None, packed.ROWS_LAST) == (None, None)     # host tensors: never


def test_cpu_quantisers_and_layers_unchanged():
    """CPU tensors evaluate the reference expressions, carry no tag, and the layers contract them with F.linear / F.conv2d."""
    torch.manual_seed(0)
    x2, x4 = torch.randn(9, 24) * 3, torch.randn(2, 5, 7, 7) * 3
    for dtype, fsr, bits, sign in [("lin", 1, 8, False), ("lin", 2, 4, True), ("log", 1, 2, True), ("log", 2, 3, False)]:
        q = log_lin_connect.nnQuant(dtype, fsr, bits, with_sign=sign)
        for x in (x2, x4):
            y = q(x)
            expr = log_lin_connect._lin_expr(x, fsr, bits, 1 if sign else 0) if dtype == "lin" else \
                log_lin_connect._log_expr(x, fsr, bits, sign)
            assert torch.equal(y, expr)
            assert packed.lookup_levels(y, packed.ROWS_LAST) is None and packed.lookup_levels(y, packed.NHWC) is None
        lin = LinearQuant(24, 10, True, dtype=dtype, fsr=fsr, bit_width=bits)
        conv = QuantConv2d(5, 6, 3, padding=1, fsr=fsr, bit_width=bits, dtype=dtype)
        a2, a4 = q(x2), q(x4)
        for mode in (True, False):
            lin.train(mode), conv.train(mode)
            with torch.no_grad():
                assert torch.equal(lin(a2), F.linear(a2, lin.weight_op(lin.weight), lin.bias))
                cw = conv.weight_op(conv.weight) if mode else conv.weight
                assert torch.equal(conv(a4), F.conv2d(a4, cw, conv.bias, 1, 1))
        lin.train(True), conv.train(True)
        xi = a2.clone().requires_grad_(True)
        lin(xi).sum().backward()
        assert xi.grad is not None and lin.weight.grad is not None
