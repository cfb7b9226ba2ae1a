"""Depthwise DorefaConv2d inside the fused int8 code chain, the host side: the code-plane entries exist and validate before they
launch, the wrappers reject host tensors, ``FusedDepthwiseDorefaBnQuant`` declines what it cannot run, ``lazy.depthwise_deferred``
restores both switches, host layers never defer, and the reference of tests/_dw_codes.py is pinned on hand-computed outputs and
holds no sensitive element for any case of the GPU list.  The kernels: tests/test_gpu_dw_codes.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _codes_exact as C
import _dw_codes as R
from pytorch_quantize_impls_amd import _lib, lazy, ops, packed
from pytorch_quantize_impls_amd.layers import BinConv2d, DorefaConv2d, FusedDepthwiseDorefaBnQuant, FusedDorefaConvBnQuant

ENTRIES = ("qt_dwconv2d_codes", "qt_dwconv2d_codes_f32")
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
PTR = 0x7f0000001000        # stands for a device pointer: every call below must return before anything could read it


def test_entries_are_declared_in_the_header_and_bound():
    declared = _lib.header_declared_functions()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def _codes(lib, **kw):
    """C = 40, m = 1: 48-byte rows on both sides."""
    a = dict(x=PTR, ldx=48, ihy=1, ihx=1, inv_n=1.0 / 15, w=PTR, bias=None, alpha=PTR, beta=PTR, stats=None, relu=1, bits=4, codes=PTR,
             ldc=48, ohy=1, ohx=1, flag=PTR, N=2, C=40, m=1, H=5, W=5, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1)
    a.update(kw)
    return lib.qt_dwconv2d_codes(a["x"], a["ldx"], a["ihy"], a["ihx"], a["inv_n"], a["w"], a["bias"], a["alpha"], a["beta"], a["stats"],
                                 a["relu"], a["bits"], a["codes"], a["ldc"], a["ohy"], a["ohx"], a["flag"], a["N"], a["C"], a["m"],
                                 a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], None)


def _f32(lib, **kw):
    a = dict(x=PTR, ldx=48, ihy=0, ihx=0, inv_n=1.0 / 15, w=PTR, bias=None, flag=None, y=PTR, N=2, C=40, m=1, H=5, W=5, kh=3, kw=3,
             sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, ys=(1000, 25, 5, 1))
    a.update(kw)
    return lib.qt_dwconv2d_codes_f32(a["x"], a["ldx"], a["ihy"], a["ihx"], a["inv_n"], a["w"], a["bias"], a["flag"], a["y"], a["N"],
                                     a["C"], a["m"], a["H"], a["W"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"],
                                     a["dw"], *a["ys"], None)


def test_codes_entry_validates_before_it_launches():
    lib = _lib.load()
    # 1. negative halos and sizes, a kernel / stride below 1; too many taps
    assert _codes(lib, ihy=-1) == INVALID and _codes(lib, ihx=-1) == INVALID
    assert _codes(lib, ohy=-1) == INVALID and _codes(lib, ohx=-1) == INVALID
    assert _codes(lib, N=-1) == INVALID and _codes(lib, m=0) == INVALID and _codes(lib, sh=0) == INVALID
    assert _codes(lib, kh=5, kw=10) == UNSUPPORTED                                   # 50 taps
    assert _codes(lib, N=0, ohy=-1) == INVALID                                       # the halo's sign is looked at first
    # 2. empty tensors: nothing to do, whatever the pointers are
    assert _codes(lib, N=0, x=None, w=None, alpha=None, beta=None, codes=None, flag=None) == OK
    assert _codes(lib, C=0, x=None, codes=None) == OK
    # 3. the other limits
    assert _codes(lib, ihy=65) == UNSUPPORTED and _codes(lib, ohx=65) == UNSUPPORTED
    assert _codes(lib, C=1 << 20, m=2, N=1, H=3, W=3, ldx=1 << 20, ldc=1 << 21) == UNSUPPORTED       # C m > QT_DW_MAX_CHANNELS
    assert _codes(lib, N=1 << 20, C=1, H=40, W=40, ldx=16, ldc=16, ihy=64, ihx=64) == UNSUPPORTED   # 2^31 pixel rows and more in the input plane
    assert _codes(lib, N=1 << 20, C=1, H=40, W=40, ldx=16, ldc=16, ohy=64, ohx=64) == UNSUPPORTED   # ... in the output plane
    assert _codes(lib, kh=7, kw=7, ph=0, pw=0) == INVALID                            # does not fit a 5 x 5 image
    # 4. null tensors, the quantiser, the row strides ...
    for name in ("x", "w", "alpha", "beta", "codes", "flag"):
        assert _codes(lib, **{name: None}) == INVALID, name
    assert _codes(lib, bits=1) == INVALID and _codes(lib, bits=9) == INVALID
    assert _codes(lib, relu=2) == INVALID and _codes(lib, relu=-1) == INVALID
    assert _codes(lib, ldx=32) == INVALID and _codes(lib, ldc=32) == INVALID         # below 40 rounded up to 16
    assert _codes(lib, ldx=40) == INVALID and _codes(lib, ldc=47) == INVALID         # ... even where the channels would fit
    # ... then the alignments
    for name in ("w", "alpha", "beta", "flag"):
        assert _codes(lib, **{name: PTR + 2}) == ALIGNMENT, name
    assert _codes(lib, bias=PTR + 1) == ALIGNMENT and _codes(lib, stats=PTR + 2) == ALIGNMENT
    assert _codes(lib, ldx=52) == ALIGNMENT and _codes(lib, ldc=56) == ALIGNMENT
    assert _codes(lib, x=PTR + 4) == ALIGNMENT and _codes(lib, codes=PTR + 8) == ALIGNMENT
    assert _codes(lib, C=3, ldx=16, ldc=16, alpha=None) == INVALID                   # no C % 4 restriction: only the null pointer is refused
    assert _codes(lib, bits=1, alpha=PTR + 2) == INVALID                             # INVALID_ARG comes before ALIGNMENT


def test_f32_entry_validates_before_it_launches():
    lib = _lib.load()
    assert _f32(lib, ihy=-1) == INVALID and _f32(lib, N=-1) == INVALID and _f32(lib, kh=5, kw=10) == UNSUPPORTED
    assert _f32(lib, N=0, x=None, w=None, y=None) == OK and _f32(lib, H=0, x=None, y=None) == OK
    assert _f32(lib, ihx=65) == UNSUPPORTED
    assert _f32(lib, x=None) == INVALID and _f32(lib, w=None) == INVALID and _f32(lib, y=None) == INVALID
    assert _f32(lib, ys=(1000, 25, 5, 2)) == INVALID                                 # not a dense layout
    assert _f32(lib, ldx=32) == INVALID
    assert _f32(lib, x=PTR + 4) == ALIGNMENT and _f32(lib, y=PTR + 1) == ALIGNMENT and _f32(lib, bias=PTR + 2) == ALIGNMENT
    assert _f32(lib, flag=PTR + 2) == ALIGNMENT and _f32(lib, ldx=52) == ALIGNMENT
    assert _f32(lib, kh=7, kw=7, ph=0, pw=0) == INVALID


def _host_planes(N=1, Cc=4, H=5, W=5):
    return ops.CodePlanes(codes=torch.zeros((N * H * W, 16), dtype=torch.int8), rows=N * H * W, K=Cc, inv_n=1.0 / 15, bit_width=4)


def test_wrappers_reject_host_tensors():
    w, a = torch.randn(4, 1, 3, 3), torch.ones(4)
    epi = ops.CodeEpilogue(a, a, 4)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_codes(_host_planes(), (1, 4, 5, 5), w, None, epi, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_from_codes(_host_planes(), (1, 4, 5, 5), w, None, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_codes(torch.zeros(1, 4, 5, 5), (1, 4, 5, 5), w, None, epi, 1, 1, 1)
    with pytest.raises(TypeError):
        ops.depthwise_conv2d_from_codes(object(), (1, 4, 5, 5), w)


def _bn(c):
    return nn.BatchNorm2d(c)


def test_fused_depthwise_block_declines_what_it_cannot_run():
    ok = FusedDepthwiseDorefaBnQuant(DorefaConv2d(8, 8, 3, padding=1, groups=8, bit_width=1), _bn(8), 4)
    assert ok.out_halo == (0, 0) and ok.fold == "reference" and ok.relu == 1 and ok.bit_width == 4
    k3 = FusedDepthwiseDorefaBnQuant(DorefaConv2d(8, 16, 3, stride=2, padding=1, groups=8, bit_width=3), _bn(16), 2, relu=False,
                                     out_halo=(2, 1), fold="device")
    assert k3.fold == "device" and k3.out_halo == (2, 1) and k3.relu == 0          # any weight bit_width
    for conv, bn in ((DorefaConv2d(8, 8, 3, padding=1, groups=2, bit_width=1), _bn(8)),
                     (DorefaConv2d(8, 8, 3, padding=1, bit_width=1), _bn(8)),
                     (DorefaConv2d(1, 1, 3, padding=1, groups=1, bit_width=1), _bn(1)),
                     (BinConv2d(8, 8, 3, padding=1, groups=8), _bn(8)),
                     (DorefaConv2d(8, 8, 3, padding="same", groups=8, bit_width=1), _bn(8)),
                     (nn.Conv2d(8, 8, 3, padding=1, groups=8), _bn(8)),
                     (DorefaConv2d(8, 8, 3, padding=1, groups=8, bit_width=1), _bn(16)),
                     (DorefaConv2d(8, 8, (5, 10), padding=5, groups=8, bit_width=1), _bn(8))):                     # 50 taps
        with pytest.raises(ValueError):
            FusedDepthwiseDorefaBnQuant(conv, bn, 4)
    dwl = DorefaConv2d(8, 8, 3, padding=1, groups=8, bit_width=1)
    with pytest.raises(ValueError):
        FusedDepthwiseDorefaBnQuant(dwl, nn.BatchNorm1d(8), 4)
    with pytest.raises(ValueError):
        FusedDepthwiseDorefaBnQuant(dwl, _bn(8), 4, relu="pre")
    for bits in (1, 9):
        with pytest.raises(ValueError):
            FusedDepthwiseDorefaBnQuant(dwl, _bn(8), bits)
    # the ungrouped sibling keeps declining a depthwise conv
    with pytest.raises(ValueError):
        FusedDorefaConvBnQuant(dwl, _bn(8), 4)
    act = packed.CodeActivation(_host_planes(1, 8), (1, 8, 5, 5))
    assert act.source_channels_last is True
    with pytest.raises(ValueError):
        ok(act)                                                                      # training mode
    ok.eval()
    with pytest.raises(ValueError):
        ok(act, residual=act)
    with pytest.raises(TypeError):
        ok(torch.randn(1, 8, 5, 5))                                                  # not a CodeActivation
    with pytest.raises(ValueError):
        ok(packed.CodeActivation(_host_planes(1, 4), (1, 4, 5, 5)))                  # another channel count
    with pytest.raises(TypeError):
        ok(act)                                                                      # a host plane
    ok.refold()


def test_depthwise_deferred_restores_both_switches():
    start = (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES)
    for on in (True, False):
        with lazy.depthwise_deferred(on):
            assert (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES) == (on, on)
            with lazy.depthwise_deferred(not on):
                assert (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES) == (not on, not on)
            assert (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES) == (on, on)
        assert (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES) == start
    # the two switches are independent outside the block: a mixed setting comes back as it was
    lazy.DEFER_DEPTHWISE_CODES = not start[0]
    try:
        with pytest.raises(KeyError):
            with lazy.depthwise_deferred(start[0]):
                raise KeyError("x")
        assert (lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES) == (start[0], not start[0])
    finally:
        lazy.DEFER_DEPTHWISE_CODES = start[1]


def test_host_depthwise_dorefa_layers_never_defer():
    """On the host nothing defers, whatever the switches say: the layer keeps the torch expression."""
    dwl = DorefaConv2d(8, 8, 3, padding=1, groups=8, bit_width=1).eval()
    x = torch.randn(1, 8, 5, 5)
    for on in (True, False):
        with torch.no_grad(), lazy.depthwise_deferred(on):
            assert not lazy._dorefa_can_defer(dwl, x)
            assert not lazy._dorefa_can_defer(dwl, lazy._CodeShapeOnly((1, 8, 5, 5)))
            y = dwl(x)
        assert type(y) is torch.Tensor and torch.equal(y, torch.nn.functional.conv2d(x, dwl.weight, dwl.bias, 1, 1, 1, 8))


# ---- the reference ----------------------------------------------------------------------------------------------------------------

def test_reference_on_hand_computed_outputs():
    """One channel, 3 x 3 image of codes, 3 x 3 taps of 1/2, padding 1, inv_n = 1/4, folded alpha = 1, beta = 0, levels 15, ReLU:
        q = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    corner (0, 0): taps (1,1) (1,2) (2,1) (2,2) hit q = 1, 2, 4, 5: y = 12 / 8 = 1.5, 15 y = 22.5 — a tie, half to even: 22;
    centre (1, 1): all nine, y = 45 / 8 = 5.625, 15 y = 84.375: 84;   edge (0, 1): q = 1..6, y = 21 / 8 = 2.625, 39.375: 39;
    corner (2, 2): q = 5, 6, 8, 9: y = 3.5, 52.5 — a tie: 52."""
    q = np.arange(1, 10, dtype=np.int64).reshape(1, 1, 3, 3)
    w = np.full((1, 3, 3), 0.5, dtype=np.float32)
    one, zero = torch.ones(1), torch.zeros(1)
    geom = ((3, 3), (1, 1), (1, 1), (1, 1))
    ref = R.reference(q, 0.25, w, None, geom, C.Epi(alpha=one, beta=zero, levels=15.0, relu=1))
    codes = ref["codes"][0, :, :, 0]
    assert ref["y"][0, 0, 0, 0] == 1.5 and ref["y"][0, 0, 1, 1] == 5.625
    assert (int(codes[0, 0]), int(codes[1, 1]), int(codes[0, 1]), int(codes[2, 2])) == (22, 84, 39, 52)
    assert not ref["flag"] and ref["flag_head"] == 0 and int(C.sensitive(ref).sum()) == 0
    # the same through a negative slope: the ReLU clips everything, -0.0 included, to code 0
    neg = R.reference(q, 0.25, w, None, geom, C.Epi(alpha=-one, beta=zero, levels=15.0, relu=1))
    assert int(neg["codes"].abs().sum()) == 0
    # without the ReLU the same ties on the negative side: -22.5 -> -22, -52.5 -> -52; device form with mean 0.5, rs 2, weight -1/2,
    # bias 1/2 is t = -(y - 0.5) + 0.5 = 1 - y: corner 15 * -0.5 = -7.5 -> -8 (half to even)
    plain = R.reference(q, 0.25, w, None, geom, C.Epi(alpha=-one, beta=zero, levels=15.0, relu=0))
    assert (int(plain["codes"][0, 0, 0, 0]), int(plain["codes"][0, 2, 2, 0])) == (-22, -52)
    devf = R.reference(q, 0.25, w, None, geom, C.Epi(alpha=-one / 2, beta=one / 2, levels=15.0, stats=(one / 2, one * 2), relu=0))
    assert int(devf["codes"][0, 0, 0, 0]) == -8
    # levels 255: 255 * 1.5 = 382.5 leaves int8: code 0, flag value 1; a huge slope: flag value 3
    big = R.reference(q, 0.25, w, None, geom, C.Epi(alpha=one, beta=zero, levels=255.0, relu=1))
    assert big["flag"] and big["flag_head"] == 1 and int(big["codes"][0, 0, 0, 0]) == 0
    huge = R.reference(q, 0.25, w, None, geom, C.Epi(alpha=one * 1e6, beta=zero, levels=15.0, relu=1))
    assert huge["flag_head"] == 3
    # the plane: pixel rows of 16 bytes, the code in byte 0, a zero border
    plane = R.out_plane(ref, (1, 2))
    assert plane.shape == (5 * 7, 16) and int(plane[1 * 7 + 2, 0]) == 22 and int(plane[2 * 7 + 3, 0]) == 84
    assert int(plane.count_nonzero()) == 9
    assert torch.equal(C.decode_plane(plane, 1, 3, 3, 1, (1, 2)), ref["codes"].permute(0, 3, 1, 2))
    # a bias is added last, a multiplier reads its input channel twice
    two = R.reference(q, 0.25, np.stack([w[0], 2 * w[0]]), np.array([0.25, -0.5], dtype=np.float32), geom,
                      C.Epi(alpha=torch.ones(2), beta=torch.zeros(2), levels=3.0, relu=0))
    assert two["y"][0, 0, 0, 0] == 1.75 and two["y"][0, 1, 0, 0] == 2.5 and two["codes"][0, 0, 0].tolist() == [5, 8]


def test_the_case_list_covers_every_axis_value():
    cs = R.CASES
    assert {(c.C, c.m) for c in cs} == set(R.CM) and {(c.H, c.W) for c in cs} == set(R.MAPS) and {c.N for c in cs} == set(R.BATCHES)
    assert {(c.kernel, c.stride, c.padding, c.dilation) for c in cs} == set(R.GEOMS)
    assert {c.in_halo for c in cs} == set(R.HALOS) == {c.out_halo for c in cs}
    assert any(c.in_halo[0] > c.padding[0] and c.in_halo[1] > c.padding[1] for c in cs)         # a halo larger than the padding
    assert any(c.in_halo == (0, 0) and c.padding != (0, 0) for c in cs)                         # ... and a padding without a halo
    assert {c.in_bits for c in cs} == set(R.BITS) == {c.out_bits for c in cs}
    assert {c.relu for c in cs} == {True, False} and {c.form for c in cs} == set(R.FORMS) and {c.taps for c in cs} == set(R.TAPS)
    assert {(c.form, c.bias) for c in cs} == {(f, b) for f in R.FORMS for b in (True, False)}
    assert len({c.id for c in cs}) == len(cs)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[c.id for c in R.CASES])
def test_reference_has_no_sensitive_element_in_any_gpu_case(i):
    """The waiver of _codes_exact.compare_codes is capped at waiver_cap(numel) — 0 at these sizes — so the seeds of the list are
    chosen such that the reference itself is unambiguous everywhere: the GPU comparison is then exact."""
    r = R.build(i)
    codes = r.ref["codes"]
    assert C.waiver_cap(codes.numel()) == 0
    assert int(C.sensitive(r.ref).sum()) <= C.waiver_cap(codes.numel())
    assert int(codes.count_nonzero()) > codes.numel() // 20                          # the case says something
    assert int(codes.abs().max()) <= 127


def test_designed_case_sits_on_ties_and_on_the_relu_boundary():
    d = R.designed()
    assert d.ties >= 8 and d.on_relu >= 8 and d.below_relu > 100
    assert int(C.sensitive(d.ref).sum()) == 0 and not d.ref["flag"]
