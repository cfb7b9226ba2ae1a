"""qt_bn_add_sign_f32 (csrc/resid_sign.hip) on the GPU — the entry through ctypes, then ops.bn_add_sign, then
layers.fused.FusedConvBnAddSign — against the independent reference of tests/_resid_exact.py (float64 steps rounded to fp32 once,
numpy plane packers; pinned by tests/test_resid_exact_cpu.py).

Designed operands (dyadic, every step exact, sums placed on 0, -0.0, the smallest subnormals, lo, hi, NaN, +-inf, and a case that
tells the fused multiply-add from a separately rounded one): the sum is compared by BIT PATTERN and both planes word by word.
Realistic operands: equal except where the reference itself reports the fma ambiguous, at most ``waiver_cap`` such elements (0 at
these sizes).  Every buffer the launch writes lies between sentinel words, the gap columns of pitched rows included.  All shapes are
small: a case is eleven option tuples, each launched on a designed and a realistic operand set of a few thousand elements."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import _resid_exact as R
from pytorch_quantize_impls_amd import _lib, lazy, ops, packed
from pytorch_quantize_impls_amd.functions import BinaryConnect
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d
from pytorch_quantize_impls_amd.layers.fused import FusedConvBnAddSign, FusedConvPoolBnSign

pytestmark = pytest.mark.gpu

ENTRY = "qt_bn_add_sign_f32"
OK, INVALID, ALIGNMENT, UNSUPPORTED = 0, -1, -2, -4
SENT_F = 12345.0
SENT_W = 0x5A5A5A5A
PAD = 64                     # elements: guarded views stay 16-byte aligned


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


class Buf:
    """A device buffer of ``rows`` rows of ``ld`` elements (``cols`` of them live) between sentinel elements, ``shift`` elements off
    the 16-byte alignment."""

    def __init__(self, dev, rows, cols, ld, dtype, shift=0):
        self.rows, self.cols, self.ld, self.shift = rows, cols, ld, shift
        self.sent = SENT_F if dtype == torch.float32 else SENT_W
        self.raw = torch.full((2 * PAD + rows * ld + shift,), self.sent, dtype=dtype, device=dev)
        self.view = self.raw[PAD + shift:PAD + shift + rows * ld].view(rows, ld)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def fill(self, rows_by_cols: torch.Tensor):
        self.view[:, :self.cols] = rows_by_cols.to(self.view.device)

    def live(self):
        return self.view[:, :self.cols].cpu()

    def assert_guards(self, what):
        raw = self.raw.cpu()
        lo, hi = PAD + self.shift, PAD + self.shift + self.rows * self.ld
        ok = bool((raw[:lo] == self.sent).all()) and bool((raw[hi:] == self.sent).all())
        gaps = self.view[:, self.cols:].cpu()
        assert ok and bool((gaps == self.sent).all()), f"{what}: a sentinel around the buffer or between its rows was overwritten"

    def assert_untouched(self, what):
        assert bool((self.raw == self.sent).all()), f"{what}: written although the call was refused"


def _rows(t_nchw):
    N, C, H, W = t_nchw.shape
    return t_nchw.permute(0, 2, 3, 1).reshape(N * H * W, C)


def _launch(lib, dev, d, shape, res_form, sum_mode, planes, halo, hardtanh, ldx_extra=0):
    """One launch on guarded buffers; returns what it wrote (CPU) after checking every sentinel."""
    N, C, H, W = shape
    rows = N * H * W
    xb = Buf(dev, rows, C, C + ldx_extra, torch.float32)
    xb.fill(_rows(d["x"]))
    if res_form == "nchw":
        rb = Buf(dev, 1, N * C * H * W, N * C * H * W, torch.float32)
        rb.fill(d["r"].reshape(1, -1))
        rs = (C * H * W, H * W, W, 1)
    else:
        P = C + (8 if res_form == "cl_pitch" else 0)
        rb = Buf(dev, rows, C, P, torch.float32, shift=1 if res_form == "cl_misaligned" else 0)
        rb.fill(_rows(d["r"]))
        rs = (H * W * P, 1, W * P, P)
    consts = {k: d[k].to(dev).contiguous() for k in ("weight", "bias")}
    stats = torch.cat([d["mean"], d["rs"]]).to(dev).contiguous()
    sb = None
    if sum_mode == "separate":
        sb = Buf(dev, rows, C, C + 4, torch.float32)
    elif sum_mode == "nchw":
        sb = Buf(dev, 1, N * C * H * W, N * C * H * W, torch.float32)
    sum_ptr, lds = (xb.ptr, xb.ld) if sum_mode == "inplace" else ((sb.ptr, sb.ld) if sb is not None else (None, 0))
    ss = (C * H * W, H * W, W, 1) if sum_mode == "nchw" else (H * W * lds, 1, W * lds, lds)
    hy, hx = halo
    gb = Buf(dev, rows, R.packed_ld(C), R.packed_ld(C), torch.int32) if planes in ("sign", "both") else None
    prow = N * (H + 2 * hy) * (W + 2 * hx)
    nb = Buf(dev, prow, R.pixel_ld_nib(C), R.pixel_ld_nib(C), torch.int32) if planes in ("nib", "both") else None
    ht, lo, hi = (0, 0.0, 0.0) if hardtanh is None else (1, hardtanh[0], hardtanh[1])
    x_before = xb.live().clone()
    rc = getattr(lib, ENTRY)(xb.ptr, xb.ld, consts["weight"].data_ptr(), consts["bias"].data_ptr(), stats.data_ptr(), rb.ptr, *rs, ht,
                             lo, hi, sum_ptr, *ss, gb.ptr if gb else None, gb.ld if gb else 0, nb.ptr if nb else None,
                             nb.ld if nb else 0, hy, hx, N, C, H, W, ops._stream(dev))
    assert rc == OK, rc
    torch.cuda.synchronize()
    for b, what in ((xb, "x"), (rb, "residual"), (sb, "sum"), (gb, "sign plane"), (nb, "nibble plane")):
        if b is not None:
            b.assert_guards(what)
    assert bool(R.same_bits(rb.live(), _rows(d["r"]) if res_form != "nchw" else d["r"].reshape(1, -1)).all()), "the residual was written"
    out = {"sum": None}
    if sum_mode == "inplace":
        out["sum"] = xb.live()
    else:
        assert bool(R.same_bits(xb.live(), x_before).all()), "x was written although the sum goes elsewhere"
        if sb is not None:
            out["sum"] = sb.live() if sum_mode == "separate" else _rows(sb.live().view(N, C, H, W))
    out["sign"] = gb.view.cpu().numpy().view(np.uint32) if gb else None
    out["nib"] = nb.view.cpu().numpy().view(np.uint32) if nb else None
    return out


def _check(out, ref, shape, halo, designed, what):
    amb = ref["ambiguous"]
    n_amb = int(amb.sum())
    if designed:
        assert n_amb == 0, f"{what}: the designed class must not be ambiguous"
    assert n_amb <= R.waiver_cap(amb.numel()), f"{what}: {n_amb} ambiguous elements"
    if out["sum"] is not None:
        same = R.same_bits(out["sum"], _rows(ref["v"])) | _rows(amb)
        assert bool(same.all()), f"{what}: {int((~same).sum())} sum elements differ in their bits"
    if n_amb == 0:
        if out["sign"] is not None:
            assert np.array_equal(out["sign"], R.sign_plane(ref["neg"])), f"{what}: sign plane"
        if out["nib"] is not None:
            assert np.array_equal(out["nib"], R.nib_plane(ref["neg"], halo)), f"{what}: nibble plane"


@pytest.mark.parametrize("shape3", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("C", R.CHANNELS)
def test_entry_matches_the_exact_reference(dev, C, shape3):
    lib = _lib.load()
    shape = (shape3[0], C, shape3[1], shape3[2])
    for i, (res_form, sum_mode, planes, halo, hardtanh) in enumerate(R.combos(C, shape3)):
        seed = R.seed_of(C, shape3, i)
        what = f"C={C} {shape3} {res_form} sum={sum_mode} planes={planes} halo={halo} hardtanh={hardtanh}"
        for designed in (True, False):
            d = R.designed(shape, seed, hardtanh) if designed else R.realistic(shape, seed)
            ref = R.reference(d["x"], d["mean"], d["rs"], d["weight"], d["bias"], d["r"], hardtanh)
            out = _launch(lib, dev, d, shape, res_form, sum_mode, planes, halo, hardtanh, ldx_extra=4 if i % 2 else 0)
            _check(out, ref, shape, halo, designed, what + (" designed" if designed else " realistic"))
            if designed and d["fma_case"] and hardtanh is None and out["sum"] is not None:
                # the placed case: only a FUSED multiply-add leaves 2^-25 here (a separately rounded product leaves -2^-25)
                assert float(out["sum"][0, 1]) == 2.0 ** -25


def test_more_than_one_workgroup_per_form(dev):
    """The shapes of the matrix are a handful of workgroups.  5 x 64 x 30 x 30 is 4500 rows of 2 words: 282 tiles of the LDS form, 282
    workgroups of the row form, images that end inside a tile — every residual form, the sum in place and in NCHW storage."""
    lib = _lib.load()
    shape = (5, 64, 30, 30)
    d = R.realistic(shape, 77)
    ref = R.reference(d["x"], d["mean"], d["rs"], d["weight"], d["bias"], d["r"], (-1.0, 1.0))
    for res_form in R.RESIDUALS:
        for sum_mode in ("inplace", "nchw"):
            out = _launch(lib, dev, d, shape, res_form, sum_mode, "both", (1, 1), (-1.0, 1.0))
            _check(out, ref, shape, (1, 1), False, f"{res_form} sum={sum_mode}")


def _call(lib, **kw):
    P = 0x7f0000001000            # stands for a device pointer: every refused call returns before anything could read it
    a = dict(x=P, ldx=40, weight=P, bias=P, stats=P, r=P, rs=(1000, 25, 5, 1), ht=1, lo=-1.0, hi=1.0, sum=P + 0x100000, lds=40,
             sign=P + 0x200000, ldb=4, nib=P + 0x300000, ldn=8, hy=1, hx=1, N=2, C=40, H=5, W=5)
    a.update(kw)
    lds = a["lds"]
    ss = a.get("ss") or (a["H"] * a["W"] * lds, 1, a["W"] * lds, lds)          # the sum as rows with a pitch, unless ``ss`` says otherwise
    return getattr(lib, ENTRY)(a["x"], a["ldx"], a["weight"], a["bias"], a["stats"], a["r"], *a["rs"], a["ht"], a["lo"], a["hi"],
                               a["sum"], *ss, a["sign"], a["ldb"], a["nib"], a["ldn"], a["hy"], a["hx"], a["N"], a["C"], a["H"],
                               a["W"], None)


def test_every_validation_rule_returns_its_status_without_writing(dev):
    """The rules in the header's order, on REAL buffers full of sentinels: a refused call writes nothing."""
    lib = _lib.load()
    N, C, H, W = 2, 40, 5, 5
    rows = N * H * W
    bufs = {"x": Buf(dev, rows, C, C, torch.float32), "sum": Buf(dev, rows, C, C, torch.float32),
            "sign": Buf(dev, rows, 4, 4, torch.int32), "nib": Buf(dev, N * (H + 2) * (W + 2), 8, 8, torch.int32),
            "r": Buf(dev, rows, C, C, torch.float32), "c": Buf(dev, 1, 2 * C, 2 * C, torch.float32)}
    real = dict(x=bufs["x"].ptr, sum=bufs["sum"].ptr, sign=bufs["sign"].ptr, nib=bufs["nib"].ptr, r=bufs["r"].ptr,
                weight=bufs["c"].ptr, bias=bufs["c"].ptr, stats=bufs["c"].ptr)
    cl = (H * W * C, 1, W * C, C)

    def call(**kw):
        return _call(lib, **{**real, **kw})

    # 1. negative sizes and halos, before the empty-problem rule
    for k in ("N", "C", "H", "W", "hy", "hx"):
        assert call(**{k: -1}) == INVALID
    assert call(N=0, hy=-1) == INVALID
    # 2. empty problems: OK whatever the pointers are
    for k in ("N", "C", "H", "W"):
        assert call(**{k: 0}, x=None, r=None, weight=None, sum=None, sign=None, nib=None) == OK
    # 3. limits
    assert call(hy=65) == UNSUPPORTED and call(hx=65) == UNSUPPORTED
    assert call(N=1 << 20, H=1 << 6, W=1 << 5, rs=((1 << 11) * 40, 1 << 11, 1 << 5, 1)) == UNSUPPORTED          # 2^31 plane rows
    # 4. arguments
    for k in ("x", "weight", "bias", "stats", "r"):
        assert call(**{k: None}) == INVALID
    assert call(sum=None, sign=None, nib=None) == INVALID                                # no output at all
    assert call(ht=2) == INVALID and call(lo=1.0, hi=-1.0) == INVALID and call(lo=float("nan")) == INVALID
    assert call(ldx=39) == INVALID and call(lds=39) == INVALID
    assert call(rs=(1000, 25, 5, 2)) == INVALID and call(rs=(cl[0], 1, cl[2], 39)) == INVALID       # not dense; pitch below C
    assert call(rs=(cl[0] + 40, 1, cl[2], 40)) == INVALID
    assert call(ldb=3) == INVALID and call(ldn=4) == INVALID
    assert call(sum=real["x"] + 16) == INVALID and call(sum=real["x"], lds=44, ldx=40) == INVALID   # partial aliasing
    assert call(sum=real["x"] - 16) == INVALID
    nchw = (C * H * W, H * W, W, 1)
    assert call(ss=(1000, 25, 5, 2)) == INVALID and call(sum=real["x"], ss=nchw) == INVALID           # no dense form; NCHW over x
    # 5. alignment
    for k in ("x", "weight", "bias", "stats", "r", "sum", "sign"):
        assert call(**{k: real[k] + 2}) == ALIGNMENT
    assert call(nib=real["nib"] + 4) == ALIGNMENT and call(ldn=10) == ALIGNMENT
    # a plane that is not wanted is not validated
    assert call(sign=None, ldb=0, ldn=4) == INVALID and call(nib=None, ldn=0, ldb=3) == INVALID
    torch.cuda.synchronize()
    for name, b in bufs.items():
        b.assert_untouched(name)
    # ... and the same call with nothing wrong runs (in place, too)
    bufs["x"].fill(torch.ones(rows, C)), bufs["r"].fill(torch.zeros(rows, C)), bufs["c"].fill(torch.ones(1, 2 * C))
    assert call(rs=cl) == OK and call(rs=cl, sum=real["x"]) == OK
    torch.cuda.synchronize()
    assert bool((bufs["sum"].live() == 1.0).all()) and bool((bufs["x"].live() == 1.0).all())
    bufs["sum"].fill(torch.zeros(rows, C))
    assert call(ss=nchw) == OK
    torch.cuda.synchronize()
    assert bool((bufs["sum"].live() == 1.0).all())      # fma((1 - 1) * 1, 1, 1) + 0


# ---- ops.bn_add_sign ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C, shape3", [(20, (2, 3, 5)), (33, (3, 7, 7)), (64, (2, 14, 14))])
def test_ops_wrapper(dev, C, shape3):
    shape = (shape3[0], C, shape3[1], shape3[2])
    N, _, H, W = shape
    before = _lib.call_counts.get(ENTRY, 0)
    for i, (hardtanh, halo, layout) in enumerate(((None, None, "nchw"), ((-1.0, 1.0), (1, 1), "cl"), ((-0.5, 2.0), (2, 1), "strided"))):
        d = R.designed(shape, 5 + i, hardtanh)
        ref = R.reference(d["x"], d["mean"], d["rs"], d["weight"], d["bias"], d["r"], hardtanh)
        x2 = _rows(d["x"]).contiguous().to(dev)
        r = d["r"].to(dev)
        if layout == "cl":
            r = r.contiguous(memory_format=torch.channels_last)
        elif layout == "strided":
            r = torch.cat([d["r"], d["r"]], dim=3).to(dev)[..., :W]          # neither dense form: the wrapper copies it
        stats = torch.cat([d["mean"], d["rs"]]).to(dev)
        args = (d["weight"].to(dev), d["bias"].to(dev), stats, r)
        s_new, bits, nib = ops.bn_add_sign(x2, shape, *args, hardtanh=hardtanh, sum_out="new", out_halo=halo)
        assert s_new.data_ptr() != x2.data_ptr() and torch.equal(x2.cpu(), _rows(d["x"]))
        assert bool(R.same_bits(s_new.cpu(), _rows(ref["v"])).all())
        assert isinstance(bits, ops.BitPlanes) and (bits.rows, bits.K) == (N * H * W, C)
        assert np.array_equal(bits.sign.cpu().numpy().view(np.uint32), R.sign_plane(ref["neg"]))
        if halo is None:
            assert nib is None
        else:
            assert isinstance(nib, ops.NibPlanes) and nib.K == C
            assert np.array_equal(nib.words.cpu().numpy().view(np.uint32), R.nib_plane(ref["neg"], halo))
        s_in, bits2, _ = ops.bn_add_sign(x2, shape, *args, hardtanh=hardtanh)                     # in place, sign plane only
        assert s_in.data_ptr() == x2.data_ptr() and bool(R.same_bits(x2.cpu(), _rows(ref["v"])).all())
        assert torch.equal(bits2.sign, bits.sign)
        x3 = _rows(d["x"]).contiguous().to(dev)
        s_nchw, bits3, _ = ops.bn_add_sign(x3, shape, *args, hardtanh=hardtanh, sum_out="nchw")
        assert s_nchw.shape == shape and s_nchw.is_contiguous() and bool(R.same_bits(s_nchw.cpu(), ref["v"]).all())
        assert torch.equal(bits3.sign, bits.sign) and torch.equal(x3.cpu(), _rows(d["x"]))
    assert _lib.call_counts[ENTRY] == before + 9
    with pytest.raises(ValueError):
        ops.bn_add_sign(x2, shape, *args, sum_out=None, want_sign=False)                          # nothing to write
    with pytest.raises(ValueError):
        ops.bn_add_sign(x2, shape, args[0], args[1], args[2], r[:, :, :, :1])
    with pytest.raises(TypeError):
        ops.bn_add_sign(x2.cpu(), shape, *args)


# ---- layers.fused.FusedConvBnAddSign -----------------------------------------------------------------------------------------------

def _bn(c, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g) * 3)
        bn.running_var.copy_(torch.rand(c, generator=g) * 20 + 0.5)
        bn.weight.copy_(torch.randn(c, generator=g))
        bn.bias.copy_(torch.randn(c, generator=g))
    return bn


@pytest.mark.parametrize("conv_t, cin, cout, groups, hardtanh", [
    (BinConv2d, 16, 16, 1, None), (TerConv2d, 20, 20, 1, (-1.0, 1.0)), (BinConv2d, 16, 16, 16, (-1.0, 1.0)), (BinConv2d, 16, 16, 4, None)])
def test_block_equals_the_module_graph(dev, conv_t, cin, cout, groups, hardtanh):
    """conv -> BatchNorm2d -> + r -> [Hardtanh] -> BinaryConnect, module by module under lazy.eager(), against the block on the
    PackedActivation a fused producer hands over and on the fp32 +-1 tensor itself: the sum and the signs are torch.equal."""
    torch.manual_seed(3)
    conv = conv_t(cin, cout, 3, padding=1, groups=groups).to(dev).eval()
    bn = _bn(cout, 11).to(dev).eval()
    head = BinConv2d(cin, cin, 3, padding=1).to(dev).eval()
    head_bn = _bn(cin, 12).to(dev).eval()
    x0 = torch.randn(2, cin, 8, 8, device=dev)
    r = torch.randn(2, cout, 8, 8, device=dev)
    sign = BinaryConnect()
    with torch.no_grad(), lazy.eager():
        a = sign(head_bn(head(sign(x0))))
        s = bn(conv(a)) + r
        if hardtanh is not None:
            s = nn.functional.hardtanh(s, *hardtanh)
        want_sum, want_sign = s, sign(s)
        act = FusedConvPoolBnSign(head, head_bn, fold="device")(sign(x0))
    before = _lib.call_counts.get(ENTRY, 0)
    blk = FusedConvBnAddSign(conv, bn, hardtanh=hardtanh, fold="device")
    with torch.no_grad():
        for inp in (act, a):
            got, total = blk(inp, r)
            assert isinstance(got, packed.PackedActivation) and got.shape == (2, cout, 8, 8)
            assert torch.equal(total, want_sum)
            # the sum has the storage the module graph works in: NCHW behind the NCHW tensor, channels-last behind the planes
            assert total.is_contiguous() == (inp is a) and got.source_channels_last == (inp is not a)
            assert np.array_equal(got.planes.sign.cpu().numpy().view(np.uint32), R.sign_plane((want_sign < 0).cpu()))
        blk.out_nib_halo = (1, 1)
        got, total = blk(act, r.contiguous(memory_format=torch.channels_last))
        assert got.nib is not None and got.halo == (1, 1) and torch.equal(total, want_sum)
        neg = (want_sign < 0).cpu()
        assert np.array_equal(got.nib.words.cpu().numpy().view(np.uint32), R.nib_plane(neg, (1, 1)))
    assert _lib.call_counts[ENTRY] == before + 3


def test_block_declines_what_it_cannot_run(dev):
    from pytorch_quantize_impls_amd.layers import XNORConv2d
    bn = nn.BatchNorm2d(8)
    for conv, b, kw in ((BinConv2d(8, 8, 3, padding=1, deterministic=False), bn, {}),
                        (TerConv2d(8, 8, 3, padding=1, deterministic=False), bn, {}),
                        (XNORConv2d(8, 8, 3, padding=1), bn, {}),
                        (nn.Conv2d(8, 8, 3, padding=1), bn, {}),
                        (BinConv2d(8, 8, 3, padding=1), nn.MaxPool2d(2), {}),            # a pool in front of the BatchNorm
                        (BinConv2d(8, 8, 3, padding=1), nn.BatchNorm2d(4), {}),
                        (BinConv2d(8, 8, 3, padding=1).half(), bn, {}),
                        (BinConv2d(8, 8, 3, padding=1), bn, {"hardtanh": (0.5, 1.0)}),
                        (BinConv2d(8, 8, 3, padding=1), bn, {"fold": "reference"})):
        with pytest.raises(ValueError):
            FusedConvBnAddSign(conv, b, **kw)
    blk = FusedConvBnAddSign(BinConv2d(8, 8, 3, padding=1), bn).to(dev)
    x, r = torch.randn(1, 8, 4, 4, device=dev), torch.randn(1, 8, 4, 4, device=dev)
    with pytest.raises(RuntimeError):
        blk(x, r)                                                                        # training mode
    blk.eval()
    with pytest.raises(ValueError):
        blk(x.half(), r)
    with pytest.raises(ValueError):
        blk(x, r[:, :4])
    with pytest.raises(TypeError):
        blk(x.cpu(), r)
