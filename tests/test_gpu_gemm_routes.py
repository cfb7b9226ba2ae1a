"""Every matrix-core GEMM family (csrc/mfma_gemm_kernel.h through csrc/mfma_gemm.hip) on every tile configuration its selector can
pick, against exact sums.

  (a) the dense entry points — qt_nib_gemm (ElemFp4), qt_nib_gemm_h (ElemFp4Out<1> / <2>: bf16 / fp16 results), qt_bf16_gemm,
      qt_f16_gemm, qt_i8_gemm — on the eleven configurations of launch_gemm_auto, M, N and K all off the tile grid, each shape at a
      K a few elements short of the row stride and at about half of it; long K on the skinny rungs;
  (b) the half epilogue's two store paths on a wide and on a skinny tile, with sums that round (bf16 ties, fp16 above 2048, fp16
      overflow), and the fp32 epilogue's dwordx4 path; NaN in the bias;
  (c) the explicit variants of qt_nib_gemm_variant, and what 30 / 31 refuse;
  (d) qt_i8_gemm_splitk on every configuration of select_gemm_batched(M, N, false), slice by slice.

The operand planes are built in torch from integer matrices (tests/_gemm_exact.py: no packer of the project is on the path) and the
entry points are called through _lib.call.  Every partial sum is an integer below 2^24 (tests/test_gemm_exact_cpu.py), so the fp64
product is the only right answer: every comparison is torch.equal.  Y is a view into a larger buffer of sentinels, with ldy > N and
spare rows: after the call every element outside [0, M) x [0, N) still holds the sentinel and none inside does.  Each case asks the
describe entry point which configuration its shape gets, asserts that this is the rung the case was written for, runs under
torch.profiler and asserts that exactly one mfma_gemm_kernel instance ran, with that alias and element class.

Run the whole module: the coverage test reads what the cases before it pinned."""
import ctypes
import time

import pytest
import torch

import _gemm_exact as G
import _routes as R

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib  # noqa: E402

PINNED = {}                 # "Alias<Element>" -> case names whose profiler trace named it (dense entry points, variant 0)
PINNED_VARIANTS = {}
PINNED_SPLITK = {}
PEAK = {}
TOTALS = {"cases": 0, "elements": 0, "t0": None}
QT_DTYPE = {torch.bfloat16: 1, torch.float16: 2}
SPARE_ROWS, TAIL = 3, 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    if TOTALS["t0"] is None:
        TOTALS["t0"] = time.time()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    PEAK[request.node.name] = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def describe(family, variant, M, N, ld):
    buf = ctypes.create_string_buffer(64)
    rc = _lib.load().qt_gemm_tile_describe(family, variant, M, N, ld, ld, buf, 64)
    return rc, buf.value.decode()


def tile_text(alias):
    """GemmCfg alias -> the tile text of qt_nib_gemm_describe, from the configuration's numbers."""
    wm, wn, tmw, tnw, pipe, _, sb = next(t for t, n in R.GEMM_CFG.items() if n == alias)[:7]
    stages = f"{sb}-byte stages, " if sb != (64 if pipe == 2 else 128) else ""
    return f"{32 * wm * tmw}x{32 * wn * tnw}, {stages}pipe={pipe}{' (ping-pong)' if pipe == 2 else ''}"


def traced(fn, label, case):
    """fn under torch.profiler: exactly one mfma_gemm_kernel instance ran, and it is ``label`` ('PP256<ElemI8>')."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    ran = [k for k in names if "mfma_gemm_kernel" in k]
    assert len(ran) == 1 and R.mfma_routes(ran) == {label}, (case, label, ran)


class Result:
    """A result matrix as a view into a buffer of sentinels: ``off`` elements in front, ldy > N, SPARE_ROWS rows below M, TAIL after."""

    def __init__(self, dtype, M, N, ldy, off, dev, planes=1, stride=None):
        self.dtype, self.M, self.N, self.ldy, self.off, self.planes = dtype, M, N, ldy, off, planes
        self.stride = (M + SPARE_ROWS) * ldy if stride is None else stride
        self.bits = torch.full((off + planes * self.stride + TAIL,), G.SENTINEL[dtype], dtype=G.INT_VIEW[dtype], device=dev)
        self.ptr = self.bits.data_ptr() + off * self.bits.element_size()

    def plane(self, z=0):
        """[M, N] of plane z, as the result dtype."""
        lo = self.off + z * self.stride
        return self.bits[lo:lo + self.M * self.ldy].view(self.M, self.ldy)[:, :self.N].view(self.dtype)

    def untouched(self):
        return bool((self.bits == G.SENTINEL[self.dtype]).all())

    def check_sentinels(self, case):
        """Every element outside the planes' [0, M) x [0, N) still holds the sentinel, and no element inside does."""
        sent = G.SENTINEL[self.dtype]
        inside = 0
        for z in range(self.planes):
            hit = self.plane(z).view(G.INT_VIEW[self.dtype]) == sent
            if bool(hit.any()):
                r, col = (int(v) for v in hit.nonzero()[0])
                raise AssertionError((case, "element never written", "plane", z, "row", r, "column", col, "of", int(hit.sum())))
            inside += self.M * self.N
        kept = int((self.bits == sent).sum())
        if kept != self.bits.numel() - inside:
            mask = self.bits != sent
            for z in range(self.planes):
                lo = self.off + z * self.stride
                mask[lo:lo + self.M * self.ldy].view(self.M, self.ldy)[:, :self.N] = False
            i = int(mask.nonzero()[0]) - self.off
            z, rem = divmod(i, self.stride) if i >= 0 else (-1, i)
            raise AssertionError((case, "store outside the result", "plane", z, "row", rem // self.ldy, "column", rem % self.ldy,
                                  "elements", int(mask.sum())))


def assert_same(got, want, case, tile=None):
    """torch.equal with NaN == NaN; on a mismatch the first wrong (row, column), how many, and the extent of the wrong region."""
    assert got.shape == want.shape and got.dtype == want.dtype, (case, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn) | (~wn & (got != want))
    if bool(bad.any()):
        idx = bad.nonzero()
        r, col = (int(v) for v in idx[0])
        rows, cols = idx[:, 0], idx[:, 1]
        raise AssertionError((case, "first wrong (row, column)", (r, col), "got", float(got[r, col]), "want", float(want[r, col]),
                              "wrong elements", int(bad.sum()), "rows", (int(rows.min()), int(rows.max())),
                              "columns", (int(cols.min()), int(cols.max())), "tile", tile))
    TOTALS["elements"] += got.numel()


def launch_dense(c, xp, wp, bias, scale_dev, res):
    args_xw = (xp.data_ptr(), c.ld, wp.data_ptr(), c.ld)
    b = bias.data_ptr() if bias is not None else None
    sd = scale_dev.data_ptr() if scale_dev is not None else None
    tail = (res.ldy, c.M, c.N, c.K, _stream())
    if c.elem == "ElemFp4":
        if c.variant:
            _lib.call("qt_nib_gemm_variant", c.variant, *args_xw, b, res.ptr, *tail)
        else:
            _lib.call("qt_nib_gemm", *args_xw, b, res.ptr, *tail)
    elif c.elem in G.OUT_DTYPE:
        _lib.call("qt_nib_gemm_h", *args_xw, b, res.ptr, QT_DTYPE[c.out_dtype], *tail)
    elif c.elem == "ElemBf16":
        _lib.call("qt_bf16_gemm", *args_xw, b, res.ptr, *tail)
    elif c.elem == "ElemF16":
        _lib.call("qt_f16_gemm", *args_xw, b, c.scale[0], sd, res.ptr, *tail)
    else:
        _lib.call("qt_i8_gemm", *args_xw, b, c.scale[0], sd, c.max_abs_code, res.ptr, *tail)


def run_dense(dev, c, pinned):
    rc, alias = describe(0, c.variant, c.M, c.N, c.ld)
    assert rc == 0 and alias == c.rung, (c.name, "described", rc, alias, "written for", c.rung)
    if c.elem == "ElemFp4" and not c.variant:
        buf = ctypes.create_string_buffer(128)
        assert _lib.load().qt_nib_gemm_describe(c.M, c.N, c.K, c.ld, c.ld, buf, 128) == 0
        assert buf.value.decode() == f"mfma_gemm_kernel<ElemFp4, {tile_text(alias)}>", (c.name, buf.value)
    label = f"{alias}<{c.elem}>"
    xq, wq = G.operands(c)
    xp, wp = G.make_plane(c.family, xq, c.ld).to(dev), G.make_plane(c.family, wq, c.ld).to(dev)
    bias = G.bias_of(c)
    bias_d = bias.to(dev) if bias is not None else None
    scale_dev = torch.tensor([c.scale[1]], dtype=torch.float32, device=dev) if c.scale[1] is not None else None
    res = Result(c.out_dtype, c.M, c.N, c.ldy, c.y[1], dev)
    traced(lambda: launch_dense(c, xp, wp, bias_d, scale_dev, res), label, c.name)
    res.check_sentinels(c.name)
    s = xq.to(dev).double() @ wq.to(dev).double().t()                  # integers below 2^24: exact in any order
    if c.out_dtype is not torch.float32 or c.bias == "frac":
        # the roundings on the CPU: fl32(sum + bias), then .to(dtype)
        want, got = G.expected(s.to(torch.int32).cpu().double(), c, bias), res.plane().cpu()
    else:
        want, got = G.expected(s, c, bias_d), res.plane()
    assert_same(got, want, c.name, R.tile_of(alias))
    if c.bias == "nan":
        cols = torch.isnan(got).all(0).nonzero().flatten().tolist()
        assert cols == G.nan_columns(c.N) and int(torch.isnan(got).sum()) == c.M * len(cols), (c.name, cols)
    if c.bias == "inf":
        assert bool(torch.isinf(got).any()) and bool(torch.isfinite(got).any())
    pinned.setdefault(label, []).append(c.name)
    TOTALS["cases"] += 1


# ---- (a) the dense rungs --------------------------------------------------------------------------------------------------------

DENSE = G.dense_cases()
LONG_K = G.long_k_cases()
STORE = G.store_path_cases()
SPECIAL = G.special_cases()
VARIANT = G.variant_cases()
SPLITK = G.splitk_cases()


@pytest.mark.parametrize("c", DENSE, ids=[c.name for c in DENSE])
def test_dense_rung_computes_the_exact_product(dev, c):
    run_dense(dev, c, PINNED)


@pytest.mark.parametrize("c", LONG_K, ids=[c.name for c in LONG_K])
def test_long_k_on_the_skinny_rungs(dev, c):
    run_dense(dev, c, PINNED)


# ---- (b) store paths, roundings, NaN and overflow -------------------------------------------------------------------------------

@pytest.mark.parametrize("c", STORE, ids=[c.name for c in STORE])
def test_store_paths_and_roundings(dev, c):
    wide = c.N % 8 == 0 and c.ldy % 8 == 0 and c.y[1] == 0
    if c.elem in G.OUT_DTYPE:
        assert wide == ("store wide" in c.name)                 # the 16-byte path exactly where the case says so
    else:
        assert c.N % 4 == 0 and c.ldy % 4 == 0
    run_dense(dev, c, PINNED)


@pytest.mark.parametrize("c", SPECIAL, ids=[c.name for c in SPECIAL])
def test_nan_bias_and_fp16_overflow(dev, c):
    run_dense(dev, c, PINNED)


# ---- (c) the explicit variants --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", VARIANT, ids=[c.name for c in VARIANT])
def test_explicit_variant_computes_the_exact_product(dev, c):
    assert G.VARIANTS[c.variant] == c.rung
    run_dense(dev, c, PINNED_VARIANTS)


@pytest.mark.parametrize("variant,ld", G.REFUSALS)
def test_skinny_variants_refuse_strides_they_cannot_take(dev, variant, ld):
    M, N, K = 1000, 130, 8 * ld - 6
    assert describe(0, variant, M, N, ld)[0] == -2
    c = G.Case(f"refusal {variant} ld{ld}", "ElemFp4", "", M, N, ld, K)
    xq, wq = G.operands(c)
    xp, wp = G.nib_plane(xq, ld).to(dev), G.nib_plane(wq, ld).to(dev)
    res = Result(torch.float32, M, N, N + 3, 0, dev)
    rc = _lib.load().qt_nib_gemm_variant(variant, xp.data_ptr(), ld, wp.data_ptr(), ld, None, res.ptr, res.ldy, M, N, K, _stream())
    torch.cuda.synchronize()
    assert rc == -2 and res.untouched()                          # QT_ERR_ALIGNMENT, nothing launched


# ---- (d) the batched family: qt_i8_gemm_splitk ----------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SPLITK, ids=[c.name for c in SPLITK])
def test_splitk_slices_are_exact_and_stay_inside_their_planes(dev, c):
    rc, alias = describe(2, 0, c.M, c.N, c.ld)
    assert rc == 0 and alias == c.rung, (c.name, rc, alias)
    label = f"{alias}<ElemI8>"
    xq, wq = G.splitk_operands(c)
    xp, wp = G.i8_plane(xq, c.ld).to(dev), G.i8_plane(wq, c.ld).to(dev)
    res = Result(torch.float32, c.M, c.N, c.ldy, 0, dev, planes=c.nslice, stride=c.y_stride)
    traced(lambda: _lib.call("qt_i8_gemm_splitk", xp.data_ptr(), c.ld, wp.data_ptr(), c.ld, res.ptr, c.ldy, c.M, c.N, c.kslice, c.nslice,
                             c.y_stride, _stream()), label, c.name)
    res.check_sentinels(c.name)                  # pad columns, rows past M, the gap between M * ldy and y_stride, the tail
    xd, wd = xq.to(dev).double(), wq.to(dev).double()
    total = torch.zeros((c.M, c.N), dtype=torch.float64, device=dev)
    for z in range(c.nslice):                    # every slice holds the product of ITS byte range
        k0, k1 = z * c.kslice, min(c.K, (z + 1) * c.kslice)
        assert k1 > k0
        assert_same(res.plane(z), (xd[:, k0:k1] @ wd[:, k0:k1].t()).float(), f"{c.name} slice {z}", R.tile_of(alias))
        total += res.plane(z).double()
    assert torch.equal(total, xd @ wd.t())       # the slices sum to the whole product
    PINNED_SPLITK.setdefault(label, []).append(c.name)
    TOTALS["cases"] += 1


# ---- coverage -------------------------------------------------------------------------------------------------------------------

def test_every_gemm_configuration_ran_against_the_exact_product():
    if not PINNED:
        pytest.skip("run the whole module: the cases above record the configurations the profiler named")
    want = {f"{r}<{e}>" for r in G.AUTO_RUNGS for e in G.ELEMS}
    assert len(want) == 66
    lines = [f"{k}: {len(PINNED.get(k, []))} cases" for k in sorted(want)]
    lines += [f"variant {v} {a}<ElemFp4>: {len(PINNED_VARIANTS.get(f'{a}<ElemFp4>', []))} cases" for v, a in sorted(G.VARIANTS.items())]
    lines += [f"split-K {k}: {len(v)} cases" for k, v in sorted(PINNED_SPLITK.items())]
    print("\n".join(["GEMM configurations pinned by profiler name:"] + lines))
    wall = time.time() - TOTALS["t0"] if TOTALS["t0"] else float("nan")
    print(f"cases {TOTALS['cases']}, elements compared {TOTALS['elements']}, wall {wall:.1f} s, peak device memory "
          f"{max(PEAK.values()) / 2**30:.2f} GiB ({max(PEAK, key=PEAK.get)})")
    assert set(PINNED) == want, (sorted(want - set(PINNED)), sorted(set(PINNED) - want))
    assert set(PINNED_VARIANTS) == {f"{a}<ElemFp4>" for a in G.VARIANTS.values()}
    # select_gemm_batched(M, N, false) has four outcomes; launch_gemm_batched refuses the fifth (the 384-row tile) for int8
    assert set(PINNED_SPLITK) == {f"{a}<ElemI8>" for a in ("PP256", "PP192", "PP128", "PP64")}
