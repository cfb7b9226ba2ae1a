"""What tests/test_gpu_gemm_routes.py relies on, without a device: the planes of tests/_gemm_exact.py round-trip to the integer
matrices they were built from, every pad unit is zero, every partial sum of every case is an integer below 2^24 (so the fp64
product is the only right answer), the tie cases are tie cases, and the shapes get the rungs they were chosen for."""
import ctypes

import pytest
import torch

import _gemm_exact as G
import _routes as R

ROWS = 384          # rows of the big operands whose fp64 product the per-case checks form (every row is a draw of one generator)


def _head(c):
    """The first ROWS rows of the case's operands; the bound of every partial sum is taken over ALL rows first."""
    x, w = G.operands(c)
    rng = {"fp4": 1, "i8": 127 * c.wmax, "bf16": 64, "f16": 64}[c.family]
    assert x.shape == (c.M, c.K) and w.shape == (c.N, c.K) and G.abs_bound(x, w) <= rng * c.K < G.EXACT
    return x[:ROWS], w[:ROWS]


CASES = G.all_dense_cases()


def test_case_names_are_unique_and_every_pair_has_a_case():
    names = [c.name for c in CASES] + [c.name for c in G.splitk_cases()]
    assert len(names) == len(set(names))
    pairs = {(c.rung, c.elem) for c in CASES if c.variant == 0}
    assert pairs == {(r, e) for r in G.AUTO_RUNGS for e in G.ELEMS} and len(pairs) == 66
    assert {c.rung for c in G.splitk_cases()} == {"PP256", "PP192", "PP128", "PP64"}
    assert set(G.VARIANTS.values()) <= set(R.CFG_ARGS)


@pytest.mark.parametrize("family,gen", [("fp4", "ternary"), ("fp4", "corr"), ("i8", "x"), ("i8", "w1"), ("i8", "w15"), ("bf16", "u"), ("f16", "u")])
@pytest.mark.parametrize("rows,K,ld", [(5, 26, 4), (70, 250, 32), (33, 61, 36), (9, 1017, 128)])
def test_planes_round_trip_and_pad_with_zeros(family, gen, rows, K, ld):
    K = min(K, G.PER_WORD[family] * ld)
    q = {"ternary": lambda: G.ternary(3, rows, K), "corr": lambda: G.correlated_pm1(3, rows, K, 5, 0.2),
         "x": lambda: G.uniform_ints(3, rows, K, -127, 127), "w1": lambda: G.uniform_ints(3, rows, K, -1, 1),
         "w15": lambda: G.uniform_ints(3, rows, K, -15, 15), "u": lambda: G.uniform_ints(3, rows, K, -8, 8)}[gen]()
    plane = G.make_plane(family, q, ld)
    assert plane.is_contiguous() and plane.shape[0] == rows and plane.shape[1] * plane.element_size() == 4 * ld
    val, raw = G.decode_plane(family, plane)
    assert torch.equal(val[:, :K], q) and not bool(raw[:, K:].any())
    # every row and every column has its own pattern: no two rows, no two columns agree
    assert len({tuple(r.tolist()) for r in q}) == rows
    if rows >= 33:
        assert len({tuple(col.tolist()) for col in q.t()}) == K


def test_nibble_codes_and_element_order():
    """+1 -> 0x2, -1 -> 0xA, 0 -> 0x0; element k is nibble k % 8 of word k / 8, little end first (tests/test_gpu_c2_pack.py _nib_ref)."""
    q = torch.tensor([[1, -1, 0, 1, 1, 0, -1, -1, -1, 1]])
    words = G.nib_plane(q, 4).view(torch.int32)[0].tolist()
    assert [w & 0xFFFFFFFF for w in words] == [0xAA0220A2, 0x0000002A, 0, 0]
    assert G.i8_plane(torch.tensor([[1, -2, 127]]), 4).view(torch.int32)[0, 0].item() & 0xFFFFFF == 0x7FFE01
    assert G.half_plane(torch.tensor([[1, -2]]), 4, torch.bfloat16).view(torch.int32)[0, 0].item() & 0xFFFFFFFF == 0xC0003F80
    assert G.half_plane(torch.tensor([[1, -2]]), 4, torch.float16).view(torch.int32)[0, 0].item() & 0xFFFFFFFF == 0xC0003C00


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_every_partial_sum_is_an_exact_integer(c):
    x, w = _head(c)
    assert x.shape[1] == w.shape[1] == c.K <= G.PER_WORD[c.family] * c.ld and c.ld % 4 == 0
    if c.family == "i8":        # max_abs_code is passed truthfully
        assert c.max_abs_code * c.K < G.EXACT and int(x.abs().max()) * int(w.abs().max()) <= c.max_abs_code
    s = x.double() @ w.double().t()
    assert G.abs_sum_max(x, w) <= G.abs_bound(x, w) and float(s.abs().max()) <= G.abs_sum_max(x, w)
    # the scale is a power of two and the scaled sum + an integer bias stays an fp32 integer or dyadic fraction: no rounding at all
    m, e = torch.frexp(torch.tensor(c.total_scale, dtype=torch.float64))
    assert float(m) == 0.5
    b = G.bias_of(c)
    if c.bias in (None, "int"):
        y64 = s * c.total_scale + (b[: w.shape[0]].double() if b is not None else 0)
        assert torch.equal(y64.float().double(), y64)
    vx, rx = G.decode_plane(c.family, G.make_plane(c.family, x, c.ld))
    assert torch.equal(vx[:, :c.K], x) and not bool(rx[:, c.K:].any())


def test_k_pairs_leave_a_tail_and_whole_zero_stages():
    assert G.k_pair("fp4", 32) == (250, 130) and G.k_pair("bf16", 32) == (61, 35) and G.k_pair("i8", 32) == (125, 70)
    for fam, per in G.PER_WORD.items():
        for ld in (4, 32, 36, 64, 128, 1152):
            k1, k2 = G.k_pair(fam, ld)
            bytes1, bytes2, cap = k1 * 4 / per, k2 * 4 / per, 4 * ld
            assert 0 < k2 < k1 < per * ld and cap - bytes1 < 16                  # the tail ends inside the row's last 16-byte chunk
            assert ld < 32 or (bytes2 % 64 != 0 and cap - bytes2 >= 56)          # ... and the short run leaves whole 64-byte stages zero


TIES = [c for c in CASES if G.is_tie_case(c)]


@pytest.mark.parametrize("c", TIES, ids=[c.name for c in TIES])
def test_bf16_tie_cases_are_tie_cases(c):
    """Found: 0.29 .. 0.34 of the outputs of every tie case are exact ties of bf16, with sums on both sides of 512 (spacing 2 and 4)."""
    x, w = _head(c)
    y32 = (x.double() @ w.double().t() + G.bias_of(c)[: w.shape[0]].double()).float()
    share = G.tie_share(y32, torch.bfloat16)
    a = y32.abs()
    print(f"{c.name}: tie share {share:.3f}, |sum + bias| {float(a.min()):.0f} .. {float(a.max()):.0f}")
    assert share >= 0.25
    assert float(((a > 256) & (a < 512)).float().mean()) > 0.1 and float((a > 512).float().mean()) > 0.1
    assert float((y32.to(torch.bfloat16).float() != y32).float().mean()) > 0.5          # most outputs round at all


def test_fp16_cases_reach_the_rounding_and_the_overflow():
    longk = [c for c in G.long_k_cases() if c.elem == "ElemFp4Out<2>"]
    assert len(longk) == 2
    for c in longk:
        x, w = _head(c)
        b = G.bias_of(c)
        y32 = (x.double() @ w.double().t() + (b[: w.shape[0]].double() if b is not None else 0)).float()
        a = y32.abs()
        share = G.tie_share(y32, torch.float16)
        print(f"{c.name}: fp16 tie share {share:.3f}, |sum| up to {float(a.max()):.0f}")
        # found: every |sum| above 3000; a quarter of them below 4096, where every odd sum is a tie (share 0.05 .. 0.08); 0.75 .. 1.0 of the outputs round
        # (an odd integer above 2048 is no fp16 number; the integer bias of the second case makes half of its columns even)
        assert c.K % 2 == 1 and float((a > 2048).float().mean()) > 0.9 and share >= 0.04
        assert float((y32.to(torch.float16).float() != y32).float().mean()) > 0.5
    over = [c for c in CASES if c.bias == "inf"]
    assert len(over) == 2
    for c in over:
        x, w = _head(c)
        y = G.expected(x.double() @ w.double().t(), c, G.bias_of(c)[: w.shape[0]])
        assert bool((y == float("inf")).any()) and bool((y == float("-inf")).any()) and bool(torch.isfinite(y).any())
    frac = [c for c in CASES if c.elem == "ElemFp4Out<2>" and c.bias == "frac" and c.kind == "corr"]
    for c in frac[:2]:
        x, w = _head(c)
        y32 = (x.double() @ w.double().t() + G.bias_of(c)[: w.shape[0]].double()).float()
        assert float((y32.to(torch.float16).float() != y32).float().mean()) > 0.9


def test_fractional_bias_adds_exactly_in_fp64_and_rounds_in_fp32():
    c = next(c for c in CASES if c.bias == "frac")
    b = G.bias_of(c)
    assert b.dtype == torch.float32 and float(b.abs().min()) >= 2.0 ** -20 and float(b.abs().max()) < 64
    x, w = _head(c)
    s = x.double() @ w.double().t()
    y64 = s + b[: w.shape[0]].double()                      # |sum| < 2^14, |bias| in [2^-20, 2^6) with 24 bits: < 53 bits in all
    assert torch.equal(y64 - s, b[: w.shape[0]].double().expand_as(s))
    assert float((y64.float().double() != y64).double().mean()) > 0.5


def test_sentinels_are_nans_no_kernel_writes():
    for dt, bits in G.SENTINEL.items():
        t = torch.tensor([bits], dtype=torch.int64).to(G.INT_VIEW[dt]).view(dt)
        assert bool(torch.isnan(t).all())
        canon = (torch.tensor([float("nan")]) + 1.0).to(dt).view(G.INT_VIEW[dt])
        assert int(canon) != int(t.view(G.INT_VIEW[dt]))


# ---- the shapes get the rungs they were chosen for (the selector runs without a device) -----------------------------------------

@pytest.fixture(scope="module")
def lib():
    from pytorch_quantize_impls_amd import _lib
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_shapes_get_their_rungs(lib):
    buf = ctypes.create_string_buffer(64)
    for c in CASES:
        assert lib.qt_gemm_tile_describe(0, c.variant, c.M, c.N, c.ld, c.ld, buf, 64) == 0 and buf.value.decode() == c.rung, (c.name, buf.value)
    for c in G.splitk_cases():
        assert lib.qt_gemm_tile_describe(2, 0, c.M, c.N, c.ld, c.ld, buf, 64) == 0 and buf.value.decode() == c.rung, (c.name, buf.value)
        assert c.kslice % 64 == 0 and (c.nslice - 1) * c.kslice < c.K < c.nslice * c.kslice and 127 * c.kslice * c.nslice < G.EXACT
        assert c.ldy % 4 == 0 and c.ldy > c.N and c.y_stride % 4 == 0 and c.y_stride > c.M * c.ldy
    for v, ld in G.REFUSALS:
        assert lib.qt_gemm_tile_describe(0, v, 1000, 130, ld, ld, buf, 64) == -2


def test_gemm_aliases_of_the_variants_are_in_the_route_table():
    for name, args in (("Cfg256_1", "2, 4, 4, 2, 1, 0, 128, 0, 1"), ("Cfg192_1", "4, 2, 2, 3, 1, 0, 128, 0, 1"), ("Cfg128_1", "2, 4, 4, 1, 1, 0, 128, 0, 1")):
        assert R.CFG_ARGS[name] == args
    k = "void (anonymous namespace)::mfma_gemm_kernel<(anonymous namespace)::GemmCfg<(anonymous namespace)::ElemFp4Out<1>, 2, 4, 4, 2, 1, 0, 128, 0, 1>, false>(...)"
    assert R.mfma_routes([k]) == {"Cfg256_1<ElemFp4Out<1>>"}
