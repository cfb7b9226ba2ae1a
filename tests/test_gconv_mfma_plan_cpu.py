"""The launch plans of the matrix-core grouped convs (csrc/gconv_mfma.hip gm_plan / gmw_plan, csrc/gconv_planes_mfma.hip gp_walk)
through qt_gmconv2d_describe / ``ops.grouped_mfma_plan``, swept over the whole window on the host: tiles, LDS, the patch bound, the
splits, the workspace, and the planes kernel's division-free pixel walk replayed against ``divmod``.  The models are in
tests/_gm_walks.py; so are the cases of tests/test_gpu_gconv_mfma_walks.py, whose properties are checked here without a GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import _gconv_exact as R
import _gm_walks as M
from pytorch_quantize_impls_amd import _lib, ops

OK, INVALID, UNSUPPORTED = 0, -1, -4
GEOMS = tuple(itertools.product((1, 3), (1, 2), (0, 1)))                           # (kernel, stride, padding)
GROUPS, BATCHES = (1, 3, 8, 9, 32, 128, 1024), (1, 2, 33, 256)
MAPS = ((1, 1), (7, 7), (14, 14), (28, 28), (56, 56), (5, 37), (3, 65), (1, 70), (64, 3), (9, 40), (8, 56), (8, 32), (17, 65))
FP32_OPS = ("forward", "grad_input", "grad_weight")


def _fits(hw, k, p):
    return min(hw) + 2 * p >= k


@pytest.mark.parametrize("op", FP32_OPS)
def test_fp32_plans_over_the_whole_window(op):
    """Tiles of at most 128 pixels and 32 columns that cover the map, LDS inside 64 KiB, a patch that holds the largest box any
    tile reads (boxes recomputed from the definition of the conv), 1 <= splits <= units, and the workspace of grad_weight."""
    seen, shrunk = set(), {"tr": [], "tc": []}
    for (ci, co), (k, s, p), (H, W) in itertools.product(itertools.product(M.CIN_G, M.COUT_G), GEOMS, MAPS):
        if not _fits((H, W), k, p):
            continue
        (Ho, Wo), (Hd, Wd) = M.out_hw(H, W, k, s, p, p), M.dest_map(op, H, W, k, s, p, p)
        first = None
        for G, N in itertools.product(GROUPS, BATCHES):
            if N * G * max(ci * H * W, co * Ho * Wo) >= 2 ** 31:                # the entries take tensors below 2^31 elements
                continue
            pl = M.plan(op, ci, co, G, N, H, W, k, s, p, p)
            case = (op, ci, co, k, s, p, H, W, G, N, pl)
            tile = {key: pl[key] for key in ("kernel", "TR", "TC", "tiles_r", "tiles_c", "npmax", "lds_bytes", "tr_shrunk", "tc_shrunk")}
            if first is None:                      # the tile is a function of the map and the channels, not of G and N
                first = tile
                assert 1 <= pl["TR"] and 1 <= pl["TC"] <= 32 and pl["TR"] * pl["TC"] <= 128, case
                assert pl["tiles_r"] * pl["TR"] >= Hd > (pl["tiles_r"] - 1) * pl["TR"], case
                assert pl["tiles_c"] * pl["TC"] >= Wd > (pl["tiles_c"] - 1) * pl["TC"], case
                assert pl["lds_bytes"] <= 64 * 1024, case
                assert pl["npmax"] >= M.largest_box(op, pl, H, W, k, s, p, p), case    # 0: a 1 x 1 kernel that only meets padding
                want = (k * k, ci // 8, co // 16) if op == "grad_weight" else (k * k, (co if op == "grad_input" else ci) // 8)
                assert pl["template"] == want and pl["block"] == 256, case
                seen.add(pl["kernel"])
                for axis in ("tr", "tc"):
                    if pl[axis + "_shrunk"]:
                        shrunk[axis].append((ci, co, k, s, p, H, W))
            assert tile == first, case
            cap = -(-1024 // G)
            assert pl["units"] == N * pl["tiles_r"] * pl["tiles_c"] and pl["grid"] == G * pl["splits"], case
            assert pl["splits"] == min(pl["units"], cap if op != "grad_weight" else min(cap, ops.GM_WGRAD_MAX_SPLITS)), case
            assert 1 <= pl["splits"] <= pl["units"], case
            if op == "grad_weight":
                floats = ops.grouped_mfma_grad_weight_work_floats((N, G * ci, H, W), (G * co, ci, k, k), s, p, 1, G)
                assert floats == pl["splits"] * G * (k * k * co * ci + co) and pl["gpix"] == -(-pl["TR"] * pl["TC"] // 32) * 32, case
    assert len(seen) == (18 if op == "grad_weight" else 6), sorted(seen)
    # The budget loop takes rows on the maps of real ResNeXt stages, and columns in forward and grad_input.  gmw_plan never takes
    # a column: its largest one-row tile (32 columns, 3 x 3, stride 2, 32 -> 48) needs 62416 of the 65536 bytes.
    assert any(c[-1] >= 28 for c in shrunk["tr"]) and bool(shrunk["tc"]) == (op != "grad_weight"), (op, len(shrunk["tr"]), shrunk["tc"])
    print(op, "tile rows taken by the budget on", len(shrunk["tr"]), "shapes, columns on", len(shrunk["tc"]), "e.g.", shrunk["tc"][:3])


def test_planes_walk_equals_divmod_on_every_step_of_every_wave():
    seen, walks = set(), set()
    for (ci, co), (k, s, p), (H, W) in itertools.product(itertools.product(M.PLANES_CIN_G, M.COUT_G), GEOMS, MAPS):
        if not _fits((H, W), k, p):
            continue
        Ho, Wo = M.out_hw(H, W, k, s, p, p)
        for G, N in itertools.product(GROUPS, BATCHES):
            if N * G * max(ci * H * W, co * Ho * Wo) >= 2 ** 31:
                continue
            pl = M.plan("planes", ci, co, G, N, H, W, k, s, p, p)
            case = (ci, co, k, s, p, H, W, G, N, pl)
            npix = N * Ho * Wo
            step = 16 * pl["splits"]
            assert pl["template"] == (k * k, ci // 16, co // 16) and pl["units"] == -(-npix // 16), case
            assert pl["splits"] == max(1, min(pl["units"], 4096 // G)) and pl["grid"] == -(-G * pl["splits"] // 4), case
            assert (pl["d_n"], pl["d_ho"], pl["d_wo"]) == (step // (Ho * Wo), step // Wo % Ho, step % Wo), case
            seen.add(pl["kernel"])
            walks.add((N, Ho, Wo, pl["units"], pl["splits"], pl["d_n"], pl["d_ho"], pl["d_wo"]))
    assert len(seen) == 12, sorted(seen)
    for N, Ho, Wo, units, splits, d_n, d_ho, d_wo in sorted(walks):              # the walk knows neither channels nor taps
        pl = dict(units=units, splits=splits, d_n=d_n, d_ho=d_ho, d_wo=d_wo)
        covered = []
        for flat, inside, (rn, rho, rwo) in M.walk(N, Ho, Wo, pl):
            n, r = np.divmod(flat, Ho * Wo)
            ho, wo = np.divmod(r, Wo)
            assert (rn[inside] == n[inside]).all() and (rho[inside] == ho[inside]).all() and (rwo[inside] == wo[inside]).all(), pl
            covered.append(flat[inside])
        assert np.array_equal(np.sort(np.concatenate(covered)), np.arange(N * Ho * Wo)), pl      # every output pixel once


def test_gpu_cases_hold_the_property_each_exists_for():
    for c in M.WALKS:
        assert M.multi_unit("forward", c) and M.multi_unit("grad_input", c), c
    assert {c[2][1] for c in M.WALKS} == {1, 2} and any(c[0][0] == 24 for c in M.WALKS)
    assert {c[4][0] for c in M.WALKS} == {c[4][1] for c in M.WALKS} == {"nchw", "channels_last"}
    for op in FP32_OPS:                                                          # every workgroup meets tiles of two shapes
        for c in M.WALKS + (M.WGRAD_WALK,):
            assert all(len({t[:2] for t in w}) >= 2 and len({t[2:] for t in w}) >= 2 for w in M.unit_walks(op, c)), (op, c)
    assert M.multi_unit("grad_weight", M.WGRAD_WALK) and M.fp32_plan("grad_weight", M.WGRAD_WALK)["kernel"] != "gmw_kernel<9,2,1>"
    for op, c in M.SHRINK_ROWS.items():
        assert M.fp32_plan(op, c)["tr_shrunk"] > 0 and M.dest_map(op, *c[3], *c[2], c[2][2])[1] >= 28, (op, c)
    for op, c in M.SHRINK_COLS.items():
        assert M.fp32_plan(op, c)["tc_shrunk"] > 0, (op, c)
    assert len(M.PAIRS_LEFT) == 6 and len(M.INSTANCES) == 12 and len(M.WGRAD_INSTANCES) == 18
    assert len({M.fp32_plan("grad_weight", c)["kernel"] for c in M.WGRAD_INSTANCES}) == 18
    assert {M.planes_plan(c)["template"] for c in M.PLANES_INSTANCES} == {(1, 1, 1), (1, 1, 3), (1, 2, 2), (1, 2, 1), (9, 2, 1)}


@pytest.mark.parametrize("c", M.PLANES_WALKS, ids=lambda c: "g{0}i{1}o{2}N{3}-{4}x{5}".format(*c))
def test_planes_walk_cases_would_catch_a_dropped_carry_or_term(c):
    """On the walk model: every wave takes at least two steps and some three, all increments are non-zero, both carries fire on
    pixels inside the image, the last tile is partial — and the walk without either carry or any one term visits other pixels."""
    G, _ci, _co, N, H, W, k, s, (ph, pw) = c
    Ho, Wo = M.out_hw(H, W, k, s, ph, pw)
    pl = M.planes_plan(c)
    least, most, carry_wo, carry_ho = M.walk_facts(N, Ho, Wo, pl)
    assert least >= 2 and most >= 3 and min(pl["d_n"], pl["d_ho"], pl["d_wo"]) > 0 and carry_wo and carry_ho, (pl, least, most)
    assert N * Ho * Wo % 16 != 0 and pl["units"] >= 2 * pl["splits"] + 1
    good = M.visited(N, Ho, Wo, pl)
    for name in M.MUTANTS:
        assert not np.array_equal(M.visited(N, Ho, Wo, pl, without=name), good), name
    assert any(case[0] % 4 for case in M.PLANES_WALKS)


def test_the_issue_shapes_give_the_plans_they_were_chosen_for():
    pl = M.plan("forward", 16, 16, 128, 3, 9, 40, 3, 1, 1, 1)
    assert (pl["tiles_r"], pl["tiles_c"], pl["units"], pl["splits"]) == (2, 2, 12, 8)
    # ... but that shape is no walk case: 12 units are fewer than 2 * 8 + 1, and 8 splits over the 4 tiles of an image give every
    # workgroup the same tile of another image, so no tile follows one of another shape.  M.WALKS steps by 7 or 9 instead.
    issue = ((16, 16), 128, (3, 1, 1), (9, 40), M.LAYOUTS[0], "binary", 3)
    assert not M.multi_unit("forward", issue) and all(len(set(w)) == 1 for w in M.unit_walks("forward", issue))
    pl = M.planes_plan((128, 16, 16, 50, 5, 5, 1, 1, (0, 0)))
    assert (pl["units"], pl["splits"], pl["d_n"], pl["d_ho"], pl["d_wo"]) == (79, 32, 20, 2, 2)
    pl = M.planes_plan((256, 16, 16, 23, 5, 5, 1, 1, (0, 0)))
    assert (pl["d_n"], pl["d_ho"], pl["d_wo"]) == (10, 1, 1)


def test_describe_entry_returns_the_status_of_the_entry_it_stands_for():
    lib, buf = _lib.load(), ctypes.create_string_buffer(384)
    geo = (2, 8, 16, 32, 5, 5, 3, 3, 1, 1, 1, 1, 1, 1)
    call = lambda op, g=geo, out=buf, cap=384: lib.qt_gmconv2d_describe(op, *g, out, cap)          # noqa: E731
    edit = lambda **kw: tuple(kw.get(name, v) for name, v in zip(("N", "G", "cin_g", "cout_g", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw"), geo))   # noqa: E731
    for op in range(4):
        assert call(op) == OK and buf.value.startswith(b"kernel=g")
        assert call(op, out=None) == INVALID and call(op, cap=1) == INVALID
        assert call(op, edit(N=-1, cin_g=20)) == INVALID and call(op, edit(kh=5, kw=10)) == UNSUPPORTED
        assert call(op, edit(N=0, cin_g=20)) == OK and buf.value == b""                    # an empty problem: nothing to say
        assert call(op, edit(cin_g=8)) == UNSUPPORTED and call(op, edit(cout_g=64)) == UNSUPPORTED and call(op, edit(sh=2)) == UNSUPPORTED
        assert call(op, edit(H=1, W=1, ph=0, pw=0)) == INVALID                             # the kernel does not fit
        assert call(op, edit(cin_g=24)) == (UNSUPPORTED if op == 3 else OK)
        assert call(op, cap=16) == OK and len(buf.value) == 15                             # truncated, terminated
    assert call(4) == INVALID and call(-1) == INVALID
    with pytest.raises(ValueError):
        ops.grouped_mfma_plan("backward", (2, 128, 5, 5), (256, 16, 3, 3), 1, 1, 1, 8)
    with pytest.raises(ValueError):
        ops.grouped_mfma_plan("forward", (2, 128, 5, 5), (256, 16, 3, 3), 1, 1, 1, 4)
    with pytest.raises(_lib.QtStatusError):
        ops.grouped_mfma_plan("planes", (2, 192, 5, 5), (256, 24, 3, 3), 1, 1, 1, 8)
    assert ops.grouped_mfma_plan("forward", (0, 128, 5, 5), (256, 16, 3, 3), 1, 1, 1, 8) == {}


def test_matrix_product_references_equal_the_pinned_ones_on_integers():
    """tests/_gm_walks.py's float64 references (used where the channels run into the thousands) against tests/_gconv_exact.py's."""
    for i, (G, ci, co, k, s, p, hw) in enumerate(((3, 16, 32, 3, 2, 1, (6, 7)), (2, 24, 16, 1, 2, 0, (5, 4)), (2, 32, 48, 3, 1, 0, (4, 5)))):
        xs, ws = (2, G * ci) + hw, (G * co, ci, k, k)
        x, wq, b = R.small_ints(i, xs), R.quantize(R.weights(10 + i, ws), "ternary"), R.small_ints(20 + i, (G * co,))
        y = R.forward(x, wq, b, G, k, s, p, 1, dtype=np.float64)
        go = R.small_ints(30 + i, y.shape)
        assert np.array_equal(M.forward64(x, wq, b, G, k, s, p, p), y)
        assert np.array_equal(M.grad_input64(go, wq, xs, G, k, s, p, p), R.grad_input(go, wq, xs, G, k, s, p, 1, dtype=np.float64))
        gw, _ab, gb = R.grad_weight(x, go, G, ci, k, s, p, 1)
        gw2, gb2 = M.grad_weight64(x, go, G, ci, k, s, p, p)
        assert np.array_equal(gw2, gw) and np.array_equal(gb2, gb)
