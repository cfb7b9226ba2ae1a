"""The matrix-core grouped convs (csrc/gconv_mfma.hip, csrc/gconv_planes_mfma.hip) where the other three GPU modules do not reach:
workgroups and waves that walk several tiles of different shapes, tiles the LDS budget shrank, every template instantiation.  Every
comparison is exact — designed integers against float64 sums below 2^24 for the fp32 kernels, +-1 inputs bit for bit for the planes
kernel — and every output lies between sentinels.  Each case first asserts, from ``ops.grouped_mfma_plan``, the property it exists
for, so a retuned plan fails here instead of leaving the case blind.  Cases and models: tests/_gm_walks.py (checked on the host by
tests/test_gconv_mfma_plan_cpu.py); runners, generators and packers: the three modules and tests/_gconv_exact.py, tests/_dw_planes.py."""
import functools

import numpy as np
import pytest

import _dw_planes as P
import _gconv_exact as R
import _gm_walks as M
import test_gpu_gconv_mfma as F
import test_gpu_gconv_mfma_wgrad as W
import test_gpu_gconv_planes_mfma as PL
from pytorch_quantize_impls_amd import _lib, ops

pytestmark = pytest.mark.gpu

dev = F.dev                                                              # the forward module's device fixture
# What the tests of this module compared, filled as they run IN THIS PROCESS: the last test prints it and asserts that nothing
# differed.  Run alone, or with the module spread over several workers, that test sees a partial (or empty) tally; each test
# asserts its own comparisons, and the instantiation counts of the last test come from the plan, not from this record.
TALLY = dict(tests=0, comparisons=0, elements=0, differing=0, waived=0)


def _differing(got, want):
    """Elements of ``got`` that are not the reference's, counted into the tally."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = int((got != want).sum())
    TALLY["comparisons"] += 1
    TALLY["elements"] += got.size
    TALLY["differing"] += bad
    return bad


def _id(c):
    return "i{0[0]}o{0[1]}g{1}-k{2[0]}s{2[1]}p{2[2]}-{3[0]}x{3[1]}-{4[0]}-{4[1]}-{5}-N{6}".format(*c)


def _shapes(c):
    (ci, co), G, (k, s, p), (H, W), _lay, _kind, N = c
    Ho, Wo = M.out_hw(H, W, k, s, p, p)
    return (N, G * ci, H, W), (G * co, ci, k, k), (N, G * co, Ho, Wo)


# ---- forward and grad_input ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(c):
    """Designed integers of case c and the float64 results with their sums of magnitudes: (x, go, w, b, y, |y|, gx, |gx|)."""
    xs, ws, ys = _shapes(c)
    seed = sum(ws) + 7 * xs[3]
    x, go = F._spiked(seed, xs), F._spiked(seed + 1, ys)
    w = R.grid_weights(seed + 2, ws) if c[5] == "raw" else R.weights(seed + 2, ws)
    b = R.small_ints(seed + 3, (ws[0],))
    wq = R.quantize(w, c[5])
    G, (k, s, p) = c[1], c[2]
    return (x, go, w, b, M.forward64(x, wq, b, G, k, s, p, p), M.forward64(np.abs(x), np.abs(wq), np.abs(b), G, k, s, p, p),
            M.grad_input64(go, wq, xs, G, k, s, p, p), M.grad_input64(np.abs(go), np.abs(wq), xs, G, k, s, p, p))


def _forward_and_grad_input(dev, c):
    x, go, w, b, y64, ya, g64, ga = _reference(c)
    assert ya.max() < 2 ** 24 and ga.max() < 2 ** 24            # from the reference alone: every partial sum is an exact integer
    (k, s, p), lay, kind, G = c[2], c[4], c[5], c[1]
    xs, _ws, ys = _shapes(c)
    by, oy = F._guarded(dev, ys, lay[1])
    bx, ox = F._guarded(dev, xs, lay[0])
    wd = F._to(dev, w)
    calls = dict(_lib.call_counts)
    y = ops.grouped_mfma_conv2d(F._to(dev, x, lay[0]), wd, F._to(dev, b), s, p, 1, G, kind=kind, out=oy)
    gx = ops.grouped_mfma_conv2d_grad_input(xs, wd, F._to(dev, go, lay[1]), s, p, 1, G, kind=kind, out=ox)
    assert (F._used(calls).get(F.FWD), F._used(calls).get(F.GIN)) == (1, 1)
    for buf in (by, bx):
        assert bool((buf[:F.PAD] == F.SENTINEL).all() and (buf[-F.PAD:] == F.SENTINEL).all())
    bad = _differing(y.cpu().numpy().astype(np.float64), y64), _differing(gx.cpu().numpy().astype(np.float64), g64)
    assert bad == (0, 0), bad
    TALLY["tests"] += 1


@pytest.mark.parametrize("c", M.WALKS, ids=_id)
def test_workgroups_walk_several_ragged_tiles_forward_and_grad_input(dev, c):
    assert M.multi_unit("forward", c) and M.multi_unit("grad_input", c), (M.fp32_plan("forward", c), M.fp32_plan("grad_input", c))
    _forward_and_grad_input(dev, c)


@pytest.mark.parametrize("axis,op", [("tr", "forward"), ("tr", "grad_input"), ("tc", "forward"), ("tc", "grad_input")])
def test_tiles_the_lds_budget_shrank_forward_and_grad_input(dev, axis, op):
    c = (M.SHRINK_ROWS if axis == "tr" else M.SHRINK_COLS)[op]
    pl = M.fp32_plan(op, c)
    assert pl[axis + "_shrunk"] > 0 and (axis == "tc" or M.dest_map(op, *c[3], *c[2], c[2][2])[1] >= 28), pl
    _forward_and_grad_input(dev, c)


@pytest.mark.parametrize("c", M.INSTANCES, ids=_id)
def test_the_channel_pairs_the_forward_module_leaves_out(dev, c):
    assert M.fp32_plan("forward", c)["template"] == (c[2][0] ** 2, c[0][0] // 8)
    assert M.fp32_plan("grad_input", c)["template"] == (c[2][0] ** 2, c[0][1] // 8)
    _forward_and_grad_input(dev, c)


# ---- grad_weight -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _wgrad_reference(c, design):
    """(x, go, w, gw, sum |go x|, gbias) of case c: the wgrad module's spikes, about two per channel."""
    xs, ws, ys = _shapes(c)
    L, seed = ys[0] * ys[2] * ys[3], sum(ws) + 7 * xs[3]
    x, go = W._spiked(seed, xs, W.DESIGNS[design][0], L), W._spiked(seed + 1, ys, W.DESIGNS[design][1], L)
    G, (k, s, p) = c[1], c[2]
    gw, gb = M.grad_weight64(x, go, G, c[0][0], k, s, p, p)
    return x, go, R.weights(seed + 2, ws), gw, M.grad_weight64(np.abs(x), np.abs(go), G, c[0][0], k, s, p, p)[0], gb


def _grad_weight(dev, c, design):
    x, go, w, gw64, ab, gb64 = _wgrad_reference(c, design)
    assert ab.max() < 2 ** 24 and np.abs(go).sum((0, 2, 3)).max() < 2 ** 24      # from the reference alone: every sum is an exact integer
    for ste, want in ((R.STE, R.ste_mask(gw64, w)), (0.0, gw64)):
        calls = dict(_lib.call_counts)
        gw, gb = W._run(dev, c[:5] + (c[6],), x, go, w, ste)
        assert F._used(calls).get(W.GWT) == 1
        bad = _differing(gw.cpu().numpy().astype(np.float64), want), _differing(gb.cpu().numpy().astype(np.float64), gb64)
        assert bad == (0, 0), (ste, bad)
    TALLY["tests"] += 1


def test_workgroups_walk_several_ragged_tiles_grad_weight(dev):
    c = M.WGRAD_WALK
    assert M.multi_unit("grad_weight", c) and M.fp32_plan("grad_weight", c)["kernel"] != "gmw_kernel<9,2,1>", M.fp32_plan("grad_weight", c)
    _grad_weight(dev, c, "both_medium")


def test_tiles_the_lds_budget_shrank_grad_weight(dev):
    c = M.SHRINK_ROWS["grad_weight"]
    pl = M.fp32_plan("grad_weight", c)
    assert pl["tr_shrunk"] > 0 and M.dest_map("grad_weight", *c[3], *c[2], c[2][2])[1] >= 28, pl     # gmw_plan never takes a column
    _grad_weight(dev, c, "x_wide")


@pytest.mark.parametrize("i", range(len(M.WGRAD_INSTANCES)), ids=[_id(c) for c in M.WGRAD_INSTANCES])
def test_every_grad_weight_instantiation_with_and_without_the_ste_mask(dev, i):
    c = M.WGRAD_INSTANCES[i]
    assert M.fp32_plan("grad_weight", c)["template"] == (c[2][0] ** 2, c[0][0] // 8, c[0][1] // 16)
    _grad_weight(dev, c, tuple(W.DESIGNS)[i % 3])


# ---- the planes kernel -----------------------------------------------------------------------------------------------------------------

def _planes_every_output_form(dev, c, i):
    """tests/test_gpu_gconv_planes_mfma.py's walk over the output forms, with thresholds that sit exactly on a sum in every fourth
    channel (alpha 1, beta minus a value the channel takes: the tie gives bit 0)."""
    kind = M.KINDS[i % 3]
    xs, ws, ys = PL._shapes(c)
    x, w = R.pm1(100 + i, xs), R.weights(200 + i, ws)
    wq = R.quantize(w, "ternary" if kind == "raw" else kind)
    w_in = wq if kind == "raw" else w
    b = R.gauss6(300 + i, (ys[1],)) if i % 2 == 0 else None
    y = PL._ref(c, x, wq, b)
    r = np.random.RandomState(400 + i)
    alpha, beta = r.randn(ys[1]).astype(np.float32), (r.randn(ys[1]) * 3).astype(np.float32)
    alpha[1::5] = 0
    alpha[::4], beta[::4] = 1, -y[0, ::4, ys[2] // 2, ys[3] // 2]
    neg = P.threshold_bits(y, alpha, beta)
    tie = (y[:, ::4] + beta[None, ::4, None, None]) == 0
    assert tie.any() and not neg[:, ::4][tie].any() and neg.any() and not neg.all()
    args = (dev, c, x, w_in, b, alpha, beta, kind)
    bad = [_differing(PL._sign(*args), P.pack_sign(neg))]
    bad += [_differing(PL._sign(*args, halo=halo), P.pack_nib(neg, halo)) for halo in PL.HALOS]
    both = PL._sign(*args, halo=PL.HALOS[i % 3], with_bits=True)
    bad += [_differing(both[0], P.pack_sign(neg)), _differing(both[1], P.pack_nib(neg, PL.HALOS[i % 3]))]
    bad += [_differing(PL._f32(dev, c, x, w_in, b, kind, layout), y) for layout in ("nchw", "channels_last")]
    assert not any(bad), bad
    TALLY["tests"] += 1


@pytest.mark.parametrize("i", range(len(M.PLANES_WALKS)), ids=["g{0}i{1}o{2}N{3}-{4}x{5}".format(*c) for c in M.PLANES_WALKS])
def test_waves_walk_two_and_three_tiles_with_both_carries(dev, i):
    c = M.PLANES_WALKS[i]
    G, _ci, _co, N, H, W_, k, s, (ph, pw) = c
    Ho, Wo = M.out_hw(H, W_, k, s, ph, pw)
    pl = M.planes_plan(c)
    least, most, carry_wo, carry_ho = M.walk_facts(N, Ho, Wo, pl)
    assert least >= 2 and most >= 3 and min(pl["d_n"], pl["d_ho"], pl["d_wo"]) > 0 and carry_wo and carry_ho, (pl, least, most)
    assert N * Ho * Wo % 16 != 0 and (i < 2 or G % 4 != 0)
    _planes_every_output_form(dev, c, i)


@pytest.mark.parametrize("i", range(len(M.PLANES_INSTANCES)), ids=["g{0}i{1}o{2}-k{6}".format(*c) for c in M.PLANES_INSTANCES])
def test_the_planes_instantiations_the_planes_module_leaves_out(dev, i):
    c = M.PLANES_INSTANCES[i]
    assert M.planes_plan(c)["template"] == (c[6] ** 2, c[1] // 16, c[2] // 16)
    _planes_every_output_form(dev, c, 3 + i)


# ---- what the four modules reach together --------------------------------------------------------------------------------------------

def test_every_instantiation_is_reached_and_nothing_differed():
    """The template instantiations the cases of this module and of the three it builds on launch, from the plan: all 18 of
    grad_weight, all 12 of forward / grad_input (six kernels, each in both directions), all 12 of the planes kernel."""
    fp32 = [c + (2,) for c in F.CASES] + list(M.WALKS) + list(M.SHRINK_ROWS.values()) + list(M.SHRINK_COLS.values()) + list(M.INSTANCES)
    gin_fwd = {(op, M.fp32_plan(op, c)["kernel"]) for c in fp32 for op in ("forward", "grad_input")}
    wgrad = [c[:5] + ("binary", c[5]) for c in W.CASES] + [M.WGRAD_WALK, M.SHRINK_ROWS["grad_weight"]] + list(M.WGRAD_INSTANCES)
    gwt = {M.fp32_plan("grad_weight", c)["kernel"] for c in wgrad}
    planes = {M.planes_plan(c)["kernel"] for c in PL.CASES + M.PLANES_WALKS + M.PLANES_INSTANCES}
    print("instantiations reached: grad_weight {}/18, forward + grad_input {}/12, planes {}/12".format(len(gwt), len(gin_fwd), len(planes)))
    print("exact comparisons of this module: tests {tests}, comparisons {comparisons}, elements {elements}, differing bit patterns "
          "{differing}, waived {waived}".format(**TALLY))
    assert (len(gwt), len(gin_fwd), len(planes)) == (18, 12, 12)
    assert TALLY["differing"] == 0 and TALLY["waived"] == 0
