"""Every rung of the forward route ladder of real-valued first-layer convs (functions/_fused.py ``first_layer_conv_routes``) against
EXACT float64 sums, bit for bit: designed images (tests/_first_exact.py: integers below 2^21 times one quantum, so that both splits
reproduce them under every scale a kernel may choose and every summation order gives the same fp32 value) whose LAST split term is
populated — a kernel that dropped, mis-scaled or mis-placed ``lo`` of the fp16 pair or the third bf16 term fails here, which the
recorded digests of tests/test_gpu_first_layer_routes.py and the normalised tolerances of tests/test_gpu_r3.py cannot see
(tests/test_first_exact_cpu.py shows each of those mutations caught by these very operands).

Each group runs through the entry point of tests/test_gpu_first_layer_routes.py (``_fused.quant_conv2d_forward``, an eval-mode
``FusedConvPoolBnSign``, the functional ``XNORConv2d``) and through ``_fused.first_layer_conv_routes`` called as that entry point
calls it, with ``taken`` naming the rung.  fp32 results are compared as int32 patterns; bit planes, nibble planes (halo and pad
channels zero) and pooled planes with tests/_exact.py ``predicate`` of the exact sum everywhere — the sums are exact, so there
are no ties to waive, and the threshold sets put accumulators exactly ON their thresholds.  Nothing here has a tolerance.
``ops.float_linear`` (LinearBin / LinearTer on a real input) is compared the same way."""
import time

import pytest
import torch

import _exact as X
import _first_exact as FE
import _grad_exact as G
import test_gpu_first_layer_routes as R
from pytorch_quantize_impls_amd import ops
from pytorch_quantize_impls_amd.functions import _fused, xnor_connect
from pytorch_quantize_impls_amd.layers import fused as fused_mod

pytestmark = pytest.mark.gpu

PAIRS = [(g, d) for g in FE.GROUPS for d in g.designs]
RAN = {}                        # (rung, form, table split) -> comparisons
TALLY = {"cases": 0, "elements": 0, "differing": 0, "waived": 0, "seconds": 0.0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def stored(x: torch.Tensor, how: str, dev) -> torch.Tensor:
    """The image on the device as "cl" (channels-last), "nchw", or "view": the channels 1.. of a buffer with one channel more,
    cropped out of a larger map — the rest of the buffer holds 3.0, which no kernel may read."""
    if how == "nchw":
        return x.to(dev).contiguous()
    if how == "cl":
        return x.to(dev).contiguous(memory_format=torch.channels_last)
    assert how == "view", how
    N, C, H, W = x.shape
    big = torch.full((N, C + 1, H + 3, W + 2), 3.0, dtype=torch.float32, device=dev)
    view = big[:, 1:, 1:H + 1, 2:]
    view.copy_(x)
    assert not view.is_contiguous() and view.stride(1) == (H + 3) * (W + 2)
    return view


def count(key, got, want, what):
    """Tally one comparison (bool or int32-pattern tensors of equal shape); returns the number of differing elements."""
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    bad = int((got != want).sum())
    RAN[key] = RAN.get(key, 0) + 1
    TALLY["cases"] += 1
    TALLY["elements"] += int(want.numel())
    TALLY["differing"] += bad
    return bad


def compare(g, c, form, res, alpha, beta, what, pooled_result=True):
    """One kernel output against the exact reference.  ``res``: the fp32 NCHW tensor, or the words of a bit / nibble plane."""
    N, Cout, Ho, Wo = g.batch, g.geom[1], c.Ho, c.Wo
    key = (g.rung, form, g.table_split)
    if form == "f32":
        got = res.detach().cpu().contiguous()
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, Cout, Ho, Wo), (what, got.dtype, tuple(got.shape))
        bad = count(key, got.view(torch.int32), c.y32.view(torch.int32), what)
        assert bad == 0, G.mismatch_report(got, c.y32, names=("n", "c", "y", "x"), what=what) or f"{what}: {bad} zero signs differ"
        return
    words = res.detach().cpu()
    assert words.dtype == torch.int32, (what, words.dtype)
    pool = form == "pool" and pooled_result
    want, v = FE.want_bits(c, alpha, beta, pool=pool)
    if pool:
        Ho, Wo = Ho // 2, Wo // 2
    if form.startswith("nib"):
        halo = {"nib11": (1, 1), "nib22": (2, 2)}[form]
        got = X.nib_to_bits(X.decode_nib(words, N, Ho, Wo, Cout, halo))
    else:
        assert int(words.shape[0]) == N * Ho * Wo, (what, tuple(words.shape), (N, Ho, Wo))
        X.check_pad_bits(words, Cout, what)
        got = X.bits_of_words(words.view(N, Ho, Wo, -1), Cout)
    bad = count(key, got, want, what)
    assert bad == 0, X.mismatch_report(got, want, acc=None if pool else c.y64.permute(0, 2, 3, 1), v=v, what=what)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return bool(torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)))


@pytest.mark.parametrize("g,design", PAIRS, ids=[f"{g.id}-{d}" for g, d in PAIRS])
def test_rung_equals_the_exact_sums(dev, g, design):
    t0 = time.perf_counter()
    c = g.case(design)
    assert c.ok, c.why                                             # (a proof that fails is a failure, not a skip)
    assert c.coverage >= FE.COVERAGE, c.coverage
    C, Cout, k, st, pd, dl, H, W = g.geom
    x, w, b = stored(c.x, g.storage, dev), c.w.to(dev), c.bias.to(dev)
    seed = FE.seed_of("gpu", g.id, design)
    sw = dict(g.sw)
    if g.switch:
        sw["FLOAT_SPLIT"] = g.switch
    # the weight image the rungs compute with is the designed one
    with torch.no_grad():
        wq_dev = xnor_connect.xnor_weight(w, [0, 1])[0] if g.kind == "xnor" else _fused.quantize_weight_f32(w, g.kind)
    assert same_bits(wq_dev, c.wq) or bool(torch.equal(wq_dev.cpu(), c.wq)), "the quantised weight image is not the designed one"
    if g.entry == "block":
        bn = tuple(t.to(dev) for t in FE.bn_set(c, seed))
        probe = torch.nn.BatchNorm2d(Cout).to(dev).eval()
        for dst, src in zip((probe.running_mean, probe.running_var, probe.weight.data, probe.bias.data), bn):
            dst.copy_(src)
        alpha_d, beta_d = fused_mod.fold_batchnorm(probe)
        alpha, beta = alpha_d.cpu(), beta_d.cpu()
        ra, rb = FE.fold_bn(*FE.bn_set(c, seed))
        assert same_bits(alpha, ra) and same_bits(beta, rb), "the BatchNorm fold differs from its restated fp32 operations"
        given = (x, w, b, None, None, bn)
    else:
        alpha, beta = FE.affine_set(c, seed)
        alpha_d, beta_d = alpha.to(dev), beta.to(dev)
        given = (x, w, b, alpha_d, beta_d)
    ties = FE.want_bits(c, alpha, beta)[1] == 0
    assert int(ties[..., 8:].sum()) >= 1, "no accumulator sits exactly on its threshold"

    for form in g.forms:
        what = f"{g.id} {design} {form}"
        res, calls = R.run_case((g.id, g.rung, g.entry, g.kind, g.geom, g.batch, form, sw), dev, given=given)
        assert any(calls.get(m) for m in R.MARKS[g.rung]), (what, calls)
        for ahead in R._AHEAD.get(g.rung, ()):
            assert not any(calls.get(m) for m in R.MARKS[ahead]), (what, ahead, calls)
        compare(g, c, form, res, alpha, beta, what + " entry")

        # the ladder itself, called as the entry point calls it: ``taken`` names the rung
        taken = []
        with R.switches(sw), torch.no_grad():
            if g.entry == "forward":
                out = _fused.first_layer_conv_routes(x, w, b, st, pd, dl, g.kind, epi=R.forward_epi(form, alpha_d, beta_d),
                                                     rungs=FE.FORWARD_RUNGS, taken=taken)
            elif g.entry == "function":
                out = _fused.first_layer_conv_routes(x, w, b, st, pd, dl, "xnor", weight_q=wq_dev, taken=taken)
            else:
                blk = R.make_block(g.kind, g.geom, form, dev, w, b, bn)
                conv = blk.conv
                epi = (alpha_d, beta_d) if form in ("bits", "pool") else ops.NibEpilogue(alpha_d, beta_d, blk.out_nib_halo)
                args = (x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, g.kind)
                if g.kind == "xnor":
                    out = _fused.first_layer_conv_routes(*args, epi=epi, cache=conv._conv_triples, taken=taken)
                else:
                    out = _fused.first_layer_conv_routes(*args, epi=epi, cache=conv._conv_triples, rungs=FE.BLOCK_RUNGS,
                                                         pooled=form == "pool", taken=taken)
                    if out is None:                                 # the block falls through to the conv's own ladder
                        assert taken == [] and g.rung not in FE.BLOCK_RUNGS, (what, taken)
                        out = _fused.first_layer_conv_routes(*args, epi=epi, weight_q=conv.weight, cache=conv._conv_triples,
                                                             rungs=FE.FORWARD_RUNGS, taken=taken)
        assert out is not None and taken == [g.rung], (what, taken)
        y, shape = out
        assert tuple(shape) == (g.batch, Cout, c.Ho, c.Wo), (what, shape)
        if form == "f32":
            y = y.view(g.batch, c.Ho, c.Wo, Cout).permute(0, 3, 1, 2)
        else:
            assert isinstance(y, ops.NibPlanes if form.startswith("nib") else ops.BitPlanes), (what, type(y))
            y = y.words if form.startswith("nib") else y.sign
        compare(g, c, form, y, alpha, beta, what + " ladder", pooled_result=False)      # (the ladder hands the pool its un-pooled bits)
    TALLY["seconds"] += time.perf_counter() - t0


LIN = FE.linear_cases()


@pytest.mark.parametrize("M,N,K,split,design,with_bias", LIN, ids=["-".join(str(v) for v in t) for t in LIN])
def test_float_linear_equals_the_exact_product(dev, M, N, K, split, design, with_bias):
    t0 = time.perf_counter()
    c = FE.linear_case(M, N, K, split, design, with_bias)
    assert c.ok, c.why
    if design == "ramp" or FE.dense_reaches(K, split):
        assert c.coverage >= FE.COVERAGE, c.coverage
    with ops.float_split(split), torch.no_grad():
        y = ops.float_linear(c.x.to(dev), c.w.to(dev), "binary", c.bias.to(dev) if with_bias else None)
    got = y.cpu()
    bad = count(("float_linear", "f32", split), got.view(torch.int32), c.y32.view(torch.int32), "float_linear")
    assert bad == 0, G.mismatch_report(got, c.y32, names=("m", "n"), what=f"float_linear {M}x{N}x{K} {split} {design}")
    TALLY["seconds"] += time.perf_counter() - t0


def test_every_rung_form_and_split_ran_against_the_exact_reference():
    """Rung x output form x split from the table of tests/_first_exact.py; every rung ``first_layer_rungs`` can name is in it."""
    named = set()
    for kind in ("binary", "xnor"):
        for geom in ((3, 64, 3, 1, 1, 1, 6, 6), (6, 32, 3, 1, 1, 1, 6, 6), (3, 24, 11, 4, 2, 1, 33, 35)):
            C, Cout, k, st, pd, dl, H, W = geom
            named.update(_fused.first_layer_rungs(C, Cout, (k, k), st, pd, dl, H, W, kind, out=(1, 1)))
    assert named == set(FE.FORMS), named ^ set(FE.FORMS)
    missing = [t for t in FE.table() if not RAN.get(t)]
    assert not missing, missing
    for split in ("f16x2", "bf16x3"):
        assert RAN.get(("float_linear", "f32", split)) == len(LIN) // 2
    print(f"\nfirst-layer exact tally: {TALLY['cases']} comparisons, {TALLY['elements']} elements compared, "
          f"{TALLY['differing']} differing bit patterns, {TALLY['waived']} waived, {TALLY['seconds']:.1f} s")
    assert TALLY["differing"] == 0 and TALLY["waived"] == 0
