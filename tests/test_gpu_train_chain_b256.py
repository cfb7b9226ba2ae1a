"""The training chains of csrc/train_chain.hip (layers.FusedTrainPoolBnSign, layers.FusedTrainBnActQuant) at the row counts of
the batch-256 training steps, against the float64 module chain and the designed operands of tests/_chain_exact.py.

Rows and channels are independent in these kernels (a workgroup owns a row slab and walks all channel chunks), so the row
regimes run at C = 8 and the channel regimes at R = 8448; no case needs the workload's full tensors (largest: 256 x 8 x 55 x 55).

  rows      R = 48 (fewer partials than fold lanes), 8192 (full fold, one row per thread), 8448 (slab 17: the first off a multiple
            of 16), 186 624 (slab 365, ragged last slab of 109: AlexNet-Bin conv1 behind its 3 / 2 pool), 262 144 (slab 512:
            the DoReFa ResNet-18 stem) and the other chain shapes of the two steps (43 264, 9216, 256, 65 536, 16 384, 4096);
            every case asserts its regime with ``rows_plan``;
  channels  C = 4, 68, 256, 260 and one representative of every (chunks, last chunk full, last fold group full) class the
            models have (64, 512, 576, 768, 1152 at R = 8448; 4096 at R = 528);
  pools     (k, s, H, W) = (2, 2, 9, 11), (2, 3, 8, 11), (3, 1, 7, 6), (5, 3, 13, 17), (11, 11, 11, 22), an NCHW-contiguous input.

  (a) designed operands, exact in fp32 whatever the summation order (``proves_exact`` first): mean / invstd, sign image, p and
      idx, dgamma, dbeta, g_res and running_mean bit for bit; g_x bit for bit against the fp32 restatement of the last pass
      (``grad_x_f32``) and within 1e-5 per channel of float64; values sit exactly on y = 0, y = +-1, t = 0 and the Hardtanh
      ends, so the strictness of every mask shows.  (Where a mask is 0, g_y is 0 but g_x is not: BatchNorm's backward leaves
      the batch terms -dbeta / R - xhat dgamma / R on every element.  The bit-exact comparison covers exactly those elements;
      with upstream gradients that cancel in every (channel, deviation) group, dbeta = dgamma = 0 and g_x IS exactly 0 there:
      ``balanced_grad``, at R = 8448, 186 624, 262 144 and C = 260.)  A second design whose slab partials cancel (+-2^23 units)
      pins the double fold of the partials.
  (b) Gaussian operands over six decades of per-channel scale, every fourth channel at 32 sigma, de-tied: signs, g_res masks
      and int8 codes exact with nothing excluded; g_x / g_res within 1e-5 per channel; |dgamma err| <= 1e-5 sum|g_y xhat|,
      |dbeta err| <= 1e-5 sum|g_y|; running_mean within 1e-6 mean|p| of the channel (the bound of a sum's error is relative to
      sum|p|), running_var within 1e-6 of itself; pixels outside every window get exactly 0; the mean equals the fp32
      restatement of the summation tree (``tree_stats``) bit for bit, which pins the slab plan, the lane stride and the fold.
  (c) integer inputs (ties in every window) through overlapping pools, (3, 2) at R = 186 624: idx and the gradient's routing.
  (d) NaN, +inf and an all -inf window through the pool: p / idx as F.max_pool2d, nothing leaks across the lanes of a quad.
  (e) every chain call of one training step of both benchmark models, scaled to batch 256, has a case here with the same
      (rows_plan(R), k, s) and the same channel class, and every kernel of train_chain.hip was launched by a comparing case.

Run the whole module: the coverage test reads what the cases before it recorded and prints the module's wall time and peak
device memory (88 cases; 26 s and 0.27 GiB measured on an MI355X).

Each of these deliberate changes to train_chain.hip, tried one at a time, fails cases here (and, but for the last, none of the
batch-8 chain tests of tests/test_gpu_r3.py): a slab of rows_per_block + 1 rows, a lane stride of 32 (the mean is no longer the
tree's: the Gaussian cases; the stride also every designed case above 16 rows per slab), partials folded in fp32
(test_cancelling_partials_need_the_double_fold), a one-pass variance (the Gaussian cases: running_var misses 1e-6 on the 32 sigma
channels), y >= lo in the Hardtanh mask and t >= 0 in the ReLU mask (the designed cases), no NaN clause in the pool (d), the first
window column of the pooling gather off by one (every pooled case; test_gpu_r3.py sees this one too)."""
import copy
import os
import re
import time

import pytest
import torch
import torch.nn.functional as F

import _chain_exact as X
from test_gpu_grad_b256 import kernel_label, profiled  # noqa: F401

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib, ops, packed  # noqa: E402
from pytorch_quantize_impls_amd.layers import FusedTrainBnActQuant, FusedTrainPoolBnSign  # noqa: E402

BAR = 1e-5                  # the project's TOL / BAR
STAT_BAR = 1e-6             # running statistics
T0 = time.time()
PEAK = {}
COVERED = {}                # kernel of train_chain.hip -> cases that compared its output
TRIPLES = {}                # (rows_plan(R), k, s) -> cases
CLASSES = {}                # channel class -> cases


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _free_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    PEAK[request.node.name] = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()


class _Spy:
    """Keeps what ops.<name> returns while the module under test calls it (mean / invstd / p / idx never leave the autograd node)."""

    def __init__(self, name):
        self.name, self.got = name, []

    def __enter__(self):
        self.orig = getattr(ops, self.name)

        def wrapped(*a, **k):
            r = self.orig(*a, **k)
            self.got.append(r)
            return r
        setattr(ops, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(ops, self.name, self.orig)


def _bn(C, gamma, beta, eps, momentum, four):
    bn = (torch.nn.BatchNorm2d if four else torch.nn.BatchNorm1d)(C, eps=eps, momentum=momentum, affine=gamma is not None)
    if gamma is not None:
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
    return bn


def _image(rows, N, H, W):
    """[N H W, C] rows -> the NCHW view of that NHWC storage (channels_last)."""
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _record(case, kernels, R, k, s, C):
    for kn in kernels:
        COVERED.setdefault(kn, []).append(case)
    TRIPLES.setdefault((X.rows_plan(R), k, s), []).append(case)
    CLASSES.setdefault(X.channel_class(C), []).append(case)


def _put(x, dev, nchw=False):
    xd = x.to(dev)
    if x.dim() == 4:
        xd = xd.contiguous() if nchw else xd.contiguous(memory_format=torch.channels_last)
    return xd.requires_grad_(True)


def _run_sign(dev, case, x, g, bn, pool, ht, nchw=False, mod=None):
    """One forward + backward of FusedTrainPoolBnSign on the device under the profiler -> dict of CPU tensors (NCHW)."""
    if mod is None:
        mod = FusedTrainPoolBnSign(copy.deepcopy(bn).to(dev), torch.nn.MaxPool2d(*pool) if pool else None,
                                   torch.nn.Hardtanh(*ht) if ht else None).train()
    xd = _put(x, dev, nchw)
    for prm in mod.bn.parameters():
        prm.grad = None

    def go():
        with _Spy("pool_bn_sign_train") as spy:
            y = mod(xd)
            y.backward(g.to(dev))
        return y, spy.got

    (y, got), kernels, calls, lib = profiled(go)
    assert not lib, f"{case}: dense-library paths taken: {lib}"
    assert calls.get("qt_pool_bn_sign_train_f32") == 1 and calls.get("qt_pool_bn_sign_train_backward_f32") == 1, (case, calls)
    p_or_x, idx, mean, invstd, (N, H, W, C, k, s) = got[0][1]
    Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
    _record(case, kernels, N * Ho * Wo, k, s, C)
    if nchw:
        assert xd.grad.is_contiguous()
    out = dict(y=y.detach().cpu(), g_x=xd.grad.cpu(), mean=mean.cpu(), invstd=invstd.cpu(), mod=mod, tagged=y,
               dgamma=mod.bn.weight.grad.cpu() if mod.bn.affine else None, dbeta=mod.bn.bias.grad.cpu() if mod.bn.affine else None,
               running_mean=mod.bn.running_mean.cpu(), running_var=mod.bn.running_var.cpu(), nbt=int(mod.bn.num_batches_tracked))
    if k > 1:
        out["p"], out["idx"] = p_or_x.permute(0, 3, 1, 2).cpu(), idx.permute(0, 3, 1, 2).cpu()
    return out


def _run_act(dev, case, x, g, bn, res, relu=True, bits=4, nchw=False, mod=None):
    if mod is None:
        mod = FusedTrainBnActQuant(copy.deepcopy(bn).to(dev), bits, relu=relu).train()
    xd = _put(x, dev, nchw)
    rd = _put(res, dev, nchw) if res is not None else None
    for prm in mod.bn.parameters():
        prm.grad = None

    def go():
        with _Spy("bn_train_stats") as spy:
            y = mod(xd, residual=rd)
            y.backward(g.to(dev))
        return y, spy.got

    (y, got), kernels, calls, lib = profiled(go)
    assert not lib, f"{case}: dense-library paths taken: {lib}"
    assert calls.get("qt_bn_train_stats_f32") == 1 and calls.get("qt_bn_act_train_backward_f32") == 1, (case, calls)
    C = int(x.shape[1])
    R = x.numel() // C
    _record(case, kernels, R, 1, 1, C)
    stats2 = got[0][1].cpu()
    out = dict(y=y.detach().cpu(), g_x=xd.grad.cpu(), g_res=rd.grad.cpu() if rd is not None else None, mean=stats2[:C], invstd=stats2[C:],
               dgamma=mod.bn.weight.grad.cpu() if mod.bn.affine else None, dbeta=mod.bn.bias.grad.cpu() if mod.bn.affine else None,
               running_mean=mod.bn.running_mean.cpu(), running_var=mod.bn.running_var.cpu(), nbt=int(mod.bn.num_batches_tracked), mod=mod)
    if bits:
        tag = packed.lookup_codes(y, packed.NHWC if x.dim() == 4 else packed.ROWS_LAST)
        assert tag is not None and tag.bit_width == bits, case
        codes = tag.codes[:, :C].cpu()
        out["codes"] = codes.reshape(x.shape[0], x.shape[2], x.shape[3], C).permute(0, 3, 1, 2) if x.dim() == 4 else codes.reshape(x.shape)
    return out


def _same(got, want64, what):
    """bit for bit: ``want64`` holds fp32 values (asserted)."""
    w32 = want64.to(torch.float32)
    assert torch.equal(w32.double(), want64.double()), f"{what}: the reference is not an fp32 value"
    bad = got.cpu() != w32
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} differ; first at {bad.nonzero()[0].tolist()}: " \
        f"got {got.cpu()[bad][0].item()!r}, want {w32[bad][0].item()!r}"


def _check_bars(case, got, ref, affine=True, res=False):
    """(b)'s float bars, which hold for the designed operands as well."""
    e = X.channel_err(got["g_x"], ref["g_x"])
    print(f"{case}: g_x per-channel err {float(e.max()):.2e}", end="")
    assert float(e.max()) <= BAR, (case, "g_x per channel", float(e.max()), int(e.argmax()))
    if res:
        e = X.channel_err(got["g_res"], ref["g_res"])
        assert float(e.max()) <= BAR, (case, "g_res per channel", float(e.max()))
    if affine:
        dg = (got["dgamma"].double() - ref["dgamma"]).abs()
        db = (got["dbeta"].double() - ref["dbeta"]).abs()
        print(f", dgamma {float((dg / ref['abs_dgamma'].clamp(min=1e-300)).max()):.2e}, dbeta "
              f"{float((db / ref['abs_dbeta'].clamp(min=1e-300)).max()):.2e} of sum|summand|", end="")
        assert bool((dg <= BAR * ref["abs_dgamma"]).all()), (case, "dgamma", float(dg.max()))
        assert bool((db <= BAR * ref["abs_dbeta"]).all()), (case, "dbeta", float(db.max()))
    scale = ref["bn"].momentum * ref["p"].abs().mean(X._dims(ref["p"]))
    em = (got["running_mean"].double() - ref["running_mean"]).abs() / scale
    ev = (got["running_var"].double() - ref["running_var"]).abs() / ref["running_var"]
    print(f", running mean {float(em.max()):.2e} var {float(ev.max()):.2e}")
    assert float(em.max()) <= STAT_BAR, (case, "running_mean", float(em.max()), int(em.argmax()))
    assert float(ev.max()) <= STAT_BAR, (case, "running_var", float(ev.max()), int(ev.argmax()))


def _check_designed(case, got, ref, D, gamma, beta, R, res=None):
    ok, why = X.proves_exact(ref, D["unit"], gamma, beta, res=res, dev_unit=D["dev_unit"])
    assert ok, f"{case}: the designed operands are not exact ({why})"
    _same(got["mean"], ref["mean"], case + " mean")
    _same(got["invstd"], ref["invstd"], case + " invstd")
    if gamma is not None:
        _same(got["dgamma"], ref["dgamma"], case + " dgamma")
        _same(got["dbeta"], ref["dbeta"], case + " dbeta")
    _same(got["running_mean"], ref["running_mean"], case + " running_mean")
    if res is not None:
        _same(got["g_res"], ref["g_res"], case + " g_res")
        assert not bool(got["g_res"][ref["t"] == 0].any()) and bool((ref["t"] == 0).any())


def _check_tree(case, got, ref):
    """The device's mean is the fp32 restatement of its summation tree bit for bit (``tree_stats``: slabs of rows_plan(R) rows,
    16 lanes striding by 16, lane fold, partials in double), and the launch is sized by the same plan.  Any other slab length,
    lane stride or fold precision rounds differently on Gaussian data."""
    rows = ref["p"].movedim(1, -1).reshape(-1, ref["p"].shape[1]).to(torch.float32)
    R, C = rows.shape
    assert int(_lib.load().qt_train_chain_partial_floats(R, C)) == 2 * X.rows_plan(R)[1] * C, case
    mean, invstd = X.tree_stats(rows, ref["bn"].eps)
    bad = got["mean"] != mean
    assert not bool(bad.any()), f"{case}: the mean is not the one of the stated summation tree in {int(bad.sum())} of {C} channels " \
        f"(first: channel {int(bad.nonzero()[0])}, got {got['mean'][bad][0].item()!r}, tree {mean[bad][0].item()!r})"
    e = (got["invstd"].double() - invstd.double()).abs() / invstd.double()
    assert float(e.max()) <= 2.0 ** -22, (case, "invstd vs the tree's", float(e.max()))


def _gp_exact(ref, gamma, beta, R):
    return X.grad_x_f32(ref["p"], ref["g_y"], ref["mean"], ref["invstd"], gamma, beta, ref["dgamma"], ref["dbeta"], R)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

# R -> ((N, H, W) of the un-pooled chain or None for a [R, C] matrix, rows per block, blocks, rows of the last block)
ROWS = {
    48: (None, 16, 3, 16),
    8192: ((32, 16, 16), 16, 512, 16),
    8448: ((33, 16, 16), 17, 497, 16),
    186624: (None, 365, 512, 109),                 # [256 * 729, 8]; pooled 3 / 2 from 256 x 55 x 55 below
    262144: ((256, 32, 32), 512, 512, 512),
    # the other chain shapes of the two batch-256 steps (the coverage test asks for each)
    43264: ((256, 13, 13), 85, 509, 84),           # AlexNet-Bin conv3 / conv4
    256: (None, 16, 16, 16),                       # its classifier's BatchNorm1d
    65536: ((256, 16, 16), 128, 512, 128),         # ResNet-18 layer2
    16384: ((256, 8, 8), 32, 512, 32),             # layer3
    4096: ((256, 4, 4), 16, 256, 16),              # layer4
}
# pooled (3, 2) chains of the AlexNet-Bin step: R -> (N, H, W) of the input
POOLED_ROWS = {186624: (256, 55, 55), 43264: (256, 27, 27), 9216: (256, 13, 13)}
CHANNELS = [(4, 8448), (68, 8448), (256, 8448), (260, 8448),
            (64, 8448), (512, 8448), (576, 8448), (768, 8448), (1152, 8448), (4096, 528)]   # one per class the models have
POOLS = [(2, 2, 9, 11), (2, 3, 8, 11), (3, 1, 7, 6), (5, 3, 13, 17), (11, 11, 11, 22)]


def _assert_regime(R):
    shape, rpb, nblk, last = ROWS[R] if R in ROWS else (None,) + {9216: (18, 512, 18)}[R]
    assert X.rows_plan(R) == (rpb, nblk) and R - (nblk - 1) * rpb == last, (R, X.rows_plan(R))
    return shape


def _shape_rows(rows, R):
    shape = ROWS[R][0] if R in ROWS else None
    return _image(rows, *shape) if shape is not None else rows


def _designed_sign(dev, R, C, ht=(-1.0, 1.0), affine=True, shape=None, tag=""):
    case = f"designed sign chain R={R} C={C} ht={ht} affine={affine}{tag}"
    D = X.designed_rows(R, C, seed=R + C)
    ga, be = X.designed_affine(C) if affine else (None, None)
    x = _image(D["p"], *shape) if shape is not None else D["p"]
    g = X.designed_grad(x.shape, R + C + 1)
    bn = _bn(C, ga, be, X.DESIGNED_EPS, 0.25, x.dim() == 4)
    ref = X.sign_chain64(x, g, bn, ht=ht)
    got = _run_sign(dev, case, x, g, bn, None, ht)
    _check_designed(case, got, ref, D, ga, be, R)
    _same(got["y"], ref["out"], case + " sign image")
    if affine:
        assert bool((got["y"][ref["y"] == 0] == 1.0).all()) and bool((ref["y"] == 0).any()), case + ": y == 0 -> +1"
    dead = ~ref["mask"]
    assert bool(dead.any()) and bool(ref["mask"].any()), case
    want = _gp_exact(ref, ga, be, R)
    _same(got["g_x"], want, case + " g_x (fp32 restatement; where the mask is 0: the batch terms alone)")
    _check_bars(case, got, ref, affine)
    assert got["nbt"] == 1
    return got, ref


@pytest.mark.parametrize("R", sorted(ROWS))
def test_designed_rows_sign_chain_is_exact(dev, R):
    shape = _assert_regime(R)
    _designed_sign(dev, R, 8, shape=shape)


@pytest.mark.parametrize("C,R", CHANNELS)
def test_designed_channels_sign_chain_is_exact(dev, C, R):
    _designed_sign(dev, R, C, shape=ROWS[R][0] if R in ROWS else None)


def _designed_act(dev, R, C, shape=None, relu=True, bits=4):
    case = f"designed DoReFa chain R={R} C={C}"
    D = X.designed_rows(R, C, seed=R + C + 5)
    ga, be = X.designed_affine(C)
    res_rows = X.designed_residual(D, ga, be, seed=R + C + 6, share=0.125)
    x, res = (_image(D["p"], *shape), _image(res_rows, *shape)) if shape is not None else (D["p"], res_rows)
    g = X.designed_grad(x.shape, R + C + 7)
    bn = _bn(C, ga, be, X.DESIGNED_EPS, 0.25, x.dim() == 4)
    ref = X.act_chain64(x, g, bn, res=res, relu=relu, bits=bits)
    assert float((ref["t"] == 0).double().mean()) >= 0.11, case + ": t == 0 on an eighth of the elements"
    assert float(ref["codes"].abs().max()) <= 127
    got = _run_act(dev, case, x, g, bn, res, relu, bits)
    _check_designed(case, got, ref, D, ga, be, R, res=res)
    _same(got["codes"].float(), ref["codes"], case + " int8 codes")
    assert float((got["y"].double() - ref["out"]).abs().max()) <= 1e-6, case + " quantised image"
    _same(got["g_x"], _gp_exact(ref, ga, be, R), case + " g_x (fp32 restatement)")
    _check_bars(case, got, ref, True, res=True)
    assert got["nbt"] == 1


@pytest.mark.parametrize("R", sorted(ROWS))
def test_designed_rows_dorefa_chain_is_exact(dev, R):
    shape = _assert_regime(R)
    _designed_act(dev, R, 8, shape=shape)


@pytest.mark.parametrize("C,R", CHANNELS)
def test_designed_channels_dorefa_chain_is_exact(dev, C, R):
    _designed_act(dev, R, C, shape=ROWS[R][0] if R in ROWS else None)


@pytest.mark.parametrize("R", [8448, 186624, 262144])
def test_cancelling_partials_need_the_double_fold(dev, R):
    """Slab partials of +-2^23 units with their low bits set: exact as fp32 values, exact in the double fold, and 2^27 units
    deep in a lane of an fp32 fold.  The mean is the designed integer bit for bit; the statistics of the DoReFa entry too."""
    _assert_regime(R)
    C = 8
    D = X.designed_cancelling_rows(R, C, seed=R)
    rpb, _ = X.rows_plan(R)
    ok, why = X.proves_exact(dict(p=D["p"].double(), mean=D["m"]), D["unit"], slab_rows=rpb, variance=False)
    assert ok, why
    x = D["p"]
    g = X.designed_grad(x.shape, R)
    bn = _bn(C, None, None, 1e-4, 0.25, False)
    ref = X.sign_chain64(x, g, bn)
    case = f"cancelling partials R={R}"
    got = _run_sign(dev, case, x, g, bn, None, None)
    _same(got["mean"], D["m"], case + " mean")
    _same(got["running_mean"], 0.25 * D["m"], case + " running_mean")
    e = (got["invstd"].double() - ref["invstd"]).abs() / ref["invstd"]
    assert float(e.max()) <= STAT_BAR, (case, float(e.max()))
    _same(got["y"], ref["out"], case + " sign image")
    with torch.no_grad():
        _, stats2 = ops.bn_train_stats(x.to(dev), None, None, 1e-4, 0.25)
    _same(stats2[:C], D["m"], case + " bn_train_stats mean")


@pytest.mark.parametrize("R,C", [(8448, 8), (186624, 8), (262144, 8), (8448, 260)])
def test_balanced_gradients_leave_exact_zeros_where_a_mask_is_zero(dev, R, C):
    """Upstream gradients that cancel inside every (channel, deviation) group of the un-masked elements: dbeta = dgamma = 0
    exactly, BatchNorm's backward keeps no batch term, and g_x is EXACTLY 0 at y == +-1 (Hardtanh's strict mask), at t == 0
    (ReLU's) — and gamma invstd g, bit for bit, everywhere else."""
    shape = ROWS[R][0]
    D = X.designed_rows(R, C, seed=R + C + 20)
    ga, be = X.designed_affine(C)
    img = (lambda rows: _image(rows, *shape)) if shape is not None else (lambda rows: rows)
    x, d = img(D["p"]), img(D["d"])
    bn = _bn(C, ga, be, X.DESIGNED_EPS, 0.25, x.dim() == 4)
    scale = lambda ref: X._bc(ga.double(), x) * X._bc(ref["invstd"], x)
    # [MaxPool] -> BatchNorm -> Hardtanh -> sign
    mask = X.sign_chain64(x, torch.ones(x.shape), bn, ht=(-1.0, 1.0))["mask"]
    g = X.balanced_grad(mask, d, R + C + 21)
    ref = X.sign_chain64(x, g, bn, ht=(-1.0, 1.0))
    case = f"balanced sign chain R={R} C={C}"
    got = _run_sign(dev, case, x, g, bn, None, (-1.0, 1.0))
    assert not bool(ref["dgamma"].any()) and not bool(ref["dbeta"].any()) and float(ref["abs_dbeta"].max()) > 0
    _same(got["dgamma"], ref["dgamma"], case + " dgamma")
    _same(got["dbeta"], ref["dbeta"], case + " dbeta")
    on_edge = ref["y"].abs() == 1.0
    assert bool(on_edge.any()) and not bool(mask[on_edge].any()) and bool((g[on_edge] != 0).all())
    assert not bool(got["g_x"][~mask].any()), case + ": g_x must be exactly 0 where the mask is 0 (y == +-1 included)"
    _same(got["g_x"], ref["g_y"] * scale(ref), case + " g_x")
    # BatchNorm + shortcut -> ReLU -> quantiser
    res = img(X.designed_residual(D, ga, be, seed=R + C + 22))
    mask = X.act_chain64(x, torch.ones(x.shape), bn, res=res)["mask"]
    g = X.balanced_grad(mask, d, R + C + 23)
    ref = X.act_chain64(x, g, bn, res=res)
    case = f"balanced DoReFa chain R={R} C={C}"
    got = _run_act(dev, case, x, g, bn, res)
    assert not bool(ref["dgamma"].any()) and not bool(ref["dbeta"].any())
    _same(got["dgamma"], ref["dgamma"], case + " dgamma")
    _same(got["dbeta"], ref["dbeta"], case + " dbeta")
    at_zero = ref["t"] == 0
    assert bool(at_zero.any()) and bool((g[at_zero] != 0).all())
    assert not bool(got["g_x"][~mask].any()) and not bool(got["g_res"][~mask].any()), case + ": exactly 0 where t <= 0 (t == 0 included)"
    _same(got["g_x"], ref["g_y"] * scale(ref), case + " g_x")
    _same(got["g_res"], ref["g_y"], case + " g_res")


def test_designed_pool_2_2_with_ties_is_exact(dev):
    N, C, H, W, k = 4, 12, 9, 11, 2
    case = "designed pool (2, 2) 9x11"
    xr, D = X.designed_pool_input(N, C, H, W, k, seed=17)
    x = xr.permute(0, 3, 1, 2)
    ga, be = X.designed_affine(C)
    R = N * (H // k) * (W // k)
    g = X.designed_grad((N, C, H // k, W // k), 18)
    bn = _bn(C, ga, be, X.DESIGNED_EPS, 0.25, True)
    ref = X.sign_chain64(x, g, bn, pool=(k, k), ht=(-1.0, 1.0))
    got = _run_sign(dev, case, x, g, bn, (k, k), (-1.0, 1.0))
    _check_designed(case, got, ref, D, ga, be, R)
    _same(got["p"], ref["p"], case + " p")
    assert torch.equal(got["idx"].long(), ref["idx"]), case + " idx"
    _same(got["y"], ref["out"], case + " sign image")
    # stride == window: a pixel is in one window at most, so g_x is the routed g_p itself, bit for bit, and 0 elsewhere
    gp = _gp_exact(ref, ga, be, R)
    want = torch.zeros((N, C, H, W))
    hh = (torch.arange(H // k).reshape(-1, 1) * k + ref["idx"] // k)
    ww = (torch.arange(W // k).reshape(1, -1) * k + ref["idx"] % k)
    want.reshape(N, C, -1).scatter_(2, (hh * W + ww).reshape(N, C, -1), gp.reshape(N, C, -1))
    _same(got["g_x"], want, case + " g_x")
    assert not bool(got["g_x"][:, :, H - 1, :].any()) and not bool(got["g_x"][:, :, :, W - 1].any())
    _check_bars(case, got, ref)


def test_designed_once_each_affine_false_no_hardtanh_other_hardtanh(dev):
    R, shape = 8448, ROWS[8448][0]
    _designed_sign(dev, R, 8, affine=False, shape=shape)
    got, ref = _designed_sign(dev, R, 8, ht=None, shape=shape)
    y = ref["y"]
    assert bool(ref["mask"][y.abs() == 1.0].all()) and not bool(ref["mask"][y.abs() > 1.001].any())     # |h| <= 1.001
    got, ref = _designed_sign(dev, R, 8, ht=(-0.5, 2.0), shape=shape)
    assert bool((y == -0.5).any()) and bool((y == 2.0).any()) and not bool(ref["mask"][(y == -0.5) | (y == 2.0)].any())
    # BatchNorm without affine parameters through the DoReFa chain's entries as well (the ld4_or(nullptr) lanes)
    D = X.designed_rows(R, 8, seed=3)
    x = _image(D["p"], *shape)
    res = _image(X.designed_residual(D, torch.ones(8), torch.zeros(8), seed=4), *shape)
    g = X.designed_grad(x.shape, 5)
    bn = _bn(8, None, None, X.DESIGNED_EPS, 0.25, True)
    ref = X.act_chain64(x, g, bn, res=res)
    got = _run_act(dev, "designed DoReFa chain affine=False", x, g, bn, res)
    _check_designed("designed DoReFa chain affine=False", got, ref, D, None, None, R, res=res)
    _same(got["codes"].float(), ref["codes"], "affine=False codes")
    _same(got["g_x"], _gp_exact(ref, None, None, R), "affine=False g_x")


def test_two_consecutive_steps_update_the_running_statistics_twice(dev):
    R, C, shape = 8448, 8, ROWS[8448][0]
    ga, be = X.designed_affine(C)
    bn = _bn(C, ga, be, X.DESIGNED_EPS, 0.25, True)
    bn_a = copy.deepcopy(bn)
    mod = mod_a = None
    for step in range(2):
        D = X.designed_rows(R, C, seed=50 + step)
        x = _image(D["p"], *shape)
        g = X.designed_grad(x.shape, 60 + step)
        ref = X.sign_chain64(x, g, bn, ht=(-1.0, 1.0))
        got = _run_sign(dev, f"two steps, sign chain, step {step}", x, g, bn, None, (-1.0, 1.0), mod=mod)
        mod, bn = got["mod"], ref["bn"]
        res = _image(X.designed_residual(D, ga, be, seed=70 + step), *shape)
        ref_a = X.act_chain64(x, g, bn_a, res=res)
        got_a = _run_act(dev, f"two steps, DoReFa chain, step {step}", x, g, bn_a, res, mod=mod_a)
        mod_a, bn_a = got_a["mod"], ref_a["bn"]
    for got_, ref_ in ((got, ref), (got_a, ref_a)):
        assert got_["nbt"] == 2 and int(ref_["bn"].num_batches_tracked) == 2
        _same(got_["running_mean"], ref_["running_mean"], "running_mean after two steps")
        assert bool((ref_["running_mean"] != 0.25 * D["m"]).any())                  # the first step's share is in it
        ev = (got_["running_var"].double() - ref_["running_var"]).abs() / ref_["running_var"]
        assert float(ev.max()) <= STAT_BAR


# ---- (b) Gaussian, de-tied --------------------------------------------------------------------------------------------------

GAUSS_EPS, GAUSS_MOMENTUM = 1e-4, 0.15


def _gauss_sign(dev, case, N, C, H, W, pool=None, ht=(-1.0, 1.0), nchw=False, two_d=False, seed=0):
    rows, sigma = X.gaussian_rows(N * H * W, C, seed)
    x = rows if two_d else _image(rows, N, H, W)
    if nchw:
        x = x.contiguous()
    ga, be = X.gaussian_affine(C, seed + 1)
    bounds = (0.0,) + (tuple(ht) if ht is not None else (-X.STE_THRESHOLD, X.STE_THRESHOLD))
    x, moved = X.detie(x, sigma, ga, be, GAUSS_EPS, boundaries=bounds, pool=pool)
    bn = _bn(C, ga, be, GAUSS_EPS, GAUSS_MOMENTUM, not two_d)
    k, s = pool if pool else (1, 1)
    oshape = x.shape if pool is None else (N, C, (H - k) // s + 1, (W - k) // s + 1)
    g = torch.randn(oshape, generator=X._gen(seed + 2))
    ref = X.sign_chain64(x, g, bn, pool=pool, ht=ht)
    assert float(X.boundary_distance(ref["y"], bounds).abs().min()) >= X.BAND, case
    got = _run_sign(dev, case, x, g, bn, pool, ht, nchw=nchw)
    flips = int((got["y"].double() != ref["out"]).sum())
    assert flips == 0, f"{case}: {flips} signs differ (de-tied input, {moved} elements moved)"
    if pool:
        assert torch.equal(got["p"].double(), ref["p"]), case + " p"
        assert torch.equal(got["idx"].long(), ref["idx"]), case + " idx"
        out = ~X.covered_pixels(H, W, k, s)
        if bool(out.any()):
            assert not bool(got["g_x"][:, :, out].any()), case + ": pixels in no window must get gradient 0"
    _check_bars(case, got, ref)
    _check_tree(case, got, ref)
    return got, ref


def _gauss_act(dev, case, N, C, H, W, two_d=False, seed=0, bits=4, relu=True, with_res=True):
    rows, sigma = X.gaussian_rows(N * H * W, C, seed)
    x = rows if two_d else _image(rows, N, H, W)
    ga, be = X.gaussian_affine(C, seed + 1)
    res = torch.randn(x.shape, generator=X._gen(seed + 3)) * 0.5 if with_res else None
    if res is not None and not two_d:
        res = res.contiguous(memory_format=torch.channels_last)
    x, moved = X.detie(x, sigma, ga, be, GAUSS_EPS, boundaries=(0.0,) if relu else (), levels=float((1 << bits) - 1) if bits else 0.0,
                       res=res)
    bn = _bn(C, ga, be, GAUSS_EPS, GAUSS_MOMENTUM, not two_d)
    g = torch.randn(x.shape, generator=X._gen(seed + 2))
    ref = X.act_chain64(x, g, bn, res=res, relu=relu, bits=bits)
    got = _run_act(dev, case, x, g, bn, res, relu, bits)
    if bits:
        assert float(ref["codes"].abs().max()) <= 127, case + ": the input leaves int8 (an input fault)"
        bad = int((got["codes"].double() != ref["codes"]).sum())
        assert bad == 0, f"{case}: {bad} int8 codes differ (de-tied input, {moved} elements moved)"
        assert float((got["y"].double() - ref["out"]).abs().max()) <= 1e-6, case + " quantised image"
    else:
        e = X.channel_err(got["y"], ref["out"])
        assert float(e.max()) <= BAR, (case, "BatchNorm output per channel", float(e.max()))
    if with_res:
        assert torch.equal(got["g_res"], torch.where(ref["mask"], g, torch.zeros(()))), case + ": ReLU mask (g_res = g 1[t > 0])"
    _check_bars(case, got, ref, res=with_res)
    _check_tree(case, got, ref)


@pytest.mark.parametrize("R", sorted(ROWS))
def test_gaussian_rows_both_chains_vs_fp64(dev, R):
    shape = _assert_regime(R)
    N, H, W = shape if shape is not None else (R, 1, 1)
    _gauss_sign(dev, f"Gaussian sign chain R={R}", N, 8, H, W, two_d=shape is None, seed=R)
    _gauss_act(dev, f"Gaussian DoReFa chain R={R}", N, 8, H, W, two_d=shape is None, seed=R + 10)


@pytest.mark.parametrize("R", sorted(POOLED_ROWS))
def test_gaussian_pooled_3_2_rows_of_the_alexnet_step_vs_fp64(dev, R):
    N, H, W = POOLED_ROWS[R]
    _assert_regime(R)
    assert N * ((H - 3) // 2 + 1) * ((W - 3) // 2 + 1) == R
    _gauss_sign(dev, f"Gaussian pooled (3, 2) sign chain R={R}", N, 8, H, W, pool=(3, 2), seed=R + 1)


@pytest.mark.parametrize("C,R", CHANNELS)
def test_gaussian_channels_both_chains_vs_fp64(dev, C, R):
    shape = ROWS[R][0] if R in ROWS else None
    N, H, W = shape if shape is not None else (R, 1, 1)
    _gauss_sign(dev, f"Gaussian sign chain C={C}", N, C, H, W, two_d=shape is None, seed=C)
    _gauss_act(dev, f"Gaussian DoReFa chain C={C}", N, C, H, W, two_d=shape is None, seed=C + 10)


def test_gaussian_plain_batchnorm_of_the_shortcut_branch_vs_fp64(dev):
    # a_bits = 0, no ReLU, no shortcut input: the BatchNorm behind a 1x1 shortcut conv (act kernels with relu = 0, res = NULL)
    _gauss_act(dev, "Gaussian plain BatchNorm (shortcut) R=16384", 256, 8, 8, 8, seed=91, bits=0, relu=False, with_res=False)
    _gauss_act(dev, "Gaussian DoReFa chain without shortcut R=8448", 33, 8, 16, 16, seed=92, with_res=False)


@pytest.mark.parametrize("k,s,H,W", POOLS)
def test_gaussian_pool_geometries_vs_fp64(dev, k, s, H, W):
    _gauss_sign(dev, f"Gaussian pool ({k}, {s}) {H}x{W}", 4, 12, H, W, pool=(k, s), seed=100 * k + s)


def test_gaussian_nchw_contiguous_input_returns_an_nchw_gradient(dev):
    # R = 8448 behind a (2, 2) pool: the ctx.x_nchw return path (gx.contiguous())
    _gauss_sign(dev, "Gaussian NCHW-contiguous input, pool (2, 2), R=8448", 33, 8, 32, 32, pool=(2, 2), nchw=True, seed=77)
    assert X.rows_plan(33 * 16 * 16) == (17, 497)
    _gauss_sign(dev, "Gaussian NCHW-contiguous input, no pool, no Hardtanh", 33, 8, 16, 16, ht=None, nchw=True, seed=78)


# ---- (c) integer inputs: ties through overlapping pools ---------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,k,s", [(256, 55, 3, 2), (4, 9, 3, 1)])
def test_integer_inputs_with_ties_route_the_gradient_to_the_first_maximum(dev, N, H, k, s):
    """Conv outputs of +-1 nets are integers: equal maxima inside a window are the rule, and with overlapping windows a pixel
    collects the gradient of every window that names it.  gamma = 0.02 keeps |y| < 1 (asserted; no mask decides anything: the gradient is
    BatchNorm's backward routed by idx alone); (3, 2) at 256 x 55 x 55: R = 186 624, slabs span images."""
    C = 8
    x = torch.randint(-3, 4, (N, H, H, C), generator=X._gen(N + k + s)).float().permute(0, 3, 1, 2)
    Ho = (H - k) // s + 1
    if N == 256:
        assert X.rows_plan(N * Ho * Ho) == (365, 512)
    ga, be = torch.full((C,), 0.02), torch.linspace(-0.2, 0.2, C)
    bn = _bn(C, ga, be, 1e-5, 0.1, True)
    g = torch.randn((N, C, Ho, Ho), generator=X._gen(5))
    ref = X.sign_chain64(x, g, bn, pool=(k, s))
    assert bool(ref["mask"].all())
    case = f"integer ties pool ({k}, {s}) N={N}"
    got = _run_sign(dev, case, x, g, bn, (k, s), None)
    win = F.unfold(x[:2].reshape(-1, 1, H, H), k, stride=s)
    assert float(((win == win.amax(1, keepdim=True)).sum(1) > 1).double().mean()) > 0.3          # windows with a tie are common
    assert torch.equal(got["p"].double(), ref["p"]) and torch.equal(got["idx"].long(), ref["idx"]), case + " p / idx"
    _check_bars(case, got, ref)
    clear = ref["y"].abs() > X.BAND
    assert torch.equal(got["y"].double()[clear], ref["out"][clear])


# ---- (d) non-finite values through the pool ---------------------------------------------------------------------------------------

def test_nan_and_inf_through_the_pool_stay_in_their_lane(dev):
    N, C, H, W, k, s = 3, 8, 9, 9, 3, 2
    gen = X._gen(8)
    clean = torch.randn((N, H, W, C), generator=gen)
    x = clean.clone()
    x[0, 4, 4, 0] = float("nan")              # in four windows
    x[1, 2, 5, 1] = float("inf")
    x[2, 2:5, 4:7, 2] = -float("inf")         # window (1, 2) of image 2 is all -inf
    ga, be = X.gaussian_affine(C, 9)
    g = torch.randn((N, 4, 4, C), generator=gen).permute(0, 3, 1, 2)
    outs = []
    for data in (x, clean):
        xd = data.permute(0, 3, 1, 2).to(dev).contiguous(memory_format=torch.channels_last)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        def go():
            out, saved = ops.pool_bn_sign_train(xd, ga.to(dev), be.to(dev), rm, rv, 1e-4, 0.1, k, s, (-1.0, 1.0))
            gx, dg, db = ops.pool_bn_sign_train_backward(g.to(dev), saved, ga.to(dev), be.to(dev), (-1.0, 1.0))
            return out, saved, gx, dg, db

        (out, saved, gx, dg, db), kernels, _, _ = profiled(go)
        outs.append(dict(out=out.cpu(), p=saved[0].permute(0, 3, 1, 2).cpu(), idx=saved[1].permute(0, 3, 1, 2).cpu(),
                         mean=saved[2].cpu(), invstd=saved[3].cpu(), gx=gx.cpu(), dg=dg.cpu(), db=db.cpu(), rm=rm.cpu(), rv=rv.cpu()))
    _record("non-finite values through the pool", kernels, N * 16, k, s, C)
    bad, ok = outs
    p, flat = F.max_pool2d(x.permute(0, 3, 1, 2), k, s, return_indices=True)
    assert torch.equal(bad["p"].contiguous().view(torch.int32), p.contiguous().view(torch.int32)), "p differs from F.max_pool2d bit for bit"
    assert torch.equal(bad["idx"].long(), X.window_argmax(flat, W, k, s)), "idx differs from F.max_pool2d"
    assert int(torch.isnan(p[0, 0]).sum()) == 4 and bool(torch.isinf(p[1, 1]).any()) and float(p[2, 2, 1, 2]) == -float("inf")
    assert int(bad["idx"][2, 2, 1, 2]) == 0
    for key in ("out", "gx"):
        assert torch.equal(bad[key][:, 3:], ok[key][:, 3:]), f"{key}: the poison leaked into the untouched channels"
    for key in ("mean", "invstd", "dg", "db", "rm", "rv"):
        assert torch.equal(bad[key][3:], ok[key][3:]), f"{key}: the poison leaked into the untouched channels"
    assert bool(torch.isfinite(ok["gx"]).all())


# ---- the host fixes: non-square pools, one pooled value per channel -----------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(kernel_size=(3, 2)), dict(kernel_size=3, stride=(2, 1)), dict(kernel_size=3, stride=2, padding=(0, 1))],
                         ids=["kernel(3,2)", "stride(2,1)", "padding(0,1)"])
def test_non_square_pool_keeps_the_module_chain_on_the_device(dev, kw):
    from pytorch_quantize_impls_amd.functions import BinaryConnect
    from pytorch_quantize_impls_amd.layers import fuse_sequential, fuse_sequential_training
    torch.manual_seed(3)
    C = 8
    seq = torch.nn.Sequential(torch.nn.MaxPool2d(**kw), torch.nn.BatchNorm2d(C), torch.nn.Hardtanh(), BinaryConnect(stochastic=False)).to(dev)
    with torch.no_grad():
        seq[1].weight.uniform_(0.5, 1.5)
        seq[1].bias.normal_(0, 0.3)
        seq[1].running_mean.normal_(0, 0.5)
    x = torch.randn(4, C, 9, 10, device=dev)
    train = fuse_sequential_training(copy.deepcopy(seq).train())
    assert [type(m).__name__ for m in train] == ["MaxPool2d", "FusedTrainPoolBnSign"]
    want = copy.deepcopy(seq).train()(x)
    got = train(x)
    assert got.shape == want.shape and torch.equal(got, want)
    ev = fuse_sequential(copy.deepcopy(seq).eval(), fold="device")
    assert [type(m).__name__ for m in ev] == ["MaxPool2d", "FusedPoolBnSign"]
    with torch.no_grad():
        want = copy.deepcopy(seq).eval()(x)
        act = ev(x)
    assert tuple(act.shape) == tuple(want.shape)


def test_one_pooled_value_per_channel_raises_like_batchnorm(dev):
    mod = FusedTrainPoolBnSign(torch.nn.BatchNorm2d(8).to(dev), torch.nn.MaxPool2d(3, 3), torch.nn.Hardtanh()).train()
    before = _lib.call_counts.get("qt_pool_bn_sign_train_f32", 0)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        mod(torch.randn(1, 8, 3, 3, device=dev))
    assert _lib.call_counts.get("qt_pool_bn_sign_train_f32", 0) == before
    assert mod(torch.randn(2, 8, 3, 3, device=dev)).shape == (2, 8, 1, 1)
    assert _lib.call_counts.get("qt_pool_bn_sign_train_f32", 0) == before + 1


# ---- (e) coverage ---------------------------------------------------------------------------------------------------------------

def _chain_kernels():
    src = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "csrc", "train_chain.hip")
    with open(src) as fh:
        return sorted(set(re.findall(r"__global__\s+__launch_bounds__\(\d+\)\s+void\s+(\w+)\s*\(", fh.read())))


def _step_chain_calls(dev):
    """(model, module kind, N, C, H, W, k, s) of every chain call of one batch-2 forward of the two fused training models."""
    import bench_models
    calls = []
    torch.manual_seed(0)
    for name, build, shape in (("alexnet_bin", lambda: bench_models.TrainFusedAlexNetBin(bench_models.AlexNetBin()), (2, 3, 224, 224)),
                               ("dorefa_resnet18", lambda: bench_models.TrainFusedDorefaResNet18(bench_models.DorefaResNet18(w_bits=1, a_bits=4)),
                                (2, 3, 32, 32))):
        model = build().to(dev).to(memory_format=torch.channels_last).train()
        hooks = []
        for m in model.modules():
            if isinstance(m, (FusedTrainPoolBnSign, FusedTrainBnActQuant)):
                def hook(mod, args, name=name):
                    x = args[0]
                    N, C = int(x.shape[0]), int(x.shape[1])
                    H, W = (int(x.shape[2]), int(x.shape[3])) if x.dim() == 4 else (1, 1)
                    k, s = (mod.pool_k, mod.pool_s) if isinstance(mod, FusedTrainPoolBnSign) else (1, 1)
                    calls.append((name, type(mod).__name__, N, C, H, W, k, s))
                hooks.append(m.register_forward_pre_hook(hook))
        model(torch.randn(*shape, device=dev).contiguous(memory_format=torch.channels_last))
        for h in hooks:
            h.remove()
    return calls


def test_every_chain_shape_and_kernel_of_the_batch_256_steps_was_compared(dev):
    """Prints the table, the module's wall time and its peak device memory (26 s, 0.27 GiB on an MI355X)."""
    calls = _step_chain_calls(dev)
    assert sum(c[0] == "alexnet_bin" for c in calls) == 7 and sum(c[0] == "dorefa_resnet18" for c in calls) == 20, calls
    report, missing = [], []
    for name, kind, N, C, H, W, k, s in calls:
        assert N == 2
        R = 256 * ((H - k) // s + 1) * ((W - k) // s + 1)
        triple, cls = (X.rows_plan(R), k, s), X.channel_class(C)
        line = f"  {name}: {kind} C={C} {H}x{W} pool ({k}, {s}) -> R={R}, slab {triple[0][0]} x {triple[0][1]}, channel class {cls}"
        if triple not in TRIPLES:
            missing.append(line + ": no case with this (rows_plan, k, s)")
        elif cls not in CLASSES:
            missing.append(line + ": no channel-sweep case of this class")
        else:
            report.append(line + f" <- {TRIPLES[triple][0]}; {CLASSES[cls][0]}")
    kernels = _chain_kernels()
    assert len(kernels) >= 11, kernels
    for kn in kernels:
        if kn in COVERED:
            report.append(f"  kernel {kn} <- {len(COVERED[kn])} cases, first: {COVERED[kn][0]}")
        else:
            missing.append(f"  kernel {kn}: launched by no comparing case")
    worst = max(PEAK.items(), key=lambda kv: kv[1]) if PEAK else ("-", 0)
    print("\nchain calls of the batch-256 training steps and the kernels of train_chain.hip:\n" + "\n".join(report)
          + f"\nwall time of the module: {time.time() - T0:.1f} s; peak device memory: {worst[1] / 2**30:.2f} GiB ({worst[0]})")
    assert not missing, "not compared in this module:\n" + "\n".join(missing)
