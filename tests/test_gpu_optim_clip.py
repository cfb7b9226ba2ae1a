"""Gradient-norm clipping inside the fused update (csrc/optim_step.hip: the sum-of-squares pass, the finalise launch, the update
entries with QT_OPTIM_GSCALE; utils/optim.py ``max_grad_norm``).  Oracles: exact values where fp32 is exact (all-ones gradients, power-of-two
scales), the float64 restatement of tests/_clip_exact.py with its derived bounds elsewhere, and bit equality between forms that
must agree (coef 1.0 against the unclipped optimiser, a captured replay against the eager clipped step).  The MLP, its batches and
the state twin are those of tests/test_gpu_optim_capture.py."""
import ctypes

import numpy as np
import pytest
import torch

import _clip_exact as CX
import _optim_abi as A
import _optim_exact as X
import test_gpu_optim_capture as C
from pytorch_quantize_impls_amd import _lib, ops, utils
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import LinearBin

pytestmark = pytest.mark.gpu

INVALID, ALIGNMENT = -1, -2
# around the 4096-element unit and its 16-byte tail, three units with a tail, an empty tensor, and a view one element into its
# storage (4-byte aligned only: the dword walk)
EDGES = [1, 3, 4095, 4096, 4097, 2 * 4096 + 5, 0, "view"]
VIEW_NUMEL = 4101


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _tensor(dev, size, fill):
    """A contiguous fp32 device tensor of ``size`` elements produced by ``fill(n)`` (a host tensor); "view" = VIEW_NUMEL elements
    starting one element into their storage."""
    if size == "view":
        base = torch.zeros(VIEW_NUMEL + 1, device=dev)
        base[1:].copy_(fill(VIEW_NUMEL))
        t = base[1:]
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    return fill(size).to(dev)


N_EDGES = sum(1 for s in EDGES if s != 0)


def _sizes(n_tensors):
    """EDGES followed by small odd sizes: ``n_tensors`` NON-EMPTY tensors (what a chunk of 32 slots counts) and, among the added
    ones, one more empty tensor, so table and slot indices differ."""
    extra = [7 + 3 * i for i in range(n_tensors - N_EDGES)]
    if len(extra) > 20:
        extra.insert(20, 0)
    return EDGES + extra


def _norm(grads, dev, pad=8, finite=True, **kw):
    """(norm, coef) as numpy float32 from one optim_grad_norm call; the workspace starts as NaN (no initial content is needed) and
    the words behind it must stay untouched."""
    m = ops.optim_grad_norm_work_floats(grads)
    assert m == sum((g.numel() + 4095) // 4096 for g in grads)
    work = torch.full((m + pad,), float("nan"), device=dev)
    out = torch.full((2,), float("nan"), device=dev)
    ops.optim_grad_norm(grads, work[:m], out, **kw)
    assert bool(torch.isnan(work[m:]).all())
    assert not finite or not bool(torch.isnan(work[:m]).any())               # every unit's word was written
    o = out.cpu().numpy()
    return o[0], o[1]


# ---- 1. the norm ----------------------------------------------------------------------------------------------------------------

def test_norm_of_ones_is_exact(dev):
    sizes = EDGES + [33, 515]
    used = sum(VIEW_NUMEL if s == "view" else s for s in sizes)
    sizes.append(65536 - used)
    grads = [_tensor(dev, s, torch.ones) for s in sizes]
    assert sum(g.numel() for g in grads) == 65536 and sizes[-1] > 4 * 4096
    before = _lib.call_counts["qt_optim_grad_sumsq_f32"], _lib.call_counts["qt_optim_grad_norm_finalize_f32"]
    norm, coef = _norm(grads, dev, max_norm=64.0)
    assert (_lib.call_counts["qt_optim_grad_sumsq_f32"], _lib.call_counts["qt_optim_grad_norm_finalize_f32"]) == (before[0] + 1, before[1] + 1)
    want = np.float32(64.0) / (np.float32(256.0) + np.float32(1e-6))
    assert norm == np.float32(256.0)
    assert coef.view(np.uint32) == want.view(np.uint32) == CX.coef_f32(norm, 64.0).view(np.uint32)
    # the captured form reads max_norm from the device: the same two words
    norm_d, coef_d = _norm(grads, dev, max_norm_dev=torch.tensor([64.0], device=dev))
    assert norm_d == norm and coef_d.view(np.uint32) == coef.view(np.uint32)
    assert _norm(grads, dev, max_norm=1e30)[1] == np.float32(1.0)          # nothing to clip: exactly 1
    assert all(bool((g == 1).all()) for g in grads)                        # read only


@pytest.mark.parametrize("n_tensors", [N_EDGES, 33, 65], ids=["edges", "two_chunks", "three_chunks"])
def test_gaussian_norm_is_inside_the_bound(dev, n_tensors):
    assert ops.optim_chunk_capacity() == 32
    gen = torch.Generator().manual_seed(50 + n_tensors)
    grads = [_tensor(dev, s, lambda n: torch.randn(n, generator=gen) * 3.0) for s in _sizes(n_tensors)]
    assert sum(1 for g in grads if g.numel()) == n_tensors and sum(1 for g in grads if not g.numel()) == (1 if n_tensors < 28 else 2)
    norm64 = CX.total_norm(grads)
    norm, coef = _norm(grads, dev, max_norm=2.0)
    ratio = abs(float(norm) - norm64) / CX.norm_bound(norm64)
    print(f"{n_tensors} tensors: norm {norm!r}, float64 {norm64!r}, error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert coef.view(np.uint32) == CX.coef_f32(norm, 2.0).view(np.uint32) and coef < 1
    again = _norm(grads, dev, max_norm=2.0)
    assert again[0].view(np.uint32) == norm.view(np.uint32)                # a fixed order: the same bits every time
    if n_tensors == 65:                                                    # one tensor more or less moves the norm: all are read
        assert _norm(grads[:-1], dev, max_norm=2.0)[0] != norm


def test_norm_of_nothing_and_of_non_finite_gradients(dev):
    assert _norm([], dev, max_norm=3.0) == (np.float32(0.0), np.float32(1.0))
    assert _norm([torch.zeros(0, device=dev)], dev, max_norm=3.0) == (np.float32(0.0), np.float32(1.0))
    g = torch.ones(5000, device=dev)
    g[4500] = float("inf")
    norm, coef = _norm([g], dev, max_norm=3.0)
    assert np.isinf(norm) and coef == 0                                    # torch with error_if_nonfinite=False: the update zeroes g
    g[17] = float("nan")
    norm, coef = _norm([g], dev, max_norm=3.0, finite=False)
    assert np.isnan(norm) and np.isnan(coef)


# ---- 2. the clipped update entries ----------------------------------------------------------------------------------------------

def _scaled(tab, s):
    return [g * s for g in tab[1]]


FORMS = ["value", "dev", "guard", "value_guard"]


def _raised_guard_moves_nothing(dev, run, n_lists):
    """A raised guard, with and without ``gscale``: parameters, state and gradients keep their bits and the planes their -1 fill."""
    for gscale in (torch.tensor([0.25], device=dev), None):
        c = C._tensor_table(dev, 100)
        snap = [[t.clone() for t in lst] for lst in c[:n_lists]]
        run(c, c[1], gscale, skip=torch.ones(1, dtype=torch.int32, device=dev))
        for k in range(n_lists):
            C._same(c[k], snap[k])
        assert all(bool((pl[0].words == -1).all()) for pl in c[5] if pl is not None)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hp", [dict(), dict(momentum=0.9, weight_decay=1e-3, nesterov=True)], ids=["plain", "nesterov_wd"])
def test_clipped_sgd_entry(dev, hp, form):
    """Every walk of the update kernel (the 36-entry table of test_gpu_optim_capture.py: two chunks, planes, a dword view, empty
    tensors).  gscale 1.0 stores the bits of the unclipped entry; gscale 0.25 those of the unclipped entry on 0.25 g (a product with
    a power of two is exact, so this is an equality, not a bound).  The guarded forms ("guard": scalars from the device,
    "value_guard": by value) with a clear guard store the bits of the unguarded by-value call, with and without gscale."""
    mom = "momentum" in hp
    lr = torch.tensor([0.05], device=dev)
    clear = torch.zeros(1, dtype=torch.int32, device=dev) if "guard" in form else None

    def run(tab, grads, gscale, skip=clear, form=form):
        kw = dict(clamps=tab[4], planes=tab[5], gscale=gscale, skip=skip, **hp)
        if form.startswith("value"):
            ops.optim_step_sgd(tab[0], grads, tab[2] if mom else None, lr=0.05, **kw)
        else:
            ops.optim_step_sgd_dev(tab[0], grads, tab[2] if mom else None, lr, **kw)

    with A.recorded_forms() as calls:
        for scale in (1.0, 0.25):
            a, b = C._tensor_table(dev, 100), C._tensor_table(dev, 100)
            g0 = [g.clone() for g in b[1]]
            run(a, _scaled(a, scale), None)
            run(b, b[1], torch.tensor([scale], device=dev))
            C._same(a[0], b[0]), C._same(a[2], b[2]), C._same_planes(a[5], b[5])
            C._same(b[1], g0)                                              # the gradients in memory are not rewritten
            assert all(not bool((pl[0].words == -1).any()) for pl in b[5] if pl is not None)
            if "guard" in form:                                            # clear guard = the bits of the unguarded run
                u = C._tensor_table(dev, 100)
                run(u, _scaled(u, scale), None, skip=None, form="value")
                C._same(u[0], a[0]), C._same(u[2], a[2]), C._same_planes(u[5], a[5])
    # exactly the clipped runs carried QT_OPTIM_GSCALE, and every run the form it was asked for
    want = A.FORMS[form]
    unguarded = [("qt_optim_sgd_f32", 0)] if "guard" in form else []
    assert calls == 2 * ([("qt_optim_sgd_f32", want), ("qt_optim_sgd_f32", want | A.GSCALE)] + unguarded)
    if "guard" in form:
        _raised_guard_moves_nothing(dev, run, 3)


@pytest.mark.parametrize("form", FORMS)
def test_clipped_adam_entry(dev, form):
    hp = dict(betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)
    steps = list(range(1, C.N_TENSORS + 1))
    coef = torch.tensor(ops.adam_coefficients(steps, 3e-3, hp["betas"]), dtype=torch.float32, device=dev).reshape(-1)
    clear = torch.zeros(1, dtype=torch.int32, device=dev) if "guard" in form else None

    def run(tab, grads, gscale, skip=clear, form=form):
        kw = dict(clamps=tab[4], planes=tab[5], gscale=gscale, skip=skip, **hp)
        if form.startswith("value"):
            ops.optim_step_adam(tab[0], grads, tab[2], tab[3], steps, lr=3e-3, **kw)
        else:
            ops.optim_step_adam_dev(tab[0], grads, tab[2], tab[3], coef, **kw)

    with A.recorded_forms() as calls:
        for scale in (1.0, 0.25):
            a, b = C._tensor_table(dev, 200), C._tensor_table(dev, 200)
            g0 = [g.clone() for g in b[1]]
            run(a, _scaled(a, scale), None)
            run(b, b[1], torch.tensor([scale], device=dev))
            C._same(a[0], b[0]), C._same(a[2], b[2]), C._same(a[3], b[3]), C._same_planes(a[5], b[5])
            C._same(b[1], g0)
            if "guard" in form:                                            # clear guard = the bits of the unguarded run
                u = C._tensor_table(dev, 200)
                run(u, _scaled(u, scale), None, skip=None, form="value")
                C._same(u[0], a[0]), C._same(u[2], a[2]), C._same(u[3], a[3]), C._same_planes(u[5], a[5])
    want = A.FORMS[form]
    unguarded = [("qt_optim_adam_f32", 0)] if "guard" in form else []
    assert calls == 2 * ([("qt_optim_adam_f32", want), ("qt_optim_adam_f32", want | A.GSCALE)] + unguarded)
    if "guard" in form:
        _raised_guard_moves_nothing(dev, run, 4)


def test_abi_errors_enqueue_nothing(dev):
    lib = _lib.load()
    p, g, m, v = (torch.randn(5000, device=dev) for _ in range(4))
    keep = [t.clone() for t in (p, g, m, v)]
    tab = (ops._OptimTensor * 1)()
    e = tab[0]
    e.p, e.g, e.s0, e.s1, e.numel, e.lo, e.hi = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 5000, float("-inf"), float("inf")
    t, scal = ctypes.addressof(tab), torch.full((4,), 0.5, device=dev)
    work = torch.full((4,), -7.0, device=dev)
    s = ops._stream(dev)
    assert lib.qt_optim_sgd_f32(t, 1, A.GSCALE, 0.1, None, None, None, 0.9, 0.0, 0, s) == INVALID
    assert lib.qt_optim_sgd_f32(t, 1, A.GSCALE, 0.1, None, scal.data_ptr() + 2, None, 0.9, 0.0, 0, s) == ALIGNMENT
    assert lib.qt_optim_sgd_f32(t, 1, A.SCALARS_DEV | A.GSCALE, 0.1, scal.data_ptr(), None, None, 0.0, 0.0, 0, s) == INVALID
    assert lib.qt_optim_adam_f32(t, 1, A.GSCALE, None, None, None, 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, s) == INVALID
    assert lib.qt_optim_adam_f32(t, 1, A.SCALARS_DEV | A.GSCALE, scal.data_ptr(), scal.data_ptr() + 2, None, 0.9, 0.1, 0.999, 0.001, 1e-8,
                                 0.0, s) == ALIGNMENT
    # a valid pointer whose bit is clear, and a form with an unknown bit: refused, not read
    assert lib.qt_optim_sgd_f32(t, 1, 0, 0.1, None, scal.data_ptr(), None, 0.9, 0.0, 0, s) == INVALID
    assert lib.qt_optim_adam_f32(t, 1, A.GSCALE | 0x8, None, scal.data_ptr(), None, 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, s) == INVALID
    assert lib.qt_optim_grad_sumsq_f32(t, 1, None, s) == INVALID
    assert lib.qt_optim_grad_sumsq_f32(t, 1, work.data_ptr() + 2, s) == ALIGNMENT
    assert lib.qt_optim_grad_norm_finalize_f32(None, 2, 1.0, None, scal.data_ptr(), s) == INVALID
    assert lib.qt_optim_grad_norm_finalize_f32(work.data_ptr() + 2, 2, 1.0, None, scal.data_ptr(), s) == ALIGNMENT
    assert lib.qt_optim_sgd_f32(None, 0, A.GSCALE, 0.1, None, None, None, 0.0, 0.0, 0, s) == 0            # n == 0
    torch.cuda.synchronize()
    for a, b in zip((p, g, m, v), keep):
        assert torch.equal(a, b)
    assert bool((work == -7.0).all()) and bool((scal == 0.5).all())
    with pytest.raises(ValueError):
        ops.optim_step_sgd([p], [g], None, lr=0.1, gscale=torch.ones(2, device=dev))
    with pytest.raises(TypeError):
        ops.optim_step_sgd([p], [g], None, lr=0.1, gscale=torch.ones(1))
    with pytest.raises(ValueError):
        ops.optim_grad_norm([g], work[:1], scal[:2], max_norm=1.0)                                       # 2 units need 2 words


# ---- 3. the optimisers, eagerly -------------------------------------------------------------------------------------------------

class _Edge(torch.nn.Module):
    """LinearBin(24, 40) — a plane tensor (K = 24: three plane words of four, K % 8 == 0 but ld padded) with its +-1 clamp on weight
    and bias — next to flat parameters of the EDGES sizes."""

    def __init__(self, dev, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        self.lin = LinearBin(24, 40).to(dev)
        self.extra = torch.nn.ParameterList([torch.nn.Parameter(_tensor(dev, s, lambda n: torch.randn(n, generator=gen))) for s in EDGES])

    def set_grads(self, seed, scale=1.0):
        gen = torch.Generator().manual_seed(seed)
        for p in self.parameters():
            if p.numel() == VIEW_NUMEL:
                p.grad = _tensor(p.device, "view", lambda n: torch.randn(n, generator=gen) * scale)
            else:
                p.grad = (torch.randn(p.shape, generator=gen) * scale).to(p.device)


def _two_groups(model, cls, **kw):
    """The model's parameters in two groups with different learning rates, clamps and planes as given the module."""
    opt = cls(model, **kw)
    params = opt.param_groups[0]["params"]
    opt.param_groups[0]["params"] = params[:3]
    opt.add_param_group({"params": params[3:], "lr": kw["lr"] * 0.5})
    assert len(opt.param_groups) == 2 and opt._plane_of(model.lin.weight) is not None
    return opt


SGD_FORMS = {"plain": dict(lr=0.05), "momentum": dict(lr=0.05, momentum=0.9), "nesterov": dict(lr=0.05, momentum=0.9, nesterov=True),
             "wd": dict(lr=0.05, momentum=0.9, weight_decay=1e-3)}


def _snapshot(model, opt):
    out = []
    for p in model.parameters():
        st = opt.state.get(p) or {}
        out.append((p.detach().clone(), p.grad.clone(), {k: v.clone() for k, v in st.items() if torch.is_tensor(v) and v.is_cuda}))
    return out


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_clipped_step_against_float64(dev, kind):
    model = _Edge(dev, 3)
    hp = dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True) if kind == "sgd" else dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6,
                                                                                                weight_decay=1e-2)
    opt = _two_groups(model, utils.FusedQuantSGD if kind == "sgd" else utils.FusedQuantAdam, max_grad_norm=1.5, **hp)
    plan = utils.clamp_plan(model)
    assert plan[model.lin.weight] == (-1.0, 1.0)
    counts = {k: _lib.call_counts[k] for k in ("qt_optim_grad_sumsq_f32", "qt_optim_grad_norm_finalize_f32")}
    worst = worst_norm = 0.0
    updates = []
    for step in (1, 2, 3):
        model.set_grads(70 + step)
        snap = _snapshot(model, opt)
        with A.recorded_forms() as calls:
            opt.step()
        updates += calls
        norm, coef = opt.grad_norm.cpu().numpy(), opt.clip_coef.cpu().numpy()
        assert opt.grad_norm.dim() == 0 and opt.grad_norm.dtype == torch.float32 and opt.grad_norm.is_cuda
        norm64 = CX.total_norm([s[1] for s in snap])
        worst_norm = max(worst_norm, abs(float(norm) - norm64) / CX.norm_bound(norm64))
        assert coef.view(np.uint32) == CX.coef_f32(norm, 1.5).view(np.uint32) and coef < 1
        for gi, group in enumerate(opt.param_groups):
            lr = hp["lr"] * (1.0 if gi == 0 else 0.5)
            for p in group["params"]:
                p0, g0, st0 = snap[[id(q) for q in model.parameters()].index(id(p))]
                assert torch.equal(p.grad, g0)                             # p.grad stays unscaled
                kw = {k: v for k, v in hp.items() if k != "lr"}
                if kind == "sgd":
                    p64, b64, bp, bb = CX.sgd_step(p0, g0, st0.get("momentum_buffer"), coef, lr=lr, **kw)
                    worst = max(worst, X.worst(opt.state[p]["momentum_buffer"], b64, bb))
                else:
                    m0 = st0.get("exp_avg", torch.zeros_like(p0))
                    v0 = st0.get("exp_avg_sq", torch.zeros_like(p0))
                    p64, m64, v64, bp, bm, bv = CX.adam_step(p0, g0, m0, v0, coef, step, lr=lr, **kw)
                    worst = max(worst, X.worst(opt.state[p]["exp_avg"], m64, bm), X.worst(opt.state[p]["exp_avg_sq"], v64, bv))
                if p in plan:
                    p64 = np.clip(p64, *plan[p])                           # clipping is 1-Lipschitz: the bound carries over
                worst = max(worst, X.worst(p, p64, bp))
        w = model.lin.weight
        rec = w._qt_train_planes
        assert rec["version"] == w._version and torch.equal(rec["mfma"].words, ops.sign_pack_nib(w.detach()).words)
        assert float(w.detach().abs().max()) <= 1.0
    print(f"clipped {kind}: worst error / bound = {worst:.3f}, norm error / bound = {worst_norm:.3f}")
    assert worst <= 1.0 and worst_norm <= 1.0
    # ONE norm sequence per step over both groups (10 tensors: one chunk), then each group's launches; no unclipped entry
    assert _lib.call_counts["qt_optim_grad_sumsq_f32"] == counts["qt_optim_grad_sumsq_f32"] + 3
    assert _lib.call_counts["qt_optim_grad_norm_finalize_f32"] == counts["qt_optim_grad_norm_finalize_f32"] + 3
    assert updates == 6 * [(f"qt_optim_{kind}_f32", A.GSCALE)]


def _assert_models_equal(a, oa, b, ob, versions=True):
    """Parameters, optimiser state, planes and plane records, bit for bit.  ``versions=False``: the two took different numbers of
    steps on the host side (a skipped replay moves the version counters, ``cancel_replay``), so each record is only checked
    against its own parameter."""
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), name
        sp, sq = oa.state.get(p) or {}, ob.state.get(q) or {}
        assert set(sp) == set(sq), name
        for k in sp:
            assert torch.equal(sp[k], sq[k]) if torch.is_tensor(sp[k]) else sp[k] == sq[k], (name, k)
        wa, wb = oa._plane_words.get(p), ob._plane_words.get(q)
        assert (wa is None) == (wb is None)
        if wa is not None:
            assert torch.equal(wa, wb), name
            ra, rb = p._qt_train_planes, q._qt_train_planes
            assert ra["version"] == p._version and rb["version"] == q._version and ra["mfma"].words is wa and rb["mfma"].words is wb
            assert not versions or ra["version"] == rb["version"]
            assert torch.equal(ra["mfma"].words, rb["mfma"].words)


@pytest.mark.parametrize("form", list(SGD_FORMS) + ["adam"])
def test_a_coefficient_of_one_changes_no_bit_eagerly(dev, form):
    cls, hp = (utils.FusedQuantAdam, dict(lr=3e-3, weight_decay=1e-2)) if form == "adam" else (utils.FusedQuantSGD, SGD_FORMS[form])
    a, b = _Edge(dev, 5), _Edge(dev, 5)
    oa, ob = _two_groups(a, cls, max_grad_norm=1e30, **hp), _two_groups(b, cls, **hp)
    for step in range(3):
        a.set_grads(80 + step), b.set_grads(80 + step)
        oa.step(), ob.step()
        assert float(oa.clip_coef) == 1.0 and ob.clip_coef is None
        _assert_models_equal(a, oa, b, ob)
    assert not torch.equal(a.lin.weight, _Edge(dev, 5).lin.weight)


def test_off_route_parameters_send_the_whole_step_to_torch(dev):
    def pair():
        torch.manual_seed(9)
        ps = [torch.nn.Parameter(torch.randn(300, device=dev)), torch.nn.Parameter(torch.randn(6, 50, device=dev).t()),
              torch.nn.Parameter(torch.randn(70, device=dev))]
        assert not ps[1].is_contiguous()
        for p in ps:
            p.grad = torch.randn(p.shape, device=dev)
        return ps
    pa, pb = pair(), pair()
    oa = utils.FusedQuantSGD(pa, lr=0.1, momentum=0.9, max_grad_norm=0.5)
    ob = utils.FusedQuantSGD(pb, lr=0.1, momentum=0.9)
    raw = [p.grad.clone() for p in pa]
    before = dict(_fused.LIBRARY_PATHS)
    sumsq_calls = _lib.call_counts["qt_optim_grad_sumsq_f32"]
    with A.recorded_forms() as calls:
        oa.step()
    norm = torch.nn.utils.clip_grad_norm_(pb, 0.5)
    ob.step()
    grew = {k: v - before.get(k, 0) for k, v in _fused.LIBRARY_PATHS.items() if v != before.get(k, 0)}
    clip_keys = [k for k in grew if "clip_grad_norm_" in k]
    assert len(clip_keys) == 1 and grew[clip_keys[0]] == 1                 # counted once, not per parameter
    assert not any(form & A.GSCALE for _, form in calls) and _lib.call_counts["qt_optim_grad_sumsq_f32"] == sumsq_calls
    assert torch.equal(oa.grad_norm, norm) and float(oa.clip_coef) < 1
    for p, q, g in zip(pa, pb, raw):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad) and not torch.equal(p.grad, g)
        assert torch.equal(oa.state[p]["momentum_buffer"], ob.state[q]["momentum_buffer"])


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_steady_state_clipped_steps_do_not_synchronise(dev, kind):
    """The method of test_gpu_r2.py::test_steady_state_forwards_do_not_synchronise: torch's sync debug mode raises on any."""
    model = _Edge(dev, 6)
    opt = (utils.FusedQuantSGD(model, lr=0.05, momentum=0.9, max_grad_norm=1.0) if kind == "sgd"
           else utils.FusedQuantAdam(model, lr=1e-3, max_grad_norm=1.0))
    model.set_grads(90)
    opt.step()                                                             # allocations
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            opt.step()
        norm = opt.grad_norm
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(norm) > 1.0                                               # reading it is the caller's synchronise


# ---- 4. inside GraphedTrainStep -------------------------------------------------------------------------------------------------

def _make_opt(kind, **kw):
    return lambda m: C.OPTS[kind](m, emit_planes=True, **kw)


def _captured(dev, kind, recover=False, **kw):
    model = C._mlp(dev)
    opt = _make_opt(kind, **kw)(model)
    (x, t), = C._batches(dev, 1, seed=5)
    step = utils.GraphedTrainStep(model, C._loss, x, t, optimizer=opt, recover=recover)
    return model, opt, step, C.Twin(model, opt, lambda: C._mlp(dev), _make_opt(kind, **kw))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_coefficient_of_one_changes_no_bit_in_a_captured_step(dev, kind):
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, _ = _captured(dev, kind, max_grad_norm=1e30)
        plain_model, plain_opt, plain, _ = _captured(dev, kind)
        for x, t in C._batches(dev, 3):
            assert torch.equal(step(x, t), plain(x, t))
            assert float(opt.clip_coef) == 1.0 and float(opt.grad_norm) > 0
            _assert_models_equal(model, opt, plain_model, plain_opt)
            for p, q in zip(model.parameters(), plain_model.parameters()):
                assert torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_captured_clipped_step_equals_the_eager_one_and_repeats(dev, kind):
    """784-256-10 binary MLP, batch 64, 3 steps: every replay equals the eager clipped step of the twin on the same gradients, a
    second run from the same state gives the same bits, and a new max_grad_norm reaches the next replay."""
    with _fused.scope(GEMM_IMPL="mfma"):
        finals = []
        for run in range(2):
            model, opt, step, twin = _captured(dev, kind, max_grad_norm=0.25)
            coefs = []
            for call, (x, t) in enumerate(C._batches(dev, 3)):
                if call == 2:
                    opt.max_grad_norm = twin.twin_opt.max_grad_norm = 0.125
                twin.before()
                step(x, t)
                assert twin.after() == 2
                norm, coef = opt.grad_norm.cpu().numpy(), opt.clip_coef.cpu().numpy()
                assert coef.view(np.uint32) == CX.coef_f32(norm, opt.max_grad_norm).view(np.uint32) and coef < 1
                assert torch.equal(opt.grad_norm, twin.twin_opt.grad_norm) and torch.equal(opt.clip_coef, twin.twin_opt.clip_coef)
                norm64 = CX.total_norm([p.grad for p in model.parameters()])
                assert abs(float(norm) - norm64) <= CX.norm_bound(norm64)
                coefs.append(float(coef))
            finals.append(([p.detach().clone() for p in model.parameters()], coefs))
        assert finals[0][1] == finals[1][1] and all(torch.equal(p, q) for p, q in zip(finals[0][0], finals[1][0]))
        # switching clipping off (or on) after the capture: the launches are baked
        (x, t), = C._batches(dev, 1)
        opt.max_grad_norm = None
        steps = [float(opt.state[p].get("step", 0.0)) for p in model.parameters()]
        with pytest.raises(RuntimeError, match="captured"):
            step(x, t)
        assert steps == [float(opt.state[p].get("step", 0.0)) for p in model.parameters()]
        plain_model, plain_opt, plain, _ = _captured(dev, kind)
        plain_opt.max_grad_norm = 1.0
        with pytest.raises(RuntimeError, match="captured"):
            plain(x, t)


def test_captured_clipped_steps_do_not_synchronise(dev):
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, _ = _captured(dev, "adam", max_grad_norm=0.25)
        batches = C._batches(dev, 3)
        step(*batches[0])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for x, t in batches[1:]:
                step(x, t)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert float(opt.clip_coef) < 1


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_a_skipped_clipped_update_touches_nothing(dev, kind):
    """recover=True with clipping, by the forced verdict of tests/test_gpu_graph_recover.py: the step is captured on +-1 inputs, so
    the first LinearBin's remembered "+-1" verdict is wrong for a real-valued batch and the replay raises the guard.  The norm
    launches run all the same, but they write only the capture's workspace and (norm, coef) words: parameters, optimiser state and
    planes are bit-identical after the replay, and settling gives the eager clipped step.  No launch here can fault: a raised
    guard only makes the update's workgroups return."""
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, twin = _captured(dev, kind, recover=True, max_grad_norm=0.25)
        plain_model, plain_opt, plain, _ = _captured(dev, kind, max_grad_norm=0.25)
        assert step._armed
        (x, t), = C._batches(dev, 1)
        assert torch.equal(step(x, t), plain(x, t)) and step.settle() is False          # a clear guard costs no bit
        _assert_models_equal(model, opt, plain_model, plain_opt)

        g = torch.Generator().manual_seed(41)
        x, t = torch.randn(64, 784, generator=g).to(dev), torch.randint(0, 10, (64,), generator=g).to(dev)
        twin.before()
        params = [p.detach().clone() for p in model.parameters()]
        state = [{k: v.clone() for k, v in opt.state[p].items() if torch.is_tensor(v) and v.is_cuda} for p in model.parameters()]
        planes = {p: w.clone() for p, w in opt._plane_words.items()}
        assert len(planes) == 2
        loss = step(x, t)
        torch.cuda.synchronize()
        for p, p0, st0 in zip(model.parameters(), params, state):                       # the replay, before it is settled
            assert torch.equal(p, p0)
            for k, v in st0.items():
                assert torch.equal(opt.state[p][k], v), k
        for p, w in planes.items():
            assert torch.equal(opt._plane_words[p], w)
        assert step.settle() is True and step.recoveries == 1
        twin.twin_opt.zero_grad()
        want = C._loss(twin.twin(x), t)
        want.backward()
        twin.twin_opt.step()
        assert torch.equal(loss, want.detach()) and bool(torch.isfinite(loss))
        _assert_models_equal(model, opt, twin.twin, twin.twin_opt, versions=False)
        assert float(opt.clip_coef) < 1 and torch.equal(opt.clip_coef, twin.twin_opt.clip_coef)
        loss = step(*C._batches(dev, 1, seed=23)[0])                                     # and on it goes, clipped
        assert step.settle() is False and bool(torch.isfinite(loss)) and float(opt.clip_coef) < 1
