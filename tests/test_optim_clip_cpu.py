"""Gradient-norm clipping of FusedQuantSGD / FusedQuantAdam without a GPU: the bounds of tests/_clip_exact.py pinned against
torch's own fp32 ``clip_grad_norm_`` + optimiser, argument validation, the library path on host tensors (bit equality with torch),
the unchanged ``state_dict()`` / ``param_groups``, and the norm entries' declarations and statuses (nothing that passes validation
here has anything to enqueue; the clipped update's own statuses, QT_OPTIM_GSCALE, are in tests/test_optim_abi.py)."""
import ctypes

import numpy as np
import pytest
import torch

import _clip_exact as CX
import _optim_exact as X
from _optim_abi import table as _table
from pytorch_quantize_impls_amd import _lib, ops, utils
from pytorch_quantize_impls_amd.functions import _fused

INVALID, ALIGNMENT = -1, -2
DEVPTR = 0x6000             # never dereferenced on the host
NEW_ENTRIES = ("qt_optim_grad_norm_work_floats", "qt_optim_grad_sumsq_f32", "qt_optim_grad_norm_finalize_f32")

SIZES = [4099, 1, 517, 8192]          # the gradients of one clipped step: the norm is global over all of them
MAX_NORM = 10.0                       # far below the norm of X.inputs gradients (entries up to 100): the clip acts
SGD_VARIANTS = [dict(lr=0.05), dict(lr=0.05, momentum=0.9, weight_decay=1e-3),
                dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)]
ADAM_VARIANTS = [dict(lr=1e-3), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)]


def _params(seed):
    return [torch.nn.Parameter(torch.from_numpy(X.inputs(seed + i, (n,))[0].copy())) for i, n in enumerate(SIZES)]


def _set_grads(params, seed, step):
    grads = [X.inputs(seed + 31 * i, (n,), step=step)[1] for i, n in enumerate(SIZES)]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy())
    return grads


def _torch_clip(params, grads):
    """torch's own fp32 clip, checked on the way: its norm lies inside the norm bound, its coefficient is an fp32 function of its
    fp32 norm (torch writes ``max_norm / tensor``, which it evaluates as ``tensor.reciprocal() * max_norm``: within one ulp of
    ``coef_f32``, the division the kernel performs), and the gradients it leaves are g * coef, one fp32 product each.  Returns
    that coefficient (numpy float32) and the norm's error over its bound."""
    norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    assert norm.dtype == torch.float32
    norm64 = CX.total_norm(grads)
    assert norm64 > 100 * MAX_NORM
    ratio = abs(float(norm) - norm64) / CX.norm_bound(norm64)
    coef = torch.clamp(MAX_NORM / (norm + 1e-6), max=1.0).numpy()[()]
    assert coef.dtype == np.float32 and coef < 1
    assert abs(float(coef) - float(CX.coef_f32(np.float32(norm.item()), MAX_NORM))) <= float(np.spacing(coef))
    for p, g in zip(params, grads):
        assert np.array_equal(p.grad.numpy(), g * coef)
    return coef, ratio


def test_torch_norm_is_inside_the_bound():
    params = _params(1)
    worst = 0.0
    for step in range(1, 6):
        _, ratio = _torch_clip(params, _set_grads(params, 100 * step, step))
        worst = max(worst, ratio)
    print(f"torch clip_grad_norm_: worst norm error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_coef_f32_is_the_fp32_division():
    for norm in (0.0, 1e-7, 0.5, 9.999999, 10.0, 256.0, 3.4e38, float("inf"), float("nan")):
        t = torch.tensor(norm, dtype=torch.float32)
        want = torch.clamp(torch.tensor(MAX_NORM) / (t + 1e-6), max=1.0).numpy()          # tensor / tensor: a true division
        got = CX.coef_f32(np.float32(norm), MAX_NORM)
        assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), norm
    assert CX.coef_f32(np.float32("inf"), 1.0) == 0 and np.isnan(CX.coef_f32(np.float32("nan"), 1.0))
    assert CX.coef_f32(np.float32(256.0), 64.0) == np.float32(64.0) / (np.float32(256.0) + np.float32(1e-6))


@pytest.mark.parametrize("hp", SGD_VARIANTS, ids=["plain", "momentum_wd", "nesterov"])
def test_torch_clipped_sgd_is_inside_the_bound(hp):
    params = _params(3)
    opt = torch.optim.SGD(params, foreach=False, **hp)
    worst = 0.0
    for step in range(1, 6):
        grads = _set_grads(params, 10 + step, step)
        before = [p.detach().clone() for p in params]
        bufs = [opt.state[p].get("momentum_buffer") for p in params]
        bufs = [None if b is None else b.clone() for b in bufs]
        coef, _ = _torch_clip(params, grads)
        opt.step()
        for p, p0, g, buf in zip(params, before, grads, bufs):
            p64, b64, bp, bb = CX.sgd_step(p0, g, buf, coef, **hp)
            worst = max(worst, X.worst(p, p64, bp))
            if b64 is not None:
                worst = max(worst, X.worst(opt.state[p]["momentum_buffer"], b64, bb))
    print(f"clip_grad_norm_ + torch.optim.SGD {hp}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("hp", ADAM_VARIANTS, ids=["default", "custom"])
def test_torch_clipped_adam_is_inside_the_bound(hp):
    params = _params(4)
    opt = torch.optim.Adam(params, foreach=False, **hp)
    worst = 0.0
    for step in range(1, 6):
        grads = _set_grads(params, 20 + step, step)
        before = [p.detach().clone() for p in params]
        ms = [opt.state[p]["exp_avg"].clone() if opt.state[p] else torch.zeros_like(p) for p in params]
        vs = [opt.state[p]["exp_avg_sq"].clone() if opt.state[p] else torch.zeros_like(p) for p in params]
        coef, _ = _torch_clip(params, grads)
        opt.step()
        for p, p0, g, m, v in zip(params, before, grads, ms, vs):
            p64, m64, v64, bp, bm, bv = CX.adam_step(p0, g, m, v, coef, step, **hp)
            st = opt.state[p]
            worst = max(worst, X.worst(p, p64, bp), X.worst(st["exp_avg"], m64, bm), X.worst(st["exp_avg_sq"], v64, bv))
    print(f"clip_grad_norm_ + torch.optim.Adam {hp}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_the_clipped_bounds_are_the_unclipped_ones_plus_one_rounding():
    assert CX.SGD_CLIP_ROUNDINGS == X.SGD_ROUNDINGS + 1 and CX.ADAM_CLIP_ROUNDINGS == X.ADAM_ROUNDINGS + 1
    assert CX.NORM_ROUNDINGS == 32 >= 1 + 16 + 7 + 3 + 1 + 1
    p, g = X.inputs(9, (64,))
    a, b = X.sgd_step(p, g.astype(np.float64) * 0.25, None, 0.1), CX.sgd_step(p, g, None, np.float32(0.25), 0.1)
    assert np.array_equal(a[0], b[0]) and np.allclose(b[2], a[2] * 9 / 8, rtol=1e-15)


# ---- the optimisers ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [utils.FusedQuantSGD, utils.FusedQuantAdam])
def test_max_grad_norm_must_be_positive_and_finite(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1", True, torch.tensor(1.0)):
        with pytest.raises(ValueError, match="max_grad_norm"):
            cls(p, max_grad_norm=bad)
    opt = cls(p, max_grad_norm=2)
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.max_grad_norm = -3.0
    assert opt.max_grad_norm == 2.0
    opt.max_grad_norm = None
    assert opt.max_grad_norm is None and cls(p).max_grad_norm is None
    assert opt.grad_norm is None and opt.clip_coef is None
    with pytest.raises(TypeError):
        cls(p, norm_type=2.0)                                 # L2 only: there is no such argument


@pytest.mark.parametrize("cls,ref", [(utils.FusedQuantSGD, torch.optim.SGD), (utils.FusedQuantAdam, torch.optim.Adam)])
def test_no_group_key_and_an_unchanged_state_dict(cls, ref):
    def make(**kw):
        torch.manual_seed(0)
        ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))]
        return ps, cls([{"params": ps[:1]}, {"params": ps[1:], "lr": 0.5}], **kw)
    (pa, a), (pb, b), (pc, c) = make(), make(max_grad_norm=None), make(max_grad_norm=1.5)
    want_keys = set(ref([torch.nn.Parameter(torch.zeros(1))]).param_groups[0])
    for opt in (a, b, c):
        assert all(set(g) == want_keys for g in opt.param_groups)
        assert all("max_grad_norm" not in g for g in opt.state_dict()["param_groups"]) and "max_grad_norm" not in opt.defaults
    for ps, opt in ((pa, a), (pb, b)):
        for p in ps:
            p.grad = torch.full_like(p, 0.25)
        opt.step()
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] == c.state_dict()["param_groups"]
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        assert all(torch.equal(sa["state"][k][n], sb["state"][k][n]) for n in sa["state"][k])
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))


def _host_pair(seed):
    torch.manual_seed(seed)
    a = torch.nn.Sequential(torch.nn.Linear(12, 9), torch.nn.Tanh(), torch.nn.Linear(9, 4))
    b = torch.nn.Sequential(torch.nn.Linear(12, 9), torch.nn.Tanh(), torch.nn.Linear(9, 4))
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_host_tensors_take_the_library_path_and_equal_torch(kind):
    a, b = _host_pair(3)
    if kind == "sgd":
        opt, ref = utils.FusedQuantSGD(a.parameters(), lr=0.1, momentum=0.9, max_grad_norm=0.05), torch.optim.SGD(b.parameters(), lr=0.1, momentum=0.9)
    else:
        opt, ref = utils.FusedQuantAdam(a.parameters(), lr=1e-2, max_grad_norm=0.05), torch.optim.Adam(b.parameters(), lr=1e-2)
    before = dict(_fused.LIBRARY_PATHS)
    torch.manual_seed(4)
    for _ in range(3):
        x = torch.randn(16, 12)
        for model, o in ((a, opt), (b, ref)):
            o.zero_grad()
            model(x).square().sum().backward()
        raw = [p.grad.clone() for p in a.parameters()]
        norm = torch.nn.utils.clip_grad_norm_(b.parameters(), 0.05)
        opt.step(), ref.step()
        assert float(norm) > 0.05
        assert torch.equal(opt.grad_norm, norm) and opt.grad_norm.dim() == 0 and opt.grad_norm.dtype == torch.float32
        assert torch.equal(opt.clip_coef, torch.clamp(0.05 / (norm + 1e-6), max=1.0))
        for p, q, g in zip(a.parameters(), b.parameters(), raw):
            assert torch.equal(p, q)
            assert torch.equal(p.grad, q.grad) and not torch.equal(p.grad, g)       # rewritten in place, as torch does
    assert dict(_fused.LIBRARY_PATHS) == before                  # the counter is about device tensors


# ---- the C entries -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    declared = _lib.header_declared_functions()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.SIGNATURES
        fn = getattr(lib, name)                                  # exported
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0]
    assert _lib.SIGNATURES["qt_optim_grad_norm_work_floats"][0] is ctypes.c_int64


def test_workspace_size(lib):
    work = lib.qt_optim_grad_norm_work_floats
    assert work(None, 0) == 0 and work(None, 2) == INVALID and work(ctypes.addressof(_table()), -1) == INVALID
    for numel, units in ((0, 0), (1, 1), (3, 1), (4095, 1), (4096, 1), (4097, 2), (2 * 4096 + 5, 3), (1 << 33, 1 << 21)):
        assert work(ctypes.addressof(_table(numel=numel)), 1) == units, numel
    tab = _table(70, numel=4097)
    tab[3].numel, tab[3].g = 0, None                             # an empty tensor has no unit and needs no pointer
    assert work(ctypes.addressof(tab), 70) == 69 * 2
    # a plane tensor's gradient is flat memory: rows / K / ld play no part
    assert work(ctypes.addressof(_table(numel=64, kind=1, rows=2, K=32, ld=4, words=0x5000)), 1) == 1
    assert work(ctypes.addressof(_table(numel=-4)), 1) == INVALID
    assert work(ctypes.addressof(_table(g=None)), 1) == INVALID
    assert work(ctypes.addressof(_table(g=0x2002)), 1) == ALIGNMENT


def test_sumsq_and_finalise_statuses(lib):
    sumsq, fin = lib.qt_optim_grad_sumsq_f32, lib.qt_optim_grad_norm_finalize_f32
    tab = ctypes.addressof(_table())
    assert sumsq(None, 0, None, None) == 0 and sumsq(tab, 0, 0x1002, None) == 0          # nothing to do
    assert sumsq(None, 1, DEVPTR, None) == INVALID and sumsq(tab, -1, DEVPTR, None) == INVALID
    assert sumsq(tab, 1, None, None) == INVALID                                          # null workspace
    assert sumsq(tab, 1, DEVPTR + 2, None) == ALIGNMENT
    assert sumsq(ctypes.addressof(_table(g=None)), 1, DEVPTR, None) == INVALID
    assert sumsq(ctypes.addressof(_table(g=0x2002)), 1, DEVPTR, None) == ALIGNMENT
    assert sumsq(ctypes.addressof(_table(numel=-1)), 1, DEVPTR, None) == INVALID
    assert fin(DEVPTR, -1, 1.0, None, DEVPTR, None) == INVALID
    assert fin(None, 4, 1.0, None, DEVPTR, None) == INVALID and fin(DEVPTR, 4, 1.0, None, None, None) == INVALID
    assert fin(DEVPTR + 2, 4, 1.0, None, DEVPTR, None) == ALIGNMENT and fin(DEVPTR, 4, 1.0, None, DEVPTR + 1, None) == ALIGNMENT
    assert fin(DEVPTR, 4, 1.0, DEVPTR + 2, DEVPTR, None) == ALIGNMENT


def test_wrappers_reject_host_tensors_and_ambiguous_max_norm():
    g = torch.zeros(4)
    with pytest.raises(ValueError, match="exactly one"):
        ops.optim_grad_norm([g], g, g[:2])
    with pytest.raises(ValueError, match="exactly one"):
        ops.optim_grad_norm([g], g, g[:2], max_norm=1.0, max_norm_dev=g[:1])
    with pytest.raises(TypeError):
        ops.optim_grad_norm([g], g, g[:2], max_norm=1.0)
    with pytest.raises(TypeError):
        ops.optim_grad_norm_work_floats([g])
