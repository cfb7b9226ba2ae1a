"""``GraphedTrainStep(recover=True)``: the guarded training update (QT_OPTIM_SKIP) and the flag OR (csrc/optim_step.hip), and a captured step
that meets a wrong remembered verdict (utils/graphs.py).  Every comparison is bit equality against a step that cannot be wrong in the
same way: the unguarded update, a ``recover=False`` replay while no verdict flips, and the plain eager loop in "verify" mode
on the call that flips one.  The MLP, its batches, optimisers and the state twin are those of tests/test_gpu_optim_capture.py."""
import warnings

import pytest
import torch

import _optim_abi as A
import test_gpu_optim_capture as C
from pytorch_quantize_impls_amd import _lib, ops, utils
from pytorch_quantize_impls_amd.functions import _fused, nnDorefaQuant
from pytorch_quantize_impls_amd.layers import LinearDorefa

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


# ---- 1. the guarded entries -----------------------------------------------------------------------------------------------------

# every walk of the kernel: two full 4096-element units + a guarded last unit with a numel % 4 tail; a tensor below one vector
# unit; a view one element into its storage (4-byte aligned only: the dword walk); an empty tensor; a sign plane with K % 8 != 0
# and pad words (ld = 8 for 5 used words); a ternary plane
TABLE = [4096 + 4096 + 5, 7, "view", 0, (3, 40, "binary"), (2, 32, "ternary")]
SENTINEL = 0x5A5A5A5A


def _table(dev, seed):
    g = torch.Generator().manual_seed(seed)
    ps, gs, s0, s1, clamps, planes = [], [], [], [], [], []
    for i, size in enumerate(TABLE):
        shape = size[:2] if isinstance(size, tuple) else ((100,) if size == "view" else (size,))
        p = torch.randn(shape, generator=g).to(dev)
        if size == "view":
            base = torch.zeros(101, device=dev)
            base[1:].copy_(p)
            p = base[1:]
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        ps.append(p)
        gs.append(torch.randn(shape, generator=g).to(dev))
        s0.append((torch.randn(shape, generator=g) * 1e-2).to(dev))
        s1.append((torch.randn(shape, generator=g).abs() * 1e-2).to(dev))
        clamps.append((-1.0, 1.0) if i % 2 == 0 else None)
        if isinstance(size, tuple):
            rows, K, kind = size
            words = torch.full((rows, C._plane_ld(K)), SENTINEL, dtype=torch.int32, device=dev)
            planes.append((ops.NibPlanes(words=words, rows=rows, K=K), kind))
        else:
            planes.append(None)
    assert C._plane_ld(40) == 8 and (40 + 7) // 8 == 5
    return ps, gs, s0, s1, clamps, planes


def _snapshot(tab):
    return [[t.clone() for t in lst] for lst in tab[:4]] + [[pl[0].words.clone() for pl in tab[5] if pl is not None]]


def _assert_same(a, b):
    for k in range(4):
        C._same(a[k], b[k])
    C._same_planes(a[5], b[5])


def _assert_untouched(tab, snap):
    for k in range(4):
        C._same(tab[k], snap[k])
    words = [pl[0].words for pl in tab[5] if pl is not None]
    C._same(words, snap[4])
    assert all(bool((w == SENTINEL).all()) for w in words)


SGD_FORMS = {"plain": dict(), "momentum": dict(momentum=0.9, weight_decay=1e-3), "nesterov": dict(momentum=0.9, nesterov=True)}


@pytest.mark.parametrize("form", list(SGD_FORMS))
def test_guarded_sgd_entry(dev, form):
    hp = SGD_FORMS[form]
    mom = "momentum" in hp
    lr = torch.tensor([0.05], dtype=torch.float32, device=dev)
    a, b, c = _table(dev, 7), _table(dev, 7), _table(dev, 7)
    before = _snapshot(c)
    ops.optim_step_sgd_dev(a[0], a[1], a[2] if mom else None, lr, clamps=a[4], planes=a[5], **hp)
    ops.optim_step_sgd_dev(b[0], b[1], b[2] if mom else None, lr, clamps=b[4], planes=b[5],
                           skip=torch.zeros(1, dtype=torch.int32, device=dev), **hp)
    ops.optim_step_sgd_dev(c[0], c[1], c[2] if mom else None, lr, clamps=c[4], planes=c[5],
                           skip=torch.ones(1, dtype=torch.int32, device=dev), **hp)
    _assert_same(a, b)                                   # a clear guard: the bits of the unguarded entry
    _assert_untouched(c, before)                         # a raised one: parameters, state, planes and gradients as they were
    assert all(not torch.equal(p, q) for p, q in zip(a[0], before[0]) if p.numel())          # ... and the update is one
    assert all(not bool((pl[0].words == SENTINEL).any()) for pl in a[5] if pl is not None)


def test_guarded_adam_entry(dev):
    hp = dict(betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)
    steps = list(range(1, len(TABLE) + 1))
    coef = torch.tensor(ops.adam_coefficients(steps, 3e-3, hp["betas"]), dtype=torch.float32, device=dev).reshape(-1)
    a, b, c = _table(dev, 8), _table(dev, 8), _table(dev, 8)
    before = _snapshot(c)
    ops.optim_step_adam_dev(a[0], a[1], a[2], a[3], coef, clamps=a[4], planes=a[5], **hp)
    ops.optim_step_adam_dev(b[0], b[1], b[2], b[3], coef, clamps=b[4], planes=b[5],
                            skip=torch.zeros(1, dtype=torch.int32, device=dev), **hp)
    ops.optim_step_adam_dev(c[0], c[1], c[2], c[3], coef, clamps=c[4], planes=c[5],
                            skip=torch.ones(1, dtype=torch.int32, device=dev), **hp)
    _assert_same(a, b)
    _assert_untouched(c, before)
    assert all(not torch.equal(p, q) for p, q in zip(a[0], before[0]) if p.numel())
    assert all(not torch.equal(m, q) for m, q in zip(a[2], before[2]) if m.numel())
    with pytest.raises(ValueError):
        ops.optim_step_adam_dev(c[0], c[1], c[2], c[3], coef, skip=torch.zeros(2, dtype=torch.int32, device=dev), **hp)
    with pytest.raises(ValueError):
        ops.optim_step_adam_dev(c[0], c[1], c[2], c[3], coef, skip=torch.zeros(1, device=dev), **hp)


# ---- 2. the flag OR -------------------------------------------------------------------------------------------------------------

def test_flags_or(dev):
    cap = ops.flags_chunk_capacity()
    for n in (1, 3, cap, cap + 1):
        buf = torch.zeros(n, dtype=torch.int32, device=dev)
        flags = [buf[i:i + 1] for i in range(n)]
        guard = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.flags_or(flags, guard)
        assert int(guard) == 0, n                        # all clear
        buf[n - 1] = 4                                   # the last position of the last chunk; any non-zero value raises
        ops.flags_or(flags, guard)
        assert int(guard) == 1, n
        buf.zero_()
        ops.flags_or(flags, guard)
        assert int(guard) == 1, n                        # a raised guard stays raised
    guard = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.flags_or([], guard)
    assert int(guard) == 0
    with pytest.raises(ValueError):
        ops.flags_or([torch.zeros(2, dtype=torch.int32, device=dev)], guard)


# ---- 3 - 7. captured steps ------------------------------------------------------------------------------------------------------

def _real_batches(dev, n, seed=41):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(64, 784, generator=g).to(dev), torch.randint(0, 10, (64,), generator=g).to(dev)) for _ in range(n)]


def _assert_pairs_equal(model, opt, other, other_opt, grads=True):
    """Parameters, gradients, optimiser state (step counts included), module buffers and weight planes: bit for bit."""
    for (name, p), q in zip(model.named_parameters(), other.parameters()):
        assert torch.equal(p, q), name
        if grads:
            assert torch.equal(p.grad, q.grad), name
        sp, sq = opt.state.get(p) or {}, other_opt.state.get(q) or {}
        assert set(sp) == set(sq), name
        for k in C._state_keys(opt):
            assert torch.equal(sp[k], sq[k]), (name, k)
        if "step" in sp:
            assert float(sp["step"]) == float(sq["step"]), name
        words = opt._plane_words.get(p)
        if words is not None:
            assert torch.equal(words, other_opt._plane_words[q]), name
    for (name, b), c in zip(model.named_buffers(), other.buffers()):
        assert torch.equal(b, c), name


def _all_finite(model, opt):
    ts = list(model.parameters()) + list(model.buffers()) + [v for st in opt.state.values() for v in st.values() if torch.is_tensor(v)]
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


def _sync_into(ref_model, ref_opt, model, opt):
    """Values of ``model`` / ``opt`` copied INTO the tensors a captured step of ``ref_model`` / ``ref_opt`` holds."""
    ref_model.load_state_dict(model.state_dict())
    for p, q in zip(model.parameters(), ref_model.parameters()):
        for k, v in opt.state[p].items():
            ref_opt.state[q][k].copy_(v)
    ref_opt.param_groups[0]["lr"] = opt.param_groups[0]["lr"]


def _eager_twin_step(twin, x, t, loss_fn):
    """The plain loop, in the default "verify" mode, on the twin that took over the pre-call state."""
    assert _fused.detect_mode() == "verify"
    twin.twin_opt.zero_grad()
    loss = loss_fn(twin.twin(x), t)
    loss.backward()
    twin.twin_opt.step()
    return loss.detach()


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_pm1_verdict_flip_is_recovered(dev, kind):
    make_opt = lambda m: C.OPTS[kind](m, emit_planes=True)                 # noqa: E731
    with _fused.scope(GEMM_IMPL="mfma"):
        (x0, t0), = C._batches(dev, 1, seed=5)
        pm, real = C._batches(dev, 3), _real_batches(dev, 2)
        model, plain_model = C._mlp(dev), C._mlp(dev)
        opt, plain_opt = make_opt(model), make_opt(plain_model)
        assert any(isinstance(m, torch.nn.BatchNorm1d) for m in model.modules())
        flags_or = _lib.call_counts["qt_flags_or_i32"]
        with A.recorded_forms() as calls:
            step = utils.GraphedTrainStep(model, C._loss, x0, t0, optimizer=opt, recover=True)
        plain = utils.GraphedTrainStep(plain_model, C._loss, x0, t0, optimizer=plain_opt)
        assert step._armed and len(step._flags) >= 1                      # the un-tagged +-1 input of the first LinearBin
        assert any(name == A.ENTRIES[kind] and form & A.SKIP for name, form in calls)
        assert _lib.call_counts["qt_flags_or_i32"] > flags_or

        # +-1, +-1: nothing flips, and a clear guard costs no bit against the step without one
        for x, t in pm[:2]:
            loss = step(x, t)
            assert step.settle() is False
            assert torch.equal(loss, plain(x, t))
            _assert_pairs_equal(model, opt, plain_model, plain_opt)
        assert step.recoveries == step.recaptures == 0

        # randn: the remembered "+-1" is wrong
        twin = C.Twin(model, opt, lambda: C._mlp(dev), make_opt)
        twin.before()
        tracked = int(model[1].num_batches_tracked)
        x, t = real[0]
        loss = step(x, t)
        assert step.settle() is True and step.recoveries == step.recaptures == 1
        assert step.settle() is False                                      # settled is settled
        want = _eager_twin_step(twin, x, t, C._loss)
        assert torch.equal(loss, want) and bool(torch.isfinite(loss))
        _assert_pairs_equal(model, opt, twin.twin, twin.twin_opt)
        assert int(model[1].num_batches_tracked) == tracked + 1
        if kind == "adam":
            assert all(float(opt.state[p]["step"]) == 3 for p in model.parameters())

        # what the step without recovery makes of the same batch
        bad = plain(x, t)
        assert not (bool(torch.isfinite(bad)) and _all_finite(plain_model, plain_opt))

        # afterwards: the negative verdict is remembered, nothing is armed, and the step is the one a fresh capture on a real-valued
        # batch gives
        ref_model = C._mlp(dev)
        ref_opt = make_opt(ref_model)
        ref = utils.GraphedTrainStep(ref_model, C._loss, *real[0], optimizer=ref_opt)
        _sync_into(ref_model, ref_opt, model, opt)
        for x, t in (pm[2], real[1]):
            loss = step(x, t)
            assert step.settle() is False
            assert torch.equal(loss, ref(x, t)) and bool(torch.isfinite(loss))
            _assert_pairs_equal(model, opt, ref_model, ref_opt)
            assert _all_finite(model, opt)
        assert step.recoveries == step.recaptures == 1


def _dorefa_net(dev):
    torch.manual_seed(33)
    return torch.nn.Sequential(nnDorefaQuant(4), LinearDorefa(64, 32, bit_width=1), torch.nn.Linear(32, 10)).to(dev).train()


def test_code_range_flip_is_recovered(dev):
    """nnDorefaQuant(4) does not clamp: inputs in [0, 1] give codes up to 15, inputs up to 20 codes up to 300, beyond int8."""
    make_opt = lambda m: utils.FusedQuantAdam(m, lr=1e-2)                  # noqa: E731
    g = torch.Generator().manual_seed(34)
    data = [(torch.rand(16, 64, generator=g).to(dev), torch.randint(0, 10, (16,), generator=g).to(dev)) for _ in range(3)]
    model, plain_model = _dorefa_net(dev), _dorefa_net(dev)
    opt, plain_opt = make_opt(model), make_opt(plain_model)
    step = utils.GraphedTrainStep(model, C._loss, *data[0], optimizer=opt, recover=True)
    plain = utils.GraphedTrainStep(plain_model, C._loss, *data[0], optimizer=plain_opt)
    assert step._armed                                                     # the int8 route of the first layer trusts codes.overflow
    x, t = data[1]
    loss = step(x, t)
    assert step.settle() is False and torch.equal(loss, plain(x, t))
    _assert_pairs_equal(model, opt, plain_model, plain_opt)

    twin = C.Twin(model, opt, lambda: _dorefa_net(dev), make_opt)
    twin.before()
    x, t = data[2][0] * 20.0, data[2][1]
    assert float(x.max()) * 15 > 127
    loss = step(x, t)
    assert step.settle() is True                                           # the guard was raised
    assert step.recoveries == 1 and step.recaptures == 1
    want = _eager_twin_step(twin, x, t, C._loss)
    assert torch.equal(loss, want) and bool(torch.isfinite(loss))
    _assert_pairs_equal(model, opt, twin.twin, twin.twin_opt)
    assert all(float(opt.state[p]["step"]) == 2 for p in model.parameters())
    assert not bool(torch.isfinite(plain(x, t)))                           # without recovery: NaN
    loss = step(*data[1])                                                  # and on it goes, nothing armed any more
    assert step.settle() is False and step.recoveries == 1 and bool(torch.isfinite(loss)) and _all_finite(model, opt)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_schedule_and_eager_steps_after_a_recovery(dev, kind):
    make_opt = lambda m: C.OPTS[kind](m, emit_planes=True)                 # noqa: E731
    with _fused.scope(GEMM_IMPL="mfma"):
        (x0, t0), = C._batches(dev, 1, seed=5)
        real = _real_batches(dev, 3)
        model = C._mlp(dev)
        opt = make_opt(model)
        step = utils.GraphedTrainStep(model, C._loss, x0, t0, optimizer=opt, recover=True)
        step(*real[0])
        assert step.settle() is True
        twin = C.Twin(model, opt, lambda: C._mlp(dev), make_opt)
        opt.param_groups[0]["lr"] *= 0.25                                  # reaches the re-captured graph's scalar block
        twin.before()
        assert twin.twin_opt.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
        step(*real[1])
        assert step.settle() is False
        assert twin.after() == 2
        twin.before()
        opt.step()                                                         # eagerly, on the gradients the replay left
        assert twin.after() == 2
        twin.before()
        step(*real[2])
        assert step.settle() is False and twin.after() == 2
        if kind == "adam":
            assert all(float(opt.state[p]["step"]) == 4 for p in model.parameters())


def test_no_recaptures_left_means_eager_for_good(dev):
    make_opt = lambda m: C.OPTS["adam"](m, emit_planes=True)               # noqa: E731
    with _fused.scope(GEMM_IMPL="mfma"):
        (x0, t0), = C._batches(dev, 1, seed=5)
        real = _real_batches(dev, 2)
        model = C._mlp(dev)
        opt = make_opt(model)
        step = utils.GraphedTrainStep(model, C._loss, x0, t0, optimizer=opt, recover=True, max_recaptures=0)
        twin = C.Twin(model, opt, lambda: C._mlp(dev), make_opt)
        twin.before()
        with pytest.warns(RuntimeWarning, match="stays eager") as seen:
            loss = step(*real[0])
            assert step.settle() is True
        assert len([w for w in seen if "stays eager" in str(w.message)]) == 1
        assert step.recoveries == 1 and step.recaptures == 0 and step._eager
        assert torch.equal(loss, _eager_twin_step(twin, *real[0], C._loss))
        _assert_pairs_equal(model, opt, twin.twin, twin.twin_opt)
        twin.before()
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*stays eager.*")    # warned once, not per call
            loss = step(*real[1])
            assert step.settle() is False
        assert torch.equal(loss, _eager_twin_step(twin, *real[1], C._loss))
        _assert_pairs_equal(model, opt, twin.twin, twin.twin_opt)


def test_recover_without_a_captured_optimiser_settles_in_the_call(dev):
    with _fused.scope(GEMM_IMPL="mfma"):
        (x0, t0), = C._batches(dev, 1, seed=5)
        (x, t), = _real_batches(dev, 1)
        model, other = C._mlp(dev), C._mlp(dev)
        step = utils.GraphedTrainStep(model, C._loss, x0, t0, recover=True)
        other.load_state_dict(model.state_dict())
        loss = step(x, t)
        assert step.recoveries == 1 and not step._pending                  # settled before the caller's optimiser runs
        want = C._loss(other(x), t)
        want.backward()
        assert torch.equal(loss, want.detach())
        for p, q in zip(model.parameters(), other.parameters()):
            assert torch.equal(p.grad, q.grad) and bool(torch.isfinite(p.grad).all())
        for b, c in zip(model.buffers(), other.buffers()):
            assert torch.equal(b, c)


def test_default_step_calls_none_of_the_new_entries(dev):
    with _fused.scope(GEMM_IMPL="mfma"):
        flags_or = _lib.call_counts["qt_flags_or_i32"]
        with A.recorded_forms() as calls:
            model, opt, step, _ = C._captured(dev, "adam")
            assert not step.recover
            for x, t in C._batches(dev, 2):
                step(x, t)
        assert not hasattr(step, "_guard")
        assert calls and not any(form & A.SKIP for _, form in calls) and _lib.call_counts["qt_flags_or_i32"] == flags_or
