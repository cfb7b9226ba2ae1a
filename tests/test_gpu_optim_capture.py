"""The fused optimiser step inside GraphedTrainStep's hipGraph (csrc/optim_step.hip with QT_OPTIM_SCALARS_DEV, utils/optim.py capture
mode, utils/graphs.py).  Two oracles, both bit equality: the update with its scalars from device memory against the by-value form for equal scalars, and a
replayed update against the eager fused update of a twin that starts from the same parameters, state and gradients (the gradient
is taken out of the picture: captured and eager forwards may differ in torch's own kernels)."""
import copy

import numpy as np
import pytest
import torch

import _optim_exact as X
import bench_models
from pytorch_quantize_impls_amd import _lib, ops, utils
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import LinearBin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


# ---- 1. the kernels -------------------------------------------------------------------------------------------------------------

# 36 table entries, 34 of them non-empty = two chunks of the 32-slot by-value table.  The empty tensors sit at table index 5 and 33:
# the first chunk holds table entries 0 ... 32 without 5 (its slots 5 ... 31 are not their table indices) and the second starts at
# table index 34, which is no multiple of 32.  Flat sizes around the 4096-element unit and its 16-byte tail; plane tensors as
# (rows, K, kind) with K % 4 != 0 ([2, 6]), K % 8 != 0 ([5, 12], [4, 100]) and [9, 520] = 9 x 68 = 612 plane words, more than one
# 512-word plane unit.
SIZES = [1, 3, 5, (3, 8, "binary"), 4095, 0, 4096, 4097, 8199, (5, 12, "ternary"), 7, 4099, 2, 12288, (4, 100, "binary"), 9,
         6, 100, 33, 4, (2, 6, "ternary"), 1023, 1025, 64, (9, 520, "binary"), 17, 4093, 250, 31, 8, (9, 520, "ternary"), 515,
         4100, 0, 8199, (2, 6, "binary")]
VIEW = 11            # a flat tensor one element into its storage: 4-byte aligned only, the dword walk
N_TENSORS = 36


def _plane_ld(K):
    return ((K + 7) // 8 + 3) // 4 * 4


def _tensor_table(dev, seed):
    """params, grads, two zero-initialised-then-filled state lists, clamps, planes: one copy of the table."""
    assert len(SIZES) == N_TENSORS == 36 and ops.optim_chunk_capacity() == 32          # the layout the comment above relies on
    assert [i for i, n in enumerate(SIZES) if n == 0] == [5, 33] and not isinstance(SIZES[VIEW], tuple) and 9 * _plane_ld(520) == 612
    ps, gs, s0, s1, clamps, planes = [], [], [], [], [], []
    for i, size in enumerate(SIZES):
        shape = size[:2] if isinstance(size, tuple) else (size,)
        p0, g0 = X.inputs(seed + i, shape)
        m0, v0 = X.inputs(seed + 500 + i, shape)
        if i == VIEW:
            base = torch.zeros(size + 1, device=dev)
            base[1:].copy_(torch.from_numpy(p0))
            p = base[1:]
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.from_numpy(p0).to(dev)
        ps.append(p)
        gs.append(torch.from_numpy(g0).to(dev))
        s0.append(torch.from_numpy(m0 * 1e-2).to(dev))
        s1.append(torch.from_numpy(np.abs(v0) * 1e-2).to(dev))
        clamps.append((-1.0, 1.0) if i % 2 == 0 else None)
        if isinstance(size, tuple):
            rows, K, kind = size
            words = torch.full((rows, _plane_ld(K)), -1, dtype=torch.int32, device=dev)
            planes.append((ops.NibPlanes(words=words, rows=rows, K=K), kind))
        else:
            planes.append(None)
    return ps, gs, s0, s1, clamps, planes


def _same(a, b):
    for i, (ta, tb) in enumerate(zip(a, b)):
        assert torch.equal(ta, tb), i


def _same_planes(a, b):
    for i, (pa, pb) in enumerate(zip(a, b)):
        if pa is not None:
            assert torch.equal(pa[0].words, pb[0].words), i


@pytest.mark.parametrize("hp", [dict(lr=0.05), dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)], ids=["plain", "nesterov_wd"])
def test_sgd_dev_entry_stores_the_bits_of_the_by_value_entry(dev, hp):
    a, b = _tensor_table(dev, 100), _tensor_table(dev, 100)
    mom = hp.get("momentum", 0.0) != 0
    lr_dev = torch.tensor([hp["lr"]], dtype=torch.float32, device=dev)
    kw = {k: v for k, v in hp.items() if k != "lr"}
    ops.optim_step_sgd(a[0], a[1], a[2] if mom else None, lr=hp["lr"], clamps=a[4], planes=a[5], **kw)
    ops.optim_step_sgd_dev(b[0], b[1], b[2] if mom else None, lr_dev, clamps=b[4], planes=b[5], **kw)
    _same(a[0], b[0]), _same(a[2], b[2]), _same_planes(a[5], b[5])
    fresh = _tensor_table(dev, 100)                  # ... and the comparison is not one of two untouched copies
    assert all(not torch.equal(p, f) for p, f in zip(a[0], fresh[0]) if p.numel())
    assert all(torch.equal(m, f) != mom for m, f in zip(a[2], fresh[2]) if m.numel())
    assert all(not bool((pl[0].words == -1).any()) for pl in a[5] if pl is not None)


def test_adam_dev_entry_stores_the_bits_of_the_by_value_entry(dev):
    hp = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)
    a, b = _tensor_table(dev, 200), _tensor_table(dev, 200)
    steps = list(range(1, N_TENSORS + 1))            # a different step count per TABLE entry: a wrong coef index shows
    coef = torch.tensor(ops.adam_coefficients(steps, hp["lr"], hp["betas"]), dtype=torch.float32, device=dev).reshape(-1)
    before = [(p.cpu().numpy().copy(), g.cpu().numpy(), m.cpu().numpy().copy(), v.cpu().numpy().copy())
              for p, g, m, v in zip(a[0], a[1], a[2], a[3])]
    ops.optim_step_adam(a[0], a[1], a[2], a[3], steps, clamps=a[4], planes=a[5], **hp)
    kw = {k: v for k, v in hp.items() if k != "lr"}
    ops.optim_step_adam_dev(b[0], b[1], b[2], b[3], coef, clamps=b[4], planes=b[5], **kw)
    _same(a[0], b[0]), _same(a[2], b[2]), _same(a[3], b[3]), _same_planes(a[5], b[5])
    worst = 0.0
    for i, (p0, g0, m0, v0) in enumerate(before):
        p64, _, _, bound, _, _ = X.adam_step(p0, g0, m0, v0, steps[i], **hp)
        if b[4][i] is not None:
            p64 = np.clip(p64, *b[4][i])             # clipping is 1-Lipschitz: the bound carries over
        worst = max(worst, X.worst(b[0][i], p64, bound))
    print(f"qt_optim_adam_f32, scalars from the device: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_scalar_writer_rounds_like_a_by_value_float(dev):
    """1000 values = two launches of 960; every value arrives as the fp32 a by-value ``float`` argument would hold, elements past
    the values are left alone, and a later write on the same stream wins."""
    rng = np.random.default_rng(3)
    values = [float(v) for v in rng.standard_normal(1000) * 10.0 ** rng.uniform(-8, 3, 1000)] + [1e-3 / (1 - 0.9 ** 7), 0.1, 1 / 3]
    dst = torch.full((1100,), -7.0, device=dev)
    ops.optim_write_scalars(dst, [0.0] * len(values))
    ops.optim_write_scalars(dst, values)
    want = np.array(values, dtype=np.float64).astype(np.float32)
    assert np.array_equal(dst[:len(values)].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert bool((dst[len(values):] == -7.0).all())
    with pytest.raises(ValueError):
        ops.optim_write_scalars(dst[:4], [1.0] * 5)


def test_dev_wrappers_check_the_scalar_tensors(dev):
    p, g = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
    with pytest.raises(TypeError):
        ops.optim_step_sgd_dev([p], [g], None, torch.zeros(1))                       # host scalars
    with pytest.raises(ValueError):
        ops.optim_step_sgd_dev([p], [g], None, torch.zeros(2, device=dev))
    with pytest.raises(ValueError):
        ops.optim_step_adam_dev([p], [g], [g.clone()], [g.clone()], torch.zeros(1, device=dev))
    with pytest.raises(ValueError):
        ops.optim_step_adam_dev([p], [g], [g.clone()], [g.clone()], torch.zeros(2, device=dev, dtype=torch.float64))


# ---- 2 - 7. the binary MLP -----------------------------------------------------------------------------------------------------

def _mlp(dev):
    torch.manual_seed(21)
    net = torch.nn.Sequential(torch.nn.Linear(784, 256), torch.nn.BatchNorm1d(256), torch.nn.Hardtanh(), torch.nn.Linear(256, 10))
    return utils.binary_net_convert(net).to(dev).train()


def _loss(out, target):
    return torch.nn.functional.cross_entropy(out, target)


def _batches(dev, n, seed=22):
    """+-1 inputs: the first LinearBin then runs the packed matrix-core GEMM, whose weight operand is the emitted plane."""
    g = torch.Generator().manual_seed(seed)
    return [((torch.randint(0, 2, (64, 784), generator=g) * 2 - 1).float().to(dev), torch.randint(0, 10, (64,), generator=g).to(dev))
            for _ in range(n)]


OPTS = {"adam": lambda m, **kw: utils.FusedQuantAdam(m, lr=1e-2, weight_decay=1e-4, **kw),
        "sgd": lambda m, **kw: utils.FusedQuantSGD(m, lr=5e-2, momentum=0.9, **kw)}


def _state_keys(opt):
    return ("exp_avg", "exp_avg_sq") if isinstance(opt, utils.FusedQuantAdam) else ("momentum_buffer",)


class Twin:
    """A second model + optimiser that takes over parameters, buffers, optimiser state (hyper-parameters included) and planes of
    the captured pair before a call, and afterwards runs the EAGER fused step on the call's gradients."""

    def __init__(self, model, opt, make_model, make_opt):
        self.model, self.opt = model, opt
        self.twin = make_model()
        self.twin_opt = make_opt(self.twin)

    def before(self):
        self.twin.load_state_dict(self.model.state_dict())
        self.twin_opt.load_state_dict(copy.deepcopy(self.opt.state_dict()))
        for p, q in zip(self.model.parameters(), self.twin.parameters()):
            words = self.opt._plane_words.get(p)
            if words is not None:
                self.twin_opt._plane_of(q)[0].words.copy_(words)

    def after(self):
        """The eager step of the twin on the captured step's gradients; everything must be equal, bit for bit."""
        plan = utils.clamp_plan(self.model)
        for p, q in zip(self.model.parameters(), self.twin.parameters()):
            q.grad = p.grad.clone()
        self.twin_opt.step()
        planes = 0
        for (name, p), q in zip(self.model.named_parameters(), self.twin.parameters()):
            assert torch.equal(p, q), name
            sp, sq = self.opt.state.get(p) or {}, self.twin_opt.state.get(q) or {}
            assert set(sp) == set(sq), name
            for k in _state_keys(self.opt):
                assert torch.equal(sp[k], sq[k]), (name, k)
            if "step" in sq:
                assert float(sp["step"]) == float(sq["step"]) and not sp["step"].is_cuda, name
            if p in plan:
                assert float(p.detach().min()) >= plan[p][0] and float(p.detach().max()) <= plan[p][1], name
            words = self.opt._plane_words.get(p)
            if words is not None:
                assert torch.equal(words, self.twin_opt._plane_words[q]), name
                rec = p._qt_train_planes
                assert rec["version"] == p._version and rec["ptr"] == p.data_ptr() and rec["mfma"].words is words
                planes += 1
        return planes


def _captured(dev, kind, emit_planes=True, model=None, x0=None):
    model = _mlp(dev) if model is None else model
    opt = OPTS[kind](model, emit_planes=emit_planes)
    (x, t), = _batches(dev, 1, seed=5) if x0 is None else [x0]
    step = utils.GraphedTrainStep(model, _loss, x, t, optimizer=opt)
    return model, opt, step, Twin(model, opt, lambda: _mlp(dev), lambda m: OPTS[kind](m, emit_planes=emit_planes))


def _pack_calls():
    return sum(v for k, v in _lib.call_counts.items() if "pack" in k)


@pytest.mark.parametrize("emit_planes", [True, False], ids=["planes", "no_planes"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_captured_update_equals_the_eager_fused_update(dev, kind, emit_planes):
    with _fused.scope(GEMM_IMPL="mfma"):
        pair_before = _lib.call_counts["qt_pack_pair_nib_f32"]
        model, opt, step, twin = _captured(dev, kind, emit_planes)
        # the captured forward consumed the plane buffer (no weight operand was packed) exactly when planes are emitted
        assert (_lib.call_counts["qt_pack_pair_nib_f32"] == pair_before) == emit_planes
        losses = []
        for call, (x, t) in enumerate(_batches(dev, 5), 1):
            twin.before()
            versions = [p._version for p in model.parameters()]
            losses.append(float(step(x, t)))
            assert all(p._version != v for p, v in zip(model.parameters(), versions))
            assert twin.after() == (2 if emit_planes else 0)
            if kind == "adam":
                assert all(float(opt.state[p]["step"]) == call for p in model.parameters())
        assert all(np.isfinite(losses)) and len(set(losses)) == 5


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_construction_applies_no_update(dev, kind):
    with _fused.scope(GEMM_IMPL="mfma"):
        model = _mlp(dev)
        before = [p.detach().clone() for p in model.parameters()]
        model_, opt, step, _ = _captured(dev, kind, model=model)
        for p, b in zip(model.parameters(), before):
            assert torch.equal(p, b)
            st = opt.state[p]
            assert all(not st[k].any() for k in _state_keys(opt))
            assert float(st.get("step", 0.0)) == 0.0


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_learning_rate_schedule_reaches_the_replay(dev, kind):
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, twin = _captured(dev, kind)
        sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5)
        lrs = []
        for x, t in _batches(dev, 3):
            lrs.append(opt.param_groups[0]["lr"])
            twin.before()                              # takes the group's current lr with the state dict
            assert twin.twin_opt.param_groups[0]["lr"] == lrs[-1]
            step(x, t)
            twin.after()
            sched.step()
        assert lrs[1] == pytest.approx(lrs[0] * 0.5) and lrs[2] == pytest.approx(lrs[0] * 0.25)
        if kind == "adam":
            opt.param_groups[0]["betas"] = (0.5, 0.999)
        else:
            opt.param_groups[0]["momentum"] = 0.5
        (x, t), = _batches(dev, 1)
        steps = [float(opt.state[p].get("step", 0.0)) for p in model.parameters()]
        with pytest.raises(RuntimeError, match="baked"):
            step(x, t)
        assert steps == [float(opt.state[p].get("step", 0.0)) for p in model.parameters()]       # refused before anything moved


def test_stale_plane_is_repacked_once(dev):
    with _fused.scope(GEMM_IMPL="mfma"):
        batches = _batches(dev, 4)
        model, opt, step, _ = _captured(dev, "adam")
        assert isinstance(model[0], LinearBin)
        before = _pack_calls()
        for x, t in batches[:3]:
            step(x, t)
        assert _pack_calls() == before                     # no edit: nothing is packed on the host side of a replay
        with torch.no_grad():
            model[0].weight.mul_(-1)
        # the reference: a step captured WITHOUT planes, then given the same parameters, buffers and state (values copied into the
        # tensors its graph holds; its own warm-up moved nothing but BatchNorm's running statistics)
        ref_model = _mlp(dev)
        ref_model.load_state_dict(model.state_dict())
        ref_opt = OPTS["adam"](ref_model, emit_planes=False)
        ref_step = utils.GraphedTrainStep(ref_model, _loss, *batches[0], optimizer=ref_opt)
        ref_model.load_state_dict(model.state_dict())
        for p, q in zip(model.parameters(), ref_model.parameters()):
            assert torch.equal(p, q) and float(opt.state[p]["step"]) == 3
            for k in ("step", "exp_avg", "exp_avg_sq"):
                ref_opt.state[q][k].copy_(opt.state[p][k])
        x, t = batches[3]
        before = _pack_calls()
        loss = step(x, t).clone()
        assert _pack_calls() == before + 1                # exactly the first layer's plane
        assert torch.equal(model[0].weight._qt_train_planes["mfma"].words, ops.sign_pack_nib(model[0].weight.detach()).words)
        ref_loss = ref_step(x, t)
        print(f"loss after the edit: {float(loss):.9g} (planes), {float(ref_loss):.9g} (captured without planes)")
        assert torch.equal(loss, ref_loss)


def test_version_counters_move_and_eval_sees_the_update(dev):
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, twin = _captured(dev, "sgd")
        batches = _batches(dev, 4)
        seen = []
        for x, t in batches[:2]:
            step(x, t)
            seen.append(model[0].weight._version)
        assert seen[0] != seen[1]
        state = copy.deepcopy(model.state_dict())          # train-mode (fp32 master) weights
        fresh = _mlp(dev)
        fresh.load_state_dict(state)
        model.eval(), fresh.eval()
        with torch.no_grad():
            assert torch.equal(model(batches[2][0]), fresh(batches[2][0]))
        model.train()
        assert model[0].weight._qt_train_planes is None    # train() dropped the record: the next call packs the plane again
        before = _pack_calls()
        twin.before()
        step(*batches[3])
        assert _pack_calls() == before + 2
        assert twin.after() == 2


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_an_eager_step_between_replays(dev, kind):
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, twin = _captured(dev, kind)
        batches = _batches(dev, 2)
        step(*batches[0])
        opt.step()                                         # eager, on the gradients the replay left in p.grad
        if kind == "adam":
            assert all(float(opt.state[p]["step"]) == 2 for p in model.parameters())
        before = _pack_calls()
        twin.before()
        step(*batches[1])
        assert _pack_calls() == before                     # the eager step wrote the same plane buffers and recorded them
        assert twin.after() == 2
        if kind == "adam":
            assert all(float(opt.state[p]["step"]) == 3 for p in model.parameters())


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_replaced_state_and_dropped_gradients_are_refused(dev, kind):
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, twin = _captured(dev, kind)
        batches = _batches(dev, 2)
        step(*batches[0])
        opt.zero_grad()                                    # set_to_none=True: the graph's gradient buffers are no longer p.grad
        with pytest.raises(RuntimeError, match="gradient was replaced"):
            step(*batches[1])
        model, opt, step, twin = _captured(dev, kind)
        step(*batches[0])
        steps = [float(opt.state[p].get("step", 0.0)) for p in model.parameters()]
        opt.load_state_dict(copy.deepcopy(opt.state_dict()))          # new state tensors: the graph would update the old ones
        with pytest.raises(RuntimeError, match="load_state_dict"):
            step(*batches[1])
        assert steps == [float(opt.state[p].get("step", 0.0)) for p in model.parameters()]
        again = utils.GraphedTrainStep(model, _loss, *batches[0], optimizer=opt)      # load first, then capture: fine
        pair = Twin(model, opt, lambda: _mlp(dev), lambda m: OPTS[kind](m))
        pair.before()
        again(*batches[1])
        assert pair.after() == 2


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_one_optimiser_serves_two_captured_steps(dev, kind):
    """A full and a tail batch shape on one optimiser: each step keeps its own scalar block, so the first stays right after the
    second was captured (a shared, replaced block would leave its launches reading freed memory: NaN or a frozen learning rate),
    and both follow the learning-rate schedule and the shared step counts."""
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, full, twin = _captured(dev, kind)
        batches = _batches(dev, 4)
        tails = [(x[:16].clone(), t[:16].clone()) for x, t in _batches(dev, 3, seed=31)]
        tail = utils.GraphedTrainStep(model, _loss, *tails[0], optimizer=opt)
        assert full._capture is not tail._capture and full._capture.block.data_ptr() != tail._capture.block.data_ptr()
        sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5)
        calls = 0
        for step, (x, t) in [(full, batches[0]), (tail, tails[1]), (full, batches[1]), (full, batches[2]), (tail, tails[2])]:
            twin.before()
            assert bool(torch.isfinite(step(x, t)))
            assert twin.after() == 2
            sched.step()
            calls += 1
            if kind == "adam":
                assert all(float(opt.state[p]["step"]) == calls for p in model.parameters())


def test_another_capture_gets_no_plane_from_a_captured_optimiser(dev):
    """The plane buffer is handed to a capturing forward only by the capture that also holds its update.  A later GraphedTrainStep
    WITHOUT the optimiser, on the same model — after replays and an eager step() of that optimiser, whose records are current —
    packs the weight itself, so nothing has to keep a plane right for it."""
    with _fused.scope(GEMM_IMPL="mfma"):
        model, opt, step, _ = _captured(dev, "sgd")
        (x, t), = _batches(dev, 1)
        step(x, t)
        opt.step()
        rec = model[0].weight._qt_train_planes
        assert rec["version"] == model[0].weight._version              # a current record of the optimiser's buffer ...
        before = _lib.call_counts["qt_pack_pair_nib_f32"]
        plain = utils.GraphedTrainStep(model, _loss, x, t, warmup=1)
        # ... consumed by the eager warm-up forward, not by the captured one: exactly the capture packs both operands
        assert _lib.call_counts["qt_pack_pair_nib_f32"] == before + 1
        with torch.no_grad():
            model[0].weight.mul_(-1)
        fresh = _mlp(dev)
        fresh.load_state_dict(model.state_dict())
        assert torch.equal(plain(x, t), utils.GraphedTrainStep(fresh, _loss, x, t, warmup=1)(x, t))


def test_what_is_refused_on_the_device(dev):
    model = _mlp(dev)
    (x, t), = _batches(dev, 1)
    with pytest.raises(TypeError, match=r"opt\.step\(\)"):
        utils.GraphedTrainStep(model, _loss, x, t, optimizer=torch.optim.Adam(model.parameters()))
    model[3].weight.data = model[3].weight.data.double()
    with pytest.raises(ValueError, match=r"3\.weight"):
        utils.GraphedTrainStep(model, _loss, x, t, optimizer=utils.FusedQuantSGD(model, lr=0.1))


# ---- 8. a conv net: more than 32 parameters, the conv layers' clamp plan -------------------------------------------------------

def test_dorefa_resnet18_two_calls(dev):
    def make():
        torch.manual_seed(12)
        m = bench_models.DorefaResNet18(w_bits=1, a_bits=4)
        bench_models.randomize_bn(m, 5)
        return m.to(dev).train()

    def make_opt(m):
        return utils.FusedQuantSGD(m, lr=1e-2, momentum=0.9)

    def loss_fn(out, target):
        return torch.nn.functional.cross_entropy(out, target)

    model = make()
    opt = make_opt(model)
    assert len(list(model.parameters())) > ops.optim_chunk_capacity()
    g = torch.Generator().manual_seed(3)
    data = [(torch.randn(32, 3, 32, 32, generator=g).to(dev), torch.randint(0, 10, (32,), generator=g).to(dev)) for _ in range(3)]
    before = [p.detach().clone() for p in model.parameters()]
    step = utils.GraphedTrainStep(model, loss_fn, *data[0], optimizer=opt)
    assert all(torch.equal(p, b) for p, b in zip(model.parameters(), before))
    twin = Twin(model, opt, make, make_opt)
    for x, t in data[1:]:
        twin.before()
        assert bool(torch.isfinite(step(x, t)))
        twin.after()
    assert any(not torch.equal(p, b) for p, b in zip(model.parameters(), before))
