"""FusedQuantSGD / FusedQuantAdam without a GPU: the error bound of tests/_optim_exact.py pinned against torch's own optimisers,
clamp_plan against clamp_weights_, the library route of the fused optimisers (host tensors), state-dict round trips, rejected
options, and the unchanged six-argument form of QuantLinearFn."""
import copy

import pytest
import torch

import _optim_exact as X
from pytorch_quantize_impls_amd import layers as L
from pytorch_quantize_impls_amd import utils
from pytorch_quantize_impls_amd.functions import _fused

SGD_VARIANTS = [dict(lr=0.05), dict(lr=0.05, momentum=0.9, weight_decay=1e-3),
                dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)]
ADAM_VARIANTS = [dict(lr=1e-3), dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)]


@pytest.mark.parametrize("hp", SGD_VARIANTS, ids=["plain", "momentum_wd", "nesterov"])
def test_torch_sgd_is_inside_the_bound(hp):
    p0, _ = X.inputs(1, (4099,))
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([p], foreach=False, **hp)
    worst = 0.0
    for step in range(1, 6):
        _, g = X.inputs(10 + step, (4099,), step=step)
        p.grad = torch.from_numpy(g)
        before = p.detach().clone()
        buf = opt.state[p].get("momentum_buffer")
        buf = None if buf is None else buf.clone()
        opt.step()
        p64, b64, bp, bb = X.sgd_step(before, g, buf, **hp)
        worst = max(worst, X.worst(p, p64, bp))
        if b64 is not None:
            worst = max(worst, X.worst(opt.state[p]["momentum_buffer"], b64, bb))
    print(f"torch.optim.SGD {hp}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("hp", ADAM_VARIANTS, ids=["default", "custom"])
def test_torch_adam_is_inside_the_bound(hp):
    p0, _ = X.inputs(2, (4099,))
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], foreach=False, **hp)
    worst = 0.0
    for step in range(1, 6):
        _, g = X.inputs(20 + step, (4099,), step=step)
        p.grad = torch.from_numpy(g)
        before = p.detach().clone()
        st = opt.state[p]
        m = st["exp_avg"].clone() if st else torch.zeros_like(before)
        v = st["exp_avg_sq"].clone() if st else torch.zeros_like(before)
        opt.step()
        p64, m64, v64, bp, bm, bv = X.adam_step(before, g, m, v, step, **hp)
        st = opt.state[p]
        worst = max(worst, X.worst(p, p64, bp), X.worst(st["exp_avg"], m64, bm), X.worst(st["exp_avg_sq"], v64, bv))
    print(f"torch.optim.Adam {hp}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


class _OddClamp(torch.nn.Linear):
    """A layer clamp_plan does not know: its clamp() must still run (after the launch)."""

    def clamp(self):
        self.weight.data.clamp_(-3, 2)


def every_family():
    return torch.nn.Sequential(
        L.LinearBin(6, 5), L.LinearTer(6, 5, bias=False), L.BinConv2d(2, 3, 3), L.TerConv2d(2, 3, 3),
        L.LinearDorefa(6, 5), L.DorefaConv2d(2, 3, 3), L.LinearXNOR(6, 5), L.XNORConv2d(2, 3, 3),
        L.LinearQuant(6, 5, fsr=3), L.QuantConv2d(2, 3, 3, fsr=2, dtype="log"),
        L.LinearQuantLin(6, 5, bottom=-2, top=3), L.LinearQuantLog(6, 5), L.QuantConv2dLin(2, 3, 3), L.QuantConv2dLog(2, 3, 3, gamma=3),
        L.LinearQuantWLin(6, 5), L.LinearQuantWLog(6, 5, bias=False), L.QuantConv2dWLin(2, 3, 3, bottom=-0.5, top=0.25),
        L.QuantConv2dWLog(2, 3, 3), torch.nn.BatchNorm2d(3), torch.nn.Linear(6, 5), _OddClamp(6, 5))


def _set_huge(model):
    with torch.no_grad():
        for p in model.parameters():
            sign = torch.where(torch.arange(p.numel()) % 2 == 0, 1.0, -1.0).reshape(p.shape)
            p.copy_(sign * 1e6)


def test_clamp_plan_is_what_clamp_weights_does():
    model = every_family()
    plan = utils.clamp_plan(model)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items()), "clamp_plan is pure"
    _set_huge(model)
    want = copy.deepcopy(model)
    utils.clamp_weights_(want)
    from pytorch_quantize_impls_amd.utils.optim import unplanned_clamp_layers
    odd = unplanned_clamp_layers(model)
    assert [type(m) for m in odd] == [_OddClamp]
    clamped = 0
    for (name, p), (_, w) in zip(model.named_parameters(), want.named_parameters()):
        got = p.detach().clone()
        if p in plan:
            got = got.clamp(*plan[p])
            clamped += 1
        elif any(p is m.weight for m in odd):
            got = got.clamp(-3, 2)
        assert torch.equal(got, w.detach()), name
    assert clamped == 2 + 1 + 1 + 1 + 1 + 1 + 2 + 2 + 2 + 2 + 2 + 1 + 2 + 2
    # a few literal values, so the test does not only compare the plan with itself
    m = dict(model.named_children())
    assert plan[m["0"].weight] == (-1.0, 1.0) and plan[m["0"].bias] == (-1.0, 1.0)
    assert plan[m["2"].weight] == (-1.0, 1.0) and m["2"].bias not in plan
    assert plan[m["8"].weight] == (-8.0, 8.0) and m["8"].bias not in plan
    assert plan[m["10"].bias] == (-2.0, 3.0)
    assert m["6"].weight not in plan and m["7"].weight not in plan and m["4"].weight not in plan


def _mlp():
    torch.manual_seed(5)
    model = torch.nn.Sequential(L.LinearBin(12, 9), torch.nn.BatchNorm1d(9), L.LinearTer(9, 7), torch.nn.Linear(7, 4), _OddClamp(4, 3))
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(4.0)            # some entries start outside every clamp range: the clamps act from the first step on
    return model


def _grads(model, step):
    g = torch.Generator().manual_seed(100 + step)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g) * 3.0


@pytest.mark.parametrize("kind,hp", [("sgd", h) for h in SGD_VARIANTS] + [("adam", h) for h in ADAM_VARIANTS])
def test_cpu_route_equals_torch_optim_plus_clamp(kind, hp):
    a, b = _mlp(), _mlp()
    if kind == "sgd":
        fused, ref = utils.FusedQuantSGD(a, **hp), torch.optim.SGD(b.parameters(), **hp)
    else:
        fused, ref = utils.FusedQuantAdam(a, **hp), torch.optim.Adam(b.parameters(), **hp)
    frozen = list(a.parameters())[2]
    for step in range(3):
        _grads(a, step)
        _grads(b, step)
        frozen.grad = None
        list(b.parameters())[2].grad = None
        fused.step()
        ref.step()
        utils.clamp_weights_(b)
        for (name, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (step, name)
    with torch.no_grad():
        assert float(a[0].weight.abs().max()) == 1.0 and float(a[2].weight.abs().max()) == 1.0      # planned clamps
        assert float(a[3].weight.abs().max()) > 1.0 and float(a[4].weight.max()) <= 2.0             # nn.Linear; the unplanned clamp()
    for p, q in zip(a.parameters(), b.parameters()):
        sa, sb = fused.state.get(p, {}), ref.state.get(q, {})
        assert set(sa) == set(sb)
        for k in sa:
            assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), k


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_state_dict_round_trips_through_torch_optim(kind):
    hp = SGD_VARIANTS[1] if kind == "sgd" else ADAM_VARIANTS[1]
    Fused = utils.FusedQuantSGD if kind == "sgd" else utils.FusedQuantAdam
    Ref = torch.optim.SGD if kind == "sgd" else torch.optim.Adam
    a, b, c = _mlp(), _mlp(), _mlp()
    fused = Fused(a, **hp)
    for step in range(2):
        _grads(a, step)
        fused.step()
    b.load_state_dict(a.state_dict())
    c.load_state_dict(a.state_dict())
    ref = Ref(b.parameters(), lr=123.0)
    ref.load_state_dict(copy.deepcopy(fused.state_dict()))            # fused -> torch (load_state_dict keeps the tensors it is given)
    assert ref.param_groups[0]["lr"] == hp["lr"]
    back = Fused(c, lr=456.0)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))              # ... and back
    sched = torch.optim.lr_scheduler.StepLR(fused, step_size=1, gamma=0.5)
    _grads(a, 7), _grads(b, 7), _grads(c, 7)
    fused.step(), ref.step(), back.step()
    utils.clamp_weights_(b)
    for p, q, r in zip(a.parameters(), b.parameters(), c.parameters()):
        assert torch.equal(p, q) and torch.equal(p, r)
    sched.step()
    assert fused.param_groups[0]["lr"] == pytest.approx(hp["lr"] * 0.5)


def test_unsupported_options_raise():
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(maximize=True), dict(dampening=0.1, momentum=0.9), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            utils.FusedQuantSGD(ps, lr=0.1, **kw)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(decoupled_weight_decay=True)):
        with pytest.raises(NotImplementedError):
            utils.FusedQuantAdam(ps, **kw)
    with pytest.raises(ValueError):
        utils.FusedQuantSGD(ps, lr=0.1, nesterov=True)
    opt = utils.FusedQuantAdam(ps)
    opt.param_groups[0]["amsgrad"] = True                # e.g. through a loaded state dict
    ps[0].grad = torch.ones(3)
    with pytest.raises(NotImplementedError):
        opt.step()


def test_plain_parameters_have_no_plan_and_skip_missing_grads():
    layer = L.LinearBin(4, 3)
    with torch.no_grad():
        layer.weight.fill_(0.9)
    opt = utils.FusedQuantSGD(layer.parameters(), lr=1.0)
    layer.weight.grad = -torch.ones_like(layer.weight)
    bias = layer.bias.detach().clone()
    opt.step()
    assert torch.equal(layer.weight.detach(), torch.full((3, 4), 1.9))      # not clamped: no module, no plan
    assert torch.equal(layer.bias.detach(), bias) and not opt.state.get(layer.bias)


def test_quant_linear_fn_keeps_its_six_argument_form():
    torch.manual_seed(0)
    x = torch.randn(5, 8, requires_grad=True)
    w = torch.nn.Parameter(torch.randn(3, 8))
    b = torch.nn.Parameter(torch.randn(3))
    y = _fused.QuantLinearFn.apply(x, w, b, "binary", None, None)
    y.sum().backward()
    wq = torch.where(w < 0, -1.0, 1.0)
    assert torch.equal(y.detach(), torch.nn.functional.linear(x.detach(), wq, b.detach()))
    assert x.grad is not None and w.grad is not None and b.grad is not None
    y7 = _fused.QuantLinearFn.apply(x, w, b, "binary", None, None, None)
    assert torch.equal(y7, y)
