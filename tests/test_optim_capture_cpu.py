"""The capture mode of FusedQuantSGD / FusedQuantAdam and GraphedTrainStep(optimizer=...) without a GPU: what is refused and how,
and the zeroed state ``prepare_capture`` allocates against torch's own optimisers."""
import copy

import pytest
import torch

from pytorch_quantize_impls_amd import layers as L
from pytorch_quantize_impls_amd import utils


def _mlp():
    torch.manual_seed(5)
    return torch.nn.Sequential(L.LinearBin(12, 9), torch.nn.BatchNorm1d(9), L.LinearTer(9, 7), torch.nn.Linear(7, 4))


def _grads(model, seed):
    g = torch.Generator().manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=g)
        p.grad.view(-1)[0] = -0.0                      # the one entry a zeroed momentum buffer treats differently


def _mlp_with_grads():
    model = _mlp()
    _grads(model, 3)
    return model


def _loss(out, target):
    return torch.nn.functional.cross_entropy(out, target)


@pytest.mark.parametrize("make", [lambda m: utils.FusedQuantSGD(m, lr=0.1, momentum=0.9), lambda m: utils.FusedQuantAdam(m)],
                         ids=["sgd", "adam"])
def test_host_tensors_are_refused_with_a_type_error(make):
    model = _mlp()
    with pytest.raises(TypeError, match="device tensors"):
        utils.GraphedTrainStep(model, _loss, torch.randn(4, 12), torch.zeros(4, dtype=torch.long), optimizer=make(model))


def test_other_optimisers_are_pointed_to_the_old_form():
    model = _mlp()
    with pytest.raises(TypeError, match=r"opt\.step\(\)"):
        utils.GraphedTrainStep(model, _loss, torch.randn(4, 12), torch.zeros(4, dtype=torch.long),
                               optimizer=torch.optim.SGD(model.parameters(), lr=0.1))


def test_a_synchronised_model_is_refused():
    import gc
    import pickle
    model = _mlp()
    x, t = torch.randn(4, 12), torch.zeros(4, dtype=torch.long)

    def attempt():
        utils.GraphedTrainStep(model, _loss, x, t, optimizer=utils.FusedQuantSGD(model, lr=0.1))

    sync, second = utils.GradientSynchronizer(model.parameters()), utils.GradientSynchronizer(model.parameters())
    for copied in (pickle.loads(pickle.dumps(model)), copy.deepcopy(model)):      # a copy has no synchroniser behind it
        with pytest.raises(TypeError, match="device tensors"):
            utils.GraphedTrainStep(copied, _loss, x, t, optimizer=utils.FusedQuantSGD(copied, lr=0.1))
    second.remove()
    with pytest.raises(RuntimeError, match="GradientSynchronizer"):  # one of the two is still attached
        attempt()
    sync.remove()
    sync.remove()                                                    # (idempotent)
    with pytest.raises(TypeError, match="device tensors"):          # ... and is let through to the next check once it is removed
        attempt()
    dropped = utils.GradientSynchronizer(model.parameters())         # dropped without remove(): the mark goes with it
    with pytest.raises(RuntimeError, match="GradientSynchronizer"):
        attempt()
    del dropped
    gc.collect()
    with pytest.raises(TypeError, match="device tensors"):
        attempt()


def test_prepare_capture_names_the_parameter_off_the_route():
    model = _mlp()
    _grads(model, 1)
    opt = utils.FusedQuantAdam(model)
    with pytest.raises(ValueError, match=r"0\.weight"):            # host tensors: the first parameter is already off the route
        opt.prepare_capture()

    only = [p for n, p in model.named_parameters() if n == "2.weight"]
    opt = utils.FusedQuantSGD(only, lr=0.1)                          # no module: named by its place in the groups
    with pytest.raises(ValueError, match=r"param_groups\[0\]\['params'\]\[0\]"):
        opt.prepare_capture()

    d = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))      # non-fp32
    d.grad = torch.ones(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="float64"):
        utils.FusedQuantAdam([d]).prepare_capture()

    t = torch.nn.Parameter(torch.randn(6, 5).t())                    # non-contiguous
    t.grad = torch.randn(5, 6)
    with pytest.raises(ValueError, match="contiguous=False"):
        utils.FusedQuantSGD([t], lr=0.1).prepare_capture()


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_the_zeroed_state_is_the_state_before_the_first_step(kind):
    """allocate_state — the first thing prepare_capture does — creates every state tensor as zeros.  That state loads into
    torch.optim, and one torch step from it equals one torch step from no state."""
    hp = dict(lr=0.05, momentum=0.9, weight_decay=1e-3) if kind == "sgd" else dict(lr=3e-3, betas=(0.8, 0.95), weight_decay=1e-2)
    Fused = utils.FusedQuantSGD if kind == "sgd" else utils.FusedQuantAdam
    Ref = torch.optim.SGD if kind == "sgd" else torch.optim.Adam
    a, b, c = _mlp(), _mlp(), _mlp()
    _grads(a, 3), _grads(b, 3), _grads(c, 3)
    list(a.parameters())[3].grad = None                              # no gradient: no state, not part of a captured step
    fused = Fused(a, **hp)
    fused.allocate_state()                                           # what prepare_capture() does first
    for i, p in enumerate(a.parameters()):
        st = fused.state.get(p) or {}
        if i == 3:
            assert not st
            continue
        if kind == "sgd":
            assert set(st) == {"momentum_buffer"} and not st["momentum_buffer"].any()
        else:
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 0 and not st["step"].is_cuda
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    list(a.parameters())[3].grad = list(b.parameters())[3].grad.clone()
    fused.allocate_state()                                           # ... and now that one too; existing state is kept
    from_zeros, from_none = Ref(b.parameters(), lr=123.0), Ref(c.parameters(), **hp)
    from_zeros.load_state_dict(copy.deepcopy(fused.state_dict()))
    assert from_zeros.param_groups[0]["lr"] == hp["lr"]
    from_zeros.step(), from_none.step()
    for p, q in zip(b.parameters(), c.parameters()):
        assert torch.equal(p, q)
        sp, sq = from_zeros.state[p], from_none.state[q]
        assert set(sp) == set(sq)
        for k in sp:
            assert torch.equal(torch.as_tensor(sp[k]), torch.as_tensor(sq[k])), k
    back = Fused(a, lr=456.0)                                        # ... and back into the fused optimiser
    back.load_state_dict(copy.deepcopy(from_zeros.state_dict()))
    assert back.param_groups[0]["lr"] == hp["lr"]
    with pytest.raises(ValueError):                                  # host tensors: allocated, then refused by the route check
        Fused(_mlp_with_grads(), **hp).prepare_capture()


def test_captures_are_handles_and_load_state_dict_invalidates_them():
    """Host tensors cannot be captured, so the handle's bookkeeping is checked on what needs no launch: a capture of an optimiser
    with nothing to update (no gradients) has no groups and no block; load_state_dict makes its next before_replay raise."""
    model = _mlp()
    opt = utils.FusedQuantAdam(model)
    first, second = opt.prepare_capture(), opt.prepare_capture()
    assert first is not second and first.groups == [] and first.block is None
    opt.before_replay(first), opt.after_replay(first), opt.before_replay(second)
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    with pytest.raises(RuntimeError, match="load_state_dict"):
        opt.before_replay(first)
    opt.before_replay(opt.prepare_capture())                         # a capture made after the load is fine


def test_constructors_still_reject_what_they_rejected():
    ps = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError):
        utils.FusedQuantAdam(ps, capturable=True)
    opt = utils.FusedQuantSGD(ps, lr=0.1, momentum=0.9)
    ps[0].grad = torch.ones(3)
    opt.param_groups[0]["dampening"] = 0.5                           # switched on through the group dict
    with pytest.raises(NotImplementedError):
        opt.prepare_capture()
