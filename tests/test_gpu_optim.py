"""The fused training update (csrc/optim_step.hip, utils/optim.py) on the GPU: every element of every tensor against the float64
recurrence and the bound of tests/_optim_exact.py, the clamp folded into the launch, the nibble planes it leaves behind
(bit-identical to the weight-only packs), and the training forward of LinearBin / LinearTer consuming them."""
import numpy as np
import pytest
import torch

import _optim_exact as X
from pytorch_quantize_impls_amd import _lib, ops, utils
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.layers import BinConv2d, LinearBin, LinearTer

pytestmark = pytest.mark.gpu

SGD_VARIANTS = {"plain": dict(lr=0.05), "momentum_wd": dict(lr=0.05, momentum=0.9, weight_decay=1e-3),
                "nesterov": dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)}
ADAM_VARIANTS = {"default": dict(lr=1e-3), "custom": dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _sizes():
    """70 tensors (capacity + 6 if the chunk capacity is larger): more than one chunk of the by-value table.  numel 1, 3, 7, 4096
    and 70 001 as asked; 4097 / 8195 / 12288 put the 16-byte path's tail and unit boundaries in play."""
    n = max(70, ops.optim_chunk_capacity() + 6)
    fixed = [1, 3, 7, 4096, 70001, 4097, 8195, 12288, 2, 4, 5, 4095]
    rng = np.random.default_rng(7)
    return fixed + [int(v) for v in rng.integers(1, 700, n - len(fixed))]


VIEW, NO_GRAD, FROZEN = 13, 14, 15          # indices into the tensor set


def _tensor_set(dev):
    sizes = _sizes()
    params = []
    for i, n in enumerate(sizes):
        p0, _ = X.inputs(1000 + i, (n,))
        if i == VIEW:                       # a view starting one element into its storage: 4-byte aligned only
            base = torch.zeros(n + 1, device=dev)
            base[1:].copy_(torch.from_numpy(p0))
            p = torch.nn.Parameter(base[1:])
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(torch.from_numpy(p0).to(dev))
        params.append(p)
    params[FROZEN].requires_grad_(False)
    return params


def _set_grads(params, step):
    grads = []
    for i, p in enumerate(params):
        _, g = X.inputs(5000 + 97 * step + i, tuple(p.shape), step=step)
        grads.append(g)
        p.grad = None if i in (NO_GRAD, FROZEN) else torch.from_numpy(g).to(p.device)
    return grads


def _cpu(t):
    return None if t is None else t.detach().cpu().numpy().copy()


@pytest.mark.parametrize("name", list(SGD_VARIANTS))
def test_sgd_every_element_within_the_bound(dev, name):
    hp = SGD_VARIANTS[name]
    params = _tensor_set(dev)
    opt = utils.FusedQuantSGD(params, **hp)
    before_calls = _lib.call_counts["qt_optim_sgd_f32"]
    worst = 0.0
    for step in range(1, 4):
        grads = _set_grads(params, step)
        p_before = [_cpu(p) for p in params]
        b_before = [_cpu(opt.state[p].get("momentum_buffer")) if p in opt.state else None for p in params]
        versions = [p._version for p in params]
        opt.step()
        for i, p in enumerate(params):
            if i in (NO_GRAD, FROZEN):
                assert np.array_equal(_cpu(p).view(np.uint32), p_before[i].view(np.uint32)) and p._version == versions[i]
                assert not opt.state.get(p)
                continue
            assert p._version > versions[i], i
            p64, b64, bp, bb = X.sgd_step(p_before[i], grads[i], b_before[i], **hp)
            worst = max(worst, X.worst(p, p64, bp))
            if b64 is not None:
                worst = max(worst, X.worst(opt.state[p]["momentum_buffer"], b64, bb))
    print(f"FusedQuantSGD {name}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    assert _lib.call_counts["qt_optim_sgd_f32"] == before_calls + 3          # one entry call per step and group


@pytest.mark.parametrize("name", list(ADAM_VARIANTS))
def test_adam_every_element_within_the_bound(dev, name):
    hp = ADAM_VARIANTS[name]
    params = _tensor_set(dev)
    opt = utils.FusedQuantAdam(params, **hp)
    before_calls = _lib.call_counts["qt_optim_adam_f32"]
    worst = 0.0
    for step in range(1, 4):
        grads = _set_grads(params, step)
        p_before = [_cpu(p) for p in params]
        zeros = [np.zeros_like(a) for a in p_before]
        m_before = [_cpu(opt.state[p]["exp_avg"]) if opt.state.get(p) else zeros[i] for i, p in enumerate(params)]
        v_before = [_cpu(opt.state[p]["exp_avg_sq"]) if opt.state.get(p) else zeros[i] for i, p in enumerate(params)]
        versions = [p._version for p in params]
        opt.step()
        for i, p in enumerate(params):
            if i in (NO_GRAD, FROZEN):
                assert np.array_equal(_cpu(p).view(np.uint32), p_before[i].view(np.uint32)) and p._version == versions[i]
                assert not opt.state.get(p)
                continue
            assert p._version > versions[i], i
            st = opt.state[p]
            assert float(st["step"]) == step and not st["step"].is_cuda
            p64, m64, v64, bp, bm, bv = X.adam_step(p_before[i], grads[i], m_before[i], v_before[i], step, **hp)
            worst = max(worst, X.worst(p, p64, bp), X.worst(st["exp_avg"], m64, bm), X.worst(st["exp_avg_sq"], v64, bv))
    print(f"FusedQuantAdam {name}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    assert _lib.call_counts["qt_optim_adam_f32"] == before_calls + 3


def test_clamp_is_folded_into_the_launch(dev):
    torch.manual_seed(3)
    model = torch.nn.Sequential(LinearBin(100, 12), BinConv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Linear(5, 3)).to(dev)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.rand(p.shape, generator=g) * 2 - 1)
            p.grad = ((torch.rand(p.shape, generator=g) * 4 - 2)).to(dev)        # lr 1: about half the entries leave [-1, 1]
    before = {n: _cpu(p) for n, p in model.named_parameters()}
    grads = {n: _cpu(p.grad) for n, p in model.named_parameters()}
    utils.FusedQuantSGD(model, lr=1.0).step()
    clamped = {"0.weight", "0.bias", "1.weight"}
    for n, p in model.named_parameters():
        p64, _, bound, _ = X.sgd_step(before[n], grads[n], None, lr=1.0)
        got = _cpu(p).astype(np.float64)
        outside = np.abs(p64) > 1.0
        assert outside.mean() > 0.25, n                    # the update does push entries past +-1
        if n in clamped:
            assert got.min() >= -1.0 and got.max() <= 1.0, n
            inside = np.abs(p64) < 1.0 - bound
            assert inside.any() and np.all(np.abs(got - p64)[inside] <= bound[inside]), n
            far = np.abs(p64) > 1.0 + bound
            assert np.array_equal(got[far], np.sign(p64[far])), n
        else:                                              # BinConv2d.bias, BatchNorm, nn.Linear: never clamped
            assert np.all(np.abs(got - p64) <= bound), n
            assert np.abs(got).max() > 1.0, n


SHAPES = [(3, 8), (12, 100), (5, 264), (64, 256)]


def _weight_pack(layer):
    pack = ops.sign_pack_nib if isinstance(layer, LinearBin) else ops.ternary_pack_nib
    return pack(layer.weight.detach()).words


@pytest.mark.parametrize("cls", [LinearBin, LinearTer])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_planes_equal_the_weight_only_pack(dev, cls, N, K, kind):
    torch.manual_seed(N * 1000 + K)
    layer = cls(K, N).to(dev)
    with torch.no_grad():
        layer.weight.uniform_(-1.2, 1.2)
    opt = utils.FusedQuantSGD(layer, lr=0.3, momentum=0.9) if kind == "sgd" else utils.FusedQuantAdam(layer, lr=0.2)
    for step in range(2):
        layer.weight.grad = torch.randn(N, K, device=dev)
        layer.bias.grad = torch.randn(N, device=dev)
        rec = getattr(layer.weight, "_qt_train_planes", None)
        if rec is not None:
            ptr = rec["mfma"].words.data_ptr()
            rec["mfma"].words.fill_(-1)                    # the buffer is persistent: every word, pad included, must be rewritten
        opt.step()
        rec = layer.weight._qt_train_planes
        assert rec["version"] == layer.weight._version and rec["ptr"] == layer.weight.data_ptr()
        words = rec["mfma"].words
        assert tuple(words.shape) == (N, ops.packed_ld_nib(K)) and rec["mfma"].rows == N and rec["mfma"].K == K
        if step:
            assert words.data_ptr() == ptr                 # same buffer across steps
        assert torch.equal(words, _weight_pack(layer)), (cls.__name__, N, K, step)
    assert float(layer.weight.detach().abs().max()) <= 1.0


@pytest.mark.parametrize("cls", [LinearBin, LinearTer])
def test_quantiser_edge_values_reach_the_plane(dev, cls):
    h = np.float32(0.5)
    edge = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, np.nextafter(h, np.float32(0)), np.nextafter(h, np.float32(1)),
                     np.nextafter(-h, np.float32(0)), np.nextafter(-h, np.float32(-1))], dtype=np.float32)
    for N, K in ((4, 25), (4, 40)):                        # K % 4 != 0: the scalar walk; K % 4 == 0: the 16-byte walk
        layer = cls(K, N).to(dev)
        w = np.resize(edge, (N, K))
        with torch.no_grad():
            layer.weight.copy_(torch.from_numpy(w))
        layer.weight.grad = torch.rand(N, K, device=dev) + 0.5          # positive: 0 * g = +0 keeps the sign of -0.0
        layer.bias.grad = torch.zeros(N, device=dev)
        utils.FusedQuantSGD(layer, lr=0.0).step()
        assert np.array_equal(_cpu(layer.weight).view(np.uint32), w.view(np.uint32))
        assert torch.equal(layer.weight._qt_train_planes["mfma"].words, _weight_pack(layer))


def _pair(dev, in_f, out_f, deterministic=True):
    torch.manual_seed(11)
    a, b = LinearBin(in_f, out_f, deterministic=deterministic).to(dev), LinearBin(in_f, out_f, deterministic=deterministic).to(dev)
    b.load_state_dict(a.state_dict())
    return a, b


def _pm1(dev, rows, K, seed=12):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1).float().to(dev)


def _moved(fn, entry="qt_pack_pair_nib_f32"):
    before = _lib.call_counts[entry]
    out = fn()
    return out, _lib.call_counts[entry] - before


# LinearBin(1024, 512) at batch 64 as asked: the automatic selector sends that shape to the popcount kernels (its matrix-core
# window starts at K = 2048), so the case runs with the matrix-core formulation selected (the scoped switch the package has for
# it); LinearBin(2048, 512) at batch 64 is a shape the automatic selector itself routes to "mfma".
CONSUME = [(1024, 512, "mfma"), (2048, 512, "auto")]


@pytest.mark.parametrize("in_f,out_f,impl", CONSUME)
def test_train_forward_consumes_the_plane(dev, in_f, out_f, impl):
    with _fused.scope(GEMM_IMPL=impl):
        assert ops.select_gemm_impl(_fused._cfg("GEMM_IMPL"), 64, out_f, in_f) == "mfma"
        layer, twin = _pair(dev, in_f, out_f)
        x = _pm1(dev, 64, in_f)
        opt = utils.FusedQuantSGD(layer, lr=0.05)
        layer(x).square().mean().backward()
        opt.step()
        with torch.no_grad():
            twin.weight.copy_(layer.weight)
            twin.bias.copy_(layer.bias)
        assert getattr(twin.weight, "_qt_train_planes", None) is None
        layer.zero_grad()
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya, moved_a = _moved(lambda: layer(xa))
        yb, moved_b = _moved(lambda: twin(xb))
        assert moved_a == 0 and moved_b == 1               # the weight was not packed again; the twin's was
        assert torch.equal(ya, yb)
        go = torch.randn(64, out_f, generator=torch.Generator().manual_seed(13)).to(dev)
        ya.backward(go)
        yb.backward(go)
        assert torch.equal(layer.weight.grad, twin.weight.grad) and torch.equal(layer.bias.grad, twin.bias.grad)
        assert torch.equal(xa.grad, xb.grad)


def test_stale_plane_records_are_ignored(dev):
    in_f, out_f = 2048, 512
    x = _pm1(dev, 64, in_f)

    def stepped(deterministic=True):
        layer, _ = _pair(dev, in_f, out_f, deterministic)
        opt = utils.FusedQuantSGD(layer, lr=0.05)
        layer.weight.grad = torch.randn(out_f, in_f, device=dev)
        layer.bias.grad = torch.randn(out_f, device=dev)
        opt.step()
        return layer

    layer = stepped()
    assert _moved(lambda: layer(x))[1] == 0                # the record is live ...
    with torch.no_grad():
        layer.weight.mul_(1)                               # ... until the version counter moves
    assert _moved(lambda: layer(x))[1] == 1

    layer = stepped()
    layer.eval()
    layer.train()
    assert layer.weight._qt_train_planes is None and _moved(lambda: layer(x))[1] == 1

    layer = stepped()
    layer.reset_quant_cache()
    assert layer.weight._qt_train_planes is None and _moved(lambda: layer(x))[1] == 1

    layer = stepped()
    layer.load_state_dict(layer.state_dict())
    assert layer.weight._qt_train_planes is None

    layer = stepped(deterministic=False)                   # a stochastic layer gets no plane and packs its draw
    assert getattr(layer.weight, "_qt_train_planes", None) is None
    torch.manual_seed(1)
    assert _moved(lambda: layer(x))[1] == 1


def test_binary_mlp_ten_adam_steps_track_torch(dev):
    """binary_net_convert of a 784 -> 256 -> 10 MLP at batch 64: FusedQuantAdam against torch.optim.Adam + clamp_weights_, ten steps.
    After each step the fused side is re-based on the torch side, so every step is checked inside the per-step bound and a
    flipped sign cannot pull the trajectories apart."""
    hp = dict(lr=1e-2, weight_decay=1e-4)

    def make():
        torch.manual_seed(21)
        net = torch.nn.Sequential(torch.nn.Linear(784, 256), torch.nn.BatchNorm1d(256), torch.nn.Hardtanh(), torch.nn.Linear(256, 10))
        return utils.binary_net_convert(net).to(dev).train()

    a, b = make(), make()
    assert isinstance(a[0], LinearBin) and isinstance(a[3], LinearBin)
    fused, ref = utils.FusedQuantAdam(a, **hp), torch.optim.Adam(b.parameters(), **hp)
    plan = utils.clamp_plan(a)
    g = torch.Generator().manual_seed(22)
    worst = torch_worst = 0.0
    for step in range(1, 11):
        x = torch.randn(64, 784, generator=g).to(dev)
        y = torch.randint(0, 10, (64,), generator=g).to(dev)
        for net, opt in ((a, fused), (b, ref)):
            opt.zero_grad()
            torch.nn.functional.cross_entropy(net(x), y).backward()
        before = [(_cpu(p), _cpu(p.grad)) for p in a.parameters()]
        state = [(_cpu(fused.state[p]["exp_avg"]), _cpu(fused.state[p]["exp_avg_sq"])) if fused.state.get(p)
                 else (np.zeros_like(before[i][0]), np.zeros_like(before[i][0])) for i, p in enumerate(a.parameters())]
        fused.step()
        ref.step()
        utils.clamp_weights_(b)
        for i, (p, q) in enumerate(zip(a.parameters(), b.parameters())):
            p64, _, _, bound, _, _ = X.adam_step(before[i][0], before[i][1], state[i][0], state[i][1], step, **hp)
            if p in plan:
                p64 = np.clip(p64, *plan[p])               # clipping is 1-Lipschitz: the bound carries over
            worst = max(worst, X.worst(p, p64, bound))
            torch_worst = max(torch_worst, X.worst(q, p64, bound))       # torch's own step from the same state: printed only
            with torch.no_grad():                          # re-base: parameters and state of the fused side := torch's
                p.copy_(q)
                for k in ("exp_avg", "exp_avg_sq"):
                    fused.state[p][k].copy_(ref.state[q][k])
    print(f"binary MLP, ten steps: worst error / bound = {worst:.3f} (FusedQuantAdam), {torch_worst:.3f} (torch.optim.Adam + clamp)")
    assert worst <= 1.0
    assert float(a[0].weight.detach().abs().max()) <= 1.0
