"""Every fused inference chain under the configuration users get: implicit hipGraphs ON (utils/implicit.py).

The suite runs with ``QT_AUTO_GRAPH=0`` (tests/conftest.py: it counts launches, which replays hide), so the chain families were only
ever tested eagerly or under an explicit ``utils.graphed``.  Here a small, un-modified eval-mode root per family is called the way a
user calls it — twice eagerly, captured on a side stream in the third call, replayed from then on — and the REPLAYS are checked:
against the module-by-module execution (``implicit_graphs(False)`` + ``lazy.eager()``), for the sign families against a plain-torch
float64 restatement that is exact by construction, on later inputs of the same signature (the wrapper itself verifies only the first
replay), after state changes, for further signatures, and by the wrapper's counters (a declined capture or a value mismatch would
otherwise only be a silent performance regression).

Roots whose own result is a deferred activation get a consumer outside the grammar (``_Read``): a root that returns a deferred
activation — a ``LazyActivation``, or the ``LazyDense`` of a model that ends in LinearBin / LinearTer / LinearXNOR — is left eager by
design ("deferred output"), which test_a_root_that_returns_a_deferred_activation_stays_eager pins.

DoReFa code chains and the un-clamped quantiser: an input whose activation codes leave int8 makes the deferred code chain return NaN
(packed.CodeActivation: "there is no fp32 image to fall back to") where the module-by-module execution keeps the fp32 route.  That is
the chain's documented poisoning, with or without a graph; a replay has to reproduce the un-replayed deferred forward bit for bit, NaN
for NaN, and the module-by-module value wherever the chain is not poisoned.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bench_models
from conftest import norm_err
from test_gpu_dw_codes import _input as _dw_codes_input, _net as _dw_codes_net
from test_gpu_dwconv_chain import _pm1, _stack
from test_gpu_elastic import _convnet
from test_gpu_gconv_chain import _triple
from test_gpu_half import _binary_net
from pytorch_quantize_impls_amd import _lib, lazy, utils
from pytorch_quantize_impls_amd.functions import BinaryConnect, nnDorefaQuant
from pytorch_quantize_impls_amd.layers import (BinConv2d, LinearBin, LinearTer, LinearXNOR, QLayer, TerConv2d, XNORConv2d,
                                               WQR_layers as WL)
from pytorch_quantize_impls_amd.layers.elastic_layers import LossQuantMixin
from pytorch_quantize_impls_amd.utils import implicit
from pytorch_quantize_impls_amd.utils.graphs import _any_training

pytestmark = pytest.mark.gpu

TOL = 1e-5                   # the float-tail contract of the real-valued routes (test_gpu_elastic.py)
_SIGN_LAYERS = (BinConv2d, TerConv2d, LinearBin, LinearTer)
_BN = (nn.BatchNorm1d, nn.BatchNorm2d)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _replay_whatever_the_clock_says(monkeypatch):
    """KEEP_IF_FASTER = 0 switches the wall-clock verdict off ("a replay must need < 0.9 x the eager time"): on models this small it
    would decide by timing noise whether anything is replayed at all, and no test here may depend on the clock.  The verdict keeps
    its own test (test_gpu_r6.py::test_implicit_graph_keeps_a_device_bound_forward_eager)."""
    monkeypatch.setattr(implicit, "KEEP_IF_FASTER", 0.0)
    start = (lazy.ENABLED, lazy.DEFER_CODES, lazy.DEFER_DENSE, lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES, lazy.DEFER_GROUPED)
    yield
    assert (lazy.ENABLED, lazy.DEFER_CODES, lazy.DEFER_DENSE, lazy.DEFER_DEPTHWISE, lazy.DEFER_DEPTHWISE_CODES,
            lazy.DEFER_GROUPED) == start


def _is_sign(mod):
    """BinaryConnect() — a factory: the module that applies the deterministic sign Function."""
    return getattr(getattr(mod, "core", None), "_qt_records_sign", False)


class _Read(nn.Module):
    """A consumer outside the chain grammar (arithmetic on the result): what the root hands out is a plain tensor."""

    def forward(self, x):
        return x * 1.0


# ---- roots -------------------------------------------------------------------------------------------------------------------------

def _bn_run(c, g, one_d=False):
    """BatchNorm (random statistics, weights +- a power of two, every third negative) -> Hardtanh -> BinaryConnect."""
    bn = (nn.BatchNorm1d if one_d else nn.BatchNorm2d)(c)
    bn.running_mean.copy_(torch.randn(c, generator=g) * 3)
    bn.running_var.copy_(torch.rand(c, generator=g) * 20 + 5)
    gamma = torch.exp2(torch.randint(-1, 2, (c,), generator=g).float())
    gamma[::3] *= -1
    bn.weight.data.copy_(gamma)
    bn.bias.data.copy_(torch.randn(c, generator=g) * 0.5)
    return [bn, nn.Hardtanh(inplace=True), BinaryConnect()]


def _spread(root, g):
    """Latent weights over [-1.5, 1.5] (the default initialisation lies inside the ternary dead zone), small biases."""
    for m in root.modules():
        if isinstance(m, _SIGN_LAYERS + (XNORConv2d, LinearXNOR)):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * 3 - 1.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 2)
    return root


def _exactify(root, first_grid=1.0):
    """Make every sign decision of a sign-family root exact in fp32 and in float64 alike.  Sums of +-1 / 0 products are integers
    (behind a real-valued image of multiples of 1/8: multiples of ``first_grid`` = 1/8), so with integer conv / linear biases,
    BatchNorm ``running_mean`` on the half-grid between two attainable sums, ``bias`` = 0 and ``weight`` = +- a power of two,
    ``x - mean`` is exact and never 0 and the sign of BatchNorm's value is sign(x - mean) * sign(weight) in any arithmetic."""
    with torch.no_grad():
        grid = first_grid
        for m in root.modules():
            if isinstance(m, _SIGN_LAYERS) and m.bias is not None:
                m.bias.data.round_()
            elif isinstance(m, _BN):
                m.running_mean.copy_((torch.floor(m.running_mean / grid) + 0.5) * grid)
                w = m.weight.data
                w.copy_(torch.sign(w) * torch.exp2(torch.round(torch.log2(w.abs()))))
                m.bias.data.zero_()
                assert bool((w != 0).all()) and bool((m.running_var > 0).all())
                grid = 1.0
    return root


def _sign_conv_root(dev, seed=31):
    """real-valued 3 -> 32 3x3 BinConv2d -> run -> BinConv2d 3x3 -> MaxPool2d(2) -> run -> TerConv2d -> run -> flatten -> LinearBin ->
    BatchNorm1d / Hardtanh / sign -> LinearTer; only weights train (frozen BatchNorm fine-tuning keeps the statistics on their grid).
    128 channels in front of the flatten: the hand-over of a flattened chain to a Linear layer as row planes needs un-padded pixel
    rows (a multiple of 128 channels); with fewer the chain materialises, the Linear layer has to ASK the device whether its
    un-tagged input is +-1, and the capture is refused for that ("operation not permitted when stream is capturing" in
    ``capture_failures``) — documented behaviour, the signature stays eager."""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    root = nn.Sequential(BinConv2d(3, 32, 3, padding=1), *_bn_run(32, g),
                         BinConv2d(32, 48, 3, padding=1), nn.MaxPool2d(2), *_bn_run(48, g),
                         TerConv2d(48, 128, 3, padding=1), *_bn_run(128, g),
                         nn.Flatten(), LinearBin(128 * 5 * 5, 96), *_bn_run(96, g, one_d=True),
                         LinearTer(96, 10), _Read())
    root[0].binary_input = False
    _exactify(_spread(root, g), first_grid=0.125)
    for name, p in root.named_parameters():
        p.requires_grad_(name.endswith("weight") and isinstance(root[int(name.split(".")[0])], _SIGN_LAYERS))
    return root.to(dev).eval()


def _eighths(shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.round(torch.randn(shape, generator=g) * 16) / 8).to(dev)


def _gauss(shape, dev, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


class _DorefaNet(nn.Module):
    """fp32 stem conv -> BatchNorm -> ReLU -> nnDorefaQuant(4) -> one W1A4 _DorefaBlock with a strided 1x1 shortcut -> avg pool -> Linear."""

    def __init__(self):
        super().__init__()
        self.stem, self.bn, self.quant = nn.Conv2d(3, 16, 3, padding=1, bias=False), nn.BatchNorm2d(16), nnDorefaQuant(4)
        self.block = bench_models._DorefaBlock(16, 32, 2, 1, 4)
        self.linear = nn.Linear(32, 10)

    def codes_input(self, x):
        return self.quant(torch.relu(self.bn(self.stem(x))))

    def forward(self, x):
        out = self.block(self.codes_input(x))
        return self.linear(F.avg_pool2d(out, out.shape[-1]).flatten(1))


def _dorefa_root(dev):
    torch.manual_seed(4)
    m = _DorefaNet()
    bench_models.randomize_bn(m, seed=3)
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.running_var.mul_(4.0)
    return m.to(dev).to(memory_format=torch.channels_last).eval()


def _xnor_root(dev, seed=37, sign_before_flatten=False):
    """XNORConv2d (real-valued first layer) -> run -> XNORConv2d -> BatchNorm / Hardtanh -> flatten -> sign -> LinearXNOR: the
    classifier opens with its BinaryConnect BEHIND the flatten, as models/Alexnet/Alexnet_Bin.py writes it, so that module by
    module the Linear layer gets a tensor that still carries the sign planes of its quantiser and runs the same packed GEMM as the
    deferred chain.  ``sign_before_flatten``: the other order, whose module-by-module execution legitimately takes another launch
    (test_xnor_linear_behind_a_flatten_of_signs_takes_the_float_route_module_by_module)."""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    bn, hardtanh, sign = _bn_run(128, g)
    tail = [bn, hardtanh, sign, nn.Flatten()] if sign_before_flatten else [bn, hardtanh, nn.Flatten(), sign]
    root = nn.Sequential(XNORConv2d(3, 32, 3, padding=1), *_bn_run(32, g),
                         XNORConv2d(32, 128, 3, padding=1), *tail, LinearXNOR(128 * 8 * 8, 10), _Read())
    root[0].binary_input = False
    return _spread(root, g).to(dev).eval()


def _loss_aware_root(dev, which):
    """The 2-conv + 1-linear net of test_gpu_elastic.py as Elastic Log (its ``_convnet``), Elastic Lin and WQR Log layers.  The
    converters copy the float net's small initial weights, which all project onto the level next to zero — a net that ignores
    its weights' signs and, for Lin, its input: the weights are drawn again over the level range, the biases at random, before
    ``eval()``."""
    torch.manual_seed(6)
    if which == "elastic-log":
        net = _convnet()
    else:
        net = nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), nn.ReLU(), nn.Conv2d(16, 16, 3, padding=1), nn.Flatten(), nn.Linear(16 * 8 * 8, 10))
        if which == "elastic-lin":
            net = utils.loss_quant_lin_convert(net, alpha=0.03, beta=0.01)
        else:
            kw = {"kapa": 0.03, "beta": 0.01}
            net = utils.convert(net, {nn.Linear: (WL.LinearQuantWLog, kw), nn.Conv2d: (WL.QuantConv2dWLog, kw)})
    for m in net.modules():
        if isinstance(m, LossQuantMixin):
            m.weight.data.uniform_(*m._range())
            m.bias.data.uniform_(-0.5, 0.5)
    return net.to(dev).eval()


class Family:
    """One row of the table: ``root`` (eval mode, on the device), ``x`` and ``fresh(seed)`` (other data of the same kind);
    ``exact``: the float64 restatement equals the device bit for bit; ``tol``: it does within ``norm_err <= tol``; ``route``: the
    C-ABI entry whose counter has to move while the third call captures; ``codes``: the stem whose int8 activation codes the input
    scaled by 64 has to leave; ``trains``: the family also takes the train -> FusedQuantSGD step -> eval change."""

    def __init__(self, name, dev):
        self.name, self.exact, self.tol, self.route, self.codes, self.trains = name, False, None, None, None, False
        cl = torch.channels_last
        if name in ("sign-nchw", "sign-cl"):
            self.root, self.exact, self.trains = _sign_conv_root(dev), True, name == "sign-nchw"
            self.fresh = lambda s: _eighths((3, 3, 10, 10), dev, s).contiguous(memory_format=cl if name == "sign-cl" else torch.contiguous_format)
        elif name == "depthwise":
            seq = _stack(dev)
            seq[0].binary_input = True      # the +-1 hint: nothing asks the device about the input while the graph is captured
            self.root, self.exact, self.route = _exactify(nn.Sequential(*seq, _Read()).eval()), True, "qt_dwconv2d_sign"
            self.fresh = lambda s: _pm1((3, 16, 12, 12), dev, s)
        elif name in ("grouped", "grouped-pool"):
            seq = _triple(dev, BinConv2d(32, 64, 3, padding=1, groups=8), "before_bn" if name == "grouped-pool" else None)
            seq[0].binary_input = True
            self.root, self.exact, self.route = _exactify(nn.Sequential(*seq, _Read()).eval()), True, "qt_gconv2d_sign"
            self.fresh = lambda s: _pm1((3, 16, 10, 10), dev, s)
        elif name == "dorefa":
            self.root, self.route, self.trains = _dorefa_root(dev), "qt_conv2d_implicit_codes", True
            self.codes = self.root.codes_input
            self.fresh = lambda s: _gauss((2, 3, 12, 12), dev, s).contiguous(memory_format=cl)
        elif name == "dw-codes":
            self.root, self.route = _dw_codes_net(dev), "qt_dwconv2d_codes"
            self.codes = self.root.stem
            self.fresh = lambda s: _dw_codes_input(dev, seed=s)
        elif name == "xnor":
            self.root = _xnor_root(dev)
            self.fresh = lambda s: _gauss((2, 3, 8, 8), dev, s)
        else:
            self.root, self.tol = _loss_aware_root(dev, name), TOL
            self.fresh = lambda s: _gauss((4, 3, 8, 8), dev, s)
        self.x = self.fresh(101)


FAMILIES = ("sign-nchw", "sign-cl", "depthwise", "grouped", "grouped-pool", "dorefa", "dw-codes", "xnor", "elastic-lin", "elastic-log",
            "wqr-log")


# ---- references ------------------------------------------------------------------------------------------------------------------------

def _module_by_module(root, x):
    with torch.no_grad(), utils.implicit_graphs(False), lazy.eager():
        y = root(x)
    assert type(y) is torch.Tensor
    return y.clone()


def _unreplayed(root, x):
    """The default deferred forward without a graph: what calls 1 and 2 run."""
    with torch.no_grad(), utils.implicit_graphs(False):
        y = root(x)
    assert type(y) is torch.Tensor
    return y.clone()


def _ref64(root, x):
    """The root restated in plain torch, float64, on the CPU, from the modules' own parameters: conv2d / linear on the stored
    (quantised, or for the loss-aware layers projected) weight image, eval BatchNorm, Hardtanh, sign with x >= 0 -> +1.  Returns
    (value, number of pre-sign values that are exactly 0)."""
    zeros = []

    def p64(t):
        return None if t is None else t.detach().double().cpu()

    def run(mod, t):
        if isinstance(mod, nn.Sequential):
            for child in mod:
                t = run(child, t)
            return t
        if isinstance(mod, _SIGN_LAYERS):
            w = p64(mod.weight)
            assert not mod.training and bool(((w == 0) | (w.abs() == 1)).all()), "eval mode stores the quantised image"
        elif isinstance(mod, WL._WqrTrain):
            w = p64(mod.weight)                     # eval() stored the projection; the forward takes the weight as it is
        elif isinstance(mod, LossQuantMixin):
            w = p64(mod._project(mod.weight.detach()))
        if isinstance(mod, nn.Conv2d):
            return F.conv2d(t, w, p64(mod.bias), mod.stride, mod.padding, mod.dilation, mod.groups)
        if isinstance(mod, (LinearBin, LinearTer)) or (isinstance(mod, LossQuantMixin) and hasattr(mod, "in_features")):
            return F.linear(t, w, p64(mod.bias))
        if isinstance(mod, _BN):
            shape = (1, -1, 1, 1) if t.dim() == 4 else (1, -1)
            mean, var, gamma, beta = (p64(q).view(shape) for q in (mod.running_mean, mod.running_var, mod.weight, mod.bias))
            return (t - mean) / torch.sqrt(var + mod.eps) * gamma + beta
        if isinstance(mod, nn.Hardtanh):
            return t.clamp(mod.min_val, mod.max_val)
        if _is_sign(mod):
            zeros.append(int((t == 0).sum()))
            return torch.where(t >= 0, torch.ones_like(t), -torch.ones_like(t))
        if isinstance(mod, nn.MaxPool2d):
            return F.max_pool2d(t, mod.kernel_size, mod.stride, mod.padding)
        if isinstance(mod, nn.ReLU):
            return torch.relu(t)
        if isinstance(mod, nn.Flatten):
            return t.flatten(1)
        if isinstance(mod, _Read):
            return t
        raise TypeError(f"no float64 restatement of {type(mod).__name__}")

    y = run(root, x.detach().double().cpu())
    assert y.dtype == torch.float64
    return y, sum(zeros)


def _reference(fam, x):
    """The value every call has to return bit for bit: the module-by-module execution."""
    return _module_by_module(fam.root, x)


def _check_reference(fam, want, x, what):
    """``want`` (module by module, on the device) against the float64 restatement of the root's present state."""
    if not (fam.exact or fam.tol):
        return
    ref, zeros = _ref64(fam.root, x)
    if fam.exact:
        assert zeros == 0, (fam.name, what, "a pre-sign value lies on the boundary")
        assert torch.equal(want.double().cpu(), ref), (fam.name, what, float((want.double().cpu() - ref).abs().max()))
    else:
        err = norm_err(want.cpu().numpy(), ref.numpy())
        print(f"IMPLICIT-REF {fam.name} {what}: norm_err {err:.3e}")
        assert err <= fam.tol, (fam.name, what, err)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.allclose(a, b, rtol=0.0, atol=0.0, equal_nan=True)) \
        and bool(torch.equal(torch.isnan(a), torch.isnan(b)))


def _stats(root):
    return utils.implicit_graph_stats(root)


def _five_calls(root, x, want, route=None):
    """Calls 1 - 5 with one input.  Returns the results; asserts what the wrapper owes on the way: eager twice, wrapped during the
    second call, the capture in the third (the family's fused entry is launched from the host there), replays — no C-ABI call at
    all — in the fourth and fifth, results that are copies."""
    ys, counts = [], []
    with torch.no_grad():
        for i in range(5):
            assert ("forward" in root.__dict__) == (i >= 2), (i, _stats(root))
            before = dict(_lib.call_counts)
            ys.append(root(x))
            after = dict(_lib.call_counts)
            counts.append({k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)})
    for i, y in enumerate(ys):
        assert type(y) is torch.Tensor and torch.equal(y, want), i
    assert ys[3].data_ptr() != ys[4].data_ptr()
    assert counts[2], "the capturing call launched nothing from the host"
    if route is not None:
        assert counts[2].get(route, 0) > 0, (route, counts[2])
    assert counts[3] == {} and counts[4] == {}, ("a replay issued launches from the host", counts[3], counts[4])
    return ys


def _replaying(st, graphs=1):
    return (st["wrapped"] and st["graphs"] == graphs and st["value_mismatch"] == 0 and st["capture_failures"] == {}
            and st["eager_signatures"] == 0 and st["not_faster"] == 0 and st["left_eager"] is None)


# ---- A: the table ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_family_replays_under_the_default_configuration(dev, name):
    fam = Family(name, dev)
    root, x = fam.root, fam.x
    assert not _any_training(root), "an eval-mode root"
    with utils.implicit_graphs(True):
        # 1. reference values: module by module, and against float64
        want = _reference(fam, x)
        assert bool(torch.isfinite(want).all()) and float(want.std()) > 0
        _check_reference(fam, want, x, "initial state")
        assert "forward" not in root.__dict__
        # 2. five calls with one input (and 8.: the routes, inside _five_calls)
        _five_calls(root, x, want, fam.route)
        st = _stats(root)
        print(f"IMPLICIT-STATS {name}: graphs={st['graphs']} replays={st['replays']} captures={st['captures']} "
              f"capture_failures={st['capture_failures']} value_mismatch={st['value_mismatch']} eager_signatures={st['eager_signatures']}")
        assert _replaying(st) and st["replays"] >= 3 and st["captures"] == 1, st
        # 3. later inputs of the same signature: only the first replay was verified by the wrapper
        later = [("other data", fam.fresh(202)), ("scaled by 64", x * 64.0), ("negated", -x), ("other data again", fam.fresh(303))]
        if fam.codes is not None:
            with torch.no_grad(), utils.implicit_graphs(False), lazy.eager():
                assert float(fam.codes(x * 64.0).abs().max()) * 15 > 127, "the scaled input has to leave the int8 code range"
        for what, xi in later:
            assert xi.shape == x.shape and xi.stride() == x.stride()
            want_i, chain_i = _reference(fam, xi), _unreplayed(root, xi)
            r = _stats(root)["replays"]
            with torch.no_grad():
                got = root(xi)
            st = _stats(root)
            poisoned = int(torch.isnan(chain_i).sum())
            print(f"IMPLICIT-LATER {name} {what}: NaN in replay {int(torch.isnan(got).sum())}, un-replayed chain {poisoned}, "
                  f"module by module {int(torch.isnan(want_i).sum())} of {got.numel()}")
            assert type(got) is torch.Tensor and st["replays"] == r + 1 and _replaying(st), (what, st)
            assert _same(got, chain_i), (name, what)
            if poisoned:        # the un-clamped quantiser left int8: the code chain's documented poisoning, reproduced NaN for NaN
                assert fam.codes is not None and what == "scaled by 64" and poisoned == got.numel(), (name, what, poisoned)
            else:
                assert _same(got, want_i), (name, what)
            if what.startswith("other data"):
                assert not torch.equal(got, want)
        # 5. signatures: batch 1 and the other memory format each get a graph of their own
        twin = x.contiguous() if not x.is_contiguous() else x.contiguous(memory_format=torch.channels_last)
        graphs = 1
        for what, xs in (("batch 1", x[:1]), ("other memory format", twin)):
            assert (tuple(xs.shape), tuple(xs.stride())) != (tuple(x.shape), tuple(x.stride())), what
            want_s = _reference(fam, xs)
            _check_reference(fam, want_s, xs, what)
            with torch.no_grad():
                for _ in range(3):
                    assert torch.equal(root(xs), want_s), what
            graphs += 1
            st = _stats(root)
            assert _replaying(st, graphs) and graphs <= root.forward.engine.max_graphs, (what, st)
        with torch.no_grad():
            assert torch.equal(root(x), want)                   # the first signature's graph is still the first signature's
        # 4. state changes: the graphs baked the old planes / folds / thresholds in
        qlayers = [m for m in root.modules() if isinstance(m, QLayer)]
        bns = [m for m in root.modules() if isinstance(m, _BN)]
        changes = [("weight.mul_(-1)", lambda: qlayers[len(qlayers) // 2].weight.mul_(-1.0))]
        if bns:
            changes.append(("running_mean.add_(4)", lambda: bns[len(bns) // 2].running_mean.add_(4.0)))
        if fam.trains:
            changes.append(("train, FusedQuantSGD step, eval", lambda: _train_one_step(root, x)))
        old = want
        for what, change in changes:
            before = _stats(root)
            with torch.no_grad():
                change()
            new = _reference(fam, x)
            _check_reference(fam, new, x, "after " + what)
            assert bool(torch.isfinite(new).all()) and not torch.equal(new, old), (name, what, "the change does not reach the output")
            with torch.no_grad():
                for i in range(4):
                    assert torch.equal(root(x), new), (name, what, i)
            st = _stats(root)
            print(f"IMPLICIT-CHANGE {name} {what}: {st}")
            assert _replaying(st) and st["replays"] >= before["replays"] + 3 and st["captures"] == before["captures"] + 1, \
                (what, str(before), str(st))
            old = new


def _train_one_step(root, x):
    """model.train(); one step of the fused optimiser (it bumps the version counters itself); model.eval().  BatchNorm modules
    stay in eval mode where the root froze their parameters (fine-tuning on frozen statistics)."""
    with torch.enable_grad():
        root.train()
        for m in root.modules():
            if isinstance(m, _BN) and not m.weight.requires_grad:
                m.eval()
        # (sign layers: a step large enough to flip signs, the fused clamp keeps the latent weights in [-1, 1]; the DoReFa net
        # trains every parameter, BatchNorm and the fp32 head included: a small step that keeps the activations where they were)
        opt = utils.FusedQuantSGD(root, lr=0.5 if any(isinstance(m, _SIGN_LAYERS) for m in root.modules()) else 1e-3)
        out = root(x)
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).to(out.device)
        (out * g).sum().backward()
        opt.step()
        root.zero_grad(set_to_none=True)
    root.eval()


def test_xnor_linear_behind_a_flatten_of_signs_takes_the_float_route_module_by_module(dev):
    """Why the XNOR root puts its flatten in front of the sign.  With ``sign -> flatten -> LinearXNOR`` the two executions differ
    in ONE launch, legitimately: module by module the flatten hands LinearXNOR a new tensor without the sign planes BinaryConnect
    attached to its result, so the layer asks the device whether the input is +-1 (qt_check_pm1_f32) and multiplies on the bf16
    split (qt_bf16_gemm); the deferred chain hands over row planes and runs the int8 head (qt_xnor_head_i8).  Both are sums of
    +- alpha_k with different accumulation: equal within the float-tail contract, not bit for bit — and the convs in front are
    bit-identical.  (The question to the device is also why such a root, module by module, could not be captured.)"""
    root, x = _xnor_root(dev, sign_before_flatten=True), _gauss((2, 3, 8, 8), dev, 101)
    convs = nn.Sequential(*list(root)[:9]).eval()
    assert _is_sign(root[7]) and isinstance(root[8], nn.Flatten) and isinstance(root[9], LinearXNOR)

    def counted(fn):
        before = dict(_lib.call_counts)
        y = fn()
        after = dict(_lib.call_counts)
        return y, {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}

    with torch.no_grad(), utils.implicit_graphs(False):
        with lazy.eager():
            flat_eager = convs(x)
            want, c_eager = counted(lambda: root(x))
        assert torch.equal(convs(x) * 1.0, flat_eager)              # the deferred convs: the module-by-module bits
        got, c_chain = counted(lambda: root(x))
    assert c_eager.get("qt_bf16_gemm", 0) == 1 and c_eager.get("qt_check_pm1_f32", 0) >= 1 and "qt_xnor_head_i8" not in c_eager, c_eager
    assert c_chain.get("qt_xnor_head_i8", 0) == 1 and "qt_bf16_gemm" not in c_chain and "qt_check_pm1_f32" not in c_chain, c_chain
    err = norm_err(got.cpu().numpy(), want.cpu().numpy())
    print(f"IMPLICIT-XNOR sign before flatten: deferred against module by module, norm_err {err:.3e}")
    assert err <= TOL, err
    # the order the table uses: the tag survives, one launch for both, the same bits
    root2 = _xnor_root(dev)
    with torch.no_grad(), utils.implicit_graphs(False):
        with lazy.eager():
            want2, c2 = counted(lambda: root2(x))
        got2, c2d = counted(lambda: root2(x))
    assert "qt_bf16_gemm" not in c2 and torch.equal(got2, want2), (c2, c2d)


# ---- 6. deferred outputs ---------------------------------------------------------------------------------------------------------------

def test_a_block_with_a_deferred_result_inside_the_real_root_replays(dev):
    """The depthwise stack as ONE child whose own result is a deferred activation; the root the user calls is the Sequential around
    it and its consumer: that root is wrapped, not the block."""
    seq = _stack(dev)
    seq[0].binary_input = True
    root, x = nn.Sequential(seq, _Read()).eval(), _pm1((3, 16, 12, 12), dev)
    with utils.implicit_graphs(True):
        with torch.no_grad(), utils.implicit_graphs(False):
            assert isinstance(seq(x), lazy.LazyActivation)
        want = _module_by_module(root, x)
        _five_calls(root, x, want, "qt_dwconv2d_sign")
        st = _stats(root)
        assert _replaying(st) and st["replays"] >= 3 and "forward" not in seq.__dict__, st
        x2 = _pm1((3, 16, 12, 12), dev, 9)
        with torch.no_grad():
            assert torch.equal(root(x2), _module_by_module(root, x2))
        assert _replaying(_stats(root))


@pytest.mark.parametrize("ending", ("conv", "linear"))
def test_a_root_that_returns_a_deferred_activation_stays_eager(dev, ending):
    """A root whose result goes to the user as a deferred activation — the storage-less LazyActivation of a conv chain, or the
    LazyDense of a model that ends in LinearTer — is captured once, refused ("deferred output": its consumer would lose the fused
    hand-over) and left eager for that signature, with the right values and the deferred type."""
    if ending == "conv":
        root, x = _stack(dev), _pm1((3, 16, 12, 12), dev)
        root[0].binary_input = True
    else:
        full = _sign_conv_root(dev)
        root, x = nn.Sequential(*list(full)[:-1]).eval(), _eighths((3, 3, 10, 10), dev, 101)
    with utils.implicit_graphs(True):
        with torch.no_grad(), utils.implicit_graphs(False), lazy.eager():
            want = root(x).clone()
        with torch.no_grad():
            ys = [root(x) for _ in range(5)]
        for y in ys:
            assert isinstance(y, lazy.LazyActivation) and torch.equal(y.value() if ending == "conv" else y * 1.0, want)
        st = _stats(root)
        print(f"IMPLICIT-STATS deferred-output-{ending}: graphs={st['graphs']} replays={st['replays']} captures={st['captures']} "
              f"capture_failures={st['capture_failures']}")
        assert st["wrapped"] and st["capture_failures"] == {"deferred output": 1} and st["graphs"] == 0 and st["replays"] == 0, st
        assert st["eager_signatures"] == 1 and st["value_mismatch"] == 0 and st["captures"] == 1, st


# ---- 7. half ---------------------------------------------------------------------------------------------------------------------------

def test_a_bf16_model_is_never_wrapped(dev):
    net = _binary_net(dev, torch.bfloat16).eval()
    x = (_pm1((8, 32, 16, 16), dev, 5)).to(torch.bfloat16)
    with torch.no_grad(), utils.implicit_graphs(False):
        want = net(x).clone()
    with utils.implicit_graphs(True), torch.no_grad():
        ys = [net(x) for _ in range(5)]
        st = _stats(net)
    assert "forward" not in net.__dict__
    assert st["wrapped"] is False and st["opted_out"] is False and st["why"].startswith("not now") and "fp32" in st["why"], st
    for y in ys:
        assert y.dtype == torch.bfloat16 and torch.equal(y, want)
