"""Residual blocks of binarised ResNets inside the deferred sign chain (lazy.DEFER_RESIDUAL_SIGN), on un-modified models.

A Bi-Real-Net style block is ``s = BatchNorm2d(conv(sign(x))) + shortcut`` with the next block reading ``sign([Hardtanh](s))`` and
``s``.  Every result the tests read is ``torch.equal`` to the module-by-module execution (``lazy.eager()``); ``lazy.STATS``, the call
counts of qt_bn_add_sign_f32 and a counter on every conv's ``_forward_impl`` show that each block ran as ONE fused residual block,
that the sum a block emits is reused as the next shortcut without materialising anything, and that no conv ran twice.  All nets are
16 / 20 / 32 channels at 8 x 8, batch 2."""
import pytest
import torch
import torch.nn as nn

from pytorch_quantize_impls_amd import _lib, lazy, utils
from pytorch_quantize_impls_amd.functions import BinaryConnect
from pytorch_quantize_impls_amd.layers import BinConv2d, TerConv2d
from pytorch_quantize_impls_amd.utils import implicit

pytestmark = pytest.mark.gpu

ENTRY = "qt_bn_add_sign_f32"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _switch_is_restored():
    start = lazy.DEFER_RESIDUAL_SIGN
    yield
    assert lazy.DEFER_RESIDUAL_SIGN is start


def _bn(c, g):
    bn = nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g) * 3)
        bn.running_var.copy_(torch.rand(c, generator=g) * 20 + 0.5)
        bn.weight.copy_(torch.randn(c, generator=g))
        bn.bias.copy_(torch.randn(c, generator=g) * 0.5)
    return bn


class Block(nn.Module):
    """sign -> conv -> BatchNorm2d -> + shortcut -> [Hardtanh]; ``form``: how the model writes the add."""

    def __init__(self, conv, bn, hardtanh=False, form="add", shortcut=None):
        super().__init__()
        self.sign, self.conv, self.bn = BinaryConnect(), conv, bn
        self.act = nn.Hardtanh() if hardtanh else None
        self.form, self.shortcut = form, shortcut

    def forward(self, x):
        out = self.bn(self.conv(self.sign(x)))
        sc = x if self.shortcut is None else self.shortcut(x)
        if self.form == "iadd":
            out += sc
        elif self.form == "radd":
            out = sc + out
        elif self.form == "torch.add":
            out = torch.add(out, sc)
        else:
            out = out + sc
        return out if self.act is None else self.act(out)


class Net(nn.Module):
    """Blocks, then a head outside the residual grammar: sign -> [MaxPool2d] -> 1 x 1 BinConv2d -> BatchNorm2d -> arithmetic (so the
    net hands out a plain tensor and the LAST block's sign has a packed consumer, like every block before it).  ``taps``: the sums
    handed out as well, read after the head ran."""

    def __init__(self, blocks, c_last, g, pool=False, taps=()):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)
        self.sign, self.pool = BinaryConnect(), nn.MaxPool2d(2) if pool else None
        self.head, self.head_bn = BinConv2d(c_last, 8, 1), _bn(8, g)
        self.taps = tuple(taps)

    def forward(self, x):
        sums = []
        for b in self.blocks:
            x = b(x)
            sums.append(x)
        t = self.sign(x)
        if self.pool is not None:
            t = self.pool(t)
        y = self.head_bn(self.head(t)) * 1.0
        return (y,) + tuple(sums[i] * 1.0 for i in self.taps) if self.taps else y


def _spread(net, g):
    for m in net.modules():
        if isinstance(m, (BinConv2d, TerConv2d)):
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) * 3 - 1.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g).round())
    return net


def _bireal(dev, n_blocks, c, conv_t=BinConv2d, hardtanh=False, forms=("add",), seed=5, taps=(0,), groups=None, pool=False):
    g = torch.Generator().manual_seed(seed)
    groups = groups or [1] * n_blocks
    blocks = [Block(conv_t(c, c, 3, padding=1, groups=groups[i]), _bn(c, g), hardtanh, forms[i % len(forms)]) for i in range(n_blocks)]
    return _spread(Net(blocks, c, g, pool=pool, taps=taps), g).to(dev).eval()


def _count_convs(net, monkeypatch):
    """Counter per quantised conv of the calls of its ``_forward_impl`` — the route every un-fused evaluation of a conv takes, the
    one inside FusedConvBnAddSign included."""
    calls = {}
    for name, m in net.named_modules():
        if isinstance(m, (BinConv2d, TerConv2d)):
            calls[name] = 0

            def counted(x, _m=m, _name=name, _orig=m._forward_impl):
                calls[_name] += 1
                return _orig(x)
            monkeypatch.setattr(m, "_forward_impl", counted)
    return calls


def _eager(net, x):
    with torch.no_grad(), lazy.eager():
        out = net(x)
    return tuple(t.clone() for t in out) if isinstance(out, tuple) else out.clone()


def _deferred(net, x, on=True):
    lazy.STATS.clear()
    before = _lib.call_counts.get(ENTRY, 0)
    with torch.no_grad(), lazy.residual_deferred(on):
        got = net(x)
    return got, dict(lazy.STATS), _lib.call_counts.get(ENTRY, 0) - before


def _same(got, want):
    if not isinstance(want, tuple):
        got, want = (got,), (want,)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert type(a) is torch.Tensor and a.shape == b.shape and torch.equal(a, b), (i, float((a - b).abs().max()))


def _x(dev, c, seed=9, channels_last=False):
    x = torch.randn((2, c, 8, 8), generator=torch.Generator().manual_seed(seed)).to(dev)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


@pytest.mark.parametrize("conv_t", (BinConv2d, TerConv2d), ids=("bin", "ter"))
@pytest.mark.parametrize("n_blocks, c, hardtanh, forms", [
    (2, 16, False, ("add",)), (3, 20, False, ("iadd", "radd", "torch.add")), (2, 20, True, ("add", "iadd")), (3, 16, True, ("radd",))])
def test_chained_blocks_equal_the_module_graph(dev, monkeypatch, conv_t, n_blocks, c, hardtanh, forms):
    net = _bireal(dev, n_blocks, c, conv_t, hardtanh, forms, taps=tuple(range(n_blocks)))
    for cl in (False, True):
        x = _x(dev, c, channels_last=cl)
        want = _eager(net, x)
        calls = _count_convs(net, monkeypatch)
        got, stats, launches = _deferred(net, x)
        _same(got, want)
        # one fused residual block per block, one launch each; every conv deferred; every conv evaluated exactly once
        assert stats.get("residual_sign_fused") == n_blocks and launches == n_blocks, stats
        assert stats.get("deferred") == n_blocks + 1, stats
        assert all(v == 1 for v in calls.values()), calls
        # the only chain that materialises is the head's (conv, BatchNorm): no sum that is reused or read counts
        assert stats.get("materialised") == 2, stats
        assert not any(k.startswith("fallback:") and "add" in k for k in stats), stats
        monkeypatch.undo()


def test_switch_off_runs_as_without_the_mechanism(dev, monkeypatch):
    """``residual_deferred(False)``: the add is outside the grammar (a counted fallback), every chain in front of it materialises, the
    new entry is never called — and the results are the module graph's."""
    net = _bireal(dev, 2, 16, taps=(0, 1))
    x = _x(dev, 16)
    want = _eager(net, x)
    calls = _count_convs(net, monkeypatch)
    got, stats, launches = _deferred(net, x, on=False)
    _same(got, want)
    assert launches == 0 and "residual_sign_fused" not in stats, stats
    assert sum(v for k, v in stats.items() if k.startswith("fallback:") and "add" in k) == 2, stats
    assert stats.get("deferred") == 3 and stats.get("materialised") == 2 * 2 + 2, stats       # (conv, BatchNorm) of each block, the head
    assert all(v == 1 for v in calls.values()), calls


def test_stride_2_block_with_a_real_valued_shortcut(dev, monkeypatch):
    """The shortcut AvgPool2d -> Conv2d 1 x 1 -> BatchNorm2d is a plain fp32 tensor (NCHW): the LDS-transposed residual form."""
    g = torch.Generator().manual_seed(21)
    sc = nn.Sequential(nn.AvgPool2d(2), nn.Conv2d(16, 32, 1), _bn(32, g))
    blocks = [Block(BinConv2d(16, 16, 3, padding=1), _bn(16, g)),
              Block(BinConv2d(16, 32, 3, stride=2, padding=1), _bn(32, g), shortcut=sc),
              Block(BinConv2d(32, 32, 3, padding=1), _bn(32, g), hardtanh=True)]
    net = _spread(Net(blocks, 32, g, taps=(0, 1, 2)), g).to(dev).eval()
    x = _x(dev, 16)
    want = _eager(net, x)
    assert want[2].shape == (2, 32, 4, 4)                   # (head, then the three sums)
    calls = _count_convs(net, monkeypatch)
    got, stats, launches = _deferred(net, x)
    _same(got, want)
    assert stats.get("residual_sign_fused") == 3 and launches == 3 and all(v == 1 for v in calls.values()), (stats, calls)


@pytest.mark.parametrize("groups", (16, 4), ids=("depthwise", "grouped-4x4"))
def test_depthwise_and_grouped_main_convs(dev, monkeypatch, groups):
    """Block 2's conv is depthwise / has 4 groups of 4: it reads block 1's bit planes, its fp32 value comes from the planes
    (``_fused.packed_depthwise_conv2d`` / ``packed_grouped_conv2d``) and the residual pass runs behind it."""
    net = _bireal(dev, 3, 16, groups=[1, groups, 1], taps=(0, 1, 2), seed=33)
    x = _x(dev, 16)
    want = _eager(net, x)
    calls = _count_convs(net, monkeypatch)
    with lazy.depthwise_deferred(True), lazy.grouped_deferred(True):
        got, stats, launches = _deferred(net, x)
    _same(got, want)
    assert stats.get("residual_sign_fused") == 3 and launches == 3 and all(v == 1 for v in calls.values()), (stats, calls)


def test_maxpool_behind_the_sign(dev, monkeypatch):
    net = _bireal(dev, 2, 16, pool=True, taps=(1,), seed=41)
    x = _x(dev, 16)
    want = _eager(net, x)
    assert want[0].shape == (2, 8, 4, 4)
    calls = _count_convs(net, monkeypatch)
    got, stats, launches = _deferred(net, x)
    _same(got, want)
    assert stats.get("residual_sign_fused") == 2 and launches == 2 and all(v == 1 for v in calls.values()), (stats, calls)


def test_two_deferred_operands_and_a_deferred_shortcut(dev):
    """``bn(conv3x3(t)) + bn(conv1x1(t))`` with both operands deferred: the conv with more MACs keeps the chain, the other one is its
    (materialised) shortcut; then the sum — a deferred activation — is the shortcut of a following block."""
    g = torch.Generator().manual_seed(51)
    main, main_bn = BinConv2d(16, 16, 3, padding=1), _bn(16, g)
    side, side_bn = BinConv2d(16, 16, 1), _bn(16, g)
    nxt, nxt_bn = BinConv2d(16, 16, 3, padding=1), _bn(16, g)
    mods = _spread(nn.ModuleList([main, main_bn, side, side_bn, nxt, nxt_bn]), g).to(dev).eval()
    sign = BinaryConnect()
    x = _x(dev, 16)

    def run():
        t = sign(x)
        s1 = side_bn(side(t)) + main_bn(main(t))
        s2 = nxt_bn(nxt(sign(s1))) + s1
        return s2 * 1.0, s1 * 1.0

    assert mods is not None
    with torch.no_grad(), lazy.eager():
        want = run()
    lazy.STATS.clear()
    with torch.no_grad(), lazy.residual_deferred():
        got = run()
    _same(got, want)
    assert lazy.STATS["residual_sign_fused"] == 1, dict(lazy.STATS)


def test_a_write_to_the_shortcut_before_its_use_is_refused(dev):
    g = torch.Generator().manual_seed(61)
    conv, bn, nxt = BinConv2d(16, 16, 3, padding=1), _bn(16, g), BinConv2d(16, 16, 3, padding=1)
    _spread(nn.ModuleList([conv, bn, nxt]), g).to(dev).eval()
    sign = BinaryConnect()
    x, r = _x(dev, 16), _x(dev, 16, seed=62)
    with torch.no_grad(), lazy.residual_deferred():
        s = bn(conv(sign(x))) + r
        assert isinstance(s, lazy.LazyActivation)
        r.add_(1.0)
        with pytest.raises(RuntimeError, match="modified in place"):
            nxt(sign(s))
        s2 = bn(conv(sign(x))) + r                      # recorded after the write: fine
        y = nxt(sign(s2)) * 1.0
    with torch.no_grad(), lazy.eager():
        assert torch.equal(y, nxt(sign(bn(conv(sign(x))) + r)))


def test_explicit_graph_capture_and_replay(dev):
    net = _bireal(dev, 2, 16, taps=(0, 1), seed=71)
    # channels-last: BinaryConnect then attaches the planes the first conv reads; behind an NCHW input that conv has to ASK the device
    # whether its input is +-1, which no capture permits (tests/test_gpu_implicit_chains.py, _sign_conv_root)
    xs = _x(dev, 16, channels_last=True)
    want = _eager(net, xs)
    with lazy.residual_deferred():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                net(xs)                                 # builds the blocks and their folds (the probe synchronises)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        before = _lib.call_counts.get(ENTRY, 0)
        with torch.no_grad(), torch.cuda.graph(graph):
            out = net(xs)
        assert _lib.call_counts[ENTRY] == before + 2
    for seed in (72, 73):
        xs.copy_(_x(dev, 16, seed=seed, channels_last=True))
        graph.replay()
        torch.cuda.synchronize()
        _same(tuple(t.clone() for t in out), _eager(net, xs))
    assert not torch.equal(out[0], want[0])


def test_the_default_implicit_graph_replays_the_chain(dev, monkeypatch):
    """The configuration users get (tests/test_gpu_implicit_chains.py): eager twice, captured in the third call, replayed after."""
    monkeypatch.setattr(implicit, "KEEP_IF_FASTER", 0.0)          # no verdict by the clock on a model this small
    net = _bireal(dev, 2, 16, taps=(), seed=81)
    x, x2 = _x(dev, 16, channels_last=True), _x(dev, 16, seed=82, channels_last=True)       # (see the explicit capture above)
    want, want2 = _eager(net, x), _eager(net, x2)
    with utils.implicit_graphs(True), lazy.residual_deferred(), torch.no_grad():
        counts = []
        for i in range(5):
            assert ("forward" in net.__dict__) == (i >= 2), (i, utils.implicit_graph_stats(net))
            before = _lib.call_counts.get(ENTRY, 0)
            _same(net(x), want)
            counts.append(_lib.call_counts.get(ENTRY, 0) - before)
        # eager twice; the third call captures (and runs the forward again around the capture); replays launch nothing from the host
        assert counts[:2] == [2, 2] and counts[2] >= 2 and counts[3:] == [0, 0], counts
        st = utils.implicit_graph_stats(net)
        assert st["wrapped"] and st["graphs"] == 1 and st["value_mismatch"] == 0 and st["capture_failures"] == {} and st["replays"] >= 3, st
        _same(net(x2), want2)
        assert utils.implicit_graph_stats(net)["replays"] == st["replays"] + 1
