"""The deferred level chain of the Lin / Log family (lazy.py, kind "levels") as far as it can be checked without a device: the
switch and its default, the C-ABI declarations, the exported modules, the grammar's book-keeping on CPU models (nothing is ever
deferred there)."""
import os
import re

import torch
import torch.nn.functional as F

from pytorch_quantize_impls_amd import _lib, lazy, layers, ops, packed
from pytorch_quantize_impls_amd.functions import log_lin_connect
from pytorch_quantize_impls_amd.layers import LinearQuant, QuantConv2d

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW_ENTRY_POINTS = ("qt_conv2d_implicit_levels", "qt_pool_levels_bf16", "qt_bn_relu_linlog_bf16_f32")


class _Net(torch.nn.Module):
    """QuantConv2d -> BatchNorm2d -> ReLU -> nnQuant -> MaxPool2d -> flatten -> LinearQuant -> BatchNorm1d -> ReLU -> nnQuant -> LinearQuant."""

    def __init__(self, dtype):
        super().__init__()
        self.q = log_lin_connect.nnQuant("lin", 1, 8, with_sign=False)
        self.c1 = QuantConv2d(3, 8, 3, padding=1, fsr=2, bit_width=3, dtype=dtype)
        self.c2 = QuantConv2d(8, 8, 3, padding=1, fsr=2, bit_width=3, dtype=dtype)
        self.b1, self.b2, self.b3 = torch.nn.BatchNorm2d(8), torch.nn.BatchNorm2d(8), torch.nn.BatchNorm1d(12)
        self.l1 = LinearQuant(8 * 16, 12, fsr=1, bit_width=3, dtype=dtype)
        self.l2 = LinearQuant(12, 5, fsr=1, bit_width=3, dtype=dtype)

    def forward(self, x):
        x = self.q(torch.relu(self.b1(self.c1(x))))
        x = F.max_pool2d(self.q(torch.relu(self.b2(self.c2(x)))), 2)
        x = self.q(torch.relu(self.b3(self.l1(x.flatten(1)))))
        return self.l2(x)


def test_switch_is_off_by_default_and_scoped():
    assert lazy.DEFER_LEVELS is False
    with lazy.levels_deferred():
        assert lazy.DEFER_LEVELS is True
        with lazy.levels_deferred(False):
            assert lazy.DEFER_LEVELS is False
        assert lazy.DEFER_LEVELS is True
    assert lazy.DEFER_LEVELS is False


def test_entry_points_declared_and_bound():
    declared = _lib.header_declared_functions()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    # argument counts of the bindings against the header's declarations
    with open(os.path.join(ROOT, "include", "qt_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        args = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_new_modules_are_exported():
    for name in ("FusedLogLinConvBnQuant", "LevelMaxPool", "FusedBnLogLinQuant"):
        assert hasattr(layers, name) and issubclass(getattr(layers, name), torch.nn.Module), name
        assert hasattr(getattr(layers, name), "forward")
    for name in ("FusedLogLinConvBnQuant", "FusedBnLogLinQuant"):
        assert callable(getattr(getattr(layers, name), "refold"))
    assert hasattr(packed, "LevelActivation") and callable(lazy.levels) and callable(lazy.levels_deferred)


def test_cpu_model_under_the_switch_returns_plain_equal_tensors():
    for dtype in ("lin", "log"):
        torch.manual_seed(3)
        m = _Net(dtype)
        with torch.no_grad():
            for bn in (m.b1, m.b2, m.b3):
                bn.running_mean.normal_()
                bn.running_var.uniform_(0.5, 2.0)
        m.eval()
        x = torch.randn(4, 3, 8, 8)
        before = dict(lazy.STATS)
        with torch.no_grad():
            want = m(x)
            with lazy.levels_deferred():
                got = m(x)
                mid = m.c1(x)
        assert type(got) is torch.Tensor and type(mid) is torch.Tensor and not isinstance(got, lazy.LazyActivation)
        assert torch.equal(got, want)
        assert dict(lazy.STATS) == before            # nothing is deferred, fused or materialised on a CPU model
        # autograd through the switch: training mode is never deferred either
        m.train()
        with lazy.levels_deferred():
            y = m(x)
        assert y.requires_grad and type(y) is torch.Tensor


def test_quantiser_functions_carry_their_spec():
    assert log_lin_connect.LinQuant(fsr=1, bit_width=8, with_sign=False)._qt_level_spec == ("lin", 1, 8, False)
    assert log_lin_connect.LogQuant(fsr=2, bit_width=3)._qt_level_spec == ("log", 2, 3, True)
    assert log_lin_connect.nnQuant("log", 0, 2).core._qt_level_spec == ("log", 0, 2, True)
    x = torch.tensor([[-1.3, 0.0, 0.26, 7.0]])
    for spec in (("lin", 1, 8, False), ("lin", 1, 3, True), ("log", 2, 3, True), ("log", 1, 2, False), ("lin", 0, 32, True)):
        want = log_lin_connect.Quant(x, dtype=spec[0], fsr=spec[1], bit_width=spec[2], with_sign=spec[3])
        assert torch.equal(log_lin_connect.quantize_spec(x, spec), want), spec
    assert ops.levels_exact_in_bf16("lin", 1, 8) and not ops.levels_exact_in_bf16("lin", 1, 12)


def test_level_activation_geometry():
    data = torch.arange(2 * 3 * 3 * 8, dtype=torch.int16).view(18, 8)
    act = packed.LevelActivation(ops.TriplePlanes(data=data, rows=18, K=8, terms=1), (2, 8, 3, 3))
    assert act.can_flatten_hwc() and act.flatten_hwc().shape == (2, 72) and act.flatten_hwc().hwc == (8, 3, 3)
    halo = torch.zeros((2 * 5 * 5, 8), dtype=torch.int16)
    halo.view(2, 5, 5, 8)[:, 1:4, 1:4] = data.view(2, 3, 3, 8)
    padded = packed.LevelActivation(ops.TriplePlanes(data=halo, rows=50, K=8, terms=1), (2, 8, 3, 3), halo=(1, 1))
    assert not padded.can_flatten_hwc() and torch.equal(padded.without_halo().planes.data, data)
    # a level IS its bf16 value: float() widens the patterns
    vals = torch.tensor([[0.0, 0.5, -2.0, 1.75, 0.0, 0.0, 0.0, 0.0]])
    bits = (vals.view(torch.int32) >> 16).to(torch.int16)
    f = packed.LevelActivation(ops.TriplePlanes(data=bits, rows=1, K=4, terms=1), (1, 4)).float()
    assert torch.equal(f, vals[:, :4])
    try:
        packed.LevelActivation(ops.TriplePlanes(data=data, rows=18, K=8, terms=1), (2, 8, 3, 4))
    except ValueError:
        pass
    else:
        raise AssertionError("a plane that does not hold the shape must be refused")


def test_no_cyclic_collection_inside_a_graph_capture():
    """utils.graphs captures with the cyclic collector off (a dead, implicitly replayed model owns hipGraphs and is a reference
    cycle: it must not be destroyed inside another capture), collects before, and restores the collector's state after."""
    import gc
    from pytorch_quantize_impls_amd.utils import graphs

    class Cycle:
        def __init__(self):
            self.me = self

    import weakref
    assert gc.isenabled()
    c = Cycle()
    dead = weakref.ref(c)
    del c
    with graphs._no_collection_inside():
        assert dead() is None and not gc.isenabled()
        inner = Cycle()
        alive = weakref.ref(inner)
        del inner
        for _ in range(3000):                                     # enough container allocations for an automatic collection
            [[]]
        assert alive() is not None
    assert gc.isenabled()
    gc.disable()
    try:
        with graphs._no_collection_inside():
            pass
        assert not gc.isenabled()
    finally:
        gc.enable()
