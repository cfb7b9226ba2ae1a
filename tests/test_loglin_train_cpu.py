"""Lin / Log training routes without a GPU: the bf16-exactness predicate that picks them (ops.levels_exact_in_bf16), and CPU
tensors still evaluating the reference expressions F.linear / F.conv2d(x, Q(W), b), converted models included."""
import copy

import pytest
import torch
import torch.nn.functional as F

from pytorch_quantize_impls_amd import ops
from pytorch_quantize_impls_amd.functions import _fused, log_lin_connect
from pytorch_quantize_impls_amd.layers import LinearQuant, QuantConv2d
from pytorch_quantize_impls_amd.utils import log_lin_net_convert


@pytest.mark.parametrize("dtype,fsr,bits,exact", [
    ("lin", 7, 1, True), ("lin", 2, 8, True), ("lin", 1, 9, False), ("lin", 2, 12, False), ("lin", 1, 31, False),
    ("lin", 7, 32, False), ("lin", -60, 8, True), ("lin", 60, 3, True), ("lin", -61, 3, False), ("lin", 61, 3, False),
    ("log", 7, 3, True), ("log", 1, 16, False), ("log", 0, 6, True),
    ("log", 2, 7, True),            # lowest level 2^(2 - 128) = 2^-126: the smallest normal bf16
    ("log", 1, 7, False),           # 2^-127: a denormal
    ("log", -60, 6, True),          # 2^-124
    ("log", -60, 7, False), ("log", 60, 17, False), ("log", 0, 0, False),
    ("lin", 2.5, 3, False), ("bin", 1, 3, False),
])
def test_exactness_predicate(dtype, fsr, bits, exact):
    assert ops.levels_exact_in_bf16(dtype, fsr, bits) is exact


def test_predicate_matches_level_sets():
    """Brute force over the level sets the predicate accepts: every level round-trips through bf16 and is normal."""
    for dtype, fsr, bits in [("lin", f, b) for f in (-3, 0, 2, 7) for b in (1, 4, 8)] + [("log", f, b) for f in (-2, 1, 7)
                                                                                         for b in (1, 3, 6)]:
        assert ops.levels_exact_in_bf16(dtype, fsr, bits)
        if dtype == "lin":
            levels = torch.arange(0, 2 ** bits + 1, dtype=torch.float64) * 2.0 ** (fsr - bits)
        else:
            levels = torch.tensor([2.0 ** e for e in range(fsr - 2 ** bits, fsr + 1)], dtype=torch.float64)
        lv = levels.float()
        assert torch.equal(lv.double(), levels)
        assert torch.equal(lv.bfloat16().float(), lv)
        nz = lv[lv != 0]
        assert bool((nz >= 2.0 ** -126).all())


def _ref_linear(layer, x):
    q = log_lin_connect.Quant(layer.weight, dtype=layer.qdtype, fsr=layer.fsr, bit_width=layer.bit_width)
    return F.linear(x, q, layer.bias)


@pytest.mark.parametrize("dtype,fsr,bits", [("lin", 1, 8), ("log", 2, 3), ("lin", 2, 12)])
def test_cpu_layers_run_the_torch_expressions(dtype, fsr, bits):
    torch.manual_seed(0)
    lin = LinearQuant(30, 12, True, dtype=dtype, fsr=fsr, bit_width=bits)
    conv = QuantConv2d(4, 6, 3, stride=2, padding=1, fsr=fsr, bit_width=bits, dtype=dtype)
    x2 = torch.randn(5, 30, requires_grad=True)
    x4 = torch.randn(2, 4, 9, 9, requires_grad=True)
    before = dict(_fused.LIBRARY_PATHS)
    for layer, x in ((lin, x2), (conv, x4)):
        y = layer(x)
        twin = copy.deepcopy(layer)
        xt = x.detach().clone().requires_grad_(True)
        q = log_lin_connect.Quant(twin.weight, dtype=dtype, fsr=fsr, bit_width=bits)
        yt = F.linear(xt, q, twin.bias) if layer is lin else F.conv2d(xt, q, twin.bias, 2, 1)
        assert torch.equal(y, yt)
        g = torch.randn_like(y)
        y.backward(g)
        yt.backward(g)
        assert torch.equal(x.grad, xt.grad)
        assert torch.equal(layer.weight.grad, twin.weight.grad) and torch.equal(layer.bias.grad, twin.bias.grad)
    assert dict(_fused.LIBRARY_PATHS) == before              # host tensors are never counted


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.c2 = torch.nn.Conv2d(8, 8, 3, stride=2)
        self.fc = torch.nn.Linear(8 * 3 * 3, 10)

    def forward(self, x):
        x = torch.relu(self.c1(x))
        x = torch.relu(self.c2(x))
        return self.fc(F.adaptive_avg_pool2d(x, 3).flatten(1))


def _functional(net, x):
    def q(m):
        return log_lin_connect.Quant(m.weight, dtype=m.qdtype, fsr=m.fsr, bit_width=m.bit_width)
    x = torch.relu(F.conv2d(x, q(net.c1), net.c1.bias, 1, 1))
    x = torch.relu(F.conv2d(x, q(net.c2), net.c2.bias, 2, 0))
    return F.linear(F.adaptive_avg_pool2d(x, 3).flatten(1), q(net.fc), net.fc.bias)


@pytest.mark.parametrize("dtype,bits", [("lin", 8), ("log", 3)])
def test_converted_model_trains_on_cpu_as_the_reference(dtype, bits):
    torch.manual_seed(1)
    net = log_lin_net_convert(_Net(), fsr=1, bit_width=bits, dtype=dtype)
    assert isinstance(net.c1, QuantConv2d) and isinstance(net.fc, LinearQuant)
    twin = copy.deepcopy(net)
    oa, ob = torch.optim.SGD(net.parameters(), lr=0.1), torch.optim.SGD(twin.parameters(), lr=0.1)
    for step in range(3):
        x, t = torch.randn(4, 3, 12, 12), torch.randint(0, 10, (4,))
        for model, opt, fwd in ((net, oa, lambda m, v: m(v)), (twin, ob, _functional)):
            opt.zero_grad()
            F.cross_entropy(fwd(model, x), t).backward()
            opt.step()
            for m in (model.c1, model.c2, model.fc):
                m.clamp()
        for pa, pb in zip(net.parameters(), twin.parameters()):
            assert torch.equal(pa, pb), step
    lq = LinearQuant.convert(torch.nn.Linear(6, 4), dtype=dtype, fsr=2, bit_width=bits)
    x = torch.randn(3, 6, requires_grad=True)
    assert torch.equal(lq(x), _ref_linear(lq, x))
