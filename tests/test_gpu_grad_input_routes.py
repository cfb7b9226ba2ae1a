"""grad_x of every conv family through ``_fused.conv_grad_input`` / ``conv_grad_input_routes``, bit for bit (tiny shapes).

Every family's backward runs with frozen parameters (only grad_x is computed) on designed data: gradients = small integers times
a power of two, weight images exact in 16 bits, so every correct summation order gives the float64 sum in fp32
(``proves_exact`` / ``proves_exact_taps`` check the actual tensors first).  On the route (square stride, un-dilated, padding
<= k - 1) the case asserts, under both float splits and for channels-last and plain NCHW inputs:
  * x.grad == to_f32_exact(conv_grad_input64(g, image)) [x fl(scale): DoReFa's E / fl(1 / n), as tests/test_gpu_grad_b256.py],
  * the memory format of the gradient the node returns (a channels-last view from the exact-split and tap rungs whatever the
    input's format; Lin / Log and the real rung copy it for an input in NCHW storage) and of x.grad (the input's),
  * the C-ABI entries of the expected rung, and that ``_fused.LIBRARY_PATHS`` did not move.
Off the route (dilation 2, stride (2, 1), padding > k - 1; for XNOR-Net also Cout % 8 != 0) exactly one count under
"conv grad_input outside the matrix-core route" and the value of torch.nn.grad.conv2d_input in float64 on the image the
family hands to the library.  The k-bit DoReFa image c / n is no dyadic number, so no order-independent sum exists off the route:
there the case pins the image instead (weight_q itself, not levels x fl(1 / n)) by equality with the library call on it.
No number in this module is a tolerance."""
import warnings

import pytest
import torch

import _grad_exact as G
import _xnor_exact as XE

pytestmark = pytest.mark.gpu

from pytorch_quantize_impls_amd import _lib, lazy_train, ops  # noqa: E402
from pytorch_quantize_impls_amd.functions import _fused, binary_connect, dorefa_connect, terner_connect  # noqa: E402
from pytorch_quantize_impls_amd.layers import BinConv2d, DorefaConv2d, QuantConv2d, TerConv2d, XNORConv2d  # noqa: E402

# (N, Cin, Cout, H, k, stride, padding, dilation)
S1, K5, S2, S2_ROW, S2_1X1 = (2, 16, 32, 7, 3, 1, 1, 1), (2, 16, 32, 7, 5, 1, 2, 1), (2, 16, 32, 7, 3, 2, 1, 1), (2, 16, 32, 8, 3, 2, 1, 1), \
    (2, 16, 32, 8, 1, 2, 0, 1)
DILATED, RECT_STRIDE, WIDE_PAD, COUT12 = (2, 16, 32, 7, 3, 1, 1, 2), (2, 16, 32, 7, 3, (2, 1), 1, 1), (2, 16, 32, 9, 3, 1, 3, 1), \
    (2, 16, 12, 7, 3, 1, 1, 1)
ON_ROUTE, OFF_ROUTE = (S1, K5, S2, S2_ROW, S2_1X1), (DILATED, RECT_STRIDE, WIDE_PAD)
SPLITS = ("f16x2", "bf16x3")
REASON = "conv grad_input outside the matrix-core route"
AMP = 3
FAMILIES = ("bin", "ter", "draw", "w1", "w4", "loglin", "real", "xnor", "f_bin", "f_ter", "f_d1")
#: rung -> C-ABI entries of its conv launch (count in one backward), entries that must not run
RUNGS = {"q": ({"qt_conv2d_implicit": 1}, ("qt_conv2d_implicit_taps", "qt_bf16x6_pack_f32")),
         "taps": ({"qt_conv2d_implicit_taps": 1}, ("qt_conv2d_implicit", "qt_bf16x6_pack_f32")),
         "real": ({"qt_conv2d_implicit": 1}, ("qt_conv2d_implicit_taps",))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a HIP device"
    return torch.device("cuda:0")


def _frozen(layer, dev):
    layer = layer.to(dev).train()
    for p in layer.parameters():
        p.requires_grad_(False)
    return layer


def _functional(factory, *args):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return factory(*args)


def _ternary(w):
    s = G.safe_sign(w)
    return (s + G.safe_sign(w - 0.5 * s)) / 2


class Case:
    """One family on one shape: ``forward(x)``, the weight image grad_x contracts (``image``), the factor the route applies after
    (``scale``), the rung, whether the result follows the input's storage format, the image the library exit gets."""

    def __init__(self, dev, family, shape, pow2_scale=False):
        N, Cin, Cout, H, k, s, p, d = shape
        self.family, self.shape, self.scale, self.rung, self.follows_input, self.taps_alpha = family, shape, None, "q", False, None
        seed = XE.case_seed(f"{family} {shape}")
        torch.manual_seed(seed)          # (the layers' own initialisation)
        wshape, args = (Cout, Cin, k, k), (s, p, d, 1)
        conv = dict(stride=s, padding=p, dilation=d, bias=False)
        latent = G.latent_weight(wshape, seed, dev)
        if family in ("bin", "ter"):
            layer = _frozen((BinConv2d if family == "bin" else TerConv2d)(Cin, Cout, k, **conv), dev)
            layer.weight.copy_(latent)
            self.forward, self.image = layer, G.safe_sign(latent) if family == "bin" else _ternary(latent)
        elif family == "draw":          # a saved stochastic draw: +-1 / 0 that is NOT the deterministic image of the latent weight
            draw = G.pm1(wshape, seed + 1, dev, zero_frac=0.25, channels_last=False)
            self.forward, self.image = (lambda x: _fused.QuantConv2dFn.apply(x, latent, None, "ternary", draw, None, args)), draw
        elif family in ("w1", "f_d1"):      # sign(W) * E; off the route E = 1/2 exactly (the library multiplies the image by it)
            w = G.pm1(wshape, seed, dev, channels_last=False) * 0.5 if pow2_scale else G.latent_weight(wshape, seed, dev, -1.0, 1.0)
            self.image, self.scale = G.safe_sign(w), ops.abs_mean(w)
            assert not pow2_scale or float(self.scale) == 0.5
            if family == "w1":
                layer = _frozen(DorefaConv2d(Cin, Cout, k, bit_width=1, **conv), dev)
                layer.weight.copy_(w)
                self.forward = layer
            else:
                op = _functional(dorefa_connect.QuantConv2d, s, p, d, 1, 1)
                self.forward = lambda x: op.apply(x, w)
            self.lib_image = self.image * self.scale
        elif family == "w4":            # odd integer levels c, w_q = c / 15
            layer = _frozen(DorefaConv2d(Cin, Cout, k, bit_width=4, **conv), dev)
            layer.weight.copy_(G.latent_weight(wshape, seed, dev, -1.0, 1.0))
            self.lib_image = layer.weight_op.forward(layer.weight).detach()
            self.forward, self.image, self.scale = layer, torch.round(self.lib_image * 15.0), _fused._inv_levels(4)
            assert bool(((self.image.abs() <= 15) & (self.image % 2 == 1)).all())
        elif family in ("loglin", "real"):
            # Lin levels m / 4, |m| <= 16: exact in bf16 -> LogLinConv2dFn; ten bits are not -> RealConv2dFn on Q(W) = W (integers)
            layer = _frozen(QuantConv2d(Cin, Cout, k, fsr=2, bit_width=4 if family == "loglin" else 10, dtype="lin", **conv), dev)
            if family == "real":
                layer.weight.copy_(G.int_uniform(wshape, -4, 4, seed, dev, channels_last=False))
                self.rung = "real"
            assert ops.levels_exact_in_bf16("lin", 2, layer.bit_width) == (family == "loglin")
            self.forward, self.image, self.follows_input = layer, layer.weight_op.forward(layer.weight.detach()).detach(), True
        elif family == "xnor":          # +-2^e per tap: alpha = mean|W| over (0, 1) is that power of two
            exps, zero_taps, _ = XE.tap_design(k * k, Cout, "plain", x_absmax=float(AMP), bias_quanta=0, Cout=Cout)
            w = XE.pow2_tap_weight(wshape, exps, seed, dev, zero_taps)
            self.taps_alpha = XE.designed_alpha(exps, zero_taps, dev)
            layer = _frozen(XNORConv2d(Cin, Cout, k, **{**conv, "bias": True}), dev)      # (its op returns two gradients without a bias)
            layer.weight.copy_(w)
            self.forward, self.rung = layer, "taps"
            self.image = torch.sign(w) * self.taps_alpha.to(torch.float32).reshape(1, 1, k, k)
        elif family == "f_bin":
            op = _functional(binary_connect.BinaryConv2d, s, p, d, 1)
            self.forward, self.image = (lambda x: op.apply(x, latent)), G.safe_sign(latent)
        elif family == "f_ter":         # torch.sign, multiples of 1/2
            op = _functional(terner_connect.TernaryConv2d, False, s, p, d, 1)
            sg = torch.sign(latent)
            self.forward, self.image = (lambda x: op.apply(x, latent)), (sg + torch.sign(latent - 0.5 * sg)) / 2
        else:
            raise KeyError(family)
        if not hasattr(self, "lib_image"):
            self.lib_image = self.image

    def backward(self, dev, channels_last=True):
        """(x, the gradient as the node returned it, g, C-ABI call deltas, library path deltas) of one forward + backward."""
        N, Cin, Cout, H, k, s, p, d = self.shape
        seed = XE.case_seed(f"x {self.family} {self.shape}")
        x = G.pm1((N, Cin, H, H), seed, dev, channels_last=channels_last).requires_grad_()
        seen = []
        x.register_hook(seen.append)
        with lazy_train.eager():
            y = self.forward(x)
            g = G.grad_ints(tuple(y.shape), AMP, seed + 1, dev, exp=-40 if s == 1 else 30)
            calls, lib = dict(_lib.call_counts), dict(_fused.LIBRARY_PATHS)
            y.backward(g)
            if g.is_cuda:
                torch.cuda.synchronize()
        dcalls = {k_: v - calls.get(k_, 0) for k_, v in _lib.call_counts.items() if v != calls.get(k_, 0)}
        dlib = {k_: v - lib.get(k_, 0) for k_, v in _fused.LIBRARY_PATHS.items() if v != lib.get(k_, 0)}
        assert len(seen) == 1
        return x, seen[0], g, dcalls, dlib


def _cl(t):
    return t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()


def _on_route(dev, family, split, shape, channels_last):
    N, Cin, Cout, H, k, s, p, d = shape
    what = f"{family} {shape} {split} {'channels-last' if channels_last else 'NCHW'}"
    with ops.float_split(split):
        case = Case(dev, family, shape)
        x, gx, g, calls, lib = case.backward(dev, channels_last)
    print(what, "calls", calls, "library", lib, "strides", gx.stride())
    assert not lib, f"{what}: dense-library paths taken: {lib}"
    want, absent = RUNGS[case.rung]
    assert {e: calls.get(e, 0) for e in want} == want and not any(calls.get(e) for e in absent), f"{what}: {calls}"
    if case.rung == "real":
        assert calls.get("qt_bf16x6_pack_f32", 0) >= 1, f"{what}: {calls}"
    # exactness of the designed operands, as the rung reads them
    if case.rung == "taps":
        ok, why = XE.proves_exact_taps(case.taps_alpha.to(torch.float32), Cout, grad=g, reverse=True)
    else:
        ok, why = G.proves_exact(g, case.image, lambda a, b: G.conv_grad_input64(a, b, (H, H), s, p),
                                 "bf16x3" if case.rung == "real" or family == "loglin" else split,
                                 split_b="bf16x3" if case.rung == "real" else None)
    assert ok, f"{what}: the designed operands are not exact ({why})"
    ref = G.to_f32_exact(G.conv_grad_input64(g, case.image, (H, H), s, p), what)
    if case.scale is not None:
        ref = G.scaled(ref, case.scale)
    for name, got in (("returned gradient", gx), ("x.grad", x.grad)):
        rep = G.mismatch_report(got, ref, ("n", "c", "y", "x"), what=f"{what} {name}")
        assert not rep, rep
    # memory format: the rungs write NHWC rows; only Lin / Log and the real rung copy them for an input in NCHW storage
    if channels_last or not case.follows_input:
        assert _cl(gx), f"{what}: returned strides {gx.stride()}"
    else:
        assert gx.is_contiguous(), f"{what}: returned strides {gx.stride()}"
    assert x.grad.stride() == x.stride(), f"{what}: x.grad strides {x.grad.stride()} for an input of {x.stride()}"


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("family", FAMILIES)
def test_grad_x_on_the_route_is_exact_counted_and_in_the_callers_format(dev, family, split):
    for shape in ON_ROUTE:
        _on_route(dev, family, split, shape, True)
    for shape in (S1, S2_ROW):
        _on_route(dev, family, split, shape, False)


@pytest.mark.parametrize("family", FAMILIES)
def test_grad_x_off_the_route_is_one_counted_library_call(dev, family):
    for shape in OFF_ROUTE + ((COUT12,) if family == "xnor" else ()):
        N, Cin, Cout, H, k, s, p, d = shape
        what = f"{family} {shape} off the route"
        case = Case(dev, family, shape, pow2_scale=True)
        x, gx, g, calls, lib = case.backward(dev)
        print(what, "calls", calls, "library", lib)
        assert lib == {REASON: 1}, f"{what}: {lib}"
        assert not any(calls.get(e) for e in ("qt_conv2d_implicit", "qt_conv2d_implicit_taps")), f"{what}: {calls}"
        if family == "w4":
            ref = torch.nn.grad.conv2d_input(x.shape, case.lib_image, g, stride=s, padding=p, dilation=d)
        else:
            ref64 = torch.nn.grad.conv2d_input(x.shape, case.lib_image.double(), g.double(), stride=s, padding=p, dilation=d)
            ref = G.to_f32_exact(ref64, what)
        rep = G.mismatch_report(x.grad, ref, ("n", "c", "y", "x"), what=what)
        assert not rep, rep
