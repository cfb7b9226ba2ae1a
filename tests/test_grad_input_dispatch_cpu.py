"""Which grad-input rung every conv family tries, with which arguments, and whether the counted library follows (no device).

``ops.conv2d_grad_input_q``, ``ops.conv2d_grad_input_taps``, ``ops.real_conv2d``, ``ops.zero_dilated_gradient`` and
``_fused.lib_conv2d_input`` are replaced by recorders; the geometry test ``ops.grad_input_route_applicable`` is the real one, and
the recorders of the two ``conv2d_grad_input_*`` rungs answer exactly where it holds (the taps rung also wants Cout % 8 == 0), so a
shape off the route ends on the library as it does on the device.  Every family's backward is called as autograd calls it, on CPU
tensors with a hand-made ``ctx`` and ``own_conv_backward`` patched open.

How the expected table was made.  RECORDED with these same recorders and drivers from the commit BEFORE the route walks were
folded into ``_fused.conv_grad_input_routes`` (its backward bodies walked the rungs themselves and ran on CPU tensors behind the
open gate; ``_fused._conv_grad_input_route`` stood in for the geometry test): the rows of ``bin`` / ``ter`` / ``draw``
(``QuantConv2dFn``), ``w1`` / ``wk`` (the DoReFa nodes), ``f_bin`` / ``f_ter`` / ``f_d1`` / ``f_d4`` / ``f_d32`` (the functional forms of
binary_connect, terner_connect and dorefa_connect over ``_fused.conv_grad_input``), ``loglin`` (``LogLinConv2dFn.backward``) and
``xnor`` (``_XNORConv2d.backward``).  For the last two the ``ctx`` fields a device forward leaves (which operand was packed; the tap
scales) were WRITTEN BY HAND from that commit's forward.  The rows of ``real`` (``RealConv2dFn.backward``, whose own gate asks for a
device gradient) were WRITTEN BY HAND from that commit's source; the test drives the call its backward makes behind that gate.
The table is not derived from the ladder it checks.
"""
import types
import warnings

import pytest
import torch

from pytorch_quantize_impls_amd import ops
from pytorch_quantize_impls_amd.functions import _fused, binary_connect, dorefa_connect, terner_connect, xnor_connect

# (N, Cin, Cout, H, k, stride, padding, dilation)
S1, K5, S2, S2_ROW, S2_1X1 = (2, 16, 32, 7, 3, 1, 1, 1), (2, 16, 32, 7, 5, 1, 2, 1), (2, 16, 32, 7, 3, 2, 1, 1), (2, 16, 32, 8, 3, 2, 1, 1), \
    (2, 16, 32, 8, 1, 2, 0, 1)
DILATED, RECT_STRIDE, WIDE_PAD, COUT12 = (2, 16, 32, 7, 3, 1, 1, 2), (2, 16, 32, 7, 3, (2, 1), 1, 1), (2, 16, 32, 9, 3, 1, 3, 1), \
    (2, 16, 12, 7, 3, 1, 1, 1)
ON_ROUTE, OFF_ROUTE = (S1, K5, S2, S2_ROW, S2_1X1, COUT12), (DILATED, RECT_STRIDE, WIDE_PAD)
SHAPES = ON_ROUTE + OFF_ROUTE


def operands(shape):
    N, Cin, Cout, H, k, s, p, d = shape
    sh, sw = ops._pairs(s)
    Ho, Wo = ((H + 2 * p - d * (k - 1) - 1) // st + 1 for st in (sh, sw))
    g = torch.Generator().manual_seed(11)
    x = torch.where(torch.rand((N, Cin, H, H), generator=g) < 0.5, -1.0, 1.0)
    go = torch.randn((N, Cout, Ho, Wo), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g)
    return x, go, w, (s, p, d, 1)


class Recorder:
    """Stands in for the rungs and the library exit and notes every call.  ``geometry``: the rungs answer (a sentinel gradient)
    where the real geometry test holds; otherwise every rung returns None."""

    def __init__(self, monkeypatch, geometry=True):
        self.calls, self.q_args, self.sentinel, self.geometry = [], None, None, geometry
        self._dilate = ops.zero_dilated_gradient
        monkeypatch.setattr(ops, "conv2d_grad_input_q", self._q)
        monkeypatch.setattr(ops, "conv2d_grad_input_taps", self._taps)
        monkeypatch.setattr(ops, "real_conv2d", self._real)
        monkeypatch.setattr(ops, "zero_dilated_gradient", self._dilated)
        monkeypatch.setattr(_fused, "lib_conv2d_input", self._lib)
        monkeypatch.setattr(_fused, "own_conv_backward", lambda go, groups, padding, macs=None: True)

    def _answer(self, input_shape, weight_shape, stride, padding, dilation, ok=True):
        if self.geometry and ok and ops.grad_input_route_applicable(weight_shape, stride, padding, dilation):
            self.sentinel = torch.full(tuple(input_shape), 3.0)
            return self.sentinel
        return None

    def _q(self, input_shape, weight_q, go, stride, padding, dilation, kind="sign", out_scale=1.0, out_scale_dev=None, terms=None,
           weight_triples=None):
        self.calls.append("q")
        self.q_args = (kind, terms, out_scale != 1.0, out_scale_dev is not None, weight_triples is not None)
        return self._answer(input_shape, weight_q.shape, stride, padding, dilation)

    def _taps(self, input_shape, weight, go, tap_rho_flipped, stride, padding, dilation):
        self.calls.append("taps")
        assert tap_rho_flipped is TAPS.bwd
        return self._answer(input_shape, weight.shape, stride, padding, dilation, ok=weight.shape[0] % 8 == 0)

    def _real(self, x, w, bias, stride, padding, dilation):
        self.calls.append(f"real(pad={padding[0]})")
        assert bias is None and (stride, dilation) == (1, 1)
        if not self.geometry:
            return None
        k = int(w.shape[2])
        H = int(x.shape[2]) + 2 * padding[0] - k + 1
        self.sentinel = torch.full((int(x.shape[0]) * H * H, int(w.shape[0])), 3.0)
        return self.sentinel

    def _dilated(self, *args):
        self.calls.append("dilate")
        return self._dilate(*args)

    def _lib(self, input_shape, weight_q, grad_output, stride, padding, dilation, groups,
             reason="conv grad_input outside the matrix-core route"):
        self.calls.append("lib")
        assert reason == "conv grad_input outside the matrix-core route"
        self.lib_weight = weight_q
        return torch.full(tuple(input_shape), 5.0)

    @property
    def attempts(self):
        return " ".join(self.calls)


TAPS = types.SimpleNamespace(bwd=torch.ones(9))


def ctx_of(saved, **fields):
    return types.SimpleNamespace(saved_tensors=saved, needs_input_grad=(True, False, False), has_bias=False, **fields)


def functional(factory, *args):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return factory(*args)


def drive(family, shape):
    """grad_x of ``family``'s backward for ``shape``."""
    x, go, w, args = operands(shape)
    s, p, d, groups = args
    if family in ("bin", "ter", "draw"):           # QuantConv2dFn: the latent weight with its quantiser, or a saved stochastic draw
        kind = "ternary" if family == "ter" else "binary"
        wq = _fused.quantize_weight_f32(w, kind) if family == "draw" else None
        return _fused.QuantConv2dFn.backward(ctx_of((x, w, wq), kind=kind, conv_args=args, bias_dtype=None, x_is_pm1=True), go)[0]
    if family == "w1":
        return _fused.DorefaW1Conv2dFn.backward(ctx_of((x, w), conv_args=args, E=torch.tensor(0.5), x_levels=None), go)[0]
    if family == "wk":
        wq = torch.round(torch.tanh(w) * 7.5) / 15.0
        return _fused.DorefaWkConv2dFn.backward(ctx_of((x, wq), conv_args=args, bit_width=4, x_levels=None), go)[0]
    if family == "loglin":     # the forward packs the grad_x operand on the route, else the fp32 image for the library
        routed = ops.grad_input_route_applicable(w.shape, s, p, d)
        ctx = ctx_of((x, w), conv_args=args, quant=None, w_shape=tuple(w.shape), x_exact=False, gx=object() if routed else None,
                     wq=None if routed else w)
        return _fused.LogLinConv2dFn.backward(ctx, go)[0]
    if family == "xnor":       # the +-1 forward leaves the tap scales
        cls = functional(xnor_connect.XNORConv2d, [0, 1], False, s, p, d, groups)
        return cls.backward(ctx_of((x, w, torch.ones(1, 1, *w.shape[2:]), None), taps=TAPS, x_is_pm1=True), go)[0]
    if family == "real":       # RealConv2dFn.backward behind its own gate (a non-empty device fp32 gradient)
        return _fused.conv_grad_input(x, w, go, s, p, d, groups, _fused.W_REAL, gate=True)
    if family == "f_bin":
        return functional(binary_connect.BinaryConv2d, s, p, d, groups).backward(ctx_of((x, w, None)), go)[0]
    if family == "f_ter":
        wt = _fused.quantize_weight_f32(w, "ternary")
        return functional(terner_connect.TernaryConv2d, False, s, p, d, groups).backward(ctx_of((x, w, wt, None)), go)[0]
    bits = {"f_d1": 1, "f_d4": 4, "f_d32": 32}[family]
    saved = (x, w, torch.round(torch.tanh(w) * 7.5) / 15.0, w.abs().max(), None)
    return functional(dorefa_connect.QuantConv2d, s, p, d, groups, bits).backward(ctx_of(saved), go)[0]


# arguments of the conv2d_grad_input_q attempt: (kind, terms, out_scale given, out_scale_dev given, weight_triples given)
_SIGN, _BIN, _TER, _RAW = ("sign", None, False, False, False), ("binary", None, False, False, False), \
    ("ternary", None, False, False, False), ("raw", None, False, False, False)
_BIN_E, _RAW_N, _PACKED = ("binary", None, False, True, False), ("raw", None, True, False, False), ("raw", 3, False, False, True)


def _rows(on, off, cout12=None):
    return {**{s: on for s in ON_ROUTE}, **{s: off for s in OFF_ROUTE}, **({COUT12: cout12} if cout12 else {})}


#: family -> shape -> (calls in order, arguments of the conv2d_grad_input_q attempt or None)
EXPECTED = {
    "bin": _rows(("q", _BIN), ("q lib", _BIN)),
    "ter": _rows(("q", _TER), ("q lib", _TER)),
    "draw": _rows(("q", _SIGN), ("q lib", _SIGN)),
    "w1": _rows(("q", _BIN_E), ("q lib", _BIN_E)),
    "wk": _rows(("q", _RAW_N), ("q lib", _RAW_N)),
    "f_bin": _rows(("q", _BIN), ("q lib", _BIN)),
    "f_ter": _rows(("q", _RAW), ("q lib", _RAW)),
    "f_d1": _rows(("q", _BIN_E), ("q lib", _BIN_E)),
    "f_d4": _rows(("q", _RAW_N), ("q lib", _RAW_N)),
    "f_d32": _rows(("lib", None), ("lib", None)),
    # nothing was packed for grad_x off the route: no attempt
    "loglin": _rows(("q", _PACKED), ("lib", None)),
    "xnor": _rows(("taps", None), ("taps lib", None), cout12=("taps lib", None)),
    # the padding of the stride-1 conv is k - 1 - p; stride 2 first zero-dilates the gradient
    "real": {S1: ("real(pad=1)", None), K5: ("real(pad=2)", None), S2: ("dilate real(pad=1)", None), S2_ROW: ("dilate real(pad=1)", None),
             S2_1X1: ("dilate real(pad=0)", None), COUT12: ("real(pad=1)", None), DILATED: ("lib", None), RECT_STRIDE: ("lib", None),
             WIDE_PAD: ("lib", None)},
}
CASES = [(f, s) for f, rows in EXPECTED.items() for s in rows]


def _id(shape):
    return "x".join(str(v).replace(" ", "") for v in shape)


def observe(monkeypatch, family, shape):
    rec = Recorder(monkeypatch)
    got = drive(family, shape)
    assert tuple(got.shape) == operands(shape)[0].shape
    return rec.attempts, rec.q_args


@pytest.mark.parametrize("family,shape", CASES, ids=[f"{f}-{_id(s)}" for f, s in CASES])
def test_rung_arguments_and_library_exit(monkeypatch, family, shape):
    assert observe(monkeypatch, family, shape) == EXPECTED[family][shape]


def test_every_shape_of_every_family_is_in_the_table():
    assert all(set(rows) == set(SHAPES) for rows in EXPECTED.values())


LADDER_CALLS = ((_fused.W_PM1, {}), (_fused.W_LEVELS, {}), (_fused.W_PACKED, dict(operand=object())),
                (_fused.W_TAPS, dict(operand=TAPS.bwd)), (_fused.W_REAL, {}))


def test_the_ladder_itself_reports_none(monkeypatch):
    """No rung answers: None (the library is the caller's) and nothing counted; the ladder reads neither the device nor a gate."""
    before = dict(_fused.LIBRARY_PATHS)
    for w_kind, kw in LADDER_CALLS:
        for shape in SHAPES:
            x, go, w, (s, p, d, _) = operands(shape)
            rec, taken = Recorder(monkeypatch, geometry=False), []
            with _fused.scope(BWD_CONV_MFMA=False):
                assert _fused.conv_grad_input_routes(x, w, go, s, p, d, w_kind, taken=taken, **kw) is None
            assert "lib" not in rec.calls and taken == []
    assert dict(_fused.LIBRARY_PATHS) == before


@pytest.mark.parametrize("w_kind,kw", LADDER_CALLS, ids=[k for k, _ in LADDER_CALLS])
def test_first_answer_wins_and_the_library_image_is_not_built(monkeypatch, w_kind, kw):
    def image():
        raise AssertionError("the library's weight image was built although a rung answered")

    x, go, w, (s, p, d, groups) = operands(S2_ROW)
    rec, taken = Recorder(monkeypatch), []
    got = _fused.conv_grad_input_routes(x, w, go, s, p, d, w_kind, taken=taken, **kw)
    assert got is not None and len(taken) == 1 and len([c for c in rec.calls if c != "dilate"]) == 1
    rec = Recorder(monkeypatch)
    got = _fused.conv_grad_input(x, w, go, s, p, d, groups, w_kind, gate=True, lib_weight=image, **kw)
    assert "lib" not in rec.calls and torch.equal(got, torch.full(x.shape, 3.0))
    # ... and is built, once, when none does
    built = []
    rec = Recorder(monkeypatch, geometry=False)
    got = _fused.conv_grad_input(x, w, go, s, p, d, groups, w_kind, gate=True, lib_weight=lambda: built.append(1) or w, **kw)
    assert rec.calls[-1] == "lib" and built == [1] and rec.lib_weight is w and torch.equal(got, torch.full(x.shape, 5.0))


def test_a_closed_gate_goes_straight_to_the_library(monkeypatch):
    x, go, w, (s, p, d, groups) = operands(S1)
    rec = Recorder(monkeypatch)
    _fused.conv_grad_input(x, w, go, s, p, d, groups, _fused.W_PM1, gate=False)
    assert rec.attempts == "lib"
