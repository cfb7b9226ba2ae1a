"""Which weight-gradient routes every conv family tries, in which order and with which arguments (no device).

The five ``ops.conv2d_grad_weight_*`` routes, ``_fused.real_conv_grad_weight_taps`` and ``ops.code_digits`` are replaced by
recorders; the ``*_applicable`` predicates are the real ones.  Every family drives ``_fused.conv_grad_weight_routes`` the way
its backward does, on CPU tensors of the shapes below.

How the expected table was made: the rows of B (un-masked +-1), C (levels), D (codes) and E (codes beyond int8, two-term split)
were recorded with these same recorders from ``pm1_conv_grad_weight``, ``levels_conv_grad_weight`` and
``dorefa_conv_grad_weight`` of the commit BEFORE the routes were folded into one ladder (those walked the routes themselves and
were callable on the CPU); arguments a caller left out were recorded as the route's default.  The rows of A (masked +-1 /
real-valued first layer: ``QuantConv2dFn.backward``), of the real-valued branch of ``conv_grad_weight`` and of its
levels-then-real order were written by hand from that commit's source, whose entry points asked for a device tensor.  The table is
not derived from the ladder it checks.
"""
import pytest
import torch

from pytorch_quantize_impls_amd import ops
from pytorch_quantize_impls_amd.functions import _fused

# (N, Cin, Cout, H, k, stride, padding)
PM3, PM5, GEMM1, GEMM7 = (3, 32, 32, 8, 3, 1, 1), (3, 32, 32, 8, 5, 1, 2), (2, 128, 128, 6, 1, 1, 0), (2, 128, 128, 8, 7, 1, 3)
STRIDED3, STRIDED1, SWAPPED = (3, 8, 32, 8, 3, 2, 1), (3, 16, 24, 8, 1, 2, 0), (4, 32, 64, 8, 7, 1, 3)
ANY16, IMG3, IMG11, PM3_S2 = (3, 16, 16, 8, 3, 1, 1), (2, 3, 32, 8, 3, 1, 1), (2, 3, 32, 35, 11, 4, 2), (3, 32, 32, 8, 3, 2, 1)
SHAPES = (PM3, PM5, GEMM1, GEMM7, STRIDED3, STRIDED1, SWAPPED, ANY16, IMG3, IMG11)

ROUTES = {"pm": "conv2d_grad_weight_pm", "gemm": "conv2d_grad_weight_gemm", "strided": "conv2d_grad_weight_strided",
          "swapped": "conv2d_grad_weight_pm1", "s2d": "conv2d_grad_weight_s2d"}


def operands(shape):
    N, Cin, Cout, H, k, s, p = shape
    Ho = (H + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed(7)
    x = torch.where(torch.rand((N, Cin, H, H), generator=g) < 0.5, -1.0, 1.0)
    go = torch.randn((N, Cout, Ho, Ho), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g)
    return x, go, w, s, p


class Recorder:
    """Stands in for the routes: notes (name, arguments) of every attempt; a route named in ``answers`` returns a sentinel
    gradient, every other one None."""

    def __init__(self, monkeypatch, answers=()):
        self.calls, self.answers, self.sentinel = [], set(answers), None
        for name, attr in ROUTES.items():
            monkeypatch.setattr(ops, attr, self._route(name))
        monkeypatch.setattr(_fused, "real_conv_grad_weight_taps", self._route("taps"))
        monkeypatch.setattr(ops, "code_digits", self._digits)

    def _route(self, name):
        def route(x, go, *args, terms=None, x_levels=1.0, weight=None, bias_grad=None, layout_like=None, any_channels=False,
                  ste_threshold=ops.STE_THRESHOLD):
            assert ste_threshold == ops.STE_THRESHOLD
            self.calls.append((name, dict(terms=terms, x_levels=x_levels, weight=weight is not None, bias=bias_grad is not None,
                                          layout=layout_like is not None, any_channels=any_channels)))
            if name in self.answers:
                self.sentinel = torch.full((go.shape[1], x.shape[1]) + tuple(int(v) for v in args[0][-2:]), 3.0)
                return self.sentinel
            return None
        return route

    def _digits(self, x, levels, flag):
        self.calls.append(("digits", {}))
        return x, x, None

    @property
    def attempts(self):
        return " ".join(name for name, _ in self.calls)

    @property
    def first(self):
        kw = next(kw for name, kw in self.calls if name != "digits")          # (the digit split is no route)
        return (kw["terms"], kw["x_levels"], kw["weight"], kw["bias"], kw["layout"], kw["any_channels"])


def drive(family, shape):
    """The weight-gradient call of ``family``'s backward, behind an open gate."""
    x, go, w, s, p = operands(shape)
    if family == "A":          # QuantConv2dFn: masked; +-1 activation
        return _fused.conv_grad_weight_routes(x, go, w.shape, s, p, 1, _fused.X_PM1, weight=w, bias_grad=[])
    if family == "A_real":     # QuantConv2dFn over a real-valued image
        return _fused.conv_grad_weight_routes(x, go, w.shape, s, p, 1, _fused.X_REAL, weight=w, bias_grad=[])
    if family == "B":          # the functional forms / XNOR-Net: un-masked +-1
        return _fused.conv_grad_weight(x, w.shape, go, s, p, 1, 1, True, [])
    if family == "C":          # Lin / Log levels (LogLinConv2dFn)
        return _fused.conv_grad_weight(x, w.shape, go, s, p, 1, 1, False, real_any_channels=True, x_exact_bf16=True)
    if family == "D":          # DoReFa codes within int8
        return _fused.dorefa_conv_grad_weight(x, go, w.shape, s, p, 1, 15.0, True, None, layout_like=w)
    if family == "E":          # DoReFa codes beyond int8 under the two-term split
        with ops.float_split("f16x2"):
            return _fused.dorefa_conv_grad_weight(x, go, w.shape, s, p, 1, 15.0, False, torch.zeros(1, dtype=torch.int32),
                                                  layout_like=w)
    if family == "real":       # conv_grad_weight over a real-valued image (the functional forms)
        return _fused.conv_grad_weight(x, w.shape, go, s, p, 1, 1, False, [])
    if family == "real_any":   # ... of any width (RealConv2dFn, XNORConv2d with quant_input)
        return _fused.conv_grad_weight(x, w.shape, go, s, p, 1, 1, False, [], real_any_channels=True)
    raise KeyError(family)


@pytest.fixture()
def open_gate(monkeypatch):
    monkeypatch.setattr(_fused, "own_conv_backward", lambda go, groups, padding, macs=None: True)


# first-attempt arguments: (terms, x_levels, weight given, bias_grad given, layout_like given, any_channels)
_A_PM, _A_GEMM, _PLAIN = (None, 1.0, True, True, False, False), (None, 1.0, True, False, False, False), (None, 1.0, False, False, False, False)
_B_PM, _C_PM = (None, 1.0, False, True, False, False), (3, 1.0, False, False, False, False)
_D_PM, _D_GEMM, _E_PM = (None, 15.0, False, False, True, False), (None, 15.0, False, False, False, False), (2, 15.0, False, False, True, False)
_S2D, _S2D_ANY, _A_S2D = (None, 1.0, False, True, False, False), (None, 1.0, False, True, False, True), (None, 1.0, True, True, False, False)

_ANY_NOBIAS, _E_DIGIT_GEMM, _E_DIGIT_1X1 = (None, 1.0, False, False, False, True), _PLAIN, (None, 1.0, False, False, True, False)

#: family -> shape -> (attempts when every route returns None, arguments of the first attempt)
EXPECTED = {
    "A": {PM3: ("pm swapped", _A_PM), PM5: ("pm swapped", _A_PM), GEMM1: ("gemm swapped", _A_GEMM), GEMM7: ("gemm swapped", _A_GEMM),
          STRIDED3: ("strided swapped", _PLAIN), STRIDED1: ("strided swapped", _PLAIN), SWAPPED: ("swapped", _PLAIN),
          ANY16: ("swapped", _PLAIN), IMG3: ("swapped", _PLAIN), IMG11: ("swapped", _PLAIN)},
    "A_real": {PM3: ("", None), PM5: ("", None), GEMM1: ("", None), GEMM7: ("", None), STRIDED3: ("", None), STRIDED1: ("", None),
               SWAPPED: ("", None), ANY16: ("", None), IMG3: ("s2d", _A_S2D), IMG11: ("s2d", _A_S2D)},
    "B": {PM3: ("pm swapped", _B_PM), PM5: ("pm swapped", _B_PM), GEMM1: ("gemm swapped", _PLAIN), GEMM7: ("gemm swapped", _PLAIN),
          STRIDED3: ("strided swapped", _PLAIN), STRIDED1: ("strided swapped", _PLAIN), SWAPPED: ("swapped", _PLAIN),
          ANY16: ("swapped", _PLAIN), IMG3: ("swapped", _PLAIN), IMG11: ("swapped", _PLAIN)},
    # the levels rungs (recorded: pm with three terms, gemm, strided 1 x 1 only), then the real-valued rows of "real_any" without
    # a bias list (LogLinConv2dFn passes none)
    "C": {PM3: ("pm s2d taps", _C_PM), PM5: ("pm s2d taps", _C_PM), GEMM1: ("gemm taps", _PLAIN), GEMM7: ("gemm taps", _PLAIN),
          STRIDED3: ("taps", _PLAIN), STRIDED1: ("strided taps", _PLAIN), SWAPPED: ("taps", _PLAIN), ANY16: ("s2d taps", _ANY_NOBIAS),
          IMG3: ("s2d taps", _PLAIN), IMG11: ("s2d taps", _PLAIN), PM3_S2: ("taps", _PLAIN)},
    "D": {PM3: ("pm", _D_PM), PM5: ("pm", _D_PM), GEMM1: ("gemm", _D_GEMM), GEMM7: ("gemm", _D_GEMM), STRIDED3: ("strided", _D_PM),
          STRIDED1: ("strided", _D_PM), SWAPPED: ("", None), ANY16: ("", None), IMG3: ("", None), IMG11: ("", None)},
    # one pass on the rungs that run the pixel-major kernel (its fp16 activation plane), then the two digit passes of D
    "E": {PM3: ("pm digits pm", _E_PM), PM5: ("pm digits pm", _E_PM), GEMM1: ("digits gemm", _E_DIGIT_GEMM),
          GEMM7: ("digits gemm", _E_DIGIT_GEMM), STRIDED3: ("strided digits strided", _D_PM), STRIDED1: ("digits strided", _E_DIGIT_1X1),
          SWAPPED: ("digits", None), ANY16: ("digits", None), IMG3: ("digits", None), IMG11: ("digits", None)},
    "real": {PM3: ("", None), PM5: ("", None), GEMM1: ("", None), GEMM7: ("", None), STRIDED3: ("", None), STRIDED1: ("", None),
             SWAPPED: ("", None), ANY16: ("", None), IMG3: ("s2d", _S2D), IMG11: ("s2d", _S2D)},
    "real_any": {PM3: ("s2d taps", _S2D_ANY), PM5: ("s2d taps", _S2D_ANY), GEMM1: ("taps", _PLAIN), GEMM7: ("taps", _PLAIN),
                 STRIDED3: ("taps", _PLAIN), STRIDED1: ("taps", _PLAIN), SWAPPED: ("taps", _PLAIN), ANY16: ("s2d taps", _S2D_ANY),
                 IMG3: ("s2d taps", _S2D), IMG11: ("s2d taps", _S2D)},
}
CASES = [(f, s) for f, rows in EXPECTED.items() for s in rows]


@pytest.mark.parametrize("family,shape", CASES, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in CASES])
def test_attempts_and_first_arguments(monkeypatch, open_gate, family, shape):
    rec = Recorder(monkeypatch)
    drive(family, shape)             # no route answers: the families with a library exit end there (host tensors: not counted)
    attempts, first = EXPECTED[family][shape]
    assert rec.attempts == attempts
    if first is not None:
        assert rec.first == first


def test_the_ladder_itself_reports_none(monkeypatch):
    """No route answers: None (the library is the caller's), nothing counted; the ladder reads neither the device nor the gate."""
    for kind in (_fused.X_PM1, _fused.X_CODES, _fused.X_LEVELS, _fused.X_REAL):
        for shape in SHAPES:
            x, go, w, s, p = operands(shape)
            Recorder(monkeypatch)
            with _fused.scope(BWD_CONV_MFMA=False):
                assert _fused.conv_grad_weight_routes(x, go, w.shape, s, p, 1, kind, terms=3 if kind == _fused.X_LEVELS else None) is None


def test_levels_leave_out_the_strided_kxk_form(monkeypatch, open_gate):
    """3 x 3 / stride 2 with 32 channels is the strided route's shape, but that form picks its split by FLOAT_SPLIT: levels take the
    per-tap real route."""
    assert ops.wgrad_strided_applicable((3, 32, 8, 8), (3, 32, 4, 4), (3, 3), 2, 1, 1)
    rec = Recorder(monkeypatch, answers=("taps",))
    assert drive("C", PM3_S2) is rec.sentinel
    assert rec.attempts == "taps"


def test_codes_never_take_the_swapped_conv(monkeypatch):
    for family in ("D", "E"):
        for shape in SHAPES + (PM3_S2,):
            rec = Recorder(monkeypatch)
            assert drive(family, shape) is None
            assert "swapped" not in rec.attempts


def test_pm_without_a_plan_goes_on_to_the_swapped_conv(monkeypatch):
    rec = Recorder(monkeypatch)
    x, go, w, s, p = operands(PM3)
    assert _fused.conv_grad_weight_routes(x, go, w.shape, s, p, 1, _fused.X_PM1) is None
    assert rec.attempts == "pm swapped"


@pytest.mark.parametrize("masked", (False, True))
def test_first_answer_wins_and_comes_back_masked(monkeypatch, masked):
    """gemm -> swapped fall-through (7 x 7 with 128 channels holds both gates); a route after the first answer is not tried.  With
    ``weight`` the epilogue rungs (pm, gemm, s2d) return their own result, every other rung's goes through the STE mask."""
    x, go, w, s, p = operands(GEMM7)
    weight = w if masked else None
    for answers, attempts, name in ((("gemm", "swapped"), "gemm", "gemm"), (("swapped",), "gemm swapped", "swapped")):
        rec, taken = Recorder(monkeypatch, answers), []
        got = _fused.conv_grad_weight_routes(x, go, w.shape, s, p, 1, _fused.X_PM1, weight=weight, taken=taken)
        assert rec.attempts == attempts and taken == [name]
        if masked and name == "swapped":
            assert torch.equal(got, torch.where(w.abs() > ops.STE_THRESHOLD, 0.0, 3.0))
        else:
            assert got is rec.sentinel
