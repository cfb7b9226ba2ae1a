"""Forward dispatch shared by the quantised Linear / Conv2d layers and the fused Function forms.

Reference call sites this replaces (all ``torch.nn.functional.linear / conv2d`` on a quantised
weight): layers/binary_layers.py:44,46,105,106; layers/terner_layers.py:49,51,91,92;
functions/binary_connect.py:93-98,128-131; functions/terner_connect.py:92-94.

Device tensors:
  * activation known to be +-1 (bit planes attached by the quantiser, or verified on device)
        -> bit-pack the weight, XNOR-popcount / ternary GEMM in libqt_hip.so;
  * arbitrary fp32 activation (first layer of every model)
        -> weight quantised by the HIP elementwise kernel, contraction by the dense fp32 GEMM
           library (the values are exact +-1/0, so this is the reference computation itself).
CPU tensors: the same expression in torch (host logic; never used for a device tensor).
"""
from __future__ import annotations

import contextlib
import threading
import weakref
from collections import Counter
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn.functional as F

from .. import ops, packed
from .common import QtFunction

#: When True (default) an un-tagged device activation is checked on the device for being exactly
#: +-1 before the packed path is taken (costs one read of the activation and one host sync).
#: A layer can override per instance with its ``binary_input`` attribute (True / False / None).
DETECT_BINARY_INPUT = True


#: Device tensors that went through the DENSE LIBRARY (hipBLASLt / MIOpen) instead of libqt_hip.so, by reason.  The
#: HIP path is built for fp32; other dtypes, grouped / non-zero-padding-mode convs and eval-mode weights that are not
#: a quantised image take the reference expression in torch — visibly: tests assert this counter stays empty on the
#: fp32 paths.
LIBRARY_PATHS: Counter = Counter()


# ---- route switches: module attributes = process-wide DEFAULTS; ``with _fused.scope(GEMM_IMPL="valu"):`` = per-thread overrides ----
# (same mechanism as ops.scope; the autograd Functions re-open the forward's scope around their backward: functions.common.QtFunction)
_SCOPED = ("GEMM_IMPL", "DETECT_BINARY_INPUT", "FLOAT_PATH", "PAD_PLANES", "XNOR_LINEAR_DIGITS", "BWD_CONV_MFMA", "LINEAR_GRAD_X_ONE_PACK",
           "BWD_MFMA_MIN_MACS", "LOGLIN_ONE_TERM")
_scope_tls = threading.local()


def _cfg(name: str):
    ov = getattr(_scope_tls, "ov", None)
    if ov is not None and name in ov:
        return ov[name]
    return globals()[name]


def scope_overrides():
    return getattr(_scope_tls, "ov", None)


@contextlib.contextmanager
def scope(_overrides=None, **kw):
    """Thread-local overrides of this module's route switches (names: ``_SCOPED``); nests; ``scope(None)`` is a no-op."""
    if _overrides:
        kw = {**_overrides, **kw}
    bad = [k for k in kw if k not in _SCOPED]
    if bad:
        raise KeyError(f"not a scoped switch of functions._fused: {bad} (known: {_SCOPED})")
    prev = getattr(_scope_tls, "ov", None)
    if kw:
        _scope_tls.ov = {**(prev or {}), **kw}
    try:
        yield
    finally:
        _scope_tls.ov = prev


def note_library_path(input, reason: str) -> None:
    if getattr(input, "is_cuda", False):
        LIBRARY_PATHS[reason] += 1


def autograd_records(input, weight, bias=None) -> bool:
    """Autograd records this call: grad mode is on and the input or the weight requires grad.  ``bias`` is consulted only
    when it is passed (the loss-aware layers, which regularise it)."""
    return torch.is_grad_enabled() and (input.requires_grad or weight.requires_grad
                                        or (bias is not None and bias.requires_grad))


def nchw_result(y2: torch.Tensor, input: torch.Tensor, N: int, H: int, W: int, C: int) -> torch.Tensor:
    """The NHWC result rows ``y2`` as an (N, C, H, W) view; copied to NCHW storage when ``input`` is in it (the caller works
    in NCHW storage)."""
    y = y2.view(N, H, W, C).permute(0, 3, 1, 2)
    if input.is_contiguous() and not input.is_contiguous(memory_format=torch.channels_last):
        y = y.contiguous()
    return y


def _safe_sign_t(w: torch.Tensor) -> torch.Tensor:
    one = torch.ones((), dtype=w.dtype, device=w.device)
    return torch.where(w < 0, -one, one)


def quantize_weight_f32(weight: torch.Tensor, kind: str) -> torch.Tensor:
    """fp32 image of the deterministic weight quantiser of a layer family."""
    hip = weight.is_cuda and weight.dtype == torch.float32      # the kernels are fp32; other dtypes: torch expression
    if kind == "binary":  # safeSign, functions/common.py:4-7
        return ops.binarize(weight) if hip else _safe_sign_t(weight)
    if kind == "ternary":  # functions/terner_connect.py:26-27
        if hip:
            return ops.ternarize(weight)
        s = _safe_sign_t(weight)
        return (s + _safe_sign_t(weight - 0.5 * s)) / 2
    raise ValueError(f"unknown quantiser kind {kind!r}")


#: How a REAL-valued device activation meets a quantised weight: "bf16x3" = exact bf16 triple split +
#: bf16 MFMA GEMM in libqt_hip.so (fp32-GEMM accuracy); "library" = dense fp32 GEMM / conv library on
#: the HIP-quantised weight image (the reference computation itself).
FLOAT_PATH = "bf16x3"

#: Re-express strided few-channel convs (first layers) as stride-1 convs on the space-to-depth image.
USE_S2D = True

#: 'auto' | 'valu' | 'mfma' — packed-GEMM formulation used by the layers (both are bit-exact;
#: 'auto' picks by shape, see ops.select_gemm_impl).
GEMM_IMPL = "auto"
#: packed-activation convs: expand the bits into a physically zero-padded pixel plane (un-padded conv kernel)
PAD_PLANES = True


def pack_weight(weight_2d: torch.Tensor, kind: str, impl: str = "valu"):
    """Packed image (bit planes for 'valu', nibble plane for 'mfma') of the deterministic
    quantiser applied to a [N, K] device weight.  Both quantisers are idempotent, so this is also
    right for an already-quantised (eval / stochastic) weight image."""
    if kind not in ("binary", "ternary"):
        raise ValueError(f"unknown quantiser kind {kind!r}")
    return ops.pack_weights(weight_2d, kind, impl)


# ---- content-dependent routing ----------------------------------------------------------------------------------------
# Two decisions depend on the VALUES of an activation: "is this un-tagged tensor exactly +-1?" (packed route vs the
# exact bf16-triple route) and "do these DoReFa codes fit int8?" (int8 route vs fp32 route; the reference does not
# clamp).  Asking the device costs a host sync per layer per forward (13 % of the module-by-module C4 forward).
#   * A NEGATIVE answer is remembered per (consuming weight, activation shape) in every mode: the general route is
#     correct for any input, so nothing needs to be asked again (e.g. the real-valued first conv of every model).
#   * A POSITIVE answer is re-verified on every call by default (DETECT_MODE = "verify": reference-exact whatever the
#     caller feeds next, one sync per un-tagged input).  DETECT_MODE = "remember" (serving / benchmarking) trusts it and
#     folds THIS call's device flag into the bias instead: if the assumption ever stops holding, the output is NaN —
#     never a plausible wrong number — and reset_detection() re-asks.  That is the contract of the fused code-plane
#     chain (CodeActivation.float()) applied to the module-by-module graph; steady-state forwards then enqueue without
#     any host synchronisation.
# Activations that carry a tag from their quantiser (BinaryConnect, nnDorefaQuant: packed.py) never get here for the
# +-1 question.
DETECT_MODE = "verify"
_plane_capture_tls = threading.local()


@contextlib.contextmanager
def plane_capture_scope(words):
    """Inside: a training forward that runs under stream capture may consume these weight-plane buffers (``words`` tensors).  Set by
    the capture that also captures the update rewriting them (utils/optim.py: ``capturing``); thread-local, restored on exit."""
    prev = getattr(_plane_capture_tls, "ids", None)
    _plane_capture_tls.ids = frozenset(id(w) for w in words)
    try:
        yield
    finally:
        _plane_capture_tls.ids = prev


def plane_capture_allows(words) -> bool:
    ids = getattr(_plane_capture_tls, "ids", None)
    return ids is not None and id(words) in ids


_detect_tls = threading.local()


def detect_mode() -> str:
    """The detection mode in force in THIS thread: the innermost ``detect_scope(...)``, else the module default DETECT_MODE."""
    return getattr(_detect_tls, "mode", None) or DETECT_MODE


def detect_mode_override() -> Optional[str]:
    return getattr(_detect_tls, "mode", None)


@contextlib.contextmanager
def detect_scope(mode: Optional[str]):
    """``with detect_scope("remember"):`` — thread-local like ops.float_split: a capturing thread (utils.GraphedTrainStep) does not
    change what a serving thread beside it asks the device; autograd Functions re-open the forward's scope around their backward
    (functions.common.QtFunction), which runs on the engine's thread.  None = leave as is."""
    if mode is not None and mode not in ("verify", "remember"):
        raise ValueError(f"DETECT_MODE must be 'verify' or 'remember', got {mode!r}")
    prev = getattr(_detect_tls, "mode", None)
    if mode is not None:
        _detect_tls.mode = mode
    try:
        yield
    finally:
        _detect_tls.mode = prev


# ---- the flags of trusted verdicts, collected -------------------------------------------------------------------------------
# In "remember" mode a trusted positive verdict arms an int32 device flag (ops.check_pm1, ops.pack_bf16_check, codes.overflow) that
# poisons the layer's result when the verdict was wrong.  A caller that wants to KNOW (utils.GraphedTrainStep(recover=True): it
# ORs them into the guard of its captured update) opens a sink; the three functions that hand such a flag out — detect_pm1,
# detect_bf16_exact, codes_route: every poisoning site gets its flag from one of them (DESIGN.md lists the sites) — register it.
_sink_tls = threading.local()


class FlagSink:
    """What ``flag_sink()`` yields: the registered flags in order of registration, each once (by identity).  It holds the tensors, so
    a flag allocated inside a stream capture stays valid for a later launch of the same capture that reads it."""

    def __init__(self):
        self.flags, self._ids = [], set()

    def add(self, flag) -> None:
        if id(flag) not in self._ids:          # (the list keeps the tensor alive, so its id is not reused while it is in the set)
            self._ids.add(id(flag))
            self.flags.append(flag)

    def __len__(self):
        return len(self.flags)

    def __iter__(self):
        return iter(self.flags)


@contextlib.contextmanager
def flag_sink(sink: Optional[FlagSink] = None):
    """``with flag_sink() as flags:`` — collects the device flag of every REMEMBERED positive verdict handed out inside, in this
    thread and in the backward of the autograd Functions whose forward ran inside (functions.common.QtFunction carries the sink to
    the engine's thread like the detect scope).  Sinks nest: a flag goes to the innermost one only.  ``sink``: re-open an existing
    one (what QtFunction does).  No sink open: registering is a no-op."""
    sink = FlagSink() if sink is None else sink
    prev = getattr(_sink_tls, "sink", None)
    _sink_tls.sink = sink
    try:
        yield sink
    finally:
        _sink_tls.sink = prev


def current_flag_sink() -> Optional[FlagSink]:
    return getattr(_sink_tls, "sink", None)


def register_flag(flag):
    """Hand a trusted verdict's device flag to the innermost open sink (if any); returns the flag."""
    sink = getattr(_sink_tls, "sink", None)
    if sink is not None and isinstance(flag, torch.Tensor):
        sink.add(flag)
    return flag


_VERDICTS = {}     # id(weight tensor) -> (weak reference to it, {(question, shape): bool}); tensors compare element-wise, so
#                    they cannot key a WeakKeyDictionary
_VERDICTS_LOCK = threading.RLock()   # serving threads share the store; the weak-reference callback may fire inside any of them
#: "sync": decisions that needed a host sync; "cached": decisions taken from a remembered verdict (tests assert on it)
DETECT_STATS: Counter = Counter()


def reset_detection(weight: Optional[torch.Tensor] = None) -> None:
    """Forget the remembered verdicts (of one weight, or all)."""
    with _VERDICTS_LOCK:
        if weight is None:
            _VERDICTS.clear()
        else:
            _VERDICTS.pop(id(weight), None)


def _verdict(weight, tag, resolve):
    """(answer, trusted-from-cache)"""
    mode = detect_mode()
    if mode not in ("verify", "remember"):
        raise ValueError(f"DETECT_MODE must be 'verify' or 'remember', got {mode!r}")
    if weight is None:
        DETECT_STATS["sync"] += 1
        return bool(resolve()), False
    key = id(weight)
    with _VERDICTS_LOCK:
        slot = _VERDICTS.get(key)
        if slot is None or slot[0]() is not weight:
            slot = (weakref.ref(weight, _drop_verdicts(key)), {})
            _VERDICTS[key] = slot
        d = slot[1]
        if tag in d and (d[tag] is False or mode == "remember"):
            DETECT_STATS["cached"] += 1
            return d[tag], True
    answer = bool(resolve())                   # (the device check / host sync runs outside the lock)
    with _VERDICTS_LOCK:
        d[tag] = answer
        DETECT_STATS["sync"] += 1
    return answer, False


def _drop_verdicts(key):
    def drop(_ref):
        with _VERDICTS_LOCK:
            slot = _VERDICTS.get(key)
            if slot is not None and slot[0] is _ref:          # a new tensor may have taken the id meanwhile: keep its slot
                _VERDICTS.pop(key, None)
    return drop


def verdict_is_pm1(input: torch.Tensor, weight: Optional[torch.Tensor]) -> bool:
    """Did the detection for this (weight, activation shape) — run by the forward that just finished — say +-1?  Reads the
    verdict store only (no device check): a forward that packed an un-tagged activation either verified it with a sync or
    armed the device flag that poisons its output, so the backward may contract the same +-1 image."""
    if weight is None:
        return False
    with _VERDICTS_LOCK:
        slot = _VERDICTS.get(id(weight))
        return bool(slot is not None and slot[0]() is weight and slot[1].get(("pm1", tuple(input.shape[1:]))) is True)


_LAST = threading.local()      # .pm1 = (data_ptr, shape, answer) of the detection that ran last in this thread


def last_detection_said_pm1(input: torch.Tensor) -> bool:
    """Did a detection run for exactly THIS activation since ``clear_last_detection()`` and answer +-1?  (The verdict store
    is keyed by weight and shape: a forward that skipped the detection — DETECT_BINARY_INPUT switched off, a non-fp32
    early return — must not inherit an older call's positive answer)"""
    rec = getattr(_LAST, "pm1", None)
    return rec is not None and rec == (input.data_ptr(), tuple(input.shape), True)


def clear_last_detection() -> None:
    _LAST.pm1 = None


def detect_pm1(input: torch.Tensor, weight: Optional[torch.Tensor]):
    """(treat as +-1?, device flag to fold into the bias or None) for an UN-TAGGED device activation."""
    ok, cached = _verdict(weight, ("pm1", tuple(input.shape[1:])), lambda: ops.is_pm1(input))
    _LAST.pm1 = (input.data_ptr(), tuple(input.shape), bool(ok))
    if ok and cached:
        return True, register_flag(ops.check_pm1(input))   # int32[1] on the device, non-zero = some element is not +-1; no sync
    return ok, None


def detect_bf16_exact(input: torch.Tensor, weight: Optional[torch.Tensor]):
    """(one-term bf16 plane or None, device flag to fold into the bias or None) for an UN-TAGGED dense device fp32 activation of a
    Lin / Log layer: is every element exact in bf16 (a pooled or reshaped output of nnQuant)?  Same store and semantics as
    ``detect_pm1`` under the question ("bf16", shape[1:]): a negative verdict is cached in every mode (a real-valued first layer
    asks once); a positive one is re-verified per call ("verify": the check rides in the pack launch, one sync) or trusted
    ("remember": the pack's flag poisons the output if it ever stops holding).  None when the tensor has no plane geometry."""
    got = []

    def resolve():
        got.append(ops.pack_bf16_check(input))
        return got[0] is not None and int(got[0][1].item()) == 0

    ok, cached = _verdict(weight, ("bf16", tuple(input.shape[1:])), resolve)
    if not ok:
        return None, None
    if cached:
        res = ops.pack_bf16_check(input)          # no sync: the flag travels with the result
        return (None, None) if res is None else (res[0], register_flag(res[1]))
    return got[0][0], None


#: Lin / Log layers contract an activation that is exact in bf16 (the tagged output of nnQuant, or a detected one) as ONE bf16
#: term against a one-term weight plane; grad_W multiplies 3 terms of g with it instead of 6.  False: every activation is split
#: into three terms, as for a real number (A/B tools, tests).
LOGLIN_ONE_TERM = True


def loglin_act_planes(input: torch.Tensor, weight: Optional[torch.Tensor], layout):
    """(one-term plane of the activation of a Lin / Log layer or None, device flag or None): the tag of LinQuant / LogQuant
    (packed.attach_levels) when it fits the consumer's layout, else the detection."""
    if not _cfg("LOGLIN_ONE_TERM") or not (input.is_cuda and input.dtype == torch.float32 and input.numel() > 0):
        return None, None
    x = input.detach()
    tagged = packed.lookup_levels(input, layout)
    if tagged is not None:
        K = input.shape[1] if layout == packed.NHWC else input.shape[-1]
        if tagged.terms == 1 and tagged.K == K and tagged.rows * K == input.numel():
            return tagged, None
    if layout == packed.ROWS_LAST:
        if not x.is_contiguous():
            return None, None
        x = x.view(-1, x.shape[-1])
    elif x.dim() != 4:
        return None, None
    return detect_bf16_exact(x, weight)


def loglin_conv_weight_plane(conv, terms: int):
    """The eval-mode weight plane of a QuantConv2d as its own eval path caches it: one term against a level plane (the swapped weight
    already holds the levels, packed as it is), three against the exact split of a real image."""
    if terms == 1:
        return conv._eval_planes(lambda _w2: ops.pack_levels_bf16x3(conv.weight, "lin", 0, 32, True, grad_x=False, fwd_terms=1)[0],
                                 key="conv_bf16x1_levels")
    return conv._eval_planes(lambda _w2: ops.pack_conv_weight_bf16x3(conv.weight.detach(), "raw", terms=3), key="conv_bf16x3_raw")


def loglin_conv_operands(conv, input: torch.Tensor):
    """(pixel plane, weight plane, device flag or None) of an eval-mode QuantConv2d for a device fp32 (N, C, H, W) tensor, built as
    the layer's own eval path builds them: the one-term plane of a tagged / detected quantised activation, else the exact
    three-term split of the (real-valued) tensor."""
    planes, flag = loglin_act_planes(input, conv.weight, packed.NHWC)
    if planes is not None:
        return planes, loglin_conv_weight_plane(conv, 1), flag
    N, C, H, W = (int(v) for v in input.shape)
    nhwc = input.detach().permute(0, 2, 3, 1)
    if not nhwc.is_contiguous():
        nhwc = nhwc.contiguous()
    px = ops.split_bf16x3(nhwc.view(N * H * W, C), ld_bytes=ops.triple_ld_bytes(C, 16, 3), terms=3)
    return px, loglin_conv_weight_plane(conv, 3), None


def loglin_linear_weight_plane(layer, hwc=None):
    """One-term eval-mode weight plane of a LinearQuant (the quantise-and-pack launch, as its own eval path caches it); ``hwc`` =
    (C, H, W): the columns permuted to the (h, w, c) order of a flattened level plane, cached under a key of its own."""
    quant = (layer.qdtype, layer.fsr, layer.bit_width, True)
    if hwc is None:
        return layer._eval_planes(lambda _w2: ops.pack_levels_bf16x3(layer.weight, *quant, grad_x=False, fwd_terms=1)[0],
                                  key="bf16x1_levels")
    from ..layers.fused import permute_fc_weight_hwc
    return layer._eval_planes(lambda w2: ops.pack_levels_bf16x3(permute_fc_weight_hwc(w2, *hwc), *quant, grad_x=False, fwd_terms=1)[0],
                              key=("bf16x1_levels_hwc",) + tuple(hwc))


# ---- half precision (bf16 / fp16) -----------------------------------------------------------------------------------------------
# The sign families take a half activation on the packed routes when it is (treated as) exactly +-1; the result is the exact
# integer sum + bias rounded once to the activation's dtype, which is what the dense library's half GEMM / conv returns for these
# operands.  A real-valued half activation (first layers) keeps the counted torch expression.

def half_route(input, weight: torch.Tensor) -> bool:
    """May this call take the half-precision packed routes?  Device activation in bf16 / fp16 and a weight of the same dtype —
    or an fp32 weight while autocast to that dtype is on (the reference expression would then cast both; the result has the
    autocast dtype).  While autocast to ANOTHER dtype is on (a bf16 model under fp16 autocast) the reference expression casts
    both operands to that dtype: the route declines, and so does every other mix — on to the torch expression, which casts or
    raises as F.linear / F.conv2d do."""
    if not (isinstance(input, torch.Tensor) and input.is_cuda and input.dtype in ops.HALF_DTYPES and input.numel() > 0
            and weight.is_cuda and weight.numel() > 0):
        return False
    if torch.is_autocast_enabled():
        get = getattr(torch, "get_autocast_dtype", None)
        if (get("cuda") if get is not None else torch.get_autocast_gpu_dtype()) != input.dtype:
            return False
        return weight.dtype in (input.dtype, torch.float32)
    return weight.dtype == input.dtype


def _tag_fits(input: torch.Tensor, layout) -> bool:
    """Does the tensor carry a quantiser's planes that the consumer of ``layout`` will accept (activation_planes / _pixel_planes)?"""
    tagged = packed.lookup(input, layout)
    if tagged is None:
        return False
    if layout == packed.NHWC:
        return input.dim() == 4 and tagged.K == input.shape[1] and tagged.rows * tagged.K == input.numel()
    return tagged.K == input.shape[-1] and tagged.rows * tagged.K == input.numel()


def half_gate(input: torch.Tensor, weight: torch.Tensor, binary_input: Optional[bool], layout):
    """Is this half activation (treated as) exactly +-1?  Returns the ``binary_input`` argument for the forward that follows:
    False — not +-1 (the caller takes the torch expression); True — tag of a quantiser, the layer's hint, or a device check that
    was just verified on the host; an int32 device flag — a REMEMBERED "+-1" verdict whose check of this tensor rides along: the
    forward treats the activation as +-1 and folds the flag into the bias (``split_hint``), so the layer detects once per call."""
    if binary_input or _tag_fits(input, layout):
        return True
    if binary_input is False or not _cfg("DETECT_BINARY_INPUT"):
        return False
    ok, flag = detect_pm1(input, weight)
    if not ok:
        return False
    return True if flag is None else flag


def split_hint(binary_input):
    """(binary_input as True / False / None, device flag to fold into the bias or None) — see ``half_gate``."""
    if isinstance(binary_input, torch.Tensor):
        return True, binary_input
    return binary_input, None


def half_bias(bias: Optional[torch.Tensor], dtype) -> Optional[torch.Tensor]:
    """The bias as the fp32 vector the epilogues add: a half bias upcast (exact); an fp32 bias under autocast rounded to the
    autocast dtype first, as the cast in front of the reference's F.linear does."""
    if bias is None:
        return None
    b = bias.detach()
    return b.to(dtype).float() if b.dtype != dtype else b.float()


def codes_route(codes, weight: Optional[torch.Tensor]):
    """(use the int8 code planes?, device flag or None) for DoReFa activation codes whose range flag is on the device."""
    if ops._cfg("ASSUME_CODES_FIT") or codes.overflow is None:
        return True, None
    ok, cached = _verdict(weight, ("codes", int(codes.K)), codes.usable)
    if ok and cached:
        return True, register_flag(codes.overflow)
    return ok, None


def poison_bias(bias: Optional[torch.Tensor], flag: Optional[torch.Tensor], n: int, device) -> Optional[torch.Tensor]:
    """bias (+ NaN if the device flag is raised): one tiny launch instead of a host sync."""
    if flag is None:
        return bias
    if flag.dtype == torch.int32 and flag.is_cuda:
        return ops.poison(bias.detach() if bias is not None else None, flag, -1, n)
    nanv = torch.where(flag.reshape(()) != 0, float("nan"), 0.0)
    base = bias.detach() if bias is not None else torch.zeros((n,), dtype=torch.float32, device=device)
    return base + nanv


def activation_planes(input: torch.Tensor, binary_input: Optional[bool], impl: str = "valu",
                      weight: Optional[torch.Tensor] = None, half_ok: bool = False):
    """(packed image of a device activation in the format of ``impl`` if it is (treated as) exactly +-1 else None,
    device flag to fold into the bias or None).  ``half_ok``: bf16 / fp16 activations are packed as well (the sign layers'
    half route); every other caller keeps fp32 only."""
    if input.dtype not in (ops.PACK_DTYPES if half_ok else (torch.float32,)) or input.numel() == 0:
        return None, None
    tagged = packed.lookup(input, packed.ROWS_LAST)
    if tagged is not None:
        K = input.shape[-1]
        if tagged.K == K and tagged.rows * K == input.numel():
            return ops.to_impl(tagged, impl), None   # bit planes from the quantiser (1 bit -> 4 bits if mfma)
    if binary_input is False:
        return None, None
    flag = None
    if binary_input is None and tagged is None:
        if not _cfg("DETECT_BINARY_INPUT"):
            return None, None
        ok, flag = detect_pm1(input, weight)
        if not ok:
            return None, None
    return ops.pack_activations(input, impl), flag


def quant_linear_forward(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor],
                         kind: str, weight_q: Optional[torch.Tensor] = None,
                         weight_planes: Optional[ops.BitPlanes] = None,
                         binary_input: Optional[bool] = None, half_ok: bool = False) -> torch.Tensor:
    """y = input . Q(weight)^T + bias.

    ``weight_q``: explicit fp32 quantised weight (stochastic draw, or eval-mode pre-quantised
    weight); ``weight_planes``: cached planes of that same quantised weight.
    """
    if not input.is_cuda:
        wq = weight_q if weight_q is not None else quantize_weight_f32(weight, kind)
        return F.linear(input, wq, bias)

    K = input.shape[-1]
    N = weight.shape[0]
    M = input.numel() // max(K, 1)
    impl = ops.select_gemm_impl(_cfg("GEMM_IMPL"), M, N, K)
    binary_input, hint_flag = split_hint(binary_input)
    # ``half_ok`` (the sign layers' half route): a bf16 / fp16 activation is packed and the result has its dtype
    odt = input.dtype if (half_ok and input.dtype in ops.HALF_DTYPES) else None
    if odt is not None:
        bias = half_bias(bias, odt)
    if (impl == "mfma" and weight_planes is None and (input.dtype == torch.float32 or odt is not None) and input.numel() > 0
            and binary_input is not False and packed.lookup(input, packed.ROWS_LAST) is None):
        ok, flag = (True, hint_flag) if binary_input else (detect_pm1(input, weight) if _cfg("DETECT_BINARY_INPUT") else (False, None))
        if ok:
            # neither operand is packed yet (un-tagged +-1 activation, training-mode weight): one launch packs both
            wq = weight_q if weight_q is not None else weight
            xp, wp = ops.pack_linear_operands(input, wq.reshape(N, -1), kind, impl)
            return ops.packed_gemm(xp, wp, poison_bias(bias, flag, N, input.device), impl=impl,
                                   out_dtype=odt).view(*input.shape[:-1], N)
        binary_input = False                      # verdict known: do not ask again below
    xp, flag = activation_planes(input, binary_input, impl, weight, half_ok=odt is not None)
    if xp is not None:
        flag = hint_flag if flag is None else flag
        wp = weight_planes
        if wp is None:
            wq = weight_q if weight_q is not None else weight
            wp = pack_weight(wq.reshape(N, -1), kind, impl)
        y = ops.packed_gemm(xp, wp, poison_bias(bias, flag, N, input.device), impl=impl, out_dtype=odt)
        return y.view(*input.shape[:-1], N)
    if odt is not None:
        raise RuntimeError("a half-precision activation that is not +-1 has no packed route: the layers send it to the torch expression")

    if _cfg("FLOAT_PATH") == "bf16x3" and input.dtype == torch.float32 and input.numel() > 0:
        # the quantisers are idempotent, so an explicit quantised image (eval / stochastic) goes through
        # the same weight packer
        return ops.float_linear(input, weight_q if weight_q is not None else weight, kind, bias,
                                weight_triples=weight_planes if isinstance(weight_planes, ops.TriplePlanes) else None)
    wq = weight_q if weight_q is not None else quantize_weight_f32(weight, kind)
    note_library_path(input, "non-fp32 or empty linear input")
    return F.linear(input, wq, bias)


def _pixel_planes(input: torch.Tensor, binary_input: Optional[bool], weight: Optional[torch.Tensor] = None, ld_fn=None,
                  half_ok: bool = False):
    """(NHWC nibble pixel plane of a device activation that is (treated as) exactly +-1 else None, device flag to fold
    into the bias or None).  ``ld_fn``: words per pixel as a function of the channel count (default ops.pixel_ld_nib);
    ``half_ok``: as in ``activation_planes``."""
    if input.dtype not in (ops.PACK_DTYPES if half_ok else (torch.float32,)) or input.dim() != 4 or input.numel() == 0:
        return None, None
    ld_fn = ld_fn or ops.pixel_ld_nib
    tagged = packed.lookup(input, packed.NHWC)
    if tagged is not None:
        N, C, H, W = input.shape
        if tagged.K == C and tagged.rows == N * H * W:
            return ops.bits_to_nib(tagged, ld=ld_fn(C)), None
    if binary_input is False:
        return None, None
    flag = None
    if binary_input is None and tagged is None:
        if not _cfg("DETECT_BINARY_INPUT"):
            return None, None
        ok, flag = detect_pm1(input, weight)
        if not ok:
            return None, None
    return ops.pack_pixels_nib(input, ld=ld_fn(int(input.shape[1]))), flag


def first_layer_rungs(C, Cout, kernel_hw, stride, padding, dilation, H, W, kind: str, out=None, pooled: bool = False, allowed=None):
    """The rungs ``first_layer_conv_routes`` tries, in ladder order: pure (predicates and switches, read on every call; nothing is
    launched).  "binary" / "ternary": first3x3, direct3x3, d2s, first_direct, s2d, plain; "xnor" (the real image sign(W) * alpha):
    first_direct_real, bf16x6.  ``out``: None = the fp32 result, "bits" = threshold bits, (hy, hx) = the next conv's nibble plane
    with that halo.  ``pooled``: a pool follows, so a nibble ``out`` names what the BLOCK hands on and the conv writes bits; it
    matters only with a nibble ``out`` (the fused block asks for bits itself when it pools).  ``allowed``: the caller's rungs
    (None = all).  The runner walks the same code as a generator and never evaluates the predicates behind the rung that ran."""
    return tuple(_walk_first_layer_rungs(C, Cout, kernel_hw, stride, padding, dilation, H, W, kind, out, pooled, allowed))


def _walk_first_layer_rungs(C, Cout, kernel_hw, stride, padding, dilation, H, W, kind, out, pooled, allowed):
    # (imported here on purpose: layers.fused imports this module, and its two switches are read from it at call time)
    from ..layers import fused as blocks
    kernel_hw = (int(kernel_hw[0]), int(kernel_hw[1]))
    geom = (kernel_hw, stride, padding, dilation)
    if kind == "xnor":
        if (allowed is None or "first_direct_real" in allowed) and ops.first_direct_applicable(C, *geom):
            yield "first_direct_real"
        if allowed is None or "bf16x6" in allowed:
            yield "bf16x6"
        return
    nib = isinstance(out, tuple) and not pooled
    if (allowed is None or "first3x3" in allowed) and ops.first3x3_applicable(C, Cout, *geom):
        yield "first3x3"
    # planes only: the direct kernel writes bits or the halo-1 nibble plane, the output-blocked form regroups in the nibble epilogue
    if ((allowed is None or "direct3x3" in allowed) and blocks.DIRECT_FIRST_LAYER and out is not None
            and (not nib or tuple(out) == (1, 1)) and ops.direct_first_layer_applicable(C, Cout, *geom)):
        yield "direct3x3"
    if ((allowed is None or "d2s" in allowed) and blocks.D2S_FIRST_LAYER and nib
            and ops.d2s_first_layer_applicable(C, Cout, *geom, H, W)):
        yield "d2s"
    if (allowed is None or "first_direct" in allowed) and ops.first_direct_applicable(C, *geom):
        yield "first_direct"
    if (allowed is None or "s2d" in allowed) and USE_S2D and ops.s2d_applicable(C, *kernel_hw, stride, dilation, padding):
        yield "s2d"
    if allowed is None or "plain" in allowed:
        yield "plain"


def first_layer_weight_planes(form: str, wq: torch.Tensor, kind: str, stride: int, terms: Optional[int] = None):
    """The QUANTISED weight image ``wq`` as the operand of rung ``form`` (eval-mode layers cache it: ``_conv_triples``)."""
    if form == "first3x3":                                   # MFMA row fragments of the one-pass 3 x 3 kernel
        return ops.pack_first3x3_weight(wq)
    if form in ("first_direct", "first_direct_real"):        # fragment-ordered fp16 weight of the direct kernel (two terms: real)
        return ops.pack_first_layer_weight(wq, stride, real=form == "first_direct_real")
    if form == "plain":
        return ops.pack_conv_weight_bf16x3(wq, kind, terms=terms)
    if form == "bf16x6":
        return ops.pack_conv_weight_bf16x6(wq)
    # "s2d" / "d2s": (shape, split image) of the weight of the stride-1 conv on the space-to-depth image
    ws = ops.s2d_weight(ops.d2s_first_layer_weight(wq.detach()), 2) if form == "d2s" else ops.s2d_weight(wq.detach(), stride)
    return tuple(ws.shape), ops.pack_conv_weight_bf16x3(ws, "sign", terms=terms)      # zeros stay zeros


def first_layer_conv_routes(input, weight, bias, stride, padding, dilation, kind: str, epi=None, weight_q=None, cache=None,
                            rungs=None, pooled: bool = False, taken: Optional[list] = None):
    """THE ladder of the forward routes of a sign-family conv (groups == 1, zero padding) on a REAL-valued device fp32 image, the
    network's first layer: runs the first rung of ``first_layer_rungs`` whose launch wrapper takes the shape and returns
    (result, (N, Cout, Ho, Wo)); None when no rung ran.  The result is what ``epi`` asks for: None — the NHWC fp32 matrix;
    (alpha, beta) — the BitPlanes of [(conv + bias) * alpha + beta < 0]; a NibEpilogue — the next conv's nibble plane.

    Every output form of a rung comes from ONE accumulation: the threshold bits of the fused / deferred chain must come from the
    very accumulators the fp32 output of the module-by-module execution shows, or the two differ at ties.  A rung that cannot
    write the requested nibble plane is therefore handed (alpha, beta) and its bits are expanded here, once.
    ``kind``: "binary" / "ternary", or "xnor" for the real weight image sign(W) * alpha (``weight_q``).  ``cache``: the layer's
    ``_conv_triples`` (``cache(form[, terms])``: the cached operand of the eval-mode weight) or None: packed on the fly from
    ``weight_q`` (default: the idempotent quantiser of ``kind`` on ``weight``).  ``rungs``: the rungs the caller allows;
    ``pooled``: see ``first_layer_rungs``; ``taken``: a list that receives the name of the rung that ran."""
    N, C, H, W = (int(v) for v in input.shape)
    Cout, kh, kw = int(weight.shape[0]), int(weight.shape[2]), int(weight.shape[3])
    nib = epi if isinstance(epi, ops.NibEpilogue) else None
    out = None if epi is None else (tuple(nib.out_halo) if nib is not None else "bits")
    # (nothing but the walk in front of the first rung: a caller whose rungs do not apply pays for the predicates alone)
    for rung in _walk_first_layer_rungs(C, Cout, (kh, kw), stride, padding, dilation, H, W, kind, out, pooled, rungs):
        y = _first_layer_rung(rung, input, weight, bias, stride, padding, dilation, kind, epi, weight_q, cache)
        if y is None:
            continue
        Ho, Wo = ops.conv_out_hw(H, W, kh, kw, stride, padding, dilation)
        if nib is not None and isinstance(y, ops.BitPlanes):
            y = ops.bits_to_nib_pad(y, N, Ho, Wo, nib.out_halo, ld=ops.pixel_ld_nib(y.K))
        if taken is not None:
            taken.append(rung)
        return y, (N, Cout, Ho, Wo)
    return None


def _first_layer_rung(rung, input, weight, bias, stride, padding, dilation, kind, epi, weight_q, cache):
    """One rung of ``first_layer_conv_routes``: fp32 rows, BitPlanes or NibPlanes; None when the launch wrapper declines the shape."""
    (N, C, H, W), Cout, sd = (int(v) for v in input.shape), int(weight.shape[0]), ops._pairs(stride)[0]
    nib = epi if isinstance(epi, ops.NibEpilogue) else None
    affine = ops.epilogue_affine(epi)[:2] if epi is not None else None

    def planes(form, terms=None):
        got = cache(form, terms) if cache is not None else None
        if got is None:
            got = first_layer_weight_planes(form, weight_q if weight_q is not None else quantize_weight_f32(weight, kind), kind, sd, terms)
        return got

    def conv_on_s2d_image(px, Hs, Ws, s, wplanes, b, e):      # (the gather and the split were one kernel)
        return ops.float_conv2d(None, torch.empty(wplanes[0], device="meta"), "sign", b, 1, 0, 1, weight_triples=wplanes[1],
                                pixels=px, in_shape=(N, C * s * s, Hs, Ws), epi=e)

    if rung == "first3x3":
        # VGG-16's conv1_1: the one-pass kernel reads the fp32 image where it lies and writes fp32, bits or the halo-1 nibble plane
        own = nib is None or (tuple(nib.out_halo) == (1, 1) and not nib.d2s_cout)
        return ops.conv_first3x3(input, planes(rung), Cout, bias, epi=epi if own else affine)
    if rung == "direct3x3":
        # 3 x 3 / stride 1 / padding 1, <= 5 channels: the direct kernel on the padded fp16-pair (two taps per MFMA) / bf16-triple plane
        terms = ops.direct_first_layer_terms(C)
        px, _ = ops.s2d_triple_pack(input, 1, 1, terms=terms)
        return ops.conv3x3_direct_nib(px, N, C, H, W, planes("plain", terms), bias, epi)
    if rung == "d2s":
        # the 2x2 output-blocked form (ops.d2s_first_layer_weight): 2x2 taps over the space-to-depth(2) image, 4 * Cout columns,
        # depth-to-space in the nibble epilogue — the same products from a quarter of the gathered bytes (VGG-16 conv1: 550 -> 290 us)
        wplanes = planes(rung)
        px, (Hs, Ws) = ops.s2d_triple_pack(input, 2, 1)
        e = ops.NibEpilogue(affine[0].repeat(4), affine[1].repeat(4), nib.out_halo, d2s_cout=Cout)
        return conv_on_s2d_image(px, Hs, Ws, 2, wplanes, bias.detach().repeat(4) if bias is not None else None, e)
    if rung in ("first_direct", "first_direct_real"):
        # strided few-channel conv (AlexNet conv1): the direct kernel splits its patch in registers, no operand pack pass.  (Its fp32
        # store tail makes the module-by-module conv1 ~100 us slower than "s2d" there — not the inference path: tools/bench_conv1.py)
        return ops.conv_first_direct(input, planes(rung), bias, stride, padding, epi=affine)
    if rung == "s2d":
        # strided / padded few-channel conv == stride-1 conv on the space-to-depth image; pixels the rounding added are cropped (a
        # nibble epilogue maps rows with the kernel's own (H2, W2) geometry, so then: bits, cropped, expanded by the runner)
        px, (Hs, Ws) = ops.s2d_triple_pack(input, sd, padding)
        wplanes = planes(rung)
        H2, W2 = Hs - wplanes[0][2] + 1, Ws - wplanes[0][2] + 1
        Ho, Wo = ops.conv_out_hw(H, W, int(weight.shape[2]), int(weight.shape[3]), stride, padding, dilation)
        crop = (H2, W2) != (Ho, Wo)
        y = conv_on_s2d_image(px, Hs, Ws, sd, wplanes, bias, affine if (crop and nib is not None) else epi)
        if crop:
            rows = (y if epi is None else y.sign).view(N, H2, W2, -1)[:, :Ho, :Wo, :].contiguous().view(N * Ho * Wo, -1)
            y = rows if epi is None else ops.BitPlanes(sign=rows, rows=N * Ho * Wo, K=y.K)
        return y
    if rung == "plain":
        return ops.float_conv2d(input, weight_q if weight_q is not None else weight, kind, bias, stride, padding, dilation,
                                weight_triples=cache("plain") if cache is not None else None, epi=epi)
    # "bf16x6": real x real on six-term bf16 planes, implicit-GEMM conv on the matrix cores (fp32-GEMM accuracy)
    return ops.real_conv2d(input, (weight_q if weight_q is not None else weight).detach(), bias, stride, padding, dilation,
                           weight_planes=cache(rung) if cache is not None else None, epi=epi)


def quant_conv2d_forward(input, weight, bias, stride, padding, dilation, groups, kind: str,
                         weight_q: Optional[torch.Tensor] = None, weight_planes=None,
                         binary_input: Optional[bool] = None, padding_mode: str = "zeros",
                         weight_triples_fn=None, epi=None, half_ok: bool = False):
    """conv2d(input, Q(weight), bias, ...).

    ``epi`` = (alpha, beta) (inference fusion, layers/fused.py): the conv does not write fp32 but the
    threshold bits [(conv + bias) * alpha + beta < 0]; returns (BitPlanes NHWC pixel plane, (N, Cout, Ho, Wo)).

    Device tensor with +-1 activations, groups == 1, zero padding: NHWC pixel planes -> packed-domain
    im2col -> matrix-core packed GEMM (libqt_hip.so); the result keeps the input's memory format
    (channels_last in -> channels_last out, like torch's own conv).  Otherwise (first layer with real
    pixels, grouped conv): weight quantised by the HIP elementwise kernel, contraction by the dense
    conv library on the exact +-1/0 weight image."""
    packable = (input.is_cuda and groups == 1 and padding_mode == "zeros" and input.dim() == 4
                and not isinstance(padding, str))
    # ``half_ok`` (the sign layers' half route): a bf16 / fp16 +-1 activation is packed and the result has its dtype
    odt = input.dtype if (half_ok and input.is_cuda and input.dtype in ops.HALF_DTYPES) else None
    if odt is not None and epi is not None:
        raise ValueError("the threshold / code epilogues take fp32 activations")
    binary_input, hint_flag = split_hint(binary_input)
    if packable:
        px, flag = _pixel_planes(input, binary_input, weight, half_ok=odt is not None)
        if px is not None:
            flag = hint_flag if flag is None else flag
            if odt is not None:
                bias = half_bias(bias, odt)
            bias = poison_bias(bias, flag, int(weight.shape[0]), input.device)
            wq = weight_q if weight_q is not None else weight
            wp = weight_planes if isinstance(weight_planes, ops.NibPlanes) else ops.pack_conv_weight_nib(wq, kind)
            N, C, H, W = input.shape
            kh, kw = int(weight.shape[2]), int(weight.shape[3])
            y2 = ops.conv2d_nib(px, (N, C, H, W), wp, (kh, kw), bias, stride, padding, dilation, epi=epi, out_dtype=odt)
            Ho, Wo = ops.conv_out_hw(H, W, kh, kw, stride, padding, dilation)
            if epi is not None:
                return y2, (N, int(weight.shape[0]), Ho, Wo)
            return nchw_result(y2, input, N, Ho, Wo, weight.shape[0])
    if odt is not None:
        raise RuntimeError("a half-precision activation that is not +-1 has no packed route: the layers send it to the torch expression")
    if packable and _cfg("FLOAT_PATH") == "bf16x3" and input.dtype == torch.float32 and input.numel() > 0:
        # real-valued activation (first layer): split operands on the matrix cores, on the first rung of the ladder that takes it
        y2, shape = first_layer_conv_routes(input, weight, bias, stride, padding, dilation, kind, epi=epi, weight_q=weight_q,
                                            cache=weight_triples_fn, rungs=("first3x3", "first_direct", "s2d", "plain"))
        return (y2, shape) if epi is not None else nchw_result(y2, input, shape[0], shape[2], shape[3], shape[1])
    if epi is not None:
        raise ValueError("the threshold-bit epilogue needs a device fp32 NCHW input, groups == 1 and zero padding")
    wq = weight_q if weight_q is not None else quantize_weight_f32(weight, kind)
    note_library_path(input, "grouped / non-zero padding mode / non-fp32 conv")
    return F.conv2d(input, wq, bias, stride, padding, dilation, groups)


def real_weight_linear(input: torch.Tensor, weight_q: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """F.linear(input, weight_q, bias) for an ALREADY QUANTISED, real-valued weight image (the deprecated functional
    forms: TernaryDense's torch.sign formula keeps w = +-0.5 as +-0.5, QuantDense's levels are odd integers / (2^k - 1),
    functions/terner_connect.py:85-94, dorefa_connect.py:124-132).  Device fp32 2-D: six-term bf16 planes on the matrix
    cores (ops.real_linear, fp32-GEMM accuracy); everything else: the torch expression."""
    if (input.is_cuda and input.dtype == torch.float32 and weight_q.dtype == torch.float32 and input.dim() == 2
            and input.numel() > 0 and weight_q.numel() > 0):
        return ops.real_linear(input.detach(), weight_q.detach(), bias.detach() if bias is not None else None)
    return F.linear(input, weight_q, bias)


def real_weight_conv2d(input: torch.Tensor, weight_q: torch.Tensor, bias, stride, padding, dilation, groups) -> torch.Tensor:
    """F.conv2d(input, weight_q, ...) for an already quantised real-valued weight image (TernaryConv2d / QuantConv2d /
    XNORConv2d functional forms): implicit-GEMM conv over six-term bf16 planes (ops.real_conv2d) for device fp32 NCHW
    inputs with groups == 1 and numeric zero padding; the result keeps the input's memory format."""
    if (input.is_cuda and input.dtype == torch.float32 and weight_q.dtype == torch.float32 and input.dim() == 4
            and input.numel() > 0 and groups == 1 and not isinstance(padding, str)):
        y2 = ops.real_conv2d(input.detach(), weight_q.detach(), bias.detach() if bias is not None else None, stride,
                             padding, dilation)
        if y2 is not None:
            N_, _, H, W = input.shape
            Ho, Wo = ops.conv_out_hw(H, W, weight_q.shape[2], weight_q.shape[3], stride, padding, dilation)
            return nchw_result(y2, input, N_, Ho, Wo, weight_q.shape[0])
    return F.conv2d(input, weight_q, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=groups)


def packed_linear(layer, act, kind: str, hwc=None) -> torch.Tensor:
    """Eval-mode LinearBin / LinearTer on a PackedActivation (row planes): planes -> packed GEMM.  ``hwc`` = (C, H, W):
    the rows are a feature map flattened in (h, w, c) order (PackedActivation.flatten_hwc) while the layer's weight
    expects the NCHW flattening — the packed weight is built from the column-permuted image (cached like the plain one)."""
    if layer.training:
        raise RuntimeError("PackedActivation inputs are an inference feature: call .eval() first")
    N = layer.weight.shape[0]
    M, K = act.planes.rows, act.planes.K
    if K != layer.weight.shape[1]:
        raise ValueError(f"packed activation has {K} features, layer expects {layer.weight.shape[1]}")
    impl = ops.select_gemm_impl(_cfg("GEMM_IMPL"), M, N, K)
    if hwc is None:
        wp = layer._eval_planes(lambda w2: pack_weight(w2, kind, impl), key=impl)
    else:
        from ..layers.fused import permute_fc_weight_hwc
        C, H, W = (int(v) for v in hwc)
        wp = layer._eval_planes(lambda w2: pack_weight(permute_fc_weight_hwc(w2, C, H, W), kind, impl),
                                key=(impl, "hwc", C, H, W))
    y = ops.packed_gemm(ops.to_impl(act.planes, impl), wp, layer.bias, impl=impl)
    return y.view(*act.shape[:-1], N)


def packed_conv2d(layer, act, kind: str, epi=None):
    """Eval-mode BinConv2d / TerConv2d on a PackedActivation (NHWC planes).  Returns a channels_last
    [N, Cout, Ho, Wo] fp32 tensor, or with ``epi`` = (alpha, beta) the threshold-bit planes and shape
    (see quant_conv2d_forward)."""
    if layer.training:
        raise RuntimeError("PackedActivation inputs are an inference feature: call .eval() first")
    if layer.groups != 1 or layer.padding_mode != "zeros":
        raise ValueError("packed conv needs groups == 1 and zero padding")
    if kind == "xnor":
        return packed_xnor_conv2d(layer, act, epi)
    N, C, H, W = act.shape
    wp = layer._eval_planes(lambda _w2: ops.pack_conv_weight_nib(layer.weight.detach(), kind), key="conv_nib")
    kh, kw = int(layer.weight.shape[2]), int(layer.weight.shape[3])
    ph, pw = ops._pairs(layer.padding)
    if act.nib is not None:
        # the producer already wrote this conv's operand: nibble pixel plane with the padding as a physical zero border
        if act.halo != (ph, pw):
            raise ValueError(f"activation carries a {act.halo} halo, this conv pads {(ph, pw)}: re-link the fused modules")
        if ops.direct_conv3x3_applicable(C, int(layer.weight.shape[0]), (kh, kw), layer.stride, layer.padding,
                                         layer.dilation, act.halo, epi):
            y2 = ops.conv3x3_direct_nib(act.nib, N, C, H, W, wp, layer.bias, epi)
            return y2, (N, int(layer.weight.shape[0]), H, W)
        y2 = ops.conv2d_nib(act.nib, (N, C, H + 2 * ph, W + 2 * pw), wp, (kh, kw), layer.bias, layer.stride, 0,
                            layer.dilation, epi=epi)
    elif _cfg("PAD_PLANES") and (ph or pw):
        # zero padding made physical while the bits are expanded: the conv runs un-padded (no per-tap checks)
        px = ops.bits_to_nib_pad(act.planes, N, H, W, (ph, pw), ld=ops.pixel_ld_nib(C))
        y2 = ops.conv2d_nib(px, (N, C, H + 2 * ph, W + 2 * pw), wp, (kh, kw), layer.bias, layer.stride, 0,
                            layer.dilation, epi=epi)
    else:
        px = ops.bits_to_nib(act.planes, ld=ops.pixel_ld_nib(C))
        y2 = ops.conv2d_nib(px, (N, C, H, W), wp, (kh, kw), layer.bias, layer.stride, layer.padding, layer.dilation,
                            epi=epi)
    Ho, Wo = ops.conv_out_hw(H, W, kh, kw, layer.stride, layer.padding, layer.dilation)
    if epi is not None:
        return y2, (N, int(layer.weight.shape[0]), Ho, Wo)
    return y2.view(N, Ho, Wo, layer.weight.shape[0]).permute(0, 3, 1, 2)


def packed_depthwise_conv2d(layer, act):
    """Eval-mode BinConv2d / TerConv2d with ``groups == in_channels`` on a PackedActivation (NHWC bit planes): the fp32
    [N, C * m, Ho, Wo] result in NCHW storage, bias added, from one launch on the planes (ops.depthwise_conv2d_from_bits) — what a
    deferred depthwise conv whose input exists only as planes materialises to.  The stored eval image is multiplied as it is."""
    return _packed_streaming_conv2d(_DEPTHWISE, layer, act)


def _depthwise_admission(layer, act, what: str) -> None:
    if (layer.padding_mode != "zeros" or len(act.shape) != 4
            or not ops.depthwise_applicable(act.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation, layer.groups)):
        raise ValueError(f"{what} needs groups == in_channels, numeric zero padding and a shape inside the kernels' limits")


def _grouped_planes_admission(layer, act, what: str) -> None:
    if (layer.padding_mode != "zeros" or len(act.shape) != 4 or layer.groups < GROUPED_MIN_GROUPS
            or not ops.grouped_planes_applicable(act.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation, layer.groups)):
        raise ValueError(f"{what} needs at least {GROUPED_MIN_GROUPS} groups of 2, 4 or 8 input channels, numeric zero "
                         "padding and a shape inside the kernels' limits")
    if not layer._eval_on_grid():
        raise ValueError(f"{what} needs an eval-mode weight on the quantiser's grid")


def _grouped_codes_admission(layer, act, what: str) -> None:
    cin_g = int(layer.weight.shape[1])
    if (layer.padding_mode != "zeros" or len(act.shape) != 4 or layer.groups < GROUPED_MIN_GROUPS or not 2 <= cin_g <= GROUPED_MAX_CIN_G
            or not ops.grouped_codes_applicable(act.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation, layer.groups)):
        raise ValueError(f"{what} needs at least {GROUPED_MIN_GROUPS} groups of 2 ... {GROUPED_MAX_CIN_G} input channels, "
                         "numeric zero padding and a shape inside the kernels' limits")


def _packed_streaming_conv2d(fam, layer, act):
    """A deferred streaming conv (``fam``: ``_DEPTHWISE`` | ``_GROUPED``) materialised from the bit planes of its input."""
    if layer.training:
        raise RuntimeError("PackedActivation inputs are an inference feature: call .eval() first")
    if act.planes is None:
        raise ValueError(f"a {fam.ops_family.noun} conv reads bit planes; this activation was produced as another conv's nibble operand")
    fam.planes_admission(layer, act, f"packed {fam.ops_family.noun} conv")
    return ops._streaming_conv2d_from_bits(fam.ops_family, act.planes, act.shape, layer.weight.detach(), layer.bias, layer.stride,
                                           layer.padding, layer.dilation, layer.groups, "raw")


def _codes_streaming_conv2d(fam, layer, act):
    """A deferred streaming DoReFa conv materialised from the code plane of its input."""
    if layer.training:
        raise RuntimeError("CodeActivation inputs are an inference feature: call .eval() first")
    fam.codes_admission(layer, act, f"{fam.ops_family.noun} conv on codes")
    return ops._streaming_conv2d_from_codes(fam.ops_family, act.codes, act.shape, layer.weight.detach(), layer.bias, layer.stride,
                                            layer.padding, layer.dilation, layer.groups, in_halo=act.halo,
                                            channels_last=bool(act.source_channels_last), flagged=not ops._cfg("ASSUME_CODES_FIT"))


def codes_depthwise_conv2d(layer, act):
    """Eval-mode DorefaConv2d with ``groups == in_channels`` (any weight bit_width) on a CodeActivation: the fp32 [N, C * m, Ho, Wo]
    result in channels-last storage (the code tag of an NCHW fp32 tensor: NCHW, as the eager conv returns), bias added, from one launch
    on the code plane (ops.depthwise_conv2d_from_codes) — what a
    deferred depthwise DoReFa conv materialises to when its chain cannot run fused.  The stored eval image is multiplied as it is;
    a raised int8 range flag of the activation's chain makes the result NaN on the device (as ``CodeActivation.float``)."""
    return _codes_streaming_conv2d(_DEPTHWISE, layer, act)


def packed_grouped_conv2d(layer, act):
    """Eval-mode BinConv2d / TerConv2d with ``1 < groups < in_channels`` on a PackedActivation (NHWC bit planes): the fp32
    [N, G * cout_g, Ho, Wo] result in NCHW storage, bias added, from one launch on the planes (ops.grouped_conv2d_from_bits) — what a
    deferred grouped conv whose input exists only as planes materialises to.  The stored eval image is classified by its sign."""
    return _packed_streaming_conv2d(_GROUPED, layer, act)


def codes_grouped_conv2d(layer, act):
    """Eval-mode DorefaConv2d with ``1 < groups < in_channels`` (any weight bit_width) on a CodeActivation: the sibling of
    ``codes_depthwise_conv2d`` — the fp32 [N, G * cout_g, Ho, Wo] result in the layout the module graph's conv result has
    (``CodeActivation.source_channels_last``), bias added, from one launch on the code plane (ops.grouped_conv2d_from_codes); what a
    deferred grouped DoReFa conv materialises to when its chain cannot run fused.  The stored eval image is multiplied as it is; a
    raised int8 range flag of the activation's chain makes the result NaN on the device."""
    return _codes_streaming_conv2d(_GROUPED, layer, act)


def packed_xnor_conv2d(layer, act, epi=None):
    """Eval-mode XNORConv2d on a PackedActivation: the per-tap scaled fp4 conv (ops.conv2d_nib_taps) on the activation's nibble
    plane — the producer's own (zero halo = this conv's padding, un-padded kernel) when its pixel stride is whole 32-byte taps,
    else expanded from the bit planes with the padding made physical.  Same returns as packed_conv2d."""
    N, C, H, W = act.shape
    wp, taps = layer._taps_planes()
    kh, kw = int(layer.weight.shape[2]), int(layer.weight.shape[3])
    ph, pw = ops._pairs(layer.padding)
    Cw = ops.pixel_ld_nib_taps(C)
    if act.nib is not None:
        if act.halo != (ph, pw):
            raise ValueError(f"activation carries a {act.halo} halo, this conv pads {(ph, pw)}: re-link the fused modules")
        px = act.nib
        if px.ld != Cw:       # channels not a multiple of 64: widen the pixel stride to whole 32-byte taps (zero nibbles)
            wide = torch.zeros((int(px.words.shape[0]), Cw), dtype=torch.int32, device=px.device)
            wide[:, :px.ld] = px.words
            px = ops.NibPlanes(words=wide, rows=px.rows, K=px.K)
    else:
        px = ops.bits_to_nib_pad(act.planes, N, H, W, (ph, pw), ld=Cw)
    y2 = ops.conv2d_nib_taps(px, (N, C, H + 2 * ph, W + 2 * pw), wp, (kh, kw), taps.fwd, layer.bias, layer.stride, 0,
                             layer.dilation, epi=epi)
    if y2 is None:
        raise ValueError("XNOR conv outside the per-tap kernel's limits")
    Ho, Wo = ops.conv_out_hw(H, W, kh, kw, layer.stride, layer.padding, layer.dilation)
    if epi is not None:
        return y2, (N, int(layer.weight.shape[0]), Ho, Wo)
    return y2.view(N, Ho, Wo, layer.weight.shape[0]).permute(0, 3, 1, 2)


def packed_xnor_linear(layer, act, hwc=None) -> torch.Tensor:
    """Eval-mode LinearXNOR on a PackedActivation (row planes): y = (x * alpha) . sign(W)^T + b (xnor_connect.py:112-115) with
    x * alpha = +-alpha[k] built from the sign bits as two-term fp16 pairs (qt_bits_alpha_pairs_f16x2) against the replicated
    sign(W) on the fp16 matrix cores.  ``hwc`` = (C, H, W): the rows are a feature map flattened in (h, w, c) order; the pair
    kernel reads the bits in the weight's own NCHW order, so the sum runs in the module graph's order (bit-identical logits)."""
    if layer.training:
        raise RuntimeError("PackedActivation inputs are an inference feature: call .eval() first")
    N = layer.weight.shape[0]
    K = act.planes.K
    if K != layer.weight.shape[1]:
        raise ValueError(f"packed activation has {K} features, layer expects {layer.weight.shape[1]}")

    dg = xnor_linear_digits(layer) if _cfg("XNOR_LINEAR_DIGITS") else None
    if dg is not None and 3 * act.planes.rows * int(dg[0].codes.shape[1]) >= (1 << 31):
        dg = None                                               # the stacked digit planes pass the GEMM's 32-bit operand offsets
    if dg is not None:
        # integer form: alpha as three 7-bit digits against the int8 codes of sign(W) — exact partial sums, 1 byte per weight
        y = ops.xnor_digit_linear(act.planes, dg[1], dg[0], layer.bias, hwc=hwc)
    else:
        wt, ap = xnor_linear_operands(layer)
        y = ops.bf16_gemm(ops.bits_alpha_pairs(act.planes, ap, hwc=hwc), wt, layer.bias)
    return y.view(*act.shape[:-1], N)


#: LinearXNOR on packed +-1 activations: True = the digit-plane int8 form (ops.xnor_digit_linear), False = fp16 pairs of +-alpha
XNOR_LINEAR_DIGITS = True


def xnor_linear_digits(layer):
    """(int8 codes of sign(W), digit table of alpha[K] = mean(|W|, 0)) of an eval-mode LinearXNOR weight, cached per weight
    version; None when alpha has a non-finite entry or K is beyond the exact range (the pair route then reproduces the NaN / inf
    the reference would produce)."""
    def build(w2):
        ld = ops.code_ld_bytes(int(w2.shape[1]))
        if 127 * ld >= (1 << 24) or int(w2.shape[0]) * ld >= (1 << 31):       # exact fp32 partial sums; 32-bit operand offsets
            return None
        _, alpha = ops.xnor_weight(w2.contiguous(), 1)
        dg = ops.alpha_digits(alpha.view(-1))
        if dg is None:
            return None
        return ops.weight_codes(torch.sign(w2), ternary=True), dg         # torch.sign: 0 -> 0 (xnor_connect.py:113)
    return layer._eval_planes(build, key="xnor_digits")


def xnor_linear_operands(layer=None, weight=None):
    """(fp16 pair planes of sign(W), pair image of alpha[K] = mean(|W|, 0)) of a LinearXNOR weight: cached per weight version
    for an eval-mode ``layer``, built on the spot for a training-mode ``weight``."""
    def build(w2):
        _, alpha = ops.xnor_weight(w2.contiguous(), 1)                       # alpha[1, K] (eval: of the already quantised image)
        return ops.weight_bf16x3(w2, "sign", terms=2), ops.alpha_pairs(alpha.view(-1))
    if layer is not None:
        return layer._eval_planes(build, key="xnor_pairs")
    return build(weight.detach())


def _dense(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when it is dense in NCHW or channels-last order (the conv kernels take element strides), else an NCHW
    copy.  A plain ``.contiguous()`` would transpose every channels-last gradient back to NCHW."""
    if t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)):
        return t
    return t.contiguous()


class QuantConv2dFn(QtFunction):
    """Autograd node of BinConv2d / TerConv2d in training mode: forward F.conv2d(x, Q(W), b, ...)
    (layers/binary_layers.py:105); backward = what autograd derives from F.conv2d plus the STE mask
    of the weight quantiser."""

    @staticmethod
    def forward(ctx, input, weight, bias, kind, weight_q, binary_input, conv_args):
        ctx.kind, ctx.conv_args, ctx.has_bias = kind, conv_args, bias is not None
        ctx.bias_dtype = bias.dtype if bias is not None else None
        ctx.save_for_backward(input, weight, weight_q)
        stride, padding, dilation, groups = conv_args
        # +-1 activation known without a device check (tag of a quantiser, or the layer's binary_input hint)?
        ctx.x_is_pm1 = bool(split_hint(binary_input)[0]) or (input.is_cuda and input.dtype in ops.PACK_DTYPES and input.dim() == 4
                                              and packed.lookup(input, packed.NHWC) is not None)
        clear_last_detection()
        out = quant_conv2d_forward(input, weight, bias, stride, padding, dilation, groups, kind,
                                   weight_q=weight_q, binary_input=binary_input, half_ok=True)
        if not ctx.x_is_pm1 and binary_input is None and input.is_cuda and input.dim() == 4:
            # un-tagged activation THIS forward detected as +-1 (e.g. behind a MaxPool2d): same knowledge for the backward
            ctx.x_is_pm1 = last_detection_said_pm1(input)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        from .common import ste_mask
        input, weight, weight_q = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conv_args
        grad_input = grad_weight = grad_bias = None
        in_dtype, w_dtype = input.dtype, weight.dtype
        if grad_output.is_cuda and grad_output.dtype in ops.HALF_DTYPES:
            # half model: the matrix-core routes contract the upcast operands (exact), their fp32 result is rounded once below
            grad_output, input, weight = grad_output.float(), input.float(), weight.float()
            weight_q = weight_q.float() if weight_q is not None else None
        go = _dense(grad_output)
        mfma = own_conv_backward(go, groups, padding, go.numel() * weight[0].numel())
        if ctx.needs_input_grad[0]:
            # real gradient x +-1 / 0 weight: the deterministic quantiser runs inside the operand pack; a stochastic draw was saved
            grad_input = conv_grad_input(input, weight if weight_q is None else weight_q, go, stride, padding, dilation, groups, W_PM1,
                                         quantiser=ctx.kind if weight_q is None else "sign", gate=mfma)
        want_bias = ctx.has_bias and ctx.needs_input_grad[2]
        bias_by_product = []              # filled by the weight-gradient route when its gradient pack can sum the channels on the way
        if ctx.needs_input_grad[1]:
            if mfma:     # +-1 activation (or the real-valued image of a first layer) x real gradient, contraction over the pixels;
                #          the STE mask of the weight quantiser comes back applied
                grad_weight = conv_grad_weight_routes(input, go, weight.shape, stride, padding, dilation,
                                                      X_PM1 if ctx.x_is_pm1 else X_REAL, weight=weight,
                                                      bias_grad=bias_by_product if want_bias else None)
            if grad_weight is None:
                gw = lib_conv2d_weight(input, weight.shape, go, stride, padding, dilation, groups)
                grad_weight = ste_mask(gw.contiguous(), weight)
        if want_bias:
            grad_bias = bias_by_product[0] if bias_by_product else go.sum((0, 2, 3))
        if grad_input is not None and grad_input.dtype != in_dtype:
            grad_input = grad_input.to(in_dtype)
        if grad_weight is not None and grad_weight.dtype != w_dtype:
            grad_weight = grad_weight.to(w_dtype)
        if grad_bias is not None and grad_bias.dtype != ctx.bias_dtype:
            grad_bias = grad_bias.to(ctx.bias_dtype)
        return grad_input, grad_weight, grad_bias, None, None, None, None


# ---- backward of the functional (fused Function) forms ------------------------------------------------------------------------------
# BinaryDense / BinaryConv2d() / TernaryDense / TernaryConv2d() / QuantDense / QuantConv2d / XNORDense / XNORConv2d write their
# backward by hand (functions/binary_connect.py:100-112,133-146, terner_connect.py:97-152, dorefa_connect.py:140-199,
# xnor_connect.py:118-168): two contractions per layer.  These helpers are the ONLY place a dense-library call (hipBLASLt GEMM,
# MIOpen backward conv) can come from, and every such call on a device tensor is counted in LIBRARY_PATHS — the functions
# themselves contain no `.mm(` / `torch.nn.grad.` (tests/test_layers_cpu.py greps for it).

def lib_mm(a: torch.Tensor, b: torch.Tensor, reason: str = "backward GEMM on the dense library") -> torch.Tensor:
    """a @ b on the dense library: host tensors (the reference expression itself), non-fp32 device tensors; counted for device
    tensors."""
    note_library_path(a, reason)
    return a.mm(b)


def lib_conv2d_input(input_shape, weight_q, grad_output, stride, padding, dilation, groups, reason="conv grad_input outside the matrix-core route"):
    note_library_path(grad_output, reason)
    return torch.nn.grad.conv2d_input(input_shape, weight_q, grad_output, stride=stride, padding=padding, dilation=dilation,
                                      groups=groups)


def lib_conv2d_weight(input, weight_shape, grad_output, stride, padding, dilation, groups, reason="conv grad_weight outside the matrix-core route"):
    note_library_path(grad_output, reason)
    return torch.nn.grad.conv2d_weight(input, weight_shape, grad_output, stride=stride, padding=padding, dilation=dilation,
                                       groups=groups)


def own_conv_backward(go: torch.Tensor, groups, padding, macs: Optional[int] = None) -> bool:
    """May the backward of a conv use this backend's own routes for the (dense) gradient ``go``?  The switch is on, a device fp32
    gradient, groups == 1, numeric zero padding.  ``macs``: the multiply-accumulates of the contraction, held against
    BWD_MFMA_MIN_MACS (the autograd nodes of the layers); the functional forms leave it out and ask for a non-empty gradient."""
    return bool(_cfg("BWD_CONV_MFMA") and go.is_cuda and go.dtype == torch.float32 and groups == 1 and not isinstance(padding, str)
                and (macs is None or macs >= _cfg("BWD_MFMA_MIN_MACS")))


#: what the activation of a weight gradient holds (``conv_grad_weight_routes``): +-1 / 0; a k-bit DoReFa image q / n (with
#: ``x_levels`` = n; also its bare digits, n = 1); Lin / Log levels, exact in bf16 (always with ``terms`` = 3); a real-valued image
X_PM1, X_CODES, X_LEVELS, X_REAL = "pm1", "codes", "levels", "real"


def conv_grad_weight_routes(input, go, weight_shape, stride, padding, dilation, x_kind, x_levels: float = 1.0,
                            terms: Optional[int] = None, weight: Optional[torch.Tensor] = None,
                            ste_threshold: float = ops.STE_THRESHOLD, bias_grad: Optional[list] = None,
                            layout_like: Optional[torch.Tensor] = None, any_channels: bool = False, taken: Optional[list] = None):
    """THE ladder of this backend's weight-gradient routes: grad wrt the weight of conv2d(x, .) for the dense fp32 gradient ``go``
    on the first rung whose predicate holds and that returns a result (a rung returns None when its launch plan does not fit the
    byte budget); None when no rung does — the caller uses the library.  The gate (``own_conv_backward``) is the caller's.

    ``x_kind``: X_PM1 / X_CODES / X_LEVELS / X_REAL.  ``terms``: the split of the gradient on the pixel-major kernel — None =
    FLOAT_SPLIT, or pinned to 2 / 3.  ``weight``: the result comes back with the quantiser's straight-through mask
    1[|W| <= ste_threshold] applied, otherwise un-masked (the XNOR-Net combination, DoReFa's and Lin / Log's identity STE).
    ``bias_grad``: a list that receives the bias gradient when the gradient pack of the rung can sum the channels on the way.
    ``layout_like``: the parameter — the result takes its memory format where the rung can write it.  ``any_channels``: a
    real-valued activation of any width may run (channel groups of the pixel-major kernel, else one six-term GEMM per tap).
    ``taken``: a list that receives the name of the rung that produced the result (tools/bench_conv_backward.py)."""
    ksz = weight_shape[2:]
    xs, gs = input.shape, go.shape
    gw, rung, masked = None, None, True
    if x_kind != X_REAL:
        if ops.wgrad_pm_applicable(xs, gs, ksz, stride, dilation):
            # pixel-major kernel: every tap of a tile in one workgroup; STE mask and bias gradient in its own launches
            rung = "pm"
            gw = ops.conv2d_grad_weight_pm(input, go, ksz, padding, weight=weight, ste_threshold=ste_threshold, x_levels=x_levels,
                                           bias_grad=bias_grad, terms=terms, layout_like=layout_like)
        # terms pinned to 2: the activation needs the pixel-major kernel's fp16 plane (DoReFa codes beyond +-256), so no rung
        # that stores it as bf16 — the K-major GEMMs, the strided 1 x 1 form
        if gw is None and terms != 2 and ops.wgrad_gemm_applicable(xs, gs, ksz, stride, dilation):
            # batched bf16 GEMMs over K-major planes (other kernel sizes); STE mask in the reduce step
            rung = "gemm"
            gw = ops.conv2d_grad_weight_gemm(input, go, ksz, padding, weight=weight, ste_threshold=ste_threshold, x_levels=x_levels)
        # terms pinned to 3: not the strided k x k form — it runs the pixel-major kernel with the split FLOAT_SPLIT names (and gets
        # no ``bias_grad``: it never did)
        if (gw is None and terms != (2 if int(ksz[0]) == 1 else 3)
                and ops.wgrad_strided_applicable(xs, gs, ksz, stride, padding, dilation)):
            # strided convs (ResNet stage transitions): 1x1 -> GEMM over the sub-sampled positions, k x k -> the pixel-major
            # kernel on the space-to-depth image
            rung, masked = "strided", False
            gw = ops.conv2d_grad_weight_strided(input, go, ksz, stride, padding, x_levels=x_levels, layout_like=layout_like)
        if gw is None and x_kind == X_PM1:
            # the older swapped conv packs sign(x): +-1 / 0 only; it tests its own shapes
            rung, masked = "swapped", False
            gw = ops.conv2d_grad_weight_pm1(input, go, ksz, stride, padding, dilation)
    else:
        few = ops.wgrad_s2d_applicable(xs, ksz, stride, dilation)
        if few or (any_channels and ops.wgrad_s2d_applicable(xs, ksz, stride, dilation, True)):
            # a real-valued image — few channels (first layers, any stride), or any width at stride 1: space-to-depth + the
            # pixel-major kernel, the image's terms as channel groups
            rung = "s2d"
            gw = ops.conv2d_grad_weight_s2d(input, go, weight_shape, stride, padding, weight=weight, ste_threshold=ste_threshold,
                                            bias_grad=bias_grad, any_channels=not few)
    if gw is None and any_channels:
        rung, masked = "taps", False
        gw = real_conv_grad_weight_taps(input, go, weight_shape, stride, padding, dilation)
    if gw is None:
        return None
    if weight is not None and not masked:
        from .common import ste_mask
        gw = ste_mask(gw.contiguous(), weight, ste_threshold)
    if taken is not None:
        taken.append(rung)
    return gw


#: the weight of an input gradient (``conv_grad_input_routes``): +-1 / 0, or the latent weight with its ``quantiser``; levels x
#: ``out_scale``; ``operand`` = the packed Lin / Log grad_x planes; sign(W) with ``operand`` = XNOR-Net's TapScales.bwd; real-valued
W_PM1, W_LEVELS, W_PACKED, W_TAPS, W_REAL = "pm1", "levels", "packed", "taps", "real"


def conv_grad_input_routes(input, weight, go, stride, padding, dilation, w_kind, quantiser: str = "sign", out_scale: float = 1.0,
                           out_scale_dev: Optional[torch.Tensor] = None, operand=None, taken: Optional[list] = None):
    """THE ladder of this backend's input-gradient routes: grad wrt the input of conv2d(x, Q(weight)) for the dense fp32 gradient
    ``go`` as the stride-1 conv of ``ops.grad_input_operand`` with the flipped, transposed weight, on the rung ``w_kind`` names
    (W_PM1 / W_LEVELS / W_PACKED: the exact-split conv, W_TAPS: the per-tap scaled fp16 conv, W_REAL: the six-term real one); None
    outside ``ops.grad_input_route_applicable`` or when the rung returns None — library and gate are the caller's.  A channels-last
    view, copied for an ``input`` in NCHW storage by W_PACKED and W_REAL.  ``taken``: receives the rung's name (q / taps / real)."""
    gx = None
    if w_kind in (W_PM1, W_LEVELS, W_PACKED):     # W_PACKED: three exact terms of g; ``weight`` only gives the shape
        gx = ops.conv2d_grad_input_q(input.shape, weight, go, stride, padding, dilation, kind=quantiser if w_kind == W_PM1 else "raw",
                                     out_scale=out_scale, out_scale_dev=out_scale_dev, terms=3 if w_kind == W_PACKED else None,
                                     weight_triples=operand)
        if w_kind == W_PACKED and gx is not None and input.is_contiguous() and not input.is_contiguous(memory_format=torch.channels_last):
            gx = gx.contiguous()          # (as ``nchw_result`` below)
    elif w_kind == W_TAPS:
        gx = ops.conv2d_grad_input_taps(input.shape, weight, go, operand, stride, padding, dilation)
    elif ops.grad_input_route_applicable(weight.shape, stride, padding, dilation):
        wt = weight.detach().flip(2, 3).transpose(0, 1).contiguous()
        op = ops.grad_input_operand(go, input.shape, weight.shape, stride, padding, dilation)
        y2 = ops.real_conv2d(op[0], wt, None, 1, op[1], 1) if op is not None else None
        if y2 is not None:
            gx = nchw_result(y2, input, *(int(input.shape[i]) for i in (0, 2, 3, 1)))
    if gx is not None and taken is not None:
        taken.append({W_TAPS: "taps", W_REAL: "real"}.get(w_kind, "q"))
    return gx


def _hip2d(*ts) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.numel() > 0 for t in ts)


def known_pm1(input: torch.Tensor, weight: Optional[torch.Tensor], layout) -> bool:
    """Is this device activation exactly +-1?  The tag of a quantiser (BinaryConnect) answers without a device check; otherwise
    the detection the layers use (one read of the tensor; negative verdicts are remembered per weight)."""
    if not (isinstance(input, torch.Tensor) and input.is_cuda and input.dtype == torch.float32 and input.numel() > 0):
        return False
    if packed.lookup(input, layout) is not None:
        return True
    return bool(_cfg("DETECT_BINARY_INPUT") and detect_pm1(input, weight)[0])


def real_matmul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [M, J] @ b [J, K] for two REAL device matrices on the bf16 matrix cores (six-term planes, fp32-GEMM accuracy); host /
    non-fp32 tensors: the library."""
    if _hip2d(a, b):
        return ops.real_linear(a.contiguous(), b.t().contiguous())
    return lib_mm(a, b)


def dense_grad_input(grad_output: torch.Tensor, weight_q: torch.Tensor, pm1: bool) -> torch.Tensor:
    """g . weight_q for the quantised image the forward multiplied with: +-1 / 0 images (``pm1``) through the exact split of g
    against the replicated image, real-valued images (DoReFa levels, sign(W) * E) through the six-term real x real route."""
    if _hip2d(grad_output, weight_q):
        g2 = grad_output.contiguous()
        if pm1:
            return ops.float_linear(g2, weight_q.t().contiguous(), "sign")
        return ops.real_linear(g2, weight_q.t().contiguous())
    return lib_mm(grad_output, weight_q)


def dense_grad_weight(grad_output: torch.Tensor, input: torch.Tensor, x_is_pm1: bool) -> torch.Tensor:
    """g^T . x: a +-1 activation is the exact operand (rows of g^T are output features: three exact bf16 terms); two real operands
    take the six-term route."""
    if _hip2d(grad_output, input):
        gt = grad_output.t().contiguous()
        if x_is_pm1:
            return ops.float_linear(gt, input.t().contiguous(), "sign", terms=3)
        return ops.real_linear(gt, input.t().contiguous())
    return lib_mm(grad_output.t(), input)


def conv_grad_input(input, weight, grad_output, stride, padding, dilation, groups, w_kind, quantiser: str = "sign",
                    out_scale: float = 1.0, out_scale_dev=None, operand=None, gate: Optional[bool] = None, lib_weight=None):
    """grad wrt the input of conv2d(x, Q(weight)) on ``conv_grad_input_routes`` behind ``gate`` (None: the functional forms' —
    ``own_conv_backward`` and a non-empty gradient); ``w_kind`` None (a real-valued image, DoReFa at 8 < k <= 32), a closed gate
    or no answer: the library, counted, on ``lib_weight()`` (default: the quantised ``weight`` times the scales), built only then."""
    go = _dense(grad_output)
    if gate is None:
        gate = own_conv_backward(go, groups, padding) and go.numel() > 0
    if gate and w_kind is not None:
        gx = conv_grad_input_routes(input, weight, go, stride, padding, dilation, w_kind, quantiser, out_scale, out_scale_dev, operand)
        if gx is not None:
            return gx
    wq = lib_weight() if lib_weight is not None else \
        quantize_weight_f32(weight, quantiser) if quantiser in ("binary", "ternary") else weight
    if lib_weight is None and (out_scale_dev is not None or out_scale != 1.0):
        wq = wq * (float(out_scale) if out_scale_dev is None else out_scale_dev * float(out_scale))
    return lib_conv2d_input(input.shape, wq, grad_output, stride, padding, dilation, groups)


def conv_grad_weight(input, weight_shape, grad_output, stride, padding, dilation, groups, x_is_pm1: bool, bias_by_product=None,
                     real_any_channels: bool = False, x_exact_bf16: bool = False):
    """UN-masked grad wrt the weight of conv2d(x, .) on ``conv_grad_weight_routes``: +-1 activations, a real-valued image with few
    channels (first layers) or, with ``real_any_channels``, of any geometry; anything else on the library, counted.
    ``x_exact_bf16``: the activation holds Lin / Log levels — first the rungs that store it as bf16_rn(x), with the gradient in
    three exact bf16 terms (the pixel-major kernel's fp16 planes are out: Log levels reach 2^-126), then the real-valued ones."""
    go = _dense(grad_output)
    if own_conv_backward(go, groups, padding) and go.numel() > 0 and input.dtype == torch.float32:
        gw = None
        if x_exact_bf16:
            gw = conv_grad_weight_routes(input, go, weight_shape, stride, padding, dilation, X_LEVELS, terms=3)
        if gw is None:
            gw = conv_grad_weight_routes(input, go, weight_shape, stride, padding, dilation, X_PM1 if x_is_pm1 else X_REAL,
                                         bias_grad=bias_by_product, any_channels=real_any_channels)
        if gw is not None:
            return gw
    return lib_conv2d_weight(input, weight_shape, grad_output, stride, padding, dilation, groups)


def real_conv_grad_weight_taps(input, go, weight_shape, stride, padding, dilation):
    """grad wrt the weight of conv2d(x, .) for two REAL operands of any geometry (groups == 1), one six-term real x real GEMM per
    filter tap on the bf16 matrix cores:  dW[:, :, i, j] = G^T . X_ij  with G [n ho wo, Cout] the gradient and X_ij [n ho wo, Cin] the
    tap-shifted, strided view of the zero-padded input.  The general fallback of the real-valued layers (DoReFa at 8 < k <= 32, the
    quantised input of XNORConv2d) where the pixel-major kernel's geometry (stride 1, 3 x 3 / 5 x 5) does not apply: kh * kw launches
    of K = N Ho Wo, fp32-GEMM accuracy, no dense library.  None for host tensors / empty operands."""
    if not (go.is_cuda and input.is_cuda and go.dtype == torch.float32 and input.dtype == torch.float32 and go.numel() > 0
            and input.numel() > 0):
        return None
    Cout, Cin, kh, kw = (int(v) for v in weight_shape)
    (sh, sw), (ph, pw), (dh, dw) = ops._pairs(stride), ops._pairs(padding), ops._pairs(dilation)
    N_, _, Ho, Wo = (int(v) for v in go.shape)
    x = input.detach()
    if ph or pw:
        x = F.pad(x, (pw, pw, ph, ph))
    g2t = go.detach().permute(1, 0, 2, 3).reshape(Cout, -1).contiguous()                 # [Cout, n ho wo]
    gw = torch.empty((Cout, Cin, kh, kw), dtype=torch.float32, device=go.device)
    for i in range(kh):
        for j in range(kw):
            xs = x[:, :, i * dh:i * dh + sh * (Ho - 1) + 1:sh, j * dw:j * dw + sw * (Wo - 1) + 1:sw]
            x2t = xs.permute(1, 0, 2, 3).reshape(Cin, -1).contiguous()                   # [Cin, n ho wo]
            gw[:, :, i, j] = ops.real_linear(g2t, x2t)                                    # G^T . X_ij  = g2t . x2t^T
    return gw


# ---- XNOR-Net family (functions/xnor_connect.py:93-169, layers/xnor_layers.py) ------------------------------------------------------

def xnor_conv_fast_applicable(input, weight, dim, groups, padding) -> bool:
    """The per-tap scaled route: device fp32 NCHW input, groups == 1, numeric zero padding, and the scale reduced over exactly the
    first two weight dimensions (``dim`` = [0, 1], the default of the layer, the converter and the function: one alpha per tap)."""
    return (isinstance(input, torch.Tensor) and input.is_cuda and input.dtype == torch.float32 and input.dim() == 4
            and input.numel() > 0 and weight.dtype == torch.float32 and weight.dim() == 4 and groups == 1
            and not isinstance(padding, str) and not isinstance(dim, int) and sorted(int(d) for d in dim) == [0, 1])


def xnor_conv2d_forward(input, weight, bias, stride, padding, dilation, binary_input=None, planes=None, epi=None):
    """conv2d(x, sign(W) * alpha[1, 1, kh, kw]) for a +-1 activation on the fp4 matrix cores with per-tap scaling
    (qt_conv2d_implicit_taps).  ``planes`` = (weight nibble planes, TapScales) cached by an eval-mode layer.
    Returns (result, TapScales, pixel words per channel) with result = the NHWC fp32 matrix [N*Ho*Wo, Cout] (or the epilogue's
    planes), or None when the activation is not +-1 / the shape is outside the kernel's limits (the caller takes the real x real
    route)."""
    px, flag = _pixel_planes(input, binary_input, weight, ld_fn=ops.pixel_ld_nib_taps)
    if px is None:
        return None
    if planes is not None:
        wp, taps = planes
    else:
        taps = ops.xnor_tap_prep(weight)
        wp = ops.pack_conv_weight_nib(weight.detach(), "sign", cw=px.ld)
    N, C, H, W = (int(v) for v in input.shape)
    kh, kw = int(weight.shape[2]), int(weight.shape[3])
    b = poison_bias(bias.detach() if bias is not None else None, flag, int(weight.shape[0]), input.device)
    y2 = ops.conv2d_nib_taps(px, (N, C, H, W), wp, (kh, kw), taps.fwd, b, stride, padding, dilation, epi=epi)
    if y2 is None:
        return None
    return y2, taps


def xnor_weight_grad(gw: torch.Tensor, weight: torch.Tensor, mean: torch.Tensor, reduce_dim=0) -> torch.Tensor:
    """mean * gw + sign(W) * mean(gw * sign(W), DIM, keepdim) (functions/xnor_connect.py:126-127, 158-159; DIM = 0 upstream)."""
    sgn = torch.sign(weight)
    return mean * gw + sgn * torch.mean(gw * sgn, reduce_dim, keepdim=True)


def _dorefa_w1_scale(weight: torch.Tensor, prequantized: bool) -> torch.Tensor:
    """E of the 1-bit DoReFa weight sign(W)*E as a device scalar.  Training: E = mean|W|
    (functions/dorefa_connect.py:100).  Eval: the weight already holds sign(W)*E, so |w| == E for
    every entry and amax recovers it exactly."""
    return weight.detach().abs().amax() if prequantized else ops.abs_mean(weight)


def dorefa_w1_linear_forward(input, weight, bias, prequantized: bool, weight_codes=None, scale=None,
                             route: Optional[list] = None):
    """LinearDorefa(bit_width=1).forward on a device tensor (layers/dorefa_layers.py:41-45):
    y = x . (sign(W)*E)^T + b.  If the activation carries k-bit DoReFa codes (nnDorefaQuant output)
    the contraction runs on the int8 matrix cores: y = (E/n) * sum q*s + b; otherwise the dense GEMM
    library on the HIP-quantised weight image."""
    E = scale if scale is not None else _dorefa_w1_scale(weight, prequantized)
    K, N = input.shape[-1], weight.shape[0]
    if isinstance(input, packed.CodeActivation):
        codes = input.codes
        if len(input.shape) != 2 or codes.K != K or 127 * K >= (1 << 24):
            raise ValueError(f"CodeActivation {input.shape} does not fit LinearDorefa({K}, {N})")
        wc = weight_codes if weight_codes is not None else ops.weight_codes(weight.detach().reshape(N, -1))
        y = ops.i8_gemm(codes, wc, codes.inv_n, bias, scale_dev=E)
        y._qt_overflow = codes.overflow
        return y
    codes = packed.lookup_codes(input, packed.ROWS_LAST) if input.dtype == torch.float32 else None
    if codes is not None and codes.K == K and codes.rows * K == input.numel() and 127 * K < (1 << 24):
        ok, flag = codes_route(codes, weight)
        if ok:
            wc = weight_codes if weight_codes is not None else ops.weight_codes(weight.detach().reshape(N, -1))
            y = ops.i8_gemm(codes, wc, codes.inv_n, poison_bias(bias, flag, N, input.device), scale_dev=E)
            if route is not None:
                route.append("codes")
            return y.view(*input.shape[:-1], N)
    if _cfg("FLOAT_PATH") == "bf16x3" and input.dtype == torch.float32 and input.numel() > 0:
        # no usable int8 codes: exact bf16 split of the activation x sign(W) on the bf16 matrix cores, E and bias after
        y = ops.float_linear(input.detach(), weight.detach(), "binary") * E
        if bias is not None:
            y = y + bias.detach()
        if route is not None:
            route.append("split")
        return y
    wq = weight if prequantized else quantize_weight_f32(weight.detach(), "binary") * E
    note_library_path(input, "DoReFa activation without usable int8 codes")
    if route is not None:
        route.append("library")
    return F.linear(input, wq, bias)


def dorefa_w1_conv_forward(input, weight, bias, conv_args, prequantized: bool, weight_codes=None,
                           padding_mode: str = "zeros", scale=None, epi=None, route: Optional[list] = None):
    """DorefaConv2d(bit_width=1).forward on a device tensor (layers/dorefa_layers.py:77-82).  ``route``: a list that
    receives "codes" (int8 matrix cores on the activation's codes), "split" (exact bf16 split of a real-valued — or
    int8-overflowing — activation x sign(W), scaled by E) or "library"."""
    stride, padding, dilation, groups = conv_args
    E = scale if scale is not None else _dorefa_w1_scale(weight, prequantized)
    if isinstance(input, packed.CodeActivation):
        # fused inference: the activation exists only as codes (range checked once, at the end of the network)
        codes = input.codes
        N_, C, H, W = input.shape
        kh, kw = int(weight.shape[2]), int(weight.shape[3])
        if (groups != 1 or padding_mode != "zeros" or isinstance(padding, str) or codes.K != C
                or C != weight.shape[1] or 127 * kh * kw * codes.codes.shape[1] >= (1 << 24)):
            raise ValueError(f"CodeActivation {input.shape} does not fit this DorefaConv2d")
        wc = weight_codes if weight_codes is not None else ops.pack_conv_weight_codes(weight.detach())
        if epi is not None and epi.overflow is None:
            epi.overflow = codes.overflow
        if epi is not None and ops.direct_conv3x3_codes_applicable(C, int(weight.shape[0]), (kh, kw), stride, padding,
                                                                   dilation, input.halo, epi):
            y2 = ops.conv3x3_direct_codes(codes, N_, C, H, W, wc, codes.inv_n, bias, E, epi)
            return packed.CodeActivation(y2, (N_, weight.shape[0], H, W), halo=(1, 1))
        y2 = ops.conv2d_codes(codes, (N_, C, H, W), wc, (kh, kw), codes.inv_n, bias, stride, padding, dilation,
                              scale_dev=E, epi=epi, in_halo=input.halo)
        Ho, Wo = ops.conv_out_hw(H, W, kh, kw, stride, padding, dilation)
        if epi is not None:
            return packed.CodeActivation(y2, (N_, weight.shape[0], Ho, Wo), halo=epi.out_halo)
        y = y2.view(N_, Ho, Wo, weight.shape[0]).permute(0, 3, 1, 2)
        y._qt_overflow = codes.overflow          # the chain's range flag rides on to the next fused quantiser
        return y
    if epi is not None:
        raise TypeError("the code epilogue takes a CodeActivation input")
    codes = None
    if (input.dtype == torch.float32 and input.dim() == 4 and groups == 1 and padding_mode == "zeros"
            and not isinstance(padding, str)):
        codes = packed.lookup_codes(input, packed.NHWC)
    if codes is not None:
        N_, C, H, W = input.shape
        kh, kw = int(weight.shape[2]), int(weight.shape[3])
        Kb = kh * kw * codes.codes.shape[1]
        ok, flag = codes_route(codes, weight) if (codes.K == C and codes.rows == N_ * H * W and 127 * Kb < (1 << 24)) else (False, None)
        if ok:
            wc = weight_codes if weight_codes is not None else ops.pack_conv_weight_codes(weight.detach())
            y2 = ops.conv2d_codes(codes, (N_, C, H, W), wc, (kh, kw), codes.inv_n,
                                  poison_bias(bias, flag, int(weight.shape[0]), input.device), stride, padding,
                                  dilation, scale_dev=E)
            Ho, Wo = ops.conv_out_hw(H, W, kh, kw, stride, padding, dilation)
            if route is not None:
                route.append("codes")
            return y2.view(N_, Ho, Wo, weight.shape[0]).permute(0, 3, 1, 2)   # channels_last like the input
    if (_cfg("FLOAT_PATH") == "bf16x3" and input.dtype == torch.float32 and input.dim() == 4 and input.numel() > 0 and groups == 1
            and padding_mode == "zeros" and not isinstance(padding, str)):
        # no int8 codes (an un-quantised input, or the un-clamped quantiser left the int8 range): the activation is a real
        # number for the matrix cores — exact bf16 split x sign(W), E and the bias applied to the result
        N_, _, H, W = input.shape
        kh, kw = int(weight.shape[2]), int(weight.shape[3])
        Ho, Wo = ops.conv_out_hw(H, W, kh, kw, stride, padding, dilation)
        y2 = ops.float_conv2d(input.detach(), weight.detach(), "binary", bias.detach() if bias is not None else None, stride,
                              padding, dilation, out_scale_dev=E)
        y = nchw_result(y2, input, N_, Ho, Wo, weight.shape[0])
        if route is not None:
            route.append("split")
        return y
    wq = weight if prequantized else quantize_weight_f32(weight.detach(), "binary") * E
    note_library_path(input, "DoReFa activation without usable int8 codes")
    if route is not None:
        route.append("library")
    return F.conv2d(input, wq, bias, stride, padding, dilation, groups)


def _inv_levels(bit_width: int) -> float:
    """fl32(1 / (2^k - 1)) as _quantize forms it (functions/dorefa_connect.py:24)."""
    n = float((1 << int(bit_width)) - 1)
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(n, dtype=torch.float32))


def dorefa_wk_linear_forward(input, weight_q, bias, bit_width: int, weight_codes):
    """Eval-mode LinearDorefa(bit_width = k, 2 <= k <= 7) on a device activation that carries DoReFa codes:
    with x = q / n_a and w_q = c / n_w (c = odd integer level, functions/dorefa_connect.py:108-112)
        y = (1 / (n_a n_w)) * sum q c + b
    on the int8 matrix cores (int32 accumulate).  The reference sums fl(x) * fl(w_q) in fp32, so parity is the
    float-tail tolerance, not bit equality.  Returns None when the activation has no usable codes."""
    codes = packed.lookup_codes(input, packed.ROWS_LAST) if input.dtype == torch.float32 else None
    K, N = input.shape[-1], weight_q.shape[0]
    n_w = (1 << int(bit_width)) - 1
    if codes is None or codes.K != K or codes.rows * K != input.numel() or 127 * n_w * K >= (1 << 31):
        return None
    ok, flag = codes_route(codes, weight_q)
    if not ok:
        return None
    y = ops.i8_gemm(codes, weight_codes, codes.inv_n * _inv_levels(bit_width), poison_bias(bias, flag, N, input.device),
                    max_abs_code=127 * n_w)
    return y.view(*input.shape[:-1], N)


def dorefa_wk_conv_forward(input, weight_q, bias, conv_args, bit_width: int, weight_codes, padding_mode="zeros"):
    """Eval-mode DorefaConv2d(bit_width = k, 2 <= k <= 7) on a code-carrying activation; see
    dorefa_wk_linear_forward.  Returns None when the packed path does not apply."""
    stride, padding, dilation, groups = conv_args
    if not (input.dtype == torch.float32 and input.dim() == 4 and groups == 1 and padding_mode == "zeros"
            and not isinstance(padding, str)):
        return None
    codes = packed.lookup_codes(input, packed.NHWC)
    if codes is None:
        return None
    N_, C, H, W = input.shape
    kh, kw = int(weight_q.shape[2]), int(weight_q.shape[3])
    Kb = kh * kw * codes.codes.shape[1]
    n_w = (1 << int(bit_width)) - 1
    if codes.K != C or codes.rows != N_ * H * W or 127 * n_w * Kb >= (1 << 31):
        return None
    ok, flag = codes_route(codes, weight_q)
    if not ok:
        return None
    y2 = ops.conv2d_codes(codes, (N_, C, H, W), weight_codes, (kh, kw), codes.inv_n * _inv_levels(bit_width),
                          poison_bias(bias, flag, int(weight_q.shape[0]), input.device),
                          stride, padding, dilation, max_abs_code=127 * n_w)
    Ho, Wo = ops.conv_out_hw(H, W, kh, kw, stride, padding, dilation)
    return y2.view(N_, Ho, Wo, weight_q.shape[0]).permute(0, 3, 1, 2)   # channels_last like the input


#: k-bit DoReFa weights whose integer levels c = (2^k - 1) w_q (odd, |c| <= 2^k - 1) are exact in BOTH split formats (bf16: 8
#: significant bits, fp16: 11): the level image is the exact operand of the real-activation routes up to this bit width
LEVEL_MAX_BITS = 8
#: ... and fit the int8 matrix cores (|c| <= 127) up to this one
LEVEL_INT8_BITS = 7


def dorefa_levels_conv_forward(input, weight_q, bias, conv_args, bit_width: int, level_planes=None):
    """conv2d(x, w_q, b) for a k-bit DoReFa weight image w_q = c / n_w (2 <= k <= LEVEL_MAX_BITS) and ANY fp32 activation —
    real-valued, or a k-bit image whose codes left the int8 range, or 8-bit weights whose levels do not fit int8: the split
    activation x the exact level image on the matrix cores, 1 / n_w and the bias in the epilogue
    (layers/dorefa_layers.py:77-82).  Returns None outside the route's limits (groups, padding mode, empty)."""
    stride, padding, dilation, groups = conv_args
    if not (input.is_cuda and input.dim() == 4 and input.dtype == torch.float32 and groups == 1 and not isinstance(padding, str)
            and input.numel() > 0 and 2 <= int(bit_width) <= LEVEL_MAX_BITS):
        return None
    N_, _, H, W = input.shape
    Ho, Wo = ops.conv_out_hw(H, W, int(weight_q.shape[2]), int(weight_q.shape[3]), stride, padding, dilation)
    y2 = ops.float_conv2d(input.detach(), _weight_levels(weight_q, bit_width), "raw",
                          bias.detach() if bias is not None else None, stride, padding, dilation,
                          weight_triples=level_planes, out_scale=_inv_levels(bit_width))
    return nchw_result(y2, input, N_, Ho, Wo, weight_q.shape[0])


def dorefa_levels_linear_forward(input, weight_q, bias, bit_width: int, level_planes=None):
    """The dense twin of dorefa_levels_conv_forward (layers/dorefa_layers.py:41-45)."""
    if not (input.is_cuda and input.dtype == torch.float32 and input.numel() > 0 and 2 <= int(bit_width) <= LEVEL_MAX_BITS):
        return None
    y = ops.float_linear(input.detach(), _weight_levels(weight_q, bit_width), "raw", weight_triples=level_planes) * _inv_levels(bit_width)
    if bias is not None:
        y = y + bias.detach()
    return y


def _levels_grad_weight_linear(g2, x2, x_levels, codes_fit: bool):
    """g2^T . x2 for a k-bit image x2 = q / n: codes (or their 256-digits when they left int8) as the exact bf16 operand."""
    inv = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(x_levels), dtype=torch.float32))
    q = torch.round(x2.detach() * float(x_levels))
    # three exact bf16 terms: a row of g2^T is ONE output feature's gradient (the two-term form's scale is per tensor)
    gT = ops.split_bf16x3(g2.t().contiguous(), terms=3)
    if codes_fit:
        return ops.bf16_gemm(gT, ops.weight_bf16x3(q.t().contiguous(), "raw", terms=3)) * inv
    hi = torch.floor(q * (1.0 / 256.0))
    lo = q - hi * 256.0
    bad = torch.where(hi.abs().amax() >= 256.0, float("nan"), 0.0)
    return (ops.bf16_gemm(gT, ops.weight_bf16x3(hi.t().contiguous(), "raw", terms=3)) * 256.0
            + ops.bf16_gemm(gT, ops.weight_bf16x3(lo.t().contiguous(), "raw", terms=3))) * inv + bad


class DorefaW1LinearFn(QtFunction):
    """Training-mode LinearDorefa(bit_width=1): forward above; backward as autograd derives it from
    F.linear(x, _ignore_factor_op(sign(W), E), b): grad_x = g . (sign(W) E), grad_W = g^T . x passed
    through UNscaled (functions/dorefa_connect.py:66-79) with the identity STE of the quantiser.  From 2^27 MACs on both
    GEMMs run on the bf16 matrix cores (g split exactly, sign(W) / the activation's codes as the exact operand)."""

    @staticmethod
    def forward(ctx, input, weight, bias):
        ctx.has_bias = bias is not None
        ctx.save_for_backward(input, weight)
        ctx.x_levels = _act_levels(input, packed.ROWS_LAST) if input.dim() >= 2 else None
        route = []
        y = dorefa_w1_linear_forward(input, weight, bias, prequantized=False, route=route)
        ctx.codes_fit = route == ["codes"]
        return y

    @staticmethod
    def backward(ctx, grad_output):
        input, weight = ctx.saved_tensors
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        x2 = input.reshape(-1, input.shape[-1])
        grad_input = grad_weight = grad_bias = None
        big = (g2.is_cuda and g2.dtype == torch.float32 and g2.numel() > 0 and g2.shape[0] * g2.shape[1] * x2.shape[1] >= _cfg("BWD_MFMA_MIN_MACS"))
        if ctx.needs_input_grad[0]:
            sgn = quantize_weight_f32(weight, "binary")
            E = ops.abs_mean(weight)
            if big:
                grad_input = (ops.float_linear(g2.contiguous(), sgn.t().contiguous(), "sign") * E).view(input.shape)
            else:
                grad_input = lib_mm(g2, sgn * E).view(input.shape)
        if ctx.needs_input_grad[1]:
            if big and ctx.x_levels is not None:
                grad_weight = _levels_grad_weight_linear(g2, x2, ctx.x_levels, ctx.codes_fit)
            if grad_weight is None:
                grad_weight = real_matmul(g2.t(), x2) if big else lib_mm(g2.t(), x2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = g2.sum(0)
        return grad_input, grad_weight, grad_bias


class DorefaW1Conv2dFn(QtFunction):
    """Training-mode DorefaConv2d(bit_width=1); see DorefaW1LinearFn."""

    @staticmethod
    def forward(ctx, input, weight, bias, conv_args):
        ctx.has_bias, ctx.conv_args = bias is not None, conv_args
        ctx.save_for_backward(input, weight)
        # k-bit activation with valid int8 codes (the tag nnDorefaQuant leaves): its image is codes / (2^k - 1), so the
        # weight gradient can contract the integer codes on the bf16 matrix cores
        ctx.x_levels, ctx.code_flag = None, None
        if input.is_cuda and input.dtype == torch.float32 and input.dim() == 4:
            codes = packed.lookup_codes(input, packed.NHWC)
            if codes is not None and codes.K == input.shape[1]:
                ctx.x_levels = float((1 << int(codes.bit_width)) - 1)
                ctx.code_flag = codes.overflow
        route = []
        ctx.E = _dorefa_w1_scale(weight, False) if input.is_cuda else None     # mean|W|: the backward scales grad_x by it again
        y = dorefa_w1_conv_forward(input, weight, bias, conv_args, prequantized=False, route=route, scale=ctx.E)
        ctx.codes_fit = route == ["codes"]
        return y

    @staticmethod
    def backward(ctx, grad_output):
        input, weight = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conv_args
        go = _dense(grad_output)
        grad_input = grad_weight = grad_bias = None
        mfma = own_conv_backward(go, groups, padding, go.numel() * weight[0].numel())
        if ctx.needs_input_grad[0]:
            E = ctx.E if ctx.E is not None else ops.abs_mean(weight)
            # g * (sign(W) E) = E * (g * sign(W)): the exact-split conv on the flipped +-1 weight, scaled after
            grad_input = conv_grad_input(input, weight, go, stride, padding, dilation, groups, W_PM1, quantiser="binary", out_scale_dev=E,
                                         gate=mfma, lib_weight=lambda: quantize_weight_f32(weight, "binary") * E)
        if ctx.needs_input_grad[1]:
            if mfma and ctx.x_levels is not None and ctx.x_levels <= 255:
                # UNscaled and un-masked, as upstream (_ignore_factor_op, identity STE): functions/dorefa_connect.py:66-79
                grad_weight = dorefa_conv_grad_weight(input, go, weight.shape, stride, padding, dilation, ctx.x_levels,
                                                      ctx.codes_fit, ctx.code_flag, layout_like=weight)
            if grad_weight is None:
                grad_weight = lib_conv2d_weight(input, weight.shape, go, stride, padding, dilation, groups)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = go.sum((0, 2, 3))
        return grad_input, grad_weight, grad_bias, None


def _weight_levels(weight_q: torch.Tensor, bit_width: int) -> torch.Tensor:
    """Integer levels c = rint((2^k - 1) * w_q) of a k-bit DoReFa weight image (odd integers, |c| <= 2^k - 1 <= 127: exact
    in bf16 and in int8), as an fp32 tensor shaped like w_q."""
    return torch.round(weight_q.detach() * float((1 << int(bit_width)) - 1))


def _act_levels(t: torch.Tensor, layout):
    """n = 2^k - 1 of a k-bit DoReFa activation that carries valid int8 codes (the tag nnDorefaQuant leaves), else None."""
    if t.is_cuda and t.dtype == torch.float32:
        codes = packed.lookup_codes(t, layout)
        if codes is not None and codes.K == t.shape[1 if layout is packed.NHWC else -1]:
            n = float((1 << int(codes.bit_width)) - 1)
            return n if n <= 255 else None
    return None


def dorefa_conv_grad_weight(input, go, weight_shape, stride, padding, dilation, x_levels: float, codes_fit: bool, code_flag=None,
                            layout_like=None):
    """grad wrt the (quantised) weight of a DoReFa conv whose activation is a k-bit image q / n (n = ``x_levels``): the
    integer codes q are exact in bf16 while |q| <= 256, so the contraction runs on the weight-gradient routes (pixel-major,
    K-major, strided) with the split gradient.  ``codes_fit`` False — the un-clamped quantiser left the int8 range
    (functions/dorefa_connect.py:11-25 has no clamp):
      * pixel-major routes with the two-plane gradient: their activation plane is fp16, where |q| <= 2048 is still exact — one
        pass as before; ``code_flag`` (the quantiser's device flag, bit 1 = a code beyond +-2047) poisons the result with NaN
        instead of a host sync for a case that does not occur (an activation beyond 136 at 4 bits);
      * otherwise q = 256 hi + lo with both digits exact in bf16 (ops.code_digits: one launch), two passes,
        (256 GW(hi) + GW(lo)) / n (ops.digit_combine: one launch), NaN from |q| >= 2^16 through the device flag.
    ``layout_like``: the parameter — the result takes its memory format where the route can write it (no re-layout copy when
    autograd accumulates it).  No route for the shape: None, the caller uses the library."""
    def run(xt, levels, terms=None):
        return conv_grad_weight_routes(xt, go, weight_shape, stride, padding, dilation, X_CODES, x_levels=levels,
                                       terms=terms, layout_like=layout_like)

    if codes_fit:
        return run(input, x_levels)
    if code_flag is not None and ops.split_terms() == 2:
        gw = run(input, x_levels, terms=2)            # only the rungs on the pixel-major kernel
        if gw is not None:
            if code_flag.dtype != torch.int32:
                return gw + torch.where((code_flag.reshape(()) & 2) != 0, float("nan"), 0.0)
            if ops._storage_dense(gw) and not gw.is_contiguous():
                # keep the parameter's (channels-last) layout through the poison pass: it works in storage order
                st = gw.permute(0, 2, 3, 1)
                return ops.poison(st, code_flag, 2).permute(0, 3, 1, 2)
            return ops.poison(gw, code_flag, 2)
    hi, lo, dflag = ops.code_digits(input, float(x_levels), code_flag)
    g_hi = run(hi, 1.0)
    if g_hi is None:
        return None
    g_lo = run(lo, 1.0)
    # |q| >= 2^16 (an activation beyond 4369 at 4 bits): the high digit is not exact in bf16 any more — the result is poisoned on
    # the device (NaN, like the chain's int8 flag) instead of a host sync per layer for a case that does not occur
    return ops.digit_combine(g_hi, g_lo, ops._inv_f32(float(x_levels)), dflag)


class DorefaWkConv2dFn(QtFunction):
    """Training-mode DorefaConv2d(bit_width = k), 2 <= k <= 8: conv2d(x, w_q, b) for the quantised image w_q the layer's
    weight_op produced (layers/dorefa_layers.py:77-82, functions/dorefa_connect.py:99-111); the gradient w.r.t. w_q flows on
    into weight_op's own autograd graph (tanh and its normalisation), exactly as in the reference.

    w_q = c / n_w with odd integer levels c, so every contraction has one operand that is exact in bf16 / int8:
      forward   activation with int8 codes (nnDorefaQuant tag) and k <= 7: (1 / (n_a n_w)) * sum q c on the int8 matrix cores
                (dorefa_wk_conv_forward); real-valued activation, codes beyond int8, or k = 8 (|c| <= 255 does not fit int8 but
                is exact in bf16 / fp16): (1 / n_w) * the split conv with the level image (dorefa_levels_conv_forward);
      grad_x    (1 / n_w) * the exact-split conv of the gradient with the flipped level image (any square stride);
      grad_w_q  activation codes x exact-split gradient on the pixel-major / K-major / strided weight-gradient routes."""

    @staticmethod
    def forward(ctx, input, weight_q, bias, bit_width, conv_args):
        stride, padding, dilation, groups = conv_args
        ctx.has_bias, ctx.conv_args, ctx.bit_width = bias is not None, conv_args, int(bit_width)
        ctx.save_for_backward(input, weight_q)
        ctx.x_levels = _act_levels(input, packed.NHWC) if input.dim() == 4 else None
        ctx.code_flag = packed.lookup_codes(input, packed.NHWC).overflow if ctx.x_levels is not None else None
        y = None
        ok = groups == 1 and not isinstance(padding, str) and input.dim() == 4 and input.dtype == torch.float32
        if ok and ctx.x_levels is not None and bit_width <= LEVEL_INT8_BITS:
            wc = ops.pack_conv_weight_dorefa_codes(weight_q.detach(), bit_width)
            y = dorefa_wk_conv_forward(input, weight_q, bias, conv_args, bit_width, wc)
        ctx.codes_fit = y is not None            # the int8 route ran: every |code| <= 127
        if y is None and ok and _cfg("FLOAT_PATH") == "bf16x3":
            y = dorefa_levels_conv_forward(input, weight_q, bias, conv_args, bit_width)
        if y is None:
            note_library_path(input, "k-bit DoReFa conv outside the level routes")
            y = F.conv2d(input, weight_q, bias, stride, padding, dilation, groups)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        input, weight_q = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conv_args
        go = _dense(grad_output)
        k = ctx.bit_width
        grad_input = grad_weight = grad_bias = None
        mfma = own_conv_backward(go, groups, padding, go.numel() * weight_q[0].numel())
        if ctx.needs_input_grad[0]:
            grad_input = conv_grad_input(input, _weight_levels(weight_q, k) if mfma else None, go, stride, padding, dilation, groups,
                                         W_LEVELS, out_scale=_inv_levels(k), gate=mfma, lib_weight=lambda: weight_q)
        if ctx.needs_input_grad[1]:
            if mfma and ctx.x_levels is not None:
                grad_weight = dorefa_conv_grad_weight(input, go, weight_q.shape, stride, padding, dilation, ctx.x_levels, ctx.codes_fit,
                                                      ctx.code_flag)
            if grad_weight is None:
                grad_weight = lib_conv2d_weight(input, weight_q.shape, go, stride, padding, dilation, groups)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = go.sum((0, 2, 3))
        return grad_input, grad_weight, grad_bias, None, None


class DorefaWkLinearFn(QtFunction):
    """Training-mode LinearDorefa(bit_width = k), 2 <= k <= 8; see DorefaWkConv2dFn (layers/dorefa_layers.py:41-45)."""

    @staticmethod
    def forward(ctx, input, weight_q, bias, bit_width):
        ctx.has_bias, ctx.bit_width = bias is not None, int(bit_width)
        ctx.save_for_backward(input, weight_q)
        ctx.x_levels = _act_levels(input, packed.ROWS_LAST)
        y = None
        if input.dtype == torch.float32 and ctx.x_levels is not None and bit_width <= LEVEL_INT8_BITS:
            wc = ops.dorefa_weight_codes(weight_q.detach(), bit_width)
            y = dorefa_wk_linear_forward(input, weight_q, bias, bit_width, wc)
        ctx.codes_fit = y is not None
        if y is None and _cfg("FLOAT_PATH") == "bf16x3":
            y = dorefa_levels_linear_forward(input, weight_q, bias, bit_width)
        if y is None:
            note_library_path(input, "k-bit DoReFa linear outside the level routes")
            y = F.linear(input, weight_q, bias)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        input, weight_q = ctx.saved_tensors
        k = ctx.bit_width
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        x2 = input.reshape(-1, input.shape[-1])
        grad_input = grad_weight = grad_bias = None
        big = (g2.is_cuda and g2.dtype == torch.float32 and g2.numel() > 0
               and g2.shape[0] * g2.shape[1] * x2.shape[1] >= _cfg("BWD_MFMA_MIN_MACS"))
        if ctx.needs_input_grad[0]:
            if big:        # real gradient x integer levels
                lv = _weight_levels(weight_q, k)
                grad_input = (ops.float_linear(g2.contiguous(), lv.t().contiguous(), "raw") * _inv_levels(k)).view(input.shape)
            else:
                grad_input = lib_mm(g2, weight_q).view(input.shape)
        if ctx.needs_input_grad[1]:
            if big and ctx.x_levels is not None:   # g^T . x with x = codes / n_a
                grad_weight = _levels_grad_weight_linear(g2, x2, ctx.x_levels, ctx.codes_fit)
            if grad_weight is None:
                grad_weight = real_matmul(g2.t(), x2) if big else lib_mm(g2.t(), x2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = g2.sum(0)
        return grad_input, grad_weight, grad_bias, None


class RealLinearFn(QtFunction):
    """F.linear(x, W, b) for two REAL fp32 device operands on the matrix cores (six-term bf16 planes, fp32-GEMM accuracy), forward
    and both gradients: LinearDorefa(bit_width = 32), whose weight quantiser is the identity (functions/dorefa_connect.py:100-101,
    layers/dorefa_layers.py:41-45) — the layer is an un-quantised nn.Linear."""

    @staticmethod
    def forward(ctx, input, weight, bias):
        ctx.has_bias = bias is not None
        ctx.save_for_backward(input, weight)
        x2 = input.reshape(-1, input.shape[-1])
        y = ops.real_linear(x2.detach().contiguous(), weight.detach(), bias.detach() if bias is not None else None)
        return y.view(*input.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, grad_output):
        input, weight = ctx.saved_tensors
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        x2 = input.reshape(-1, input.shape[-1])
        grad_input = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            grad_input = real_matmul(g2, weight).view(input.shape)
        if ctx.needs_input_grad[1]:
            grad_weight = real_matmul(g2.t(), x2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = g2.sum(0)
        return grad_input, grad_weight, grad_bias


class RealConv2dFn(QtFunction):
    """F.conv2d(x, W, b) for two REAL fp32 device operands (groups == 1, zero padding): DorefaConv2d(bit_width = 32).  Forward and
    — for stride 1, dilation 1 — grad_x (the conv of the gradient with the flipped, transposed weight) on the six-term implicit
    GEMM; grad_W on the pixel-major kernel (stride 1, 3 x 3 / 5 x 5: the image's terms as channel groups) or one six-term GEMM per
    filter tap (real_conv_grad_weight_taps)."""

    @staticmethod
    def forward(ctx, input, weight, bias, conv_args):
        stride, padding, dilation, groups = conv_args
        ctx.has_bias, ctx.conv_args = bias is not None, conv_args
        ctx.save_for_backward(input, weight)
        return real_weight_conv2d(input, weight, bias, stride, padding, dilation, groups)

    @staticmethod
    def backward(ctx, grad_output):
        input, weight = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conv_args
        go = _dense(grad_output)
        grad_input = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            grad_input = conv_grad_input(input, weight, go, stride, padding, dilation, groups, W_REAL,
                                         gate=go.is_cuda and go.dtype == torch.float32 and go.numel() > 0)
        if ctx.needs_input_grad[1]:
            grad_weight = conv_grad_weight(input, weight.shape, go, stride, padding, dilation, groups, x_is_pm1=False,
                                           real_any_channels=True)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = go.sum((0, 2, 3))
        return grad_input, grad_weight, grad_bias, None


# ---- Lin / Log fixed-point family (layers/log_lin_layers.py) in training mode -----------------------------------------------------
# Reference: F.linear / F.conv2d(x, Q(W), b) with Q = LinQuant / LogQuant(lin_back=True): the weight quantiser's backward is the
# identity, so grad_W is the UN-masked dL/dQ(W).  Q(W) is exact in bf16 (ops.levels_exact_in_bf16) -> the forward and grad_x are
# exact three-term splits of the real operand (x, g) against the replicated levels; grad_W multiplies two real operands (six-term
# routes of RealLinearFn / RealConv2dFn).  Both weight operands come from ONE quantise-and-pack launch per step
# (ops.pack_levels_bf16x3).  Configurations whose levels are not exact in bf16 train on RealLinearFn / RealConv2dFn instead.
# An activation that is itself exact in bf16 — the tagged output of nnQuant, or a detected one (loglin_act_planes) — enters the
# forward as ONE term against a one-term weight plane, and grad_W as the exact operand of three terms of g (LOGLIN_ONE_TERM).

class LogLinLinearFn(QtFunction):
    """F.linear(x, Q(W), b) for a device fp32 x, Q the Lin / Log quantiser ``quant`` = (dtype, fsr, bit_width, with_sign) with
    levels exact in bf16."""

    @staticmethod
    def forward(ctx, input, weight, bias, quant):
        ctx.has_bias = bias is not None
        ctx.save_for_backward(input)
        planes, flag = loglin_act_planes(input, weight, packed.ROWS_LAST)
        ctx.x_exact = planes is not None
        fwd, gx, _ = ops.pack_levels_bf16x3(weight, *quant, grad_x=ctx.needs_input_grad[0], fwd_terms=1 if ctx.x_exact else 3)
        ctx.gx, ctx.w_shape = gx, tuple(weight.shape)
        b = bias.detach() if bias is not None else None
        if ctx.x_exact:          # one term x one term
            y = ops.float_linear(None, weight.detach(), "raw", poison_bias(b, flag, weight.shape[0], input.device),
                                 weight_triples=fwd, planes=planes)
        else:
            x2 = input.reshape(-1, input.shape[-1])
            y = ops.float_linear(x2.detach().contiguous(), weight.detach(), "raw", b, weight_triples=fwd, terms=3)
        return y.view(*input.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, grad_output):
        input, = ctx.saved_tensors
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        x2 = input.reshape(-1, input.shape[-1])
        grad_input = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            N, K = ctx.w_shape
            shape_t = torch.empty((K, N), dtype=torch.float32, device="meta")
            grad_input = ops.float_linear(g2.contiguous(), shape_t, "raw", weight_triples=ctx.gx, terms=3).view(input.shape)
        if ctx.needs_input_grad[1]:
            if ctx.x_exact and _hip2d(g2, x2):
                # x is exact in bf16: three exact terms of g^T against the levels replicated ("raw" — pm1_matmul would take sign(x))
                grad_weight = ops.float_linear(g2.t().contiguous(), x2.detach().t().contiguous(), "raw", terms=3)
            else:
                grad_weight = real_matmul(g2.t(), x2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = g2.sum(0)
        ctx.gx = None
        return grad_input, grad_weight, grad_bias, None


class LogLinConv2dFn(QtFunction):
    """F.conv2d(x, Q(W), b) (groups == 1, zero padding) for a device fp32 NCHW / channels-last x, Q as in LogLinLinearFn.  grad_x
    outside ops.grad_input_route_applicable (dilation, non-square stride, ...) uses the counted library helper on Q(W), whose fp32
    image then comes from the same pack launch."""

    @staticmethod
    def forward(ctx, input, weight, bias, quant, conv_args):
        stride, padding, dilation, groups = conv_args
        ctx.has_bias, ctx.conv_args, ctx.quant = bias is not None, conv_args, quant
        ctx.save_for_backward(input, weight)
        want_gx = ctx.needs_input_grad[0]
        routed = ops.grad_input_route_applicable(weight.shape, stride, padding, dilation)    # what the backward's rung will take
        planes, flag = loglin_act_planes(input, weight, packed.NHWC)
        ctx.x_exact = planes is not None
        fwd, gx, wq = ops.pack_levels_bf16x3(weight, *quant, grad_x=want_gx and routed, image=want_gx and not routed,
                                             fwd_terms=1 if ctx.x_exact else 3)
        ctx.gx, ctx.wq, ctx.w_shape = gx, wq, tuple(weight.shape)
        N, C, H, W = input.shape
        Cout, _, kh, kw = (int(v) for v in weight.shape)
        b = bias.detach() if bias is not None else None
        if ctx.x_exact:          # one term x one term on the same implicit GEMM
            y2 = ops.float_conv2d(None, weight.detach(), "raw", poison_bias(b, flag, Cout, input.device), stride, padding, dilation,
                                  weight_triples=fwd, pixels=planes, in_shape=tuple(input.shape))
        else:
            y2 = ops.float_conv2d(input.detach(), weight.detach(), "raw", b, stride, padding, dilation, weight_triples=fwd, terms=3)
        Ho, Wo = ops.conv_out_hw(H, W, kh, kw, stride, padding, dilation)
        return nchw_result(y2, input, N, Ho, Wo, Cout)

    @staticmethod
    def backward(ctx, grad_output):
        input, weight = ctx.saved_tensors
        stride, padding, dilation, groups = ctx.conv_args
        go = _dense(grad_output)
        grad_input = grad_weight = grad_bias = None
        if ctx.needs_input_grad[0]:
            def image():                  # the forward's; an empty gradient: nothing was packed for it
                return ctx.wq if ctx.wq is not None else ops.pack_levels_bf16x3(weight, *ctx.quant, forward=False, grad_x=False, image=True)[2]
            grad_input = conv_grad_input(input, weight, go, stride, padding, dilation, groups, W_PACKED, operand=ctx.gx,
                                         gate=ctx.gx is not None and go.numel() > 0, lib_weight=image)
        if ctx.needs_input_grad[1]:
            grad_weight = conv_grad_weight(input, ctx.w_shape, go, stride, padding, dilation, groups, x_is_pm1=False,
                                           real_any_channels=True, x_exact_bf16=ctx.x_exact)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = go.sum((0, 2, 3))
        ctx.gx = ctx.wq = None
        return grad_input, grad_weight, grad_bias, None, None


# ---- depthwise convs (groups == in_channels) ---------------------------------------------------------------------------------------
# K = kh * kw <= 49 is no matrix-core shape: one streaming launch forward, one per gradient (csrc/dwconv.hip, DESIGN.md "Depthwise
# convs").  The kernels multiply whatever the activation holds, so nothing here asks whether it is +-1: no tag lookup, no detection,
# no host synchronisation — the node can be captured in a hipGraph as it is.

def _streaming_grad_output(grad_output: torch.Tensor, input: torch.Tensor) -> torch.Tensor:
    """The incoming gradient as the streaming kernels read it: dense, and of the activation's dtype (the gradient entries take one
    element type for the activation side; it already has it unless something between the layers changed the dtype)."""
    go = _dense(grad_output)
    return go if go.dtype == input.dtype else go.to(input.dtype)


class _StreamingFamily(NamedTuple):
    """One family of streaming convs as this module uses it: the descriptor the shared bodies of ``ops`` take (they are called
    directly, with ``groups`` in its place: the depthwise family does not look at it), and what admits a layer to the
    materialising helpers (``(layer, act, what)``: raises the family's ValueError).  The autograd bodies, the two helpers' bodies
    and these two instances are all there is per family here: a new operation is written once."""
    ops_family: ops._Streaming
    planes_admission: Callable
    codes_admission: Callable


_DEPTHWISE = _StreamingFamily(ops._DW, _depthwise_admission, _depthwise_admission)
_GROUPED = _StreamingFamily(ops._GC, _grouped_planes_admission, _grouped_codes_admission)


def _streaming_forward(fam: _StreamingFamily, ctx, input, weight, bias, kind, weight_q, ste, conv_args):
    stride, padding, dilation, groups = conv_args
    ctx.kind = kind if weight_q is None else "raw"
    ctx.conv_args, ctx.ste, ctx.has_bias = conv_args, float(ste), bias is not None
    ctx.bias_dtype = bias.dtype if bias is not None else None
    input = _dense(input)
    ctx.save_for_backward(input, weight, weight_q)
    if input.dtype in ops.HALF_DTYPES:      # the "_h" entries add an fp32 bias vector before their one rounding
        bias = half_bias(bias, input.dtype)
    return ops._streaming_conv2d(fam.ops_family, input, weight if weight_q is None else weight_q, bias, stride, padding, dilation, groups,
                                 ctx.kind)


def _streaming_backward(fam: _StreamingFamily, ctx, grad_output):
    input, weight, weight_q = ctx.saved_tensors
    stride, padding, dilation, groups = ctx.conv_args
    go = _streaming_grad_output(grad_output, input)
    grad_input = grad_weight = grad_bias = None
    if ctx.needs_input_grad[0]:
        grad_input = ops._streaming_conv2d_grad_input(
            fam.ops_family, input.shape, weight if weight_q is None else weight_q, go, stride, padding, dilation, groups, ctx.kind,
            input.is_contiguous(memory_format=torch.channels_last) and not input.is_contiguous())          # channels_last
    want_bias = ctx.has_bias and ctx.needs_input_grad[2]
    if ctx.needs_input_grad[1] or want_bias:
        grad_weight, grad_bias = ops._streaming_conv2d_grad_weight(fam.ops_family, input, go, weight, stride, padding, dilation, groups,
                                                                   ctx.ste, want_bias)
        if not ctx.needs_input_grad[1]:
            grad_weight = None
    if grad_bias is not None and grad_bias.dtype != ctx.bias_dtype:
        grad_bias = grad_bias.to(ctx.bias_dtype)
    return grad_input, grad_weight, grad_bias, None, None, None, None


#: routes taken by ``depthwise_half_route`` / ``grouped_half_route`` layers, by family ("depthwise" | "grouped"); the tests read it
STREAMING_HALF_STATS: Counter = Counter()

#: depthwise BinConv2d / TerConv2d on bf16 / fp16 activations run the "_h" streaming kernels (False: the dense library's half conv,
#: counted in LIBRARY_PATHS).  Set from tools/bench_half_streaming.py by the rule of DESIGN.md "Half-precision streaming convs":
#: True iff for both dtypes and all six MobileNet-v1 shapes the forward+backward round range lies entirely below the library's.
#: Measured (profiles/half_streaming_bench_line.json): it does on all twelve rows, 1.5x - 7x; the forward alone is level with the
#: library (0.5x - 1.1x of its time; behind it by 9 - 11 % at 256 channels, 28 x 28).
DEPTHWISE_HALF = True
#: most input channels per group that take the grouped "_h" kernels (0: off; never above GROUPED_MAX_CIN_G): the largest measured
#: value of 4, 8 up to which, for both dtypes, the training-step round range lies below the library's and the forward median is not
#: above the library's.  Measured: 4 and 8 both pass in both dtypes (step 2.0x - 14x, forward 1.5x - 7.6x; the closest row is
#: 256 x 28 x 28 with 8 channels per group in fp16: forward 319 against 488 us, step 1603 - 1627 against 3149 - 3157 us).
GROUPED_HALF_MAX_CIN_G = 8


def _streaming_half_common(layer, input) -> bool:
    """What both half routes ask: ``half_route`` holds (same half dtype, or an fp32 weight under autocast to the activation's
    dtype), a 4-D device activation, padding mode "zeros" with numeric padding."""
    return (half_route(input, layer.weight) and input.dim() == 4 and layer.padding_mode == "zeros"
            and not isinstance(layer.padding, str))


def _streaming_f32_common(layer, input) -> bool:
    """What both fp32 routes ask: a 4-D fp32 device tensor, an fp32 weight, padding mode "zeros"."""
    return (isinstance(input, torch.Tensor) and input.is_cuda and input.dtype == torch.float32 and input.dim() == 4
            and layer.weight.dtype == torch.float32 and layer.padding_mode == "zeros")


def depthwise_half_route(layer, input) -> bool:
    """``depthwise_route`` for a bf16 / fp16 activation: the "_h" streaming kernels, switched by ``DEPTHWISE_HALF``.  As on fp32
    nothing asks whether the activation is +-1."""
    return (bool(DEPTHWISE_HALF) and _streaming_half_common(layer, input) and layer.groups > 1
            and ops.depthwise_applicable(input.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation, layer.groups))


def grouped_half_route(layer, input) -> bool:
    """``grouped_route`` for a bf16 / fp16 activation: at least ``GROUPED_MIN_GROUPS`` groups of 2 ... ``GROUPED_HALF_MAX_CIN_G``
    (capped by ``GROUPED_MAX_CIN_G``) input channels each."""
    top = min(int(GROUPED_HALF_MAX_CIN_G), GROUPED_MAX_CIN_G)
    return (_streaming_half_common(layer, input) and layer.groups >= GROUPED_MIN_GROUPS
            and 2 <= int(layer.weight.shape[1]) <= top
            and ops.grouped_applicable(input.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation, layer.groups))


def depthwise_route(layer, input) -> bool:
    """``layer`` (a Conv2d subclass with an fp32 weight) applied to ``input`` is a depthwise conv the HIP kernels take: a 4-D fp32
    device tensor, ``groups == in_channels > 1``, padding mode "zeros" with numeric padding."""
    return (_streaming_f32_common(layer, input) and layer.groups > 1
            and ops.depthwise_applicable(input.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation, layer.groups))


class DepthwiseConv2dFn(QtFunction):
    """conv2d(x, Q(W), b, groups = C) with one input channel per group.  ``kind``: the quantiser the forward and grad_input kernels
    apply to the taps ("binary" | "ternary" | "raw"); ``weight_q``: an image that replaces Q(W) (a saved stochastic draw, the stored
    eval-mode image) — the kernels then run "raw" on it; ``ste``: threshold of the straight-through mask on the UNquantised
    ``weight`` (0: none).  Forward one launch; backward grad_input and grad_weight (partials + combine inside one call), the bias
    gradient being a by-product of the latter."""

    @staticmethod
    def forward(ctx, input, weight, bias, kind, weight_q, ste, conv_args):
        return _streaming_forward(_DEPTHWISE, ctx, input, weight, bias, kind, weight_q, ste, conv_args)

    @staticmethod
    def backward(ctx, grad_output):
        return _streaming_backward(_DEPTHWISE, ctx, grad_output)


# ---- grouped convs with a few channels per group -----------------------------------------------------------------------------------
# K = cin_g * kh * kw <= 512 on a block-diagonal operand is no matrix-core shape either: one streaming launch forward, one per
# gradient (csrc/gconv.hip, DESIGN.md "Grouped convs"), instead of one conv per group on copied slices.  As above, nothing asks
# whether the activation is +-1.

#: fewer groups keep the per-group loop: it is short and its tiles are reasonably full
GROUPED_MIN_GROUPS = 4
#: most input channels per group that take the grouped kernels; set from tools/bench_grouped.py by the rule of DESIGN.md "Grouped
#: convs" (the largest measured cin_g of 4, 8, 16, 24 up to which a training step beats both the loop and the dense library and
#: the forward is not behind the better of the two), never above 31.  Measured: 4 and 8 pass; at 16 the library wins the forward.
GROUPED_MAX_CIN_G = 8


def grouped_route(layer, input) -> bool:
    """``layer`` (a Conv2d subclass with an fp32 weight) applied to ``input`` is a grouped conv the HIP kernels take: a 4-D fp32
    device tensor, ``groups >= GROUPED_MIN_GROUPS`` with 2 ... ``GROUPED_MAX_CIN_G`` input channels each, padding mode "zeros"
    with numeric padding."""
    return (_streaming_f32_common(layer, input) and layer.groups >= GROUPED_MIN_GROUPS
            and 2 <= int(layer.weight.shape[1]) <= GROUPED_MAX_CIN_G
            and ops.grouped_applicable(input.shape, layer.weight.shape, layer.stride, layer.padding, layer.dilation, layer.groups))


class GroupedConv2dFn(QtFunction):
    """conv2d(x, Q(W), b, groups = G) with a few input channels per group: the sibling of ``DepthwiseConv2dFn``, same arguments.
    Forward one launch; backward grad_input and grad_weight (partials + combine inside one call), the bias gradient being a
    by-product of the latter."""

    @staticmethod
    def forward(ctx, input, weight, bias, kind, weight_q, ste, conv_args):
        return _streaming_forward(_GROUPED, ctx, input, weight, bias, kind, weight_q, ste, conv_args)

    @staticmethod
    def backward(ctx, grad_output):
        return _streaming_backward(_GROUPED, ctx, grad_output)


def grouped_quant_conv(layer, input, kind: str, quant_op):
    """BinConv2d / TerConv2d with ``groups`` > 1 (layers/binary_layers.py:59-60,103-106 hand ``groups`` to F.conv2d): group g is
    an independent conv of its channel slice with its rows of the weight, and the element-wise quantisers (safeSign, the fixed
    ternary thresholds) commute with slicing — so every group runs on the groups == 1 routes of this backend, forward and
    backward, and the results are concatenated.  Returns None when the case is not this path's (eval mode with autograd, a
    weight off the quantiser's grid): the caller continues with its general code."""
    G = int(layer.groups)
    cin, cout = int(input.shape[1]) // G, int(layer.weight.shape[0]) // G
    args = (layer.stride, layer.padding, layer.dilation, 1)
    if not layer.training:
        if autograd_records(input, layer.weight):
            return None
        if not layer._eval_on_grid():
            return None
    wq_full = None
    if layer.training and not layer.deterministic:
        wq_full = quant_op.apply(layer.weight.detach())          # ONE stochastic draw for the whole weight, as upstream
    cl = input.is_contiguous(memory_format=torch.channels_last) and not input.is_contiguous()
    # a +-1 tag of the whole activation (BinaryConnect's sign planes) holds for every channel slice
    known_pm1 = True if (layer.binary_input or packed.lookup(input, packed.NHWC) is not None) else layer.binary_input
    flag = None
    if (known_pm1 is None and _cfg("DETECT_BINARY_INPUT") and input.is_cuda and input.dtype == torch.float32 and input.dim() == 4
            and input.numel() > 0):
        # un-tagged activation, no hint: ONE detection on the whole activation, remembered under the layer's own weight (the
        # per-group weight views are fresh tensors on every call: verdicts keyed on them die with them — a host sync per group
        # per call, and nothing for DETECT_MODE = "remember" to remember)
        ok, flag = detect_pm1(input, layer.weight)
        known_pm1 = bool(ok)
    ys = []
    for g in range(G):
        xg = input[:, g * cin:(g + 1) * cin]
        xg = xg.contiguous(memory_format=torch.channels_last) if cl else xg.contiguous()
        wg = layer.weight[g * cout:(g + 1) * cout]
        bg = layer.bias[g * cout:(g + 1) * cout] if layer.bias is not None else None
        if layer.training:
            wq = wq_full[g * cout:(g + 1) * cout] if wq_full is not None else None
            ys.append(QuantConv2dFn.apply(xg, wg, bg, kind, wq, known_pm1, args))
        else:
            ys.append(quant_conv2d_forward(xg, wg, bg, *args, kind, weight_q=wg, binary_input=known_pm1, padding_mode="zeros"))
    out = torch.cat(ys, 1)
    if flag is not None:          # a remembered "+-1" verdict: the device flag of THIS activation turns a wrong assumption into NaN
        out = out + torch.where(flag.reshape(()) != 0, float("nan"), 0.0).to(out.dtype)
    return out


#: backward GEMMs with one +-1/0 operand (grad_x = g . Q(W); grad_W = g^T . x for +-1 activations) run on the bf16
#: matrix cores from this many multiply-accumulates on: the real operand is split exactly into bf16 triples, the
#: +-1/0 operand is exact in bf16, accumulation is fp32 — fp32-GEMM accuracy at ~2.5x the fp32 library's speed
#: (4096^3: 0.51 vs 1.03 ms per GEMM incl. transposes and splits, max error 1.6e-6 vs 3.0e-6 of fp64; tools/bench_backward.py).  Below it the dense library is used (launch-bound either way).
BWD_MFMA_MIN_MACS = 0          # (round 4: every size on the own routes; 1 << 27 was the measured break-even against hipBLASLt)


#: backward convs with a +-1 / 0 operand on the bf16 matrix cores (ops.conv2d_grad_input_q / conv2d_grad_weight_pm1)
BWD_CONV_MFMA = True


#: grad_x of LinearBin / LinearTer packs Q(W)^T in one kernel from W (A/B switch for tools/)
LINEAR_GRAD_X_ONE_PACK = True


def pm1_matmul(a: torch.Tensor, b_pm1: torch.Tensor, terms=None) -> torch.Tensor:
    """a [M, J] (real) @ b_pm1 [J, K] (entries in {-1, 0, +1}) -> [M, K] fp32.  ``terms``: split of a (ops.float_linear)."""
    M, J = a.shape
    K = b_pm1.shape[1]
    if a.is_cuda and a.dtype == torch.float32 and M * J * K >= _cfg("BWD_MFMA_MIN_MACS") and a.numel() > 0 and b_pm1.numel() > 0:
        return ops.float_linear(a.contiguous(), b_pm1.t().contiguous(), "sign", terms=terms)
    return lib_mm(a, b_pm1, "backward GEMM below BWD_MFMA_MIN_MACS / non-fp32")


class QuantLinearFn(QtFunction):
    """Autograd node of LinearBin / LinearTer in training mode.

    forward : F.linear(x, Q(W), b)                         layers/binary_layers.py:44
    backward: grad_x = g . Q(W) ; grad_W = (g^T . x) * 1[|W| <= 1.001] ; grad_b = sum g
              (what autograd derives from F.linear + the STE backward of the quantiser,
              functions/binary_connect.py:31-38 / terner_connect.py:29-34)
    """

    @staticmethod
    def forward(ctx, input, weight, bias, kind, weight_q, binary_input, weight_planes=None):
        """``weight_planes``: the ready nibble plane of Q(weight) (written by the fused optimiser step, utils/optim.py) — the forward
        then packs the activation alone.  The backward does not use it: it reads the fp32 weight."""
        ctx.kind = kind
        ctx.has_bias = bias is not None
        ctx.bias_dtype = bias.dtype if bias is not None else None
        # a stochastic draw must be kept; the deterministic image is recomputed in backward
        ctx.save_for_backward(input, weight, weight_q)
        # +-1 activation known without a device check (tag of a quantiser, or the layer's binary_input hint)?
        ctx.x_is_pm1 = bool(split_hint(binary_input)[0]) or (input.is_cuda and input.dtype in ops.PACK_DTYPES
                                              and packed.lookup(input, packed.ROWS_LAST) is not None)
        clear_last_detection()
        out = quant_linear_forward(input, weight, bias, kind, weight_q=weight_q, weight_planes=weight_planes, binary_input=binary_input,
                                   half_ok=True)
        if not ctx.x_is_pm1 and binary_input is None and input.is_cuda:
            # un-tagged activation THIS forward detected as +-1 (a reshaped / flattened sign image): the backward's g^T . x then
            # runs on the matrix cores as well instead of the dense library
            ctx.x_is_pm1 = last_detection_said_pm1(input)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        from .common import ste_mask
        input, weight, weight_q = ctx.saved_tensors
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        grad_input = grad_weight = grad_bias = None
        in_dtype, w_dtype = input.dtype, weight.dtype
        if g2.is_cuda and g2.dtype in ops.HALF_DTYPES:
            # half model: a half value is exact in fp32, so the matrix-core routes below contract the upcast operands and their fp32
            # result is rounded once to the dtype autograd expects (input's / the parameter's)
            g2, input, weight = g2.float(), input.float(), weight.float()
            weight_q = weight_q.float() if weight_q is not None else None
        if ctx.needs_input_grad[0]:
            Nf, Kf = int(weight.shape[0]), int(weight[0].numel())
            if (_cfg("LINEAR_GRAD_X_ONE_PACK") and weight_q is None and ctx.kind in ("binary", "ternary") and g2.is_cuda and g2.dtype == torch.float32
                    and weight.dtype == torch.float32 and ops.split_terms() == 2 and Nf % 4 == 0 and g2.numel() > 0 and weight.numel() > 0):
                # g . Q(W): the operand Q(W)^T comes from ONE kernel that reads W where it lies (quantiser + transpose + fp16 pairs:
                # qt_f16x2_pack_conv_weight_f32 on the [N, K, 1, 1] view) instead of quantise, transpose-copy and pack (three passes,
                # 280 us for AlexNet's 9216 x 4096 layer)
                wt = ops.pack_conv_weight_bf16x3(weight.detach().reshape(Nf, Kf, 1, 1), ctx.kind, terms=2, transpose_flip=True)
                shape_t = torch.empty((Kf, Nf), dtype=torch.float32, device="meta")
                grad_input = ops.float_linear(g2.contiguous(), shape_t, ctx.kind, weight_triples=wt, terms=2).view(input.shape)
            else:
                wq = weight_q if weight_q is not None else quantize_weight_f32(weight, ctx.kind)
                grad_input = pm1_matmul(g2, wq).view(input.shape)
        if ctx.needs_input_grad[1]:
            x2 = input.reshape(-1, input.shape[-1])
            # (rows of g2^T are output features: the exact three-term split, not the per-tensor-scaled two-term one)
            if ctx.x_is_pm1:
                gw = pm1_matmul(g2.t(), x2, terms=3)
            else:
                gw = real_matmul(g2.t(), x2)          # two real operands (a real-valued first layer): six-term planes
            grad_weight = ste_mask(gw, weight)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_bias = g2.sum(0)
        if grad_input is not None and grad_input.dtype != in_dtype:
            grad_input = grad_input.to(in_dtype)
        if grad_weight is not None and grad_weight.dtype != w_dtype:
            grad_weight = grad_weight.to(w_dtype)
        if grad_bias is not None and grad_bias.dtype != ctx.bias_dtype:
            grad_bias = grad_bias.to(ctx.bias_dtype)
        return grad_input, grad_weight, grad_bias, None, None, None, None
