"""A fixed list of calls into the depthwise / grouped streaming-conv wrappers of ``ops`` and a recorder of what each hands to the
C-ABI (helper module, not a test).  ``record_calls`` returns, per case, the ``[entry, [args ...]]`` of every ``_lib.call`` and
``qt_*_work_floats`` the wrapper made, or ``{"raises": type, "text": message}``; ``record_predicates`` the values of the pure shape
predicates.  ``tests/golden/streaming_call_trace_v1.json`` holds both as recorded on the commit BEFORE the wrappers were folded
into one body per operation (``python tests/_streaming_cases.py OUT.json`` with that commit's package on the path);
test_streaming_trace_cpu.py and test_gpu_streaming_trace.py replay the list on the code under test and compare.

An argument is recorded by value (ints, floats), as "stream", or — a pointer — as null, the LABEL of the tensor the case supplied
that it equals (x, w, bias, alpha, beta, stats, flag, go, out, out_sign, out_nib, out_bias, workspace, planes, codes) or "other".
The cases supply their outputs (all but the few that are about the layout of a result the wrapper allocates), so nearly every
pointer is labelled and a swapped pair shows.

Without a device (``device=None``) the tensors are CPU tensors of a subclass that says ``is_cuda``, ``ops._stream`` is replaced
and no entry runs (the work sizes, pure host functions, do); with a device the calls go through to the library."""
import contextlib
import ctypes
import itertools
import json
import sys

import torch

from pytorch_quantize_impls_amd import _lib, ops

F32, BF16, F16, I32, I8 = torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int8

# every geometry value distinct per axis: a transposed pair changes the trace
N, H, W, KH, KW = 2, 7, 6, 3, 2
GEO = dict(stride=(2, 1), padding=(1, 0), dilation=(1, 2))          # -> a 4 x 4 output
HO = WO = 4


class Fam:
    """One family at one shape: the public names' prefix, the ``groups`` keyword, the shapes."""

    def __init__(self, prefix, C, Cout, cin_g, groups):
        self.prefix, self.C, self.Cout, self.groups = prefix, C, Cout, groups
        self.x, self.w, self.y = (N, C, H, W), (Cout, cin_g, KH, KW), (N, Cout, HO, WO)
        self.kw = {} if prefix == "depthwise" else {"groups": groups}

    def op(self, name):
        return getattr(ops, f"{self.prefix}_{name}")


DW = Fam("depthwise", 3, 6, 1, 3)                   # multiplier 2
GC = Fam("grouped", 12, 8, 3, 4)                    # G = 4, cin_g = 3, cout_g = 2: the fp32 / half entries
GP = Fam("grouped", 8, 12, 2, 4)                    # G = 4, cin_g = 2, cout_g = 3: the plane and code entries
GP8 = Fam("grouped", 32, 12, 8, 4)                  # cin_g = 8


class _Dev(torch.Tensor):
    is_cuda = True


class Tensors:
    """Makes the tensors of one case and remembers their labels."""

    def __init__(self, device):
        self.device, self.labels, self.calls = device, {}, []

    def __call__(self, label, shape, dtype=F32, cl=False):
        t = torch.zeros(tuple(shape), dtype=dtype, device=self.device or "cpu")
        if cl:
            t = t.contiguous(memory_format=torch.channels_last)
        if self.device is None:
            t = t.as_subclass(_Dev)
        if t.numel():
            self.labels[t.data_ptr()] = label
        return t

    def planes(self, shape, mask=False):
        n, c, h, w = shape
        sign = self("planes", (n * h * w, ops.packed_ld(c)), I32)
        return ops.BitPlanes(sign=sign, rows=n * h * w, K=c, mask=self("other", sign.shape, I32) if mask else None)

    def codes(self, shape, halo=(0, 0), flag=True):
        n, c, h, w = shape
        rows = n * (h + 2 * halo[0]) * (w + 2 * halo[1])
        return ops.CodePlanes(codes=self("codes", (rows, ops.code_ld_bytes(c, 16)), I8), rows=rows, K=c, inv_n=ops.inv_levels(3),
                              bit_width=3, overflow=self("flag", (1,), I32) if flag else None)


# ---- the cases: name -> function(T) that makes its tensors with T and calls one wrapper ------------------------------------------

CASES = {}


def case(name):
    def add(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return add


DTYPES = {"f32": (F32, F32), "bf16": (BF16, BF16), "bf16_w32": (BF16, F32), "f16": (F16, F16), "f16_w32": (F16, F32)}


def _x_of(f, n=N):
    return (n,) + f.x[1:]


def _y_of(f, n=N):
    return (n,) + f.y[1:]


def _forward(f, dt="f32", cl=False, kind="raw", bias=True, n=N, w_shape=None, out_shape=None, bias_len=None, geo=GEO):
    def run(T):
        a, wd = DTYPES[dt] if isinstance(dt, str) else dt
        f.op("conv2d")(T("x", _x_of(f, n), a, cl), T("w", w_shape or f.w, wd), T("bias", (bias_len or f.Cout,)) if bias else None,
                       **geo, **f.kw, kind=kind, out=T("out", out_shape or _y_of(f, n), a, cl))
    return run


def _grad_input(f, dt="f32", cl=False, kind="raw", channels_last=None, n=N, go_dtype=None, with_out=True):
    """``with_out`` False: the result is the wrapper's own tensor ("other"), in the layout ``channels_last`` asks for — with ``out``
    given the argument is not looked at."""
    def run(T):
        a, wd = DTYPES[dt]
        f.op("conv2d_grad_input")(_x_of(f, n), T("w", f.w, wd), T("go", _y_of(f, n), go_dtype or a, cl), **GEO, **f.kw, kind=kind,
                                  channels_last=channels_last, out=T("out", _x_of(f, n), a, cl) if with_out else None)
    return run


def _grad_weight(f, dt="f32", cl=False, bias="out", ste=1.001, n=N, short=0, go_dtype=None):
    def run(T):
        a, wd = DTYPES[dt]
        need = f.op("grad_weight_work_floats")(f.x, f.w, **GEO, **f.kw)
        T.calls.clear()                 # the case's own question is not part of the wrapper's trace
        f.op("conv2d_grad_weight")(T("x", _x_of(f, n), a, cl), T("go", _y_of(f, n), go_dtype or a, cl), T("w", f.w, wd), **GEO, **f.kw,
                                   ste_threshold=ste, want_bias=bias == "want", out=T("out", f.w, wd),
                                   out_bias=T("out_bias", (f.Cout,), wd) if bias == "out" else None,
                                   workspace=T("workspace", (need - short,)))
    return run


def _sign_outputs(T, f, n, out_halo, with_bits):
    kw = {}
    if out_halo is None or with_bits:
        kw["out_sign"] = T("out_sign", (n * HO * WO, ops.packed_ld(f.Cout)), I32)
    if out_halo is not None:
        hy, hx = (abs(int(v)) for v in out_halo)
        kw["out_nib"] = T("out_nib", (n * (HO + 2 * hy) * (WO + 2 * hx), ops.pixel_ld_nib(f.Cout)), I32)
    return kw


def _sign(f, src="planes", cl=False, kind="raw", bias=True, out_halo=None, with_bits=False, n=N, mask=False, w_shape=None):
    def run(T):
        x = T("x", _x_of(f, n), F32, cl) if src == "tensor" else T.planes(_x_of(f, n), mask)
        f.op("conv2d_sign")(x, T("w", w_shape or f.w), T("bias", (f.Cout,)) if bias else None, T("alpha", (f.Cout,)),
                            T("beta", (f.Cout,)), **GEO, **f.kw, kind=kind, shape=_x_of(f, n), out_halo=out_halo, with_bits=with_bits,
                            **_sign_outputs(T, f, n, out_halo, with_bits))
    return run


def _from_bits(f, cl=False, kind="raw", bias=True, n=N, mask=False):
    def run(T):
        f.op("conv2d_from_bits")(T.planes(_x_of(f, n), mask), _x_of(f, n), T("w", f.w), T("bias", (f.Cout,)) if bias else None, **GEO,
                                 **f.kw, kind=kind, channels_last=cl, out=T("out", _y_of(f, n), F32, cl))
    return run


def _codes(f, stats=False, relu=True, bits=8, in_halo=(0, 0), out_halo=(0, 0), bias=True, n=N, residual=False, flag="epi",
           w_shape=None):
    def run(T):
        plane = T.codes(_x_of(f, n), in_halo, flag=flag == "plane")
        epi = ops.CodeEpilogue(T("alpha", (f.Cout,)), T("beta", (f.Cout,)), bits, relu, out_halo=out_halo,
                               bn_stats=T("stats", (2 * f.Cout,)) if stats else None,
                               overflow=T("flag", (1,), I32) if flag == "epi" else None,
                               res_f32=T("other", (n * HO * WO, f.Cout)) if residual else None)
        hy, hx = (abs(int(v)) for v in out_halo)
        f.op("conv2d_codes")(plane, _x_of(f, n), T("w", w_shape or f.w), T("bias", (f.Cout,)) if bias else None, epi, **GEO, **f.kw,
                             in_halo=in_halo, out=T("out", (n * (HO + 2 * hy) * (WO + 2 * hx), ops.code_ld_bytes(f.Cout, 16)), I8))
    return run


def _from_codes(f, cl=True, flagged=True, in_halo=(0, 0), bias=True, n=N):
    def run(T):
        f.op("conv2d_from_codes")(T.codes(_x_of(f, n), in_halo), _x_of(f, n), T("w", f.w), T("bias", (f.Cout,)) if bias else None,
                                  **GEO, **f.kw, in_halo=in_halo, channels_last=cl, out=T("out", _y_of(f, n), F32, cl),
                                  flagged=flagged)
    return run


def _work_floats(f, w_shape=None):
    return lambda T: f.op("grad_weight_work_floats")(f.x, w_shape or f.w, **GEO, **f.kw)


TAPS50 = dict(stride=1, padding=5, dilation=1)      # with a 5 x 10 kernel: 50 taps on an image it fits


def _add_cases():
    for tag, f, fp in (("dw", DW, DW), ("gc", GC, GP)):      # f: the fp32 / half entries' shape; fp: the plane / code entries'
        # forward and both gradients: every dtype pair in both layouts; the kinds, no bias, the bias forms, an empty batch
        for (dt, cl) in itertools.product(DTYPES, (False, True)):
            lay = "cl" if cl else "nchw"
            case(f"{tag}.forward.{dt}.{lay}")(_forward(f, dt, cl))
            case(f"{tag}.grad_input.{dt}.{lay}")(_grad_input(f, dt, cl))
            case(f"{tag}.grad_weight.{dt}.{lay}")(_grad_weight(f, dt, cl))
        for kind in ("binary", "ternary"):
            case(f"{tag}.forward.{kind}")(_forward(f, kind=kind))
            case(f"{tag}.forward.{kind}.bf16.nobias")(_forward(f, "bf16", True, kind, bias=False))
            case(f"{tag}.grad_input.{kind}")(_grad_input(f, kind=kind))
            case(f"{tag}.grad_input.{kind}.f16_w32")(_grad_input(f, "f16_w32", True, kind))
        case(f"{tag}.forward.nobias")(_forward(f, bias=False))
        case(f"{tag}.forward.empty")(_forward(f, n=0))
        case(f"{tag}.grad_input.channels_last_arg")(_grad_input(f, channels_last=True, with_out=False))      # NCHW go, NHWC result
        case(f"{tag}.grad_input.channels_last_off")(_grad_input(f, cl=True, channels_last=False, with_out=False))  # and the reverse
        case(f"{tag}.grad_input.layout_of_go")(_grad_input(f, cl=True, with_out=False))
        case(f"{tag}.grad_input.empty")(_grad_input(f, n=0))
        case(f"{tag}.grad_weight.nobias")(_grad_weight(f, bias=None, ste=0.0))
        case(f"{tag}.grad_weight.want_bias")(_grad_weight(f, bias="want"))
        case(f"{tag}.grad_weight.want_bias.bf16_w32")(_grad_weight(f, "bf16_w32", True, bias="want", ste=0.0))
        case(f"{tag}.grad_weight.empty")(_grad_weight(f, n=0))
        case(f"{tag}.work_floats")(_work_floats(f))
        # the sign planes, from planes (and, depthwise, from a tensor): kinds, bias, the three output forms
        sources = [("planes", fp, False)] + ([("tensor", fp, False), ("tensor", fp, True)] if tag == "dw" else [("planes8", GP8, False)])
        for name, g, cl in sources:
            src = "tensor" if name == "tensor" else "planes"
            name += ".cl" if cl else ""
            for halo, wb in ((None, False), ((1, 2), False), ((1, 2), True)):
                form = "bits" if halo is None else "nib+bits" if wb else "nib"
                case(f"{tag}.sign.{name}.{form}")(_sign(g, src, cl, out_halo=halo, with_bits=wb))
            for kind in ("binary", "ternary"):
                case(f"{tag}.sign.{name}.{kind}.nobias")(_sign(g, src, cl, kind, bias=False, out_halo=(1, 2)))
            case(f"{tag}.sign.{name}.empty")(_sign(g, src, cl, n=0))
            if src == "planes":
                for kind, cl2, bias in (("raw", False, True), ("binary", True, False), ("ternary", True, True)):
                    case(f"{tag}.from_bits.{name}.{kind}.{'cl' if cl2 else 'nchw'}")(_from_bits(g, cl2, kind, bias))
                case(f"{tag}.from_bits.{name}.empty")(_from_bits(g, n=0))
        # the code chain: folded and with bn_stats, relu, both ends of the bit widths, halos on either side, the flag's sources
        for stats, relu, bits, ih, oh in ((False, True, 8, (0, 0), (0, 0)), (True, False, 2, (2, 1), (1, 2)),
                                          (False, False, 2, (2, 1), (0, 0)), (True, True, 8, (0, 0), (1, 2))):
            case(f"{tag}.codes.{'stats' if stats else 'folded'}.relu{int(relu)}.k{bits}.in{ih[0]}{ih[1]}.out{oh[0]}{oh[1]}")(
                _codes(fp, stats, relu, bits, ih, oh))
        case(f"{tag}.codes.nobias.plane_flag")(_codes(fp, bias=False, flag="plane"))
        case(f"{tag}.codes.empty")(_codes(fp, n=0))
        for cl, flagged, ih in ((True, True, (0, 0)), (False, False, (2, 1)), (True, False, (0, 0)), (False, True, (2, 1))):
            case(f"{tag}.from_codes.{'cl' if cl else 'nchw'}.flagged{int(flagged)}.in{ih[0]}{ih[1]}")(_from_codes(fp, cl, flagged, ih))
        case(f"{tag}.from_codes.nobias")(_from_codes(fp, bias=False))
        case(f"{tag}.from_codes.empty")(_from_codes(fp, n=0))
        # refusals
        alien = (f.Cout, 2, KH, KW) if tag == "dw" else (f.Cout, 5, KH, KW)          # not the family's weight shape
        case(f"{tag}.refuse.f32_activation_half_weight")(_forward(f, (F32, BF16)))
        case(f"{tag}.refuse.two_activation_dtypes")(_grad_weight(f, "bf16", go_dtype=F16))
        case(f"{tag}.refuse.two_activation_dtypes.grad_input")(_grad_input(f, "bf16", go_dtype=F32))
        case(f"{tag}.refuse.out_shape")(_forward(f, out_shape=(N, f.Cout, HO, WO + 1)))
        case(f"{tag}.refuse.bias_length")(_forward(f, bias_len=f.Cout + 1))
        case(f"{tag}.refuse.sign.negative_out_halo")(_sign(fp, out_halo=(1, -2)))
        case(f"{tag}.refuse.codes.negative_out_halo")(_codes(fp, out_halo=(-1, 2)))
        case(f"{tag}.refuse.codes.residual")(_codes(fp, residual=True))
        case(f"{tag}.refuse.codes.relu_pre")(_codes(fp, relu="pre"))
        case(f"{tag}.refuse.codes.bit_width_9")(_codes(fp, bits=9))
        case(f"{tag}.refuse.workspace_short")(_grad_weight(f, short=1))
        case(f"{tag}.refuse.sign.mask")(_sign(fp, mask=True))
        case(f"{tag}.refuse.from_bits.mask")(_from_bits(fp, mask=True))
        case(f"{tag}.refuse.weight_shape")(_forward(f, w_shape=alien))
        case(f"{tag}.refuse.weight_shape.sign")(_sign(fp, w_shape=alien))
        case(f"{tag}.refuse.weight_shape.codes")(_codes(fp, w_shape=alien))
        case(f"{tag}.refuse.work_floats.taps50")(_work_floats(f, (f.Cout, f.w[1], 5, 10)))
        case(f"{tag}.refuse.taps50")(_forward(f, w_shape=(f.Cout, f.w[1], 5, 10), geo=TAPS50, out_shape=(N, f.Cout, 13, 7)))
    case("gc.refuse.sign.cin_g3")(_sign(GC))
    case("gc.refuse.from_bits.cin_g3")(_from_bits(GC))
    case("dw.refuse.sign.input_type")(lambda T: ops.depthwise_conv2d_sign(None, T("w", DW.w), None, T("alpha", (6,)), T("beta", (6,))))
    case("gc.refuse.sign.tensor_input")(lambda T: ops.grouped_conv2d_sign(T("x", GP.x), T("w", GP.w), None, T("alpha", (12,)),
                                                                          T("beta", (12,)), **GEO, groups=4, shape=GP.x))


_add_cases()


# ---- the recorder ----------------------------------------------------------------------------------------------------------------

WORK = ("qt_dwconv2d_grad_weight_work_floats", "qt_gconv2d_grad_weight_work_floats")


@contextlib.contextmanager
def _recording(device, calls, labels):
    lib, real_call, real_stream = _lib.load(), _lib.call, ops._stream

    def encode(name, args):
        argtypes = _lib.SIGNATURES[name][1]
        assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
        out = []
        for i, (a, ct) in enumerate(zip(args, argtypes)):
            if ct is not ctypes.c_void_p:
                assert isinstance(a, (int, float)) and not isinstance(a, bool), f"{name}: argument {i} is {a!r}"
                out.append(a)
            elif i == len(args) - 1:
                out.append("stream")
            else:
                out.append(None if a is None else labels.get(a, "other"))
        return [name, out]

    def call(name, *args):
        calls.append(encode(name, args))
        if device is not None:
            real_call(name, *args)

    def work(name, real):
        def fn(*args):
            calls.append(encode(name, args))
            return real(*args)
        return fn

    reals = {n: getattr(lib, n) for n in WORK}
    _lib.call = call
    if device is None:
        ops._stream = lambda dev: 0
    for n, real in reals.items():
        setattr(lib, n, work(n, real))
    try:
        yield
    finally:
        _lib.call, ops._stream = real_call, real_stream
        for n, real in reals.items():
            setattr(lib, n, real)


def record_calls(device=None, names=None):
    """{case name: [[entry, [args ...]], ...] or {"raises": ..., "text": ...}} of ``names`` (default: every case)."""
    out = {}
    for name in (names or CASES):
        T = Tensors(device)
        with _recording(device, T.calls, T.labels):
            try:
                CASES[name](T)
                out[name] = T.calls
            except Exception as e:              # noqa: BLE001 - the type and the text ARE the recorded result
                # the device's name and the stand-in's class are the only things in a message that differ between the two modes
                text = str(e).replace(str(device or "cpu"), "DEV").replace(repr(_Dev), repr(torch.Tensor))
                out[name] = {"raises": type(e).__name__, "text": text}
    return out


# ---- the pure shape predicates ---------------------------------------------------------------------------------------------------

_C = 66
_M = 1 << 10
PREDICATE_CASES = [
    # tests/test_dwconv_cpu.py
    ((2, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8), ((2, 8, 7, 7), (24, 1, 3, 3), (2, 1), (2, 0), 2, 8), ((1, 1, 5, 5), (2, 1, 1, 1), 1, 0, 1, 1),
    ((2, 8, 9, 9), (8, 1, 7, 7), 1, 3, 1, 8), ((2, 8, 7, 7), (8, 2, 3, 3), 1, 1, 1, 4), ((2, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 4),
    ((2, 8, 12, 12), (8, 1, 5, 10), 1, 5, 1, 8), ((2, 8, 7, 7), (8, 1, 3, 3), 1, "same", 1, 8), ((2, 8, 7, 7), (8, 1, 3, 3), 1, "valid", 1, 8),
    ((2, 8, 7, 7), (12, 1, 3, 3), 1, 1, 1, 8), ((8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8), ((2, 8, 2, 2), (8, 1, 5, 5), 1, 0, 1, 8),
    ((0, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8), ((1 << 12, _M, 1 << 5, 1 << 4), (_M, 1, 3, 3), 1, 1, 1, _M),
    ((1 << 12, _M, 1 << 4, 1 << 4), (_M, 1, 3, 3), 1, 1, 1, _M), ((1 << 12, _M, 1 << 4, 1 << 4), (1 << 11, 1, 3, 3), 1, 1, 1, _M),
    ((256, 1024, 7, 7), (2048, 1, 3, 3), 1, 1, 1, 1024),
    # tests/test_gconv_cpu.py
    ((2, 12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 4), ((2, 12, 7, 7), (20, 3, 3, 3), (2, 1), (2, 0), (1, 2), 4), ((2, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1, 8),
    ((1, 5, 5, 5), (2, 5, 1, 1), 1, 0, 1, 1), ((1, 64, 9, 9), (2, 32, 4, 4), 1, 0, 1, 2), ((1, 66, 9, 9), (2, 33, 3, 3), 1, 0, 1, 2),
    ((1, 64, 9, 9), (2, 32, 3, 6), 1, 0, 1, 2), ((1, 20, 9, 9), (2, 10, 7, 7), 1, 3, 1, 2), ((1, 22, 9, 9), (2, 11, 7, 7), 1, 3, 1, 2),
    ((2, 8, 12, 12), (8, 2, 5, 10), 1, 5, 1, 4), ((2, 12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 2), ((2, 12, 7, 7), (10, 3, 3, 3), 1, 1, 1, 4),
    ((2, 12, 7, 7), (8, 3, 3, 3), 1, "same", 1, 4), ((12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 4), ((2, 12, 2, 2), (8, 3, 5, 5), 1, 0, 1, 4),
    ((0, 12, 7, 7), (8, 3, 3, 3), 1, 1, 1, 4), ((2, 12, 7, 7), (8, 3, 3, 3), 0, 1, 1, 4),
    ((1 << 12, _M, 1 << 5, 1 << 4), (_M, 2, 3, 3), 1, 1, 1, 1 << 9), ((1 << 12, _M, 1 << 4, 1 << 4), (_M, 2, 3, 3), 1, 1, 1, 1 << 9),
    ((1 << 12, _M, 1 << 4, 1 << 4), (1 << 11, 2, 3, 3), 1, 1, 1, 1 << 9), ((1, 8, 1, 1), (2 * ops.DW_MAX_CHANNELS, 2, 1, 1), 1, 0, 1, 4),
    ((256, 128, 56, 56), (128, 4, 3, 3), 1, 1, 1, 32),
    # plane-sized groups, and values the limits check must refuse on either family
    ((2, 8, 7, 7), (12, 2, 3, 3), 1, 1, 1, 4), ((2, 16, 7, 7), (8, 4, 3, 3), 1, 1, 1, 4), ((2, 32, 7, 7), (8, 8, 3, 3), 1, 1, 1, 4),
    ((2, 8, 7, 7), (8, 1, 3, 3), 1, -1, 1, 8), ((2, 8, 7, 7), (8, 1, 3, 3), 1, 1, 1 << 24, 8), ((2, 8, 7, 7), (8, 1, 3, 3), 1, (1, 2, 3), 1, 8),
    ((2, 8, 7, 7), (8, 1, 3, 3), 1, None, 1, 8), ((2, 8, 7, 7), (8, 1, 3, 3), (), 1, 1, 8),
] + [
    # groups x channels per group x taps, in channel counts where C == groups * cin_g holds and where it does not
    ((1, c, 12, 12), (_C, cin_g, *k), 1, 5, 1, g)
    for c in (_C, 2, 4) for g in (1, 2, c) for cin_g in (1, 2, 33) for k in ((7, 7), (5, 10))
]

PREDICATES = ("depthwise_applicable", "grouped_applicable", "grouped_planes_applicable", "grouped_codes_applicable")


def record_predicates():
    """{repr(arguments): [the four predicates' values]} over ``PREDICATE_CASES``."""
    return {repr(a): [bool(getattr(ops, p)(*a)) for p in PREDICATES] for a in PREDICATE_CASES}


if __name__ == "__main__":
    dev = torch.device("cuda:0") if len(sys.argv) > 2 and sys.argv[2] == "gpu" else None
    with open(sys.argv[1], "w", encoding="utf-8") as fh:
        json.dump({"calls": record_calls(dev), "predicates": record_predicates()}, fh, indent=0, sort_keys=True)
        fh.write("\n")
