"""Host side of ``GraphedTrainStep(recover=True)``: the status codes of qt_flags_or_i32 (nothing that passes validation here has
anything to launch), the thread-local collector of trusted verdict flags (``_fused.flag_sink``) and what stays refused.  The
statuses of the guarded training update (QT_OPTIM_SKIP) are in tests/test_optim_abi.py.  No GPU needed."""
import ctypes
import threading

import pytest
import torch

from pytorch_quantize_impls_amd import _lib, ops, utils
from pytorch_quantize_impls_amd.functions import _fused
from pytorch_quantize_impls_amd.functions.common import QtFunction

INVALID, ALIGNMENT = -1, -2


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_entries_are_declared_and_bound(lib):
    declared = _lib.header_declared_functions()
    for name in ("qt_optim_sgd_f32", "qt_optim_adam_f32", "qt_flags_or_i32", "qt_flags_chunk_capacity"):
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ctypes.sizeof(ops._OptimTensor) == 96            # the guarded form takes the descriptor as it is
    # 8 bytes per pointer, the guard pointer and the count next to them: inside HIP's 4096-byte argument block
    assert 1 <= ops.flags_chunk_capacity() and 8 * ops.flags_chunk_capacity() + 16 <= 4096


def test_flags_or_status_codes(lib):
    ptrs = (ctypes.c_void_p * 3)(0x1000, 0x2000, 0x3000)
    tab = ctypes.addressof(ptrs)
    assert lib.qt_flags_or_i32(None, 0, None, None) == 0                                 # nothing to fold
    assert lib.qt_flags_or_i32(tab, 0, 0x8002, None) == 0
    assert lib.qt_flags_or_i32(None, 3, 0x8000, None) == INVALID
    assert lib.qt_flags_or_i32(tab, 3, None, None) == INVALID
    assert lib.qt_flags_or_i32(tab, -1, 0x8000, None) == INVALID
    assert lib.qt_flags_or_i32(tab, 3, 0x8002, None) == ALIGNMENT
    ptrs[2] = 0x3002
    assert lib.qt_flags_or_i32(tab, 3, 0x8000, None) == ALIGNMENT                        # the last pointer: all are looked at first
    ptrs[2] = None
    assert lib.qt_flags_or_i32(tab, 3, 0x8000, None) == INVALID


def test_wrappers_reject_host_tensors():
    p, g = torch.zeros(4), torch.zeros(4)
    with pytest.raises(TypeError):
        ops.flags_or([torch.zeros(1, dtype=torch.int32)], torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.optim_step_sgd_dev([p], [g], None, torch.zeros(1), skip=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.optim_step_adam_dev([p], [g], [g.clone()], [g.clone()], torch.zeros(2), skip=torch.zeros(1, dtype=torch.int32))


# ---- flag_sink ------------------------------------------------------------------------------------------------------------------

def test_no_sink_is_a_no_op():
    f = torch.zeros(1, dtype=torch.int32)
    assert _fused.current_flag_sink() is None
    assert _fused.register_flag(f) is f
    assert _fused.current_flag_sink() is None


def test_sink_collects_once_by_identity_and_keeps_the_tensors():
    a, b = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)          # equal values, two tensors
    with _fused.flag_sink() as flags:
        for f in (a, b, a, a, b):
            assert _fused.register_flag(f) is f
        _fused.register_flag(None)                                                      # "no flag" is not a flag
    assert len(flags) == 2 and flags.flags[0] is a and flags.flags[1] is b
    ida = id(a)
    del a
    assert id(flags.flags[0]) == ida                                                    # still alive in the sink
    assert _fused.current_flag_sink() is None


def test_sinks_nest_and_the_innermost_gets_the_flag():
    a, b, c = (torch.zeros(1, dtype=torch.int32) for _ in range(3))
    with _fused.flag_sink() as outer:
        _fused.register_flag(a)
        with _fused.flag_sink() as inner:
            _fused.register_flag(b)
            assert _fused.current_flag_sink() is inner
        assert _fused.current_flag_sink() is outer
        _fused.register_flag(c)
    assert [id(f) for f in outer] == [id(a), id(c)] and [id(f) for f in inner] == [id(b)]


def test_sink_is_thread_local():
    a, b = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    seen = {}

    def other():
        seen["sink"] = _fused.current_flag_sink()
        _fused.register_flag(b)                                                         # no sink in THIS thread: dropped

    with _fused.flag_sink() as flags:
        th = threading.Thread(target=other)
        th.start()
        th.join()
        _fused.register_flag(a)
    assert seen["sink"] is None and [id(f) for f in flags] == [id(a)]


class _Registers(QtFunction):
    """Stand-in for a layer Function: hands one flag out in forward, one in backward, and reports the backward's thread."""
    FWD = torch.zeros(1, dtype=torch.int32)
    BWD = torch.zeros(1, dtype=torch.int32)
    threads = []

    @staticmethod
    def forward(ctx, x):
        _fused.register_flag(_Registers.FWD)
        return x * 2.0

    @staticmethod
    def backward(ctx, g):
        _Registers.threads.append(threading.get_ident())
        _fused.register_flag(_Registers.BWD)
        return g * 2.0


def test_sink_is_carried_into_the_backward_on_another_thread():
    x = torch.ones(3, requires_grad=True)
    with _fused.flag_sink() as flags:
        y = _Registers.apply(x).sum()
    assert [id(f) for f in flags] == [id(_Registers.FWD)]
    # the backward runs after the sink was closed, on a thread that never opened it: what the autograd engine does for device graphs
    th = threading.Thread(target=y.backward)
    th.start()
    th.join()
    assert _Registers.threads[-1] != threading.get_ident()
    assert [id(f) for f in flags] == [id(_Registers.FWD), id(_Registers.BWD)]
    assert torch.equal(x.grad, torch.full((3,), 2.0)) and _fused.current_flag_sink() is None
    # built outside any sink: the backward registers nowhere
    x.grad = None
    _Registers.apply(x).sum().backward()
    assert len(flags) == 2


def test_detectors_register_only_trusted_flags(monkeypatch):
    """detect_pm1 under a sink: a verdict that was just ASKED hands out no flag and registers none; a remembered one hands out the
    check's flag and registers exactly that tensor.  (The device calls are replaced: the question is who registers what.)"""
    flag = torch.zeros(1, dtype=torch.int32)
    monkeypatch.setattr(ops, "is_pm1", lambda x: True)
    monkeypatch.setattr(ops, "check_pm1", lambda x: flag)
    w, x = torch.zeros(2, 4), torch.ones(3, 4)
    _fused.reset_detection(w)
    with _fused.detect_scope("remember"), _fused.flag_sink() as flags:
        assert _fused.detect_pm1(x, w) == (True, None) and len(flags) == 0
        ok, got = _fused.detect_pm1(x, w)
        assert ok and got is flag and [id(f) for f in flags] == [id(flag)]
    with _fused.detect_scope("verify"), _fused.flag_sink() as flags:
        assert _fused.detect_pm1(x, w) == (True, None) and len(flags) == 0
    _fused.reset_detection(w)


# ---- what stays refused ---------------------------------------------------------------------------------------------------------

def test_recover_on_host_tensors_raises_as_without_it():
    model = torch.nn.Linear(4, 2)
    x, t = torch.zeros(3, 4), torch.zeros(3, dtype=torch.long)
    loss = torch.nn.functional.cross_entropy
    with pytest.raises(TypeError) as plain:
        utils.GraphedTrainStep(model, loss, x, t)
    with pytest.raises(TypeError) as rec:
        utils.GraphedTrainStep(model, loss, x, t, recover=True)
    assert str(plain.value) == str(rec.value) == "graph capture needs device tensors"
    with pytest.raises(TypeError, match=r"opt\.step\(\)"):
        utils.GraphedTrainStep(model, loss, x, t, optimizer=torch.optim.SGD(model.parameters(), lr=0.1), recover=True)


def test_recover_refuses_an_optimiser_whose_clamp_it_cannot_guard(monkeypatch):
    """A layer whose clamp() the clamp plan cannot restate runs as torch code inside the graph: the guard could not skip it.  The
    constructor refuses it before anything is captured — after the host-tensor check, so the stand-in input claims to be a
    device tensor; nothing ever touches it."""
    class Odd(torch.nn.Linear):
        def clamp(self):
            self.weight.data.clamp_(-0.5, 0.5)

    model = torch.nn.Sequential(Odd(4, 2))
    opt = utils.FusedQuantSGD(model, lr=0.1)
    assert [type(m).__name__ for m in opt._post_clamp] == ["Odd"]

    class FakeDevice(torch.Tensor):
        is_cuda = True

    x = torch.zeros(3, 4).as_subclass(FakeDevice)
    with pytest.raises(ValueError, match=r"recover=True.*clamp\(\) of \['Odd'\]"):
        utils.GraphedTrainStep(model, torch.nn.functional.cross_entropy, x, torch.zeros(3, dtype=torch.long), optimizer=opt,
                               recover=True)
