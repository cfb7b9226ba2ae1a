"""What feeds a training update that reads its per-step scalars from device memory (QT_OPTIM_SCALARS_DEV): the statuses of the
scalar writer, the wrappers' refusal of host tensors, and the bias-correction helper both forms of the Adam update share.  The
statuses of the update entries themselves, in every form, are in tests/test_optim_abi.py.  No GPU needed."""
import ctypes
import math

import pytest
import torch

from pytorch_quantize_impls_amd import _lib, ops

INVALID, ALIGNMENT = -1, -2
@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_entries_are_declared_and_bound(lib):
    declared = _lib.header_declared_functions()
    for name in ("qt_optim_sgd_f32", "qt_optim_adam_f32", "qt_optim_scalars_f32"):
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ctypes.sizeof(ops._OptimTensor) == 96            # one descriptor for every form


def test_scalar_writer(lib):
    v = (ctypes.c_float * 4)(1, 2, 3, 4)
    host = ctypes.addressof(v)
    assert lib.qt_optim_scalars_f32(None, None, 0, None) == 0                                   # nothing to write
    assert lib.qt_optim_scalars_f32(None, host, 4, None) == INVALID and lib.qt_optim_scalars_f32(0x1000, None, 4, None) == INVALID
    assert lib.qt_optim_scalars_f32(0x1000, host, -1, None) == INVALID
    assert lib.qt_optim_scalars_f32(0x1002, host, 4, None) == ALIGNMENT
    with pytest.raises(TypeError):
        ops.optim_write_scalars(torch.zeros(4), [1.0])                                           # a host destination


def test_wrappers_reject_host_tensors():
    p, g = torch.zeros(4), torch.zeros(4)
    with pytest.raises(TypeError):
        ops.optim_step_sgd_dev([p], [g], None, torch.zeros(1))
    with pytest.raises(TypeError):
        ops.optim_step_adam_dev([p], [g], [g.clone()], [g.clone()], torch.zeros(2))


@pytest.mark.parametrize("lr,betas", [(1e-3, (0.9, 0.999)), (3e-3, (0.8, 0.95))])
def test_adam_coefficients_are_the_closed_form(lr, betas):
    steps = [1, 2, 10, 1000, 2, 1]
    got = ops.adam_coefficients(steps, lr, betas)
    assert len(got) == len(steps) and got[1] == got[4] and got[0] == got[5]
    for t, (c0, c1) in zip(steps, got):
        assert c0 == lr / (1.0 - betas[0] ** t) and c1 == math.sqrt(1.0 - betas[1] ** t)


def test_optim_step_adam_writes_the_helper_values_into_its_descriptors(monkeypatch):
    """The by-value wrapper fills c0 / c1 from the same helper: its ctypes table is read back through a stubbed ``_lib.call`` (the
    table is built by ``_optim_table``, replaced here by one that needs no device tensors)."""
    steps, lr, betas = [1, 2, 10, 1000], 2e-3, (0.85, 0.97)
    seen = {}

    def fake_table(params, grads, s0, s1, clamps, planes):
        return (ops._OptimTensor * len(params))(), torch.device("cpu")

    def fake_call(name, table, n, *rest):
        tab = (ops._OptimTensor * n).from_address(table)
        seen[name] = [(tab[i].c0, tab[i].c1) for i in range(n)]

    monkeypatch.setattr(ops, "_optim_table", fake_table)
    monkeypatch.setattr(ops._lib, "call", fake_call)
    monkeypatch.setattr(ops, "_on", lambda dev: ops._SAME_DEVICE)
    monkeypatch.setattr(ops, "_stream", lambda dev: None)
    t = [torch.zeros(1)] * len(steps)
    ops.optim_step_adam(t, t, t, t, steps, lr=lr, betas=betas)
    as_f32 = [(ctypes.c_float(c0).value, ctypes.c_float(c1).value) for c0, c1 in ops.adam_coefficients(steps, lr, betas)]
    assert seen["qt_optim_adam_f32"] == as_f32
