"""Argument validation of the training-update entries that read their per-step scalars from device memory
(qt_optim_sgd_dev_f32 / qt_optim_adam_dev_f32): every status of tests/test_optim_abi.py through the new entries, the scalar
pointers' own checks, and the bias-correction helper both forms of the Adam update share (no GPU needed: nothing that passes
validation here has a tensor to update)."""
import ctypes
import math

import pytest
import torch

from pytorch_quantize_impls_amd import _lib, ops

INVALID, ALIGNMENT = -1, -2
SCALARS = 0x6000            # never dereferenced on the host


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _sgd(lib, tab, n, momentum=0.0, nesterov=0, lr=SCALARS):
    ptr = ctypes.addressof(tab) if tab is not None else None
    return lib.qt_optim_sgd_dev_f32(ptr, n, lr, momentum, 0.0, nesterov, None)


def _adam(lib, tab, n, coef=SCALARS):
    ptr = ctypes.addressof(tab) if tab is not None else None
    return lib.qt_optim_adam_dev_f32(ptr, n, coef, 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, None)


def _table(**fields):
    tab = (ops._OptimTensor * 1)()
    e = tab[0]
    e.p, e.g, e.s0, e.s1, e.numel = 0x1000, 0x2000, 0x3000, 0x4000, 64
    e.lo, e.hi = float("-inf"), float("inf")
    for k, v in fields.items():
        setattr(e, k, v)
    return tab


def test_entries_are_declared_and_bound(lib):
    declared = _lib.header_declared_functions()
    for name in ("qt_optim_sgd_dev_f32", "qt_optim_adam_dev_f32", "qt_optim_scalars_f32"):
        assert name in declared and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert ctypes.sizeof(ops._OptimTensor) == 96            # the descriptor is the by-value entries'


def test_scalar_pointers(lib):
    assert _sgd(lib, None, 0, lr=None) == 0 and _adam(lib, None, 0, coef=None) == 0           # nothing to do
    assert _sgd(lib, None, 0, lr=0x1002) == 0 and _adam(lib, None, 0, coef=0x1002) == 0
    assert _sgd(lib, _table(), 1, lr=None) == INVALID and _adam(lib, _table(), 1, coef=None) == INVALID
    assert _sgd(lib, _table(), 1, lr=0x1002) == ALIGNMENT and _adam(lib, _table(), 1, coef=0x1002) == ALIGNMENT
    assert _sgd(lib, _table(), -1, lr=0x1002) == INVALID and _adam(lib, _table(), -1, coef=0x1002) == INVALID    # the table's status first
    assert _sgd(lib, _table(), -1, lr=None) == INVALID and _adam(lib, _table(), -1, coef=None) == INVALID
    assert _sgd(lib, _table(numel=0, p=None, g=None), 1) == 0 and _adam(lib, _table(numel=0, p=None, g=None), 1) == 0


def test_scalar_writer(lib):
    v = (ctypes.c_float * 4)(1, 2, 3, 4)
    host = ctypes.addressof(v)
    assert lib.qt_optim_scalars_f32(None, None, 0, None) == 0                                   # nothing to write
    assert lib.qt_optim_scalars_f32(None, host, 4, None) == INVALID and lib.qt_optim_scalars_f32(0x1000, None, 4, None) == INVALID
    assert lib.qt_optim_scalars_f32(0x1000, host, -1, None) == INVALID
    assert lib.qt_optim_scalars_f32(0x1002, host, 4, None) == ALIGNMENT
    with pytest.raises(TypeError):
        ops.optim_write_scalars(torch.zeros(4), [1.0])                                           # a host destination


def test_tables(lib):
    assert _sgd(lib, None, 3) == INVALID and _adam(lib, None, 3) == INVALID     # null table with n > 0
    assert _sgd(lib, _table(), -1) == INVALID and _adam(lib, _table(), -1) == INVALID
    assert _sgd(lib, _table(numel=0, p=None, g=None), 1) == 0                   # an empty tensor is skipped
    assert _sgd(lib, _table(numel=-4), 1) == INVALID
    assert _sgd(lib, _table(p=None), 1) == INVALID and _sgd(lib, _table(g=None), 1) == INVALID
    assert _sgd(lib, _table(s0=None), 1, momentum=0.9) == INVALID               # momentum needs its buffer
    assert _adam(lib, _table(s0=None), 1) == INVALID and _adam(lib, _table(s1=None), 1) == INVALID
    assert _sgd(lib, _table(p=0x1002), 1) == ALIGNMENT                          # not even element-aligned
    assert _sgd(lib, _table(), 1, momentum=0.0, nesterov=1) == INVALID


def test_planes(lib):
    ok = dict(kind=1, words=0x5000, rows=2, K=32, ld=4)
    assert _sgd(lib, _table(kind=3), 1) == INVALID and _sgd(lib, _table(kind=-1), 1) == INVALID
    assert _sgd(lib, _table(**{**ok, "ld": 3}), 1) == ALIGNMENT                 # ld < ceil(K / 8)
    assert _sgd(lib, _table(**{**ok, "ld": 6}), 1) == ALIGNMENT                 # ld % 4 != 0
    assert _sgd(lib, _table(**{**ok, "words": 0x5004}), 1) == ALIGNMENT
    assert _sgd(lib, _table(**{**ok, "words": None}), 1) == INVALID
    assert _sgd(lib, _table(**{**ok, "rows": 3}), 1) == INVALID                 # rows * K != numel
    assert _sgd(lib, _table(**{**ok, "rows": -2, "K": -32}), 1) == INVALID
    assert _adam(lib, _table(**{**ok, "kind": 2, "ld": 2}), 1) == ALIGNMENT


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
