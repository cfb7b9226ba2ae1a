"""Argument validation of the training-update entries (qt_optim_sgd_f32 / qt_optim_adam_f32): a status, never a crash, and
nothing is launched for a table that does not pass (no GPU needed)."""
import ctypes

import pytest

from pytorch_quantize_impls_amd import _lib, ops

INVALID, ALIGNMENT = -1, -2


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _sgd(lib, tab, n, momentum=0.0, nesterov=0):
    ptr = ctypes.addressof(tab) if tab is not None else None
    return lib.qt_optim_sgd_f32(ptr, n, 0.1, momentum, 0.0, nesterov, None)


def _adam(lib, tab, n):
    ptr = ctypes.addressof(tab) if tab is not None else None
    return lib.qt_optim_adam_f32(ptr, n, 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, None)


def _table(**fields):
    tab = (ops._OptimTensor * 1)()
    e = tab[0]
    e.p, e.g, e.s0, e.s1, e.numel = 0x1000, 0x2000, 0x3000, 0x4000, 64
    e.lo, e.hi = float("-inf"), float("inf")
    for k, v in fields.items():
        setattr(e, k, v)
    return tab


def test_descriptor_layout_matches_the_header(lib):
    assert ctypes.sizeof(ops._OptimTensor) == 96 and ops._OptimTensor.kind.offset == 88
    assert lib.qt_optim_chunk_capacity() == ops.optim_chunk_capacity() >= 1


def test_tables(lib):
    assert _sgd(lib, None, 0) == 0 and _adam(lib, None, 0) == 0                 # nothing to do
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
    import torch
    p, g = torch.zeros(4), torch.zeros(4)
    with pytest.raises(TypeError):
        ops.optim_step_sgd([p], [g], lr=0.1)
    with pytest.raises(TypeError):
        ops.optim_step_adam([p], [g], [g.clone()], [g.clone()], [1], lr=0.1)
