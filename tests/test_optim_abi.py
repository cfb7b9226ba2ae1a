"""Argument validation of the two training-update entries (qt_optim_sgd_f32 / qt_optim_adam_f32) in every form: a status, never a
crash, in the order include/qt_hip.h states.  No GPU needed, and none is used where there is one: every call here either ends in
a negative status or has nothing to enqueue (n == 0, or only empty tensors)."""
import ctypes

import pytest

import _optim_abi as A
from _optim_abi import ALIGNMENT, INVALID, table
from pytorch_quantize_impls_amd import _lib, ops

every_form = pytest.mark.parametrize("form", list(A.FORMS.values()), ids=list(A.FORMS))
every_rule = pytest.mark.parametrize("rule", ["sgd", "adam"])
EMPTY = dict(numel=0, p=None, g=None)
PLANE = dict(kind=1, words=0x5000, rows=2, K=32, ld=4)


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_descriptor_layout_matches_the_header(lib):
    assert ctypes.sizeof(ops._OptimTensor) == 96 and ops._OptimTensor.kind.offset == 88
    assert lib.qt_optim_chunk_capacity() == ops.optim_chunk_capacity() >= 1


def test_entries_and_form_bits_are_declared_and_bound(lib):
    declared = _lib.header_declared_functions()
    for name in A.ENTRIES.values():
        assert name in declared and name in _lib.SIGNATURES
        fn = getattr(lib, name)                                  # exported
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0]
        assert _lib.HEADER.functions[name][1][A.FORM_ARG] == ("form", ctypes.c_int)
    assert (A.SCALARS_DEV, A.GSCALE, A.SKIP, _lib.DEFINES["QT_OPTIM_FORM_MASK"]) == (1, 2, 4, 7)
    assert sorted(A.FORMS.values()) == list(range(8))
    gone = [n for n in declared if n.startswith("qt_optim_") and ("_dev" in n or "_clip" in n)]
    assert not gone                                              # one entry per rule: no per-form entries next to them


@every_rule
@every_form
def test_tables(lib, rule, form):
    up = lambda tab, n, **kw: A.update(lib, rule, tab, n, form, **kw)    # noqa: E731
    assert up(None, 0) == 0                                      # nothing to do
    assert up(None, 3) == INVALID                                # null table with n > 0
    assert up(table(), -1) == INVALID
    assert up(table(**EMPTY), 1) == 0                            # an empty tensor is skipped
    assert up(table(numel=-4), 1) == INVALID
    assert up(table(p=None), 1) == INVALID and up(table(g=None), 1) == INVALID
    assert up(table(p=0x1002), 1) == ALIGNMENT                   # not even element-aligned
    assert up(table(kind=3), 1) == INVALID
    if rule == "sgd":
        assert up(table(s0=None), 1, momentum=0.9) == INVALID    # momentum needs its buffer
        assert up(table(), 1, momentum=0.0, nesterov=1) == INVALID
    else:
        assert up(table(s0=None), 1) == INVALID and up(table(s1=None), 1) == INVALID


@every_rule
@every_form
def test_planes(lib, rule, form):
    up = lambda **fields: A.update(lib, rule, table(**fields), 1, form)  # noqa: E731
    assert up(kind=3) == INVALID and up(kind=-1) == INVALID
    assert up(**{**PLANE, "ld": 3}) == ALIGNMENT                 # ld < ceil(K / 8)
    assert up(**{**PLANE, "ld": 6}) == ALIGNMENT                 # ld % 4 != 0
    assert up(**{**PLANE, "words": 0x5004}) == ALIGNMENT
    assert up(**{**PLANE, "words": None}) == INVALID
    assert up(**{**PLANE, "rows": 3}) == INVALID                 # rows * K != numel
    assert up(**{**PLANE, "rows": -2, "K": -32}) == INVALID
    assert up(**{**PLANE, "kind": 2, "ld": 2}) == ALIGNMENT


@every_rule
@every_form
def test_optional_pointers(lib, rule, form):
    """Each of the three pointers is there exactly when its bit is set; what the form implies for the other two is left alone."""
    up = lambda tab, n, **kw: A.update(lib, rule, tab, n, form, **kw)    # noqa: E731
    nothing = dict(scalars=None, gscale=None, skip=None)
    assert up(None, 0, **nothing) == 0                           # n == 0: whatever they are
    assert up(table(**EMPTY), 1) == 0                            # every flagged pointer given, only empty tensors
    for name, bit in A.BIT.items():
        odd = A.FAKE[name] + 2
        assert up(None, 0, **{name: odd}) == 0
        assert up(table(), -1, **{name: odd}) == INVALID         # the count's status first
        assert up(table(), -1, **{name: None}) == INVALID
        if form & bit:
            assert up(table(), 1, **{name: None}) == INVALID     # flagged and null
            assert up(table(), 1, **{name: odd}) == ALIGNMENT
        else:
            assert up(table(), 1, **{name: A.FAKE[name]}) == INVALID     # not flagged and non-null
            assert up(table(), 1, **{name: odd}) == INVALID
            assert up(table(**EMPTY), 1, **{name: A.FAKE[name]}) == INVALID


@every_rule
def test_unknown_form_bits(lib, rule):
    for form in (0x8, 0x10, A.GSCALE | 0x8, 0x7 | 0x100, -1, 1 << 30):
        assert A.update(lib, rule, table(), 1, form) == INVALID, form
        assert A.update(lib, rule, None, 0, form) == INVALID, form           # refused even where there is nothing to do
        assert A.update(lib, rule, table(**EMPTY), 1, form) == INVALID, form


@every_rule
def test_the_order_of_the_checks(lib, rule):
    """A later check's status never hides an earlier one's: the two statuses tell the steps apart."""
    all3 = A.SCALARS_DEV | A.GSCALE | A.SKIP
    up = lambda tab, n, form=all3, **kw: A.update(lib, rule, tab, n, form, **kw)     # noqa: E731
    odd = {k: v + 2 for k, v in A.FAKE.items()}
    if rule == "sgd":                                            # 1. nesterov without momentum, before n == 0
        assert up(None, 0, nesterov=1) == INVALID and up(None, 0, form=0, nesterov=1) == INVALID
    assert up(None, 0, form=all3 | 0x8) == INVALID               # 2. the form's bits, before n == 0
    assert up(None, 0, **odd) == 0                               # 3. n == 0, before the pointers
    assert up(table(), -1, **odd) == INVALID                     # 4. n < 0, before the pointers
    # 5. scalars, then gscale, then skip
    assert up(table(), 1, scalars=odd["scalars"], gscale=None) == ALIGNMENT
    assert up(table(), 1, scalars=None, gscale=odd["gscale"]) == INVALID
    assert up(table(), 1, gscale=odd["gscale"], skip=None) == ALIGNMENT
    assert up(table(), 1, gscale=None, skip=odd["skip"]) == INVALID
    assert up(table(), 1, form=A.GSCALE, scalars=A.FAKE["scalars"], gscale=odd["gscale"]) == INVALID     # unflagged scalars first
    assert up(table(), 1, form=A.SCALARS_DEV, scalars=odd["scalars"], skip=A.FAKE["skip"]) == ALIGNMENT
    # ... all three before 6. the table
    assert up(table(p=None), 1, skip=odd["skip"]) == ALIGNMENT
    assert up(table(p=0x1002), 1, skip=None) == INVALID
    assert up(None, 3, skip=odd["skip"]) == ALIGNMENT
    assert up(table(p=0x1002), 1) == ALIGNMENT and up(table(p=None), 1) == INVALID


def test_wrappers_reject_host_tensors():
    import torch
    p, g = torch.zeros(4), torch.zeros(4)
    with pytest.raises(TypeError):
        ops.optim_step_sgd([p], [g], lr=0.1)
    with pytest.raises(TypeError):
        ops.optim_step_adam([p], [g], [g.clone()], [g.clone()], [1], lr=0.1)
