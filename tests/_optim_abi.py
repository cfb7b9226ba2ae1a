"""What the tests of the two training-update entries (qt_optim_sgd_f32 / qt_optim_adam_f32, include/qt_hip.h "Training update")
share: the form bits, a one-descriptor table of made-up addresses, one caller for both rules, and a recorder of the forms the
Python wrappers called the entries with."""
import contextlib
import ctypes

from pytorch_quantize_impls_amd import _lib, ops

INVALID, ALIGNMENT = -1, -2
SCALARS_DEV, GSCALE, SKIP = (_lib.DEFINES[k] for k in ("QT_OPTIM_SCALARS_DEV", "QT_OPTIM_GSCALE", "QT_OPTIM_SKIP"))
ENTRIES = {"sgd": "qt_optim_sgd_f32", "adam": "qt_optim_adam_f32"}
FORM_ARG = 2                                                  # `form` is argument 2 of both entries
# every combination of the three optional inputs, under the names the GPU tests use for them
FORMS = {"value": 0, "dev": SCALARS_DEV, "value_clip": GSCALE, "dev_clip": SCALARS_DEV | GSCALE, "value_guard": SKIP,
         "guard": SCALARS_DEV | SKIP, "value_guard_clip": GSCALE | SKIP, "guard_clip": SCALARS_DEV | GSCALE | SKIP}
# made-up device addresses: never dereferenced on the host, and no call that passes validation has anything to enqueue
FAKE = {"scalars": 0x6000, "gscale": 0x6100, "skip": 0x7000}
BIT = {"scalars": SCALARS_DEV, "gscale": GSCALE, "skip": SKIP}
GIVEN = object()                                              # "the fake address if the form flags this pointer, else null"


def table(n=1, **fields):
    tab = (ops._OptimTensor * n)()
    for e in tab:
        e.p, e.g, e.s0, e.s1, e.numel = 0x1000, 0x2000, 0x3000, 0x4000, 64
        e.lo, e.hi = float("-inf"), float("inf")
        for k, v in fields.items():
            setattr(e, k, v)
    return tab


def update(lib, rule, tab, n, form, momentum=0.0, nesterov=0, **pointers):
    """Status of one call of the entry of ``rule`` in ``form``.  ``pointers``: scalars= (SGD's lr_dev, Adam's coef), gscale=,
    skip= override what the form implies."""
    ptr = {k: pointers.pop(k, GIVEN) for k in FAKE}
    assert not pointers, pointers
    ptr = {k: ((FAKE[k] if form & BIT[k] else None) if v is GIVEN else v) for k, v in ptr.items()}
    t = ctypes.addressof(tab) if tab is not None else None
    if rule == "sgd":
        return lib.qt_optim_sgd_f32(t, n, form, 0.1, ptr["scalars"], ptr["gscale"], ptr["skip"], momentum, 0.0, nesterov, None)
    return lib.qt_optim_adam_f32(t, n, form, ptr["scalars"], ptr["gscale"], ptr["skip"], 0.9, 0.1, 0.999, 0.001, 1e-8, 0.0, None)


@contextlib.contextmanager
def recorded_forms():
    """[(entry, form)] of every successful call of an update entry made through ``_lib.call`` inside the block."""
    calls, real = [], _lib.call

    def call(name, *args):
        real(name, *args)
        if name in ENTRIES.values():
            calls.append((name, args[FORM_ARG]))

    _lib.call = call
    try:
        yield calls
    finally:
        _lib.call = real
