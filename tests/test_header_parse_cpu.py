"""_lib.parse_header(): the one reader of include/qt_hip.h that the ctypes signatures, the QT_* constants and the structures of
the package come from.  Synthetic header text shows which spellings it takes and that it refuses the rest by name; a handful of
entry points of the real header are written out here by hand (tests/test_half_cpu.py and tests/test_loglin_lazy_cpu.py keep
their own, independent parsers for their slices).  No GPU, no library: text in, ctypes out."""
import ctypes
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

import pytest

from pytorch_quantize_impls_amd import _lib

SYNTHETIC = """
/* a header in the style of qt_hip.h
 * int qt_in_block_comment(int a);
 */
#ifndef QT_SYNTH_H
#define QT_SYNTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* qt_stream_t; /* hipStream_t */
typedef enum qt_status { QT_OK = 0, QT_ERR_INVALID_ARG = -1 } qt_status;
enum { QT_KIND_A = 0, QT_KIND_B = 1 };
#define QT_TABLE_MAX 64
#define QT_SOME_FLAG 0x20     /* a flag bit */
#define QT_NOT_A_NUMBER (1 << 3)
// int qt_in_line_comment(float b);
int qt_version(void);
const char* qt_strerror(int status);
int qt_device_info(char* name, int cap);
int64_t qt_work_words(int64_t rows,
                      int64_t K);
int qt_many_lines(const float* x, int64_t ldx,      /* the input */
                  uint16_t* A, const int8_t* codes,
                  int32_t mask, float thr,
                  qt_stream_t stream);
typedef struct qt_pair {
    const float* p;
    int64_t ld, rows, K;
    float lo, hi;
    int32_t kind;
} qt_pair;
int qt_flags_or(const int32_t* const* flags, const qt_pair* table, int const n, qt_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_accepted_forms():
    functions, defines, structs = _lib.parse_header(SYNTHETIC)
    assert list(functions) == ["qt_version", "qt_strerror", "qt_device_info", "qt_work_words", "qt_many_lines", "qt_flags_or"]
    assert functions["qt_version"] == (c_int, [])
    assert functions["qt_strerror"] == (c_char_p, [("status", c_int)])
    assert functions["qt_device_info"] == (c_int, [("name", c_char_p), ("cap", c_int)])
    assert functions["qt_work_words"] == (c_int64, [("rows", c_int64), ("K", c_int64)])
    assert functions["qt_many_lines"] == (c_int, [("x", c_void_p), ("ldx", c_int64), ("A", c_void_p), ("codes", c_void_p),
                                                  ("mask", c_int32), ("thr", c_float), ("stream", c_void_p)])
    assert functions["qt_flags_or"] == (c_int, [("flags", c_void_p), ("table", c_void_p), ("n", c_int), ("stream", c_void_p)])
    assert defines == {"QT_TABLE_MAX": 64, "QT_SOME_FLAG": 0x20}          # integer literals only; enums are not #defines
    assert structs == {"qt_pair": [("p", c_void_p), ("ld", c_int64), ("rows", c_int64), ("K", c_int64), ("lo", c_float),
                                   ("hi", c_float), ("kind", c_int32)]}


@pytest.mark.parametrize("declaration, named", [
    ("int qt_bad_scalar(const float* x, double eps);", "qt_bad_scalar"),              # a scalar outside the type map
    ("int qt_bad_unsigned(uint32_t n);", "qt_bad_unsigned"),                          # uint32_t is known as a pointee only
    ("void qt_bad_return(int n);", "qt_bad_return"),                                  # no void entry points
    ("int qt_bad_callback(void (*done)(int), int n);", "qt_bad_callback"),            # not a prototype the pattern takes
    ("int qt_bad_array(const float x[4]);", "qt_bad_array"),
    ("int qt_bad_unnamed(int64_t);", "qt_bad_unnamed"),
    ("int qt_version(int again);", "qt_version"),                                     # declared twice
    ("typedef struct qt_bad_struct { float* a, b; } qt_bad_struct;", "qt_bad_struct"),
    ("static inline int qt_bad_inline(int n) { return n; }", "qt_bad_inline"),
])
def test_rejected_forms(declaration, named):
    text = SYNTHETIC.replace("int qt_device_info(char* name, int cap);", declaration)
    assert text != SYNTHETIC
    with pytest.raises(_lib.QtLibraryError, match=named):
        _lib.parse_header(text)


def test_missing_header_names_the_path(tmp_path):
    path = str(tmp_path / "no_such_qt_hip.h")
    with pytest.raises(_lib.QtLibraryError, match="no_such_qt_hip.h"):
        _lib.header_declared_functions(path)


def test_real_header_anchors():
    S = _lib.SIGNATURES
    assert sorted(S) == _lib.header_declared_functions() and len(S) == len(_lib.HEADER.functions)
    assert S["qt_version"] == (c_int, [])
    assert S["qt_strerror"] == (c_char_p, [c_int])
    assert S["qt_device_info"] == (c_int, [c_char_p, c_int])
    assert S["qt_optim_grad_norm_work_floats"] == (c_int64, [c_void_p, c_int64])
    assert S["qt_flags_or_i32"] == (c_int, [c_void_p, c_int64, c_void_p, c_void_p])
    assert S["qt_poison_f32"] == (c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_void_p])
    assert _lib.HEADER.functions["qt_poison_f32"][1][2] == ("mask", c_int32)
    restype, argtypes = S["qt_conv2d_implicit_codes"]
    assert restype is c_int and len(argtypes) == 44
    assert [i for i, t in enumerate(argtypes) if t is c_float] == [17, 27]          # scale, res_scale
    names = [n for n, _ in _lib.HEADER.functions["qt_conv2d_implicit_codes"][1]]
    assert (names[0], names[17], names[27], names[42], names[43]) == ("elem", "scale", "res_scale", "flags", "stream")


def test_real_header_structs():
    from pytorch_quantize_impls_amd import ops
    want = [("p", c_void_p), ("g", c_void_p), ("s0", c_void_p), ("s1", c_void_p), ("numel", c_int64), ("words", c_void_p),
            ("ld", c_int64), ("rows", c_int64), ("K", c_int64), ("lo", c_float), ("hi", c_float), ("c0", c_float), ("c1", c_float),
            ("kind", c_int32), ("flags", c_int32)]
    assert _lib.STRUCTS["qt_optim_tensor"] == want and ops._OptimTensor._fields_ == want
    assert ctypes.sizeof(ops._OptimTensor) == 5 * 8 + 8 + 3 * 8 + 4 * 4 + 2 * 4 == 96     # the C layout: no padding anywhere
    assert _lib.STRUCTS["qt_reg_term"] == [("code", c_int32), ("t1", c_float), ("t2", c_float), ("c", c_float)]
    term = type("qt_reg_term", (ctypes.Structure,), {"_fields_": _lib.STRUCTS["qt_reg_term"]})
    assert ctypes.sizeof(term) == 16            # one row of the [n, 4] int32 tables ops.weight_reg hands over


def test_real_header_defines_reach_ops():
    from pytorch_quantize_impls_amd import ops
    import torch
    D = _lib.DEFINES
    assert (D["QT_LEVELS_MAX"], D["QT_REG_TERMS_MAX"]) == (ops.LEVELS_MAX, ops.REG_TERMS_MAX) == (64, 128)
    assert [D["QT_EPI_" + n] for n in ("PLAIN", "BITS", "NIB", "CODES", "HALO_BN", "LEVELS", "HALF_BF16", "HALF_F16")] == list(range(8))
    assert (ops.EPI_PLAIN, ops.EPI_BITS, ops.EPI_NIB, ops.EPI_CODES, ops.EPI_HALO_BN, ops.EPI_LEVELS, ops.EPI_HALF_BF16,
            ops.EPI_HALF_F16) == tuple(range(8))
    assert ops._DTYPE_CODE == {torch.bfloat16: 1, torch.float16: 2} and D["QT_DTYPE_F32"] == 0
    assert (ops.CONV_NO_DEEP_RING, ops.CONV_COMPARE_THRESHOLDS, ops.CONV_NO_DIRECT_CODES, ops.CONV_FLAGS_MASK) == (0x10, 0x20, 0x40, 0x70)
