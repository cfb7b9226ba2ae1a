"""Half-precision (bf16 / fp16) sign layers, the part that needs no GPU.

* The fixtures of tests/golden/make_golden_half.py (produced by the reference on CPU half tensors) obey the rule the HIP routes
  implement: every forward result is round-to-nearest-even of fl32(exact integer sum + bias), the quantiser edges follow the
  bit-pattern semantics of include/qt_hip.h.  Recomputed here with plain integer / fp64 arithmetic — this guards the fixtures
  and passes with or without the feature.
* The rounding cases really exercise the rounding (floors on the share of outputs that are not representable in the dtype,
  asserted on the data the file was made from), so a fixture that stopped doing so fails instead of passing vacuously:

      case                                      measured            asserted
      Linear K = 4097, bf16, binary / ternary   1.00 / 0.95-1.00    >= 0.5
      Linear K = 4097, fp16, binary / ternary   1.00 (ties) / 0.51+ >= 0.5 and ties present / >= 0.25
      conv, bf16, binary / ternary              0.87-0.88 / 0.92    >= 0.5
      conv, fp16, ternary                       0.36-0.40           >= 0.2
      conv, fp16, binary                        0.06 (K = 4800 even: the sums are even integers, nearly all representable) none

* include/qt_hip.h and _lib.SIGNATURES both declare the half packers, the half +-1 check and the output-dtype GEMM / conv entry
  points, with equal argument lists (fails without the feature).
"""
import json
import os
import re

import numpy as np
import pytest
import torch

import _half_cases as HC
from conftest import GOLDEN_DIR
from pytorch_quantize_impls_amd import _lib


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "golden_half_v1.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def gold_hashes():
    with open(os.path.join(GOLDEN_DIR, "golden_half_hashes.json")) as fh:
        return json.load(fh)["sha256_of_uint16_bits"]


def test_fixture_file_is_small():
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "golden_half_v1.npz")) <= 1 << 20


@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_quantiser_edges_follow_the_bit_pattern_semantics(gold, name):
    p, one, half, inf, _ = HC.FORMAT[name]
    e = gold[f"edge_{name}_in"].astype(np.int64)
    assert np.array_equal(e, HC.edge_bits(name).astype(np.int64))
    mag, neg = e & 0x7FFF, (e >> 15) == 1
    nan = mag > inf
    # safeSign: -1 iff negative, non-zero and not NaN (a negative subnormal is negative; -0.0 and NaN give +1)
    is_neg = neg & (mag != 0) & ~nan
    assert np.array_equal(gold[f"edge_{name}_bin_out"], np.where(is_neg, one | 0x8000, one).astype(np.uint16))
    # ternary: x >= 0.5 -> +1 (NaN too, as the fp32 formula does), x < -0.5 -> -1, else 0 (+0: the sum of s and its negation)
    pos = nan | (~neg & (mag >= half))
    tneg = neg & (mag > half) & ~nan
    want = np.where(pos, one, np.where(tneg, one | 0x8000, 0)).astype(np.uint16)
    got = gold[f"edge_{name}_ter_out"]
    assert np.array_equal(got & 0x7FFF, want & 0x7FFF) and np.array_equal(got[want != 0], want[want != 0])
    # STE mask 1[|x| <= 1.001] against the half value: 1.0 kept; bf16 1.0078125 masked; fp16 1.0009765625 kept; inf masked
    keep = (mag <= (one if name == "bf16" else one + 1)) | nan          # (NaN > thr is false: the gradient passes)
    for q in ("bin", "ter"):
        assert np.array_equal(gold[f"edge_{name}_{q}_mask"], np.where(keep, one, 0).astype(np.uint16)), q
    x1 = HC.from_bits(np.array([one + 1], dtype=np.uint16), HC.DTYPES[name]).double().item()
    assert (x1 > 1.001) == (name == "bf16")


FLOORS = {("lin", "bf16", "binary"): 0.5, ("lin", "bf16", "ternary"): 0.5, ("lin", "fp16", "binary"): 0.5,
          ("lin", "fp16", "ternary"): 0.25, ("conv", "bf16", "binary"): 0.5, ("conv", "bf16", "ternary"): 0.5,
          ("conv", "fp16", "ternary"): 0.2}


@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_linear_fixtures_are_rne_of_the_exact_sum(gold, gold_hashes, name, kind):
    dt = HC.DTYPES[name]
    seen_corr = 0
    for case in HC.linear_cases():
        x, w, b = HC.linear_inputs(case, kind, name)
        assert bool((x.abs() == 1).all())
        y64 = HC.exact_linear(x, HC.quantise(w, kind), b)
        want = HC.rne_of_fl32(y64, dt)
        key = f"{case['name']}_{kind}_{name}_y"
        assert HC.digest(want) == gold_hashes[key], key
        if key in gold.files:
            assert np.array_equal(gold[key], HC.bits(want)), key
        if case["corr"]:
            seen_corr += 1
            share = HC.not_representable_share(y64, dt)
            assert share >= FLOORS[("lin", name, kind)], (key, share)
            if (name, kind) == ("fp16", "binary") and case["bias"] != "nonzero":
                assert HC.tie_share(y64, dt, name) > 0, key
    assert seen_corr == 4


@pytest.mark.parametrize("kind", HC.KINDS)
@pytest.mark.parametrize("name", list(HC.DTYPES))
def test_conv_fixtures_are_rne_of_the_exact_sum(gold, gold_hashes, name, kind):
    dt = HC.DTYPES[name]
    for case in HC.conv_cases():
        if case["name"] == "conv_alexnet2" and (name, kind) != ("bf16", "binary"):
            continue                                     # (fp64 conv of the large case once is enough for this guard)
        x, w, b = HC.conv_inputs(case, kind, name)
        y64 = HC.exact_conv(x, HC.quantise(w, kind), b, case["stride"], case["pad"])
        want = HC.rne_of_fl32(y64, dt)
        key = f"{case['name']}_{kind}_{name}_y"
        assert HC.digest(want) == gold_hashes[key], key
        if case["corr"]:
            floor = FLOORS.get(("conv", name, kind))
            share = HC.not_representable_share(y64, dt)
            assert floor is None or share >= floor, (key, share)


def test_c2_fixture_is_rne_of_the_exact_sum(gold_hashes):
    x, w = HC.c2_inputs()
    y = (x.float() @ HC.quantise(w, "binary").float().t())          # exact in fp32: integers below 2^24
    assert HC.digest(y.to(torch.bfloat16)) == gold_hashes["c2_4096_bf16_y"]


# ---- C-ABI ----------------------------------------------------------------------------------------------------------------------
HALF_ENTRY_POINTS = ("qt_sign_pack_h", "qt_ternary_pack_h", "qt_check_pm1_h", "qt_sign_pack_nib_h", "qt_ternary_pack_nib_h",
                     "qt_pack_pair_nib_h", "qt_nib_gemm_h", "qt_conv2d_implicit_h")


def _header_prototypes():
    with open(_lib.HEADER_PATH, encoding="utf-8") as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(qt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def _ctype_of(arg: str):
    import ctypes
    arg = " ".join(arg.split())
    if "*" in arg or arg.startswith("qt_stream_t"):
        return ctypes.c_void_p
    if arg.startswith("int64_t"):
        return ctypes.c_int64
    if arg.startswith("float"):
        return ctypes.c_float
    assert arg.startswith("int "), arg
    return ctypes.c_int


def test_header_and_signatures_declare_the_half_entry_points_alike():
    protos = _header_prototypes()
    for name in HALF_ENTRY_POINTS:
        assert name in protos, f"{name} is not declared in include/qt_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        want = [_ctype_of(a) for a in protos[name].split(",")]
        restype, argtypes = _lib.SIGNATURES[name]
        assert list(argtypes) == want, name
        assert "dtype" in protos[name], f"{name} takes the element type as an argument"
    assert _lib.header_declared_functions() == sorted(_lib.SIGNATURES)


def test_library_version_was_bumped():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    assert _lib.version() >= 200


def test_half_entry_points_validate_their_arguments():
    """Argument validation only (nothing is launched): unknown dtype codes, misaligned planes, empty inputs."""
    import ctypes
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    null, fake, i64 = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_int64
    assert lib.qt_sign_pack_h(fake, 0, i64(64), fake, i64(4), null, i64(0), i64(1), i64(64), null) == -1     # fp32 is not a half dtype
    assert lib.qt_sign_pack_h(fake, 1, i64(64), fake, i64(3), null, i64(0), i64(1), i64(64), null) == -2
    assert lib.qt_sign_pack_h(fake, 2, i64(64), fake, i64(4), null, i64(0), i64(0), i64(64), null) == 0      # no rows
    assert lib.qt_check_pm1_h(null, 1, i64(0), fake, null) == 0
    assert lib.qt_check_pm1_h(null, 3, i64(0), fake, null) == -1
    assert lib.qt_nib_gemm_h(fake, i64(32), fake, i64(32), null, fake, 0, i64(8), i64(8), i64(8), i64(64), null) == -1
    assert lib.qt_nib_gemm_h(fake, i64(32), fake, i64(32), null, fake, 1, i64(8), i64(0), i64(8), i64(64), null) == 0
    assert lib.qt_nib_gemm_h(fake, i64(32), fake, i64(30), null, fake, 2, i64(8), i64(8), i64(8), i64(64), null) == -2
