"""The tile selector (csrc/tile_select.h) against the routes recorded from the commit before it existed.

tests/golden/tile_routes_v1.json holds, for a grid of shapes around every bound of the old ladders, the GemmCfg alias and element
class each launching entry point handed to launch_cfg (its header says how they were recorded).  The describe entry points run the
selector the launch runs, take numbers only, and need no device: every row must come out as recorded."""
import ctypes
import json
import os

import pytest

from pytorch_quantize_impls_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_routes_v1.json")
# gemm rows: entry -> (family of qt_gemm_tile_describe, element class of the launch)
GEMM_ENTRY = {0: (0, "ElemFp4"), 2: (0, "ElemBf16"), 3: (0, "ElemF16"), 4: (0, "ElemI8"), 5: (2, "ElemI8"), 6: (1, "ElemBf16")}
# aliases with a PIPE parameter: the fixture's "Cfg256_0" is TileCfg::Cfg256_0 — the same spelling


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def fx():
    with open(FIXTURE, encoding="utf-8") as fh:
        return json.load(fh)


def _geo_1x1(valid, M, Cw):
    return (M, 1, 1, Cw, 1, 1, 1, 1, 0, 0, 1, 1) if valid else (M, 1, 1, Cw, 1, 1, 3, 3, 1, 1, 1, 1)


def _expect(fx, ix):
    return (0, fx["names"][ix]) if ix >= 0 else (ix, "")


def test_fixture_is_complete_and_small(fx):
    assert os.path.getsize(FIXTURE) < 200_000
    reached = {n.split("<")[0] for n in fx["names"]}
    # every configuration the product library's ladders can launch (TileCfg without the profiling-only enumerators)
    assert len(reached) == 41 and {"ConvV128x128D", "ConvV128x64D", "ConvVPP256x192", "ConvSkinny", "CfgSkinny512", "PP384x192", "PP64",
                                   "Cfg192_1", "ConvPP64", "ConvV64x2"} <= reached
    assert {n.split("<", 1)[1][:-1] for n in fx["names"]} == {"ElemFp4", "ElemFp4T", "ElemFp4Out<1>", "ElemFp4Out<2>", "ElemI8", "ElemF16",
                                                                "ElemBf16", "ElemBf16L", "ElemFp4Taps", "ElemF16Taps"}


def test_conv_describe_names_the_recorded_kernel(lib, fx):
    buf = ctypes.create_string_buffer(128)
    rows = [r[:-1] for r in fx["conv"]] + [[r[0], *_geo_1x1(r[1], r[2], r[3]), r[4], r[5], 0, 0, *r[6:10]] for r in fx["conv_1x1"]]
    want = [r[-1] for r in fx["conv"]] + [r[-1] for r in fx["conv_1x1"]]
    assert len(rows) > 3000
    bad = []
    for r, w in zip(rows, want):
        rc = lib.qt_conv2d_implicit_describe(*r, buf, 128)
        if (rc, buf.value.decode()) != _expect(fx, w):
            bad.append((r, rc, buf.value.decode(), _expect(fx, w)))
    assert not bad, (len(bad), bad[:5])


def test_taps_describe_names_the_recorded_kernel(lib, fx):
    buf = ctypes.create_string_buffer(128)
    rows = [r[:-1] for r in fx["taps"]] + [[r[0], *_geo_1x1(r[1], r[2], r[3]), r[4], r[5], r[6]] for r in fx["taps_1x1"]]
    want = [r[-1] for r in fx["taps"]] + [r[-1] for r in fx["taps_1x1"]]
    bad = []
    for r, w in zip(rows, want):
        rc = lib.qt_conv2d_implicit_taps_describe(*r[:15], 0, 0, r[15], 0, 0, 0, buf, 128)
        if (rc, buf.value.decode()) != _expect(fx, w):
            bad.append((r, rc, buf.value.decode(), _expect(fx, w)))
    assert not bad, (len(bad), bad[:5])


def test_gemm_describe_names_the_recorded_kernel_and_keeps_its_wording(lib, fx):
    buf = ctypes.create_string_buffer(128)
    bad = []
    for row in fx["gemm"]:
        entry, v, M, N, ldxp, ldwp, w = row[:7]
        if entry == 1:
            family, variant, elem = 0, 0, f"ElemFp4Out<{v}>"          # QT_DTYPE_BF16 = 1, QT_DTYPE_F16 = 2: ElemFp4Out's parameter
        else:
            (family, elem), variant = GEMM_ENTRY[entry], v
        rc = lib.qt_gemm_tile_describe(family, variant, M, N, ldxp, ldwp, buf, 128)
        got = (rc, f"{buf.value.decode()}<{elem}>" if rc == 0 else "")
        if got != _expect(fx, w):
            bad.append((row, got, _expect(fx, w)))
        if len(row) > 7:        # qt_nib_gemm, automatic rule: the string bench.py prints, byte for byte
            rc = lib.qt_nib_gemm_describe(M, N, 64, ldxp, ldwp, buf, 128)
            if rc != 0 or buf.value.decode() != fx["describe"][row[7]]:
                bad.append((row, rc, buf.value.decode(), fx["describe"][row[7]]))
    assert len(fx["gemm"]) > 900 and not bad, (len(bad), bad[:5])


def test_describe_refuses_what_no_entry_point_takes(lib):
    buf = ctypes.create_string_buffer(64)
    geo = (0, 4, 8, 8, 8, 3, 3, 1, 1, 1, 1, 1, 1, 96, 64)
    assert lib.qt_conv2d_implicit_describe(*geo, 0, 0, 0, 0, 0, 0, buf, 64) == 0 and buf.value
    assert lib.qt_conv2d_implicit_describe(*geo, 0, 0, 8, 0, 0, 0, buf, 64) == -1              # unknown epilogue
    assert lib.qt_conv2d_implicit_describe(*geo, 0, 0, 1, 0, 0, 2, buf, 64) == -1              # a tile form beside a fused epilogue
    assert lib.qt_conv2d_implicit_describe(*geo, 0, 0, 0, 1, 0, 0, buf, 64) == -1              # thresholds without a threshold epilogue
    assert lib.qt_conv2d_implicit_describe(*geo, 0, 0, 0, 0, 0, 0x80, buf, 64) == -1           # unknown flag
    assert lib.qt_conv2d_implicit_describe(*geo, 0, 0, 0, 0, 0, 0, None, 64) == -1
    assert lib.qt_conv2d_implicit_taps_describe(*geo[:3], 8, *geo[4:], 0, 0, 0, 0, 0, 0x10, buf, 64) == -1
    assert lib.qt_gemm_tile_describe(3, 0, 8, 8, 32, 32, buf, 64) == -1
