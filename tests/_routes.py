"""Names of the matrix-core kernel instances, shared by the GPU modules that pin routes with the profiler.

One table GemmCfg tuple -> alias name (csrc/mfma_gemm_kernel.h), the parsing of profiler kernel names into 'Alias<Element>' labels,
and the check that ties a pinned route to the describe entry points (ops.*_kernel_name, i.e. csrc/tile_select.h)."""
import re

# GemmCfg<E, WM, WN, TMW, TNW, PIPE, ABL, SB, CONV, OCC>: CONV = 2 on un-padded / halo planes (ConvV*), 1 with bounds-checked taps
# (Conv*), 0 = GEMM.  Tile = 32 WM TMW rows x 32 WN TNW columns.
GEMM_CFG = {
    (2, 4, 4, 2, 1, 0, 128, 2, 1): "ConvV256",
    (2, 4, 4, 1, 1, 0, 128, 2, 1): "ConvV128",
    (4, 2, 2, 1, 1, 0, 128, 2, 1): "ConvV64",
    (4, 2, 2, 3, 1, 0, 128, 2, 1): "ConvV192",
    (2, 4, 4, 2, 2, 0, 64, 2, 1): "ConvVPP256",
    (4, 2, 2, 1, 1, 0, 64, 2, 3): "ConvV64x2",
    (2, 4, 4, 1, 1, 0, 64, 2, 2): "ConvV128x2",
    (4, 2, 3, 3, 2, 0, 64, 2, 1): "ConvVPP192",
    (2, 4, 4, 1, 2, 0, 64, 2, 1): "ConvVPP128",
    (4, 2, 2, 3, 2, 0, 64, 2, 1): "ConvVPP256x192",
    (2, 2, 1, 1, 1, 0, 512, 2, 1): "ConvVSkinny",
    (2, 4, 2, 1, 1, 0, 128, 2, 1): "ConvV128x128",
    (4, 2, 1, 1, 1, 0, 256, 2, 1): "ConvV128x64",
    (2, 4, 2, 1, 4, 0, 128, 2, 1): "ConvV128x128D",
    (4, 2, 1, 1, 3, 0, 256, 2, 1): "ConvV128x64D",
    (2, 4, 4, 2, 2, 0, 64, 1, 1): "ConvPP256",
    (4, 2, 3, 3, 2, 0, 64, 1, 1): "ConvPP192",
    (2, 4, 4, 1, 2, 0, 64, 1, 1): "ConvPP128",
    (4, 2, 2, 3, 2, 0, 64, 1, 1): "ConvPP256x192",
    (4, 2, 2, 1, 2, 0, 64, 1, 1): "ConvPP64",
    (2, 4, 4, 2, 1, 0, 128, 1, 1): "Conv256",
    (2, 4, 4, 1, 1, 0, 128, 1, 1): "Conv128",
    (4, 2, 2, 1, 1, 0, 128, 1, 1): "Conv64",
    (4, 2, 2, 3, 1, 0, 128, 1, 1): "Conv192",
    (2, 4, 2, 1, 1, 0, 128, 1, 1): "Conv128x128",
    (2, 2, 1, 1, 1, 0, 512, 1, 1): "ConvSkinny",
    # GEMM (the automatic rule of the fp4 GEMM: tests/test_gpu_tile_select.py)
    (2, 2, 1, 1, 1, 0, 512, 0, 1): "CfgSkinny512",
    (4, 2, 1, 1, 1, 0, 256, 0, 1): "CfgSkinny",
    (2, 4, 4, 2, 2, 0, 64, 0, 1): "PP256",
    (4, 2, 3, 3, 2, 0, 64, 0, 1): "PP384x192",
    (4, 2, 2, 3, 2, 0, 64, 0, 1): "PP192",
    (2, 4, 4, 1, 2, 0, 64, 0, 1): "PP128",
    (4, 2, 2, 1, 2, 0, 64, 0, 1): "PP64",
    (2, 4, 4, 2, 0, 0, 128, 0, 1): "Cfg256_0",
    (4, 2, 2, 3, 0, 0, 128, 0, 1): "Cfg192_0",
    (2, 4, 4, 1, 0, 0, 128, 0, 1): "Cfg128_0",
    (4, 2, 2, 1, 0, 0, 128, 0, 1): "Cfg64_0",
    (4, 2, 2, 1, 1, 0, 128, 0, 1): "Cfg64_1",
    # ... and the double-buffered tiles only qt_nib_gemm_variant launches (tests/test_gpu_gemm_routes.py)
    (2, 4, 4, 2, 1, 0, 128, 0, 1): "Cfg256_1",
    (4, 2, 2, 3, 1, 0, 128, 0, 1): "Cfg192_1",
    (2, 4, 4, 1, 1, 0, 128, 0, 1): "Cfg128_1",
}
CFG_ARGS = {name: ", ".join(map(str, t)) for t, name in GEMM_CFG.items()}      # alias -> "WM, WN, ..., OCC" as the profiler prints it
assert len(CFG_ARGS) == len(GEMM_CFG)


def tile_of(cfg):
    """(rows, columns) of a configuration's tile."""
    wm, wn, tmw, tnw = next(t for t, n in GEMM_CFG.items() if n == cfg)[:4]
    return 32 * wm * tmw, 32 * wn * tnw


def mfma_routes(names, elem=r"Elem\w+(?:<\d+>)?"):
    """Profiler kernel names -> labels 'ConvVPP256<ElemFp4T>' of the mfma_gemm_kernel instances among them (element classes
    matching ``elem``); a tuple outside the table stays a tuple."""
    out = set()
    for k in names:
        m = re.search(rf"GemmCfg<({elem}), ([\d, ]+)>", k.replace("(anonymous namespace)::", ""))
        if m:
            t = tuple(int(v) for v in m.group(2).split(","))
            out.add(f"{GEMM_CFG.get(t, t)}<{m.group(1)}>")
    return out


def code_conv3x3_routes(names):
    """Profiler kernel names -> labels 'code_conv3x3<CB,MODE>' of the persistent direct 3 x 3 code conv (csrc/code_conv3x3.hip)."""
    out = set()
    for k in names:
        m = re.search(r"code_conv3x3_kernel<(\d+), (\d+)>", k.replace("(anonymous namespace)::", ""))
        if m:
            out.add(f"code_conv3x3<{m.group(1)},{m.group(2)}>")
    return out


def assert_described(described, expect, case):
    """The describe entry point (``described``: an ops.*_kernel_name(...) result, or None where the case has none) names the
    configuration the profiler saw."""
    assert described is None or described == expect, (case, "described", described, "ran", expect)
