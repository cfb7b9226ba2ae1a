// Which GemmCfg instantiation of mfma_gemm_kernel a shape gets: EVERY tile rule of the matrix-core GEMMs and implicit-GEMM
// convs, as plain host functions of the shape.  No HIP, no element types, no launches, no pointers: mfma_gemm.hip and
// conv_taps.hip turn the TileCfg chosen here into a launch with one switch per family, and the describe entry points
// (qt_nib_gemm_describe, qt_conv2d_implicit_describe, qt_conv2d_implicit_taps_describe) print the same choice, so the
// launch and its description cannot disagree.  tests/test_tile_select_cpu.py walks these functions against the routes
// recorded in tests/golden/tile_routes_v1.json without a device.
//
// The persistent direct 3 x 3 code kernel (code_conv3x3.hip) and the first-layer kernels decide their own applicability
// before the implicit GEMM is asked: they are outside this selector, and the conv describe entry points report the
// implicit-GEMM choice (what qt_conv2d_implicit_codes runs under QT_CONV_NO_DIRECT_CODES).
#pragma once
#include <cstdint>
#include "../../include/qt_hip.h"   // the QT_CONV_* flag bits and the status codes, nothing else

// One enumerator per GemmCfg alias (mfma_gemm_kernel.h) the ladders launch, named as the alias is; aliases with a PIPE
// parameter have one enumerator per pipe value in use (Cfg256_0 = Cfg256<E, 0>).
enum class TileCfg {
    None,   // no configuration: the caller returns QT_ERR_UNSUPPORTED
    // GEMM
    CfgSkinny512, CfgSkinny, Cfg256_0, Cfg256_1, Cfg192_0, Cfg192_1, Cfg128_0, Cfg128_1, Cfg64_0, Cfg64_1,
    PP256, PP384x192, PP192, PP128, PP64,
    // conv, bounds-checked taps
    Conv256, Conv192, Conv128, Conv64, Conv128x128, ConvSkinny, ConvPP256, ConvPP192, ConvPP256x192, ConvPP128, ConvPP64,
    // conv, un-padded / physically padded planes
    ConvV256, ConvV192, ConvV128, ConvV64, ConvV64x2, ConvV128x2, ConvVPP256, ConvVPP192, ConvVPP256x192, ConvVPP128,
    ConvVSkinny, ConvV128x128, ConvV128x64, ConvV128x128D, ConvV128x64D,
#ifdef QT_PROFILING_VARIANTS   // stamped / ablated kernels: never in the product library
    PP256_A5, PP256_A6, Cfg256_1_A1, Cfg256_1_A2, Cfg256_1_A3, Cfg256_1_A4, ConvPP192Stamps, ConvVPP192Stamps,
#endif
};

// the alias name of a configuration, as the describe entry points print it
inline const char* tile_cfg_name(TileCfg c) {
    switch (c) {
#define QT_TILE_NAME(n) case TileCfg::n: return #n;
        QT_TILE_NAME(CfgSkinny512) QT_TILE_NAME(CfgSkinny) QT_TILE_NAME(Cfg256_0) QT_TILE_NAME(Cfg256_1) QT_TILE_NAME(Cfg192_0)
        QT_TILE_NAME(Cfg192_1) QT_TILE_NAME(Cfg128_0) QT_TILE_NAME(Cfg128_1) QT_TILE_NAME(Cfg64_0) QT_TILE_NAME(Cfg64_1)
        QT_TILE_NAME(PP256) QT_TILE_NAME(PP384x192) QT_TILE_NAME(PP192) QT_TILE_NAME(PP128) QT_TILE_NAME(PP64)
        QT_TILE_NAME(Conv256) QT_TILE_NAME(Conv192) QT_TILE_NAME(Conv128) QT_TILE_NAME(Conv64) QT_TILE_NAME(Conv128x128)
        QT_TILE_NAME(ConvSkinny) QT_TILE_NAME(ConvPP256) QT_TILE_NAME(ConvPP192) QT_TILE_NAME(ConvPP256x192) QT_TILE_NAME(ConvPP128)
        QT_TILE_NAME(ConvPP64) QT_TILE_NAME(ConvV256) QT_TILE_NAME(ConvV192) QT_TILE_NAME(ConvV128) QT_TILE_NAME(ConvV64)
        QT_TILE_NAME(ConvV64x2) QT_TILE_NAME(ConvV128x2) QT_TILE_NAME(ConvVPP256) QT_TILE_NAME(ConvVPP192) QT_TILE_NAME(ConvVPP256x192)
        QT_TILE_NAME(ConvVPP128) QT_TILE_NAME(ConvVSkinny) QT_TILE_NAME(ConvV128x128) QT_TILE_NAME(ConvV128x64)
        QT_TILE_NAME(ConvV128x128D) QT_TILE_NAME(ConvV128x64D)
#ifdef QT_PROFILING_VARIANTS
        QT_TILE_NAME(PP256_A5) QT_TILE_NAME(PP256_A6) QT_TILE_NAME(Cfg256_1_A1) QT_TILE_NAME(Cfg256_1_A2) QT_TILE_NAME(Cfg256_1_A3)
        QT_TILE_NAME(Cfg256_1_A4) QT_TILE_NAME(ConvPP192Stamps) QT_TILE_NAME(ConvVPP192Stamps)
#endif
#undef QT_TILE_NAME
        case TileCfg::None: break;
    }
    return "";
}

// ---- the named bounds (each with the measurement it came from) -------------------------------------------------------

// GEMM tile width is narrowed while the launch has fewer tiles than this (pick_tile_n_gemm)
constexpr int64_t GEMM_MIN_TILES = 160;
// skinny GEMM (FC at batch <= 512): the K loop is a chain of latency-bound stage round trips on a quarter of
// the CUs — 128x64 tiles and 256-byte stages (tools/bench_gemm_variants.py: 256x4096x25088 75 -> 48 us)
// ... and 64x64 tiles with 512-byte stages up to M = 256 (256x4096x9216: 21.4 -> 13.7 us)
constexpr int64_t SKINNY512_MAX_M = 256, SKINNY_MAX_M = 512;
// small M (small-batch inference, late layers of small images): few tiles and a long, latency-bound K loop — 64x64 tiles
// with 512-byte stages, as the skinny GEMM configuration (weight rows must be padded to whole 512-byte stages).  Taken
// for M <= 4096, and beyond that while the standard tiling leaves CUs idle (< 256 tiles) and the weight re-reads of the
// small row tiles ((M / 64) x the weight matrix through L2) stay under 256 MB
constexpr int64_t SMALL_M_ROWS = 4096, SMALL_M_IDLE_TILES = 256, SMALL_M_REREAD_BYTES = 256ll << 20;
// ... 128x128 / 128x64 tiles where those already give every CU a workgroup, and "fewer 256-row tiles than CUs" on the padded
// planes (tools/bench_conv_small_maps.py: 256 ch @ 8x8 137 -> 83 us, 512 ch @ 4x4 239 -> 102 us incl. the operand split)
constexpr int64_t FILL_TILES = 200;
// at most this many 256-row tiles and 128 x 128 tiles: 128 x 128 tiles with the deep ring (A/B: profiles/r6_c3_pmc.md)
constexpr int64_t SMALL_GRID = 128, SMALL_TILES = 512;
// long K (>= 2 KiB per output row): the ping-pong main loop and the 512-byte-stage tiles pay; a handful of K stages
// (<= 1 KiB): a tile is all prologue + epilogue, so co-resident 64-byte-stage workgroups that overlap each other win
constexpr int64_t LONG_K_BYTES = 2048, SHORT_K_BYTES = 1024;

// ---- tile widths ---------------------------------------------------------------------------------------------------

// tile width (256 / 192 / 128 / 64) that wastes the fewest padded columns; ties go to the wider tile
inline int pick_tile_n(int64_t N) {
    int best = 256;
    int64_t best_pad = (N + 255) / 256 * 256;
    const int cands[3] = {192, 128, 64};
    for (int c : cands) {
        const int64_t pad = (N + c - 1) / c * c;
        if (pad < best_pad) { best = c; best_pad = pad; }
    }
    return best;
}

// GEMM tile width: the padding-minimal width, narrowed while the launch would leave most of the 256 CUs
// without a tile (a workgroup walks the whole K loop alone, so a 256x4096x9216 problem on 16 wide tiles
// takes 50 us and on 64 narrow ones 24 us).
inline int pick_tile_n_gemm(int64_t M, int64_t N) {
    int tn = pick_tile_n(N);
    const int64_t mt = (M + 255) / 256;
    while (tn > 64 && mt * ((N + tn - 1) / tn) < GEMM_MIN_TILES) tn = tn == 256 ? 128 : 64;
    return tn;
}

// 192-wide column tiles come with 256 or 384 rows.  The 384-row tile does 50 % more work per workgroup at a
// better MFMA : fragment-read ratio; it wins unless it leaves CUs idle (fewer tiles than the 256 CUs) or adds a
// partial round.  Cost model: rounds of 256 concurrent workgroups x rows per tile; ties go to 384.
inline bool prefer_384_rows(int64_t M, int64_t N) {
    const int64_t nt = (N + 191) / 192;
    const int64_t c256 = (((M + 255) / 256) * nt + 255) / 256 * 256;
    const int64_t c384 = (((M + 383) / 384) * nt + 255) / 256 * 384;
    return c384 <= c256;
}

// ---- GEMM ------------------------------------------------------------------------------------------------------------

// the contract of the pipelined kernels (PIPE 1 / 2): row strides of whole 128-byte stages, operands below 2^31 bytes
inline bool gemm_pipe_ok(int64_t M, int64_t N, int64_t ldxp, int64_t ldwp) {
    return !(ldxp & 31) && !(ldwp & 31) && M * ldxp * 4 < (1ll << 31) && N * ldwp * 4 < (1ll << 31);
}

// automatic dispatch: tile width by N and CU fill, fast path when its contract holds
inline TileCfg select_gemm(int64_t M, int64_t N, int64_t ldxp, int64_t ldwp) {
    const bool pipe_ok = gemm_pipe_ok(M, N, ldxp, ldwp);
    const int tn = pick_tile_n_gemm(M, N);
    if (pipe_ok && M <= SKINNY512_MAX_M && !((ldxp | ldwp) & 127)) return TileCfg::CfgSkinny512;
    if (pipe_ok && M <= SKINNY_MAX_M && !((ldxp | ldwp) & 63)) return TileCfg::CfgSkinny;
    if (pipe_ok) {
        if (tn == 256) return TileCfg::PP256;
        if (tn == 192 && prefer_384_rows(M, N)) return TileCfg::PP384x192;
        if (tn == 192) return TileCfg::PP192;
        if (tn == 128) return TileCfg::PP128;
        return TileCfg::Cfg64_1;
    }
    if (tn == 256) return TileCfg::Cfg256_0;
    if (tn == 192) return TileCfg::Cfg192_0;
    if (tn == 128) return TileCfg::Cfg128_0;
    return TileCfg::Cfg64_0;
}

// the explicit variants of qt_nib_gemm_variant (tools / A/B runs), with the alignment each configuration needs
inline int gemm_variant_cfg(int variant, bool pipe_ok, int64_t ldxp, int64_t ldwp, TileCfg* cfg) {
    TileCfg c;
    bool need_pipe = true;
    switch (variant) {
        case 15: c = TileCfg::Cfg192_1; break;
        case 16: c = TileCfg::Cfg192_0; need_pipe = false; break;
        case 5: c = TileCfg::Cfg256_0; need_pipe = false; break;
        case 6: c = TileCfg::Cfg256_1; break;
        case 7: c = TileCfg::Cfg128_1; break;
        case 8: c = TileCfg::Cfg64_1; break;
        case 9: c = TileCfg::Cfg128_0; need_pipe = false; break;
        case 10: c = TileCfg::Cfg64_0; need_pipe = false; break;
        case 30: if ((ldxp | ldwp) & 63) return QT_ERR_ALIGNMENT; c = TileCfg::CfgSkinny; break;
        case 31: if ((ldxp | ldwp) & 127) return QT_ERR_ALIGNMENT; c = TileCfg::CfgSkinny512; break;
        case 20: c = TileCfg::PP256; break;
#ifdef QT_PROFILING_VARIANTS   // stamped / ablated kernels (Y is garbage): never in the product library
        case 165: c = TileCfg::PP256_A5; break;
        case 166: c = TileCfg::PP256_A6; break;
        case 161: c = TileCfg::Cfg256_1_A1; break;
        case 162: c = TileCfg::Cfg256_1_A2; break;
        case 163: c = TileCfg::Cfg256_1_A3; break;
        case 164: c = TileCfg::Cfg256_1_A4; break;
#endif
        case 21: c = TileCfg::PP128; break;
        case 22: c = TileCfg::PP192; break;
        case 23: c = TileCfg::PP64; break;
        case 24: c = TileCfg::PP384x192; break;
        default: return QT_ERR_UNSUPPORTED;
    }
    if (need_pipe && !pipe_ok) return QT_ERR_ALIGNMENT;
    *cfg = c;
    return QT_OK;
}

// batched GEMMs (blockIdx.y = tap / K slice: qt_bf16_gemm_taps, qt_i8_gemm_splitk): always ping-pong, width by padding alone.
// allow_384 (the bf16 tap GEMM): the 384-row tile when it pads M no further than 256-row tiles do.  This is NOT
// prefer_384_rows — the batch dimension fills the CUs, so rounds of workgroups do not enter — and is kept as it is.
inline TileCfg select_gemm_batched(int64_t M, int64_t N, bool allow_384) {
    const int tn = pick_tile_n(N);
    if (tn == 256) return TileCfg::PP256;
    if (tn == 192) {
        if (allow_384 && (M + 383) / 384 * 384 <= (M + 255) / 256 * 256) return TileCfg::PP384x192;
        return TileCfg::PP192;
    }
    if (tn == 128) return TileCfg::PP128;
    return TileCfg::PP64;
}

// ---- implicit-GEMM conv ----------------------------------------------------------------------------------------------

// What the conv ladders read of a launch.  form: the tile form (low 4 bits of `variant`, include/qt_hip.h): 0 = automatic,
// 1 = double-buffered, 2 = ping-pong, 3 = stamped (profiling builds), 4 = automatic without the un-padded fast path,
// 5 = 128x128 tiles, 6 = 64x64 tiles with 512-byte stages (5 / 6: plain epilogue only).
struct ConvPick {
    int64_t M, Cout;      // output pixels, output channels
    int64_t kbytes;       // bytes per (virtual) im2col row
    int64_t ldwp;         // weight row stride, words
    bool valid;           // un-padded / physically padded plane: the CONV_ = 2 kernels apply
    bool d2s;             // depth-to-space output
    bool plain_tiles;     // plain epilogue, or the level epilogue (which walks the tiles of the plain conv of its geometry)
    bool has_alpha;       // any epilogue with a per-channel affine (threshold bits, nibbles, codes, BatchNorm, levels)
    int form;             // 0 .. 6
    int flags;            // QT_CONV_* bits; the selector reads QT_CONV_NO_DEEP_RING
};
struct ConvChoice {
    TileCfg cfg;
    bool sign_bit_capable;   // the configuration also exists as the weights-as-rows (ElemFp4T) instantiation
};

// only the configurations the fused AlexNet / VGG-16 chains launch exist in the sign-bit (weights-as-rows) form
inline bool conv_sign_bit_capable(TileCfg c) {
    return c == TileCfg::ConvV128x128D || c == TileCfg::ConvV128x2 || c == TileCfg::ConvVPP192 || c == TileCfg::ConvVPP256 ||
           c == TileCfg::ConvVPP256x192;
}

inline bool conv_long_k(int64_t kbytes, int64_t ldwp) { return kbytes >= LONG_K_BYTES && !(ldwp & 127); }

// Small M on an un-padded plane, shared by the un-scaled and the per-tap scaled convs (the comments at the bounds above).
// deep_ring: the ring-of-stages forms of the 128-row tiles (the per-tap scaled convs have none).  False: not a small-M shape.
inline bool select_conv_small_m(int64_t M, int64_t Cout, int tn, int64_t kbytes, int64_t ldwp, bool d2s, bool deep_ring, TileCfg* cfg) {
    if (!conv_long_k(kbytes, ldwp) || d2s) return false;
    if (!(M <= SMALL_M_ROWS || (((M + 255) / 256) * ((Cout + tn - 1) / tn) < SMALL_M_IDLE_TILES &&
                                (M / 64) * Cout * kbytes <= SMALL_M_REREAD_BYTES)))
        return false;
    if (M > SMALL_M_ROWS && ((M + 127) / 128) * ((Cout + 127) / 128) >= FILL_TILES)
        *cfg = deep_ring ? TileCfg::ConvV128x128D : TileCfg::ConvV128x128;
    else if (((M + 127) / 128) * ((Cout + 63) / 64) >= FILL_TILES)   // 512 ch @ 4x4: 128x64 tiles, 256-byte stages
        *cfg = deep_ring ? TileCfg::ConvV128x64D : TileCfg::ConvV128x64;
    else
        *cfg = TileCfg::ConvVSkinny;
    return true;
}

// Small maps on a padded plane: fewer 256-row tiles than CUs (same accumulation order, bit-identical results).  Shared likewise.
inline bool select_conv_small_map(int64_t M, int64_t Cout, int tn, int64_t kbytes, int64_t ldwp, TileCfg* cfg) {
    if (((M + 255) / 256) * ((Cout + tn - 1) / tn) >= FILL_TILES) return false;
    *cfg = ((M + 127) / 128) * ((Cout + 127) / 128) < FILL_TILES && conv_long_k(kbytes, ldwp) ? TileCfg::ConvSkinny : TileCfg::Conv128x128;
    return true;
}

inline TileCfg select_conv_cfg(const ConvPick& p) {
    const int64_t M = p.M, Cout = p.Cout;
    const int tn = pick_tile_n(Cout);
    const int form = p.form;
    const bool plain = !p.has_alpha && p.plain_tiles;    // the plain fp32 / half epilogue
    TileCfg c;
#ifdef QT_PROFILING_VARIANTS
    if (p.valid && form == 3 && tn == 192 && !p.has_alpha) return TileCfg::ConvVPP192Stamps;
#else
    if (form == 3) return TileCfg::None;
#endif
    if (p.valid && form != 4 && form != 3) {
        // ring of 3 / 4 stage buffers on the small-map tiles (ConvV128x128D / ConvV128x64D); QT_CONV_NO_DEEP_RING: the
        // double-buffered configurations of round 4 (A/B runs and the bit-identity test)
        const bool deep_ring = !(p.flags & QT_CONV_NO_DEEP_RING);
        if (form == 0 && select_conv_small_m(M, Cout, tn, p.kbytes, p.ldwp, p.d2s, deep_ring, &c)) return c;
        // a handful of K stages: a tile is all prologue + epilogue, so 2 co-resident 256x128 workgroups per CU
        // that overlap each other's beat the 1-per-CU ping-pong tiles (output-blocked first layers: K = 320 B)
        if (form == 0 && tn == 256 && p.kbytes <= SHORT_K_BYTES) return TileCfg::ConvV128x2;
        // a few big tiles on a small map (128 -> 256 stride 2 @ 16x16, K = 1152 B: 64 tiles of 256x256): 128x128 tiles
        // with the deep ring give every CU one
        if (form == 0 && deep_ring && !p.d2s && ((M + 255) / 256) * ((Cout + tn - 1) / tn) <= SMALL_GRID &&
            ((M + 127) / 128) * ((Cout + 127) / 128) >= FILL_TILES && ((M + 127) / 128) * ((Cout + 127) / 128) <= SMALL_TILES)
            return TileCfg::ConvV128x128D;
        if (form != 1) {
            // 192-wide tiles: ping-pong on a 384x192 tile, whose 96x96 wave tiles keep the load segment under the compute
            // segment (AlexNet conv2 302 -> 275 us)
            if (tn == 192 && (form == 2 || prefer_384_rows(M, Cout))) return TileCfg::ConvVPP192;
            if (tn == 256) return TileCfg::ConvVPP256;
            // 192-wide tiles whose 384-row form wastes a round (576 -> 1152 @ 13x13): 256x192 ping-pong for long K
            if (tn == 192 && form == 0 && p.kbytes >= LONG_K_BYTES) return TileCfg::ConvVPP256x192;
        }
        if (form == 0 && tn == 64 && p.kbytes <= SHORT_K_BYTES) return TileCfg::ConvV64x2;
        if (form == 0 && tn == 128 && p.kbytes <= SHORT_K_BYTES) return TileCfg::ConvV128x2;
        if (tn == 256) return TileCfg::ConvV256;
        if (tn == 192) return TileCfg::ConvV192;
        if (tn == 128) return TileCfg::ConvV128;
        return TileCfg::ConvV64;
    }
#ifdef QT_PROFILING_VARIANTS
    if (form == 3 && tn == 192 && !p.has_alpha) return TileCfg::ConvPP192Stamps;
#endif
    if (form == 5 && plain) return TileCfg::Conv128x128;
    if (form == 6 && plain && conv_long_k(p.kbytes, p.ldwp)) return TileCfg::ConvSkinny;
    if (form == 0 && p.plain_tiles && select_conv_small_map(M, Cout, tn, p.kbytes, p.ldwp, &c)) return c;
    if (form == 0 && tn == 192 && prefer_384_rows(M, Cout)) return TileCfg::ConvPP192;
    // long K (>= 2 KiB per output row), wide tiles: the ping-pong main loop beats the double-buffered one on the
    // padded convs too (tools/bench_grad_input_variants.py: grad_x 512 ch @ 28x28 0.532 -> 0.485 ms, 768 -> 1152
    // @ 13x13 1.34 -> 1.25); the 384-row tile only where its rounds pay (above), else 256 rows
    if (form == 0 && p.kbytes >= LONG_K_BYTES) {
        if (tn == 256) return TileCfg::ConvPP256;
        if (tn == 192) return TileCfg::ConvPP256x192;
    }
    if (form == 2) {
        if (tn == 256) return TileCfg::ConvPP256;
        if (tn == 192) return TileCfg::ConvPP192;
        if (tn == 128) return TileCfg::ConvPP128;
        return TileCfg::ConvPP64;
    }
    if (tn == 256) return TileCfg::Conv256;
    if (tn == 192) return TileCfg::Conv192;
    if (tn == 128) return TileCfg::Conv128;
    return TileCfg::Conv64;
}

inline ConvChoice select_conv(const ConvPick& p) {
    const TileCfg c = select_conv_cfg(p);
    return {c, conv_sign_bit_capable(c)};
}

// Per-tap scaled convs (conv_taps.hip).  Tile widths: the in-place multiply needs the accumulators in VALU-addressable
// registers next to the fragments (a wave of an 8-wave workgroup owns 256 registers, arch + acc together).  256x256 (128
// accumulator registers) fits its MAIN LOOP in them — the ~80 spilled dwords are prologue / epilogue values — and is what
// Cout = 768 / 256 want (AlexNet conv4: 163 -> 137 us, conv5: 60 -> 41 us against 256x192 / 256x128 tiles); the
// 144-register 384x192 tile of the un-scaled conv does not.  No deep ring, no forms.
inline TileCfg select_conv_taps(int64_t M, int64_t Cout, int64_t kbytes, int64_t ldwp, bool valid, bool d2s, bool plain) {
    const int tn = pick_tile_n(Cout);
    TileCfg c;
    if (valid) {
        if (select_conv_small_m(M, Cout, tn, kbytes, ldwp, d2s, false, &c)) return c;
        if (tn == 256) return TileCfg::ConvVPP256;
        if (tn == 192 && prefer_384_rows(M, Cout)) return TileCfg::ConvVPP192;
        if (tn == 192) return TileCfg::ConvVPP256x192;
        if (tn == 128) return TileCfg::ConvVPP128;
        return TileCfg::ConvV64;
    }
    if (plain && select_conv_small_map(M, Cout, tn, kbytes, ldwp, &c)) return c;
    if (tn == 256) return TileCfg::ConvPP256;
    if (tn == 192 && prefer_384_rows(M, Cout)) return TileCfg::ConvPP192;
    if (tn == 192) return TileCfg::ConvPP256x192;
    if (tn == 128) return TileCfg::ConvPP128;
    return TileCfg::Conv64;
}
