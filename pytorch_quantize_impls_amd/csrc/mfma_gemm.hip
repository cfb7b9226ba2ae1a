// Packed low-bit GEMMs on the matrix cores.
//
//   fp4 ("nibble planes", include/qt_hip.h): +-1 / {-1,0,+1} operands as FP4-E2M1 nibbles, contracted
//       with the block-scaled MX MFMA  v_mfma_scale_f32_32x32x64_f8f6f4  (A = B = fp4, every block
//       scale 2^0).  E2M1 holds -1, 0, +1 exactly and the accumulator is fp32, so every partial sum is
//       an integer of magnitude <= K < 2^24: bit-identical to the popcount formulation and to the
//       reference's fp32 GEMM on +-1 tensors.  Measured issue rate on MI355X: 9.0 PFLOP/s vs 1.49 Pop/s
//       for the xor+bcnt pair (profiles/r1_ubench.txt) — which is why large shapes are routed here.
//   int8 ("code planes"): DoReFa k-bit activation codes q = rint((2^k-1) x) x +-1/0 weight codes with
//       v_mfma_i32_32x32x32_i8, int32 accumulate (exact), one fp32 scale in the epilogue.
//   bf16 ("triple planes"): real-valued activations split exactly into hi + mid + lo bf16 terms x +-1/0 weights
//       replicated three times, v_mfma_f32_32x32x16_bf16, fp32 accumulate (fp32-GEMM accuracy).
//
// Y[m,n] = scale * sum_k X[m,k] * W[n,k] (+ bias);  X: M x K, W: N x K, row-major byte rows.
//
// One kernel template serves all three: everything is organised in BYTES of K.  A stage is 128 (PIPE 0/1) or 64
// (PIPE 2) bytes of K per row = 4 / 2 MFMA k-steps of 32 bytes; lane l of a wave supplies, for the 32x32 MFMA,
// row (l & 31) and the 16-byte chunk (2*kk + (l >> 5)) of the stage row.
//
// Workgroup = 8 waves (2 per SIMD).  X is the MFMA "A" operand (D rows = m) and W the "B" operand (D cols = n).
// Epilogues: fp32 Y through a wave-private LDS transpose and dwordx4 full-line stores (or dword stores when Y is
// not 16-byte friendly), or — inference fusion — one THRESHOLD BIT per output ([(acc + bias) * alpha + beta < 0],
// EpiArgs) assembled with wave ballots.
//
// LDS: stage rows are 16-byte chunks, chunk c of row r stored at position c ^ f(r) (swz<>): the 16 rows a
// ds_read_b128 lane group touches (distinct mod 16) fall on 16 distinct 16-B slots of the 256-B bank row ->
// conflict-free fragment reads.
//
// Staging is LDS-DMA (global_load_lds_dwordx4: no VGPR round trip; the swizzle is applied on the per-lane SOURCE
// address because the LDS side of the instruction is lane-linear).
//   PIPE = 2 (ping-pong; every GEMM tile, conv on the 384x192 / 256x256 tiles): 64-byte stages in a ring of 4;
//       a wave's stage is a LOAD segment (all fragment reads of the stage + its DMA pieces of stage s+3) followed
//       by a COMPUTE segment (register-only MFMAs), and the two waves of a SIMD run one segment apart, so one owns
//       the matrix pipe while the other owns LDS / DMA issue.  See the comment at the loop.
//   PIPE = 1 (double-buffered; the remaining conv tiles): the DMA is issued from inline asm, so hipcc has no
//       outstanding-DMA knowledge (with the builtin it drains vmcnt(0) in front of the next ds_read); the pieces of
//       stage s+1 are interleaved with software-pipelined fragment reads and the MFMAs of stage s; one manual
//       vmcnt(0) + barrier per stage; last stage peeled so the steady-state body is one basic block.
//       Contract of PIPE 1/2: row strides are whole 128-byte stages (ld % 32 words == 0, pad zero) and each operand
//       spans < 2^31 bytes (32-bit lane offsets).
//   PIPE = 0 (generic): builtin DMA, 64-bit addresses, any ld % 4 words; chunks past the row stride read a 16-byte
//       zero word.  All fragment reads of a stage are issued before the DMA of the next.
// Conv (CONV_ = 1 / 2): the X operand is an NHWC pixel plane and a stage gathers the 16-byte chunks of the taps it
// covers (implicit GEMM, no im2col buffer): per-tap bounds checks + zero page (1), or — un-padded / physically
// padded planes — plain 32-bit offsets with the per-(stage, chunk) tap offsets tabulated once in LDS (2).
// Profiling-only variants (ABL_ != 0) exist only in -DQT_PROFILING_VARIANTS builds (qt_nib_gemm_variant 161-166,
// qt_conv2d_implicit_variant 3); the product library does not contain them.

#include <cstdio>
#include "mfma_gemm_kernel.h"
#include "tile_select.h"
#include "qt_elt.h"
#include "nib_quant.h"

namespace {

int check_common(const void* Xn, int64_t ldxp, const void* Wn, int64_t ldwp, const float* Y, int64_t ldy,
                 int64_t M, int64_t N, int64_t K, int64_t kwords) {
    if (M < 0 || N < 0 || K < 0) return QT_ERR_INVALID_ARG;
    if (M == 0 || N == 0) return 1;  // nothing to do
    if (!Y || ldy < N) return QT_ERR_INVALID_ARG;
    if (M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return QT_ERR_UNSUPPORTED;
    if (K > 0 && (!Xn || !Wn)) return QT_ERR_INVALID_ARG;
    if (ldxp < kwords || ldwp < kwords) return QT_ERR_INVALID_ARG;
    if ((ldxp & 3) || (ldwp & 3)) return QT_ERR_ALIGNMENT;
    if (K > 0 && (!qt_aligned16(Xn) || !qt_aligned16(Wn))) return QT_ERR_ALIGNMENT;
    return QT_OK;
}

// ---- TileCfg (tile_select.h) -> launch: one switch per family, whose cases are the configurations that family instantiates ----
// (a: the arguments of launch_cfg.  A configuration outside the family's set is QT_ERR_UNSUPPORTED, never another kernel.)

// automatic GEMM dispatch (select_gemm)
template <class E, class... A>
int launch_gemm_auto(TileCfg cfg, A&&... a) {
    switch (cfg) {
        case TileCfg::CfgSkinny512: return launch_cfg<CfgSkinny512<E>>(a...);
        case TileCfg::CfgSkinny: return launch_cfg<CfgSkinny<E>>(a...);
        case TileCfg::PP256: return launch_cfg<PP256<E>>(a...);
        case TileCfg::PP384x192: return launch_cfg<PP384x192<E>>(a...);
        case TileCfg::PP192: return launch_cfg<PP192<E>>(a...);
        case TileCfg::PP128: return launch_cfg<PP128<E>>(a...);
        case TileCfg::Cfg64_1: return launch_cfg<Cfg64<E, 1>>(a...);
        case TileCfg::Cfg256_0: return launch_cfg<Cfg256<E, 0>>(a...);
        case TileCfg::Cfg192_0: return launch_cfg<Cfg192<E, 0>>(a...);
        case TileCfg::Cfg128_0: return launch_cfg<Cfg128<E, 0>>(a...);
        case TileCfg::Cfg64_0: return launch_cfg<Cfg64<E, 0>>(a...);
        default: return QT_ERR_UNSUPPORTED;
    }
}

// explicit variants (gemm_variant_cfg)
template <class E, class... A>
int launch_gemm_variant(TileCfg cfg, A&&... a) {
    switch (cfg) {
        case TileCfg::Cfg192_1: return launch_cfg<Cfg192<E, 1>>(a...);
        case TileCfg::Cfg192_0: return launch_cfg<Cfg192<E, 0>>(a...);
        case TileCfg::Cfg256_0: return launch_cfg<Cfg256<E, 0>>(a...);
        case TileCfg::Cfg256_1: return launch_cfg<Cfg256<E, 1>>(a...);
        case TileCfg::Cfg128_1: return launch_cfg<Cfg128<E, 1>>(a...);
        case TileCfg::Cfg64_1: return launch_cfg<Cfg64<E, 1>>(a...);
        case TileCfg::Cfg128_0: return launch_cfg<Cfg128<E, 0>>(a...);
        case TileCfg::Cfg64_0: return launch_cfg<Cfg64<E, 0>>(a...);
        case TileCfg::CfgSkinny: return launch_cfg<CfgSkinny<E>>(a...);
        case TileCfg::CfgSkinny512: return launch_cfg<CfgSkinny512<E>>(a...);
        case TileCfg::PP256: return launch_cfg<PP256<E>>(a...);
#ifdef QT_PROFILING_VARIANTS   // stamped / ablated kernels (Y is garbage): never in the product library
        case TileCfg::PP256_A5: return launch_cfg<PP256<E, 5>>(a...);
        case TileCfg::PP256_A6: return launch_cfg<PP256<E, 6>>(a...);
        case TileCfg::Cfg256_1_A1: return launch_cfg<Cfg256<E, 1, 1>>(a...);
        case TileCfg::Cfg256_1_A2: return launch_cfg<Cfg256<E, 1, 2>>(a...);
        case TileCfg::Cfg256_1_A3: return launch_cfg<Cfg256<E, 1, 3>>(a...);
        case TileCfg::Cfg256_1_A4: return launch_cfg<Cfg256<E, 1, 4>>(a...);
#endif
        case TileCfg::PP128: return launch_cfg<PP128<E>>(a...);
        case TileCfg::PP192: return launch_cfg<PP192<E>>(a...);
        case TileCfg::PP64: return launch_cfg<PP64<E>>(a...);
        case TileCfg::PP384x192: return launch_cfg<PP384x192<E>>(a...);
        default: return QT_ERR_UNSUPPORTED;
    }
}

// batched GEMMs (select_gemm_batched); ROWS384: the bf16 tap GEMM's set has the 384-row tile, the int8 split-K set has not
template <class E, bool ROWS384, class... A>
int launch_gemm_batched(TileCfg cfg, A&&... a) {
    switch (cfg) {
        case TileCfg::PP256: return launch_cfg<PP256<E>>(a...);
        case TileCfg::PP384x192:
            if constexpr (ROWS384) return launch_cfg<PP384x192<E>>(a...);
            else return QT_ERR_UNSUPPORTED;
        case TileCfg::PP192: return launch_cfg<PP192<E>>(a...);
        case TileCfg::PP128: return launch_cfg<PP128<E>>(a...);
        case TileCfg::PP64: return launch_cfg<PP64<E>>(a...);
        default: return QT_ERR_UNSUPPORTED;
    }
}

// implicit-GEMM convs (select_conv).  t: the weights-as-rows (sign-bit) instantiation of a configuration that has one
template <class E, class... A>
int launch_conv(TileCfg cfg, bool t, A&&... a) {
    switch (cfg) {
        case TileCfg::ConvV128x128D: return launch_cfg_t<ConvV128x128D, E>(t, a...);
        case TileCfg::ConvV128x128: return launch_cfg<ConvV128x128<E>>(a...);
        case TileCfg::ConvV128x64D: return launch_cfg<ConvV128x64D<E>>(a...);
        case TileCfg::ConvV128x64: return launch_cfg<ConvV128x64<E>>(a...);
        case TileCfg::ConvVSkinny: return launch_cfg<ConvVSkinny<E>>(a...);
        case TileCfg::ConvV128x2: return launch_cfg_t<ConvV128x2, E>(t, a...);
        case TileCfg::ConvVPP192: return launch_cfg_t<ConvVPP192, E>(t, a...);
        case TileCfg::ConvVPP256: return launch_cfg_t<ConvVPP256, E>(t, a...);
        case TileCfg::ConvVPP256x192: return launch_cfg_t<ConvVPP256x192, E>(t, a...);
        case TileCfg::ConvV64x2: return launch_cfg<ConvV64x2<E>>(a...);
        case TileCfg::ConvV256: return launch_cfg<ConvV256<E>>(a...);
        case TileCfg::ConvV192: return launch_cfg<ConvV192<E>>(a...);
        case TileCfg::ConvV128: return launch_cfg<ConvV128<E>>(a...);
        case TileCfg::ConvV64: return launch_cfg<ConvV64<E>>(a...);
        case TileCfg::Conv128x128: return launch_cfg<Conv128x128<E>>(a...);
        case TileCfg::ConvSkinny: return launch_cfg<ConvSkinny<E>>(a...);
        case TileCfg::ConvPP192: return launch_cfg<ConvPP192<E>>(a...);
        case TileCfg::ConvPP256: return launch_cfg<ConvPP256<E>>(a...);
        case TileCfg::ConvPP256x192: return launch_cfg<ConvPP256x192<E>>(a...);
        case TileCfg::ConvPP128: return launch_cfg<ConvPP128<E>>(a...);
        case TileCfg::ConvPP64: return launch_cfg<ConvPP64<E>>(a...);
        case TileCfg::Conv256: return launch_cfg<Conv256<E>>(a...);
        case TileCfg::Conv192: return launch_cfg<Conv192<E>>(a...);
        case TileCfg::Conv128: return launch_cfg<Conv128<E>>(a...);
        case TileCfg::Conv64: return launch_cfg<Conv64<E>>(a...);
#ifdef QT_PROFILING_VARIANTS
        case TileCfg::ConvVPP192Stamps: return launch_cfg<ConvVPP192Stamps<E>>(a...);
        case TileCfg::ConvPP192Stamps: return launch_cfg<ConvPP192Stamps<E>>(a...);
#endif
        default: return QT_ERR_UNSUPPORTED;
    }
}

template <class E>
int dispatch_gemm_auto(const uint32_t* Xn, int64_t ldxp, const uint32_t* Wn, int64_t ldwp,
                       const float* bias, float scale, const float* scale_dev, float* Y, int64_t ldy, int64_t M,
                       int64_t N, int64_t K, qt_stream_t stream) {
    return launch_gemm_auto<E>(select_gemm(M, N, ldxp, ldwp), Xn, ldxp, Wn, ldwp, bias, scale, scale_dev, Y, ldy, M, N, K, stream);
}

template <class E>
int dispatch_gemm(int variant, const uint32_t* Xn, int64_t ldxp, const uint32_t* Wn, int64_t ldwp,
                  const float* bias, float scale, const float* scale_dev, float* Y, int64_t ldy, int64_t M,
                  int64_t N, int64_t K, qt_stream_t stream) {
    if (variant == 0) return dispatch_gemm_auto<E>(Xn, ldxp, Wn, ldwp, bias, scale, scale_dev, Y, ldy, M, N, K, stream);
    TileCfg cfg;
    const int rc = gemm_variant_cfg(variant, gemm_pipe_ok(M, N, ldxp, ldwp), ldxp, ldwp, &cfg);
    if (rc != QT_OK) return rc;
    return launch_gemm_variant<E>(cfg, Xn, ldxp, Wn, ldwp, bias, scale, scale_dev, Y, ldy, M, N, K, stream);
}

// "<tile>, <pipeline>" of an automatic-dispatch configuration, as qt_nib_gemm_describe has always printed it
const char* gemm_tile_text(TileCfg cfg) {
    switch (cfg) {
        case TileCfg::CfgSkinny512: return "64x64, 512-byte stages, pipe=1";
        case TileCfg::CfgSkinny: return "128x64, 256-byte stages, pipe=1";
        case TileCfg::PP256: return "256x256, pipe=2 (ping-pong)";
        case TileCfg::PP384x192: return "384x192, pipe=2 (ping-pong)";
        case TileCfg::PP192: return "256x192, pipe=2 (ping-pong)";
        case TileCfg::PP128: return "256x128, pipe=2 (ping-pong)";
        case TileCfg::Cfg64_1: return "256x64, pipe=1";
        case TileCfg::Cfg256_0: return "256x256, pipe=0";
        case TileCfg::Cfg192_0: return "256x192, pipe=0";
        case TileCfg::Cfg128_0: return "256x128, pipe=0";
        case TileCfg::Cfg64_0: return "256x64, pipe=0";
        default: return "?";
    }
}

// ---- fp32 / bf16 / fp16 -> nibble plane (element types: qt_elt.h) ---------------------------------
// (the nibble codes NibSign / NibTernary / NibSign0: nib_quant.h, shared with the training update)
template <class Enc>
__device__ __forceinline__ uint32_t nib_half(const float4& v) {   // 4 elements -> 16 bits
    return Enc::nib(v.x) | (Enc::nib(v.y) << 4) | (Enc::nib(v.z) << 8) | (Enc::nib(v.w) << 12);
}
template <class Enc, class E>
__device__ __forceinline__ uint32_t nib_word(const typename E::vec& v) {   // 8 half elements -> one whole word
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) w |= Enc::template nib<E>(v.e[i]) << (4 * i);
    return w;
}
template <class Enc, class E>
__device__ __forceinline__ uint32_t nib_of(typename E::scalar x) {
    if constexpr (E::EPV == 4) return Enc::nib(x);
    else return Enc::template nib<E>(x);
}

// Write-through (sc1) dword store: the nibble plane is read by the GEMM that follows, through the L2s / MALL, and a kernel
// that leaves its output dirty in the L2s pays the write-back at its end-of-kernel boundary (the GEMM epilogue's stores,
// mfma_gemm_kernel.h).  s_nop: the store reads its data register late and the hazard recogniser does not look inside asm.
__device__ __forceinline__ void store_wt(uint32_t* p, uint32_t v) {
    asm volatile("global_store_dword %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
}

// fp32 rows -> nibble plane, the work of one wave.  Unit = 256 consecutive float4 slots of one padded row (ldp words =
// 2 ldp slots); lane l takes slots 64 j + l of the unit, j = 0..3: four independent dwordx4 loads per lane in flight, each
// load instruction one contiguous KiB.  The 16-bit halves of lanes (2i, 2i + 1) form one word (one DPP swap per pair of
// groups): even lanes store the words of groups 0 / 2, odd lanes those of groups 1 / 3, so each store instruction has all
// lanes active on 256 contiguous bytes.  Slots past K/4 produce zero nibbles (the pad-is-zero invariant).  Units are walked
// wave-strided (gw, gw + nw, ...) with the (row, unit) position advanced by a precomputed step: 32-bit arithmetic, no
// division in the loop.  Host contract (pack_fits_32bit): rows, 2 ldp, K/4 < 2^30; K >= 4.
// Half elements (E::EPV == 8): a 16-byte slot is eight elements = one whole word, a padded row is ldp slots, and the
// unit's four loads per lane become four full-wave dword stores of 256 contiguous bytes each — no lane exchange.
template <class Enc, class E>
__device__ __forceinline__ void nib_pack_rows(const typename E::scalar* __restrict__ x, int64_t ldx, uint32_t* __restrict__ out,
                                              int64_t ldp, int rows, int k4, int gw, int nw) {
    const int lane = threadIdx.x & 63;
    const bool odd = lane & 1;
    const int spr = (int)ldp * (8 / E::EPV), upr = (spr + 255) >> 8;
    int row = gw / upr, seg = gw - row * upr;
    const int srow = nw / upr, sseg = nw - srow * upr;
    while (row < rows) {
        const typename E::scalar* xr = x + (int64_t)row * ldx;
        uint32_t* orow = out + (int64_t)row * ldp;
        const int s0 = seg * 256 + lane;
        if constexpr (E::EPV == 8) {
            typename E::vec v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const typename E::vec*>(xr + min(s0 + 64 * j, k4 - 1) * 8);
            uint32_t word[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) word[j] = nib_word<Enc, E>(v[j]) & (s0 + 64 * j < k4 ? 0xFFFFFFFFu : 0u);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (s0 + 64 * j < spr) store_wt(orow + s0 + 64 * j, word[j]);
        } else {
            // unconditional loads (slot clamped into the row's K), masked after: a guarded load becomes a branch around a load
            // and its wait, i.e. one load in flight
            float4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const float4*>(xr + min(s0 + 64 * j, k4 - 1) * 4);
            uint32_t h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = nib_half<Enc>(v[j]) & (s0 + 64 * j < k4 ? 0xFFFFu : 0u);
            uint32_t word[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const uint32_t send = odd ? h[2 * p] : h[2 * p + 1];
                const uint32_t recv = (uint32_t)__builtin_amdgcn_mov_dpp((int)send, 0xB1, 0xF, 0xF, false);  // quad_perm [1,0,3,2]
                word[p] = odd ? (recv | (h[2 * p + 1] << 16)) : (h[2 * p] | (recv << 16));
            }
            // both stores after the last load is consumed: the compiler does not count the asm stores, so a store issued
            // between the loads would turn its later vmcnt waits into waits for the store's completion
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int ws = seg * 256 + 128 * p + (odd ? 63 + lane : lane);   // first slot of the word this lane stores
                if (ws < spr) store_wt(orow + (ws >> 1), word[p]);
            }
        }
        seg += sseg;
        row += srow;
        if (seg >= upr) { seg -= upr; ++row; }
    }
}

template <class Enc, class E>
__global__ __launch_bounds__(256) void nib_pack_vec_kernel(const typename E::scalar* __restrict__ x, int64_t ldx,
                                                           uint32_t* __restrict__ out, int64_t ldp, int rows, int k4) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    nib_pack_rows<Enc, E>(x, ldx, out, ldp, rows, k4, blockIdx.x * 4 + wave, gridDim.x * 4);
}

// Both operands of one LinearBin / LinearTer forward in ONE launch (activation: safeSign, weight: EncW): saves a
// kernel boundary and one ramp / tail of a ~12 us HBM-bound kernel.  Workgroups [0, ga) pack the activation, the rest
// the weight (ga: the activation's share of the units).
template <class EncW, class E>
__global__ __launch_bounds__(256) void nib_pack_pair_kernel(const typename E::scalar* __restrict__ xa, int64_t lda,
                                                            uint32_t* __restrict__ oa, int64_t ldpa, int rowsa,
                                                            const typename E::scalar* __restrict__ xb, int64_t ldb,
                                                            uint32_t* __restrict__ ob, int64_t ldpb, int rowsb,
                                                            int k4, int ga) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    if (b < ga) nib_pack_rows<NibSign, E>(xa, lda, oa, ldpa, rowsa, k4, b * 4 + wave, ga * 4);
    else nib_pack_rows<EncW, E>(xb, ldb, ob, ldpb, rowsb, k4, (b - ga) * 4 + wave, ((int)gridDim.x - ga) * 4);
}

// Generic path (any K / alignment): one thread per output word, scalar loads.
template <class Enc, class E>
__global__ __launch_bounds__(256) void nib_pack_scalar_kernel(const typename E::scalar* __restrict__ x, int64_t ldx,
                                                              uint32_t* __restrict__ out, int64_t ldp,
                                                              int64_t rows, int64_t K) {
    const int64_t total = rows * ldp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ldp, w = i - row * ldp;
        uint32_t word = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t k = w * 8 + e;
            if (k < K) word |= nib_of<Enc, E>(x[row * ldx + k]) << (4 * e);
        }
        out[i] = word;
    }
}

// ---- bit planes -> nibble plane (derived MFMA operand format) ---------------------------------------
// One thread = one 32-bit word of the planes -> four nibble words (16 B).  sign-only planes:
// nibble = 0x2 | s<<3.  mask+sign: nibble = m<<1 | (s&m)<<3.  Words past the bit planes' stride are 0.
__global__ __launch_bounds__(256) void bits_to_nib_kernel(const uint32_t* __restrict__ sign,
                                                          const uint32_t* __restrict__ mask,
                                                          int64_t ldb, uint32_t* __restrict__ out,
                                                          int64_t ldn, int64_t rows, int64_t K) {
    const int64_t groups_per_row = ldn / 4;  // one group = 4 nibble words = 32 elements
    const int64_t total = rows * groups_per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / groups_per_row, g = i - row * groups_per_row;
        uint32_t sw = 0, mw = 0;
        if (g < ldb) {
            sw = sign[row * ldb + g];
            if (mask) {
                mw = mask[row * ldb + g];
            } else {  // binary: every element inside K is non-zero
                const int64_t rem = K - g * 32;
                mw = rem >= 32 ? 0xFFFFFFFFu : (rem > 0 ? ((1u << rem) - 1u) : 0u);
            }
        }
        sw &= mw;
        uint4 o;
        o.x = (spread8(mw) << 1) | (spread8(sw) << 3);
        o.y = (spread8(mw >> 8) << 1) | (spread8(sw >> 8) << 3);
        o.z = (spread8(mw >> 16) << 1) | (spread8(sw >> 16) << 3);
        o.w = (spread8(mw >> 24) << 1) | (spread8(sw >> 24) << 3);
        *reinterpret_cast<uint4*>(out + row * ldn + g * 4) = o;
    }
}

// Same expansion into a PHYSICALLY zero-padded NHWC pixel plane [N][H + 2ph][W + 2pw][ldn]: border pixels
// are fp4 zeros, so a padded conv becomes an un-padded one on this plane and takes the conv kernels'
// VALID mode (no per-tap bounds checks, 32-bit offsets).
__global__ __launch_bounds__(256) void bits_to_nib_pad_kernel(const uint32_t* __restrict__ sign,
                                                              const uint32_t* __restrict__ mask, int64_t ldb,
                                                              uint32_t* __restrict__ out, int64_t ldn, int64_t N,
                                                              int H, int W, int ph, int pw, int64_t K) {
    const int64_t groups_per_row = ldn / 4;
    const int Hp = H + 2 * ph, Wp = W + 2 * pw;
    const int64_t total = N * Hp * Wp * groups_per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t orow = i / groups_per_row, g = i - orow * groups_per_row;
        const int64_t n = orow / ((int64_t)Hp * Wp);
        const int rem = (int)(orow - n * Hp * Wp);
        const int y = rem / Wp - ph, x = rem % Wp - pw;
        uint32_t sw = 0, mw = 0;
        if (g < ldb && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            const int64_t row = (n * H + y) * W + x;
            sw = sign[row * ldb + g];
            if (mask) {
                mw = mask[row * ldb + g];
            } else {
                const int64_t r2 = K - g * 32;
                mw = r2 >= 32 ? 0xFFFFFFFFu : (r2 > 0 ? ((1u << r2) - 1u) : 0u);
            }
        }
        sw &= mw;
        uint4 o;
        o.x = (spread8(mw) << 1) | (spread8(sw) << 3);
        o.y = (spread8(mw >> 8) << 1) | (spread8(sw >> 8) << 3);
        o.z = (spread8(mw >> 16) << 1) | (spread8(sw >> 16) << 3);
        o.w = (spread8(mw >> 24) << 1) | (spread8(sw >> 24) << 3);
        *reinterpret_cast<uint4*>(out + orow * ldn + g * 4) = o;
    }
}

// nib_pack_rows' 32-bit position arithmetic: row + units-per-wave step and the slot index stay below 2^31
bool pack_fits_32bit(int64_t rows, int64_t ldp) { return rows < (1ll << 30) && ldp < (1ll << 29); }
// one unit = one wave's work = 256 16-byte slots; spw = slots per plane word (2 for fp32, 1 for the half types)
int64_t pack_units(int64_t rows, int64_t ldp, int spw = 2) { return rows * ((ldp * spw + 255) / 256); }

template <class Enc, class E = EltF32>
int launch_nib_pack(const typename E::scalar* x, int64_t ldx, uint32_t* out, int64_t ldp, int64_t rows, int64_t K,
                    qt_stream_t stream) {
    constexpr int EPV = E::EPV;
    if (rows < 0 || K < 0 || ldx < K) return QT_ERR_INVALID_ARG;
    if (rows == 0) return QT_OK;
    if (!out || (!x && K > 0)) return QT_ERR_INVALID_ARG;
    const int64_t kw = (K + 7) / 8;
    if (ldp < kw || (ldp & 3) != 0 || !qt_aligned16(out)) return QT_ERR_ALIGNMENT;
    if (ldp == 0) return QT_OK;
    const bool vec = K > 0 && (K % EPV == 0) && (ldx % EPV == 0) && qt_aligned16(x) && pack_fits_32bit(rows, ldp);
    if (vec) {
        const int grid = qt_stream_grid((pack_units(rows, ldp, 8 / EPV) + 3) / 4);
        hipLaunchKernelGGL((nib_pack_vec_kernel<Enc, E>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x,
                           ldx, out, ldp, (int)rows, (int)(K / EPV));
    } else {
        const int grid = qt_stream_grid((rows * ldp + 255) / 256);
        hipLaunchKernelGGL((nib_pack_scalar_kernel<Enc, E>), dim3(grid), dim3(256), 0, (hipStream_t)stream,
                           x, ldx, out, ldp, rows, K);
    }
    return qt_check_launch();
}

// Both operands of a training-mode Linear in one launch (qt_pack_pair_nib_f32 / _h).
template <class E>
int pack_pair_any(const typename E::scalar* x, int64_t ldx, uint32_t* x_plane, int64_t ldxp, int64_t rows_x,
                  const typename E::scalar* w, int64_t ldw, uint32_t* w_plane, int64_t ldwp, int64_t rows_w, int64_t K,
                  int w_ternary, qt_stream_t stream) {
    constexpr int EPV = E::EPV;
    if (rows_x < 0 || rows_w < 0 || K < 0 || ldx < K || ldw < K) return QT_ERR_INVALID_ARG;
    const bool vec = rows_x > 0 && rows_w > 0 && K > 0 && (K % EPV == 0) && (ldx % EPV == 0) && (ldw % EPV == 0) &&
                     qt_aligned16(x) && qt_aligned16(w) && x && w && x_plane && w_plane;
    if (!vec) {   // ragged / empty operands: the two single-operand launches handle every case
        const int rc = launch_nib_pack<NibSign, E>(x, ldx, x_plane, ldxp, rows_x, K, stream);
        if (rc != QT_OK) return rc;
        return w_ternary ? launch_nib_pack<NibTernary, E>(w, ldw, w_plane, ldwp, rows_w, K, stream)
                         : launch_nib_pack<NibSign, E>(w, ldw, w_plane, ldwp, rows_w, K, stream);
    }
    const int64_t kw = (K + 7) / 8;
    if (ldxp < kw || ldwp < kw || (ldxp & 3) || (ldwp & 3) || !qt_aligned16(x_plane) || !qt_aligned16(w_plane))
        return QT_ERR_ALIGNMENT;
    if (!pack_fits_32bit(rows_x, ldxp) || !pack_fits_32bit(rows_w, ldwp)) {
        const int rc = launch_nib_pack<NibSign, E>(x, ldx, x_plane, ldxp, rows_x, K, stream);
        if (rc != QT_OK) return rc;
        return w_ternary ? launch_nib_pack<NibTernary, E>(w, ldw, w_plane, ldwp, rows_w, K, stream)
                         : launch_nib_pack<NibSign, E>(w, ldw, w_plane, ldwp, rows_w, K, stream);
    }
    // workgroups (4 waves each) split between the operands in proportion to their units, at least one each
    const int64_t ua = pack_units(rows_x, ldxp, 8 / EPV), ub = pack_units(rows_w, ldwp, 8 / EPV);
    const int grid = qt_stream_grid((ua + 3) / 4 + (ub + 3) / 4);   // >= 2: both operands have rows and K > 0
    const int ga = (int)std::min<int64_t>(std::max<int64_t>(1, (grid * ua + (ua + ub) / 2) / (ua + ub)), grid - 1);
    if (w_ternary)
        hipLaunchKernelGGL((nib_pack_pair_kernel<NibTernary, E>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ldx,
                           x_plane, ldxp, (int)rows_x, w, ldw, w_plane, ldwp, (int)rows_w, (int)(K / EPV), ga);
    else
        hipLaunchKernelGGL((nib_pack_pair_kernel<NibSign, E>), dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ldx,
                           x_plane, ldxp, (int)rows_x, w, ldw, w_plane, ldwp, (int)rows_w, (int)(K / EPV), ga);
    return qt_check_launch();
}

}  // namespace

// code_conv3x3.hip
int qt_code_conv3x3_try(const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                        int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias, float scale,
                        const float* scale_dev, const float* alpha, const float* beta, const float* res_f32, const float* res_alpha,
                        const int8_t* res_codes, int64_t ldrc_bytes, float res_scale, int relu, int bit_width, int8_t* codes,
                        int64_t ldc_bytes, int64_t Cout, int32_t* overflow, int64_t ihy, int64_t ihx, int64_t ohy, int64_t ohx,
                        int64_t rhy, int64_t rhx, const float* bn_stats, qt_stream_t stream);

extern "C" {

int qt_sign_pack_nib_f32(const float* x, int64_t ldx, uint32_t* nib_plane, int64_t ldp, int64_t rows,
                         int64_t K, qt_stream_t stream) {
    return launch_nib_pack<NibSign>(x, ldx, nib_plane, ldp, rows, K, stream);
}

int qt_ternary_pack_nib_f32(const float* x, int64_t ldx, uint32_t* nib_plane, int64_t ldp,
                            int64_t rows, int64_t K, qt_stream_t stream) {
    return launch_nib_pack<NibTernary>(x, ldx, nib_plane, ldp, rows, K, stream);
}

int qt_sign0_pack_nib_f32(const float* x, int64_t ldx, uint32_t* nib_plane, int64_t ldp, int64_t rows, int64_t K,
                          qt_stream_t stream) {
    return launch_nib_pack<NibSign0>(x, ldx, nib_plane, ldp, rows, K, stream);
}

int qt_pack_pair_nib_f32(const float* x, int64_t ldx, uint32_t* x_plane, int64_t ldxp, int64_t rows_x,
                         const float* w, int64_t ldw, uint32_t* w_plane, int64_t ldwp, int64_t rows_w, int64_t K,
                         int w_ternary, qt_stream_t stream) {
    return pack_pair_any<EltF32>(x, ldx, x_plane, ldxp, rows_x, w, ldw, w_plane, ldwp, rows_w, K, w_ternary, stream);
}

int qt_sign_pack_nib_h(const void* x, int dtype, int64_t ldx, uint32_t* nib_plane, int64_t ldp, int64_t rows, int64_t K,
                       qt_stream_t stream) {
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    if (dtype == QT_DTYPE_BF16) return launch_nib_pack<NibSign, EltBf16>(xh, ldx, nib_plane, ldp, rows, K, stream);
    if (dtype == QT_DTYPE_F16) return launch_nib_pack<NibSign, EltF16>(xh, ldx, nib_plane, ldp, rows, K, stream);
    return QT_ERR_INVALID_ARG;
}

int qt_ternary_pack_nib_h(const void* x, int dtype, int64_t ldx, uint32_t* nib_plane, int64_t ldp, int64_t rows, int64_t K,
                          qt_stream_t stream) {
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    if (dtype == QT_DTYPE_BF16) return launch_nib_pack<NibTernary, EltBf16>(xh, ldx, nib_plane, ldp, rows, K, stream);
    if (dtype == QT_DTYPE_F16) return launch_nib_pack<NibTernary, EltF16>(xh, ldx, nib_plane, ldp, rows, K, stream);
    return QT_ERR_INVALID_ARG;
}

int qt_pack_pair_nib_h(const void* x, int dtype, int64_t ldx, uint32_t* x_plane, int64_t ldxp, int64_t rows_x, const void* w,
                       int64_t ldw, uint32_t* w_plane, int64_t ldwp, int64_t rows_w, int64_t K, int w_ternary,
                       qt_stream_t stream) {
    const uint16_t *xh = static_cast<const uint16_t*>(x), *wh = static_cast<const uint16_t*>(w);
    if (dtype == QT_DTYPE_BF16)
        return pack_pair_any<EltBf16>(xh, ldx, x_plane, ldxp, rows_x, wh, ldw, w_plane, ldwp, rows_w, K, w_ternary, stream);
    if (dtype == QT_DTYPE_F16)
        return pack_pair_any<EltF16>(xh, ldx, x_plane, ldxp, rows_x, wh, ldw, w_plane, ldwp, rows_w, K, w_ternary, stream);
    return QT_ERR_INVALID_ARG;
}

int qt_nib_gemm_variant(int variant, const uint32_t* Xn, int64_t ldxp, const uint32_t* Wn,
                        int64_t ldwp, const float* bias, float* Y, int64_t ldy, int64_t M, int64_t N,
                        int64_t K, qt_stream_t stream) {
    const int rc = check_common(Xn, ldxp, Wn, ldwp, Y, ldy, M, N, K, (K + 7) / 8);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    if (K >= (1 << 24)) return QT_ERR_UNSUPPORTED;  // fp32-exact bound of the accumulator
    return dispatch_gemm<ElemFp4>(variant, Xn, ldxp, Wn, ldwp, bias, 1.0f, nullptr, Y, ldy, M, N, K, stream);
}

int qt_nib_gemm_describe(int64_t M, int64_t N, int64_t K, int64_t ldxp, int64_t ldwp, char* out, int cap) {
    // the tile configuration the automatic rule (select_gemm, which dispatch_gemm_auto launches from) gives this shape:
    // "<kernel><element, tile, pipeline>"
    if (!out || cap < 2 || M <= 0 || N <= 0 || K < 0) return QT_ERR_INVALID_ARG;
    snprintf(out, (size_t)cap, "mfma_gemm_kernel<ElemFp4, %s>", gemm_tile_text(select_gemm(M, N, ldxp, ldwp)));
    return QT_OK;
}

int qt_nib_gemm(const uint32_t* Xn, int64_t ldxp, const uint32_t* Wn, int64_t ldwp, const float* bias,
                float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, qt_stream_t stream) {
    return qt_nib_gemm_variant(0, Xn, ldxp, Wn, ldwp, bias, Y, ldy, M, N, K, stream);
}

int qt_nib_gemm_h(const uint32_t* Xn, int64_t ldxp, const uint32_t* Wn, int64_t ldwp, const float* bias, void* Y, int dtype,
                  int64_t ldy, int64_t M, int64_t N, int64_t K, qt_stream_t stream) {
    if (dtype != QT_DTYPE_BF16 && dtype != QT_DTYPE_F16) return QT_ERR_INVALID_ARG;
    float* Yf = static_cast<float*>(Y);          // the kernel's pointer type; the half epilogue re-types it
    const int rc = check_common(Xn, ldxp, Wn, ldwp, Yf, ldy, M, N, K, (K + 7) / 8);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    if (K >= (1 << 24)) return QT_ERR_UNSUPPORTED;  // fp32-exact bound of the accumulator
    if (dtype == QT_DTYPE_BF16)
        return dispatch_gemm_auto<ElemFp4Out<1>>(Xn, ldxp, Wn, ldwp, bias, 1.0f, nullptr, Yf, ldy, M, N, K, stream);
    return dispatch_gemm_auto<ElemFp4Out<2>>(Xn, ldxp, Wn, ldwp, bias, 1.0f, nullptr, Yf, ldy, M, N, K, stream);
}

int qt_bf16_gemm(const uint32_t* Xh, int64_t ldxp, const uint32_t* Wh, int64_t ldwp, const float* bias,
                 float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, qt_stream_t stream) {
    const int rc = check_common(Xh, ldxp, Wh, ldwp, Y, ldy, M, N, K, (K + 1) / 2);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    return dispatch_gemm<ElemBf16>(0, Xh, ldxp, Wh, ldwp, bias, 1.0f, nullptr, Y, ldy, M, N, K, stream);
}

int qt_f16_gemm(const uint32_t* Xh, int64_t ldxp, const uint32_t* Wh, int64_t ldwp, const float* bias, float scale,
                const float* scale_dev, float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, qt_stream_t stream) {
    const int rc = check_common(Xh, ldxp, Wh, ldwp, Y, ldy, M, N, K, (K + 1) / 2);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    return dispatch_gemm<ElemF16>(0, Xh, ldxp, Wh, ldwp, bias, scale, scale_dev, Y, ldy, M, N, K, stream);
}

int qt_bf16_gemm_taps(const uint32_t* Xh, int64_t ldxp, const uint32_t* Wh, int64_t ldwp, float* Y, int64_t ldy,
                      int64_t M, int64_t N, int64_t K, int64_t tap_rows, int64_t tap_cols, int64_t nslice,
                      int64_t w_copy_bytes, int64_t w_row_bytes, int64_t y_stride, qt_stream_t stream) {
    const int rc = check_common(Xh, ldxp, Wh, ldwp, Y, ldy, M, N, K, 0);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    if (tap_rows < 1 || tap_cols < 1 || nslice < 1 || tap_rows * tap_cols * nslice > 65535) return QT_ERR_INVALID_ARG;
    if (K <= 0 || (K & 31)) return QT_ERR_ALIGNMENT;                       // whole 64-byte stages per slice
    if ((w_copy_bytes | w_row_bytes) & 15) return QT_ERR_ALIGNMENT;        // every tap's W base stays 16-byte aligned
    if (y_stride < M * ldy || (ldy & 3) || !qt_aligned16(Y) || (y_stride & 3)) return QT_ERR_ALIGNMENT;
    if (!gemm_pipe_ok(M, N, ldxp, ldwp)) return QT_ERR_UNSUPPORTED;
    ConvArgs cg{};
    cg.H = (int)(tap_rows * tap_cols);
    cg.z_nslice = (int)nslice;
    cg.z_kw = (int)tap_cols;
    cg.z_kslice_bytes = K * 2;
    cg.z_w_copy_bytes = w_copy_bytes;
    cg.z_w_row_bytes = w_row_bytes;
    cg.z_y_stride = y_stride;
    return launch_gemm_batched<ElemBf16, true>(select_gemm_batched(M, N, true), Xh, ldxp, Wh, ldwp, nullptr, 1.0f, nullptr, Y, ldy, M, N, K, stream, cg);
}

int qt_i8_gemm(const uint32_t* Xc, int64_t ldxp, const uint32_t* Wc, int64_t ldwp, const float* bias,
               float scale, const float* scale_dev, int64_t max_abs_code, float* Y, int64_t ldy, int64_t M,
               int64_t N, int64_t K, qt_stream_t stream) {
    const int rc = check_common(Xc, ldxp, Wc, ldwp, Y, ldy, M, N, K, (K + 3) / 4);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    // max_abs_code bounds |x code * w code| (127 for +-1/0 weight codes, up to 127*127 for k-bit weight codes):
    // |sum| <= max_abs_code * K must fit the int32 accumulator; below 2^24 the int32 -> fp32 conversion in
    // the epilogue is exact as well (the +-1/0 weight case), above it rounds once (relative 6e-8)
    if (max_abs_code < 0 || max_abs_code > 127 * 127 || max_abs_code * K >= (1ll << 31)) return QT_ERR_UNSUPPORTED;
    return dispatch_gemm<ElemI8>(0, Xc, ldxp, Wc, ldwp, bias, scale, scale_dev, Y, ldy, M, N, K, stream);
}

// Split-K form of qt_i8_gemm for skinny problems (few row tiles, long K: the digit-plane GEMM of LinearXNOR at batch 256):
// blockIdx.y = K slice, slice z contracts bytes [z * kslice, (z + 1) * kslice) of every row and writes its exact integer partial
// sums (as fp32, no scale, no bias) to Y + z * y_stride — 256 x 256 tiles keep the operand bytes per MAC low, the slices fill the
// CUs the few tiles leave idle.  The planes must hold nslice * kslice bytes per row (zero padded).
int qt_i8_gemm_splitk(const uint32_t* Xc, int64_t ldxp, const uint32_t* Wc, int64_t ldwp, float* Y, int64_t ldy, int64_t M, int64_t N,
                      int64_t kslice, int64_t nslice, int64_t y_stride, qt_stream_t stream) {
    const int rc = check_common(Xc, ldxp, Wc, ldwp, Y, ldy, M, N, kslice * nslice, (kslice * nslice + 3) / 4);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    if (nslice < 1 || nslice > 65535 || kslice <= 0 || (kslice & 63)) return QT_ERR_ALIGNMENT;          // whole 64-byte stages per slice
    if (127 * kslice * nslice >= (1ll << 24)) return QT_ERR_UNSUPPORTED;                                 // partial sums exact in fp32
    if (y_stride < M * ldy || (ldy & 3) || !qt_aligned16(Y) || (y_stride & 3)) return QT_ERR_ALIGNMENT;
    if (!gemm_pipe_ok(M, N, ldxp, ldwp)) return QT_ERR_UNSUPPORTED;
    ConvArgs cg{};
    cg.H = 1;
    cg.z_nslice = (int)nslice;
    cg.z_kw = 1;
    cg.z_kslice_bytes = kslice;
    cg.z_y_stride = y_stride;
    return launch_gemm_batched<ElemI8, false>(select_gemm_batched(M, N, false), Xc, ldxp, Wc, ldwp, nullptr, 1.0f, nullptr, Y, ldy, M, N, kslice, stream, cg);
}

// conv kernel variant = tile form | QT_CONV_* flags (an ARGUMENT: qt_conv2d_implicit_variant takes both, the bits / nib / codes entries
// the flags only, every other entry point passes 0; no environment is read in a default build).  Tile form: 0 = automatic
// (192-wide tiles: ping-pong on a 384x192 tile, whose 96x96 wave tiles keep the load segment under the compute segment:
// AlexNet conv2 302 -> 275 us; other widths: double-buffered, equal or faster there), 1 = double-buffered, 2 = ping-pong,
// 4 = automatic without the un-padded fast path; 3 = stamped 384x192 ping-pong, only in -DQT_PROFILING_VARIANTS builds

// What conv_implicit_impl launches, worked out from the numbers alone (the describe entry point calls this and stops here).
enum class ConvElem { Fp4, Fp4T, Fp4OutBf16, Fp4OutF16, I8, F16, Bf16, Bf16L };
struct ConvPlan {
    ConvArgs cg;
    int64_t M, K, p_offset;
    TileCfg cfg;
    ConvElem elem;
};
static int conv_plan(int elem, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                     int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t ldwp, int64_t ldy, int64_t Cout, EpiArgs& epi, int64_t hy,
                     int64_t hx, int variant, int out_dtype, ConvPtrs ptrs, ConvPlan& pl) {
    int form = variant & 0xf;          // the entry points have refused unknown bits
#ifdef QT_EXPERIMENT   // A/B builds only (make EXTRA=-DQT_EXPERIMENT): a variant for the entry points that take none
    if (form == 0 && getenv("QT_CONV_FORCE_EXP")) form = atoi(getenv("QT_CONV_FORCE_EXP"));
#endif
    bool valid;
    int64_t kwords;
    const int rc = conv_geometry(elem, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, ldwp, ldy, Cout, epi, hy, hx, ptrs, pl.cg, valid,
                                 pl.M, pl.K, kwords, pl.p_offset);
    if (rc != QT_OK) return rc;
    // weights-as-rows threshold epilogue (sign-bit form): fp4, integer thresholds, whole 32-channel blocks, bit plane or nibble plane
    // out, no depth-to-space; QT_CONV_COMPARE_THRESHOLDS: the compare form (A/B runs and the bit-identity test)
    const bool swapt = elem == 0 && epi.alpha && epi.thr && (Cout & 31) == 0 && !epi.d2s_cout && (epi.mode == 0 || epi.mode == 3) &&
                       !(variant & QT_CONV_COMPARE_THRESHOLDS);
    // the level epilogue (mode 5) walks the tiles of the plain conv of its geometry: the accumulators are then the same bits
    const bool plain_tiles = (!epi.alpha && epi.mode == 0) || epi.mode == 5;
    const ConvChoice pick = select_conv({pl.M, Cout, kwords * 4, ldwp, valid, epi.d2s_cout != 0, plain_tiles, epi.alpha != nullptr, form,
                                         variant & QT_CONV_FLAGS_MASK});
    if (pick.cfg == TileCfg::None) return QT_ERR_UNSUPPORTED;
    pl.cfg = pick.cfg;
    pl.elem = elem == 0 && out_dtype == QT_DTYPE_BF16 ? ConvElem::Fp4OutBf16
              : elem == 0 && out_dtype == QT_DTYPE_F16 ? ConvElem::Fp4OutF16
              : elem == 0 ? (swapt && pick.sign_bit_capable ? ConvElem::Fp4T : ConvElem::Fp4)
              : elem == 1 ? ConvElem::I8
              : elem == 3 ? ConvElem::F16
              : epi.mode == 5 ? ConvElem::Bf16L : ConvElem::Bf16;
    return QT_OK;
}

// elem: 0 = fp4 nibble planes, 1 = int8 code planes, 2 = bf16 (triple) planes, 3 = fp16 (pair) planes.  epi.alpha != nullptr:
// Y is the threshold-bit plane and ldy its row stride in words.
static int conv_implicit_impl(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                              int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                              int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias, float scale,
                              const float* scale_dev, float* Y, int64_t ldy, int64_t Cout, qt_stream_t stream,
                              const EpiArgs& epi_in, int64_t hy = 0, int64_t hx = 0, int variant = 0, int out_dtype = 0) {
    // out_dtype (fp4 planes, plain epilogue only): QT_DTYPE_BF16 / QT_DTYPE_F16 = Y holds 2-byte elements (ElemFp4Out)
    // (hy, hx): halo of the INPUT plane, [N][H + 2hy][W + 2hx][Cw] with a zero border: a conv whose padding fits in
    // the halo runs as the un-padded conv on the window that starts (hy - ph, hx - pw) into the plane.
    EpiArgs epi = epi_in;
    ConvPlan pl;
    const int rc = conv_plan(elem, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, ldwp, ldy, Cout, epi, hy, hx, variant, out_dtype,
                             conv_check_pointers(P, Wmat, Y), pl);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    P += pl.p_offset;
    const bool t = pl.elem == ConvElem::Fp4T;
    switch (pl.elem) {
#define QT_CONV_AS(E) return launch_conv<E>(pl.cfg, t, P, 0, Wmat, ldwp, bias, scale, scale_dev, Y, ldy, pl.M, Cout, pl.K, stream, pl.cg, epi)
        case ConvElem::Fp4OutBf16: QT_CONV_AS(ElemFp4Out<1>);
        case ConvElem::Fp4OutF16: QT_CONV_AS(ElemFp4Out<2>);
        case ConvElem::Fp4: case ConvElem::Fp4T: QT_CONV_AS(ElemFp4);
        case ConvElem::I8: QT_CONV_AS(ElemI8);
        case ConvElem::F16: QT_CONV_AS(ElemF16);
        case ConvElem::Bf16L: QT_CONV_AS(ElemBf16L);
        case ConvElem::Bf16: QT_CONV_AS(ElemBf16);
#undef QT_CONV_AS
    }
    return QT_ERR_UNSUPPORTED;
}

int qt_conv2d_implicit_variant(int variant, int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                               int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                               int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias, float scale,
                               const float* scale_dev, float* Y, int64_t ldy, int64_t Cout, qt_stream_t stream) {
    if (variant < 0 || (variant & ~(0xf | QT_CONV_FLAGS_MASK)) || (variant & 0xf) > 6) return QT_ERR_INVALID_ARG;
    return conv_implicit_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale,
                              scale_dev, Y, ldy, Cout, stream, EpiArgs{}, 0, 0, variant);
}

int qt_conv2d_implicit(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                       int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                       int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias, float scale,
                       const float* scale_dev, float* Y, int64_t ldy, int64_t Cout, qt_stream_t stream) {
    return conv_implicit_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale,
                              scale_dev, Y, ldy, Cout, stream, EpiArgs{});
}

int qt_conv2d_implicit_h(const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh,
                         int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat, int64_t ldwp,
                         const float* bias, void* Y, int dtype, int64_t ldy, int64_t Cout, qt_stream_t stream) {
    if (dtype != QT_DTYPE_BF16 && dtype != QT_DTYPE_F16) return QT_ERR_INVALID_ARG;
    return conv_implicit_impl(0, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, 1.0f, nullptr,
                              static_cast<float*>(Y), ldy, Cout, stream, EpiArgs{}, 0, 0, 0, dtype);
}

int qt_conv2d_implicit_bits(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                            int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                            int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias, float scale,
                            const float* scale_dev, const float* alpha, const float* beta, const float* thr,
                            uint32_t* neg_plane, int64_t ldb, int64_t Cout, int flags, qt_stream_t stream) {
    if (!alpha || !beta || (flags & ~QT_CONV_FLAGS_MASK)) return QT_ERR_INVALID_ARG;
    if (thr && elem >= 2) return QT_ERR_INVALID_ARG;       // integer thresholds need integer accumulators
    if (ldb & 3) return QT_ERR_ALIGNMENT;
    EpiArgs epi;
    epi.alpha = alpha;
    epi.beta = beta;
    epi.thr = thr;
    return conv_implicit_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale,
                              scale_dev, reinterpret_cast<float*>(neg_plane), ldb, Cout, stream, epi, 0, 0, flags);
}

int qt_conv2d_implicit_nib(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                           int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                           int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias, float scale,
                           const float* scale_dev, const float* alpha, const float* beta, const float* thr,
                           uint32_t* nib_plane, int64_t ldn, int64_t Cout, int64_t out_halo_h, int64_t out_halo_w,
                           int64_t d2s_cout, int flags, qt_stream_t stream) {
    if (!alpha || !beta || (flags & ~QT_CONV_FLAGS_MASK)) return QT_ERR_INVALID_ARG;
    if (thr && elem >= 2) return QT_ERR_INVALID_ARG;       // integer thresholds need integer accumulators
    if (out_halo_h < 0 || out_halo_w < 0 || out_halo_h > 64 || out_halo_w > 64) return QT_ERR_INVALID_ARG;
    if ((ldn & 3) || !qt_aligned16(nib_plane)) return QT_ERR_ALIGNMENT;
    if (d2s_cout < 0 || (d2s_cout && (d2s_cout % 32 || Cout != 4 * d2s_cout))) return QT_ERR_INVALID_ARG;
    // every word of a pixel is written by a column block
    if (ldn != ((d2s_cout ? d2s_cout : Cout) + 31) / 32 * 4) return QT_ERR_INVALID_ARG;
    EpiArgs epi;
    epi.alpha = alpha;
    epi.beta = beta;
    epi.mode = 3;
    epi.thr = thr;
    epi.ohy = (int)out_halo_h;
    epi.ohx = (int)out_halo_w;
    epi.d2s_cout = (int)d2s_cout;
    return conv_implicit_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale,
                              scale_dev, reinterpret_cast<float*>(nib_plane), ldn, Cout, stream, epi, 0, 0, flags);
}

int qt_conv2d_implicit_codes(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                             int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh,
                             int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias, float scale,
                             const float* scale_dev, const float* alpha, const float* beta, const float* res_f32,
                             int64_t ldr, const float* res_alpha, const float* res_beta, const int8_t* res_codes,
                             int64_t ldrc_bytes, float res_scale, int relu, int bit_width, int8_t* codes,
                             int64_t ldc_bytes, int64_t Cout, int32_t* overflow, int64_t in_halo_h,
                             int64_t in_halo_w, int64_t out_halo_h, int64_t out_halo_w, int64_t res_halo_h,
                             int64_t res_halo_w, const float* bn_stats, const float* res_bn_stats, int flags,
                             qt_stream_t stream) {
    if (flags & ~QT_CONV_FLAGS_MASK) return QT_ERR_INVALID_ARG;
    if (res_bn_stats || (bn_stats && res_alpha)) return QT_ERR_UNSUPPORTED;   // device form: the residual arrives normalised
    if (!alpha || !beta || !overflow || bit_width < 2 || bit_width > 8 || relu < 0 || relu > 2) return QT_ERR_INVALID_ARG;
    if (out_halo_h < 0 || out_halo_w < 0 || res_halo_h < 0 || res_halo_w < 0 || out_halo_h > 64 || out_halo_w > 64 ||
        res_halo_h > 64 || res_halo_w > 64 || ((res_halo_h | res_halo_w) && !res_codes))
        return QT_ERR_INVALID_ARG;
    if (elem != 1) return QT_ERR_UNSUPPORTED;   // the epilogue is instantiated for the int8 (DoReFa) configs
    if ((res_f32 && ldr < Cout) || (!res_alpha != !res_beta) || (res_alpha && !res_f32)) return QT_ERR_INVALID_ARG;
    if ((ldc_bytes & 15) || !qt_aligned16(codes)) return QT_ERR_ALIGNMENT;
    if (res_codes && (ldrc_bytes < ((Cout + 3) & ~3ll) || (ldrc_bytes & 3) || (reinterpret_cast<uintptr_t>(res_codes) & 3)))
        return QT_ERR_ALIGNMENT;
    EpiArgs epi;
    epi.alpha = alpha;
    epi.beta = beta;
    epi.mode = 2;
    epi.relu = relu;
    epi.levels = (float)((1 << bit_width) - 1);
    epi.res_f32 = res_f32;
    epi.ldr = ldr;
    epi.ralpha = res_alpha;
    epi.rbeta = res_beta;
    epi.res_codes = res_codes;
    epi.ldrc = ldrc_bytes;
    epi.rscale = res_scale;
    epi.overflow = overflow;
    epi.ohy = (int)out_halo_h;
    epi.ohx = (int)out_halo_w;
    epi.rhy = (int)res_halo_h;
    epi.rhx = (int)res_halo_w;
    epi.bn_stats = bn_stats;
    // small-channel 3 x 3 / stride 1 layers: the persistent direct kernel (code_conv3x3.hip), bit-identical codes
    if (!(flags & QT_CONV_NO_DIRECT_CODES)) {
        const int rc = qt_code_conv3x3_try(P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale, scale_dev, alpha,
                                           beta, res_f32, res_alpha, res_codes, ldrc_bytes, res_scale, relu, bit_width, codes, ldc_bytes,
                                           Cout, overflow, in_halo_h, in_halo_w, out_halo_h, out_halo_w, res_halo_h, res_halo_w, bn_stats,
                                           stream);
        if (rc != QT_ERR_UNSUPPORTED) return rc;
    }
    return conv_implicit_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale,
                              scale_dev, reinterpret_cast<float*>(codes), ldc_bytes, Cout, stream, epi, in_halo_h,
                              in_halo_w, flags);
}

int qt_conv2d_implicit_levels(const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t in_halo_h, int64_t in_halo_w,
                              int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw,
                              const uint32_t* Wmat, int64_t ldwp, const float* bias, const float* bn_weight, const float* bn_bias,
                              const float* bn_stats, int relu, int dtype, int fsr, int bit_width, int mode, uint16_t* plane,
                              int64_t ld_bytes, int64_t Cout, int64_t out_halo_h, int64_t out_halo_w, qt_stream_t stream) {
    if (!bn_weight || !bn_bias || !bn_stats || !plane || relu < 0 || relu > 1) return QT_ERR_INVALID_ARG;
    if (out_halo_h < 0 || out_halo_w < 0 || out_halo_h > 64 || out_halo_w > 64) return QT_ERR_INVALID_ARG;
    if (!qt_aligned16(plane)) return QT_ERR_ALIGNMENT;
    if (ld_bytes != ((2 * Cout + 15) & ~15ll)) return QT_ERR_INVALID_ARG;      // every byte of a pixel is written by a column block
    EpiArgs epi;
    epi.alpha = bn_weight;
    epi.beta = bn_bias;
    epi.bn_stats = bn_stats;
    epi.mode = 5;
    epi.relu = relu;
    epi.lq_kind = dtype;
    epi.lq_mode = mode;
    {   // the parameter windows of qt_linlog_quantize_bf16_f32: every level one bf16 term
        const int rc = qt_act_level_params(dtype, fsr, bit_width, mode, epi.lq_a, epi.lq_b);
        if (rc != QT_OK) return rc;
    }
    epi.ohy = (int)out_halo_h;
    epi.ohx = (int)out_halo_w;
    return conv_implicit_impl(2, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, 1.0f, nullptr,
                              reinterpret_cast<float*>(plane), ld_bytes, Cout, stream, epi, in_halo_h, in_halo_w);
}

int qt_conv2d_implicit_halo(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                            int64_t halo_h, int64_t halo_w, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                            int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat, int64_t ldwp,
                            const float* bias, float scale, const float* scale_dev, float* Y, int64_t ldy,
                            int64_t Cout, qt_stream_t stream) {
    return conv_implicit_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale,
                              scale_dev, Y, ldy, Cout, stream, EpiArgs{}, halo_h, halo_w);
}

int qt_conv2d_implicit_halo_bn(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw,
                               int64_t halo_h, int64_t halo_w, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                               int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat, int64_t ldwp,
                               const float* bias, float scale, const float* scale_dev, const float* bn_weight,
                               const float* bn_bias, const float* bn_stats, float* Y, int64_t ldy, int64_t Cout,
                               qt_stream_t stream) {
    if (!bn_weight || !bn_bias || !bn_stats || ldy < Cout) return QT_ERR_INVALID_ARG;
    if (elem != 1) return QT_ERR_UNSUPPORTED;               // instantiated for the int8 (DoReFa) configurations
    if ((Cout & 3) || (ldy & 3) || !qt_aligned16(Y) || !qt_aligned16(bn_weight) || !qt_aligned16(bn_bias) || !qt_aligned16(bn_stats))
        return QT_ERR_ALIGNMENT;
    EpiArgs epi;
    epi.alpha = bn_weight;
    epi.beta = bn_bias;
    epi.bn_stats = bn_stats;
    epi.mode = 4;
    return conv_implicit_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale,
                              scale_dev, Y, ldy, Cout, stream, epi, halo_h, halo_w);
}

int qt_conv2d_implicit_describe(int elem, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                                int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t ldwp, int64_t Cout, int64_t in_halo_h,
                                int64_t in_halo_w, int epilogue, int has_thr, int64_t d2s_cout, int variant, char* out, int cap) {
    // The entry point of this epilogue with a dense output plane, up to the launch: its own argument checks on the numbers, then
    // conv_plan — the function conv_implicit_impl launches from.
    if (!out || cap < 2) return QT_ERR_INVALID_ARG;
    out[0] = 0;
    if (variant < 0 || (variant & ~(0xf | QT_CONV_FLAGS_MASK)) || (variant & 0xf) > 6) return QT_ERR_INVALID_ARG;
    const bool halo = (in_halo_h | in_halo_w) != 0;
    if ((epilogue != QT_EPI_PLAIN && (variant & 0xf)) || (has_thr && epilogue != QT_EPI_BITS && epilogue != QT_EPI_NIB) ||
        (d2s_cout && epilogue != QT_EPI_NIB))
        return QT_ERR_INVALID_ARG;         // no entry point takes these together
    static const float some = 0.0f;        // "a pointer was given": nothing is read through it
    EpiArgs epi;
    int64_t ldy = Cout;
    int out_dtype = 0;
    switch (epilogue) {
        case QT_EPI_PLAIN: break;
        case QT_EPI_HALF_BF16: case QT_EPI_HALF_F16:
            if (elem != 0 || halo) return QT_ERR_INVALID_ARG;
            out_dtype = epilogue == QT_EPI_HALF_BF16 ? QT_DTYPE_BF16 : QT_DTYPE_F16;
            break;
        case QT_EPI_BITS: case QT_EPI_NIB:
            if (halo || (has_thr && elem >= 2)) return QT_ERR_INVALID_ARG;
            epi.alpha = epi.beta = &some;
            epi.thr = has_thr ? &some : nullptr;
            ldy = ((Cout + 31) / 32 + 3) & ~3ll;
            if (epilogue == QT_EPI_NIB) {
                if (d2s_cout < 0 || (d2s_cout && (d2s_cout % 32 || Cout != 4 * d2s_cout))) return QT_ERR_INVALID_ARG;
                epi.mode = 3;
                epi.d2s_cout = (int)d2s_cout;
                ldy = ((d2s_cout ? d2s_cout : Cout) + 31) / 32 * 4;
            }
            break;
        case QT_EPI_CODES:
            if (elem != 1) return QT_ERR_UNSUPPORTED;
            epi.alpha = epi.beta = &some;
            epi.mode = 2;
            ldy = (Cout + 15) & ~15ll;
            break;
        case QT_EPI_HALO_BN:
            if (elem != 1) return QT_ERR_UNSUPPORTED;
            if (Cout & 3) return QT_ERR_ALIGNMENT;
            epi.alpha = epi.beta = epi.bn_stats = &some;
            epi.mode = 4;
            break;
        case QT_EPI_LEVELS:
            if (elem != 2) return QT_ERR_INVALID_ARG;
            epi.alpha = epi.beta = epi.bn_stats = &some;
            epi.mode = 5;
            ldy = (2 * Cout + 15) & ~15ll;
            break;
        default: return QT_ERR_INVALID_ARG;
    }
    ConvPlan pl;
    const int rc = conv_plan(elem, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, ldwp, ldy, Cout, epi, in_halo_h, in_halo_w, variant,
                             out_dtype, ConvPtrs{true, true}, pl);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;      // nothing to do: QT_OK and an empty name
    static const char* const elem_name[] = {"ElemFp4", "ElemFp4T", "ElemFp4Out<1>", "ElemFp4Out<2>", "ElemI8", "ElemF16", "ElemBf16", "ElemBf16L"};
    snprintf(out, (size_t)cap, "%s<%s>", tile_cfg_name(pl.cfg), elem_name[(int)pl.elem]);
    return QT_OK;
}

int qt_gemm_tile_describe(int family, int variant, int64_t M, int64_t N, int64_t ldxp, int64_t ldwp, char* out, int cap) {
    if (!out || cap < 2 || M <= 0 || N <= 0) return QT_ERR_INVALID_ARG;
    out[0] = 0;
    TileCfg cfg;
    if (family == QT_GEMM_FAMILY_DENSE) {
        if (variant == 0) {
            cfg = select_gemm(M, N, ldxp, ldwp);
        } else {
            const int rc = gemm_variant_cfg(variant, gemm_pipe_ok(M, N, ldxp, ldwp), ldxp, ldwp, &cfg);
            if (rc != QT_OK) return rc;
        }
    } else if (family == QT_GEMM_FAMILY_BF16_TAPS || family == QT_GEMM_FAMILY_I8_SPLITK) {
        if (variant != 0) return QT_ERR_INVALID_ARG;
        if (!gemm_pipe_ok(M, N, ldxp, ldwp)) return QT_ERR_UNSUPPORTED;
        cfg = select_gemm_batched(M, N, family == QT_GEMM_FAMILY_BF16_TAPS);
    } else {
        return QT_ERR_INVALID_ARG;
    }
    snprintf(out, (size_t)cap, "%s", tile_cfg_name(cfg));
    return QT_OK;
}

int qt_bits_to_nib(const uint32_t* sign_plane, const uint32_t* mask_plane, int64_t ldb,
                   uint32_t* nib_plane, int64_t ldn, int64_t rows, int64_t K, qt_stream_t stream) {
    if (rows < 0 || K < 0) return QT_ERR_INVALID_ARG;
    if (rows == 0) return QT_OK;
    if (!nib_plane || (K > 0 && !sign_plane)) return QT_ERR_INVALID_ARG;
    if (ldb < (K + 31) / 32 || ldn < (K + 7) / 8) return QT_ERR_INVALID_ARG;
    if ((ldb & 3) || (ldn & 3) || !qt_aligned16(nib_plane)) return QT_ERR_ALIGNMENT;
    const int grid = qt_stream_grid((rows * (ldn / 4) + 255) / 256);
    hipLaunchKernelGGL(bits_to_nib_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, sign_plane,
                       mask_plane, ldb, nib_plane, ldn, rows, K);
    return qt_check_launch();
}

int qt_bits_to_nib_pad(const uint32_t* sign_plane, const uint32_t* mask_plane, int64_t ldb, uint32_t* nib_plane,
                       int64_t ldn, int64_t N, int64_t H, int64_t W, int64_t ph, int64_t pw, int64_t K,
                       qt_stream_t stream) {
    if (N < 0 || H <= 0 || W <= 0 || ph < 0 || pw < 0 || K < 0) return QT_ERR_INVALID_ARG;
    if (N == 0) return QT_OK;
    if (!nib_plane || (K > 0 && !sign_plane)) return QT_ERR_INVALID_ARG;
    if (ldb < (K + 31) / 32 || ldn < (K + 7) / 8) return QT_ERR_INVALID_ARG;
    if ((ldb & 3) || (ldn & 3) || !qt_aligned16(nib_plane)) return QT_ERR_ALIGNMENT;
    if (H + 2 * ph > 32767 || W + 2 * pw > 32767) return QT_ERR_UNSUPPORTED;
    const int64_t total = N * (H + 2 * ph) * (W + 2 * pw) * (ldn / 4);
    const int grid = qt_stream_grid((total + 255) / 256);
    hipLaunchKernelGGL(bits_to_nib_pad_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, sign_plane, mask_plane,
                       ldb, nib_plane, ldn, N, (int)H, (int)W, (int)ph, (int)pw, K);
    return qt_check_launch();
}

}  // extern "C"
