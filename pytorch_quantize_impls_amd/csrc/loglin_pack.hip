// Quantise-and-pack of Lin / Log fixed-point weights for a training step (layers/log_lin_layers.py, functions/_fused.py
// LogLinLinearFn / LogLinConv2dFn).  One read of the fp32 master weight [Cout][Cin][kh][kw] (element strides: contiguous,
// channels-last, or a Linear weight [N][K] as kh = kw = 1) applies the Lin / Log quantiser (loglin_quant.h: the bits of
// qt_lin_quantize_f32 / qt_log_quantize_f32) and writes, each optional:
//   fwd  the forward operand: bf16_rn(q) replicated into the three slots of a bf16-triple plane, rows = Cout, tap-major with
//        16-byte tap granules (Cb = 6*Cin rounded up to 16 bytes), rows zero-padded to ld = max(128, kh*kw*Cb rounded to 128);
//        for kh = kw = 1 this is exactly the plane of qt_bf16x3_pack_f32(mode 4) with a 128-byte row granule;
//   gx   the grad_x operand: the same plane of q.flip(2, 3).transpose(0, 1) — rows = Cin, channels = Cout, tap t' = taps-1-t
//        (Linear: the plane of q^T);
//   wq   the fp32 quantised image, written with the weight's own strides.
// The one-term entry points (qt_bf16x1_pack_levels_f32 / qt_bf16x1_pack_conv_levels_f32) write fwd with each level ONCE (2*Cin
// bytes per tap, same granules) for an activation that is itself exact in bf16 (loglin_act.hip); gx keeps three slots (g is real).
// A block owns one (tap, 64 x 64 output-channel x input-channel) tile: the quantised bf16 bits go through LDS, so both planes
// are written as whole 16-byte words along their rows (32 lanes x 16 B per row).  Reads are coalesced along Cin when Cin has unit
// stride (channels-last, Linear); for NCHW kh x kw the other taps of a cache line are read by neighbouring tiles from L2.
#include "qt_common.h"
#include "loglin_quant.h"

namespace {

__device__ __forceinline__ uint32_t level_bf16_bits(float f) {   // round-to-nearest-even, NaN kept quiet (as split_bf16.hip)
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

struct LevelQuant {   // log 0: qt_lin_quant(step = a, maxv = b, mode); log 1: qt_log_quant(lo = a, hi = b, with_sign = mode); 2: identity
    int log;
    float a, b;
    int mode;
    __device__ __forceinline__ float operator()(float x) const {
        if (log == 2) return x;
        return log ? qt_log_quant(x, a, b, mode) : qt_lin_quant(x, a, b, mode);
    }
};

constexpr int kTile = 64;
constexpr int kSlots = 32;     // 16-byte words a block may write per plane row: <= 24 of its tile + <= 7 of row padding

// 16-byte word `s` of a plane row segment that starts at local channel 0 of the tile: bf16 element u = 8 s + e belongs to local
// channel u / TERMS; channels at or beyond `valid` (the tap's pad and the row's pad) are zero.
template <bool TRANSPOSED, int TERMS>
__device__ __forceinline__ uint4 plane_word(const uint32_t (*tile)[kTile + 1], int r, int s, int valid) {
    uint32_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = (8 * s + e) / TERMS;
        h[e] = c < valid ? (TRANSPOSED ? tile[c][r] : tile[r][c]) : 0u;
    }
    return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

template <int FT>      // bf16 slots per level of the forward plane: 3 (against a triple-split activation) or 1
__global__ __launch_bounds__(256) void level_pack_kernel(const float* __restrict__ w, int64_t so, int64_t si, int64_t sh,
                                                         int64_t sw, int Cout, int Cin, int kh, int kw, LevelQuant quant,
                                                         uint16_t* __restrict__ fwd, int64_t fwd_ld, uint16_t* __restrict__ gx,
                                                         int64_t gx_ld, float* __restrict__ wq) {
    __shared__ uint32_t tile[kTile][kTile + 1];                  // [co][ci] bf16 bits of q
    const int taps = kh * kw;
    const int to_n = (Cout + kTile - 1) / kTile, ti_n = (Cin + kTile - 1) / kTile;
    const int64_t tiles = (int64_t)taps * to_n * ti_n;
    const int64_t cb_f = (2ll * FT * Cin + 15) / 16 * 16, cb_g = (6ll * Cout + 15) / 16 * 16;   // bytes per tap of each plane
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x >> 6;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int tap = (int)(t / ((int64_t)to_n * ti_n));
        const int rem = (int)(t - (int64_t)tap * to_n * ti_n);
        const int co0 = (rem / ti_n) * kTile, ci0 = (rem % ti_n) * kTile;
        const int i = tap / kw, j = tap - i * kw;
#pragma unroll 4
        for (int m = 0; m < kTile / 4; ++m) {
            const int co = co0 + ly + 4 * m, ci = ci0 + lx;
            uint32_t bits = 0;
            if (co < Cout && ci < Cin) {
                const int64_t off = co * so + ci * si + i * sh + j * sw;
                const float q = quant(w[off]);
                if (wq) wq[off] = q;
                bits = level_bf16_bits(q);
            }
            tile[ly + 4 * m][lx] = bits;
        }
        __syncthreads();
        if (fwd) {      // rows co, channels ci of tap `tap`
            const bool last_c = ci0 + kTile >= Cin;
            const int64_t start = tap * cb_f + 2ll * FT * ci0;
            const int64_t end = !last_c ? start + 2 * FT * kTile : (tap == taps - 1 ? fwd_ld : (tap + 1) * cb_f);
            const int nslots = (int)((end - start) / 16), valid = Cin - ci0 < kTile ? Cin - ci0 : kTile;
            for (int job = threadIdx.x; job < kTile * kSlots; job += blockDim.x) {
                const int r = job / kSlots, s = job - r * kSlots;
                if (co0 + r >= Cout || s >= nslots) continue;
                *reinterpret_cast<uint4*>(reinterpret_cast<char*>(fwd) + (co0 + r) * fwd_ld + start + 16 * s) =
                    plane_word<false, FT>(tile, r, s, valid);
            }
        }
        if (gx) {       // rows ci, channels co of the flipped tap taps - 1 - tap
            const int tapg = taps - 1 - tap;
            const bool last_c = co0 + kTile >= Cout;
            const int64_t start = tapg * cb_g + 6ll * co0;
            const int64_t end = !last_c ? start + 6 * kTile : (tapg == taps - 1 ? gx_ld : (tapg + 1) * cb_g);
            const int nslots = (int)((end - start) / 16), valid = Cout - co0 < kTile ? Cout - co0 : kTile;
            for (int job = threadIdx.x; job < kTile * kSlots; job += blockDim.x) {
                const int r = job / kSlots, s = job - r * kSlots;
                if (ci0 + r >= Cin || s >= nslots) continue;
                *reinterpret_cast<uint4*>(reinterpret_cast<char*>(gx) + (ci0 + r) * gx_ld + start + 16 * s) =
                    plane_word<true, 3>(tile, r, s, valid);
            }
        }
        __syncthreads();
    }
}

int64_t plane_ld(int64_t taps, int64_t chans, int terms = 3) {
    const int64_t kbytes = taps * ((2 * terms * chans + 15) / 16 * 16);
    return kbytes < 128 ? 128 : (kbytes + 127) / 128 * 128;
}

int pack_levels(int fwd_terms, const float* w, int64_t stride_o, int64_t stride_i, int64_t stride_h, int64_t stride_w, int64_t Cout,
                int64_t Cin, int64_t kh, int64_t kw, int dtype, int fsr, int bit_width, int with_sign, uint16_t* fwd,
                int64_t fwd_ld_bytes, uint16_t* gx, int64_t gx_ld_bytes, float* wq, qt_stream_t stream) {
    if (Cout <= 0 || Cin <= 0 || kh <= 0 || kw <= 0 || !w || (!fwd && !gx && !wq)) return QT_ERR_INVALID_ARG;
    if (dtype < 0 || dtype > 1 || fsr < -60 || fsr > 60 || bit_width < 1 || bit_width > (dtype ? 16 : 32)) return QT_ERR_INVALID_ARG;
    if ((fwd && fwd_ld_bytes != plane_ld(kh * kw, Cin, fwd_terms)) || (gx && gx_ld_bytes != plane_ld(kh * kw, Cout))) return QT_ERR_INVALID_ARG;
    if ((fwd && !qt_aligned16(fwd)) || (gx && !qt_aligned16(gx)) || (reinterpret_cast<uintptr_t>(wq) & 3u)) return QT_ERR_ALIGNMENT;
    if (Cout * Cin * kh * kw >= (1ll << 31) || Cout * fwd_ld_bytes >= (1ll << 40) || Cin * gx_ld_bytes >= (1ll << 40))
        return QT_ERR_UNSUPPORTED;
    LevelQuant quant;
    if (dtype == 0 && bit_width == 32) {            // LinQuant(bit_width = 32) is the identity (qt_lin_quantize_f32: OpCopy)
        quant = LevelQuant{2, 0.0f, 0.0f, 0};
    } else if (dtype == 0) {                        // the parameters of qt_lin_quantize_f32, mode 1 (with_sign) / 0
        quant = LevelQuant{0, ldexpf(1.0f, fsr - bit_width), ldexpf(1.0f, fsr), with_sign ? 1 : 0};
    } else {                                        // the parameters of qt_log_quantize_f32
        quant = LevelQuant{1, (float)fsr - (float)(1 << bit_width), (float)fsr, with_sign ? 1 : 0};
    }
    const int64_t tiles = kh * kw * ((Cout + kTile - 1) / kTile) * ((Cin + kTile - 1) / kTile);
    if (fwd_terms == 1)
        hipLaunchKernelGGL(level_pack_kernel<1>, dim3(qt_stream_grid(tiles)), dim3(256), 0, (hipStream_t)stream, w, stride_o, stride_i,
                           stride_h, stride_w, (int)Cout, (int)Cin, (int)kh, (int)kw, quant, fwd, fwd_ld_bytes, gx, gx_ld_bytes, wq);
    else
        hipLaunchKernelGGL(level_pack_kernel<3>, dim3(qt_stream_grid(tiles)), dim3(256), 0, (hipStream_t)stream, w, stride_o, stride_i,
                           stride_h, stride_w, (int)Cout, (int)Cin, (int)kh, (int)kw, quant, fwd, fwd_ld_bytes, gx, gx_ld_bytes, wq);
    return qt_check_launch();
}

}  // namespace

extern "C" {

int qt_bf16x3_pack_conv_levels_f32(const float* w, int64_t stride_o, int64_t stride_i, int64_t stride_h, int64_t stride_w,
                                   int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int dtype, int fsr, int bit_width,
                                   int with_sign, uint16_t* fwd, int64_t fwd_ld_bytes, uint16_t* gx, int64_t gx_ld_bytes,
                                   float* wq, qt_stream_t stream) {
    return pack_levels(3, w, stride_o, stride_i, stride_h, stride_w, Cout, Cin, kh, kw, dtype, fsr, bit_width, with_sign, fwd,
                       fwd_ld_bytes, gx, gx_ld_bytes, wq, stream);
}

int qt_bf16x1_pack_conv_levels_f32(const float* w, int64_t stride_o, int64_t stride_i, int64_t stride_h, int64_t stride_w,
                                   int64_t Cout, int64_t Cin, int64_t kh, int64_t kw, int dtype, int fsr, int bit_width,
                                   int with_sign, uint16_t* fwd, int64_t fwd_ld_bytes, uint16_t* gx, int64_t gx_ld_bytes,
                                   float* wq, qt_stream_t stream) {
    return pack_levels(1, w, stride_o, stride_i, stride_h, stride_w, Cout, Cin, kh, kw, dtype, fsr, bit_width, with_sign, fwd,
                       fwd_ld_bytes, gx, gx_ld_bytes, wq, stream);
}

int qt_bf16x1_pack_levels_f32(const float* w, int64_t stride_n, int64_t stride_k, int64_t N, int64_t K, int dtype, int fsr,
                              int bit_width, int with_sign, uint16_t* fwd, int64_t fwd_ld_bytes, uint16_t* gx, int64_t gx_ld_bytes,
                              float* wq, qt_stream_t stream) {
    return pack_levels(1, w, stride_n, stride_k, 0, 0, N, K, 1, 1, dtype, fsr, bit_width, with_sign, fwd, fwd_ld_bytes, gx,
                       gx_ld_bytes, wq, stream);
}

int qt_bf16x3_pack_levels_f32(const float* w, int64_t stride_n, int64_t stride_k, int64_t N, int64_t K, int dtype, int fsr,
                              int bit_width, int with_sign, uint16_t* fwd, int64_t fwd_ld_bytes, uint16_t* gx, int64_t gx_ld_bytes,
                              float* wq, qt_stream_t stream) {
    return qt_bf16x3_pack_conv_levels_f32(w, stride_n, stride_k, 0, 0, N, K, 1, 1, dtype, fsr, bit_width, with_sign, fwd,
                                          fwd_ld_bytes, gx, gx_ld_bytes, wq, stream);
}

}  // extern "C"
