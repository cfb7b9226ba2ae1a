// Lin / Log quantised ACTIVATIONS as one-term bf16 operands (functions/log_lin_connect.py nnQuant -> layers/log_lin_layers.py).
// A Lin level m * 2^(fsr - bit_width) (m <= 2^bit_width, bit_width <= 8) or a Log level +-2^e (e >= -126) has at most 8
// significant bits: its bf16 image is the value itself, the high half of its fp32 pattern.  The layer that consumes such an
// activation contracts ONE bf16 term per element instead of the three of the exact split of a real number (split_bf16.hip).
//   qt_linlog_quantize_bf16_f32  the quantiser of qt_lin_quantize_f32 / qt_log_quantize_f32 (loglin_quant.h: the same device
//                                functions, the same bits) writing the fp32 image in the input's own layout AND the one-term plane
//                                [pixel][channel] the consumer reads, in one pass;
//   qt_bf16_pack_check_f32       the same plane of an fp32 tensor that is only BELIEVED to hold such values, OR-ing a device flag
//                                when an element is not exact;
//   qt_check_bf16_exact_f32      the predicate alone.
// One kernel serves every layout: a block owns a 64 pixel x 64 channel tile, reads it along whichever of the two has unit stride
// (rows / channels-last: channels; NCHW: pixels), passes the bf16 bits through LDS and writes whole 16-byte words along the
// plane rows.  Pad bytes of a row (channel granule, 128-byte row granule of GEMM operands) are written as zeros by the tile that
// holds the row's last channels.
#include "qt_common.h"
#include "loglin_quant.h"

namespace {

struct ActQuant {   // kind 0: qt_lin_quant(step = a, maxv = b, mode); 1: qt_log_quant(lo = a, hi = b, with_sign = mode); 2: identity
    int kind;
    float a, b;
    int mode;
    __device__ __forceinline__ float operator()(float x) const {
        if (kind == 2) return x;
        return kind ? qt_log_quant(x, a, b, mode) : qt_lin_quant(x, a, b, mode);
    }
};

// high half of the fp32 pattern; a NaN whose payload sits in the low half only would become an infinity: made quiet instead
__device__ __forceinline__ uint32_t act_bf16_hi(float f) {
    const uint32_t u = __float_as_uint(f);
    uint32_t h = u >> 16;
    if ((u & 0x7fffffffu) > 0x7f800000u && !(h & 0x7fu)) h |= 0x40u;
    return h;
}

// finite, low 16 bits zero, and zero or a NORMAL number (bf16 denormals on the matrix cores are not relied on)
__device__ __forceinline__ bool act_bf16_exact(float f) {
    const uint32_t u = __float_as_uint(f);
    const uint32_t e = (u >> 23) & 0xffu;
    return !(u & 0xffffu) && e != 0xffu && (e != 0u || !(u & 0x7fffffffu));
}

constexpr int kTile = 64;

template <bool CH_FAST>
__global__ __launch_bounds__(256) void act_plane_kernel(const float* __restrict__ x, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                                                        int64_t P, int C, int HW, int W, ActQuant quant, float* __restrict__ y,
                                                        uint16_t* __restrict__ plane, int64_t ld, int32_t* __restrict__ flag) {
    __shared__ uint32_t tile[kTile][kTile + 1];                   // [channel][pixel] bf16 bits
    const int tc_n = (C + kTile - 1) / kTile;
    const int64_t tiles = (P + kTile - 1) / kTile * tc_n;
    const int lx = threadIdx.x & (kTile - 1), ly = threadIdx.x >> 6;
    bool bad = false;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ct = (int)(t % tc_n);
        const int64_t p0 = (t / tc_n) * kTile;
        const int c0 = ct * kTile;
#pragma unroll 4
        for (int m = 0; m < kTile / 4; ++m) {
            const int cl = CH_FAST ? lx : ly + 4 * m, pl = CH_FAST ? ly + 4 * m : lx;
            const int c = c0 + cl;
            const int64_t p = p0 + pl;
            uint32_t bits = 0;
            if (c < C && p < P) {
                const int64_t n = p / HW;
                const int r = (int)(p - n * HW);
                const int h = r / W, w = r - h * W;
                const int64_t off = n * sn + c * sc + h * sh + w * sw;
                const float q = quant(x[off]);
                if (y) y[off] = q;
                bad |= !act_bf16_exact(q);
                bits = act_bf16_hi(q);
            }
            tile[cl][pl] = bits;
        }
        __syncthreads();
        // plane row p: bytes [128 ct, 128 ct + 16 nslots) — the tile's channels, and the row's pad when it holds the last ones
        const int64_t row_end = ct == tc_n - 1 ? ld : 128ll * (ct + 1);
        const int nslots = (int)((row_end - 128ll * ct) / 16), valid = C - c0 < kTile ? C - c0 : kTile;
        for (int job = threadIdx.x; job < kTile * 8; job += blockDim.x) {
            const int pl = job >> 3, s = job & 7;
            if (p0 + pl >= P || s >= nslots) continue;
            uint32_t h[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = 8 * s + e < valid ? tile[8 * s + e][pl] : 0u;
            *reinterpret_cast<uint4*>(reinterpret_cast<char*>(plane) + (p0 + pl) * ld + 128ll * ct + 16 * s) =
                make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        }
        __syncthreads();
    }
    if (flag && __any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void check_exact_kernel(const float* __restrict__ x, int64_t n, int32_t* __restrict__ flag) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        bad |= !act_bf16_exact(x[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

int launch_act_plane(const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int64_t N, int64_t C, int64_t H, int64_t W,
                     ActQuant quant, float* y, uint16_t* plane, int64_t ld, int32_t* flag, qt_stream_t stream) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || !x || !plane) return QT_ERR_INVALID_ARG;
    const int64_t tc_n = (C + kTile - 1) / kTile;
    // a row holds its 2 C bytes and at most the pad of the tile with its last channels (16- and 128-byte granules both do)
    if ((ld & 15) || ld < 2 * C || ld > 128 * tc_n) return QT_ERR_INVALID_ARG;
    if (!qt_aligned16(plane) || (reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(y) & 3u)) return QT_ERR_ALIGNMENT;
    const int64_t P = N * H * W;
    if (P >= (1ll << 31) || C >= (1ll << 24) || P * ld >= (1ll << 40)) return QT_ERR_UNSUPPORTED;
    const int grid = qt_stream_grid((P + kTile - 1) / kTile * tc_n);
    if (sc == 1 || C == 1)
        hipLaunchKernelGGL(act_plane_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, sn, sc, sh, sw, P, (int)C,
                           (int)(H * W), (int)W, quant, y, plane, ld, flag);
    else
        hipLaunchKernelGGL(act_plane_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, sn, sc, sh, sw, P, (int)C,
                           (int)(H * W), (int)W, quant, y, plane, ld, flag);
    return qt_check_launch();
}

}  // namespace

extern "C" {

int qt_linlog_quantize_bf16_f32(const float* x, int64_t stride_n, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t N,
                                int64_t C, int64_t H, int64_t W, int dtype, int fsr, int bit_width, int mode, float* y,
                                uint16_t* plane, int64_t ld_bytes, qt_stream_t stream) {
    if (!y || dtype < 0 || dtype > 1 || mode < 0 || mode > 1 || fsr < -60 || fsr > 60 || bit_width < 1) return QT_ERR_INVALID_ARG;
    ActQuant quant;
    if (dtype == 0) {            // the parameters of qt_lin_quantize_f32; more than 8 bits are not one bf16 term
        if (bit_width > 8) return QT_ERR_UNSUPPORTED;
        quant = ActQuant{0, ldexpf(1.0f, fsr - bit_width), ldexpf(1.0f, fsr), mode};
    } else {                     // the parameters of qt_log_quantize_f32; levels below 2^-126 would be bf16 denormals
        if (bit_width > 16 || fsr - (1 << bit_width) < -126) return QT_ERR_UNSUPPORTED;
        quant = ActQuant{1, (float)fsr - (float)(1 << bit_width), (float)fsr, mode};
    }
    return launch_act_plane(x, stride_n, stride_c, stride_h, stride_w, N, C, H, W, quant, y, plane, ld_bytes, nullptr, stream);
}

int qt_bf16_pack_check_f32(const float* x, int64_t stride_n, int64_t stride_c, int64_t stride_h, int64_t stride_w, int64_t N,
                           int64_t C, int64_t H, int64_t W, uint16_t* plane, int64_t ld_bytes, int32_t* flag, qt_stream_t stream) {
    if (!flag) return QT_ERR_INVALID_ARG;
    return launch_act_plane(x, stride_n, stride_c, stride_h, stride_w, N, C, H, W, ActQuant{2, 0.0f, 0.0f, 0}, nullptr, plane,
                            ld_bytes, flag, stream);
}

int qt_check_bf16_exact_f32(const float* x, int64_t n, int32_t* flag, qt_stream_t stream) {
    if (n < 0 || !flag || (n > 0 && !x)) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    hipLaunchKernelGGL(check_exact_kernel, dim3(qt_stream_grid((n + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream, x, n, flag);
    return qt_check_launch();
}

}  // extern "C"
