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
// The deferred inference chain (lazy.py, kind "levels") keeps such planes between the layers and never writes the fp32 image:
//   qt_pool_levels_bf16          MaxPool2d(k, s) on an NHWC level plane into the next conv's halo plane;
//   qt_bn_relu_linlog_bf16_f32   BatchNorm1d (device arithmetic) -> [ReLU] -> quantiser over the fp32 result of a Linear layer, one
//                                pass that writes the next Linear layer's row plane (and, on request, the fp32 image).
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

// MaxPool2d(k, s), no padding, floor mode, on a one-term level plane: in [N][H][W][ld bytes] -> out [N][Ho + 2hy][Wo + 2hx][ld] (the
// halo border is written as zeros).  The quantisers are monotone non-decreasing, so the max of the levels is the level of the max:
// the plane of F.max_pool2d of the fp32 image.  Values are compared as floats in ATen's window order with ATen's update rule
// (val > max or val is NaN), so NaN propagates and ties between +0 and -0 resolve as they do there.  One thread = 8 channels (one
// 16-byte word) of one output pixel.
__global__ __launch_bounds__(256) void pool_levels_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, int64_t ldq, int64_t N,
                                                          int H, int W, int pk, int ps, int Ho, int Wo, int hy, int hx) {
    const int Hop = Ho + 2 * hy, Wop = Wo + 2 * hx;
    const int64_t total = N * Hop * Wop * ldq;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = i / ldq;
        const int q = (int)(i - pix * ldq);
        const int64_t n = pix / ((int64_t)Hop * Wop);
        const int rem = (int)(pix - n * Hop * Wop);
        const int ho = rem / Wop - hy, wo = rem % Wop - hx;
        uint4 o = make_uint4(0, 0, 0, 0);
        if ((unsigned)ho < (unsigned)Ho && (unsigned)wo < (unsigned)Wo) {
            const uint4* base = in + ((n * H + (int64_t)ho * ps) * W + (int64_t)wo * ps) * ldq + q;
            uint32_t best[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) best[e] = 0xff80u;                  // -inf
            for (int a = 0; a < pk; ++a)
                for (int b = 0; b < pk; ++b) {
                    const uint4 v = base[((int64_t)a * W + b) * ldq];
                    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const uint32_t h = (w4[e >> 1] >> (16 * (e & 1))) & 0xffffu;
                        const float f = __uint_as_float(h << 16), m = __uint_as_float(best[e] << 16);
                        if (f > m || f != f) best[e] = h;
                    }
                }
            o = make_uint4(best[0] | (best[1] << 16), best[2] | (best[3] << 16), best[4] | (best[5] << 16), best[6] | (best[7] << 16));
        }
        out[pix * ldq + q] = o;
    }
}

// fp32 [rows][C] (the result of a Linear layer) -> BatchNorm1d(eval) in the device's arithmetic with st = [mean | rs]: form 0
// t = fma(fl(fl(x - mean) * rs), weight, bias) (bn_eval_device_kernel's expression, what the library evaluates on 4-D tensors), form 1
// t = fma(fl(weight * fl(x - mean)), rs, bias) (the order of ATen's own row kernel); the caller's probe says which one F.batch_norm
// is on a 2-D tensor (layers.fused.device_bn_fold_rows) -> [ReLU] -> Lin / Log quantiser -> the one-term row plane [rows][ld bytes]
// (128-byte row granule, pad zero) and, when y != nullptr, the fp32 image [rows][ldy].  One thread = 8 channels: one 16-byte word
// of the plane.
__global__ __launch_bounds__(256) void bn_relu_quant_rows_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                                 const float* __restrict__ b, const float* __restrict__ st, int form,
                                                                 int relu, ActQuant quant, float* __restrict__ y, int64_t ldy,
                                                                 uint4* __restrict__ plane, int64_t ldq, int64_t rows, int C) {
    const int64_t total = rows * ldq;
    const bool vec = !(C & 3) && !(ldx & 3) && !(reinterpret_cast<uintptr_t>(x) & 15);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ldq;
        const int c0 = (int)(i - row * ldq) * 8;
        float v[8];
        if (vec && c0 + 8 <= C) {
            const float4 lo = *reinterpret_cast<const float4*>(x + row * ldx + c0), hi = *reinterpret_cast<const float4*>(x + row * ldx + c0 + 4);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = c0 + e < C ? x[row * ldx + c0 + e] : 0.0f;
        }
        uint32_t h[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            h[e] = 0u;
            const int c = c0 + e;
            if (c < C) {
                const float d = __fsub_rn(v[e], st[c]);
                float t = form ? __fmaf_rn(__fmul_rn(w[c], d), st[C + c], b[c]) : __fmaf_rn(__fmul_rn(d, st[C + c]), w[c], b[c]);
                if (relu) t = qt_torch_relu(t);
                const float q = quant(t);
                if (y) y[row * ldy + c] = q;
                h[e] = act_bf16_hi(q);
            }
        }
        plane[i] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
}

// the quantiser parameters of qt_linlog_quantize_bf16_f32's (dtype, fsr, bit_width, mode), or an error code
int make_act_quant(int dtype, int fsr, int bit_width, int mode, ActQuant& quant) {
    float a = 0.0f, b = 0.0f;
    const int rc = qt_act_level_params(dtype, fsr, bit_width, mode, a, b);
    if (rc == QT_OK) quant = ActQuant{dtype, a, b, mode};
    return rc;
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
    if (!y) return QT_ERR_INVALID_ARG;
    ActQuant quant;
    const int rc = make_act_quant(dtype, fsr, bit_width, mode, quant);
    if (rc != QT_OK) return rc;
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

int qt_pool_levels_bf16(const uint16_t* in_plane, int64_t N, int64_t H, int64_t W, int64_t ld_bytes, int64_t pool_k, int64_t pool_s,
                        uint16_t* out_plane, int64_t out_halo_h, int64_t out_halo_w, qt_stream_t stream) {
    if (N < 0 || H <= 0 || W <= 0 || ld_bytes <= 0 || pool_k < 1 || pool_s < 1 || out_halo_h < 0 || out_halo_w < 0)
        return QT_ERR_INVALID_ARG;
    if (pool_k > H || pool_k > W) return QT_ERR_INVALID_ARG;
    if (N == 0) return QT_OK;
    if (!in_plane || !out_plane) return QT_ERR_INVALID_ARG;
    if ((ld_bytes & 15) || !qt_aligned16(in_plane) || !qt_aligned16(out_plane)) return QT_ERR_ALIGNMENT;
    if (H > 32767 || W > 32767 || out_halo_h > 64 || out_halo_w > 64) return QT_ERR_UNSUPPORTED;
    const int64_t Ho = (H - pool_k) / pool_s + 1, Wo = (W - pool_k) / pool_s + 1;  // floor mode, no padding
    const int64_t ldq = ld_bytes / 16;
    const int grid = qt_stream_grid((N * (Ho + 2 * out_halo_h) * (Wo + 2 * out_halo_w) * ldq + 255) / 256);
    hipLaunchKernelGGL(pool_levels_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint4*>(in_plane),
                       reinterpret_cast<uint4*>(out_plane), ldq, N, (int)H, (int)W, (int)pool_k, (int)pool_s, (int)Ho, (int)Wo,
                       (int)out_halo_h, (int)out_halo_w);
    return qt_check_launch();
}

int qt_bn_relu_linlog_bf16_f32(const float* x, int64_t ldx, const float* weight, const float* bias, const float* bn_stats, int bn_form,
                               int relu, int dtype, int fsr, int bit_width, int mode, float* y, int64_t ldy, uint16_t* plane,
                               int64_t ld_bytes, int64_t rows, int64_t C, qt_stream_t stream) {
    if (rows < 0 || C <= 0 || relu < 0 || relu > 1 || bn_form < 0 || bn_form > 1 || ldx < C || (y && ldy < C)) return QT_ERR_INVALID_ARG;
    ActQuant quant;
    const int rc = make_act_quant(dtype, fsr, bit_width, mode, quant);
    if (rc != QT_OK) return rc;
    if (rows == 0) return QT_OK;
    if (!x || !weight || !bias || !bn_stats || !plane) return QT_ERR_INVALID_ARG;
    if ((ld_bytes & 15) || ld_bytes < 2 * C || !qt_aligned16(plane)) return QT_ERR_ALIGNMENT;
    if (C >= (1ll << 28) || rows * ld_bytes >= (1ll << 40)) return QT_ERR_UNSUPPORTED;
    const int64_t ldq = ld_bytes / 16;
    const int grid = qt_stream_grid((rows * ldq + 255) / 256);
    hipLaunchKernelGGL(bn_relu_quant_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, ldx, weight, bias, bn_stats, bn_form,
                       relu, quant, y, ldy, reinterpret_cast<uint4*>(plane), ldq, rows, (int)C);
    return qt_check_launch();
}

}  // extern "C"
