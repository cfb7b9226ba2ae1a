// Per-element Lin / Log fixed-point quantisers of "Convolutional Neural Networks using Logarithmic Data Representation"
// (functions/log_lin_connect.py).  One copy for every kernel that applies them: qt_lin_quantize_f32 / qt_log_quantize_f32
// (elementwise.hip) and the quantise-and-pack of Lin / Log weights (loglin_pack.hip), so both produce the same bits.
#pragma once
#include "qt_common.h"

// torch.sign = (0 < x) - (x < 0): sign(+-0) = +0, sign(NaN) = NaN
__device__ __forceinline__ float qt_torch_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : (x != x ? x : 0.0f)); }
__device__ __forceinline__ float qt_torch_clamp(float v, float lo, float hi) {   // torch.clamp propagates NaN
    return v != v ? v : (v < lo ? lo : (v > hi ? hi : v));   // compare chain: clamp(-0, 0, hi) stays -0, like ATen
}

// log_lin_connect.py:61-67, step = 2^(fsr - bit_width), maxv = 2^fsr.  mode 0: clamp(round(x/step)*step, 0, 2^fsr); mode 1:
// sign(x) * the same of |x|; mode 2: sign(g) * clamp(round(g/step)*step, 0, 2^fsr) (the quantised-gradient backward, :79 —
// negative g clamps to 0, so it yields -0: reproduced)
__device__ __forceinline__ float qt_lin_quant(float x, float step, float maxv, int mode) {
    const float a = mode == 1 ? fabsf(x) : x;
    const float q = qt_torch_clamp(rintf(a / step) * step, 0.0f, maxv);
    return mode == 0 ? q : qt_torch_sign(x) * q;
}

// log_lin_connect.py:31-33: [sign(x) *] 2^clamp(round(log2|x|), lo, hi) with lo = fsr - 2^bits, hi = fsr.  with_sign 2: AP2's
// safeSign instead of torch.sign
__device__ __forceinline__ float qt_log_quant(float x, float lo, float hi, int with_sign) {
    const float e = qt_torch_clamp(rintf(log2f(fabsf(x))), lo, hi);   // x = 0: -inf -> lo
    const float p = exp2f(e);                                        // integer e: exact (0 below 2^-149)
    return with_sign == 2 ? qt_safe_sign(x) * p : (with_sign ? qt_torch_sign(x) * p : p);
}
