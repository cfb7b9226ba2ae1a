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

// A plane element of a one-term bf16 level plane (loglin_act.hip, the level epilogue of the implicit conv): the high half of the
// fp32 pattern; a NaN whose payload sits in the low half only would become an infinity: made quiet instead
__device__ __forceinline__ uint32_t act_bf16_hi(float f) {
    const uint32_t u = __float_as_uint(f);
    uint32_t h = u >> 16;
    if ((u & 0x7fffffffu) > 0x7f800000u && !(h & 0x7fu)) h |= 0x40u;
    return h;
}

// torch.relu on the device: clamp_min(x, 0) = NaN stays NaN, else the device's own max (relu(-0) is what v_max_f32 makes of it)
__device__ __forceinline__ float qt_torch_relu(float x) { return x != x ? x : fmaxf(x, 0.0f); }

// Host side: the two parameters (Lin: step, maxv; Log: lo, hi) of an activation quantiser (dtype 0 = lin, 1 = log) whose levels are
// single bf16 terms, or an error code.  One copy for qt_linlog_quantize_bf16_f32, the rows pass and the conv's level epilogue: the
// three produce the same bits only from the same parameters
inline int qt_act_level_params(int dtype, int fsr, int bit_width, int mode, float& a, float& b) {
    if (dtype < 0 || dtype > 1 || mode < 0 || mode > 1 || fsr < -60 || fsr > 60 || bit_width < 1) return QT_ERR_INVALID_ARG;
    if (dtype == 0) {            // the parameters of qt_lin_quantize_f32; more than 8 bits are not one bf16 term
        if (bit_width > 8) return QT_ERR_UNSUPPORTED;
        a = ldexpf(1.0f, fsr - bit_width);
        b = ldexpf(1.0f, fsr);
    } else {                     // the parameters of qt_log_quantize_f32; levels below 2^-126 would be bf16 denormals
        if (bit_width > 16 || fsr - (1 << bit_width) < -126) return QT_ERR_UNSUPPORTED;
        a = (float)fsr - (float)(1 << bit_width);
        b = (float)fsr;
    }
    return QT_OK;
}
