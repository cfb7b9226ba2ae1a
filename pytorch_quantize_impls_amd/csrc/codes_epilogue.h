// The code epilogue of the DoReFa inference chain, shared by the elementwise pass (codes_i8.hip) and the depthwise and grouped convs
// on code planes (dwconv.hip, gconv.hip): per-channel constants of one output dword and the arithmetic that turns four fp32 values
// into four int8 codes.
#pragma once
#include "qt_common.h"

namespace {

// Inference fusion of the DoReFa activation chain (k-bit form):
//   conv / linear output x -> eval BatchNorm folded to t = fl(fl(x*alpha[c]) + beta[c])
//     [+ residual: fl(fl(r*ralpha[c]) + rbeta[c]) of an fp32 tensor (a shortcut conv before ITS BatchNorm), or
//        fl(rscale * code) of an int8 code plane (identity shortcut that carries DoReFa codes)]
//     [-> ReLU] -> nnDorefaQuant(k): q = rint(n * t)   (functions/dorefa_connect.py:24-25, unclamped)
// written as the next layer's int8 code plane (and, on request, the fp32 image fl(fl(1/n) * q)).
// One thread = 4 consecutive channels; per element 4 B in (+ 4 B or 1 B residual), 1 B out: HBM-bound.
// Per-channel constants of one thread's 4 channels (loaded once per thread on the fixed-slot path).
struct AffineConsts {
    float al[4], be[4], mean[4], rs[4], ral[4], rbe[4], rmean[4], rrs[4];
};

__device__ __forceinline__ void affine_load_consts(AffineConsts& c, int64_t k0, int64_t C, const float* __restrict__ alpha,
                                                   const float* __restrict__ beta, const float* __restrict__ ralpha,
                                                   const float* __restrict__ rbeta, const float* __restrict__ bn_stats,
                                                   const float* __restrict__ rbn_stats) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool in = k0 + e < C;
        c.al[e] = in ? alpha[k0 + e] : 0.0f;
        c.be[e] = in ? beta[k0 + e] : 0.0f;
        c.mean[e] = (in && bn_stats) ? bn_stats[k0 + e] : 0.0f;
        c.rs[e] = (in && bn_stats) ? bn_stats[C + k0 + e] : 1.0f;
        c.ral[e] = (in && ralpha) ? ralpha[k0 + e] : 1.0f;
        c.rbe[e] = (in && ralpha) ? rbeta[k0 + e] : 0.0f;
        c.rmean[e] = (in && rbn_stats) ? rbn_stats[k0 + e] : 0.0f;
        c.rrs[e] = (in && rbn_stats) ? rbn_stats[C + k0 + e] : 1.0f;
    }
}

// one output dword (4 channels of one row): the arithmetic of the header comment, every rounding spelled out
__device__ __forceinline__ uint32_t affine_codes_word(const float (&v)[4], const float (&r)[4], uint32_t rword, const AffineConsts& c,
                                                      int nvalid, bool devbn, bool has_rf, bool has_ralpha, bool rdevbn, bool has_rc,
                                                      float rscale, int relu, float n, float (&q4)[4], int& bad) {
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int q = 0;
        q4[e] = 0.0f;
        if (e < nvalid) {
            const float x0 = (relu == 2 && v[e] < 0.0f) ? 0.0f : v[e];          // ReLU in front of the BatchNorm
            // folded form: fl(fl(x * alpha) + beta).  Device form (bn_stats = [mean | rs], alpha = weight, beta = bias):
            // fma(fl(fl(x - mean) * rs), weight, bias) — the expression this device's eval-mode F.batch_norm evaluates
            float t = devbn ? __fmaf_rn(__fmul_rn(__fsub_rn(x0, c.mean[e]), c.rs[e]), c.al[e], c.be[e])
                            : __fadd_rn(__fmul_rn(x0, c.al[e]), c.be[e]);
            if (has_rf) {
                float u = r[e];
                if (has_ralpha)
                    u = rdevbn ? __fmaf_rn(__fmul_rn(__fsub_rn(u, c.rmean[e]), c.rrs[e]), c.ral[e], c.rbe[e])
                               : __fadd_rn(__fmul_rn(u, c.ral[e]), c.rbe[e]);
                t = __fadd_rn(t, u);
            }
            if (has_rc) t = __fadd_rn(t, __fmul_rn(rscale, (float)(int8_t)(rword >> (8 * e))));
            if (relu == 1) t = t < 0.0f ? 0.0f : t;             // NaN stays NaN (flagged below)
            const float q_ = rintf(__fmul_rn(n, t));
            q4[e] = q_;
            if (!(q_ >= -127.0f && q_ <= 127.0f)) { bad |= (q_ >= -2047.0f && q_ <= 2047.0f) ? 1 : 3; q = 0; } else q = (int)q_;
        }
        word |= (uint32_t)(uint8_t)(int8_t)q << (8 * e);
    }
    return word;
}

}  // namespace
