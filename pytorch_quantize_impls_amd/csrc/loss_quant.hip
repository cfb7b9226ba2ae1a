// Loss-aware quantisation families (Elastic / WQR, functions/elastic_quant_connect.py, functions/WQR_connect.py):
// the projection of a weight onto its level set and the fused "sawtooth" regulariser of its gradient.  Both are one
// streaming pass (16-byte loads / stores, grid-stride); the level set and the regulariser's term table travel BY VALUE
// in the kernel arguments, so a launch allocates nothing, never syncs and can be captured in a graph.
//
// Bit-exactness: every quantity is formed in the order the reference's torch expressions form it, in fp32, without
// contraction (the Makefile's -ffp-contract=off).  See DESIGN.md "Loss-aware quantisation".
#include "qt_common.h"

namespace {

struct LevelTable {
    float v[QT_LEVELS_MAX];
    int n;
};

struct RegTable {
    qt_reg_term t[QT_REG_TERMS_MAX];
    int n1, n2;
};

// _proj_val: set[argmin_j |x - set[j]|] — ties to the first index, a NaN distance wins (torch.argmin), so NaN / +-inf
// inputs give set[0]; the result is the table entry itself (signed zeros from the table).
__device__ __forceinline__ float project_one(float x, const LevelTable& L) {
    float best = fabsf(x - L.v[0]);
    float val = L.v[0];
    for (int j = 1; j < L.n; ++j) {
        const float d = fabsf(x - L.v[j]);
        if (best == best && (d < best || d != d)) {
            best = d;
            val = L.v[j];
        }
    }
    return val;
}

__global__ __launch_bounds__(256) void level_project_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int vec,
                                                            const LevelTable L) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const int64_t n4 = vec ? n / 4 : 0;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* y4 = reinterpret_cast<float4*>(y);
    for (int64_t i = tid; i < n4; i += nthreads) {
        const float4 v = x4[i];
        float4 r;
        r.x = project_one(v.x, L); r.y = project_one(v.y, L); r.z = project_one(v.z, L); r.w = project_one(v.w, L);
        y4[i] = r;
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += nthreads) y[i] = project_one(x[i], L);
}

// torch.sign: +1 / -1 / +0 for +-0 / NaN for NaN
__device__ __forceinline__ float tsign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : (x != x ? x : 0.0f)); }

__device__ __forceinline__ bool cmp(int op, float x, float t) {
    switch (op) {
        case QT_CMP_LT: return x < t;
        case QT_CMP_LE: return x <= t;
        case QT_CMP_GT: return x > t;
        default: return x >= t;
    }
}

// One table entry applied to one element: res +-= ((V(x) * m1) * m2), V of the entry's kind.  `a` is the family's
// coefficient (alpha / beta / kapa), `k` the entry's constant (QT_REG_L2_LIN: the additive term, already c * a).
__device__ __forceinline__ float term_value(int kind, float x, float a, float c, float k) {
    switch (kind) {
        case QT_REG_L2_LIN: return a * x + k;                                   // alpha*x + (-c)*alpha
        case QT_REG_L2_EXP: return a * (x - c);                                 // alpha*(x - c)
        case QT_REG_L1: return a;                                               // beta
        case QT_REG_WQR_LIN: return a * (tsign(x) * fabsf(x - c) + fabsf(x) * tsign(x - c));
        case QT_REG_WQR_EXP_POS: return a * (tsign(x) * fabsf(x - c) + fabsf(x));
        default: return a * (tsign(x) * fabsf(x - c) - fabsf(x));               // QT_REG_WQR_EXP_NEG: + -1*|x|
    }
}

__device__ __forceinline__ void apply_terms(const qt_reg_term* T, int lo, int hi, float a, bool a_dev, float r[4], const float x[4]) {
    for (int e = lo; e < hi; ++e) {
        const int code = T[e].code;
        const int kind = code & 15, op1 = (code >> 4) & 3, op2 = (code >> 6) & 3;
        const bool neg = (code >> 8) & 1;
        const float c = T[e].c;
        // lin_l2's additive constant: a Python coefficient gives the double product (-c)*alpha rounded once (host, in c);
        // a tensor coefficient gives fl(fl(-c) * alpha) (c holds fl(-c))
        const float k = a_dev ? c * a : c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = term_value(kind, x[q], a, c, k);
            v = v * (cmp(op1, x[q], T[e].t1) ? 1.0f : 0.0f);
            v = v * (cmp(op2, x[q], T[e].t2) ? 1.0f : 0.0f);
            r[q] = neg ? r[q] - v : r[q] + v;
        }
    }
}

__global__ __launch_bounds__(256) void weight_reg_kernel(const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ out,
                                                         int64_t n, int vec, const RegTable T, float a1v, const float* __restrict__ a1p,
                                                         float a2v, const float* __restrict__ a2p) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const float a1 = a1p ? *a1p : a1v;
    const float a2 = a2p ? *a2p : a2v;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t i = tid; i < n4; i += nthreads) {
        const float4 wv = reinterpret_cast<const float4*>(w)[i];
        const float x[4] = {wv.x, wv.y, wv.z, wv.w};
        float r1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, r2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        apply_terms(T.t, 0, T.n1, a1, a1p != nullptr, r1, x);
        float4 o;
        if (g) {
            apply_terms(T.t, T.n1, T.n1 + T.n2, a2, a2p != nullptr, r2, x);
            const float4 gv = reinterpret_cast<const float4*>(g)[i];
            o.x = (gv.x - r1[0]) - r2[0]; o.y = (gv.y - r1[1]) - r2[1];
            o.z = (gv.z - r1[2]) - r2[2]; o.w = (gv.w - r1[3]) - r2[3];
        } else {
            o.x = r1[0]; o.y = r1[1]; o.z = r1[2]; o.w = r1[3];
        }
        reinterpret_cast<float4*>(out)[i] = o;
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += nthreads) {
        const float x[4] = {w[i], 0.0f, 0.0f, 0.0f};      // lanes 1..3 unused
        float r1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, r2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        apply_terms(T.t, 0, T.n1, a1, a1p != nullptr, r1, x);
        if (g) {
            apply_terms(T.t, T.n1, T.n1 + T.n2, a2, a2p != nullptr, r2, x);
            out[i] = (g[i] - r1[0]) - r2[0];
        } else {
            out[i] = r1[0];
        }
    }
}

}  // namespace

extern "C" {

int qt_level_project_f32(const float* x, float* y, int64_t n, const float* levels, int n_levels, qt_stream_t stream) {
    if (n < 0 || !levels || n_levels < 1 || n_levels > QT_LEVELS_MAX || (n > 0 && (!x || !y))) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    LevelTable L;
    for (int j = 0; j < QT_LEVELS_MAX; ++j) L.v[j] = j < n_levels ? levels[j] : 0.0f;
    L.n = n_levels;
    const int vec = qt_aligned16(x) && qt_aligned16(y);
    hipLaunchKernelGGL(level_project_kernel, dim3(qt_stream_grid((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, x, y, n, vec, L);
    return qt_check_launch();
}

int qt_weight_reg_f32(const float* w, const float* g, float* out, int64_t n, const qt_reg_term* terms, int n_terms1, int n_terms2,
                      float coef1, const float* coef1_dev, float coef2, const float* coef2_dev, qt_stream_t stream) {
    if (n < 0 || n_terms1 < 0 || n_terms2 < 0 || n_terms1 + n_terms2 > QT_REG_TERMS_MAX) return QT_ERR_INVALID_ARG;
    if ((n_terms1 + n_terms2 > 0 && !terms) || (!g && n_terms2 > 0) || (n > 0 && (!w || !out))) return QT_ERR_INVALID_ARG;
    for (int e = 0; e < n_terms1 + n_terms2; ++e) {
        const int code = terms[e].code;
        if ((code & 15) > QT_REG_WQR_EXP_NEG || (code >> 9) != 0) return QT_ERR_INVALID_ARG;
    }
    if (n == 0) return QT_OK;
    RegTable T;
    for (int e = 0; e < QT_REG_TERMS_MAX; ++e) T.t[e] = e < n_terms1 + n_terms2 ? terms[e] : qt_reg_term{0, 0.0f, 0.0f, 0.0f};
    T.n1 = n_terms1;
    T.n2 = n_terms2;
    const int vec = qt_aligned16(w) && qt_aligned16(out) && (!g || qt_aligned16(g));
    hipLaunchKernelGGL(weight_reg_kernel, dim3(qt_stream_grid((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, w, g, out, n, vec, T,
                       coef1, coef1_dev, coef2, coef2_dev);
    return qt_check_launch();
}

}  // extern "C"
