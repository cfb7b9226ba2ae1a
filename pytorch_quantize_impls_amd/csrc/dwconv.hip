// Depthwise conv2d (groups == in_channels, out_channels = m * in_channels) in fp32: forward, grad_input, grad_weight — and the
// forward on / into the bit planes of the fused sign chain and the int8 code planes of the fused DoReFa chain (second half of
// the file).  include/qt_hip.h "Depthwise convolution" states the contract; DESIGN.md "Depthwise convs" the layout and the byte counts.
//
// These are streaming kernels: K = kh * kw <= 49 is no matrix-core shape.  One thread owns ONE channel for the whole launch and
// keeps that channel's quantised taps in registers (the quantisers are the shared device helpers of qt_common.h); it then walks
// the outputs of its channel that the thread map hands it.  Two thread maps, chosen by the layout of the tensor that is written:
//   NCHW          : tid -> (channel slot, row of the tile, column of the tile), TW x TH x slots = 256, all powers of two.  Lanes
//                   run along W.  A large plane gives slots = 1 (a workgroup owns 4-row strips of one (n, channel) plane, its taps
//                   come from wave-uniform addresses); a 14 x 14 or 7 x 7 plane gives a 16 x 16 or 8 x 8 tile and 1 or 4 channel
//                   slots per workgroup, so the waves stay populated.
//   channels-last : tid -> (pixel slot, channel lane), lanes run along C (up to 64), 256 / lanes pixels per step.
// A workgroup is (channel group, split): it walks units split, split + S, ... of its channels, so the grid is one-dimensional and
// bounded by the plan, never by N * C * m.  The row re-reads of neighbouring taps are left to L1 / L2 (no LDS staging).
//
// Arithmetic: one fp32 multiply and one fp32 add per tap (the build has -ffp-contract=off), the accumulator starts at +0, taps in
// row-major order, taps outside the image skipped, bias last.  grad_weight: per-thread partial sums in walk order, a butterfly over
// the lanes that share a channel, the waves in index order, one partial per (split, channel, tap) in the workspace; a second launch
// adds the splits in index order.  No atomics anywhere: equal inputs give equal bits.
#include "qt_common.h"
#include "dw_map.h"
#include "dw_planes.h"
#include "codes_epilogue.h"

namespace {

constexpr int DW_MAX_TAPS = QT_DW_MAX_TAPS;
constexpr int64_t DW_MAX_ELEMS = (int64_t)1 << 31;
constexpr int64_t DW_MAX_CHANNELS = QT_DW_MAX_CHANNELS;      // bounds the one-dimensional grid: channel groups + the split target

// KH == 0: any kernel of up to 49 taps, tap coordinates divided out at run time; else the compile-time kernel
template <int KH, int KW>
struct DwTaps {
    static constexpr bool GEN = KH == 0;
    static constexpr int CAP = GEN ? DW_MAX_TAPS : KH * KW;
    __device__ __forceinline__ static int kw(const DwGeom& g) { return GEN ? g.kw : KW; }
    __device__ __forceinline__ static int kk(const DwGeom& g) { return GEN ? g.kh * g.kw : KH * KW; }
};

// XT: element type of x and y, WT: of w (dw_map.h: float, DwBf16, DwF16); the accumulator and the bias are fp32 for all of them
template <int KH, int KW, typename XT = float, typename WT = float>
__global__ __launch_bounds__(DW_THREADS) void dw_forward_kernel(const XT* __restrict__ x, const WT* __restrict__ w,
                                                                const float* __restrict__ bias, XT* __restrict__ y, DwGeom g,
                                                                DwStrides xs, DwStrides ys, DwMap mp, int kind) {
    using T = DwTaps<KH, KW>;
    const int tid = threadIdx.x;
    const int64_t cg = blockIdx.x / mp.splits;
    const int split = (int)(blockIdx.x - cg * mp.splits);
    const int64_t co = cg * mp.slots + dw_slot(mp, tid);
    if (co >= g.Cout) return;
    const int kw = T::kw(g), kk = T::kk(g);
    float wq[T::CAP];
#pragma unroll
    for (int t = 0; t < T::CAP; ++t) wq[t] = t < kk ? dw_quant(kind, dw_ld(w[co * kk + t])) : 0.0f;
    const float b = bias ? bias[co] : 0.0f;
    const int64_t c = co / g.m;
    for (int u = split; u < mp.units; u += mp.splits) {
        int n, ho, wo;
        if (!dw_pos(mp, u, tid, n, ho, wo)) continue;
        const XT* xp = x + n * xs.n + c * xs.c;
        const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
        float acc = 0.0f;
#pragma unroll
        for (int t = 0; t < T::CAP; ++t) {
            if (!T::GEN || t < kk) {
                const int i = t / kw, j = t - i * kw;
                const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                if (hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) acc = acc + dw_ld(xp[hi * xs.h + wi * xs.w]) * wq[t];
            }
        }
        if (bias) acc = acc + b;
        dw_st(&y[n * ys.n + co * ys.c + ho * ys.h + wo * ys.w], acc);
    }
}

// gather form: gx[n, c, h, w] = sum over j < m, taps (i, j') of go[n, c m + j, ho, wo] Q(w)[c m + j, i, j'] where
// ho sh = h + ph - i dh and wo sw = w + pw - j' dw have a solution inside the output
template <int KH, int KW, typename XT = float, typename WT = float>
__global__ __launch_bounds__(DW_THREADS) void dw_grad_input_kernel(const XT* __restrict__ go, const WT* __restrict__ w,
                                                                   XT* __restrict__ gx, DwGeom g, DwStrides gs, DwStrides xs,
                                                                   DwMap mp, int kind) {
    using T = DwTaps<KH, KW>;
    const int tid = threadIdx.x;
    const int64_t cg = blockIdx.x / mp.splits;
    const int split = (int)(blockIdx.x - cg * mp.splits);
    const int64_t c = cg * mp.slots + dw_slot(mp, tid);
    if (c >= g.C) return;
    const int kw = T::kw(g), kk = T::kk(g);
    const bool one = g.m == 1;            // the taps of the only output channel stay in registers
    float wq[T::CAP];
#pragma unroll
    for (int t = 0; t < T::CAP; ++t) wq[t] = (one && t < kk) ? dw_quant(kind, dw_ld(w[c * kk + t])) : 0.0f;
    for (int u = split; u < mp.units; u += mp.splits) {
        int n, h, x0;
        if (!dw_pos(mp, u, tid, n, h, x0)) continue;
        float acc = 0.0f;
        for (int j = 0; j < g.m; ++j) {
            const int64_t co = c * g.m + j;
            const XT* gp = go + n * gs.n + co * gs.c;
            const WT* wp = w + co * kk;
#pragma unroll
            for (int t = 0; t < T::CAP; ++t) {
                if (!T::GEN || t < kk) {
                    const int i = t / kw, jj = t - i * kw;
                    const int hh = h + g.ph - i * g.dh, ww = x0 + g.pw - jj * g.dw;
                    if (hh >= 0 && ww >= 0) {
                        const int ho = hh / g.sh, wo = ww / g.sw;
                        if (ho * g.sh == hh && wo * g.sw == ww && ho < g.Ho && wo < g.Wo) {
                            const float q = one ? wq[t] : dw_quant(kind, dw_ld(wp[t]));
                            acc = acc + dw_ld(gp[ho * gs.h + wo * gs.w]) * q;
                        }
                    }
                }
            }
        }
        dw_st(&gx[n * xs.n + c * xs.c + h * xs.h + x0 * xs.w], acc);
    }
}

// stage 1 of grad_weight: work[(split * Cout + co) * (kk + 1) + t] = this workgroup's share of sum go * x for tap t, and of
// sum go for t == kk
// (two type parameters like its siblings, so that one dispatch macro serves all three; go and x share XT)
template <int KH, int KW, typename XT = float, typename = XT>
__global__ __launch_bounds__(DW_THREADS) void dw_grad_weight_kernel(const XT* __restrict__ go, const XT* __restrict__ x,
                                                                    float* __restrict__ work, DwGeom g, DwStrides gs, DwStrides xs,
                                                                    DwMap mp) {
    using T = DwTaps<KH, KW>;
    constexpr int CAP = T::CAP;
    __shared__ float red[(CAP + 1) * DW_THREADS];
    const int tid = threadIdx.x;
    const int64_t cg = blockIdx.x / mp.splits;
    const int split = (int)(blockIdx.x - cg * mp.splits);
    const int64_t co = cg * mp.slots + dw_slot(mp, tid);
    const bool live = co < g.Cout;
    const int kw = T::kw(g), kk = T::kk(g);
    const int64_t c = live ? co / g.m : 0;
    float acc[CAP + 1];
#pragma unroll
    for (int t = 0; t <= CAP; ++t) acc[t] = 0.0f;
    if (live) {
        for (int u = split; u < mp.units; u += mp.splits) {
            int n, ho, wo;
            if (!dw_pos(mp, u, tid, n, ho, wo)) continue;
            const float gv = dw_ld(go[n * gs.n + co * gs.c + ho * gs.h + wo * gs.w]);
            const XT* xp = x + n * xs.n + c * xs.c;
            const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
            acc[CAP] = acc[CAP] + gv;
#pragma unroll
            for (int t = 0; t < CAP; ++t) {
                if (!T::GEN || t < kk) {
                    const int i = t / kw, j = t - i * kw;
                    const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                    if (hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) acc[t] = acc[t] + gv * dw_ld(xp[hi * xs.h + wi * xs.w]);
                }
            }
        }
    }
    // the lanes of a wave that share a channel: the low lane bits (NCHW map) or the bits from the channel lanes up (channels-last)
    const int group = DW_THREADS / mp.slots;                       // NCHW: threads per channel slot
    const int lo = mp.cl ? mp.slots : 1;
    const int hi = mp.cl ? 64 : (group < 64 ? group : 64);
#pragma unroll
    for (int t = 0; t <= CAP; ++t) {
        float v = acc[t];
        for (int off = lo; off < hi; off <<= 1) v = v + __shfl_xor(v, off, 64);
        red[t * DW_THREADS + tid] = v;
    }
    __syncthreads();
    const int per = kk + 1;
    for (int e = tid; e < mp.slots * per; e += DW_THREADS) {
        const int q = e / per, t = e - q * per;
        const float* r = red + (t == kk ? CAP : t) * DW_THREADS;
        float s;
        if (mp.cl) {
            s = r[q];
            for (int wv = 1; wv < DW_THREADS / 64; ++wv) s = s + r[wv * 64 + q];
        } else {
            s = r[q * group];
            for (int wv = 1; wv < group / 64; ++wv) s = s + r[q * group + wv * 64];
        }
        const int64_t oc = cg * mp.slots + q;
        if (oc < g.Cout) work[((int64_t)split * g.Cout + oc) * per + t] = s;
    }
}

// stage 2: the splits in index order, the STE mask on the unquantised weight, the bias gradient; WT: element type of w, gw, gbias
template <typename WT = float>
__global__ __launch_bounds__(DW_THREADS) void dw_grad_weight_combine_kernel(const float* __restrict__ work, const WT* __restrict__ w,
                                                                            WT* __restrict__ gw, WT* __restrict__ gbias,
                                                                            int64_t Cout, int kk, int splits, float thr) {
    const int per = kk + 1;
    const int64_t total = Cout * per;
    for (int64_t e = (int64_t)blockIdx.x * DW_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * DW_THREADS) {
        const int64_t co = e / per;
        const int t = (int)(e - co * per);
        float s = 0.0f;
        for (int sp = 0; sp < splits; ++sp) s = s + work[((int64_t)sp * Cout + co) * per + t];
        if (t < kk) {
            if (thr > 0.0f && fabsf(dw_ld(w[co * kk + t])) > thr) s = 0.0f;
            dw_st(&gw[co * kk + t], s);
        } else if (gbias) {
            dw_st(&gbias[co], s);
        }
    }
}

// validates the shape arguments and fills g; QT_OK with *empty set when there is nothing to compute
int dw_geometry(int64_t N, int64_t C, int64_t m, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                int dw, DwGeom* g, bool* empty) {
    *empty = false;
    if (N < 0 || C < 0 || m < 1 || H < 0 || W < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || dh < 1 || dw < 1)
        return QT_ERR_INVALID_ARG;
    if ((int64_t)kh * kw > DW_MAX_TAPS) return QT_ERR_UNSUPPORTED;
    if (N == 0 || C == 0 || H == 0 || W == 0) {
        *empty = true;
        return QT_OK;
    }
    if (N >= DW_MAX_ELEMS || C >= DW_MAX_ELEMS || H >= DW_MAX_ELEMS || W >= DW_MAX_ELEMS || m >= DW_MAX_ELEMS || ph >= (1 << 24) ||
        pw >= (1 << 24) || dh >= (1 << 24) || dw >= (1 << 24))
        return QT_ERR_UNSUPPORTED;
    if (H + 2 * (int64_t)ph >= DW_MAX_ELEMS || W + 2 * (int64_t)pw >= DW_MAX_ELEMS) return QT_ERR_UNSUPPORTED;     // tap coordinates are int
    const int64_t eh = H + 2 * (int64_t)ph - (int64_t)dh * (kh - 1) - 1, ew = W + 2 * (int64_t)pw - (int64_t)dw * (kw - 1) - 1;
    if (eh < 0 || ew < 0) return QT_ERR_INVALID_ARG;          // the kernel does not fit the padded image
    const int64_t Ho = eh / sh + 1, Wo = ew / sw + 1;
    const double in = (double)N * (double)C * (double)H * (double)W, out = (double)N * (double)C * (double)m * (double)Ho * (double)Wo;
    if (in >= (double)DW_MAX_ELEMS || out >= (double)DW_MAX_ELEMS || (double)C * (double)m > (double)DW_MAX_CHANNELS)
        return QT_ERR_UNSUPPORTED;
    g->N = (int)N; g->C = (int)C; g->m = (int)m; g->H = (int)H; g->W = (int)W; g->Ho = (int)Ho; g->Wo = (int)Wo;
    g->kh = kh; g->kw = kw; g->sh = sh; g->sw = sw; g->ph = ph; g->pw = pw; g->dh = dh; g->dw = dw;
    g->Cout = C * m;
    return QT_OK;
}

constexpr int DW_TARGET_STREAM = 2048;      // workgroups of a forward / grad_input launch: 8 per CU
constexpr int DW_TARGET_REDUCE = 1024;      // ... of the grad_weight stage 1: each one leaves Cout-share x (taps + 1) partials

#define DW_DISPATCH(KERNEL, g, ...)                                                                   \
    do {                                                                                              \
        if ((g).kh == 1 && (g).kw == 1) KERNEL<1, 1><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);        \
        else if ((g).kh == 3 && (g).kw == 3) KERNEL<3, 3><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else if ((g).kh == 5 && (g).kw == 5) KERNEL<5, 5><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else if ((g).kh == 7 && (g).kw == 7) KERNEL<7, 7><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else KERNEL<0, 0><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);                                   \
    } while (0)

// the same for the kernel templates with two element types
#define DW_DISPATCH_T(KERNEL, TA, TB, g, ...)                                                                   \
    do {                                                                                                        \
        if ((g).kh == 1 && (g).kw == 1) KERNEL<1, 1, TA, TB>   <<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);        \
        else if ((g).kh == 3 && (g).kw == 3) KERNEL<3, 3, TA, TB>   <<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else if ((g).kh == 5 && (g).kw == 5) KERNEL<5, 5, TA, TB>   <<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else if ((g).kh == 7 && (g).kw == 7) KERNEL<7, 7, TA, TB>   <<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else KERNEL<0, 0, TA, TB>   <<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);                                   \
    } while (0)

// the same for a kernel template with one more (bool) parameter
#define DW_DISPATCH_B(KERNEL, B, g, ...)                                                                 \
    do {                                                                                                 \
        if ((g).kh == 1 && (g).kw == 1) KERNEL<1, 1, B><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);        \
        else if ((g).kh == 3 && (g).kw == 3) KERNEL<3, 3, B><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else if ((g).kh == 5 && (g).kw == 5) KERNEL<5, 5, B><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else if ((g).kh == 7 && (g).kw == 7) KERNEL<7, 7, B><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);   \
        else KERNEL<0, 0, B><<<grid, DW_THREADS, 0, s>>>(__VA_ARGS__);                                   \
    } while (0)

inline int64_t dw_work_floats(const DwGeom& g, const DwMap& mp) { return (int64_t)mp.splits * g.Cout * (g.kh * g.kw + 1); }

// ---- the forward on / into bit planes (include/qt_hip.h "Depthwise convolution on bit planes") -------------------------------------
// dw_planes_kernel (sign-plane and channels-last fp32 inputs; also planes -> fp32): a HALF-wave (32 lanes) owns one 32-channel word
// of one output pixel, a workgroup (plane word, split) walks 8 pixels per step, so every lane keeps ONE output channel — its taps,
// bias, alpha and beta in registers — for the whole launch.  A plane input costs one word per tap and half-wave (the same address
// in 32 lanes for m == 1), the lane picks its bit; a channels-last fp32 input is read in rows of 32 channels.  The threshold bits
// of a wave come from one __ballot: its low word is the first pixel's, its high word the second's.
// dw_planes_nchw_kernel (NCHW fp32 input): lanes along the pixels, the votes transposed through LDS (see there).
// Either way one lane per (pixel, word) stores the word, the four nibble words made from it and — for the last word of a pixel —
// the pad words of the row.  Nothing is read from an output buffer; the border pixels of a halo plane are zeroed by a walk of
// the whole grid over the plane after the main loop.  That writing stage (DwPlaneOut, dw_store_word, dw_zero_border) is shared with
// the grouped plane kernel of gconv.hip and lives in dw_planes.h.
// BITS_IN: x is the NHWC sign plane of a +-1 activation (ldx words per pixel; bit 1 -> -1.0f, bit 0 -> +1.0f), else fp32 by xs
template <int KH, int KW, bool BITS_IN>
__global__ __launch_bounds__(DW_THREADS) void dw_planes_kernel(const void* __restrict__ xv, int64_t ldx, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ alpha,
                                                               const float* __restrict__ beta, DwPlaneOut o, DwGeom g, DwStrides xs,
                                                               DwStrides ys, int units, int splits, int kind) {
    using T = DwTaps<KH, KW>;
    const int tid = threadIdx.x, lane = tid & 31;
    const int wd = (int)(blockIdx.x / splits);
    const int split = (int)(blockIdx.x - (unsigned)wd * splits);
    const int64_t co = (int64_t)wd * 32 + lane;
    const bool live = co < g.Cout;
    const int kw = T::kw(g), kk = T::kk(g);
    float wq[T::CAP];
#pragma unroll
    for (int t = 0; t < T::CAP; ++t) wq[t] = (live && t < kk) ? dw_quant(kind, w[co * kk + t]) : 0.0f;
    const float b = (live && bias) ? bias[co] : 0.0f;
    const float al = (live && alpha) ? alpha[co] : 0.0f, be = (live && beta) ? beta[co] : 0.0f;
    const int64_t c = live ? co / g.m : 0;
    const int hw = g.Ho * g.Wo;
    const int64_t npix = (int64_t)g.N * hw;
    const float* xf = static_cast<const float*>(xv);
    const uint32_t* xb = static_cast<const uint32_t*>(xv);
    for (int u = split; u < units; u += splits) {
        const int64_t pix = (int64_t)u * DW_PIX_PER_STEP + (tid >> 5);
        const bool in = pix < npix;
        int n = 0, ho = 0, wo = 0;
        if (in) {
            const int p = (int)pix;
            n = p / hw;
            const int r = p - n * hw;
            ho = r / g.Wo;
            wo = r - ho * g.Wo;
        }
        float acc = 0.0f;
        if (in && live) {
            const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
#pragma unroll
            for (int t = 0; t < T::CAP; ++t) {
                if (!T::GEN || t < kk) {
                    const int i = t / kw, j = t - i * kw;
                    const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                    if (hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) {
                        float v;
                        if (BITS_IN) {
                            const uint32_t word = xb[(((int64_t)n * g.H + hi) * g.W + wi) * ldx + (c >> 5)];
                            v = ((word >> (c & 31)) & 1u) ? -1.0f : 1.0f;
                        } else {
                            v = xf[n * xs.n + c * xs.c + hi * xs.h + wi * xs.w];
                        }
                        acc = acc + v * wq[t];
                    }
                }
            }
            if (bias) acc = acc + b;
        }
        if (o.y) {                                   // uniform over the launch
            if (in && live) o.y[n * ys.n + co * ys.c + ho * ys.h + wo * ys.w] = acc;
            continue;
        }
        // two roundings (the build has -ffp-contract=off), as in pool_affine_sign_pack_kernel; dead lanes vote 0
        const int neg = (in && live) ? (int)qt_neg_bit(acc * al + be) : 0;
        const unsigned long long votes = __ballot(neg);
        if (lane != 0 || !in) continue;
        dw_store_word(o, g, wd, pix, n, ho, wo, (uint32_t)(votes >> (tid & 32)));
    }
    if (!o.y) dw_zero_border(o, g, tid);
}

// fp32 NCHW input -> planes.  The map above would read such an input with one image plane between neighbouring lanes, so here
// the 64 lanes of a wave run along 64 consecutive output pixels (rows of x, coalesced) and a wave walks 8 of the workgroup's 32
// channels with wave-uniform taps, bias, alpha and beta.  The votes of (channel, 64 pixels) go through 256 bytes of LDS and come
// back as (pixel, 32 channels) words, which wave 0 stores as above.  Same arithmetic, same bits.
template <int KH, int KW>
__global__ __launch_bounds__(DW_THREADS) void dw_planes_nchw_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, const float* __restrict__ alpha,
                                                                    const float* __restrict__ beta, DwPlaneOut o, DwGeom g,
                                                                    DwStrides xs, int units, int splits, int kind) {
    using T = DwTaps<KH, KW>;
    __shared__ unsigned long long votes[32];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wd = (int)(blockIdx.x / splits);
    const int split = (int)(blockIdx.x - (unsigned)wd * splits);
    const int kw = T::kw(g), kk = T::kk(g);
    const int hw = g.Ho * g.Wo;
    const int64_t npix = (int64_t)g.N * hw;
    for (int u = split; u < units; u += splits) {
        const int64_t pix = (int64_t)u * 64 + lane;
        const bool in = pix < npix;
        int n = 0, ho = 0, wo = 0;
        if (in) {
            const int p = (int)pix;
            n = p / hw;
            const int r = p - n * hw;
            ho = r / g.Wo;
            wo = r - ho * g.Wo;
        }
        const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
        for (int q = 0; q < 8; ++q) {
            const int cl = wave * 8 + q;
            const int64_t co = (int64_t)wd * 32 + cl;             // wave-uniform
            int neg = 0;
            if (co < g.Cout && in) {
                const float* xp = x + n * xs.n + (co / g.m) * xs.c;
                const float* wp = w + co * kk;
                float acc = 0.0f;
                auto tap = [&](int t) {
                    const int i = t / kw, j = t - i * kw;
                    const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                    if (hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) acc = acc + xp[hi * xs.h + wi * xs.w] * dw_quant(kind, wp[t]);
                };
                if (T::GEN) {               // the taps are read where they are used (wave-uniform): nothing to keep in registers
                    for (int t = 0; t < kk; ++t) tap(t);
                } else {
#pragma unroll
                    for (int t = 0; t < T::CAP; ++t) tap(t);
                }
                if (bias) acc = acc + bias[co];
                neg = (int)qt_neg_bit(acc * alpha[co] + beta[co]);      // two roundings
            }
            const unsigned long long v = __ballot(neg);
            if (lane == 0) votes[cl] = v;
        }
        __syncthreads();
        if (tid < 64 && in) {
            uint32_t word = 0;
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) word |= (uint32_t)((votes[cc] >> lane) & 1ull) << cc;
            dw_store_word(o, g, wd, pix, n, ho, wo, word);
        }
        __syncthreads();
    }
    dw_zero_border(o, g, tid);
}

// the shared body of the two plane entries: exactly one of (x, x_plane) is given; o.y, or at least one of o.sign / o.nib
int dw_planes_launch(const float* x, const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, const float* alpha,
                     const float* beta, DwPlaneOut o, int64_t halo_h, int64_t halo_w, int64_t N, int64_t C, int64_t m, int64_t H,
                     int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, DwStrides xs, DwStrides ys, int kind,
                     qt_stream_t stream) {
    DwGeom g{};
    bool empty;
    if (halo_h < 0 || halo_w < 0) return QT_ERR_INVALID_ARG;
    const int rc = dw_geometry(N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (halo_h > DW_MAX_HALO || halo_w > DW_MAX_HALO) return QT_ERR_UNSUPPORTED;
    if (o.nib && (double)N * (double)(g.Ho + 2 * halo_h) * (double)(g.Wo + 2 * halo_w) >= (double)DW_MAX_ELEMS) return QT_ERR_UNSUPPORTED;
    if (kind != QT_DW_RAW && kind != QT_DW_SIGN && kind != QT_DW_TERNARY) return QT_ERR_INVALID_ARG;
    if ((x == nullptr) == (x_plane == nullptr) || !w) return QT_ERR_INVALID_ARG;
    if (o.y) {
        if (dw_layout(N, g.Cout, g.Ho, g.Wo, ys) < 0) return QT_ERR_INVALID_ARG;
    } else {
        if ((!o.sign && !o.nib) || !alpha || !beta) return QT_ERR_INVALID_ARG;
        if (o.sign && o.ldb < dw_packed_ld(g.Cout)) return QT_ERR_INVALID_ARG;
        if (o.nib && o.ldn < dw_pixel_ld_nib(g.Cout)) return QT_ERR_INVALID_ARG;
    }
    if (x && dw_layout(N, C, H, W, xs) < 0) return QT_ERR_INVALID_ARG;
    if (x_plane && ldx < dw_packed_ld(C)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(x) || !dw_aligned4(x_plane) || !dw_aligned4(w) || !dw_aligned4(bias) || !dw_aligned4(alpha) || !dw_aligned4(beta) ||
        !dw_aligned4(o.y) || !dw_aligned4(o.sign))
        return QT_ERR_ALIGNMENT;
    if (o.nib && ((o.ldn & 3) || !dw_aligned16(o.nib))) return QT_ERR_ALIGNMENT;
    o.hy = (int)halo_h;
    o.hx = (int)halo_w;
    const int64_t npix = (int64_t)g.N * g.Ho * g.Wo;
    const int64_t nw = (g.Cout + 31) / 32;
    const bool nchw = x && !o.y && dw_layout(N, C, H, W, xs) == 0;      // lanes along the pixels, 64 per step
    const int per_step = nchw ? 64 : DW_PIX_PER_STEP;
    const int units = (int)((npix + per_step - 1) / per_step);
    int64_t sp = (DW_TARGET_STREAM + nw - 1) / nw;
    if (sp > units) sp = units;
    const int splits = (int)(sp < 1 ? 1 : sp);
    const unsigned grid = (unsigned)(nw * splits);
    hipStream_t s = (hipStream_t)stream;
    if (nchw) {
        DW_DISPATCH(dw_planes_nchw_kernel, g, x, w, bias, alpha, beta, o, g, xs, units, splits, kind);
        return qt_check_launch();
    }
    const void* xv = x ? static_cast<const void*>(x) : static_cast<const void*>(x_plane);
#define DW_PLANES_ARGS xv, ldx, w, bias, alpha, beta, o, g, xs, ys, units, splits, kind
    if (x) DW_DISPATCH_B(dw_planes_kernel, false, g, DW_PLANES_ARGS);
    else DW_DISPATCH_B(dw_planes_kernel, true, g, DW_PLANES_ARGS);
#undef DW_PLANES_ARGS
    return qt_check_launch();
}

// ---- the forward on / into int8 code planes (include/qt_hip.h "Depthwise convolution on int8 code planes") -------------------------
// dw_codes_kernel: a lane owns ONE DWORD of output channels (4 codes) for the whole launch — its 4 x taps, biases and BatchNorm
// constants in registers — and the lanes of a workgroup run along the dwords of a pixel row first (`lanes` = the row's dwords
// rounded up to a power of two, at most 64), then along 256 / lanes consecutive output pixels.  A workgroup is (dword group, split)
// and walks pixel steps split, split + S, ...: the pixel advances by a constant, so (n, ho, wo) move by constant increments with
// two carries (no division per element; the FIXED walk of affine_dorefa_codes is the model).  For m == 1 a tap is one 4-byte load
// per lane, contiguous along the channels across the lanes; for m > 1 the four input bytes are read one by one.  Taps outside the
// image are not added; their (discarded) load goes to the nearest pixel INSIDE the image, never to the halo.  The epilogue is
// affine_codes_word of codes_epilogue.h; the dwords past C m of a row are written by lanes of their own as zero, the border pixels
// of a halo plane by the same thread map after the main loop.  Nothing is read from the output.
struct DwCodesMap {
    int lanes_log;            // log2 of the lanes along the dwords of a pixel row
    int slots;                // dwords per output pixel row that are written: ldc / 4, or ceil(C m / 4) for the fp32 form
    int units, splits;        // pixel steps of 256 >> lanes_log pixels, workgroups per dword group
    int d_n, d_ho, d_wo;      // splits * (256 >> lanes_log) pixels as (images, rows, columns)
    int ihy, ihx, ohy, ohx;   // halos of the input and the output plane
};

struct DwCodesEpi {
    const float* alpha;
    const float* beta;
    const float* bn_stats;
    int relu;
    float n;
    int8_t* codes;
    int64_t ldc;
    int32_t* overflow;
};

struct DwF32Out {
    float* y;
    DwStrides ys;
    const int32_t* overflow;
    int vec;                  // channels-last, C m % 4 == 0, 16-byte aligned: one float4 store per lane
};

template <int KH, int KW, bool F32OUT>
__global__ __launch_bounds__(DW_THREADS) void dw_codes_kernel(const int8_t* __restrict__ x, int64_t ldx, float inv_n,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              DwCodesEpi ep, DwF32Out fo, DwGeom g, DwCodesMap mp) {
    using T = DwTaps<KH, KW>;
    const int tid = threadIdx.x;
    const int lanes = 1 << mp.lanes_log, tpix = DW_THREADS >> mp.lanes_log;
    const int sg = (int)(blockIdx.x / mp.splits);
    const int split = (int)(blockIdx.x - (unsigned)sg * mp.splits);
    const int slot = sg * lanes + (tid & (lanes - 1));
    const int ps = tid >> mp.lanes_log;
    const bool row_lane = slot < mp.slots;                     // this lane writes a dword of every pixel row
    const int64_t co0 = (int64_t)slot * 4;
    const int nvalid = (int)(g.Cout - co0 < 0 ? 0 : (g.Cout - co0 > 4 ? 4 : g.Cout - co0));
    const int kw = T::kw(g), kk = T::kk(g);
    const bool one = g.m == 1;
    float wq[4][T::CAP], b[4];
    int cin[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool live = e < nvalid;
#pragma unroll
        for (int t = 0; t < T::CAP; ++t) wq[e][t] = (live && t < kk) ? w[(co0 + e) * kk + t] : 0.0f;
        b[e] = (live && bias) ? bias[co0 + e] : 0.0f;
        cin[e] = live ? (int)((co0 + e) / g.m) : 0;
    }
    AffineConsts ac;
    if (!F32OUT) affine_load_consts(ac, co0, g.Cout, ep.alpha, ep.beta, nullptr, nullptr, ep.bn_stats, nullptr);
    const bool devbn = ep.bn_stats != nullptr;
    const bool nan_all = F32OUT && fo.overflow != nullptr && *fo.overflow != 0;
    const int Hp = g.H + 2 * mp.ihy, Wp = g.W + 2 * mp.ihx;
    const int Hop = g.Ho + 2 * mp.ohy, Wop = g.Wo + 2 * mp.ohx;
    const unsigned npix = (unsigned)g.N * (unsigned)(g.Ho * g.Wo);              // < 2^31: host check
    int bad = 0;
    // the first pixel of this thread, then constant increments
    unsigned p = (unsigned)split * tpix + ps;
    int n = (int)(p / (unsigned)(g.Ho * g.Wo));
    int ho, wo;
    {
        const unsigned r = p - (unsigned)n * (unsigned)(g.Ho * g.Wo);
        ho = (int)(r / (unsigned)g.Wo);
        wo = (int)(r - (unsigned)ho * g.Wo);
    }
    for (int u = split; u < mp.units; u += mp.splits) {
        if (p < npix && row_lane) {
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (nvalid > 0) {
                const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
                int i = 0, j = 0;
#pragma unroll
                for (int t = 0; t < T::CAP; ++t) {
                    if (!T::GEN || t < kk) {
                        const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                        const bool ok = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                        const int hc = hi < 0 ? 0 : (hi >= g.H ? g.H - 1 : hi), wc = wi < 0 ? 0 : (wi >= g.W ? g.W - 1 : wi);
                        const int8_t* px = x + (int64_t)((n * Hp + hc + mp.ihy) * Wp + wc + mp.ihx) * ldx;
                        float v[4];
                        if (one) {
                            const uint32_t word = *reinterpret_cast<const uint32_t*>(px + co0);       // co0 + 3 < ldx: rows are 16-byte padded
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = inv_n * (float)(int8_t)(word >> (8 * e));
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = inv_n * (float)px[cin[e]];
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = ok ? acc[e] + v[e] * wq[e][t] : acc[e];
                    }
                    if (++j == kw) { j = 0; ++i; }
                }
                if (bias) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] = acc[e] + b[e];
                }
            }
            if (F32OUT) {
                if (nan_all) acc[0] = acc[1] = acc[2] = acc[3] = __builtin_nanf("");
                float* dst = fo.y + n * fo.ys.n + co0 * fo.ys.c + ho * fo.ys.h + wo * fo.ys.w;
                if (fo.vec) {
                    *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < nvalid) dst[e * fo.ys.c] = acc[e];
                }
            } else {
                const float r0[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                float q4[4];
                const uint32_t word = affine_codes_word(acc, r0, 0u, ac, nvalid, devbn, false, false, false, false, 0.0f, ep.relu, ep.n, q4, bad);
                *reinterpret_cast<uint32_t*>(ep.codes + (int64_t)((n * Hop + ho + mp.ohy) * Wop + wo + mp.ohx) * ep.ldc + co0) = word;
            }
        }
        p += (unsigned)mp.splits * tpix;
        wo += mp.d_wo;
        const int c1 = wo >= g.Wo;
        wo -= c1 ? g.Wo : 0;
        ho += mp.d_ho + c1;
        const int c2 = ho >= g.Ho;
        ho -= c2 ? g.Ho : 0;
        n += mp.d_n + c2;
    }
    if (F32OUT) return;
    if ((mp.ohy | mp.ohx) && row_lane) {
        // the border pixels of the output plane, enumerated alone: per image ohy rows on top, 2 ohx columns beside each of the
        // Ho image rows, ohy rows below (the enumeration of halo_zero_border in codes_i8.hip); one dword per lane
        const unsigned top = (unsigned)mp.ohy * Wop, side = 2u * mp.ohx * g.Ho, per_img = 2u * top + side;
        const unsigned total = (unsigned)g.N * per_img;                        // < 2^31: host check on the plane's pixel rows
        for (unsigned t = (unsigned)split * tpix + ps; t < total; t += (unsigned)mp.splits * tpix) {
            const unsigned img = t / per_img, r = t - img * per_img;
            unsigned h, c;
            if (r < top) { h = r / Wop; c = r - h * Wop; }
            else if (r < top + side) {
                const unsigned q = r - top, row = q / (2u * mp.ohx), k = q - row * 2u * mp.ohx;
                h = mp.ohy + row;
                c = k < (unsigned)mp.ohx ? k : g.Wo + k;
            } else { const unsigned q = r - top - side; h = mp.ohy + g.Ho + q / Wop; c = q % Wop; }
            *reinterpret_cast<uint32_t*>(ep.codes + (int64_t)((img * Hop + h) * Wop + c) * ep.ldc + co0) = 0u;
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(ep.overflow, __any(bad & 2) ? 3 : 1);
}

inline int64_t dw_code_ld(int64_t K) { return std::max<int64_t>(16, (K + 15) / 16 * 16); }

// the shared body of the two code-plane entries: ep.codes (code plane out) or fo.y (fp32 out)
int dw_codes_launch(const int8_t* x_plane, int64_t ldx, int64_t ihy, int64_t ihx, float inv_n, const float* w, const float* bias,
                    DwCodesEpi ep, int bit_width, int64_t ohy, int64_t ohx, DwF32Out fo, int64_t N, int64_t C, int64_t m, int64_t H,
                    int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, bool f32, qt_stream_t stream) {
    DwGeom g{};
    bool empty;
    if (ihy < 0 || ihx < 0 || ohy < 0 || ohx < 0) return QT_ERR_INVALID_ARG;
    const int rc = dw_geometry(N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (ihy > DW_MAX_HALO || ihx > DW_MAX_HALO || ohy > DW_MAX_HALO || ohx > DW_MAX_HALO) return QT_ERR_UNSUPPORTED;
    if ((double)N * (double)(H + 2 * ihy) * (double)(W + 2 * ihx) >= (double)DW_MAX_ELEMS ||
        (double)N * (double)(g.Ho + 2 * ohy) * (double)(g.Wo + 2 * ohx) >= (double)DW_MAX_ELEMS)
        return QT_ERR_UNSUPPORTED;
    if (!x_plane || !w) return QT_ERR_INVALID_ARG;
    if (f32) {
        if (!fo.y || dw_layout(N, g.Cout, g.Ho, g.Wo, fo.ys) < 0) return QT_ERR_INVALID_ARG;
    } else {
        if (bit_width < 2 || bit_width > 8 || ep.relu < 0 || ep.relu > 1) return QT_ERR_INVALID_ARG;
        if (!ep.alpha || !ep.beta || !ep.codes || !ep.overflow) return QT_ERR_INVALID_ARG;
        if (ep.ldc < dw_code_ld(g.Cout)) return QT_ERR_INVALID_ARG;
        if (ep.ldc >= DW_MAX_ELEMS) return QT_ERR_UNSUPPORTED;
    }
    if (ldx < dw_code_ld(C)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(w) || !dw_aligned4(bias) || !dw_aligned4(ep.alpha) || !dw_aligned4(ep.beta) || !dw_aligned4(ep.bn_stats) ||
        !dw_aligned4(ep.overflow) || !dw_aligned4(fo.overflow) || !dw_aligned4(fo.y))
        return QT_ERR_ALIGNMENT;
    if ((ldx & 15) || !dw_aligned16(x_plane) || (ep.ldc & 15) || !dw_aligned16(ep.codes)) return QT_ERR_ALIGNMENT;
    ep.n = (float)((1 << (f32 ? 2 : bit_width)) - 1);
    fo.vec = f32 && dw_layout(N, g.Cout, g.Ho, g.Wo, fo.ys) == 1 && fo.ys.c == 1 && (g.Cout & 3) == 0 && dw_aligned16(fo.y);
    DwCodesMap mp{};
    const int64_t slots = f32 ? (g.Cout + 3) / 4 : ep.ldc / 4;
    const int lanes = dw_pow2ceil(slots < 64 ? slots : 64);
    mp.lanes_log = dw_log2(lanes);
    mp.slots = (int)slots;
    const int tpix = DW_THREADS / lanes;
    const int64_t npix = (int64_t)g.N * g.Ho * g.Wo;
    mp.units = (int)((npix + tpix - 1) / tpix);
    const int64_t groups = (slots + lanes - 1) / lanes;
    int64_t sp = (DW_TARGET_STREAM + groups - 1) / groups;
    if (sp > mp.units) sp = mp.units;
    mp.splits = (int)(sp < 1 ? 1 : sp);
    const int64_t step = (int64_t)mp.splits * tpix;
    mp.d_wo = (int)(step % g.Wo);
    mp.d_ho = (int)((step / g.Wo) % g.Ho);
    mp.d_n = (int)(step / g.Wo / g.Ho);
    mp.ihy = (int)ihy; mp.ihx = (int)ihx; mp.ohy = (int)ohy; mp.ohx = (int)ohx;
    const unsigned grid = (unsigned)(groups * mp.splits);
    hipStream_t s = (hipStream_t)stream;
    if (f32) DW_DISPATCH_B(dw_codes_kernel, true, g, x_plane, ldx, inv_n, w, bias, ep, fo, g, mp);
    else DW_DISPATCH_B(dw_codes_kernel, false, g, x_plane, ldx, inv_n, w, bias, ep, fo, g, mp);
    return qt_check_launch();
}

// The bodies of the three entries for any element types (the "_f32" entries: all float).  Validation order: qt_hip.h.
template <typename XT, typename WT>
int dw_forward_entry(const XT* x, const WT* w, const float* bias, XT* y, int64_t N, int64_t C, int64_t m, int64_t H, int64_t W, int kh,
                     int kw, int sh, int sw, int ph, int pw, int dh, int dw, const DwStrides& xs, const DwStrides& ys, int kind,
                     qt_stream_t stream) {
    DwGeom g{};
    bool empty;
    const int rc = dw_geometry(N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (kind != QT_DW_RAW && kind != QT_DW_SIGN && kind != QT_DW_TERNARY) return QT_ERR_INVALID_ARG;
    if (!x || !w || !y) return QT_ERR_INVALID_ARG;
    const int ly = dw_layout(N, g.Cout, g.Ho, g.Wo, ys);
    if (dw_layout(N, C, H, W, xs) < 0 || ly < 0) return QT_ERR_INVALID_ARG;
    if (!dw_aligned_elt(x) || !dw_aligned_elt(w) || !dw_aligned_elt(y) || !dw_aligned4(bias)) return QT_ERR_ALIGNMENT;
    const DwMap mp = dw_plan(ly, N, g.Cout, g.Ho, g.Wo, DW_TARGET_STREAM);
    const unsigned grid = (unsigned)(mp.cgs * mp.splits);
    hipStream_t s = (hipStream_t)stream;
    DW_DISPATCH_T(dw_forward_kernel, XT, WT, g, x, w, bias, y, g, xs, ys, mp, kind);
    return qt_check_launch();
}

template <typename XT, typename WT>
int dw_grad_input_entry(const XT* go, const WT* w, XT* gx, int64_t N, int64_t C, int64_t m, int64_t H, int64_t W, int kh, int kw, int sh,
                        int sw, int ph, int pw, int dh, int dw, const DwStrides& gs, const DwStrides& xs, int kind, qt_stream_t stream) {
    DwGeom g{};
    bool empty;
    const int rc = dw_geometry(N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (kind != QT_DW_RAW && kind != QT_DW_SIGN && kind != QT_DW_TERNARY) return QT_ERR_INVALID_ARG;
    if (!go || !w || !gx) return QT_ERR_INVALID_ARG;
    const int lx = dw_layout(N, C, H, W, xs);
    if (dw_layout(N, g.Cout, g.Ho, g.Wo, gs) < 0 || lx < 0) return QT_ERR_INVALID_ARG;
    if (!dw_aligned_elt(go) || !dw_aligned_elt(w) || !dw_aligned_elt(gx)) return QT_ERR_ALIGNMENT;
    const DwMap mp = dw_plan(lx, N, C, g.H, g.W, DW_TARGET_STREAM);
    const unsigned grid = (unsigned)(mp.cgs * mp.splits);
    hipStream_t s = (hipStream_t)stream;
    DW_DISPATCH_T(dw_grad_input_kernel, XT, WT, g, go, w, gx, g, gs, xs, mp, kind);
    return qt_check_launch();
}

template <typename XT, typename WT>
int dw_grad_weight_entry(const XT* go, const XT* x, const WT* w, WT* gw, WT* gbias, float* work, int64_t work_floats, int64_t N,
                         int64_t C, int64_t m, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                         const DwStrides& gs, const DwStrides& xs, float ste_threshold, qt_stream_t stream) {
    DwGeom g{};
    bool empty;
    const int rc = dw_geometry(N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK) return rc;
    if (empty) return QT_OK;          // nothing is written: the caller owns the zero gradient of an empty batch
    if (!gw || (ste_threshold > 0.0f && !w) || !(ste_threshold >= 0.0f)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned_elt(gw) || !dw_aligned_elt(gbias) || !dw_aligned_elt(w)) return QT_ERR_ALIGNMENT;
    hipStream_t s = (hipStream_t)stream;
    const int kk = kh * kw;
    if (!go || !x || !work || work_floats < 0) return QT_ERR_INVALID_ARG;
    const int lg = dw_layout(N, g.Cout, g.Ho, g.Wo, gs);
    if (lg < 0 || dw_layout(N, C, H, W, xs) < 0) return QT_ERR_INVALID_ARG;
    if (!dw_aligned_elt(go) || !dw_aligned_elt(x) || !dw_aligned4(work)) return QT_ERR_ALIGNMENT;
    const DwMap mp = dw_plan(lg, N, g.Cout, g.Ho, g.Wo, DW_TARGET_REDUCE);
    if (work_floats < dw_work_floats(g, mp)) return QT_ERR_INVALID_ARG;
    const unsigned grid = (unsigned)(mp.cgs * mp.splits);
    DW_DISPATCH_T(dw_grad_weight_kernel, XT, XT, g, go, x, work, g, gs, xs, mp);
    int st = qt_check_launch();
    if (st != QT_OK) return st;
    dw_grad_weight_combine_kernel<WT><<<qt_stream_grid((g.Cout * (kk + 1) + DW_THREADS - 1) / DW_THREADS), DW_THREADS, 0, s>>>(
        work, w, gw, gbias, g.Cout, kk, mp.splits, ste_threshold);
    return qt_check_launch();
}

}  // namespace

extern "C" int qt_dwconv2d_f32(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t C, int64_t m, int64_t H,
                               int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t xs_n, int64_t xs_c,
                               int64_t xs_h, int64_t xs_w, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w, int kind,
                               qt_stream_t stream) {
    return dw_forward_entry(x, w, bias, y, N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, DwStrides{xs_n, xs_c, xs_h, xs_w},
                            DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}

extern "C" int qt_dwconv2d_h(const void* x, int dtype, const void* w, int w_dtype, const float* bias, void* y, int64_t N, int64_t C,
                             int64_t m, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                             int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int64_t ys_n, int64_t ys_c, int64_t ys_h,
                             int64_t ys_w, int kind, qt_stream_t stream) {
    int rc = QT_ERR_INVALID_ARG;
    dw_half_types(dtype, w_dtype, [&](auto* xt, auto* wt) {
        using XT = std::remove_pointer_t<decltype(xt)>;
        using WT = std::remove_pointer_t<decltype(wt)>;
        rc = dw_forward_entry(static_cast<const XT*>(x), static_cast<const WT*>(w), bias, static_cast<XT*>(y), N, C, m, H, W, kh, kw, sh,
                              sw, ph, pw, dh, dw, DwStrides{xs_n, xs_c, xs_h, xs_w}, DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
    });
    return rc;
}

extern "C" int qt_dwconv2d_grad_input_f32(const float* go, const float* w, float* gx, int64_t N, int64_t C, int64_t m, int64_t H,
                                          int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t gs_n,
                                          int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c, int64_t xs_h,
                                          int64_t xs_w, int kind, qt_stream_t stream) {
    return dw_grad_input_entry(go, w, gx, N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, DwStrides{gs_n, gs_c, gs_h, gs_w},
                               DwStrides{xs_n, xs_c, xs_h, xs_w}, kind, stream);
}

extern "C" int qt_dwconv2d_grad_input_h(const void* go, int dtype, const void* w, int w_dtype, void* gx, int64_t N, int64_t C, int64_t m,
                                        int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                        int64_t gs_n, int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c,
                                        int64_t xs_h, int64_t xs_w, int kind, qt_stream_t stream) {
    int rc = QT_ERR_INVALID_ARG;
    dw_half_types(dtype, w_dtype, [&](auto* xt, auto* wt) {
        using XT = std::remove_pointer_t<decltype(xt)>;
        using WT = std::remove_pointer_t<decltype(wt)>;
        rc = dw_grad_input_entry(static_cast<const XT*>(go), static_cast<const WT*>(w), static_cast<XT*>(gx), N, C, m, H, W, kh, kw, sh,
                                 sw, ph, pw, dh, dw, DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, kind, stream);
    });
    return rc;
}

extern "C" int64_t qt_dwconv2d_grad_weight_work_floats(int64_t N, int64_t C, int64_t m, int64_t H, int64_t W, int kh, int kw, int sh,
                                                       int sw, int ph, int pw, int dh, int dw) {
    DwGeom g{};
    bool empty;
    const int rc = dw_geometry(N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK) return rc;
    if (empty) return 0;
    // either layout of the gradient: the larger of the two plans
    const int64_t a = dw_work_floats(g, dw_plan(0, N, g.Cout, g.Ho, g.Wo, DW_TARGET_REDUCE));
    const int64_t b = dw_work_floats(g, dw_plan(1, N, g.Cout, g.Ho, g.Wo, DW_TARGET_REDUCE));
    return a > b ? a : b;
}

extern "C" int qt_dwconv2d_grad_weight_f32(const float* go, const float* x, const float* w, float* gw, float* gbias, float* work,
                                           int64_t work_floats, int64_t N, int64_t C, int64_t m, int64_t H, int64_t W, int kh, int kw,
                                           int sh, int sw, int ph, int pw, int dh, int dw, int64_t gs_n, int64_t gs_c, int64_t gs_h,
                                           int64_t gs_w, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, float ste_threshold,
                                           qt_stream_t stream) {
    return dw_grad_weight_entry(go, x, w, gw, gbias, work, work_floats, N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                                DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, ste_threshold, stream);
}

extern "C" int qt_dwconv2d_grad_weight_h(const void* go, const void* x, int dtype, const void* w, void* gw, void* gbias, int w_dtype,
                                         float* work, int64_t work_floats, int64_t N, int64_t C, int64_t m, int64_t H, int64_t W, int kh,
                                         int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t gs_n, int64_t gs_c,
                                         int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w,
                                         float ste_threshold, qt_stream_t stream) {
    int rc = QT_ERR_INVALID_ARG;
    dw_half_types(dtype, w_dtype, [&](auto* xt, auto* wt) {
        using XT = std::remove_pointer_t<decltype(xt)>;
        using WT = std::remove_pointer_t<decltype(wt)>;
        rc = dw_grad_weight_entry(static_cast<const XT*>(go), static_cast<const XT*>(x), static_cast<const WT*>(w), static_cast<WT*>(gw),
                                  static_cast<WT*>(gbias), work, work_floats, N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                                  DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, ste_threshold, stream);
    });
    return rc;
}

extern "C" int qt_dwconv2d_sign(const float* x, const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias,
                                const float* alpha, const float* beta, uint32_t* sign_plane, int64_t ldb, uint32_t* nib_plane,
                                int64_t ldn, int64_t out_halo_h, int64_t out_halo_w, int64_t N, int64_t C, int64_t m, int64_t H,
                                int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t xs_n, int64_t xs_c,
                                int64_t xs_h, int64_t xs_w, int kind, qt_stream_t stream) {
    DwPlaneOut o{};
    o.sign = sign_plane;
    o.ldb = ldb;
    o.nib = nib_plane;
    o.ldn = ldn;
    return dw_planes_launch(x, x_plane, ldx, w, bias, alpha, beta, o, out_halo_h, out_halo_w, N, C, m, H, W, kh, kw, sh, sw, ph, pw,
                            dh, dw, DwStrides{xs_n, xs_c, xs_h, xs_w}, DwStrides{0, 0, 0, 0}, kind, stream);
}

extern "C" int qt_dwconv2d_bits_f32(const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, float* y, int64_t N,
                                    int64_t C, int64_t m, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                    int dw, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w, int kind, qt_stream_t stream) {
    DwGeom g{};
    bool empty;
    const int rc = dw_geometry(N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (!x_plane || !y) return QT_ERR_INVALID_ARG;
    DwPlaneOut o{};
    o.y = y;
    return dw_planes_launch(nullptr, x_plane, ldx, w, bias, nullptr, nullptr, o, 0, 0, N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                            DwStrides{0, 0, 0, 0}, DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}

extern "C" int qt_dwconv2d_codes(const int8_t* x_plane, int64_t ldx_bytes, int64_t in_halo_h, int64_t in_halo_w, float inv_n,
                                 const float* w, const float* bias, const float* alpha, const float* beta, const float* bn_stats,
                                 int relu, int bit_width, int8_t* codes, int64_t ldc_bytes, int64_t out_halo_h, int64_t out_halo_w,
                                 int32_t* overflow, int64_t N, int64_t C, int64_t m, int64_t H, int64_t W, int kh, int kw, int sh,
                                 int sw, int ph, int pw, int dh, int dw, qt_stream_t stream) {
    DwCodesEpi ep{};
    ep.alpha = alpha;
    ep.beta = beta;
    ep.bn_stats = bn_stats;
    ep.relu = relu;
    ep.codes = codes;
    ep.ldc = ldc_bytes;
    ep.overflow = overflow;
    return dw_codes_launch(x_plane, ldx_bytes, in_halo_h, in_halo_w, inv_n, w, bias, ep, bit_width, out_halo_h, out_halo_w, DwF32Out{},
                           N, C, m, H, W, kh, kw, sh, sw, ph, pw, dh, dw, false, stream);
}

extern "C" int qt_dwconv2d_codes_f32(const int8_t* x_plane, int64_t ldx_bytes, int64_t in_halo_h, int64_t in_halo_w, float inv_n,
                                     const float* w, const float* bias, const int32_t* overflow, float* y, int64_t N, int64_t C,
                                     int64_t m, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                     int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w, qt_stream_t stream) {
    DwF32Out fo{};
    fo.y = y;
    fo.ys = DwStrides{ys_n, ys_c, ys_h, ys_w};
    fo.overflow = overflow;
    return dw_codes_launch(x_plane, ldx_bytes, in_halo_h, in_halo_w, inv_n, w, bias, DwCodesEpi{}, 0, 0, 0, fo, N, C, m, H, W, kh, kw,
                           sh, sw, ph, pw, dh, dw, true, stream);
}
