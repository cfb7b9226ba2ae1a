// Grouped conv2d with a few channels per group (1 <= cin_g <= 32, K = cin_g * kh * kw <= 512) in fp32: forward, grad_input,
// grad_weight — and the forward on / into the bit planes of the fused sign chain (gc_planes_kernel) and the int8 code planes of the
// fused DoReFa chain (gc_codes_kernel), both further down.
// include/qt_hip.h "Grouped convolution" states the contract; DESIGN.md "Grouped convs" the layout and the counts.
//
// Streaming kernels on the vector units, siblings of dwconv.hip: K is no matrix-core shape and the block-diagonal operand would
// waste `groups` times the tile.  What separates them from cout_g depthwise passes is the register block: a lane owns ONE pixel
// and CB channels of it (CB = 4, 8 or 16), so every input it loads feeds CB multiply-adds.
//   forward    : a workgroup is (group, block of CB output channels of that group, split of the pixels).  It quantises its
//                CB x K weights once into LDS as wl[k][CB] (k = ci * taps + t, the weight's own order), so the CB weights of a
//                term are one wave-uniform 16 / 32 / 64-byte read (a broadcast, no bank conflict whatever the layout), then walks
//                pixels split * 256 + tid, (split + S) * 256 + tid, ... of the flat (n, ho, wo) index: lanes run along W of an
//                NCHW tensor (coalesced loads and stores) and along the pixels of a channels-last one (each lane reads the cin_g
//                and writes the CB consecutive channels of its pixel).
//   grad_input : the same with the roles turned: the block is CB input channels of the group, the terms run over the group's
//                output channels j (outermost) and the taps; the weights wl[j][t][CB] are staged in chunks of j that fit 32 KiB.
//   grad_weight: 1 x 1 and 3 x 3: a lane owns one output pixel and the partial sums of a COB x CIB block of (output, input)
//                channels of one group in registers (gc_grad_weight_tile_kernel).  Any other kernel: the stage-1 reduction of
//                dwconv.hip over "virtual channels" v = co * cin_g + ci (the thread map of dw_map.h, chosen by the layout of go;
//                go is read cin_g times, from cache).  Either way one partial per (split, v, tap) in the workspace and one more
//                per (split, co) for the bias gradient; a second launch adds the splits in index order.
// The compile-time forms (1 x 1, 3 x 3) are branch-free: all loads of a channel go out together; the generic forms branch per tap.
//
// Arithmetic (the build has -ffp-contract=off): one fp32 multiply and one fp32 add per term, the accumulator starts at +0, terms
// in the order stated above, taps outside the image skipped, bias last.  No atomics anywhere: equal inputs give equal bits.
#include "qt_common.h"
#include "dw_map.h"
#include "dw_planes.h"
#include "codes_epilogue.h"

namespace {

constexpr int GC_MAX_CIN_G = QT_GC_MAX_CIN_G;
constexpr int GC_MAX_K = QT_GC_MAX_K;
constexpr int GC_MAX_TAPS = QT_DW_MAX_TAPS;
constexpr int GC_LDS_FLOATS = 16 * GC_MAX_K;                 // 32 KiB: the largest forward block, the chunk size of grad_input
constexpr int64_t GC_MAX_ELEMS = (int64_t)1 << 31;
constexpr int64_t GC_MAX_CHANNELS = QT_DW_MAX_CHANNELS;      // bounds the one-dimensional grid: channel blocks + the split target
constexpr int GC_TARGET_STREAM = 2048;                       // workgroups of a forward / grad_input launch: 8 per CU
constexpr int GC_TARGET_REDUCE = 1024;                       // ... of the grad_weight stage 1

struct GcGeom {
    int N, G, cin_g, cout_g, H, W, Ho, Wo;
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int64_t Cin, Cout;
};

// (group, channel block) x split of the pixel units of 256 pixels
struct GcPlan {
    int cb;          // channels per block
    int nblk;        // blocks per group
    int units, splits;
    int jc;          // grad_input: output channels of the group per LDS chunk
};

inline int gc_block(int chans) { return chans > 8 ? 16 : (chans > 4 ? 8 : 4); }

GcPlan gc_plan(const GcGeom& g, int chans_g, int64_t npix, int other_g) {
    GcPlan pl{};
    pl.cb = gc_block(chans_g);
    pl.nblk = (chans_g + pl.cb - 1) / pl.cb;
    pl.units = (int)((npix + DW_THREADS - 1) / DW_THREADS);
    const int64_t blocks = (int64_t)g.G * pl.nblk;
    int64_t s = (GC_TARGET_STREAM + blocks - 1) / blocks;
    if (s > pl.units) s = pl.units;
    pl.splits = (int)(s < 1 ? 1 : s);
    int jc = GC_LDS_FLOATS / (pl.cb * g.kh * g.kw);
    pl.jc = jc > other_g ? other_g : jc;
    return pl;
}

// XT: element type of x and y, WT: of w (dw_map.h: float, DwBf16, DwF16); LDS weights, accumulators and the bias are fp32 for all
template <int KH, int KW, int CB, typename XT = float, typename WT = float>
__global__ __launch_bounds__(DW_THREADS) void gc_forward_kernel(const XT* __restrict__ x, const WT* __restrict__ w,
                                                                const float* __restrict__ bias, XT* __restrict__ y, GcGeom g,
                                                                DwStrides xs, DwStrides ys, GcPlan pl, int kind) {
    constexpr bool GEN = KH == 0;
    extern __shared__ float wl[];                                 // [K][CB]
    const int taps = GEN ? g.kh * g.kw : KH * KW;
    const int K = g.cin_g * taps;
    const int tid = threadIdx.x;
    const int blk = (int)(blockIdx.x / pl.splits);
    const int split = (int)(blockIdx.x - (unsigned)blk * pl.splits);
    const int grp = blk / pl.nblk;
    const int j0 = (blk - grp * pl.nblk) * CB;
    const int live = g.cout_g - j0 < CB ? g.cout_g - j0 : CB;
    const int64_t co0 = (int64_t)grp * g.cout_g + j0;
    for (int e = tid; e < CB * K; e += DW_THREADS) {
        const int j = e / K, k = e - j * K;
        wl[k * CB + j] = j < live ? dw_quant(kind, dw_ld(w[(co0 + j) * K + k])) : 0.0f;
    }
    __syncthreads();
    const int hw = g.Ho * g.Wo;
    const int64_t npix = (int64_t)g.N * hw;
    for (int u = split; u < pl.units; u += pl.splits) {
        const int64_t pix = (int64_t)u * DW_THREADS + tid;
        if (pix >= npix) continue;
        const int p = (int)pix;
        const int n = p / hw;
        const int r = p - n * hw;
        const int ho = r / g.Wo, wo = r - ho * g.Wo;
        const XT* xp = x + n * xs.n + (int64_t)grp * g.cin_g * xs.c;
        const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
        float acc[CB];
#pragma unroll
        for (int j = 0; j < CB; ++j) acc[j] = 0.0f;
        if (!GEN) {
            // no branch per tap: the loads of a channel go out together (a tap outside the image reads element 0 of the plane
            // instead) and a term outside the image is added as +0, which leaves the accumulator's bits as they are (it starts
            // at +0 and a sum is -0 only when both terms are, so it never holds -0)
            constexpr int T = GEN ? 1 : KH * KW;
            int off[T];
            bool ok[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int i = t / (GEN ? 1 : KW), jj = t - i * (GEN ? 1 : KW);
                const int hi = h0 + i * g.dh, wi = w0 + jj * g.dw;
                ok[t] = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                off[t] = ok[t] ? (int)(hi * xs.h + wi * xs.w) : 0;
            }
            constexpr int UNROLL = T == 1 ? 8 : 2;               // channels whose loads are in flight together
#pragma unroll UNROLL
            for (int ci = 0; ci < g.cin_g; ++ci) {
                const XT* xc = xp + ci * xs.c;
                const float* wk = wl + ci * T * CB;
                XT raw[T];
                float v[T];
#pragma unroll
                for (int t = 0; t < T; ++t) raw[t] = xc[off[t]];
                dw_loads_issued<XT, T>();
#pragma unroll
                for (int t = 0; t < T; ++t) v[t] = dw_ld(raw[t]);
#pragma unroll
                for (int t = 0; t < T; ++t) {
#pragma unroll
                    for (int j = 0; j < CB; ++j) {
                        const float p = v[t] * wk[t * CB + j];
                        acc[j] = acc[j] + (ok[t] ? p : 0.0f);
                    }
                }
            }
        } else {
            for (int ci = 0; ci < g.cin_g; ++ci) {
                const XT* xc = xp + ci * xs.c;
                const float* wk = wl + ci * taps * CB;
                for (int i = 0; i < g.kh; ++i) {
                    const int hi = h0 + i * g.dh;
                    if (hi < 0 || hi >= g.H) continue;
                    for (int jj = 0; jj < g.kw; ++jj) {
                        const int wi = w0 + jj * g.dw;
                        if (wi < 0 || wi >= g.W) continue;
                        const float v = dw_ld(xc[hi * xs.h + wi * xs.w]);
                        const float* wt = wk + (i * g.kw + jj) * CB;
#pragma unroll
                        for (int j = 0; j < CB; ++j) acc[j] = acc[j] + v * wt[j];
                    }
                }
            }
        }
        XT* yp = y + n * ys.n + co0 * ys.c + ho * ys.h + wo * ys.w;
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            if (j < live) {
                if (bias) acc[j] = acc[j] + bias[co0 + j];
                dw_st(&yp[j * ys.c], acc[j]);
            }
        }
    }
}

// gather form: gx[n, g cin_g + ci, h, w] = sum over j < cout_g (outermost), taps (i, j') row-major of
// go[n, g cout_g + j, ho, wo] Q(w)[g cout_g + j, ci, i, j'] where ho sh = h + ph - i dh and wo sw = w + pw - j' dw have a solution
// inside the output
template <int KH, int KW, int CB, typename XT = float, typename WT = float>
__global__ __launch_bounds__(DW_THREADS) void gc_grad_input_kernel(const XT* __restrict__ go, const WT* __restrict__ w,
                                                                   XT* __restrict__ gx, GcGeom g, DwStrides gs, DwStrides xs,
                                                                   GcPlan pl, int kind) {
    constexpr bool GEN = KH == 0;
    extern __shared__ float wl[];                                 // [jc][taps][CB]
    const int taps = GEN ? g.kh * g.kw : KH * KW;
    const int tid = threadIdx.x;
    const int blk = (int)(blockIdx.x / pl.splits);
    const int split = (int)(blockIdx.x - (unsigned)blk * pl.splits);
    const int grp = blk / pl.nblk;
    const int c0 = (blk - grp * pl.nblk) * CB;
    const int live = g.cin_g - c0 < CB ? g.cin_g - c0 : CB;
    const int64_t ci0 = (int64_t)grp * g.cin_g + c0;
    const int64_t cog = (int64_t)grp * g.cout_g;
    const bool once = pl.jc >= g.cout_g;                          // the whole group's weights fit: staged once per workgroup
    const int per = CB * taps;
    auto stage = [&](int jb) {
        for (int e = tid; e < pl.jc * per; e += DW_THREADS) {
            const int jj = e / per, r = e - jj * per;
            const int c = r / taps, t = r - c * taps;
            const bool in = jb + jj < g.cout_g && c < live;
            wl[(jj * taps + t) * CB + c] = in ? dw_quant(kind, dw_ld(w[((cog + jb + jj) * g.cin_g + c0 + c) * taps + t])) : 0.0f;
        }
    };
    if (once) {
        stage(0);
        __syncthreads();
    }
    const int hw = g.H * g.W;
    const int64_t npix = (int64_t)g.N * hw;
    for (int u = split; u < pl.units; u += pl.splits) {           // uniform over the workgroup: the barriers below are too
        const int64_t pix = (int64_t)u * DW_THREADS + tid;
        const bool in = pix < npix;
        const int p = in ? (int)pix : 0;
        const int n = p / hw;
        const int r = p - n * hw;
        const int h = r / g.W, x0 = r - h * g.W;
        constexpr int T = GEN ? 1 : KH * KW;
        int off[T];
        bool ok[T];
        if (!GEN) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int i = t / (GEN ? 1 : KW), jj = t - i * (GEN ? 1 : KW);
                const int hh = h + g.ph - i * g.dh, ww = x0 + g.pw - jj * g.dw;
                const int ho = g.sh == 1 ? hh : hh / g.sh, wo = g.sw == 1 ? ww : ww / g.sw;
                ok[t] = in && hh >= 0 && ww >= 0 && ho * g.sh == hh && wo * g.sw == ww && ho < g.Ho && wo < g.Wo;
                off[t] = ok[t] ? (int)(ho * gs.h + wo * gs.w) : 0;
            }
        }
        float acc[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[c] = 0.0f;
        for (int jb = 0; jb < g.cout_g; jb += pl.jc) {
            if (!once) {
                __syncthreads();
                stage(jb);
                __syncthreads();
            }
            if (!in) continue;
            const int jn = g.cout_g - jb < pl.jc ? g.cout_g - jb : pl.jc;
            constexpr int UNROLL = GEN ? 1 : (KH * KW == 1 ? 8 : 2);
#pragma unroll UNROLL
            for (int jj = 0; jj < jn; ++jj) {
                const XT* gp = go + n * gs.n + (cog + jb + jj) * gs.c;
                const float* wk = wl + jj * per;
                if (!GEN) {                           // branch-free, as in the forward
                    XT raw[T];
                    float v[T];
#pragma unroll
                    for (int t = 0; t < T; ++t) raw[t] = gp[off[t]];
                    dw_loads_issued<XT, T>();
#pragma unroll
                    for (int t = 0; t < T; ++t) v[t] = dw_ld(raw[t]);
#pragma unroll
                    for (int t = 0; t < T; ++t) {
#pragma unroll
                        for (int c = 0; c < CB; ++c) {
                            const float p = v[t] * wk[t * CB + c];
                            acc[c] = acc[c] + (ok[t] ? p : 0.0f);
                        }
                    }
                } else {
                    for (int i = 0; i < g.kh; ++i) {
                        const int hh = h + g.ph - i * g.dh;
                        if (hh < 0) continue;
                        const int ho = hh / g.sh;
                        if (ho * g.sh != hh || ho >= g.Ho) continue;
                        for (int t2 = 0; t2 < g.kw; ++t2) {
                            const int ww = x0 + g.pw - t2 * g.dw;
                            if (ww < 0) continue;
                            const int wo = ww / g.sw;
                            if (wo * g.sw != ww || wo >= g.Wo) continue;
                            const float v = dw_ld(gp[ho * gs.h + wo * gs.w]);
                            const float* wt = wk + (i * g.kw + t2) * CB;
#pragma unroll
                            for (int c = 0; c < CB; ++c) acc[c] = acc[c] + v * wt[c];
                        }
                    }
                }
            }
        }
        if (in) {
            XT* xp = gx + n * xs.n + ci0 * xs.c + h * xs.h + x0 * xs.w;
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < live) dw_st(&xp[c * xs.c], acc[c]);
        }
    }
}

// stage 1 of grad_weight for any kernel of up to 49 taps, over the virtual channels v = co * cin_g + ci: work[(split * Cv + v) * (kk + 1) + t] = this workgroup's
// share of sum go[., co] * x[., g cin_g + ci] for tap t, and of sum go[., co] for t == kk
template <typename XT = float>
__global__ __launch_bounds__(DW_THREADS) void gc_grad_weight_kernel(const XT* __restrict__ go, const XT* __restrict__ x,
                                                                    float* __restrict__ work, GcGeom g, DwStrides gs, DwStrides xs,
                                                                    DwMap mp) {
    constexpr int CAP = GC_MAX_TAPS;
    __shared__ float red[(CAP + 1) * DW_THREADS];
    const int tid = threadIdx.x;
    const int64_t cg = blockIdx.x / mp.splits;
    const int split = (int)(blockIdx.x - cg * mp.splits);
    const int64_t v = cg * mp.slots + dw_slot(mp, tid);
    const bool live = v < mp.chans;
    const int kw = g.kw, kk = g.kh * g.kw;
    const int64_t co = live ? v / g.cin_g : 0;
    const int64_t c = live ? (co / g.cout_g) * g.cin_g + (v - co * g.cin_g) : 0;
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
                if (t < kk) {
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
        float s = acc[t];
        for (int off = lo; off < hi; off <<= 1) s = s + __shfl_xor(s, off, 64);
        red[t * DW_THREADS + tid] = s;
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
        const int64_t ov = cg * mp.slots + q;
        if (ov < mp.chans) work[((int64_t)split * mp.chans + ov) * per + t] = s;
    }
}

// stage 1 of grad_weight for the compile-time kernels (1 x 1, 3 x 3), register-tiled: a lane owns one output pixel and the
// COB x CIB x taps partial sums of a block of COB output and CIB input channels of one group, so the COB gradient values and the
// CIB x taps inputs it loads feed COB x CIB x taps multiply-adds (4 + 36 loads for 144 at 3 x 3).  A workgroup is (group, output
// block, input block, split) and walks pixels split * 256 + tid, (split + S) * 256 + tid, ...; at the end a butterfly over the 64
// lanes, then the four waves in index order through LDS.  Same workspace layout as the kernel above; the bias partial of an
// output channel comes from the workgroup of input block 0.  Branch-free like the forward: a term outside the image adds +0.
struct GcTilePlan {
    int nco, nci;        // output / input channel blocks per group
    int units, splits;
};

template <int KH, int KW, int COB, int CIB, typename XT = float>
__global__ __launch_bounds__(DW_THREADS) void gc_grad_weight_tile_kernel(const XT* __restrict__ go, const XT* __restrict__ x,
                                                                         float* __restrict__ work, GcGeom g, DwStrides gs,
                                                                         DwStrides xs, GcTilePlan tp) {
    constexpr int T = KH * KW, A = COB * CIB * T, R = A + COB;
    __shared__ float red[DW_THREADS / 64][R];
    const int tid = threadIdx.x;
    const int blk = (int)(blockIdx.x / tp.splits);
    const int split = (int)(blockIdx.x - (unsigned)blk * tp.splits);
    const int per_g = tp.nco * tp.nci;
    const int grp = blk / per_g;
    const int rb = blk - grp * per_g;
    const int jb = rb / tp.nci, cb = rb - jb * tp.nci;
    const int j0 = jb * COB, c0 = cb * CIB;
    const int live_j = g.cout_g - j0 < COB ? g.cout_g - j0 : COB;
    const int live_c = g.cin_g - c0 < CIB ? g.cin_g - c0 : CIB;
    const int64_t co0 = (int64_t)grp * g.cout_g + j0, ci0 = (int64_t)grp * g.cin_g + c0;
    float acc[A], gsum[COB];
#pragma unroll
    for (int a = 0; a < A; ++a) acc[a] = 0.0f;
#pragma unroll
    for (int j = 0; j < COB; ++j) gsum[j] = 0.0f;
    const int hw = g.Ho * g.Wo;
    const int64_t npix = (int64_t)g.N * hw;
    for (int u = split; u < tp.units; u += tp.splits) {
        const int64_t pix = (int64_t)u * DW_THREADS + tid;
        if (pix >= npix) continue;
        const int p = (int)pix;
        const int n = p / hw;
        const int r = p - n * hw;
        const int ho = r / g.Wo, wo = r - ho * g.Wo;
        const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
        int off[T];
        bool ok[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int i = t / KW, jj = t - i * KW;
            const int hi = h0 + i * g.dh, wi = w0 + jj * g.dw;
            ok[t] = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
            off[t] = ok[t] ? (int)(hi * xs.h + wi * xs.w) : 0;
        }
        const XT* gp = go + n * gs.n + co0 * gs.c + ho * gs.h + wo * gs.w;
        float gv[COB];
#pragma unroll
        for (int j = 0; j < COB; ++j) {
            gv[j] = j < live_j ? dw_ld(gp[j * gs.c]) : 0.0f;
            gsum[j] = gsum[j] + gv[j];
        }
        const XT* xp = x + n * xs.n + ci0 * xs.c;
#pragma unroll
        for (int c = 0; c < CIB; ++c) {
            if (c < live_c) {                                     // uniform over the workgroup
                XT raw[T];
                float xv[T];
#pragma unroll
                for (int t = 0; t < T; ++t) raw[t] = xp[c * xs.c + off[t]];
                dw_loads_issued<XT, T>();
#pragma unroll
                for (int t = 0; t < T; ++t) xv[t] = dw_ld(raw[t]);
#pragma unroll
                for (int t = 0; t < T; ++t) {
#pragma unroll
                    for (int j = 0; j < COB; ++j) {
                        const float pr = gv[j] * xv[t];
                        acc[(j * CIB + c) * T + t] = acc[(j * CIB + c) * T + t] + (ok[t] ? pr : 0.0f);
                    }
                }
            }
        }
    }
    const int wave = tid >> 6;
#pragma unroll
    for (int a = 0; a < R; ++a) {
        float v = a < A ? acc[a < A ? a : 0] : gsum[a < A ? 0 : a - A];
        for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
        if ((tid & 63) == 0) red[wave][a] = v;
    }
    __syncthreads();
    const int64_t Cv = g.Cout * g.cin_g;
    for (int e = tid; e < R; e += DW_THREADS) {
        float sum = red[0][e];
        for (int wv = 1; wv < DW_THREADS / 64; ++wv) sum = sum + red[wv][e];
        if (e < A) {
            const int j = e / (CIB * T), r = e - j * CIB * T;
            const int c = r / T, t = r - c * T;
            if (j < live_j && c < live_c) work[((int64_t)split * Cv + (co0 + j) * g.cin_g + c0 + c) * (T + 1) + t] = sum;
        } else {
            const int j = e - A;
            if (j < live_j && cb == 0) work[((int64_t)split * Cv + (co0 + j) * g.cin_g) * (T + 1) + T] = sum;
        }
    }
}

template <int COB, int CIB>
GcTilePlan gc_tile_plan(const GcGeom& g) {
    GcTilePlan tp{};
    tp.nco = (g.cout_g + COB - 1) / COB;
    tp.nci = (g.cin_g + CIB - 1) / CIB;
    tp.units = (int)(((int64_t)g.N * g.Ho * g.Wo + DW_THREADS - 1) / DW_THREADS);
    const int64_t blocks = (int64_t)g.G * tp.nco * tp.nci;
    int64_t s = (GC_TARGET_REDUCE + blocks - 1) / blocks;
    if (s > tp.units) s = tp.units;
    tp.splits = (int)(s < 1 ? 1 : s);
    return tp;
}

// register blocks of the tiled stage 1: 144 partial sums per lane at 3 x 3, 64 at 1 x 1
constexpr int GC_T3_COB = 4, GC_T3_CIB = 4, GC_T1_COB = 8, GC_T1_CIB = 8;

// stage 2: the splits in index order, the STE mask on the unquantised weight, the bias gradient from the ci == 0 channel;
// WT: element type of w, gw and gbias
template <typename WT = float>
__global__ __launch_bounds__(DW_THREADS) void gc_grad_weight_combine_kernel(const float* __restrict__ work, const WT* __restrict__ w,
                                                                            WT* __restrict__ gw, WT* __restrict__ gbias,
                                                                            int64_t Cv, int cin_g, int kk, int splits, float thr) {
    const int per = kk + 1;
    const int64_t total = Cv * per;
    for (int64_t e = (int64_t)blockIdx.x * DW_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * DW_THREADS) {
        const int64_t v = e / per;
        const int t = (int)(e - v * per);
        if (t == kk && (!gbias || v % cin_g != 0)) continue;
        float s = 0.0f;
        for (int sp = 0; sp < splits; ++sp) s = s + work[((int64_t)sp * Cv + v) * per + t];
        if (t < kk) {
            if (thr > 0.0f && fabsf(dw_ld(w[v * kk + t])) > thr) s = 0.0f;
            dw_st(&gw[v * kk + t], s);
        } else {
            dw_st(&gbias[v / cin_g], s);
        }
    }
}

// validates the shape arguments and fills g; QT_OK with *empty set when there is nothing to compute
int gc_geometry(int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                int pw, int dh, int dw, GcGeom* g, bool* empty) {
    *empty = false;
    if (N < 0 || G < 0 || cin_g < 1 || cout_g < 1 || H < 0 || W < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 ||
        dh < 1 || dw < 1)
        return QT_ERR_INVALID_ARG;
    if ((int64_t)kh * kw > GC_MAX_TAPS) return QT_ERR_UNSUPPORTED;
    if (N == 0 || G == 0 || H == 0 || W == 0) {
        *empty = true;
        return QT_OK;
    }
    if (cin_g > GC_MAX_CIN_G || cin_g * kh * kw > GC_MAX_K) return QT_ERR_UNSUPPORTED;
    if (N >= GC_MAX_ELEMS || G >= GC_MAX_ELEMS || H >= GC_MAX_ELEMS || W >= GC_MAX_ELEMS || cout_g >= GC_MAX_ELEMS || ph >= (1 << 24) ||
        pw >= (1 << 24) || dh >= (1 << 24) || dw >= (1 << 24))
        return QT_ERR_UNSUPPORTED;
    if (H + 2 * (int64_t)ph >= GC_MAX_ELEMS || W + 2 * (int64_t)pw >= GC_MAX_ELEMS) return QT_ERR_UNSUPPORTED;     // tap coordinates are int
    const int64_t eh = H + 2 * (int64_t)ph - (int64_t)dh * (kh - 1) - 1, ew = W + 2 * (int64_t)pw - (int64_t)dw * (kw - 1) - 1;
    if (eh < 0 || ew < 0) return QT_ERR_INVALID_ARG;          // the kernel does not fit the padded image
    const int64_t Ho = eh / sh + 1, Wo = ew / sw + 1;
    const double cin = (double)G * (double)cin_g, cout = (double)G * (double)cout_g;
    if ((double)N * cin * (double)H * (double)W >= (double)GC_MAX_ELEMS || (double)N * cout * (double)Ho * (double)Wo >= (double)GC_MAX_ELEMS ||
        cout > (double)GC_MAX_CHANNELS)
        return QT_ERR_UNSUPPORTED;
    g->N = (int)N; g->G = (int)G; g->cin_g = (int)cin_g; g->cout_g = (int)cout_g; g->H = (int)H; g->W = (int)W; g->Ho = (int)Ho; g->Wo = (int)Wo;
    g->kh = kh; g->kw = kw; g->sh = sh; g->sw = sw; g->ph = ph; g->pw = pw; g->dh = dh; g->dw = dw;
    g->Cin = G * cin_g;
    g->Cout = G * cout_g;
    return QT_OK;
}

bool gc_kind_ok(int kind) { return kind == QT_DW_RAW || kind == QT_DW_SIGN || kind == QT_DW_TERNARY; }

// TA, TB: the two element types of the kernel template
#define GC_LAUNCH_CB(KERNEL, KH, KW, TA, TB, pl, ...)                                              \
    do {                                                                                           \
        if ((pl).cb == 16) KERNEL<KH, KW, 16, TA, TB><<<grid, DW_THREADS, lds, s>>>(__VA_ARGS__);  \
        else if ((pl).cb == 8) KERNEL<KH, KW, 8, TA, TB><<<grid, DW_THREADS, lds, s>>>(__VA_ARGS__); \
        else KERNEL<KH, KW, 4, TA, TB><<<grid, DW_THREADS, lds, s>>>(__VA_ARGS__);                 \
    } while (0)

#define GC_DISPATCH(KERNEL, TA, TB, g, pl, ...)                                                    \
    do {                                                                                           \
        if ((g).kh == 1 && (g).kw == 1) GC_LAUNCH_CB(KERNEL, 1, 1, TA, TB, pl, __VA_ARGS__);       \
        else if ((g).kh == 3 && (g).kw == 3) GC_LAUNCH_CB(KERNEL, 3, 3, TA, TB, pl, __VA_ARGS__);  \
        else GC_LAUNCH_CB(KERNEL, 0, 0, TA, TB, pl, __VA_ARGS__);                                  \
    } while (0)

// ---- the forward on / into bit planes (include/qt_hip.h "Grouped convolution on bit planes") ---------------------------------------
// The input is the NHWC sign plane of a +-1 activation and every tap is classified to -1 / 0 / +1, so the cin_g operands of a group
// at one tap are a cin_g-bit FIELD of one plane word (cin_g in {2, 4, 8}: a field never straddles a word) and the group's dot
// product at that tap is  popc(nz) - 2 popc((field ^ neg) & nz)  with the tap's masks nz (weight != 0) and neg (weight < 0): one
// XOR, one AND and a popcount instead of cin_g multiply-adds.  The sum S over the taps inside the image is an integer of magnitude
// <= 8 * 49, so (float)S is what any order of fp32 additions of the +-1 products gives, and fl((float)S + bias) has the bits
// qt_gconv2d_f32 stores for the decoded image.
// The map is that of dw_planes_kernel: a HALF-wave owns one 32-channel output word of one pixel, a workgroup (plane word, split)
// walks 8 pixels per step, so a lane keeps ONE output channel for the whole launch — its (neg, nz) masks of all taps (two taps per
// register: at most 25), bias, alpha and beta.  Lane co reads input word (g cin_g) >> 5 at shift (g cin_g) & 31, g = co / cout_g.
// The 1 x 1 and 3 x 3 forms are branch-free: all tap loads go out together, a tap outside the image loads the nearest pixel inside
// and contributes through a select on its nz mask; dead lanes and pixels past the end compute on pixel 0 and are not stored.  The
// writing stage is dw_planes.h.  (Tried: a whole wave per pixel, so that the tap coordinates and row addresses run on the scalar
// unit — slower at every measured shape, DESIGN.md "Grouped convs", "Tried".)

template <int KH, int KW>
__global__ __launch_bounds__(DW_THREADS) void gc_planes_kernel(const uint32_t* __restrict__ xb, int64_t ldx, const float* __restrict__ w,
                                                               const float* __restrict__ bias, const float* __restrict__ alpha,
                                                               const float* __restrict__ beta, DwPlaneOut o, DwGeom g, int cin_g,
                                                               int cout_g, DwStrides ys, int units, int splits, int d_n, int d_ho, int d_wo,
                                                               int kind) {
    constexpr bool GEN = KH == 0;
    constexpr int CAP = GEN ? GC_MAX_TAPS : KH * KW;
    const int tid = threadIdx.x, lane = tid & 31;
    const int wd = (int)(blockIdx.x / splits);
    const int split = (int)(blockIdx.x - (unsigned)wd * splits);
    const int64_t co = (int64_t)wd * 32 + lane;
    const bool live = co < g.Cout;
    const int kw = GEN ? g.kw : KW, kk = GEN ? g.kh * g.kw : KH * KW;
    // tap t: nz in bits 0 .. 7 and neg in bits 8 .. 15 of half (t & 1) of pk[t >> 1]
    uint32_t pk[(CAP + 1) / 2];
#pragma unroll
    for (int r = 0; r < (CAP + 1) / 2; ++r) pk[r] = 0u;
    if (live) {
        for (int ci = 0; ci < cin_g; ++ci) {
            const float* wp = w + (co * cin_g + ci) * kk;
            float wv[CAP];                                       // the loads of a channel go out together, then the (branching) quantiser
#pragma unroll
            for (int t = 0; t < CAP; ++t) wv[t] = (!GEN || t < kk) ? wp[t] : 0.0f;
#pragma unroll
            for (int t = 0; t < CAP; ++t) {
                if (!GEN || t < kk) {
                    const float q = dw_quant(kind, wv[t]);
                    const uint32_t cls = ((q > 0.0f || q < 0.0f) ? 1u : 0u) | (q < 0.0f ? 0x100u : 0u);
                    pk[t >> 1] |= cls << (ci + 16 * (t & 1));
                }
            }
        }
    }
    const float b = (live && bias) ? bias[co] : 0.0f;
    const float al = (live && alpha) ? alpha[co] : 0.0f, be = (live && beta) ? beta[co] : 0.0f;
    const int c0 = live ? (int)(co / cout_g) * cin_g : 0;          // first input channel of the lane's group
    const int xw = c0 >> 5, xsh = c0 & 31;
    const int hw = g.Ho * g.Wo;
    const int64_t npix = (int64_t)g.N * hw;
    // the first pixel of this half-wave is divided out once; a step advances it by splits * 8 pixels = (d_n, d_ho, d_wo) images,
    // rows and columns with two carries (the walk of dw_codes_kernel): no division per output
    int64_t next = (int64_t)split * DW_PIX_PER_STEP + (tid >> 5);
    int rn = 0, rho = 0, rwo = 0;
    if (next < npix) {
        const int p = (int)next;
        rn = p / hw;
        const int r = p - rn * hw;
        rho = r / g.Wo;
        rwo = r - rho * g.Wo;
    }
    for (int u = split; u < units; u += splits) {
        const int64_t pix = next;
        const bool in = pix < npix;
        const int n = in ? rn : 0, ho = in ? rho : 0, wo = in ? rwo : 0;
        next += (int64_t)splits * DW_PIX_PER_STEP;
        rwo += d_wo;
        const int c1 = rwo >= g.Wo;
        rwo -= c1 ? g.Wo : 0;
        rho += d_ho + c1;
        const int c2 = rho >= g.Ho;
        rho -= c2 ? g.Ho : 0;
        rn += d_n + c2;
        const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
        const uint32_t* xn = xb + (int64_t)n * g.H * g.W * ldx + xw;
        int S = 0;
        if (!GEN) {
            uint32_t word[CAP];
            bool ok[CAP];
#pragma unroll
            for (int t = 0; t < CAP; ++t) {
                const int i = t / (GEN ? 1 : KW), j = t - i * (GEN ? 1 : KW);
                const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                ok[t] = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                const int hc = hi < 0 ? 0 : (hi >= g.H ? g.H - 1 : hi), wc = wi < 0 ? 0 : (wi >= g.W ? g.W - 1 : wi);
                word[t] = xn[((int64_t)hc * g.W + wc) * ldx];
            }
#pragma unroll
            for (int t = 0; t < CAP; ++t) {
                const uint32_t m = pk[t >> 1] >> (16 * (t & 1));
                const uint32_t nz = ok[t] ? (m & 0xFFu) : 0u;
                S += __popc(nz) - 2 * __popc(((word[t] >> xsh) ^ (m >> 8)) & nz);
            }
        } else {
            int i = 0, j = 0;
#pragma unroll
            for (int t = 0; t < CAP; ++t) {
                if (t < kk) {
                    const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                    const bool ok = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                    const int hc = hi < 0 ? 0 : (hi >= g.H ? g.H - 1 : hi), wc = wi < 0 ? 0 : (wi >= g.W ? g.W - 1 : wi);
                    const uint32_t word = xn[((int64_t)hc * g.W + wc) * ldx];
                    const uint32_t m = pk[t >> 1] >> (16 * (t & 1));
                    const uint32_t nz = ok ? (m & 0xFFu) : 0u;
                    S += __popc(nz) - 2 * __popc(((word >> xsh) ^ (m >> 8)) & nz);
                    if (++j == kw) { j = 0; ++i; }
                }
            }
        }
        float acc = (float)S;
        if (bias) acc = acc + b;
        if (o.y) {                                   // uniform over the launch
            if (in && live) o.y[n * ys.n + co * ys.c + ho * ys.h + wo * ys.w] = acc;
            continue;
        }
        // two roundings (the build has -ffp-contract=off), as in dw_planes_kernel; dead lanes vote 0
        const int neg = (in && live) ? (int)qt_neg_bit(acc * al + be) : 0;
        const unsigned long long votes = __ballot(neg);
        if (lane != 0 || !in) continue;
        dw_store_word(o, g, wd, pix, n, ho, wo, (uint32_t)(votes >> (tid & 32)));
    }
    if (!o.y) dw_zero_border(o, g, tid);
}

// the shared body of the two plane entries: o.y, or at least one of o.sign / o.nib
int gc_planes_launch(const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, const float* alpha, const float* beta,
                     DwPlaneOut o, bool f32, int64_t halo_h, int64_t halo_w, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
                     int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, DwStrides ys, int kind,
                     qt_stream_t stream) {
    GcGeom gg{};
    bool empty;
    if (halo_h < 0 || halo_w < 0) return QT_ERR_INVALID_ARG;
    const int rc = gc_geometry(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &gg, &empty);
    if (rc != QT_OK) return rc;
    if (cin_g != 2 && cin_g != 4 && cin_g != 8) return QT_ERR_UNSUPPORTED;      // a group's field must not straddle a plane word
    if (empty) return QT_OK;
    if (halo_h > DW_MAX_HALO || halo_w > DW_MAX_HALO) return QT_ERR_UNSUPPORTED;
    if (o.nib && (double)N * (double)(gg.Ho + 2 * halo_h) * (double)(gg.Wo + 2 * halo_w) >= (double)GC_MAX_ELEMS) return QT_ERR_UNSUPPORTED;
    if (!gc_kind_ok(kind)) return QT_ERR_INVALID_ARG;
    if (!x_plane || !w) return QT_ERR_INVALID_ARG;
    if (f32) {
        if (!o.y || dw_layout(N, gg.Cout, gg.Ho, gg.Wo, ys) < 0) return QT_ERR_INVALID_ARG;
    } else {
        if ((!o.sign && !o.nib) || !alpha || !beta) return QT_ERR_INVALID_ARG;
        if (o.sign && o.ldb < dw_packed_ld(gg.Cout)) return QT_ERR_INVALID_ARG;
        if (o.nib && o.ldn < dw_pixel_ld_nib(gg.Cout)) return QT_ERR_INVALID_ARG;
    }
    if (ldx < dw_packed_ld(gg.Cin)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(x_plane) || !dw_aligned4(w) || !dw_aligned4(bias) || !dw_aligned4(alpha) || !dw_aligned4(beta) || !dw_aligned4(o.y) ||
        !dw_aligned4(o.sign))
        return QT_ERR_ALIGNMENT;
    if (o.nib && ((o.ldn & 3) || !dw_aligned16(o.nib))) return QT_ERR_ALIGNMENT;
    o.hy = (int)halo_h;
    o.hx = (int)halo_w;
    DwGeom g{};                                     // the record the writing stage reads; m is not used
    g.N = gg.N; g.C = (int)gg.Cin; g.H = gg.H; g.W = gg.W; g.Ho = gg.Ho; g.Wo = gg.Wo;
    g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw; g.dh = dh; g.dw = dw;
    g.Cout = gg.Cout;
    const int64_t npix = (int64_t)g.N * g.Ho * g.Wo;
    const int64_t nw = (g.Cout + 31) / 32;
    const int units = (int)((npix + DW_PIX_PER_STEP - 1) / DW_PIX_PER_STEP);
    int64_t sp = (GC_TARGET_STREAM + nw - 1) / nw;
    if (sp > units) sp = units;
    const int splits = (int)(sp < 1 ? 1 : sp);
    const unsigned grid = (unsigned)(nw * splits);
    const int64_t step = (int64_t)splits * DW_PIX_PER_STEP;
    const int d_wo = (int)(step % g.Wo), d_ho = (int)((step / g.Wo) % g.Ho), d_n = (int)(step / g.Wo / g.Ho);
    hipStream_t s = (hipStream_t)stream;
#define GC_PLANES_ARGS x_plane, ldx, w, bias, alpha, beta, o, g, gg.cin_g, gg.cout_g, ys, units, splits, d_n, d_ho, d_wo, kind
    if (kh == 1 && kw == 1) gc_planes_kernel<1, 1><<<grid, DW_THREADS, 0, s>>>(GC_PLANES_ARGS);
    else if (kh == 3 && kw == 3) gc_planes_kernel<3, 3><<<grid, DW_THREADS, 0, s>>>(GC_PLANES_ARGS);
    else gc_planes_kernel<0, 0><<<grid, DW_THREADS, 0, s>>>(GC_PLANES_ARGS);
#undef GC_PLANES_ARGS
    return qt_check_launch();
}

// ---- the forward on / into int8 code planes (include/qt_hip.h "Grouped convolution on int8 code planes") ----------------------------
// gc_codes_kernel: the thread map of dw_codes_kernel (dwconv.hip) — a lane owns ONE DWORD of output channels (4 codes) for the whole
// launch, the lanes of a workgroup run along the dwords of a pixel row first (`lanes`, a power of two), then along 256 / lanes
// consecutive output pixels; a workgroup is (dword group, split) and walks pixel steps split, split + S, ... with constant
// increments and two carries.  What differs is the inner product: cin_g x taps terms per output instead of taps.
//   weights : 4 x K per lane (K = cin_g taps) do not fit registers beyond 1 x 1, so the workgroup stages the weights of its `lanes`
//             dwords once into LDS as wl[k][lane] float4 (k = ci * taps + t, the weight's own order): lanes on consecutive dwords
//             read consecutive 16 bytes, lanes on other pixels the same address (a broadcast).  The host caps `lanes` at 2048 / K,
//             so the block is at most 32 KiB whatever K <= 512 is.  The 1 x 1 forms keep their 4 x cin_g weights in registers.
//   forms   : CING in {2, 4, 8} with cout_g % 4 == 0 and a 1 x 1 or 3 x 3 kernel are compile-time forms: the lane's four channels
//             share one group, whose cin_g input bytes of a tap are ONE aligned 2- / 4- / 8-byte load at byte g cin_g of the pixel
//             row; all tap loads go out together (a tap outside the image loads the nearest pixel inside it, never the halo) and a
//             term outside the image is added as +0 — a select on the product, which leaves the accumulator's bits as they are (it
//             never holds -0, see gc_forward_kernel).  Everything else (CING == 0) is the generic form: per channel of the dword,
//             per input channel, per tap one byte load under a branch; correct for a dword that straddles groups, not fast.
// The order of every output's sum is that of gc_forward_kernel: +0, input channel ascending (outermost), taps row-major, one fp32
// multiply then one fp32 add per term on x = fl(inv_n * (float)q), bias last.  The epilogue is affine_codes_word of
// codes_epilogue.h; dwords past G cout_g are written by lanes of their own as zero, the border of a halo plane by the same map.
struct GcCodesMap {
    int lanes_log;            // log2 of the lanes along the dwords of a pixel row
    int slots;                // dwords per output pixel row that are written: ldc / 4, or ceil(G cout_g / 4) for the fp32 form
    int units, splits;        // pixel steps of 256 >> lanes_log pixels, workgroups per dword group
    int d_n, d_ho, d_wo;      // splits * (256 >> lanes_log) pixels as (images, rows, columns)
    int ihy, ihx, ohy, ohx;   // halos of the input and the output plane
};

struct GcCodesEpi {
    const float* alpha;
    const float* beta;
    const float* bn_stats;
    int relu;
    float n;
    int8_t* codes;
    int64_t ldc;
    int32_t* overflow;
};

struct GcF32Out {
    float* y;
    DwStrides ys;
    const int32_t* overflow;
    int vec;                  // channels-last, G cout_g % 4 == 0, 16-byte aligned: one float4 store per lane
};

template <int KH, int KW, int CING, bool F32OUT>
__global__ __launch_bounds__(DW_THREADS) void gc_codes_kernel(const int8_t* __restrict__ x, int64_t ldx, float inv_n,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              GcCodesEpi ep, GcF32Out fo, GcGeom g, GcCodesMap mp) {
    constexpr bool GEN = CING == 0;
    constexpr int T = GEN ? 1 : KH * KW;
    constexpr bool REGW = !GEN && T == 1;                       // the weights stay in registers
    extern __shared__ float4 wl4[];                             // [K][lanes]
    const int tid = threadIdx.x;
    const int lanes = 1 << mp.lanes_log, tpix = DW_THREADS >> mp.lanes_log;
    const int sg = (int)(blockIdx.x / mp.splits);
    const int split = (int)(blockIdx.x - (unsigned)sg * mp.splits);
    const int ln = tid & (lanes - 1);
    const int slot = sg * lanes + ln;
    const int ps = tid >> mp.lanes_log;
    const bool row_lane = slot < mp.slots;                     // this lane writes a dword of every pixel row
    const int64_t co0 = (int64_t)slot * 4;
    const int nvalid = (int)(g.Cout - co0 < 0 ? 0 : (g.Cout - co0 > 4 ? 4 : g.Cout - co0));
    const int taps = GEN ? g.kh * g.kw : T;
    const int K = g.cin_g * taps;
    float4 wr[REGW ? CING : 1];
    if (REGW) {
#pragma unroll
        for (int ci = 0; ci < (REGW ? CING : 1); ++ci) {
            float we[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) we[e] = e < nvalid ? w[(co0 + e) * K + ci] : 0.0f;
            wr[ci] = make_float4(we[0], we[1], we[2], we[3]);
        }
    } else {
        float* wl = reinterpret_cast<float*>(wl4);
        const int64_t cb = (int64_t)sg * lanes * 4;             // first channel of this workgroup's dwords
        for (int e = tid; e < lanes * 4 * K; e += DW_THREADS) {
            const int j = e / K, k = e - j * K;
            wl[(k * lanes + (j >> 2)) * 4 + (j & 3)] = cb + j < g.Cout ? w[(cb + j) * K + k] : 0.0f;
        }
        __syncthreads();
    }
    float b[4];
    int cbase[4];                                               // first input channel of each channel's group
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool live = e < nvalid;
        b[e] = (live && bias) ? bias[co0 + e] : 0.0f;
        cbase[e] = live ? (int)((co0 + e) / g.cout_g) * g.cin_g : 0;
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
                if (!GEN) {
                    constexpr int NW = CING == 8 ? 2 : 1;
                    uint32_t raw[T][NW];
                    bool ok[T];
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const int i = t / (GEN ? 1 : KW), j = t - i * (GEN ? 1 : KW);
                        const int hi = h0 + i * g.dh, wi = w0 + j * g.dw;
                        ok[t] = hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
                        const int hc = hi < 0 ? 0 : (hi >= g.H ? g.H - 1 : hi), wc = wi < 0 ? 0 : (wi >= g.W ? g.W - 1 : wi);
                        const int8_t* px = x + (int64_t)((n * Hp + hc + mp.ihy) * Wp + wc + mp.ihx) * ldx + cbase[0];
                        if (CING == 8) {
                            const uint2 v2 = *reinterpret_cast<const uint2*>(px);
                            raw[t][0] = v2.x;
                            raw[t][NW - 1] = v2.y;
                        } else if (CING == 4) {
                            raw[t][0] = *reinterpret_cast<const uint32_t*>(px);
                        } else {
                            raw[t][0] = *reinterpret_cast<const uint16_t*>(px);
                        }
                    }
#pragma unroll
                    for (int ci = 0; ci < (GEN ? 1 : CING); ++ci) {
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            const float v = inv_n * (float)(int8_t)(raw[t][ci >> 2] >> (8 * (ci & 3)));
                            const float4 wv = REGW ? wr[REGW ? ci : 0] : wl4[(ci * T + t) * lanes + ln];
                            const float p0 = v * wv.x, p1 = v * wv.y, p2 = v * wv.z, p3 = v * wv.w;
                            acc[0] = acc[0] + (ok[t] ? p0 : 0.0f);
                            acc[1] = acc[1] + (ok[t] ? p1 : 0.0f);
                            acc[2] = acc[2] + (ok[t] ? p2 : 0.0f);
                            acc[3] = acc[3] + (ok[t] ? p3 : 0.0f);
                        }
                    }
                } else {
                    const float* wl = reinterpret_cast<const float*>(wl4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (e < nvalid) {
                            float a = 0.0f;
                            for (int ci = 0; ci < g.cin_g; ++ci) {
                                for (int i = 0; i < g.kh; ++i) {
                                    const int hi = h0 + i * g.dh;
                                    if (hi < 0 || hi >= g.H) continue;
                                    for (int j = 0; j < g.kw; ++j) {
                                        const int wi = w0 + j * g.dw;
                                        if (wi < 0 || wi >= g.W) continue;
                                        const int8_t q = x[(int64_t)((n * Hp + hi + mp.ihy) * Wp + wi + mp.ihx) * ldx + cbase[e] + ci];
                                        const float v = inv_n * (float)q;
                                        a = a + v * wl[(((ci * g.kh + i) * g.kw + j) * lanes + ln) * 4 + e];
                                    }
                                }
                            }
                            acc[e] = a;
                        }
                    }
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
        // the border pixels of the output plane, enumerated alone as in dw_codes_kernel: per image ohy rows on top, 2 ohx columns
        // beside each of the Ho image rows, ohy rows below; one dword per lane
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

inline int64_t gc_code_ld(int64_t K) { return std::max<int64_t>(16, (K + 15) / 16 * 16); }

// the shared body of the two code-plane entries: ep.codes (code plane out) or fo.y (fp32 out)
int gc_codes_launch(const int8_t* x_plane, int64_t ldx, int64_t ihy, int64_t ihx, float inv_n, const float* w, const float* bias,
                    GcCodesEpi ep, int bit_width, int64_t ohy, int64_t ohx, GcF32Out fo, int64_t N, int64_t G, int64_t cin_g,
                    int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, bool f32,
                    qt_stream_t stream) {
    GcGeom g{};
    bool empty;
    if (ihy < 0 || ihx < 0 || ohy < 0 || ohx < 0) return QT_ERR_INVALID_ARG;
    const int rc = gc_geometry(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (ihy > DW_MAX_HALO || ihx > DW_MAX_HALO || ohy > DW_MAX_HALO || ohx > DW_MAX_HALO) return QT_ERR_UNSUPPORTED;
    if ((double)N * (double)(H + 2 * ihy) * (double)(W + 2 * ihx) >= (double)GC_MAX_ELEMS ||
        (double)N * (double)(g.Ho + 2 * ohy) * (double)(g.Wo + 2 * ohx) >= (double)GC_MAX_ELEMS)
        return QT_ERR_UNSUPPORTED;
    if (!f32 && ep.ldc >= GC_MAX_ELEMS) return QT_ERR_UNSUPPORTED;
    if (!x_plane || !w) return QT_ERR_INVALID_ARG;
    if (f32) {
        if (!fo.y || dw_layout(N, g.Cout, g.Ho, g.Wo, fo.ys) < 0) return QT_ERR_INVALID_ARG;
    } else {
        if (bit_width < 2 || bit_width > 8 || ep.relu < 0 || ep.relu > 1) return QT_ERR_INVALID_ARG;
        if (!ep.alpha || !ep.beta || !ep.codes || !ep.overflow) return QT_ERR_INVALID_ARG;
        if (ep.ldc < gc_code_ld(g.Cout)) return QT_ERR_INVALID_ARG;
    }
    if (ldx < gc_code_ld(g.Cin)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(w) || !dw_aligned4(bias) || !dw_aligned4(ep.alpha) || !dw_aligned4(ep.beta) || !dw_aligned4(ep.bn_stats) ||
        !dw_aligned4(ep.overflow) || !dw_aligned4(fo.overflow) || !dw_aligned4(fo.y))
        return QT_ERR_ALIGNMENT;
    if ((ldx & 15) || !dw_aligned16(x_plane) || (ep.ldc & 15) || !dw_aligned16(ep.codes)) return QT_ERR_ALIGNMENT;
    ep.n = (float)((1 << (f32 ? 2 : bit_width)) - 1);
    fo.vec = f32 && dw_layout(N, g.Cout, g.Ho, g.Wo, fo.ys) == 1 && fo.ys.c == 1 && (g.Cout & 3) == 0 && dw_aligned16(fo.y);
    const bool fixed = (g.cout_g & 3) == 0 && (g.cin_g == 2 || g.cin_g == 4 || g.cin_g == 8) &&
                       ((kh == 1 && kw == 1) || (kh == 3 && kw == 3));
    const int K = g.cin_g * kh * kw;
    const bool regw = fixed && kh == 1;
    GcCodesMap mp{};
    const int64_t slots = f32 ? (g.Cout + 3) / 4 : ep.ldc / 4;
    int lanes = dw_pow2ceil(slots < 64 ? slots : 64);
    // the staged block wl[K][lanes] float4 stays within GC_LDS_FLOATS (K <= 512: at least 4 lanes)
    while (!regw && lanes > 1 && (int64_t)lanes * K * 4 > GC_LDS_FLOATS) lanes >>= 1;
    mp.lanes_log = dw_log2(lanes);
    mp.slots = (int)slots;
    const int tpix = DW_THREADS / lanes;
    const int64_t npix = (int64_t)g.N * g.Ho * g.Wo;
    mp.units = (int)((npix + tpix - 1) / tpix);
    const int64_t groups = (slots + lanes - 1) / lanes;
    int64_t sp = (GC_TARGET_STREAM + groups - 1) / groups;
    if (sp > mp.units) sp = mp.units;
    mp.splits = (int)(sp < 1 ? 1 : sp);
    const int64_t step = (int64_t)mp.splits * tpix;
    mp.d_wo = (int)(step % g.Wo);
    mp.d_ho = (int)((step / g.Wo) % g.Ho);
    mp.d_n = (int)(step / g.Wo / g.Ho);
    mp.ihy = (int)ihy; mp.ihx = (int)ihx; mp.ohy = (int)ohy; mp.ohx = (int)ohx;
    const unsigned grid = (unsigned)(groups * mp.splits);
    const size_t lds = regw ? 0 : sizeof(float) * 4 * lanes * K;
    hipStream_t s = (hipStream_t)stream;
#define GC_CODES_ARGS x_plane, ldx, inv_n, w, bias, ep, fo, g, mp
#define GC_CODES_LAUNCH(KH, KW, CING)                                                                                  \
    do {                                                                                                               \
        if (f32) gc_codes_kernel<KH, KW, CING, true><<<grid, DW_THREADS, lds, s>>>(GC_CODES_ARGS);                     \
        else gc_codes_kernel<KH, KW, CING, false><<<grid, DW_THREADS, lds, s>>>(GC_CODES_ARGS);                        \
    } while (0)
#define GC_CODES_CING(KH, KW)                                                                                          \
    do {                                                                                                               \
        if (g.cin_g == 2) GC_CODES_LAUNCH(KH, KW, 2);                                                                  \
        else if (g.cin_g == 4) GC_CODES_LAUNCH(KH, KW, 4);                                                             \
        else GC_CODES_LAUNCH(KH, KW, 8);                                                                               \
    } while (0)
    if (!fixed) GC_CODES_LAUNCH(0, 0, 0);
    else if (kh == 1) GC_CODES_CING(1, 1);
    else GC_CODES_CING(3, 3);
#undef GC_CODES_CING
#undef GC_CODES_LAUNCH
#undef GC_CODES_ARGS
    return qt_check_launch();
}

inline DwMap gc_reduce_plan(const GcGeom& g, int cl) { return dw_plan(cl, g.N, g.Cout * g.cin_g, g.Ho, g.Wo, GC_TARGET_REDUCE); }
inline int64_t gc_work_floats(const GcGeom& g, int splits) { return (int64_t)splits * g.Cout * g.cin_g * (g.kh * g.kw + 1); }
// 1: the 1 x 1 tile kernel, 3: the 3 x 3 one, 0: the virtual-channel kernel
inline int gc_tiled(const GcGeom& g) { return g.kh == 1 && g.kw == 1 ? 1 : (g.kh == 3 && g.kw == 3 ? 3 : 0); }
// splits of the stage 1 that runs for this geometry and layout of go
inline int gc_reduce_splits(const GcGeom& g, int cl) {
    const int tiled = gc_tiled(g);
    if (tiled == 1) return gc_tile_plan<GC_T1_COB, GC_T1_CIB>(g).splits;
    if (tiled == 3) return gc_tile_plan<GC_T3_COB, GC_T3_CIB>(g).splits;
    return gc_reduce_plan(g, cl).splits;
}

// The bodies of the three entries for any element types (the "_f32" entries: all float).  Validation order: qt_hip.h.
template <typename XT, typename WT>
int gc_forward_entry(const XT* x, const WT* w, const float* bias, XT* y, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
                     int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, const DwStrides& xs, const DwStrides& ys,
                     int kind, qt_stream_t stream) {
    GcGeom g{};
    bool empty;
    const int rc = gc_geometry(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (!gc_kind_ok(kind)) return QT_ERR_INVALID_ARG;
    if (!x || !w || !y) return QT_ERR_INVALID_ARG;
    if (dw_layout(N, g.Cin, H, W, xs) < 0 || dw_layout(N, g.Cout, g.Ho, g.Wo, ys) < 0) return QT_ERR_INVALID_ARG;
    if (!dw_aligned_elt(x) || !dw_aligned_elt(w) || !dw_aligned_elt(y) || !dw_aligned4(bias)) return QT_ERR_ALIGNMENT;
    const GcPlan pl = gc_plan(g, g.cout_g, (int64_t)g.N * g.Ho * g.Wo, g.cin_g);
    const unsigned grid = (unsigned)((int64_t)g.G * pl.nblk * pl.splits);
    const size_t lds = sizeof(float) * pl.cb * g.cin_g * kh * kw;
    hipStream_t s = (hipStream_t)stream;
    GC_DISPATCH(gc_forward_kernel, XT, WT, g, pl, x, w, bias, y, g, xs, ys, pl, kind);
    return qt_check_launch();
}

template <typename XT, typename WT>
int gc_grad_input_entry(const XT* go, const WT* w, XT* gx, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W,
                        int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, const DwStrides& gs, const DwStrides& xs,
                        int kind, qt_stream_t stream) {
    GcGeom g{};
    bool empty;
    const int rc = gc_geometry(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK || empty) return rc;
    if (!gc_kind_ok(kind)) return QT_ERR_INVALID_ARG;
    if (!go || !w || !gx) return QT_ERR_INVALID_ARG;
    if (dw_layout(N, g.Cout, g.Ho, g.Wo, gs) < 0 || dw_layout(N, g.Cin, H, W, xs) < 0) return QT_ERR_INVALID_ARG;
    if (!dw_aligned_elt(go) || !dw_aligned_elt(w) || !dw_aligned_elt(gx)) return QT_ERR_ALIGNMENT;
    const GcPlan pl = gc_plan(g, g.cin_g, (int64_t)g.N * g.H * g.W, g.cout_g);
    const unsigned grid = (unsigned)((int64_t)g.G * pl.nblk * pl.splits);
    const size_t lds = sizeof(float) * pl.jc * pl.cb * kh * kw;
    hipStream_t s = (hipStream_t)stream;
    GC_DISPATCH(gc_grad_input_kernel, XT, WT, g, pl, go, w, gx, g, gs, xs, pl, kind);
    return qt_check_launch();
}

template <typename XT, typename WT>
int gc_grad_weight_entry(const XT* go, const XT* x, const WT* w, WT* gw, WT* gbias, float* work, int64_t work_floats, int64_t N,
                         int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw,
                         int dh, int dw, const DwStrides& gs, const DwStrides& xs, float ste_threshold, qt_stream_t stream) {
    GcGeom g{};
    bool empty;
    const int rc = gc_geometry(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK) return rc;
    if (empty) return QT_OK;          // nothing is written: the caller owns the zero gradient of an empty batch
    if (!gw || (ste_threshold > 0.0f && !w) || !(ste_threshold >= 0.0f)) return QT_ERR_INVALID_ARG;
    if (!go || !x || !work || work_floats < 0) return QT_ERR_INVALID_ARG;
    const int lg = dw_layout(N, g.Cout, g.Ho, g.Wo, gs);
    if (lg < 0 || dw_layout(N, g.Cin, H, W, xs) < 0) return QT_ERR_INVALID_ARG;
    const int splits = gc_reduce_splits(g, lg);
    if (work_floats < gc_work_floats(g, splits)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned_elt(gw) || !dw_aligned_elt(gbias) || !dw_aligned_elt(w) || !dw_aligned_elt(go) || !dw_aligned_elt(x) ||
        !dw_aligned4(work))
        return QT_ERR_ALIGNMENT;
    hipStream_t s = (hipStream_t)stream;
    const int kk = kh * kw;
    const int64_t Cv = g.Cout * g.cin_g;
    const int tiled = gc_tiled(g);
    if (tiled == 1) {
        const GcTilePlan tp = gc_tile_plan<GC_T1_COB, GC_T1_CIB>(g);
        const unsigned grid = (unsigned)((int64_t)g.G * tp.nco * tp.nci * tp.splits);
        gc_grad_weight_tile_kernel<1, 1, GC_T1_COB, GC_T1_CIB, XT><<<grid, DW_THREADS, 0, s>>>(go, x, work, g, gs, xs, tp);
    } else if (tiled == 3) {
        const GcTilePlan tp = gc_tile_plan<GC_T3_COB, GC_T3_CIB>(g);
        const unsigned grid = (unsigned)((int64_t)g.G * tp.nco * tp.nci * tp.splits);
        gc_grad_weight_tile_kernel<3, 3, GC_T3_COB, GC_T3_CIB, XT><<<grid, DW_THREADS, 0, s>>>(go, x, work, g, gs, xs, tp);
    } else {
        const DwMap mp = gc_reduce_plan(g, lg);
        const unsigned grid = (unsigned)(mp.cgs * mp.splits);
        gc_grad_weight_kernel<XT><<<grid, DW_THREADS, 0, s>>>(go, x, work, g, gs, xs, mp);
    }
    const int st = qt_check_launch();
    if (st != QT_OK) return st;
    gc_grad_weight_combine_kernel<WT><<<qt_stream_grid((Cv * (kk + 1) + DW_THREADS - 1) / DW_THREADS), DW_THREADS, 0, s>>>(
        work, w, gw, gbias, Cv, g.cin_g, kk, splits, ste_threshold);
    return qt_check_launch();
}

}  // namespace

extern "C" int qt_gconv2d_f32(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t G, int64_t cin_g,
                              int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int64_t ys_n, int64_t ys_c, int64_t ys_h,
                              int64_t ys_w, int kind, qt_stream_t stream) {
    return gc_forward_entry(x, w, bias, y, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, DwStrides{xs_n, xs_c, xs_h, xs_w},
                            DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}

extern "C" int qt_gconv2d_h(const void* x, int dtype, const void* w, int w_dtype, const float* bias, void* y, int64_t N, int64_t G,
                            int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                            int dw, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int64_t ys_n, int64_t ys_c, int64_t ys_h,
                            int64_t ys_w, int kind, qt_stream_t stream) {
    int rc = QT_ERR_INVALID_ARG;
    dw_half_types(dtype, w_dtype, [&](auto* xt, auto* wt) {
        using XT = std::remove_pointer_t<decltype(xt)>;
        using WT = std::remove_pointer_t<decltype(wt)>;
        rc = gc_forward_entry(static_cast<const XT*>(x), static_cast<const WT*>(w), bias, static_cast<XT*>(y), N, G, cin_g, cout_g, H, W,
                              kh, kw, sh, sw, ph, pw, dh, dw, DwStrides{xs_n, xs_c, xs_h, xs_w}, DwStrides{ys_n, ys_c, ys_h, ys_w}, kind,
                              stream);
    });
    return rc;
}

extern "C" int qt_gconv2d_grad_input_f32(const float* go, const float* w, float* gx, int64_t N, int64_t G, int64_t cin_g,
                                         int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                         int dw, int64_t gs_n, int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c,
                                         int64_t xs_h, int64_t xs_w, int kind, qt_stream_t stream) {
    return gc_grad_input_entry(go, w, gx, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, DwStrides{gs_n, gs_c, gs_h, gs_w},
                               DwStrides{xs_n, xs_c, xs_h, xs_w}, kind, stream);
}

extern "C" int qt_gconv2d_grad_input_h(const void* go, int dtype, const void* w, int w_dtype, void* gx, int64_t N, int64_t G,
                                       int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                                       int pw, int dh, int dw, int64_t gs_n, int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n,
                                       int64_t xs_c, int64_t xs_h, int64_t xs_w, int kind, qt_stream_t stream) {
    int rc = QT_ERR_INVALID_ARG;
    dw_half_types(dtype, w_dtype, [&](auto* xt, auto* wt) {
        using XT = std::remove_pointer_t<decltype(xt)>;
        using WT = std::remove_pointer_t<decltype(wt)>;
        rc = gc_grad_input_entry(static_cast<const XT*>(go), static_cast<const WT*>(w), static_cast<XT*>(gx), N, G, cin_g, cout_g, H, W,
                                 kh, kw, sh, sw, ph, pw, dh, dw, DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w},
                                 kind, stream);
    });
    return rc;
}

extern "C" int64_t qt_gconv2d_grad_weight_work_floats(int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W,
                                                      int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw) {
    GcGeom g{};
    bool empty;
    const int rc = gc_geometry(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &empty);
    if (rc != QT_OK) return rc;
    if (empty) return 0;
    // either layout of the gradient: the larger of the two plans
    const int64_t a = gc_work_floats(g, gc_reduce_splits(g, 0)), b = gc_work_floats(g, gc_reduce_splits(g, 1));
    return a > b ? a : b;
}

extern "C" int qt_gconv2d_grad_weight_f32(const float* go, const float* x, const float* w, float* gw, float* gbias, float* work,
                                          int64_t work_floats, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
                                          int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t gs_n,
                                          int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c, int64_t xs_h,
                                          int64_t xs_w, float ste_threshold, qt_stream_t stream) {
    return gc_grad_weight_entry(go, x, w, gw, gbias, work, work_floats, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                                DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, ste_threshold, stream);
}

extern "C" int qt_gconv2d_grad_weight_h(const void* go, const void* x, int dtype, const void* w, void* gw, void* gbias, int w_dtype,
                                        float* work, int64_t work_floats, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g,
                                        int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                        int64_t gs_n, int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c,
                                        int64_t xs_h, int64_t xs_w, float ste_threshold, qt_stream_t stream) {
    int rc = QT_ERR_INVALID_ARG;
    dw_half_types(dtype, w_dtype, [&](auto* xt, auto* wt) {
        using XT = std::remove_pointer_t<decltype(xt)>;
        using WT = std::remove_pointer_t<decltype(wt)>;
        rc = gc_grad_weight_entry(static_cast<const XT*>(go), static_cast<const XT*>(x), static_cast<const WT*>(w), static_cast<WT*>(gw),
                                  static_cast<WT*>(gbias), work, work_floats, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                                  DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, ste_threshold, stream);
    });
    return rc;
}

extern "C" int qt_gconv2d_sign(const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, const float* alpha,
                               const float* beta, uint32_t* sign_plane, int64_t ldb, uint32_t* nib_plane, int64_t ldn,
                               int64_t out_halo_h, int64_t out_halo_w, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
                               int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int kind,
                               qt_stream_t stream) {
    DwPlaneOut o{};
    o.sign = sign_plane;
    o.ldb = ldb;
    o.nib = nib_plane;
    o.ldn = ldn;
    return gc_planes_launch(x_plane, ldx, w, bias, alpha, beta, o, false, out_halo_h, out_halo_w, N, G, cin_g, cout_g, H, W, kh, kw, sh,
                            sw, ph, pw, dh, dw, DwStrides{0, 0, 0, 0}, kind, stream);
}

extern "C" int qt_gconv2d_bits_f32(const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, float* y, int64_t N,
                                   int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw,
                                   int ph, int pw, int dh, int dw, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w, int kind,
                                   qt_stream_t stream) {
    DwPlaneOut o{};
    o.y = y;
    return gc_planes_launch(x_plane, ldx, w, bias, nullptr, nullptr, o, true, 0, 0, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh,
                            dw, DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}

extern "C" int qt_gconv2d_codes(const int8_t* x_plane, int64_t ldx_bytes, int64_t in_halo_h, int64_t in_halo_w, float inv_n,
                                const float* w, const float* bias, const float* alpha, const float* beta, const float* bn_stats,
                                int relu, int bit_width, int8_t* codes, int64_t ldc_bytes, int64_t out_halo_h, int64_t out_halo_w,
                                int32_t* overflow, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh,
                                int kw, int sh, int sw, int ph, int pw, int dh, int dw, qt_stream_t stream) {
    GcCodesEpi ep{};
    ep.alpha = alpha;
    ep.beta = beta;
    ep.bn_stats = bn_stats;
    ep.relu = relu;
    ep.codes = codes;
    ep.ldc = ldc_bytes;
    ep.overflow = overflow;
    return gc_codes_launch(x_plane, ldx_bytes, in_halo_h, in_halo_w, inv_n, w, bias, ep, bit_width, out_halo_h, out_halo_w, GcF32Out{},
                           N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, false, stream);
}

extern "C" int qt_gconv2d_codes_f32(const int8_t* x_plane, int64_t ldx_bytes, int64_t in_halo_h, int64_t in_halo_w, float inv_n,
                                    const float* w, const float* bias, const int32_t* overflow, float* y, int64_t N, int64_t G,
                                    int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                                    int pw, int dh, int dw, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w,
                                    qt_stream_t stream) {
    GcF32Out fo{};
    fo.y = y;
    fo.ys = DwStrides{ys_n, ys_c, ys_h, ys_w};
    fo.overflow = overflow;
    return gc_codes_launch(x_plane, ldx_bytes, in_halo_h, in_halo_w, inv_n, w, bias, GcCodesEpi{}, 0, 0, 0, fo, N, G, cin_g, cout_g, H,
                           W, kh, kw, sh, sw, ph, pw, dh, dw, true, stream);
}
