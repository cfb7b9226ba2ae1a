// Grouped conv2d with 16 ... 64 channels per group (each of cin_g, cout_g one of 16, 24, 32, 40, 48, 64) on the bf16 matrix cores:
// forward and grad_input of conv2d(x, Q(w), bias, groups = G) for fp32 tensors of ANY value.  include/qt_hip.h "Grouped convolution
// on the matrix cores, wide groups" states the contract; DESIGN.md "Grouped convs on the matrix cores, wide groups" the slicing, the
// LDS / register table and the measurements.  The arithmetic and the gather
//     dst[n, g NO + oc, r, c] = sum over taps t and k < KC of  src[n, g KC + k, sr(r, t), sc(c, t)] * Wq[oc, k, t]   (+ bias[oc])
// are those of gconv_mfma.hip (forward: src = x, KC = cin_g, NO = cout_g; grad_input: src = go, KC = cout_g, NO = cin_g), whose
// kernel keeps a group's WHOLE weight tensor in LDS beside a three-term patch of all KC channels.  At 64 / 64, 3 x 3 the weights
// alone are 72 KiB of bf16 fragments and a 128-pixel patch another 68 KiB, so here neither is resident in full:
//
// Reduction-sliced walk.  The KC channels are cut into slices of `scb` blocks of 8 (scb <= 4, balanced: 64 = 4 + 4 or 2 + 2 + 2 + 2,
// 48 = 3 + 3, 40 = 3 + 2, ...).  LDS holds ONE slice at a time: the slice's weights as B fragments wl[pair][oc] (pair = (channel
// block, tap) of the slice, padded with zero pairs to the K chunk of four; a row of wl is nopad + 1 slots so that both staging
// orders write without bank conflicts), the offset table of the tile, and the slice's channels of the tile's three-term patch.  The
// accumulators of a tile — wave w owns the 16-pixel row tiles w and w + 4 of a tile of at most 128 destination pixels, and ALL
// column tiles (at most four) of each: 8 quads, 32 VGPRs — stay in registers across the slices and taps.
// Staging a slice's weights costs as many loads as its share of a patch several times over (fp32 [oc][k][tap] in memory, quantised
// and transposed on the way), so a workgroup walks its tiles in BATCHES of GW_BATCH: per slice the weights are staged once and the
// batch's tiles run against them one after the other, each with accumulators of its own (GW_BATCH x 32 VGPRs).  Every (tile, slice)
// piece of the source box is still read from HBM exactly once.
//   stage W : fwd, lanes run along (block, tap) of one oc (the contiguous [k][tap] run of an output channel); bwd, along oc (the
//             contiguous [oc][tap] run of a reduction channel).  Eight loads, one quantiser each (`kind`), one 16-byte LDS write.
//   stage P : the bounding box of the source pixels the tile reads, clipped to the image: a thread owns (source pixel, block of 8
//             channels of the slice), splits each element exactly into three bf16 terms and stores three 16-byte LDS writes into
//             patch[term][pixel][ps].  Lanes along W for NCHW, along the blocks of a pixel for channels-last (two 16-byte loads
//             where the tensor is 16-byte aligned).  Pixel `npmax` of every term is a ZERO pixel.
//   tables  : offs[tap][q] = byte offset of the source pixel of destination pixel q under that tap, or of the zero pixel (outside
//             the image, no source under stride 2 backward, q past the tile).  The main loop has no branch on coordinates and no
//             coordinate arithmetic.
//   compute : per K chunk of 32 (four pairs) a lane (row = lane & 15, k block = lane >> 4) reads one table word per row tile, one
//             B fragment per column tile and one A fragment per row tile and term: at 64 output channels 24 MFMAs per 10 fragment
//             reads (gconv_mfma.hip: 6 per 7).  Padded columns (NO = 24, 40) are zero columns of wl and are never stored.
//   store   : pixels are the MFMA rows: a lane's quad is 4 consecutive pixels of one channel; bias added once in fp32.
// The order of every sum depends on the shapes alone: no atomics, equal inputs give equal bits.
//
// Non-finite inputs: as gconv_mfma.hip (an inf / NaN element poisons every output whose window holds it, also through a zero weight).
#include <cstdio>

#include "qt_common.h"
#include "dw_map.h"
#include "gm_plan.h"

namespace {

typedef __bf16 gw_bf8 __attribute__((ext_vector_type(8)));
typedef float gw_f4 __attribute__((ext_vector_type(4)));

constexpr int GW_BATCH = 3;                     // tiles that share one staging of a weight slice: 253 registers, two waves per SIMD
constexpr int GW_MAX_SCB = 4;                   // most channel blocks of 8 in a reduction slice
constexpr int GW_MAX_NT = 4;                    // column tiles of 16 result channels

struct GwPlan {
    int TR, TC, tiles_r, tiles_c;
    int splits;
    int npmax;               // patch pixels per term; pixel npmax is the zero pixel
    int nopad;               // NO padded to the column tile
    int scb, nslices;        // channel blocks of 8 per reduction slice (the last slice may hold fewer), slices
    int ps;                  // bytes of a patch pixel: scb blocks padded to an odd number of 16-byte slots
    int w_bytes, lds_bytes;
};

// The slice and the tile, and the LDS they need.  The tile is gm_plan's (at most 128 pixels, at most 32 columns, balanced over the
// map).  The slice is the widest (fewest passes) whose weights leave room for the whole tile's patch, down to two blocks; if even
// that does not fit, the budget loop takes rows, then columns, off the tile.  shrunk: how often it took a row, a column.
inline GwPlan gw_plan(const GmGeom& g, int taps, int* shrunk = nullptr) {
    GwPlan pl{};
    const int ks = taps == 9 ? 3 : 1, ncb = g.KC / 8;
    pl.nopad = (g.NO + 15) & ~15;
    auto need = [&](int tr, int tc) { return gm_span_cap(g.bwd, tr, g.s, ks, g.Hs) * gm_span_cap(g.bwd, tc, g.s, ks, g.Ws); };
    auto fixed = [&](int scb) { return (taps * scb + 3) / 4 * 4 * (pl.nopad + 1) * 16 + taps * GM_TILE_PIX * 4; };
    auto budget = [&](int scb) { return (GM_LDS_BYTES - fixed(scb)) / (3 * gm_ps(scb)) - 1; };     // patch pixels, the zero pixel aside
    int tc = gm_min(g.Wd, GM_TILE_COLS);
    pl.tiles_c = (g.Wd + tc - 1) / tc;
    tc = (g.Wd + pl.tiles_c - 1) / pl.tiles_c;
    int tr = gm_min(g.Hd, GM_TILE_PIX / tc);
    int scb = gm_min(ncb, GW_MAX_SCB);
    while (scb > 2 && need(tr, tc) > budget(scb)) --scb;
    pl.nslices = (ncb + scb - 1) / scb;
    pl.scb = (ncb + pl.nslices - 1) / pl.nslices;                     // balanced: never wider than the slice that fitted
    pl.ps = gm_ps(pl.scb);
    int dec[2] = {0, 0};
    while (need(tr, tc) > budget(pl.scb)) {                           // a 1 x 1 tile needs 9 pixels: this ends
        if (tr > 1) --tr, ++dec[0];
        else --tc, ++dec[1];
    }
    if (shrunk) shrunk[0] = dec[0], shrunk[1] = dec[1];
    pl.tiles_c = (g.Wd + tc - 1) / tc;
    pl.tiles_r = (g.Hd + tr - 1) / tr;
    pl.TR = (g.Hd + pl.tiles_r - 1) / pl.tiles_r;
    pl.TC = (g.Wd + pl.tiles_c - 1) / pl.tiles_c;
    pl.npmax = need(pl.TR, pl.TC);
    pl.w_bytes = fixed(pl.scb) - taps * GM_TILE_PIX * 4;
    pl.lds_bytes = fixed(pl.scb) + 3 * (pl.npmax + 1) * pl.ps;
    const int64_t units = (int64_t)g.N * pl.tiles_r * pl.tiles_c;
    int64_t s = (GM_TARGET_WGS + g.G - 1) / g.G;
    if (s * GW_BATCH > units) s = units / GW_BATCH;                   // a workgroup has a full batch where the problem has one
    pl.splits = (int)(s < 1 ? 1 : s);
    return pl;
}

__device__ __forceinline__ uint32_t gw_bf16_rn(float f) {          // round to nearest even, NaN kept quiet (split_bf16.hip)
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// v = hi + mid + lo exactly (each subtraction is exact in fp32): the three terms of element e of a block of 8 into halves of t[]
__device__ __forceinline__ void gw_split(float v, int e, uint32_t (&hi)[4], uint32_t (&mid)[4], uint32_t (&lo)[4]) {
    const uint32_t a = gw_bf16_rn(v);
    const float r1 = v - __uint_as_float(a << 16);
    const uint32_t b = gw_bf16_rn(r1);
    const float r2 = r1 - __uint_as_float(b << 16);
    const uint32_t c = gw_bf16_rn(r2);
    const int sh = 16 * (e & 1);
    hi[e >> 1] |= a << sh;
    mid[e >> 1] |= b << sh;
    lo[e >> 1] |= c << sh;
}

// the destination tile of unit u and the clipped source box it reads
struct GwTile {
    int n, r0, c0, TCa, npix;
    int lo_r, PH, lo_c, PW;
};

template <int KS>
__device__ __forceinline__ GwTile gw_tile(const GmGeom& g, const GwPlan& pl, int u) {
    GwTile t;
    const int tiles = pl.tiles_r * pl.tiles_c;
    t.n = u / tiles;
    const int tt = u - t.n * tiles, tr = tt / pl.tiles_c, tc = tt - tr * pl.tiles_c;
    t.r0 = tr * pl.TR;
    t.c0 = tc * pl.TC;
    const int TRa = gm_min(pl.TR, g.Hd - t.r0);
    t.TCa = gm_min(pl.TC, g.Wd - t.c0);
    t.npix = TRa * t.TCa;
    gm_span(g.bwd, t.r0, t.r0 + TRa, g.s, g.ph, KS, g.Hs, t.lo_r, t.PH);
    gm_span(g.bwd, t.c0, t.c0 + t.TCa, g.s, g.pw, KS, g.Ws, t.lo_c, t.PW);
    return t;
}

template <int TAPS>
__global__ __launch_bounds__(DW_THREADS) void gw_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ dst, GmGeom g,
                                                        DwStrides ss, DwStrides ds, GwPlan pl, int kind) {
    constexpr int KS = TAPS == 9 ? 3 : 1;                            // kernel side
    extern __shared__ __attribute__((aligned(16))) unsigned char gw_smem[];
    uint4* wl = reinterpret_cast<uint4*>(gw_smem);                   // [pairs of a slice, padded to 4][nopad + 1]
    int* offs = reinterpret_cast<int*>(gw_smem + pl.w_bytes);        // [TAPS][128]
    unsigned char* patch = reinterpret_cast<unsigned char*>(offs + TAPS * GM_TILE_PIX);   // [3][npmax + 1][PS]
    const int PS = pl.ps, TS = (pl.npmax + 1) * PS, zero_off = pl.npmax * PS, WLS = pl.nopad + 1;
    const int KC = g.KC, NCB = KC >> 3, NT = pl.nopad >> 4;
    const int tid = threadIdx.x;
    const int grp = (int)(blockIdx.x / pl.splits);
    const int split = (int)(blockIdx.x - (unsigned)grp * pl.splits);

    for (int e = tid; e < 3 * (PS / 16); e += DW_THREADS) {          // once: the zero pixel of every term
        const int term = e / (PS / 16), sl = e - term * (PS / 16);
        *reinterpret_cast<uint4*>(patch + term * TS + zero_off + sl * 16) = make_uint4(0u, 0u, 0u, 0u);
    }

    const int lane = tid & 63, lrow = lane & 15, kb = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int units = g.N * pl.tiles_r * pl.tiles_c;
    for (int ub = split; ub < units; ub += GW_BATCH * pl.splits) {   // uniform over the workgroup: so are the barriers
        gw_f4 acc[GW_BATCH][2][GW_MAX_NT];
#pragma unroll
        for (int tb = 0; tb < GW_BATCH; ++tb)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int nt = 0; nt < GW_MAX_NT; ++nt) acc[tb][h][nt] = gw_f4{0.0f, 0.0f, 0.0f, 0.0f};

        for (int sl = 0; sl < pl.nslices; ++sl) {
            const int cb0 = sl * pl.scb, ncbs = gm_min(pl.scb, NCB - cb0);
            const int pairs = TAPS * ncbs, nchunk = (pairs + 3) >> 2, P4 = nchunk * 4;
            __syncthreads();                                          // the previous slice / batch has been computed
            // the slice's weights as B fragments: pair p = (block cb, tap t), cb-major
            for (int e = tid; e < P4 * pl.nopad; e += DW_THREADS) {
                int p, oc;
                if (g.bwd) {
                    p = e / pl.nopad;
                    oc = e - p * pl.nopad;
                } else {
                    oc = e / P4;
                    p = e - oc * P4;
                }
                const int cb = p / TAPS, t = p - cb * TAPS;
                uint32_t h[4] = {0u, 0u, 0u, 0u};
                if (p < pairs && oc < g.NO) {
                    const int kc0 = (cb0 + cb) * 8;
                    const int64_t idx = g.bwd ? (((int64_t)grp * KC + kc0) * g.NO + oc) * TAPS + t
                                              : (((int64_t)grp * g.NO + oc) * KC + kc0) * TAPS + t;
                    const int64_t kstep = g.bwd ? (int64_t)g.NO * TAPS : TAPS;
#pragma unroll
                    for (int k = 0; k < 8; ++k) h[k >> 1] |= gw_bf16_rn(dw_quant(kind, w[idx + k * kstep])) << (16 * (k & 1));
                }
                wl[p * WLS + oc] = make_uint4(h[0], h[1], h[2], h[3]);
            }

#pragma unroll
            for (int tb = 0; tb < GW_BATCH; ++tb) {
                const int u = ub + tb * pl.splits;
                if (u >= units) break;                                // uniform
                const GwTile tl = gw_tile<KS>(g, pl, u);
                const int np = tl.PH * tl.PW;
                if (tb > 0) __syncthreads();                          // the previous tile of the batch has been computed
                const float* sbase = src + tl.n * ss.n + ((int64_t)grp * KC + cb0 * 8) * ss.c + tl.lo_r * ss.h + tl.lo_c * ss.w;
                for (int e = tid; e < np * ncbs; e += DW_THREADS) {
                    int cb, pp;
                    if (ss.c == 1) {                                  // channels-last: the blocks of a pixel on consecutive lanes
                        pp = e / ncbs;
                        cb = e - pp * ncbs;
                    } else {                                          // NCHW: consecutive lanes along W
                        cb = e / np;
                        pp = e - cb * np;
                    }
                    const int row = pp / tl.PW, col = pp - row * tl.PW;
                    const float* sp = sbase + row * ss.h + col * ss.w + cb * 8 * ss.c;
                    float v[8];
                    if (g.vec) {
                        const float4 a = *reinterpret_cast<const float4*>(sp), b = *reinterpret_cast<const float4*>(sp + 4);
                        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] = sp[k * ss.c];
                    }
                    uint32_t hi[4] = {0u, 0u, 0u, 0u}, mid[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 8; ++k) gw_split(v[k], k, hi, mid, lo);
                    unsigned char* pd = patch + pp * PS + cb * 16;
                    *reinterpret_cast<uint4*>(pd) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
                    *reinterpret_cast<uint4*>(pd + TS) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
                    *reinterpret_cast<uint4*>(pd + 2 * TS) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
                }
                for (int e = tid; e < TAPS * GM_TILE_PIX; e += DW_THREADS) {
                    const int t = e / GM_TILE_PIX, q = e - t * GM_TILE_PIX;
                    const bool in = q < tl.npix;
                    const int qr = in ? q / tl.TCa : 0;
                    const int r = tl.r0 + qr, c = tl.c0 + (in ? q - qr * tl.TCa : 0);
                    const int i = t / KS, j = t - i * KS;
                    int sr, sc;
                    bool ok = in;
                    if (!g.bwd) {
                        sr = r * g.s - g.ph + i;
                        sc = c * g.s - g.pw + j;
                    } else {
                        const int hh = r + g.ph - i, ww = c + g.pw - j;
                        ok = ok && hh >= 0 && ww >= 0;
                        sr = (hh < 0 ? 0 : hh) / g.s;
                        sc = (ww < 0 ? 0 : ww) / g.s;
                        ok = ok && sr * g.s == hh && sc * g.s == ww;
                    }
                    ok = ok && (unsigned)(sr - tl.lo_r) < (unsigned)tl.PH && (unsigned)(sc - tl.lo_c) < (unsigned)tl.PW;   // inside the image
                    offs[e] = ok ? ((sr - tl.lo_r) * tl.PW + (sc - tl.lo_c)) * PS : zero_off;
                }
                __syncthreads();

                const int nrt = (tl.npix + 15) >> 4;                  // row tiles of the tile: this wave's are `wave` and `wave + 4`
                if (wave < nrt) {
                    const bool two = wave + 4 < nrt;
                    const int q0 = wave * 16 + lrow;
                    for (int ch = 0; ch < nchunk; ++ch) {
                        const int p = 4 * ch + kb;                    // the lane's pair of this chunk
                        const int cb = p / TAPS, t = p - cb * TAPS;
                        const bool live = p < pairs;                  // a padding pair reads the zero pixel (its weights are zero too)
                        const int o0 = live ? offs[t * GM_TILE_PIX + q0] + cb * 16 : zero_off;
                        const int o1 = live && two ? offs[t * GM_TILE_PIX + q0 + 64] + cb * 16 : zero_off;
                        gw_bf8 b[GW_MAX_NT];
#pragma unroll
                        for (int nt = 0; nt < GW_MAX_NT; ++nt) {
                            if (nt < NT) {
                                const uint4 bw = wl[p * WLS + nt * 16 + lrow];
                                __builtin_memcpy(&b[nt], &bw, 16);
                            }
                        }
#pragma unroll
                        for (int term = 0; term < 3; ++term) {
                            const gw_bf8 a0 = *reinterpret_cast<const gw_bf8*>(patch + term * TS + o0);
#pragma unroll
                            for (int nt = 0; nt < GW_MAX_NT; ++nt)
                                if (nt < NT) acc[tb][0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b[nt], acc[tb][0][nt], 0, 0, 0);
                            if (two) {
                                const gw_bf8 a1 = *reinterpret_cast<const gw_bf8*>(patch + term * TS + o1);
#pragma unroll
                                for (int nt = 0; nt < GW_MAX_NT; ++nt)
                                    if (nt < NT) acc[tb][1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b[nt], acc[tb][1][nt], 0, 0, 0);
                            }
                        }
                    }
                }
            }
        }

        // D[row = 4 kb + i][col = lrow]: 4 consecutive pixels of result channel nt * 16 + lrow
#pragma unroll
        for (int tb = 0; tb < GW_BATCH; ++tb) {
            const int u = ub + tb * pl.splits;
            if (u >= units) break;
            const GwTile tl = gw_tile<KS>(g, pl, u);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int qb = (wave + 4 * h) * 16 + kb * 4;
                if (qb >= tl.npix) continue;
#pragma unroll
                for (int nt = 0; nt < GW_MAX_NT; ++nt) {
                    const int oc = nt * 16 + lrow;
                    if (oc >= g.NO) continue;                         // a padded column is never stored
                    const int64_t ch = (int64_t)grp * g.NO + oc;
                    float* dp = dst + tl.n * ds.n + ch * ds.c;
                    const float bv = bias ? bias[ch] : 0.0f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int q = qb + i;
                        if (q < tl.npix) {
                            const int qr = q / tl.TCa;
                            const float v = acc[tb][h][nt][i];
                            dp[(tl.r0 + qr) * ds.h + (tl.c0 + q - qr * tl.TCa) * ds.w] = bias ? v + bv : v;
                        }
                    }
                }
            }
        }
    }
}

// The validation of the forward and grad_input entries, in the documented order.  in / out: the tensor read (x, go) and the one
// written (y, gx).
int gw_entry(bool bwd, const float* in, const float* w, const float* bias, float* out, int64_t N, int64_t G, int64_t cin_g,
             int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, const DwStrides& is,
             const DwStrides& os, int kind, qt_stream_t stream) {
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc, true)) return rc;
    const int64_t Cin = G * cin_g, Cout = G * cout_g;
    if (kind != QT_DW_RAW && kind != QT_DW_SIGN && kind != QT_DW_TERNARY) return QT_ERR_INVALID_ARG;
    if (!in || !w || !out) return QT_ERR_INVALID_ARG;
    const DwStrides& xs = bwd ? os : is;
    const DwStrides& ys = bwd ? is : os;
    if (dw_layout(N, Cin, H, W, xs) < 0 || dw_layout(N, Cout, Ho, Wo, ys) < 0) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(in) || !dw_aligned4(w) || !dw_aligned4(out) || !dw_aligned4(bias)) return QT_ERR_ALIGNMENT;
    GmGeom g = gm_geom(bwd, N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw);
    g.vec = is.c == 1 && qt_aligned16(in) ? 1 : 0;                 // every pixel's channel block then starts on 32 bytes
    const GwPlan pl = gw_plan(g, kh * kw);
    const unsigned grid = (unsigned)((int64_t)g.G * pl.splits);
    hipStream_t s = (hipStream_t)stream;
    if (kh == 3) gw_kernel<9><<<grid, DW_THREADS, (size_t)pl.lds_bytes, s>>>(in, w, bias, out, g, is, os, pl, kind);
    else gw_kernel<1><<<grid, DW_THREADS, (size_t)pl.lds_bytes, s>>>(in, w, bias, out, g, is, os, pl, kind);
    return qt_check_launch();
}

}  // namespace

// What the launch of the forward (bwd = 0) or grad_input (bwd = 1) entry would run for these numbers: steps 1 to 3 of the
// validation, then the plan function the launch calls.  No device call.
extern "C" int qt_gwconv2d_describe(int bwd, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw,
                                    int sh, int sw, int ph, int pw, int dh, int dw, char* out, int cap) {
    if (!out || cap < 2 || (bwd != 0 && bwd != 1)) return QT_ERR_INVALID_ARG;
    out[0] = 0;
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc, true)) return rc;   // an empty problem: no text
    const GmGeom g = gm_geom(bwd != 0, N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw);
    int shrunk[2] = {0, 0};
    const GwPlan pl = gw_plan(g, kh * kw, shrunk);
    snprintf(out, (size_t)cap,
             "kernel=gw_kernel<%d> TR=%d TC=%d tiles_r=%d tiles_c=%d units=%lld splits=%d batch=%d npmax=%d scb=%d nslices=%d nopad=%d "
             "lds_bytes=%d tr_shrunk=%d tc_shrunk=%d grid=%lld block=%d",
             kh * kw, pl.TR, pl.TC, pl.tiles_r, pl.tiles_c, (long long)(N * pl.tiles_r * pl.tiles_c), pl.splits, GW_BATCH, pl.npmax,
             pl.scb, pl.nslices, pl.nopad, pl.lds_bytes, shrunk[0], shrunk[1], (long long)(G * pl.splits), DW_THREADS);
    return QT_OK;
}

extern "C" int qt_gwconv2d_f32(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t G, int64_t cin_g,
                               int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                               int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int64_t ys_n, int64_t ys_c, int64_t ys_h,
                               int64_t ys_w, int kind, qt_stream_t stream) {
    return gw_entry(false, x, w, bias, y, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                    DwStrides{xs_n, xs_c, xs_h, xs_w}, DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}

extern "C" int qt_gwconv2d_grad_input_f32(const float* go, const float* w, float* gx, int64_t N, int64_t G, int64_t cin_g,
                                          int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                          int dw, int64_t gs_n, int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c,
                                          int64_t xs_h, int64_t xs_w, int kind, qt_stream_t stream) {
    return gw_entry(true, go, w, nullptr, gx, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                    DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, kind, stream);
}
