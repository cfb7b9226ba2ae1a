// Grouped conv2d with 16, 24 or 32 input channels per group on the bf16 matrix cores: forward and grad_input of
// conv2d(x, Q(w), bias, groups = G) for fp32 tensors of ANY value.  include/qt_hip.h "Grouped convolution on the matrix cores"
// states the contract; DESIGN.md "Grouped convs on the matrix cores" the layout, the counts and the measurements.
//
// At this size a group stops being "no matrix-core shape": its output channels are one to three 16-wide MFMA column tiles and a
// K chunk of 32 is two taps of 16 channels or one tap of 32, so a workgroup that works inside ONE group wastes nothing on the
// block-diagonal zeros.  One kernel template serves both directions as a gather
//     dst[n, g NO + oc, r, c] = sum over taps t and k < KC of  src[n, g KC + k, sr(r, t), sc(c, t)] * Wq[oc, k, t]   (+ bias[oc])
//   forward    : src = x, dst = y, KC = cin_g, NO = cout_g, sr = r s - p + i
//   grad_input : src = go, dst = gx, KC = cout_g, NO = cin_g, sr = (r + p - i) / s where that division is exact (a (pixel, tap)
//                pair without a source contributes a zero fragment: no atomics, gx written in full)
// with the real operand split EXACTLY into three bf16 terms (hi = bf16_rn(v), mid = bf16_rn(v - hi), lo = bf16_rn(v - hi - mid))
// inside the launch, the quantised weight exact in bf16, and fp32 accumulation inside v_mfma_f32_16x16x32_bf16.
//
// Work split.  A workgroup (4 waves) owns ONE group and walks tiles split, split + S, ... of the flat (n, tile) index; a tile is
// TR x TC destination pixels (at most 128, balanced over the map).  Once per workgroup: the group's weights, quantised (`kind`),
// into LDS as bf16 B fragments wl[pair][oc][8] (pair = (tap, block of 8 reduction channels), padded with zero pairs to a multiple
// of four; oc padded with zero columns to a multiple of 16).  Per tile:
//   stage   : the bounding box of the source pixels the tile reads, clipped to the image, is read ONCE from HBM — a thread owns
//             (source pixel, block of 8 channels): lanes run along W for NCHW (coalesced row segments), along the channel blocks
//             of a pixel for channels-last (two 16-byte loads when the tensor is 16-byte aligned) — split once and stored as
//             three 16-byte LDS writes into patch[term][pixel][KC (+ pad)].  Pixel `npmax` of every term is a ZERO pixel.
//   tables  : offs[tap][q] = byte offset of the source pixel of destination pixel q under that tap, or of the zero pixel where it
//             lies outside the image / has no source (stride 2 backward) / q is past the tile; outq[q] = q's offset in dst or -1.
//             So the main loop has no branch and no coordinate arithmetic.
//   compute : a wave takes (pair of 16-pixel row tiles, 16-channel column tile) items round-robin.  Per K chunk of 32 a lane
//             (row = lane & 15, k block = lane >> 4) reads one table word, its B fragment (16 bytes) and per row tile and term
//             one A fragment (16 bytes at offs + term plane + channel block): 6 MFMAs per 7 fragment reads.  Pixels are the MFMA
//             rows, so a lane's accumulator quad is 4 consecutive pixels of one channel; the bias is added once in fp32.
// LDS strides: a pixel is KC * 2 bytes padded to an ODD number of 16-byte slots, so the 16 lanes of a fragment read (consecutive
// pixels) fall into 16 different slots of the 256-byte bank row; the B fragments of 16 lanes are 256 contiguous bytes.
//
// Non-finite inputs: an inf / NaN element poisons (NaN) every output whose window holds it — also through a ZERO weight
// (0 * inf), unlike the streaming kernels; elements of magnitude above ~3.39e38 overflow in the bf16 rounding of `hi`.
#include <cstdio>

#include "qt_common.h"
#include "dw_map.h"
#include "gm_describe.h"
#include "gm_plan.h"

namespace {

typedef __bf16 gm_bf8 __attribute__((ext_vector_type(8)));
typedef float gm_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t gm_bf16_rn(float f) {          // round to nearest even, NaN kept quiet (split_bf16.hip)
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}

// v = hi + mid + lo exactly (each subtraction is exact in fp32): the three terms of element e of a block of 8 into halves of t[]
__device__ __forceinline__ void gm_split(float v, int e, uint32_t (&hi)[4], uint32_t (&mid)[4], uint32_t (&lo)[4]) {
    const uint32_t a = gm_bf16_rn(v);
    const float r1 = v - __uint_as_float(a << 16);
    const uint32_t b = gm_bf16_rn(r1);
    const float r2 = r1 - __uint_as_float(b << 16);
    const uint32_t c = gm_bf16_rn(r2);
    const int sh = 16 * (e & 1);
    hi[e >> 1] |= a << sh;
    mid[e >> 1] |= b << sh;
    lo[e >> 1] |= c << sh;
}

template <int TAPS, int NCB>
__global__ __launch_bounds__(DW_THREADS) void gm_kernel(const float* __restrict__ src, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ dst, GmGeom g,
                                                        DwStrides ss, DwStrides ds, GmPlan pl, int kind) {
    constexpr int KC = NCB * 8, PAIRS = TAPS * NCB, NCHUNK = (PAIRS + 3) / 4, PS = gm_ps(NCB);
    constexpr int KS = TAPS == 9 ? 3 : 1;                            // kernel side
    extern __shared__ __attribute__((aligned(16))) unsigned char gm_smem[];
    uint4* wl = reinterpret_cast<uint4*>(gm_smem);                   // [NCHUNK * 4][nopad]
    int* offs = reinterpret_cast<int*>(gm_smem + pl.w_bytes);        // [TAPS][128]
    int* outq = offs + TAPS * GM_TILE_PIX;                           // [128]
    unsigned char* patch = reinterpret_cast<unsigned char*>(outq + GM_TILE_PIX);          // [3][npmax + 1][PS]
    const int TS = (pl.npmax + 1) * PS, zero_off = pl.npmax * PS;
    const int tid = threadIdx.x;
    const int grp = (int)(blockIdx.x / pl.splits);
    const int split = (int)(blockIdx.x - (unsigned)grp * pl.splits);

    // once: the group's weights as B fragments, the zero pixel of every term
    for (int e = tid; e < NCHUNK * 4 * pl.nopad; e += DW_THREADS) {
        const int p = e / pl.nopad, oc = e - p * pl.nopad;
        const int t = p / NCB, cb = p - t * NCB;
        uint32_t h[4] = {0u, 0u, 0u, 0u};
        if (p < PAIRS && oc < g.NO) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int kc = cb * 8 + k;
                const int64_t idx = g.bwd ? (((int64_t)grp * KC + kc) * g.NO + oc) * TAPS + t
                                          : (((int64_t)grp * g.NO + oc) * KC + kc) * TAPS + t;
                h[k >> 1] |= gm_bf16_rn(dw_quant(kind, w[idx])) << (16 * (k & 1));
            }
        }
        wl[e] = make_uint4(h[0], h[1], h[2], h[3]);
    }
    for (int e = tid; e < 3 * (PS / 16); e += DW_THREADS) {
        const int term = e / (PS / 16), sl = e - term * (PS / 16);
        *reinterpret_cast<uint4*>(patch + term * TS + zero_off + sl * 16) = make_uint4(0u, 0u, 0u, 0u);
    }

    const int wave = tid >> 6, lane = tid & 63, lrow = lane & 15, kb = lane >> 4;
    const int tiles = pl.tiles_r * pl.tiles_c;
    const int units = g.N * tiles;
    for (int u = split; u < units; u += pl.splits) {                 // uniform over the workgroup: so are the barriers
        const int n = u / tiles, tt = u - n * tiles;
        const int tr = tt / pl.tiles_c, tc = tt - tr * pl.tiles_c;
        const int r0 = tr * pl.TR, c0 = tc * pl.TC;
        const int TRa = gm_min(pl.TR, g.Hd - r0), TCa = gm_min(pl.TC, g.Wd - c0);
        const int npix = TRa * TCa;
        int lo_r, PH, lo_c, PW;
        gm_span(g.bwd, r0, r0 + TRa, g.s, g.ph, KS, g.Hs, lo_r, PH);
        gm_span(g.bwd, c0, c0 + TCa, g.s, g.pw, KS, g.Ws, lo_c, PW);
        const int np = PH * PW;
        __syncthreads();                                              // the previous tile has been read (first tile: wl is written)
        const float* sbase = src + n * ss.n + (int64_t)grp * KC * ss.c + lo_r * ss.h + lo_c * ss.w;
        for (int e = tid; e < np * NCB; e += DW_THREADS) {
            int cb, pp;
            if (ss.c == 1) {                                          // channels-last: the blocks of a pixel on consecutive lanes
                pp = e / NCB;
                cb = e - pp * NCB;
            } else {                                                  // NCHW: consecutive lanes along W
                cb = e / np;
                pp = e - cb * np;
            }
            const int row = pp / PW, col = pp - row * PW;
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
            for (int k = 0; k < 8; ++k) gm_split(v[k], k, hi, mid, lo);
            unsigned char* pd = patch + pp * PS + cb * 16;
            *reinterpret_cast<uint4*>(pd) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
            *reinterpret_cast<uint4*>(pd + TS) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
            *reinterpret_cast<uint4*>(pd + 2 * TS) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        }
        for (int e = tid; e < (TAPS + 1) * GM_TILE_PIX; e += DW_THREADS) {
            const int t = e / GM_TILE_PIX, q = e - t * GM_TILE_PIX;
            const bool in = q < npix;
            const int qr = in ? q / TCa : 0;
            const int r = r0 + qr, c = c0 + (in ? q - qr * TCa : 0);
            if (t == TAPS) {
                outq[q] = in ? (int)(r * ds.h + c * ds.w) : -1;
                continue;
            }
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
            ok = ok && (unsigned)(sr - lo_r) < (unsigned)PH && (unsigned)(sc - lo_c) < (unsigned)PW;   // inside the image: inside the box
            offs[e] = ok ? ((sr - lo_r) * PW + (sc - lo_c)) * PS : zero_off;
        }
        __syncthreads();

        const int npp = (npix + 31) >> 5;
        const int items = npp * (pl.nopad >> 4);
        for (int it = wave; it < items; it += DW_THREADS / 64) {
            const int nt = it / npp, pp = it - nt * npp;
            const int q0 = pp * 32 + lrow;
            gm_f4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ch = 0; ch < NCHUNK; ++ch) {
                const int p = 4 * ch + kb;                            // the lane's pair of this chunk
                const int t = p / NCB, cb = p - t * NCB;
                const bool live = p < PAIRS;                          // a padding pair reads the zero pixel (its weights are zero too)
                const int ti = live ? t * GM_TILE_PIX : 0;
                const int o0 = (live ? offs[ti + q0] : zero_off) + cb * 16;
                const int o1 = (live ? offs[ti + q0 + 16] : zero_off) + cb * 16;
                gm_bf8 b;
                const uint4 bw = wl[p * pl.nopad + nt * 16 + lrow];
                __builtin_memcpy(&b, &bw, 16);
#pragma unroll
                for (int term = 0; term < 3; ++term) {
                    const gm_bf8 a0 = *reinterpret_cast<const gm_bf8*>(patch + term * TS + o0);
                    const gm_bf8 a1 = *reinterpret_cast<const gm_bf8*>(patch + term * TS + o1);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b, acc1, 0, 0, 0);
                }
            }
            // D[row = 4 kb + i][col = lrow]: 4 consecutive pixels of output channel nt * 16 + lrow
            const int oc = nt * 16 + lrow;
            if (oc < g.NO) {
                const int64_t ch = (int64_t)grp * g.NO + oc;
                float* dp = dst + n * ds.n + ch * ds.c;
                const float bv = bias ? bias[ch] : 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int oa = outq[pp * 32 + kb * 4 + i], ob = outq[pp * 32 + 16 + kb * 4 + i];
                    if (oa >= 0) dp[oa] = bias ? acc0[i] + bv : acc0[i];
                    if (ob >= 0) dp[ob] = bias ? acc1[i] + bv : acc1[i];
                }
            }
        }
    }
}

template <int TAPS>
int gm_launch(int ncb, const float* src, const float* w, const float* bias, float* dst, const GmGeom& g, const DwStrides& ss,
              const DwStrides& ds, int kind, hipStream_t s) {
    const GmPlan pl = gm_plan(g, TAPS, ncb, 3);
    const unsigned grid = (unsigned)((int64_t)g.G * pl.splits);
#define GM_GO(NCB) gm_kernel<TAPS, NCB><<<grid, DW_THREADS, (size_t)pl.lds_bytes, s>>>(src, w, bias, dst, g, ss, ds, pl, kind)
    if (ncb == 2) GM_GO(2);
    else if (ncb == 3) GM_GO(3);
    else if (ncb == 4) GM_GO(4);
    else GM_GO(6);
#undef GM_GO
    return qt_check_launch();
}

// The validation of the forward and grad_input entries, in the documented order.  in / out: the tensor read (x, go) and the one
// written (y, gx).
int gm_entry(bool bwd, const float* in, const float* w, const float* bias, float* out, int64_t N, int64_t G, int64_t cin_g,
             int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, const DwStrides& is,
             const DwStrides& os, int kind, qt_stream_t stream) {
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;
    const int64_t Cin = G * cin_g, Cout = G * cout_g;
    if (kind != QT_DW_RAW && kind != QT_DW_SIGN && kind != QT_DW_TERNARY) return QT_ERR_INVALID_ARG;
    if (!in || !w || !out) return QT_ERR_INVALID_ARG;
    const DwStrides& xs = bwd ? os : is;
    const DwStrides& ys = bwd ? is : os;
    if (dw_layout(N, Cin, H, W, xs) < 0 || dw_layout(N, Cout, Ho, Wo, ys) < 0) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(in) || !dw_aligned4(w) || !dw_aligned4(out) || !dw_aligned4(bias)) return QT_ERR_ALIGNMENT;
    GmGeom g = gm_geom(bwd, N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw);
    g.vec = is.c == 1 && qt_aligned16(in) ? 1 : 0;                 // every pixel's group block then starts on 32 bytes
    hipStream_t s = (hipStream_t)stream;
    return kh == 3 ? gm_launch<9>(g.KC / 8, in, w, bias, out, g, is, os, kind, s)
                   : gm_launch<1>(g.KC / 8, in, w, bias, out, g, is, os, kind, s);
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------------
//     gw[g cout_g + oc, ci, i, j] = sum over (n, ho, wo) of  go[n, g cout_g + oc, ho, wo] * x[n, g cin_g + ci, ho s - p + i, wo s - p + j]
// is per group a dense [cin_g taps x L] . [L x cout_g] product whose reduction runs over the L = N Ho Wo output PIXELS; both
// operands are real, so both are split exactly into three bf16 terms and the six products of the project's real x real convention
// (gh xh, gh xm, gh xl, gm xh, gm xm, gl xh) go into one fp32 accumulator.
//
// Work split: as above, grid = G x splits, a workgroup owns one group and walks tiles split, split + S, ... of the flat (n, tile of
// output pixels) index with its accumulators in registers; at the end it writes ONE partial [split][g][tap][oc][ci] (+ [oc] for the
// bias gradient) with float4 stores.  gmw_reduce_kernel sums the splits in index order, masks and writes gw / gbias.
// Per tile: the go tile (TR x TC output pixels, zero-filled up to a multiple of 32) and the x patch (the bounding box the tile's taps
// read, clipped to the image; pixel npmax is a ZERO pixel) are staged once each, split, pixel-major [term][pixel][channels (+ pad)]
// like the forward's patch; offs[tap][q] is the patch offset of output pixel q's source under that tap, or the zero pixel's.
// Fragments: v_mfma_f32_16x16x32_bf16 wants 8 consecutive k (here: pixels) of one channel per lane.  ds_read_b64_tr_b16 makes
// them out of the pixel-major tiles: in a 16-lane group lane q gives the address of 4 channels (q & 3) of pixel row (q >> 2) and
// lane i receives channel i of the four rows; two reads per fragment.  Every lane supplies its own row address, so the x rows come
// straight from the offset table: no branch, no coordinate arithmetic in the main loop.
// Roles: x is the MFMA's A operand (rows = ci), go its B operand (columns = oc), so a lane's accumulator quad is 4 consecutive ci
// of one oc: one float4 of the partial.  Items are (row tile of 16 oc, column tile of 16 ci, tap) plus one "bias" item per row tile
// (go against a register fragment of ones: gbias from the same pass); the four waves take contiguous, balanced runs of them, so a
// wave's go fragments of a 32-pixel chunk are reused across its taps.  cin_g = 24 reads 8 channels past the pixel in its second
// column tile (the neighbour's, or the 16 bytes of slack after the last): MFMA rows are independent and those rows are never stored.

typedef short gm_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) gm_s4 gm_lds_s4;

// the fragment of the two transposing reads at LDS bytes a and b: elements 0-3 from a, 4-7 from b
__device__ __forceinline__ gm_bf8 gmw_frag(const unsigned char* a, const unsigned char* b) {
    const gm_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gm_lds_s4*)a);
    const gm_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gm_lds_s4*)b);
    gm_bf8 f;
    __builtin_memcpy(&f, &lo, 8);
    __builtin_memcpy(reinterpret_cast<unsigned char*>(&f) + 8, &hi, 8);
    return f;
}

// Stage pixels [0, nfill) of a PW-wide box at `base` (8 NCB channels from there) into dst[term][pixel][PS]: pixels below np are read,
// split into three terms and stored as three 16-byte writes, the others are zero.  Lanes as in the forward's stage.
template <int NCB>
__device__ __forceinline__ void gmw_stage(const float* __restrict__ base, const DwStrides& st, int vec, int PW, int np, int nfill,
                                          unsigned char* dst, int TS, int tid) {
    constexpr int PS = gm_ps(NCB);
    for (int e = tid; e < nfill * NCB; e += DW_THREADS) {
        int cb, pp;
        if (st.c == 1) {
            pp = e / NCB;
            cb = e - pp * NCB;
        } else {
            cb = e / nfill;
            pp = e - cb * nfill;
        }
        uint32_t hi[4] = {0u, 0u, 0u, 0u}, mid[4] = {0u, 0u, 0u, 0u}, lo[4] = {0u, 0u, 0u, 0u};
        if (pp < np) {
            const int row = pp / PW, col = pp - row * PW;
            const float* sp = base + row * st.h + col * st.w + cb * 8 * st.c;
            float v[8];
            if (vec) {
                const float4 a = *reinterpret_cast<const float4*>(sp), b = *reinterpret_cast<const float4*>(sp + 4);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = sp[k * st.c];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) gm_split(v[k], k, hi, mid, lo);
        }
        unsigned char* pd = dst + pp * PS + cb * 16;
        *reinterpret_cast<uint4*>(pd) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        *reinterpret_cast<uint4*>(pd + TS) = make_uint4(mid[0], mid[1], mid[2], mid[3]);
        *reinterpret_cast<uint4*>(pd + 2 * TS) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
}

// NCBX: blocks of 8 input channels of a group (2, 3, 4); RT: row tiles of 16 output channels (1, 2, 3)
template <int TAPS, int NCBX, int RT>
__global__ __launch_bounds__(DW_THREADS) void gmw_kernel(const float* __restrict__ go, const float* __restrict__ x,
                                                         float* __restrict__ work, GmGeom g, DwStrides gs, DwStrides xs, GmwPlan pl) {
    constexpr int CIN = NCBX * 8, COUT = RT * 16, CT = (NCBX + 1) / 2, NCBG = RT * 2, PSX = gm_ps(NCBX), PSG = gm_ps(NCBG);
    constexpr int KS = TAPS == 9 ? 3 : 1;
    constexpr int CONV = RT * CT * TAPS, ITEMS = CONV + RT, IPW = (ITEMS + 3) / 4;         // the bias items come last
    extern __shared__ __attribute__((aligned(16))) unsigned char gm_smem[];
    int* offs = reinterpret_cast<int*>(gm_smem);                                            // [TAPS][128]
    unsigned char* gt = gm_smem + TAPS * GM_TILE_PIX * 4;                                   // [3][gpix][PSG]
    const int TSG = pl.gpix * PSG, TSX = (pl.npmax + 1) * PSX, zero_off = pl.npmax * PSX;
    unsigned char* patch = gt + 3 * TSG;                                                    // [3][npmax + 1][PSX] (+ 16 bytes)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = (int)(blockIdx.x / pl.splits);
    const int split = (int)(blockIdx.x - (unsigned)grp * pl.splits);

    for (int e = tid; e < 3 * (PSX / 16); e += DW_THREADS) {                                // the zero pixel of every term
        const int term = e / (PSX / 16), sl = e - term * (PSX / 16);
        *reinterpret_cast<uint4*>(patch + term * TSX + zero_off + sl * 16) = make_uint4(0u, 0u, 0u, 0u);
    }

    // this wave's items it0 <= it < it1, decoded once: the row tile, and for a conv item the tap's table and the column tile's bytes
    const int it0 = (wave * ITEMS) >> 2, it1 = ((wave + 1) * ITEMS) >> 2;
    int irt[IPW], itab[IPW], icol[IPW];
    gm_f4 acc[IPW];
#pragma unroll
    for (int j = 0; j < IPW; ++j) {
        const int it = it0 + j;
        const int rt = it / (CT * TAPS), rem = it - rt * (CT * TAPS);
        const int ct = rem / TAPS;
        irt[j] = it < CONV ? rt : it - CONV;
        itab[j] = (rem - ct * TAPS) * GM_TILE_PIX;
        icol[j] = ct * 32;
        acc[j] = gm_f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    // lane l of a transposing read: pixel row 8 (l >> 4) + ((l & 15) >> 2) of the chunk (+ 4 for the second read), channels 4 (l & 3)
    const int prow = 8 * (lane >> 4) + ((lane & 15) >> 2), csub = (lane & 3) * 8;
    gm_bf8 ones, none;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        ones[k] = (__bf16)1.0f;
        none[k] = (__bf16)0.0f;
    }

    const int tiles = pl.tiles_r * pl.tiles_c;
    const int units = g.N * tiles;
    for (int u = split; u < units; u += pl.splits) {                 // uniform over the workgroup: so are the barriers
        const int n = u / tiles, tt = u - n * tiles;
        const int tr = tt / pl.tiles_c, tc = tt - tr * pl.tiles_c;
        const int r0 = tr * pl.TR, c0 = tc * pl.TC;
        const int TRa = gm_min(pl.TR, g.Hd - r0), TCa = gm_min(pl.TC, g.Wd - c0);
        const int npix = TRa * TCa;
        int lo_r, PH, lo_c, PW;
        gm_span(0, r0, r0 + TRa, g.s, g.ph, KS, g.Hs, lo_r, PH);
        gm_span(0, c0, c0 + TCa, g.s, g.pw, KS, g.Ws, lo_c, PW);
        __syncthreads();                                              // the previous tile has been read
        gmw_stage<NCBG>(go + n * gs.n + (int64_t)grp * COUT * gs.c + r0 * gs.h + c0 * gs.w, gs, pl.gvec, TCa, npix, pl.gpix, gt, TSG, tid);
        gmw_stage<NCBX>(x + n * xs.n + (int64_t)grp * CIN * xs.c + lo_r * xs.h + lo_c * xs.w, xs, g.vec, PW, PH * PW, PH * PW, patch, TSX,
                        tid);
        for (int e = tid; e < TAPS * GM_TILE_PIX; e += DW_THREADS) {
            const int t = e / GM_TILE_PIX, q = e - t * GM_TILE_PIX;
            const bool in = q < npix;
            const int qr = in ? q / TCa : 0;
            const int sr = (r0 + qr) * g.s - g.ph + t / KS, sc = (c0 + (in ? q - qr * TCa : 0)) * g.s - g.pw + (t - t / KS * KS);
            const bool ok = in && (unsigned)(sr - lo_r) < (unsigned)PH && (unsigned)(sc - lo_c) < (unsigned)PW;   // inside the image
            offs[e] = ok ? ((sr - lo_r) * PW + (sc - lo_c)) * PSX : zero_off;
        }
        __syncthreads();

        const int nch = (npix + 31) >> 5;
        for (int ch = 0; ch < nch; ++ch) {
            const int q = ch * 32 + prow;
            const unsigned char* ga = gt + q * PSG + csub;
            int prt = -1;
            gm_bf8 gh = none, gmid = none, gl = none;
#pragma unroll
            for (int j = 0; j < IPW; ++j) {
                if (it0 + j < it1) {                                  // wave-uniform, like every test on irt[]
                    if (irt[j] != prt) {
                        prt = irt[j];
                        const unsigned char* gp = ga + prt * 32;
                        gh = gmw_frag(gp, gp + 4 * PSG);
                        gmid = gmw_frag(gp + TSG, gp + TSG + 4 * PSG);
                        gl = gmw_frag(gp + 2 * TSG, gp + 2 * TSG + 4 * PSG);
                    }
                    gm_bf8 xh = ones, xm = none, xl = none;
                    if (it0 + j < CONV) {
                        const unsigned char* xa = patch + offs[itab[j] + q] + icol[j] + csub;
                        const unsigned char* xb = patch + offs[itab[j] + q + 4] + icol[j] + csub;
                        xh = gmw_frag(xa, xb);
                        xm = gmw_frag(xa + TSX, xb + TSX);
                        xl = gmw_frag(xa + 2 * TSX, xb + 2 * TSX);
                    }
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, gh, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, gh, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, gh, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, gmid, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, gmid, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, gl, acc[j], 0, 0, 0);
                }
            }
        }
    }

    // D[row = 4 (lane >> 4) + i][col = lane & 15]: 4 consecutive ci of output channel irt * 16 + (lane & 15)
    float* part = work + ((int64_t)split * g.G + grp) * gmw_block(TAPS, COUT, CIN);
#pragma unroll
    for (int j = 0; j < IPW; ++j) {
        if (it0 + j >= it1) continue;
        const int oc = irt[j] * 16 + (lane & 15);
        if (it0 + j < CONV) {
            const int ci = (icol[j] >> 1) + 4 * (lane >> 4);
            if (ci < CIN)                                             // the padded columns of cin_g = 24 are dropped here
                *reinterpret_cast<float4*>(part + ((int64_t)(itab[j] / GM_TILE_PIX) * COUT + oc) * CIN + ci) =
                    make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        } else if (lane < 16) {                                       // every row of a bias item holds the same sums
            part[TAPS * COUT * CIN + oc] = acc[j][0];
        }
    }
}

// second launch: the splits in index order, the STE mask on the unquantised weight (the rule of gc_grad_weight_combine_kernel), gw
// in the weight's own [G cout_g, cin_g, kh, kw] order, then gbias
__global__ __launch_bounds__(DW_THREADS) void gmw_reduce_kernel(const float* __restrict__ work, const float* __restrict__ w,
                                                                float* __restrict__ gw, float* __restrict__ gbias, int G, int cout_g,
                                                                int cin_g, int taps, int splits, float thr) {
    const int64_t blk = gmw_block(taps, cout_g, cin_g);
    const int64_t nw = (int64_t)G * cout_g * cin_g * taps, total = nw + (gbias ? (int64_t)G * cout_g : 0);
    for (int64_t e = (int64_t)blockIdx.x * DW_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * DW_THREADS) {
        int64_t co, at;                                               // the output channel and the element's place in a block
        if (e < nw) {
            co = e / (cin_g * taps);
            const int rem = (int)(e - co * (cin_g * taps)), ci = rem / taps, t = rem - ci * taps;
            at = ((int64_t)t * cout_g + co % cout_g) * cin_g + ci;
        } else {
            co = e - nw;
            at = (int64_t)taps * cout_g * cin_g + co % cout_g;
        }
        const float* p = work + (co / cout_g) * blk + at;
        const int64_t step = (int64_t)G * blk;
        float s = 0.0f;
        int sp = 0;
        for (; sp + 8 <= splits; sp += 8) {                           // eight loads in flight, added in index order all the same
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p[(sp + k) * step];
#pragma unroll
            for (int k = 0; k < 8; ++k) s = s + v[k];
        }
        for (; sp < splits; ++sp) s = s + p[sp * step];
        if (e >= nw) {
            gbias[co] = s;
        } else {
            if (thr > 0.0f && fabsf(w[e]) > thr) s = 0.0f;
            gw[e] = s;
        }
    }
}

template <int TAPS, int NCBX>
void gmw_launch(int rt, unsigned grid, hipStream_t s, const float* go, const float* x, float* work, const GmGeom& g, const DwStrides& gs,
                const DwStrides& xs, const GmwPlan& pl) {
#define GMW_GO(RT) gmw_kernel<TAPS, NCBX, RT><<<grid, DW_THREADS, (size_t)pl.lds_bytes, s>>>(go, x, work, g, gs, xs, pl)
    if (rt == 1) GMW_GO(1);
    else if (rt == 2) GMW_GO(2);
    else GMW_GO(3);
#undef GMW_GO
}

int gmw_entry(const float* go, const float* x, const float* w, float* gw, float* gbias, float* work, int64_t work_floats, int64_t N,
              int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
              int dw, const DwStrides& gs, const DwStrides& xs, float ste_threshold, qt_stream_t stream) {
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;
    if (!gw || (ste_threshold > 0.0f && !w) || !(ste_threshold >= 0.0f)) return QT_ERR_INVALID_ARG;
    if (!go || !x || !work || work_floats < 0) return QT_ERR_INVALID_ARG;
    if (dw_layout(N, G * cout_g, Ho, Wo, gs) < 0 || dw_layout(N, G * cin_g, H, W, xs) < 0) return QT_ERR_INVALID_ARG;
    GmGeom g = gmw_geom(N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw);
    const int taps = kh * kw, ncbx = (int)cin_g / 8, rt = (int)cout_g / 16;
    GmwPlan pl = gmw_plan(g, taps, ncbx, rt, 3);
    if (work_floats < (int64_t)pl.splits * G * gmw_block(taps, (int)cout_g, (int)cin_g)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(gw) || !dw_aligned4(gbias) || !dw_aligned4(w) || !dw_aligned4(go) || !dw_aligned4(x) || !qt_aligned16(work))
        return QT_ERR_ALIGNMENT;                                      // the partials are written as float4
    g.vec = xs.c == 1 && qt_aligned16(x) ? 1 : 0;
    pl.gvec = gs.c == 1 && qt_aligned16(go) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)(G * pl.splits);
    if (taps == 9) {
        if (ncbx == 2) gmw_launch<9, 2>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else if (ncbx == 3) gmw_launch<9, 3>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else gmw_launch<9, 4>(rt, grid, s, go, x, work, g, gs, xs, pl);
    } else {
        if (ncbx == 2) gmw_launch<1, 2>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else if (ncbx == 3) gmw_launch<1, 3>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else gmw_launch<1, 4>(rt, grid, s, go, x, work, g, gs, xs, pl);
    }
    const int st = qt_check_launch();
    if (st != QT_OK) return st;
    const int64_t total = G * cout_g * (cin_g * taps + 1);
    gmw_reduce_kernel<<<qt_stream_grid((total + DW_THREADS - 1) / DW_THREADS), DW_THREADS, 0, s>>>(
        work, w, gw, gbias, (int)G, (int)cout_g, (int)cin_g, taps, pl.splits, ste_threshold);
    return qt_check_launch();
}

}  // namespace

extern "C" int64_t qt_gmconv2d_grad_weight_work_floats(int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W,
                                                       int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw) {
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;      // an empty problem: 0
    const GmwPlan pl = gmw_plan(gmw_geom(N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw), kh * kw, (int)cin_g / 8, (int)cout_g / 16, 3);
    return (int64_t)pl.splits * G * gmw_block(kh * kw, (int)cout_g, (int)cin_g);
}

// What the launch of `op` would run for these numbers: the entry's steps 1 to 3 (gm_shape), then the plan functions the launches
// call.  The planes walk is reported by gp_describe (gconv_planes_mfma.hip).  No device call.
extern "C" int qt_gmconv2d_describe(int op, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw,
                                    int sh, int sw, int ph, int pw, int dh, int dw, char* out, int cap) {
    if (!out || cap < 2) return QT_ERR_INVALID_ARG;
    out[0] = 0;
    if (op == QT_GM_OP_PLANES) return gp_describe(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, out, cap);
    if (op != QT_GM_OP_FORWARD && op != QT_GM_OP_GRAD_INPUT && op != QT_GM_OP_GRAD_WEIGHT) return QT_ERR_INVALID_ARG;
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;      // an empty problem: no text
    const int taps = kh * kw;
    int shrunk[2] = {0, 0};
    if (op == QT_GM_OP_GRAD_WEIGHT) {
        const int ncbx = (int)cin_g / 8, rt = (int)cout_g / 16;
        const GmwPlan pl = gmw_plan(gmw_geom(N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw), taps, ncbx, rt, 3, shrunk);
        snprintf(out, (size_t)cap,
                 "kernel=gmw_kernel<%d,%d,%d> TR=%d TC=%d tiles_r=%d tiles_c=%d units=%lld splits=%d npmax=%d gpix=%d lds_bytes=%d "
                 "tr_shrunk=%d tc_shrunk=%d grid=%lld block=%d",
                 taps, ncbx, rt, pl.TR, pl.TC, pl.tiles_r, pl.tiles_c, (long long)(N * pl.tiles_r * pl.tiles_c), pl.splits, pl.npmax,
                 pl.gpix, pl.lds_bytes, shrunk[0], shrunk[1], (long long)(G * pl.splits), DW_THREADS);
        return QT_OK;
    }
    const GmGeom g = gm_geom(op == QT_GM_OP_GRAD_INPUT, N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw);
    const GmPlan pl = gm_plan(g, taps, g.KC / 8, 3, shrunk);
    snprintf(out, (size_t)cap,
             "kernel=gm_kernel<%d,%d> TR=%d TC=%d tiles_r=%d tiles_c=%d units=%lld splits=%d npmax=%d lds_bytes=%d tr_shrunk=%d "
             "tc_shrunk=%d grid=%lld block=%d",
             taps, g.KC / 8, pl.TR, pl.TC, pl.tiles_r, pl.tiles_c, (long long)(N * pl.tiles_r * pl.tiles_c), pl.splits, pl.npmax,
             pl.lds_bytes, shrunk[0], shrunk[1], (long long)(G * pl.splits), DW_THREADS);
    return QT_OK;
}

extern "C" int qt_gmconv2d_grad_weight_f32(const float* go, const float* x, const float* w, float* gw, float* gbias, float* work,
                                           int64_t work_floats, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
                                           int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t gs_n,
                                           int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c, int64_t xs_h,
                                           int64_t xs_w, float ste_threshold, qt_stream_t stream) {
    return gmw_entry(go, x, w, gw, gbias, work, work_floats, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                     DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, ste_threshold, stream);
}

extern "C" int qt_gmconv2d_f32(const float* x, const float* w, const float* bias, float* y, int64_t N, int64_t G, int64_t cin_g,
                               int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                               int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int64_t ys_n, int64_t ys_c, int64_t ys_h,
                               int64_t ys_w, int kind, qt_stream_t stream) {
    return gm_entry(false, x, w, bias, y, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                    DwStrides{xs_n, xs_c, xs_h, xs_w}, DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}

extern "C" int qt_gmconv2d_grad_input_f32(const float* go, const float* w, float* gx, int64_t N, int64_t G, int64_t cin_g,
                                          int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                          int dw, int64_t gs_n, int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c,
                                          int64_t xs_h, int64_t xs_w, int kind, qt_stream_t stream) {
    return gm_entry(true, go, w, nullptr, gx, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                    DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, kind, stream);
}
