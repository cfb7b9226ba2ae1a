// Grouped conv2d with 16, 24 or 32 input channels per group on the matrix cores, for bf16 / fp16 tensors: forward, grad_input and
// (below, "the weight gradient") grad_weight of conv2d(x, Q(w), bias, groups = G) where the activation IS an MFMA operand.  include/qt_hip.h "Grouped convolution on the matrix
// cores, half precision" states the contract; DESIGN.md "Grouped convs on the matrix cores, half precision" the layout, the counts
// and the measurements.  The gather, the tap table and the zero pixel are those of gconv_mfma.hip (gm_kernel):
//     dst[n, g NO + oc, r, c] = RNE( sum over taps t and k < KC of  src[n, g KC + k, sr(r, t), sc(c, t)] * Wq[oc, k, t]  + bias[oc] )
//   forward    : src = x, dst = y, KC = cin_g, NO = cout_g, sr = r s - p + i
//   grad_input : src = go, dst = gx, KC = cout_g, NO = cin_g, sr = (r + p - i) / s where that division is exact
// What differs is everything between HBM and the MFMA:
//   one term   : a 2-byte element goes into v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x32_f16 as it is — no split, ONE patch plane,
//                a third of the MFMAs and of the LDS of the fp32 kernel.  Q(w) in {-1, 0, +1} is exact in both types; a weight of the
//                activation's type is used as it is ("raw") or classified on its exact upcast; an fp32 weight (autocast) is quantised
//                and then rounded once, to nearest even, into the activation's type.  fp32 accumulation inside the MFMA, the fp32
//                bias added once, ONE rounding to nearest even into the output type (dw_st: the integer rounding for bf16,
//                v_cvt_f16_f32 for fp16).
//   stage      : no arithmetic.  A thread owns (source pixel, block of 8 channels).  Channels-last and 16-byte aligned (g.vec): one
//                16-byte global load is the block, stored to LDS unchanged.  Otherwise (NCHW: lanes along W; a channels-last view at
//                an odd element offset: lanes along the blocks of a pixel) eight 2-byte loads, all issued before the first is used
//                (dw_loads_issued), packed into one 16-byte LDS store.
//   plan       : gm_plan with one term: the LDS budget loop shrinks a tile far less often and a workgroup holds about a third of the
//                fp32 kernel's LDS, so more workgroups fit a CU.
//   main loop  : with one term LDS reads, not MFMAs, would bound the fp32 loop's shape (2 MFMAs per 3 fragment reads).  Here the B
//                fragments of a wave's column tile live in REGISTERS (at most 14 chunks x 4 VGPRs at KC = 48) and the wave walks
//                (pair of 16-pixel row tiles) items under them: item `it` of a tile is column tile it % nct, row-tile pair it / nct,
//                waves take it = wave, wave + 4, ...  With one or two column tiles (NO <= 32) a wave's column tile never changes: its
//                B fragments are read from LDS ONCE PER WORKGROUP and kept across the whole (image, tile) walk — one fragment read
//                per MFMA.  With three (cout_g = 48 forward) they are re-read per item: 3 reads per 2 MFMAs.
//   stores     : a lane's accumulator quad is 4 consecutive pixels of one channel; four guarded 2-byte stores in both layouts
//                (neighbouring lanes are not paired into 4-byte stores).
// Non-finite inputs: an inf / NaN element poisons every output whose window holds it, also through a ZERO weight (0 * inf = NaN);
// through a +-1 weight an inf stays +-inf (the one-term product is exact).
#include "qt_common.h"
#include "dw_map.h"
#include "gm_plan.h"

namespace {

typedef __bf16 gh_bf8 __attribute__((ext_vector_type(8)));
typedef _Float16 gh_h8 __attribute__((ext_vector_type(8)));
typedef float gh_f4 __attribute__((ext_vector_type(4)));

// one MFMA on two fragments of eight T elements each, held as their 16 bytes
template <typename T>
__device__ __forceinline__ gh_f4 gh_mfma(const uint4& a, const uint4& b, gh_f4 c) {
    if constexpr (std::is_same<T, DwBf16>::value) {
        gh_bf8 x, y;
        __builtin_memcpy(&x, &a, 16);
        __builtin_memcpy(&y, &b, 16);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, c, 0, 0, 0);
    } else {
        gh_h8 x, y;
        __builtin_memcpy(&x, &a, 16);
        __builtin_memcpy(&y, &b, 16);
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(x, y, c, 0, 0, 0);
    }
}

// the pattern of v rounded to nearest even into T
template <typename T>
__device__ __forceinline__ uint32_t gh_bits(float v) {
    T t;
    dw_st(&t, v);
    uint16_t b;
    __builtin_memcpy(&b, &t, 2);
    return b;
}

// src and the patch are handled as 16-bit patterns; T names the MFMA and the rounding of the result.  w: T or (w_f32) float.
template <int TAPS, int NCB, typename T>
__global__ __launch_bounds__(DW_THREADS) void gh_kernel(const uint16_t* __restrict__ src, const void* __restrict__ w, int w_f32,
                                                        const float* __restrict__ bias, T* __restrict__ dst, GmGeom g, DwStrides ss,
                                                        DwStrides ds, GmPlan pl, int kind) {
    constexpr int KC = NCB * 8, PAIRS = TAPS * NCB, NCHUNK = (PAIRS + 3) / 4, PS = gm_ps(NCB);
    constexpr int KS = TAPS == 9 ? 3 : 1;                            // kernel side
    extern __shared__ __attribute__((aligned(16))) unsigned char gh_smem[];
    uint4* wl = reinterpret_cast<uint4*>(gh_smem);                   // [NCHUNK * 4][nopad]
    int* offs = reinterpret_cast<int*>(gh_smem + pl.w_bytes);        // [TAPS][128]
    int* outq = offs + TAPS * GM_TILE_PIX;                           // [128]
    unsigned char* patch = reinterpret_cast<unsigned char*>(outq + GM_TILE_PIX);          // [npmax + 1][PS]
    const int zero_off = pl.npmax * PS;
    const int tid = threadIdx.x;
    const int grp = (int)(blockIdx.x / pl.splits);
    const int split = (int)(blockIdx.x - (unsigned)grp * pl.splits);

    // once: the group's weights as B fragments, the zero pixel
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
                const float wv = w_f32 ? static_cast<const float*>(w)[idx] : dw_ld(static_cast<const T*>(w)[idx]);
                h[k >> 1] |= gh_bits<T>(dw_quant(kind, wv)) << (16 * (k & 1));
            }
        }
        wl[e] = make_uint4(h[0], h[1], h[2], h[3]);
    }
    for (int e = tid; e < PS / 16; e += DW_THREADS) *reinterpret_cast<uint4*>(patch + zero_off + e * 16) = make_uint4(0u, 0u, 0u, 0u);

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, lrow = lane & 15, kb = lane >> 4;
    const int nct = pl.nopad >> 4;                                    // column tiles: 1, 2 or 3
    uint4 breg[NCHUNK];                                               // the B fragments of column tile `cur`, one per K chunk
    int cur = -1;
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
        const uint16_t* sbase = src + n * ss.n + (int64_t)grp * KC * ss.c + lo_r * ss.h + lo_c * ss.w;
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
            const uint16_t* sp = sbase + row * ss.h + col * ss.w + cb * 8 * ss.c;
            uint4 v;
            if (g.vec) {
                v = *reinterpret_cast<const uint4*>(sp);
            } else {
                uint32_t h[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) h[k] = sp[k * ss.c];
                dw_loads_issued<T, 8>();
                v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
            *reinterpret_cast<uint4*>(patch + pp * PS + cb * 16) = v;
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
        const int items = npp * nct;
        for (int it = wave; it < items; it += DW_THREADS / 64) {      // wave-uniform, like nt and the test on `cur`
            const int pp = it / nct, nt = it - pp * nct;
            if (nt != cur) {
                cur = nt;
#pragma unroll
                for (int ch = 0; ch < NCHUNK; ++ch) breg[ch] = wl[(4 * ch + kb) * pl.nopad + nt * 16 + lrow];
            }
            const int q0 = pp * 32 + lrow;
            gh_f4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ch = 0; ch < NCHUNK; ++ch) {
                const int p = 4 * ch + kb;                            // the lane's pair of this chunk
                const int t = p / NCB, cb = p - t * NCB;
                const bool live = p < PAIRS;                          // a padding pair reads the zero pixel (its weights are zero too)
                const int ti = live ? t * GM_TILE_PIX : 0;
                const int o0 = (live ? offs[ti + q0] : zero_off) + cb * 16;
                const int o1 = (live ? offs[ti + q0 + 16] : zero_off) + cb * 16;
                const uint4 a0 = *reinterpret_cast<const uint4*>(patch + o0);
                const uint4 a1 = *reinterpret_cast<const uint4*>(patch + o1);
                acc0 = gh_mfma<T>(a0, breg[ch], acc0);
                acc1 = gh_mfma<T>(a1, breg[ch], acc1);
            }
            // D[row = 4 kb + i][col = lrow]: 4 consecutive pixels of output channel nt * 16 + lrow
            const int oc = nt * 16 + lrow;
            if (oc < g.NO) {
                const int64_t ch = (int64_t)grp * g.NO + oc;
                T* dp = dst + n * ds.n + ch * ds.c;
                const float bv = bias ? bias[ch] : 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int oa = outq[pp * 32 + kb * 4 + i], ob = outq[pp * 32 + 16 + kb * 4 + i];
                    if (oa >= 0) dw_st(dp + oa, bias ? acc0[i] + bv : acc0[i]);
                    if (ob >= 0) dw_st(dp + ob, bias ? acc1[i] + bv : acc1[i]);
                }
            }
        }
    }
}

template <int TAPS, typename T>
int gh_launch(int ncb, const void* src, const void* w, int w_f32, const float* bias, void* dst, const GmGeom& g, const DwStrides& ss,
              const DwStrides& ds, int kind, hipStream_t s) {
    const GmPlan pl = gm_plan(g, TAPS, ncb, 1);
    const unsigned grid = (unsigned)((int64_t)g.G * pl.splits);
#define GH_GO(NCB)                                                                                                                   \
    gh_kernel<TAPS, NCB, T><<<grid, DW_THREADS, (size_t)pl.lds_bytes, s>>>(static_cast<const uint16_t*>(src), w, w_f32, bias,        \
                                                                          static_cast<T*>(dst), g, ss, ds, pl, kind)
    if (ncb == 2) GH_GO(2);
    else if (ncb == 3) GH_GO(3);
    else if (ncb == 4) GH_GO(4);
    else GH_GO(6);
#undef GH_GO
    return qt_check_launch();
}

bool gh_aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// The validation of the two entries, in the documented order.  in / out: the tensor read (x, go) and the one written (y, gx).
int gh_entry(bool bwd, const void* in, int dtype, const void* w, int w_dtype, const float* bias, void* out, int64_t N, int64_t G,
             int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
             const DwStrides& is, const DwStrides& os, int kind, qt_stream_t stream) {
    if (dtype != QT_DTYPE_BF16 && dtype != QT_DTYPE_F16) return QT_ERR_INVALID_ARG;
    if (w_dtype != dtype && w_dtype != QT_DTYPE_F32) return QT_ERR_INVALID_ARG;
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;
    const int64_t Cin = G * cin_g, Cout = G * cout_g;
    if (kind != QT_DW_RAW && kind != QT_DW_SIGN && kind != QT_DW_TERNARY) return QT_ERR_INVALID_ARG;
    if (!in || !w || !out) return QT_ERR_INVALID_ARG;
    const DwStrides& xs = bwd ? os : is;
    const DwStrides& ys = bwd ? is : os;
    if (dw_layout(N, Cin, H, W, xs) < 0 || dw_layout(N, Cout, Ho, Wo, ys) < 0) return QT_ERR_INVALID_ARG;
    const int w_f32 = w_dtype == QT_DTYPE_F32;
    if (!gh_aligned(in, 2) || !gh_aligned(out, 2) || !gh_aligned(w, w_f32 ? 4 : 2) || !dw_aligned4(bias)) return QT_ERR_ALIGNMENT;
    GmGeom g = gm_geom(bwd, N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw);
    g.vec = is.c == 1 && qt_aligned16(in) ? 1 : 0;                 // a pixel is G KC 2 bytes, KC a multiple of 8: every block on 16 bytes
    hipStream_t s = (hipStream_t)stream;
    const int ncb = g.KC / 8;
    if (dtype == QT_DTYPE_BF16)
        return kh == 3 ? gh_launch<9, DwBf16>(ncb, in, w, w_f32, bias, out, g, is, os, kind, s)
                       : gh_launch<1, DwBf16>(ncb, in, w, w_f32, bias, out, g, is, os, kind, s);
    return kh == 3 ? gh_launch<9, DwF16>(ncb, in, w, w_f32, bias, out, g, is, os, kind, s)
                   : gh_launch<1, DwF16>(ncb, in, w, w_f32, bias, out, g, is, os, kind, s);
}

// ---- the weight gradient ------------------------------------------------------------------------------------------------------------
//     gw[g cout_g + oc, ci, i, j] = sum over (n, ho, wo) of  go[n, g cout_g + oc, ho, wo] * x[n, g cin_g + ci, ho s - p + i, wo s - p + j]
// for bf16 / fp16 go and x: BOTH are MFMA operands as they are, so a (go, x) pair is ONE product where gmw_kernel (gconv_mfma.hip)
// needs six.  The launch shape, the walk, the tap table, the zero pixel, the transposing fragment reads and the partial layout are
// gmw_kernel's; a kernel of its own because that loop, with the split taken out, would issue 2 - 4 transposing LDS reads per MFMA:
//   stage   : no arithmetic, ONE plane per operand, [pixel][channels (+ pad)]: gh_kernel's stage (16-byte loads where the tensor is
//             channels-last and 16-byte aligned, else eight 2-byte loads issued together), go pixels past the tile end are zero.
//   items   : a wave's items are (tap, column tile of 16 ci) PAIRS, dealt to the four waves in contiguous balanced runs, and it
//             keeps an accumulator per (pair, row tile of 16 oc): at most 5 x 3 quads.  Per 32-pixel chunk it reads the go
//             fragments of ALL row tiles once into registers (at most 3), then per pair the x fragment once, used against every
//             row tile: cout_g / 16 MFMAs per two transposing reads.  A wave's neighbouring pairs are the column tiles of one tap,
//             so they share the tap's table words.  The bias item (go against a register fragment of ones, one MFMA per row tile)
//             is wave 0's, whose run is never the longest.
//   count   : per workgroup and chunk at 32 -> 32 channels, 3 x 3: 36 x reads + 16 go reads for 38 MFMAs (a count, not a
//             measurement).
// Roles as there: x is the A operand (rows = ci), go the B operand (columns = oc), a lane's accumulator quad is 4 consecutive ci of
// one oc: one float4 of the partial [split][g][tap][oc][ci] (+ [oc]).  gwh_reduce_kernel is gmw_reduce_kernel with the store (and the
// weight of the STE mask) typed on w_dtype.

typedef short gh_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) gh_s4 gh_lds_s4;

// the fragment of the two transposing reads (ds_read_b64_tr_b16) at LDS bytes a and b: elements 0-3 from a, 4-7 from b
__device__ __forceinline__ uint4 gwh_frag(const unsigned char* a, const unsigned char* b) {
    const gh_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gh_lds_s4*)a);
    const gh_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gh_lds_s4*)b);
    uint4 f;
    __builtin_memcpy(&f, &lo, 8);
    __builtin_memcpy(reinterpret_cast<unsigned char*>(&f) + 8, &hi, 8);
    return f;
}

// Stage pixels [0, nfill) of a PW-wide box at `base` (8 NCB channels from there) into dst[pixel][PS]: pixels below np are read as
// they are, the others are zero.  Lanes as in gh_kernel's stage.
template <int NCB, typename T>
__device__ __forceinline__ void gwh_stage(const uint16_t* __restrict__ base, const DwStrides& st, int vec, int PW, int np, int nfill,
                                          unsigned char* dst, int tid) {
    constexpr int PS = gm_ps(NCB);
    for (int e = tid; e < nfill * NCB; e += DW_THREADS) {
        int cb, pp;
        if (st.c == 1) {                                              // channels-last: the blocks of a pixel on consecutive lanes
            pp = e / NCB;
            cb = e - pp * NCB;
        } else {                                                      // NCHW: consecutive lanes along W
            cb = e / nfill;
            pp = e - cb * nfill;
        }
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (pp < np) {
            const int row = pp / PW, col = pp - row * PW;
            const uint16_t* sp = base + row * st.h + col * st.w + cb * 8 * st.c;
            if (vec) {
                v = *reinterpret_cast<const uint4*>(sp);
            } else {
                uint32_t h[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) h[k] = sp[k * st.c];
                dw_loads_issued<T, 8>();
                v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
        }
        *reinterpret_cast<uint4*>(dst + pp * PS + cb * 16) = v;
    }
}

// NCBX: blocks of 8 input channels of a group (2, 3, 4); RT: row tiles of 16 output channels (1, 2, 3); T names the MFMA
template <int TAPS, int NCBX, int RT, typename T>
__global__ __launch_bounds__(DW_THREADS) void gwh_kernel(const uint16_t* __restrict__ go, const uint16_t* __restrict__ x,
                                                         float* __restrict__ work, GmGeom g, DwStrides gs, DwStrides xs, GmwPlan pl) {
    constexpr int CIN = NCBX * 8, COUT = RT * 16, CT = (NCBX + 1) / 2, NCBG = RT * 2, PSX = gm_ps(NCBX), PSG = gm_ps(NCBG);
    constexpr int KS = TAPS == 9 ? 3 : 1;
    constexpr int NP = TAPS * CT, PPW = (NP + 3) / 4;                 // (tap, column tile) pairs; the most a wave gets
    extern __shared__ __attribute__((aligned(16))) unsigned char gh_smem[];
    int* offs = reinterpret_cast<int*>(gh_smem);                      // [TAPS][128]
    unsigned char* gt = gh_smem + TAPS * GM_TILE_PIX * 4;             // [gpix][PSG]
    unsigned char* patch = gt + pl.gpix * PSG;                        // [npmax + 1][PSX] (+ 16 bytes)
    const int zero_off = pl.npmax * PSX;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = (int)(blockIdx.x / pl.splits);
    const int split = (int)(blockIdx.x - (unsigned)grp * pl.splits);

    for (int e = tid; e < PSX / 16; e += DW_THREADS) *reinterpret_cast<uint4*>(patch + zero_off + e * 16) = make_uint4(0u, 0u, 0u, 0u);

    // this wave's pairs p0 <= p < p1, decoded once: the tap's table and the column tile's bytes
    const int p0 = (wave * NP) >> 2, p1 = ((wave + 1) * NP) >> 2;
    const bool biased = wave == 0;
    int itab[PPW], icol[PPW];
    gh_f4 acc[PPW][RT], accb[RT];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        const int t = (p0 + j) / CT;
        itab[j] = t * GM_TILE_PIX;
        icol[j] = (p0 + j - t * CT) * 32;
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[j][r] = gh_f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) accb[r] = gh_f4{0.0f, 0.0f, 0.0f, 0.0f};
    // lane l of a transposing read: pixel row 8 (l >> 4) + ((l & 15) >> 2) of the chunk (+ 4 for the second read), channels 4 (l & 3)
    const int prow = 8 * (lane >> 4) + ((lane & 15) >> 2), csub = (lane & 3) * 8;
    const uint32_t one2 = gh_bits<T>(1.0f) * 0x10001u;
    const uint4 ones = make_uint4(one2, one2, one2, one2);

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
        gwh_stage<NCBG, T>(go + n * gs.n + (int64_t)grp * COUT * gs.c + r0 * gs.h + c0 * gs.w, gs, pl.gvec, TCa, npix, pl.gpix, gt, tid);
        gwh_stage<NCBX, T>(x + n * xs.n + (int64_t)grp * CIN * xs.c + lo_r * xs.h + lo_c * xs.w, xs, g.vec, PW, PH * PW, PH * PW, patch, tid);
        for (int e = tid; e < TAPS * GM_TILE_PIX; e += DW_THREADS) {
            const int t = e / GM_TILE_PIX, q = e - t * GM_TILE_PIX;
            const bool in = q < npix;
            const int qr = in ? q / TCa : 0;
            const int sr = (r0 + qr) * g.s - g.ph + t / KS, sc = (c0 + (in ? q - qr * TCa : 0)) * g.s - g.pw + (t - t / KS * KS);
            const bool ok = in && (unsigned)(sr - lo_r) < (unsigned)PH && (unsigned)(sc - lo_c) < (unsigned)PW;   // inside the image
            offs[e] = ok ? ((sr - lo_r) * PW + (sc - lo_c)) * PSX : zero_off;
        }
        __syncthreads();

        if (p0 < p1 || biased) {                                      // wave-uniform, like every test on p0 + j
            const int nch = (npix + 31) >> 5;
            for (int ch = 0; ch < nch; ++ch) {
                const int q = ch * 32 + prow;
                const unsigned char* ga = gt + q * PSG + csub;
                uint4 gf[RT];
#pragma unroll
                for (int r = 0; r < RT; ++r) gf[r] = gwh_frag(ga + r * 32, ga + r * 32 + 4 * PSG);
#pragma unroll
                for (int j = 0; j < PPW; ++j) {
                    if (p0 + j < p1) {
                        const uint4 xf = gwh_frag(patch + offs[itab[j] + q] + icol[j] + csub, patch + offs[itab[j] + q + 4] + icol[j] + csub);
#pragma unroll
                        for (int r = 0; r < RT; ++r) acc[j][r] = gh_mfma<T>(xf, gf[r], acc[j][r]);
                    }
                }
                if (biased) {
#pragma unroll
                    for (int r = 0; r < RT; ++r) accb[r] = gh_mfma<T>(ones, gf[r], accb[r]);
                }
            }
        }
    }

    // D[row = 4 (lane >> 4) + i][col = lane & 15]: 4 consecutive ci of output channel r * 16 + (lane & 15)
    float* part = work + ((int64_t)split * g.G + grp) * gmw_block(TAPS, COUT, CIN);
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        if (p0 + j >= p1) continue;
        const int ci = (icol[j] >> 1) + 4 * (lane >> 4);
        if (ci >= CIN) continue;                                      // the padded columns of cin_g = 24 are dropped here
#pragma unroll
        for (int r = 0; r < RT; ++r)
            *reinterpret_cast<float4*>(part + ((int64_t)(itab[j] / GM_TILE_PIX) * COUT + r * 16 + (lane & 15)) * CIN + ci) =
                make_float4(acc[j][r][0], acc[j][r][1], acc[j][r][2], acc[j][r][3]);
    }
    if (biased && lane < 16) {                                        // every row of a bias item holds the same sums
#pragma unroll
        for (int r = 0; r < RT; ++r) part[TAPS * COUT * CIN + r * 16 + lane] = accb[r][0];
    }
}

// second launch: gmw_reduce_kernel's sums (the splits in index order, eight loads in flight), the STE mask on the exact upcast of
// the unquantised weight, ONE rounding to nearest even into WT (a float WT stores the fp32 sum)
template <typename WT>
__global__ __launch_bounds__(DW_THREADS) void gwh_reduce_kernel(const float* __restrict__ work, const WT* __restrict__ w,
                                                                WT* __restrict__ gw, WT* __restrict__ gbias, int G, int cout_g,
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
        for (; sp + 8 <= splits; sp += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p[(sp + k) * step];
#pragma unroll
            for (int k = 0; k < 8; ++k) s = s + v[k];
        }
        for (; sp < splits; ++sp) s = s + p[sp * step];
        if (e >= nw) {
            dw_st(gbias + co, s);
        } else {
            if (thr > 0.0f && fabsf(dw_ld(w[e])) > thr) s = 0.0f;
            dw_st(gw + e, s);
        }
    }
}

template <int TAPS, int NCBX, typename T>
void gwh_launch(int rt, unsigned grid, hipStream_t s, const void* go, const void* x, float* work, const GmGeom& g, const DwStrides& gs,
                const DwStrides& xs, const GmwPlan& pl) {
#define GWH_GO(RT)                                                                                                                   \
    gwh_kernel<TAPS, NCBX, RT, T><<<grid, DW_THREADS, (size_t)pl.lds_bytes, s>>>(static_cast<const uint16_t*>(go),                   \
                                                                                static_cast<const uint16_t*>(x), work, g, gs, xs, pl)
    if (rt == 1) GWH_GO(1);
    else if (rt == 2) GWH_GO(2);
    else GWH_GO(3);
#undef GWH_GO
}

template <typename T>
void gwh_launch_t(int taps, int ncbx, int rt, unsigned grid, hipStream_t s, const void* go, const void* x, float* work, const GmGeom& g,
                  const DwStrides& gs, const DwStrides& xs, const GmwPlan& pl) {
    if (taps == 9) {
        if (ncbx == 2) gwh_launch<9, 2, T>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else if (ncbx == 3) gwh_launch<9, 3, T>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else gwh_launch<9, 4, T>(rt, grid, s, go, x, work, g, gs, xs, pl);
    } else {
        if (ncbx == 2) gwh_launch<1, 2, T>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else if (ncbx == 3) gwh_launch<1, 3, T>(rt, grid, s, go, x, work, g, gs, xs, pl);
        else gwh_launch<1, 4, T>(rt, grid, s, go, x, work, g, gs, xs, pl);
    }
}

// The validation of the weight-gradient entry, in the documented order: the dtypes, gm_shape, then gmw_entry's checks.
int gwh_entry(const void* go, const void* x, int dtype, const void* w, void* gw, void* gbias, int w_dtype, float* work,
              int64_t work_floats, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh,
              int sw, int ph, int pw, int dh, int dw, const DwStrides& gs, const DwStrides& xs, float ste_threshold, qt_stream_t stream) {
    if (dtype != QT_DTYPE_BF16 && dtype != QT_DTYPE_F16) return QT_ERR_INVALID_ARG;
    if (w_dtype != dtype && w_dtype != QT_DTYPE_F32) return QT_ERR_INVALID_ARG;
    int64_t Ho, Wo;
    int rc;
    if (!gm_shape(N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;
    if (!gw || (ste_threshold > 0.0f && !w) || !(ste_threshold >= 0.0f)) return QT_ERR_INVALID_ARG;
    if (!go || !x || !work || work_floats < 0) return QT_ERR_INVALID_ARG;
    if (dw_layout(N, G * cout_g, Ho, Wo, gs) < 0 || dw_layout(N, G * cin_g, H, W, xs) < 0) return QT_ERR_INVALID_ARG;
    GmGeom g = gmw_geom(N, G, cin_g, cout_g, H, W, Ho, Wo, sh, ph, pw);
    const int taps = kh * kw, ncbx = (int)cin_g / 8, rt = (int)cout_g / 16;
    const int64_t blk = gmw_block(taps, (int)cout_g, (int)cin_g);
    // The workspace asked for is that of qt_gmconv2d_grad_weight_work_floats: the three-term plan's.  The launch uses a PREFIX of
    // it: a one-term tile is never smaller than the three-term tile (gmw_plan), so there are never more units or splits.
    if (work_floats < (int64_t)gmw_plan(g, taps, ncbx, rt, 3).splits * G * blk) return QT_ERR_INVALID_ARG;
    const unsigned wa = w_dtype == QT_DTYPE_F32 ? 4 : 2;
    if (!gh_aligned(gw, wa) || !gh_aligned(gbias, wa) || !gh_aligned(w, wa) || !gh_aligned(go, 2) || !gh_aligned(x, 2) ||
        !qt_aligned16(work))
        return QT_ERR_ALIGNMENT;                                      // the partials are written as float4
    GmwPlan pl = gmw_plan(g, taps, ncbx, rt, 1);
    g.vec = xs.c == 1 && qt_aligned16(x) ? 1 : 0;                  // a pixel's group block is a multiple of 16 bytes in both tensors
    pl.gvec = gs.c == 1 && qt_aligned16(go) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)(G * pl.splits);
    if (dtype == QT_DTYPE_BF16) gwh_launch_t<DwBf16>(taps, ncbx, rt, grid, s, go, x, work, g, gs, xs, pl);
    else gwh_launch_t<DwF16>(taps, ncbx, rt, grid, s, go, x, work, g, gs, xs, pl);
    const int st = qt_check_launch();
    if (st != QT_OK) return st;
    const int64_t total = G * cout_g * (cin_g * taps + 1);
    const unsigned rgrid = qt_stream_grid((total + DW_THREADS - 1) / DW_THREADS);
#define GWH_REDUCE(WT)                                                                                                               \
    gwh_reduce_kernel<WT><<<rgrid, DW_THREADS, 0, s>>>(work, static_cast<const WT*>(w), static_cast<WT*>(gw), static_cast<WT*>(gbias), \
                                                      (int)G, (int)cout_g, (int)cin_g, taps, pl.splits, ste_threshold)
    if (w_dtype == QT_DTYPE_F32) GWH_REDUCE(float);
    else if (dtype == QT_DTYPE_BF16) GWH_REDUCE(DwBf16);
    else GWH_REDUCE(DwF16);
#undef GWH_REDUCE
    return qt_check_launch();
}

}  // namespace

extern "C" int qt_gmconv2d_grad_weight_h(const void* go, const void* x, int dtype, const void* w, void* gw, void* gbias, int w_dtype,
                                         float* work, int64_t work_floats, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
                                         int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t gs_n,
                                         int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w,
                                         float ste_threshold, qt_stream_t stream) {
    return gwh_entry(go, x, dtype, w, gw, gbias, w_dtype, work, work_floats, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                     DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, ste_threshold, stream);
}

extern "C" int qt_gmconv2d_h(const void* x, int dtype, const void* w, int w_dtype, const float* bias, void* y, int64_t N, int64_t G,
                             int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                             int dw, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int64_t ys_n, int64_t ys_c, int64_t ys_h,
                             int64_t ys_w, int kind, qt_stream_t stream) {
    return gh_entry(false, x, dtype, w, w_dtype, bias, y, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                    DwStrides{xs_n, xs_c, xs_h, xs_w}, DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}

extern "C" int qt_gmconv2d_grad_input_h(const void* go, int dtype, const void* w, int w_dtype, void* gx, int64_t N, int64_t G,
                                        int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                                        int pw, int dh, int dw, int64_t gs_n, int64_t gs_c, int64_t gs_h, int64_t gs_w, int64_t xs_n,
                                        int64_t xs_c, int64_t xs_h, int64_t xs_w, int kind, qt_stream_t stream) {
    return gh_entry(true, go, dtype, w, w_dtype, nullptr, gx, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                    DwStrides{gs_n, gs_c, gs_h, gs_w}, DwStrides{xs_n, xs_c, xs_h, xs_w}, kind, stream);
}
