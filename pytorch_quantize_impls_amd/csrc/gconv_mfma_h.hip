// Grouped conv2d with 16, 24 or 32 input channels per group on the matrix cores, for bf16 / fp16 tensors: forward and grad_input of
// conv2d(x, Q(w), bias, groups = G) where the activation IS an MFMA operand.  include/qt_hip.h "Grouped convolution on the matrix
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

}  // namespace

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
