// Grouped conv2d with 16 or 32 input channels per group on the bit planes of a +-1 activation, on the int8 matrix cores: the
// grouped BinConv2d / TerConv2d of the last ResNeXt stages inside the fused sign chain.  include/qt_hip.h "Grouped convolution on
// bit planes, on the matrix cores" states the contract; DESIGN.md "Grouped convs on bit planes, on the matrix cores" the layout,
// the resources and what was measured.
//
// With 16 or 32 channels per group a group's operand at one tap is an aligned 16- or 32-bit field of the producer's sign plane,
// the classified weights are -1 / 0 / +1 and every sum is an integer of magnitude <= 288: v_mfma_i32_16x16x64_i8 computes it
// exactly.  Rows of the MFMA are 16 consecutive output pixels, columns 16 output channels of the group, and its K = 64 bytes are
// four K BLOCKS of 16 channels: block kb is tap kb / (cin_g / 16), half-word kb % (cin_g / 16) of the group's field.  Lane l holds
// row / column l & 15 and K block l >> 4 of a step, so a lane's 16 operand bytes are one 16-channel half-tap.  (Any permutation of
// the 64 K positions the hardware applied would apply to both operands alike; both are built by this one rule.)
//
// Work split.  A WAVE owns one group for the whole launch and walks 16-pixel tiles split, split + S, ... of the flat (n, ho, wo)
// index with constant increments and two carries (the walk of gc_planes_kernel: no division per tile).  Wave w of the grid is
// (split w / G, group w % G): the four waves of a workgroup are four neighbouring groups on the SAME pixels — they read
// neighbouring fields of the same plane rows and write neighbouring pieces of the same output rows — or, where G < 4, pixel ranges
// of the same groups.  Waves never meet: no LDS, no barrier.
//   B (weights) : once per wave, from the fp32 image: lane (column p, block q) classifies the 16 weights of output channel
//                 ct 16 + p at K block 4 s + q (`kind`, dw_quant) into bytes 0x01 / 0x00 / 0xFF, for every column tile ct and
//                 step s; K blocks past taps * cin_g / 16 are zero.  cout_g / 16 x steps x 4 registers, at most 3 x 5 x 4 = 60.
//   A (pixels)  : per tile and step the lane (pixel p, block q) loads the plane word of its tap's input pixel — all loads of a
//                 tile go out together; a tap outside the image loads the nearest pixel inside it — and expands its 16-bit field
//                 into 16 bytes +1 = 0x01 / -1 = 0xFF with a multiply per nibble (gp_expand4); a tap outside the image, and a K
//                 block past the taps, is ANDed to sixteen zero bytes.  Bit tricks, not an LDS table: 5 VALU operations per 4
//                 bytes against an LDS read whose latency every step would wait for, and the waves stay free of LDS and barriers.
//                 The fragment feeds all cout_g / 16 column tiles.
//   epilogue    : the int32 accumulator quad of a lane is channel ct 16 + p of pixels 4 q + i.  (float)S is exact; bias, alpha
//                 and beta are three fp32 roundings (the build has -ffp-contract=off); one ballot per (i, ct) holds the 16-bit
//                 channel fields of four pixels.  Lane (p < cout_g / 16, q) writes the field of column tile p of pixel 4 q + i:
//                 one aligned 2-byte store into the sign plane, one aligned 8-byte store (16 nibbles) into the nibble plane.
//                 The waves of the LAST group also write the zero bits and pad words behind G cout_g channels.  Different waves
//                 write different bytes of a word: nothing is read back, nothing is atomic.  The border of a halo plane is
//                 zeroed by dw_zero_border (dw_planes.h); the nibble row of a pixel comes by one cross-lane read per i from the
//                 lane that walks that pixel.
#include <cstdio>

#include "qt_common.h"
#include "dw_planes.h"
#include "gm_describe.h"

namespace {

typedef int gp_i4 __attribute__((ext_vector_type(4)));

constexpr int GP_WAVES = DW_THREADS / 64;
constexpr int GP_TILE = 16;                      // output pixels of a tile: the rows of one MFMA
constexpr int GP_TARGET_WGS = 1024;              // workgroups of a launch: 4 per CU, so that a wave's weight pass is amortised
constexpr int64_t GP_MAX_ROWS = (int64_t)1 << 31;

struct GpWalk {
    int G, splits, units;
    int d_n, d_ho, d_wo;                         // what a step of splits * 16 pixels adds to (n, ho, wo), before the carries
};

// bits 0 .. 3 of `nib` -> four bytes, bit k -> byte k: 0 -> 0x01 (+1), 1 -> 0xFF (-1).  The multiply puts bit k at 8 k (the four
// shifted copies never overlap: no carry).
__device__ __forceinline__ uint32_t gp_expand4(uint32_t nib) {
    const uint32_t m = ((nib & 0xFu) * 0x00204081u) & 0x01010101u;
    return (m * 0xFFu) | 0x01010101u;
}

template <int TAPS, int CB, int NCT>
__global__ __launch_bounds__(DW_THREADS) void gp_kernel(const uint32_t* __restrict__ xb, int64_t ldx, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ alpha,
                                                        const float* __restrict__ beta, DwPlaneOut o, DwGeom g, DwStrides ys,
                                                        GpWalk wk, int kind) {
    constexpr int KB = TAPS * CB;                // live K blocks of 16 channels
    constexpr int STEPS = (KB + 3) / 4;
    constexpr int CIN_G = 16 * CB, COUT_G = 16 * NCT;
    constexpr int KW = TAPS == 9 ? 3 : 1;
    const int tid = threadIdx.x, lane = tid & 63, p = lane & 15, q = lane >> 4;
    const int wave = (int)blockIdx.x * GP_WAVES + __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave < wk.G * wk.splits) {
        const int split = wave / wk.G, grp = wave - split * wk.G;
        // ---- B: the group's classified weights, resident
        gp_i4 B[NCT][STEPS];
        // a real loop over (ct, s) with the registers picked by compile-time selects: the (branching) quantiser exists once, not
        // NCT x STEPS times, and 16 loads are in flight at a time
#pragma unroll 1
        for (int it = 0; it < NCT * STEPS; ++it) {
            const int ct = it / STEPS, s = it - ct * STEPS;
            const int kb = 4 * s + q;
            const bool livek = kb < KB;
            const int tap = livek ? kb / CB : 0, half = livek ? kb % CB : 0;
            const float* wp = w + (((int64_t)grp * COUT_G + ct * 16 + p) * CIN_G + half * 16) * TAPS + tap;
            float wv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) wv[j] = livek ? wp[j * TAPS] : 0.0f;
            uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float qv = dw_quant(kind, wv[j]);
                const uint32_t byte = !livek ? 0u : (qv > 0.0f ? 0x01u : (qv < 0.0f ? 0xFFu : 0u));
                r[j >> 2] |= byte << (8 * (j & 3));
            }
            const gp_i4 frag = gp_i4{(int)r[0], (int)r[1], (int)r[2], (int)r[3]};
#pragma unroll
            for (int c = 0; c < NCT; ++c)
#pragma unroll
                for (int t = 0; t < STEPS; ++t)
                    if (it == c * STEPS + t) B[c][t] = frag;
        }
        // ---- the lane's K block of every step: tap offsets, the plane word and the shift of the 16-bit field
        int ti[STEPS], tj[STEPS], xw[STEPS], xsh[STEPS];
        bool lv[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            const int kb = 4 * s + q;
            lv[s] = kb < KB;
            const int tap = lv[s] ? kb / CB : 0, half = lv[s] ? kb % CB : 0;
            ti[s] = tap / KW;
            tj[s] = tap - ti[s] * KW;
            const int bit0 = grp * CIN_G + half * 16;
            xw[s] = bit0 >> 5;
            xsh[s] = bit0 & 31;
        }
        float b[NCT], al[NCT], be[NCT];
        int64_t co[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            co[ct] = (int64_t)grp * COUT_G + ct * 16 + p;
            b[ct] = bias ? bias[co[ct]] : 0.0f;
            al[ct] = alpha ? alpha[co[ct]] : 0.0f;
            be[ct] = beta ? beta[co[ct]] : 0.0f;
        }
        const int hw = g.Ho * g.Wo;
        const int64_t npix = (int64_t)g.N * hw;
        const int Hop = g.Ho + 2 * o.hy, Wop = g.Wo + 2 * o.hx;
        // the lane's pixel of the wave's first tile is divided out once
        int64_t next = (int64_t)split * GP_TILE + p;
        int rn = 0, rho = 0, rwo = 0;
        if (next < npix) {
            const int px = (int)next;
            rn = px / hw;
            const int r = px - rn * hw;
            rho = r / g.Wo;
            rwo = r - rho * g.Wo;
        }
        for (int u = split; u < wk.units; u += wk.splits) {
            const bool in = next < npix;
            const int n = in ? rn : 0, ho = in ? rho : 0, wo = in ? rwo : 0;
            next += (int64_t)wk.splits * GP_TILE;
            rwo += wk.d_wo;
            const int c1 = rwo >= g.Wo;
            rwo -= c1 ? g.Wo : 0;
            rho += wk.d_ho + c1;
            const int c2 = rho >= g.Ho;
            rho -= c2 ? g.Ho : 0;
            rn += wk.d_n + c2;
            // ---- A: one plane word per step, then the MFMAs
            const int h0 = ho * g.sh - g.ph, w0 = wo * g.sw - g.pw;
            const uint32_t* xn = xb + (int64_t)n * g.H * g.W * ldx;
            uint32_t word[STEPS], okm[STEPS];
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int hi = h0 + ti[s], wi = w0 + tj[s];
                okm[s] = (lv[s] && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W) ? 0xFFFFFFFFu : 0u;
                const int hc = hi < 0 ? 0 : (hi >= g.H ? g.H - 1 : hi), wc = wi < 0 ? 0 : (wi >= g.W ? g.W - 1 : wi);
                word[s] = xn[((int64_t)hc * g.W + wc) * ldx + xw[s]];
            }
            gp_i4 acc[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = gp_i4{0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const uint32_t f = word[s] >> xsh[s];
                const gp_i4 a = gp_i4{(int)(gp_expand4(f) & okm[s]), (int)(gp_expand4(f >> 4) & okm[s]),
                                      (int)(gp_expand4(f >> 8) & okm[s]), (int)(gp_expand4(f >> 12) & okm[s])};
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, B[ct][s], acc[ct], 0, 0, 0);
            }
            // ---- epilogue: the lane now is channel ct 16 + p of pixels 4 q + i of the tile
            // where pixel (n, ho, wo) lies in the output: its nibble row, or its element offset in y without the channel; -1: none
            int aux = -1;
            if (in) aux = o.y ? (int)(n * ys.n + ho * ys.h + wo * ys.w) : (int)(((int64_t)n * Hop + ho + o.hy) * Wop + wo + o.hx);
            const int64_t tile0 = (int64_t)u * GP_TILE;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t pix = tile0 + 4 * q + i;
                const int at = __shfl(aux, 4 * q + i);
                float y[NCT];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    y[ct] = (float)acc[ct][i];
                    if (bias) y[ct] = y[ct] + b[ct];
                }
                if (o.y) {                               // uniform over the launch
                    if (at >= 0) {
#pragma unroll
                        for (int ct = 0; ct < NCT; ++ct) o.y[(int64_t)at + co[ct] * ys.c] = y[ct];
                    }
                    continue;
                }
                unsigned long long mine = 0ull;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const unsigned long long votes = __ballot((int)qt_neg_bit(y[ct] * al[ct] + be[ct]));
                    if (p == ct) mine = votes;
                }
                if (at < 0) continue;                    // a pixel past the end: after the ballots, which every lane takes part in
                uint32_t* srow = o.sign ? o.sign + pix * o.ldb : nullptr;
                uint32_t* nrow = o.nib ? o.nib + (int64_t)at * o.ldn : nullptr;
                if (p < NCT) {
                    const uint32_t field = (uint32_t)(mine >> (16 * q)) & 0xFFFFu;
                    const int piece = grp * NCT + p;     // the 16-channel piece of the pixel row
                    if (srow) reinterpret_cast<uint16_t*>(srow)[piece] = (uint16_t)field;
                    if (nrow)
                        *reinterpret_cast<uint2*>(nrow + 2 * piece) =
                            make_uint2(0x22222222u | (dw_spread8(field) << 3), 0x22222222u | (dw_spread8(field >> 8) << 3));
                } else if (p == NCT && grp == wk.G - 1) {  // behind the last channel: the rest of its word, the pad words
                    const int pieces = wk.G * NCT;
                    if (srow) {
                        if (pieces & 1) reinterpret_cast<uint16_t*>(srow)[pieces] = 0;
                        for (int64_t t = (pieces + 1) >> 1; t < o.ldb; ++t) srow[t] = 0u;
                    }
                    if (nrow)
                        for (int64_t t = 2 * (int64_t)pieces; t < o.ldn; t += 2) *reinterpret_cast<uint2*>(nrow + t) = make_uint2(0u, 0u);
                }
            }
        }
    }
    if (!o.y) dw_zero_border(o, g, tid);
}

template <int TAPS, int CB>
void gp_go(int nct, unsigned grid, hipStream_t s, const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias,
           const float* alpha, const float* beta, const DwPlaneOut& o, const DwGeom& g, const DwStrides& ys, const GpWalk& wk, int kind) {
    if (nct == 1) gp_kernel<TAPS, CB, 1><<<grid, DW_THREADS, 0, s>>>(x_plane, ldx, w, bias, alpha, beta, o, g, ys, wk, kind);
    else if (nct == 2) gp_kernel<TAPS, CB, 2><<<grid, DW_THREADS, 0, s>>>(x_plane, ldx, w, bias, alpha, beta, o, g, ys, wk, kind);
    else gp_kernel<TAPS, CB, 3><<<grid, DW_THREADS, 0, s>>>(x_plane, ldx, w, bias, alpha, beta, o, g, ys, wk, kind);
}

// Steps 1 to 3 of the documented validation order, shared by the two entries and gp_describe.  False: the call ends with `rc`
// (QT_OK: an empty problem); true: Ho x Wo is the output map of a problem inside the window.
bool gp_shape(bool f32, int64_t halo_h, int64_t halo_w, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh,
              int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t& Ho, int64_t& Wo, int& rc) {
    rc = QT_ERR_INVALID_ARG;
    if (halo_h < 0 || halo_w < 0) return false;
    if (N < 0 || G < 0 || cin_g < 1 || cout_g < 1 || H < 0 || W < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 ||
        dh < 1 || dw < 1)
        return false;
    rc = QT_ERR_UNSUPPORTED;
    if ((int64_t)kh * kw > QT_DW_MAX_TAPS) return false;
    if (N == 0 || G == 0 || H == 0 || W == 0) {
        rc = QT_OK;
        return false;
    }
    if ((cin_g != 16 && cin_g != 32) || (cout_g != 16 && cout_g != 32 && cout_g != 48)) return false;
    if (!((kh == 1 && kw == 1) || (kh == 3 && kw == 3)) || sh != sw || sh > 2 || dh != 1 || dw != 1 || ph > 1 || pw > 1) return false;
    if (N >= GP_MAX_ROWS || G >= GP_MAX_ROWS || H >= GP_MAX_ROWS || W >= GP_MAX_ROWS || halo_h > DW_MAX_HALO || halo_w > DW_MAX_HALO)
        return false;
    const int64_t eh = H + 2 * (int64_t)ph - kh, ew = W + 2 * (int64_t)pw - kw;
    if (eh < 0 || ew < 0) {                                       // the kernel does not fit the padded image
        rc = QT_ERR_INVALID_ARG;
        return false;
    }
    Ho = eh / sh + 1;
    Wo = ew / sw + 1;
    // pixel rows of every plane below 2^31; so are the elements of y, whose offsets the kernel keeps in 32 bits
    return !((double)N * (double)H * (double)W >= (double)GP_MAX_ROWS ||
             (double)N * (double)(Ho + 2 * halo_h) * (double)(Wo + 2 * halo_w) >= (double)GP_MAX_ROWS ||
             (f32 && (double)N * (double)(G * cout_g) * (double)Ho * (double)Wo >= (double)GP_MAX_ROWS) ||
             G * cout_g > QT_DW_MAX_CHANNELS);
}

// the walk of a launch over N Ho Wo output pixels: tiles of 16, splits per group, what a step adds to a lane's (n, ho, wo)
GpWalk gp_walk(int64_t N, int64_t G, int64_t Ho, int64_t Wo) {
    const int64_t npix = N * Ho * Wo;
    GpWalk wk{};
    wk.G = (int)G;
    wk.units = (int)((npix + GP_TILE - 1) / GP_TILE);
    int64_t sp = (int64_t)GP_TARGET_WGS * GP_WAVES / G;
    if (sp > wk.units) sp = wk.units;
    wk.splits = (int)(sp < 1 ? 1 : sp);
    const int64_t step = (int64_t)wk.splits * GP_TILE;
    wk.d_wo = (int)(step % Wo);
    wk.d_ho = (int)((step / Wo) % Ho);
    wk.d_n = (int)(step / Wo / Ho);
    return wk;
}

// workgroups of that launch: one wave per (split, group)
unsigned gp_grid(const GpWalk& wk) { return (unsigned)(((int64_t)wk.G * wk.splits + GP_WAVES - 1) / GP_WAVES); }

// the shared body of the two entries, in the documented validation order: o.y, or at least one of o.sign / o.nib
int gp_launch(const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, const float* alpha, const float* beta,
              DwPlaneOut o, bool f32, int64_t halo_h, int64_t halo_w, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
              int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, DwStrides ys, int kind, qt_stream_t stream) {
    int64_t Ho, Wo;
    int rc;
    if (!gp_shape(f32, halo_h, halo_w, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;
    const int64_t Cin = G * cin_g, Cout = G * cout_g;
    if (kind != QT_DW_RAW && kind != QT_DW_SIGN && kind != QT_DW_TERNARY) return QT_ERR_INVALID_ARG;
    if (!x_plane || !w) return QT_ERR_INVALID_ARG;
    if (f32) {
        if (!o.y || dw_layout(N, Cout, Ho, Wo, ys) < 0) return QT_ERR_INVALID_ARG;
    } else {
        if ((!o.sign && !o.nib) || !alpha || !beta) return QT_ERR_INVALID_ARG;
        if (o.sign && o.ldb < dw_packed_ld(Cout)) return QT_ERR_INVALID_ARG;
        if (o.nib && o.ldn < dw_pixel_ld_nib(Cout)) return QT_ERR_INVALID_ARG;
    }
    if (ldx < dw_packed_ld(Cin)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(x_plane) || !dw_aligned4(w) || !dw_aligned4(bias) || !dw_aligned4(alpha) || !dw_aligned4(beta) || !dw_aligned4(o.y) ||
        !dw_aligned4(o.sign))
        return QT_ERR_ALIGNMENT;
    if (o.nib && ((o.ldn & 3) || !dw_aligned16(o.nib))) return QT_ERR_ALIGNMENT;
    o.hy = (int)halo_h;
    o.hx = (int)halo_w;
    DwGeom g{};                                     // the record the writing stage reads; m is not used
    g.N = (int)N; g.C = (int)Cin; g.H = (int)H; g.W = (int)W; g.Ho = (int)Ho; g.Wo = (int)Wo;
    g.kh = kh; g.kw = kw; g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw; g.dh = dh; g.dw = dw;
    g.Cout = Cout;
    const GpWalk wk = gp_walk(N, G, Ho, Wo);
    const unsigned grid = gp_grid(wk);
    hipStream_t s = (hipStream_t)stream;
    const int nct = (int)(cout_g / 16);
#define GP_ARGS nct, grid, s, x_plane, ldx, w, bias, alpha, beta, o, g, ys, wk, kind
    if (kh == 1) {
        if (cin_g == 16) gp_go<1, 1>(GP_ARGS);
        else gp_go<1, 2>(GP_ARGS);
    } else {
        if (cin_g == 16) gp_go<9, 1>(GP_ARGS);
        else gp_go<9, 2>(GP_ARGS);
    }
#undef GP_ARGS
    return qt_check_launch();
}

}  // namespace

// QT_GM_OP_PLANES of qt_gmconv2d_describe: gp_launch up to the walk, for qt_gmconv2d_sign without an output halo (the walk depends
// on neither the output form nor the halo)
int gp_describe(int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                int pw, int dh, int dw, char* out, int cap) {
    int64_t Ho, Wo;
    int rc;
    if (!gp_shape(false, 0, 0, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo, rc)) return rc;
    const GpWalk wk = gp_walk(N, G, Ho, Wo);
    snprintf(out, (size_t)cap, "kernel=gp_kernel<%d,%d,%d> units=%d splits=%d d_n=%d d_ho=%d d_wo=%d grid=%u block=%d", kh * kw,
             (int)cin_g / 16, (int)cout_g / 16, wk.units, wk.splits, wk.d_n, wk.d_ho, wk.d_wo, gp_grid(wk), DW_THREADS);
    return QT_OK;
}

extern "C" int qt_gmconv2d_sign(const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, const float* alpha,
                                const float* beta, uint32_t* sign_plane, int64_t ldb, uint32_t* nib_plane, int64_t ldn,
                                int64_t out_halo_h, int64_t out_halo_w, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H,
                                int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int kind,
                                qt_stream_t stream) {
    DwPlaneOut o{};
    o.sign = sign_plane;
    o.ldb = ldb;
    o.nib = nib_plane;
    o.ldn = ldn;
    return gp_launch(x_plane, ldx, w, bias, alpha, beta, o, false, out_halo_h, out_halo_w, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph,
                     pw, dh, dw, DwStrides{0, 0, 0, 0}, kind, stream);
}

extern "C" int qt_gmconv2d_bits_f32(const uint32_t* x_plane, int64_t ldx, const float* w, const float* bias, float* y, int64_t N,
                                    int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw,
                                    int ph, int pw, int dh, int dw, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w, int kind,
                                    qt_stream_t stream) {
    DwPlaneOut o{};
    o.y = y;
    return gp_launch(x_plane, ldx, w, bias, nullptr, nullptr, o, true, 0, 0, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph, pw, dh, dw,
                     DwStrides{ys_n, ys_c, ys_h, ys_w}, kind, stream);
}
