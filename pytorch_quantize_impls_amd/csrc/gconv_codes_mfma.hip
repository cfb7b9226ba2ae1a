// Grouped conv2d with 16 or 32 input channels per group on the int8 code planes of a DoReFa activation, on the int8 matrix cores:
// the grouped DorefaConv2d of the last ResNeXt stages inside the fused code chain.  include/qt_hip.h "Grouped convolution on int8
// code planes, on the matrix cores" states the contract; DESIGN.md "Grouped convs on code planes, on the matrix cores" the layout
// and the resources.
//
// A code plane is NHWC with a row pitch that is a multiple of 16 bytes, so a group's 16 channels at one tap are ONE aligned 16-byte
// piece: exactly one K block of v_mfma_i32_16x16x64_i8.  Nothing is expanded; the weight bytes are the sign (1-bit weights) or the
// integer level (2 .. 7 bits) of the fp32 eval image; every sum is an integer below 2^24.
//
// Operand roles.  The WEIGHTS are the MFMA's row operand, the PIXELS its column operand: lane l holds output pixel l & 15 of its
// wave's 16 and, as its accumulator quad, the 4 consecutive output channels 4 (l >> 4) .. + 3 of a 16-channel tile.  After the
// epilogue that quad is one dword of four int8 codes; the four lanes of a pixel write 16 contiguous bytes of its NHWC row.  No
// cross-lane byte shuffle, nothing read back.
//   weights : cout_g / 16 x steps x 4 registers (at most 60), resident for the whole launch: lane (row p, block q) classifies the 16
//             weights of output channel ct 16 + p at K block 4 s + q once, from the fp32 image.  A K block is 16 channels: a tap of
//             16 channels is one block, of 32 channels two; a step is four blocks (3 steps for 3 x 3 at cin_g = 16, 5 at cin_g = 32,
//             1 for 1 x 1); blocks past the taps are zero in both operands.
//   pixels  : a workgroup of 4 waves owns ONE group and walks 64-pixel tiles (TW x TH output pixels of one image) of its output map.
//             Per tile the source bounding box, clipped to the image, is staged once into LDS as 16-byte pieces, the pixel pitch
//             padded to an odd number of 16-byte slots; a table [tap][pixel] holds the LDS offset of every (tap, output pixel), a
//             tap outside the image and a pixel beyond the tile pointing to one zero pixel.  A wave's fragment is then one 16-byte
//             LDS read per step through the table: the main loop has no branch and no coordinate arithmetic.  The halo of the input
//             plane is never read.
//   epilogue: y = fl(fl((float)S * s) + bias) with s = fl(scale * *w_scale) — the dense code conv's value — then the shared code
//             epilogue (codes_epilogue.h) or the fp32 store.  The workgroups of the LAST group also write the pad bytes behind
//             G cout_g channels; all workgroups share the zero border of a halo plane.
#include "qt_common.h"
#include "dw_planes.h"
#include "codes_epilogue.h"

namespace {

typedef int gq_i4 __attribute__((ext_vector_type(4)));

constexpr int GQ_TILE = 64;                       // output pixels of a tile: 16 per wave
constexpr int GQ_TARGET_WGS = 1024;               // workgroups of a launch: 4 per CU, so that a wave's weight pass is amortised
constexpr int GQ_MAX_BOX = 33 * 9;                // source pixels of a tile: 16 x 4 outputs, 3 x 3, stride 2 (8 x 8: 17 x 17)
constexpr int GQ_MIN_GROUPS = 8;
constexpr int64_t GQ_MAX_ROWS = (int64_t)1 << 31;

struct GqPlan {
    int G, splits;
    int64_t tiles;                                // N * th_n * tw_n, per group
    int TW, TH, tw_log;                           // the tile: TW x TH = 64 output pixels, TW a power of two
    int th_n, tw_n;                               // tiles of one image, down and across
    int BH, BW;                                   // its source box, un-clipped
};

struct GqGeom {
    int N, H, W, Ho, Wo, s, ph, pw, ihy, ihx, ohy, ohx;
    int64_t ldx, Cout;
};

struct GqOut {
    // code form
    int8_t* codes;
    int64_t ldc;
    int32_t* overflow;
    const float *alpha, *beta, *bn_stats;
    int relu;
    float n;
    // fp32 form
    float* y;
    DwStrides ys;
    const int32_t* in_flag;
    int vec;
};

template <int TAPS, int CB, int NCT, bool F32OUT>
__global__ __launch_bounds__(DW_THREADS) void gq_kernel(const int8_t* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float scale,
                                                        const float* __restrict__ w_scale, int w_bits, GqOut o, GqGeom g, GqPlan pl) {
    constexpr int KB = TAPS * CB;                 // live K blocks of 16 channels
    constexpr int STEPS = (KB + 3) / 4;
    constexpr int CIN_G = 16 * CB, COUT_G = 16 * NCT;
    constexpr int KW = TAPS == 9 ? 3 : 1;
    constexpr int PITCH = CB | 1;                 // 16-byte slots of a staged pixel: odd
    constexpr int ZERO_OFF = GQ_MAX_BOX * PITCH * 16;
    __shared__ uint4 box[(GQ_MAX_BOX + 1) * PITCH];
    __shared__ int tab[(TAPS + 1) * GQ_TILE];
    const int tid = threadIdx.x, lane = tid & 63, p = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // neighbouring workgroups are neighbouring groups on the same tiles: they read neighbouring pieces of the same plane rows
    const int split = (int)blockIdx.x / pl.G, grp = (int)blockIdx.x - split * pl.G;

    // ---- the group's weight bytes, resident.  A real loop over (ct, s) with the registers picked by compile-time selects: the
    // classification exists once, not NCT x STEPS times
    gq_i4 Wf[NCT][STEPS];
    const float wn = (float)((1 << w_bits) - 1);
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
            int b;
            if (w_bits == 1) {
                b = wv[j] < 0.0f ? -1 : 1;                                  // +-E: the byte is the sign
            } else {
                const float l = rintf(__fmul_rn(wn, wv[j]));               // the integer level of an on-grid image
                b = (l >= -127.0f && l <= 127.0f) ? (int)l : 0;
            }
            r[j >> 2] |= (livek ? (uint32_t)(uint8_t)(int8_t)b : 0u) << (8 * (j & 3));
        }
        const gq_i4 frag = gq_i4{(int)r[0], (int)r[1], (int)r[2], (int)r[3]};
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int t = 0; t < STEPS; ++t)
                if (it == c * STEPS + t) Wf[c][t] = frag;
    }
    // ---- the lane's table row and 16-byte piece of every step; dead blocks read the table's last row: the zero pixel
    int trow[STEPS], hoff[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int kb = 4 * s + q;
        const int tap = kb / CB < TAPS ? kb / CB : TAPS;
        trow[s] = tap * GQ_TILE + wave * 16 + p;
        hoff[s] = (kb % CB) * 16;
    }
    float sc = scale;
    if (w_scale) sc = __fmul_rn(sc, *w_scale);    // device-resident factor (E of 1-bit weights): no host synchronisation
    // per-channel constants of the lane's quad of every column tile
    float b[NCT][4];
    AffineConsts ac[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int64_t co0 = (int64_t)grp * COUT_G + ct * 16 + 4 * q;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[ct][e] = bias ? bias[co0 + e] : 0.0f;
        if (!F32OUT) affine_load_consts(ac[ct], co0, g.Cout, o.alpha, o.beta, nullptr, nullptr, o.bn_stats, nullptr);
    }
    const bool devbn = o.bn_stats != nullptr;
    const bool nan_all = F32OUT && o.in_flag && *o.in_flag != 0;
    if (tid < PITCH) box[GQ_MAX_BOX * PITCH + tid] = make_uint4(0u, 0u, 0u, 0u);
    if (tid < GQ_TILE) tab[TAPS * GQ_TILE + tid] = ZERO_OFF;

    const int Hp = g.H + 2 * g.ihy, Wp = g.W + 2 * g.ihx;
    const int Hop = g.Ho + 2 * g.ohy, Wop = g.Wo + 2 * g.ohx;
    const int per_img = pl.th_n * pl.tw_n;
    const int tp = wave * 16 + p, ty = tp >> pl.tw_log, tx = tp & (pl.TW - 1);
    int bad = 0;
    for (int64_t t = split; t < pl.tiles; t += pl.splits) {
        const int n = (int)(t / per_img), rt = (int)(t - (int64_t)n * per_img);
        const int tyb = rt / pl.tw_n, txb = rt - tyb * pl.tw_n;
        const int ho0 = tyb * pl.TH, wo0 = txb * pl.TW;
        const int h_lo = ho0 * g.s - g.ph, w_lo = wo0 * g.s - g.pw;
        __syncthreads();                          // the previous tile's fragment reads are done
        // ---- stage the source box: only pixels inside the image are read and written; nothing else is reached by the table
        const int8_t* xg = x + (int64_t)grp * CIN_G;
        for (int idx = tid; idx < pl.BH * pl.BW * CB; idx += DW_THREADS) {
            const int piece = idx % CB, pix = idx / CB;
            const int bh = pix / pl.BW, bw = pix - bh * pl.BW;
            const int hi = h_lo + bh, wi = w_lo + bw;
            if (hi >= 0 && hi < g.H && wi >= 0 && wi < g.W)
                box[pix * PITCH + piece] =
                    *reinterpret_cast<const uint4*>(xg + (((int64_t)n * Hp + hi + g.ihy) * Wp + wi + g.ihx) * g.ldx + piece * 16);
        }
        for (int idx = tid; idx < TAPS * GQ_TILE; idx += DW_THREADS) {
            const int tap = idx >> 6, e = idx & 63;
            const int ey = e >> pl.tw_log, ex = e & (pl.TW - 1);
            const int ti = tap / KW, tj = tap - ti * KW;
            const int bh = ey * g.s + ti, bw = ex * g.s + tj;
            const int hi = h_lo + bh, wi = w_lo + bw;
            const bool ok = ho0 + ey < g.Ho && wo0 + ex < g.Wo && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
            tab[idx] = ok ? (bh * pl.BW + bw) * PITCH * 16 : ZERO_OFF;
        }
        __syncthreads();
        // ---- the MFMAs: one 16-byte LDS read per step feeds every column tile
        gq_i4 a[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
            a[s] = *reinterpret_cast<const gq_i4*>(reinterpret_cast<const char*>(box) + tab[trow[s]] + hoff[s]);
        gq_i4 acc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[ct] = gq_i4{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Wf[ct][s], a[s], acc[ct], 0, 0, 0);
        // ---- epilogue: the lane is pixel (ty, tx) of the tile, channels ct 16 + 4 q .. + 3
        const int ho = ho0 + ty, wo = wo0 + tx;
        if (ho >= g.Ho || wo >= g.Wo) continue;
        int8_t* crow = F32OUT ? nullptr : o.codes + (((int64_t)n * Hop + ho + g.ohy) * Wop + wo + g.ohx) * o.ldc;
        float* yrow = F32OUT ? o.y + (int64_t)n * o.ys.n + (int64_t)ho * o.ys.h + (int64_t)wo * o.ys.w : nullptr;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int64_t co0 = (int64_t)grp * COUT_G + ct * 16 + 4 * q;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(__fmul_rn((float)acc[ct][e], sc), b[ct][e]);
            if (F32OUT) {
                if (nan_all) v[0] = v[1] = v[2] = v[3] = __builtin_nanf("");
                if (o.vec) {
                    *reinterpret_cast<float4*>(yrow + co0) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) yrow[(co0 + e) * o.ys.c] = v[e];
                }
            } else {
                const float r0[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                float q4[4];
                const uint32_t word = affine_codes_word(v, r0, 0u, ac[ct], 4, devbn, false, false, false, false, 0.0f, o.relu, o.n, q4, bad);
                *reinterpret_cast<uint32_t*>(crow + co0) = word;
            }
        }
        if (!F32OUT && grp == pl.G - 1 && q == 0)   // the pad bytes behind the last channel
            for (int64_t c = g.Cout; c < o.ldc; c += 4) *reinterpret_cast<uint32_t*>(crow + c) = 0u;
    }
    if (F32OUT) return;
    if (g.ohy | g.ohx) {
        // the border pixels of the output plane, whole rows of ldc bytes, shared by all workgroups: per image ohy rows on top,
        // 2 ohx columns beside each of the Ho image rows, ohy rows below
        const int64_t ldw = o.ldc >> 2;
        const int64_t top = (int64_t)g.ohy * Wop, side = 2 * (int64_t)g.ohx * g.Ho, per = 2 * top + side;
        const int64_t total = (int64_t)g.N * per * ldw;
        for (int64_t i = (int64_t)blockIdx.x * DW_THREADS + tid; i < total; i += (int64_t)gridDim.x * DW_THREADS) {
            const int64_t bp = i / ldw, d = i - bp * ldw;
            const int64_t img = bp / per, r = bp - img * per;
            int64_t h, c;
            if (r < top) { h = r / Wop; c = r - h * Wop; }
            else if (r < top + side) {
                const int64_t k2 = r - top, row = k2 / (2 * g.ohx), k = k2 - row * 2 * g.ohx;
                h = g.ohy + row;
                c = k < g.ohx ? k : g.Wo + k;
            } else { const int64_t k2 = r - top - side; h = g.ohy + g.Ho + k2 / Wop; c = k2 % Wop; }
            reinterpret_cast<uint32_t*>(o.codes + ((img * Hop + h) * Wop + c) * o.ldc)[d] = 0u;
        }
    }
    if (__any(bad) && lane == 0) atomicOr(o.overflow, __any(bad & 2) ? 3 : 1);
}

template <int TAPS, int CB, bool F32OUT>
void gq_go(int nct, unsigned grid, hipStream_t s, const int8_t* x, const float* w, const float* bias, float scale, const float* w_scale,
           int w_bits, const GqOut& o, const GqGeom& g, const GqPlan& pl) {
    if (nct == 1) gq_kernel<TAPS, CB, 1, F32OUT><<<grid, DW_THREADS, 0, s>>>(x, w, bias, scale, w_scale, w_bits, o, g, pl);
    else if (nct == 2) gq_kernel<TAPS, CB, 2, F32OUT><<<grid, DW_THREADS, 0, s>>>(x, w, bias, scale, w_scale, w_bits, o, g, pl);
    else gq_kernel<TAPS, CB, 3, F32OUT><<<grid, DW_THREADS, 0, s>>>(x, w, bias, scale, w_scale, w_bits, o, g, pl);
}

// the tile of a launch — of 16 x 4, 8 x 8 and 4 x 16 output pixels the one that covers the map with the fewest idle pixels, 8 x 8
// on a tie (the smallest source box) — and the walk over the tiles
GqPlan gq_plan(int64_t N, int64_t G, int64_t Ho, int64_t Wo, int k, int s) {
    static const int tws[3] = {8, 16, 4};
    GqPlan pl{};
    int64_t best = -1;
    for (int i = 0; i < 3; ++i) {
        const int tw = tws[i], th = GQ_TILE / tw;
        const int64_t cover = ((Ho + th - 1) / th) * ((Wo + tw - 1) / tw);
        if (best < 0 || cover < best) {
            best = cover;
            pl.TW = tw;
            pl.TH = th;
        }
    }
    pl.tw_log = pl.TW == 4 ? 2 : (pl.TW == 8 ? 3 : 4);
    pl.th_n = (int)((Ho + pl.TH - 1) / pl.TH);
    pl.tw_n = (int)((Wo + pl.TW - 1) / pl.TW);
    pl.tiles = N * pl.th_n * pl.tw_n;
    pl.BH = (pl.TH - 1) * s + k;
    pl.BW = (pl.TW - 1) * s + k;
    pl.G = (int)G;
    int64_t sp = GQ_TARGET_WGS / G;
    if (sp > pl.tiles) sp = pl.tiles;
    pl.splits = (int)(sp < 1 ? 1 : sp);
    return pl;
}

inline int64_t gq_code_ld(int64_t K) { return (K + 15) / 16 * 16; }

// the shared body of the two entries, in the documented validation order: o.codes (code plane out) or o.y (fp32 out)
int gq_launch(const int8_t* x_plane, int64_t ldx, int64_t ihy, int64_t ihx, float inv_n, const float* w, const float* bias, GqOut o,
              int bit_width, int64_t ohy, int64_t ohx, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh,
              int kw, int sh, int sw, int ph, int pw, int dh, int dw, bool f32, const float* w_scale, int w_bits, qt_stream_t stream) {
    // 1. signs
    if (ihy < 0 || ihx < 0 || ohy < 0 || ohx < 0) return QT_ERR_INVALID_ARG;
    if (N < 0 || G < 0 || cin_g < 1 || cout_g < 1 || H < 0 || W < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 ||
        dh < 1 || dw < 1)
        return QT_ERR_INVALID_ARG;
    // 2. an empty problem
    if (N == 0 || G == 0 || H == 0 || W == 0) return QT_OK;
    // 3. the window
    if (G < GQ_MIN_GROUPS || (cin_g != 16 && cin_g != 32) || (cout_g != 16 && cout_g != 32 && cout_g != 48)) return QT_ERR_UNSUPPORTED;
    if (!((kh == 1 && kw == 1) || (kh == 3 && kw == 3)) || sh != sw || sh > 2 || dh != 1 || dw != 1 || ph > 1 || pw > 1)
        return QT_ERR_UNSUPPORTED;
    if (N >= GQ_MAX_ROWS || G >= GQ_MAX_ROWS || H >= GQ_MAX_ROWS || W >= GQ_MAX_ROWS) return QT_ERR_UNSUPPORTED;
    const int64_t eh = H + 2 * (int64_t)ph - kh, ew = W + 2 * (int64_t)pw - kw;
    if (eh < 0 || ew < 0) return QT_ERR_INVALID_ARG;              // the kernel does not fit the padded image
    const int64_t Ho = eh / sh + 1, Wo = ew / sw + 1, Cin = G * cin_g, Cout = G * cout_g;
    if (ihy > DW_MAX_HALO || ihx > DW_MAX_HALO || ohy > DW_MAX_HALO || ohx > DW_MAX_HALO) return QT_ERR_UNSUPPORTED;
    if ((double)N * (double)(H + 2 * ihy) * (double)(W + 2 * ihx) >= (double)GQ_MAX_ROWS ||
        (double)N * (double)(Ho + 2 * ohy) * (double)(Wo + 2 * ohx) >= (double)GQ_MAX_ROWS || Cout > QT_DW_MAX_CHANNELS ||
        (f32 && (double)N * (double)Cout * (double)Ho * (double)Wo >= (double)GQ_MAX_ROWS))
        return QT_ERR_UNSUPPORTED;
    if (!f32 && o.ldc >= GQ_MAX_ROWS) return QT_ERR_UNSUPPORTED;
    // 4. arguments, then alignment
    if (!x_plane || !w) return QT_ERR_INVALID_ARG;
    if (w_bits < 1 || w_bits > 7 || (w_bits == 1 && !w_scale)) return QT_ERR_INVALID_ARG;
    if (f32) {
        if (!o.y || dw_layout(N, Cout, Ho, Wo, o.ys) < 0) return QT_ERR_INVALID_ARG;
    } else {
        if (bit_width < 2 || bit_width > 8 || o.relu < 0 || o.relu > 1) return QT_ERR_INVALID_ARG;
        if (!o.alpha || !o.beta || !o.codes || !o.overflow) return QT_ERR_INVALID_ARG;
        if (o.ldc < gq_code_ld(Cout)) return QT_ERR_INVALID_ARG;
    }
    if (ldx < gq_code_ld(Cin)) return QT_ERR_INVALID_ARG;
    if (!dw_aligned4(w) || !dw_aligned4(bias) || !dw_aligned4(o.alpha) || !dw_aligned4(o.beta) || !dw_aligned4(o.bn_stats) ||
        !dw_aligned4(o.overflow) || !dw_aligned4(o.in_flag) || !dw_aligned4(o.y) || !dw_aligned4(w_scale))
        return QT_ERR_ALIGNMENT;
    if ((ldx & 15) || !dw_aligned16(x_plane) || (o.ldc & 15) || !dw_aligned16(o.codes)) return QT_ERR_ALIGNMENT;
    const GqPlan pl = gq_plan(N, G, Ho, Wo, kh, sh);
    if (pl.BH * pl.BW > GQ_MAX_BOX) return QT_ERR_UNSUPPORTED;    // (no tile of the window reaches it)
    GqGeom g{};
    g.N = (int)N; g.H = (int)H; g.W = (int)W; g.Ho = (int)Ho; g.Wo = (int)Wo; g.s = sh; g.ph = ph; g.pw = pw;
    g.ihy = (int)ihy; g.ihx = (int)ihx; g.ohy = (int)ohy; g.ohx = (int)ohx;
    g.ldx = ldx;
    g.Cout = Cout;
    o.n = (float)((1 << (f32 ? 2 : bit_width)) - 1);
    o.vec = f32 && o.ys.c == 1 && dw_aligned16(o.y);
    // the scale of the dense code conv: inv_n of the plane, times fl(1 / (2^k - 1)) for k-bit levels — one rounding — or, in the
    // kernel, times the device scalar E of 1-bit weights
    float scale = inv_n;
    if (w_bits > 1) scale = (float)((double)inv_n * (double)(1.0f / (float)((1 << w_bits) - 1)));
    const unsigned grid = (unsigned)((int64_t)pl.G * pl.splits);
    hipStream_t s = (hipStream_t)stream;
    const int nct = (int)(cout_g / 16);
    const float* ws = w_bits == 1 ? w_scale : nullptr;
#define GQ_ARGS nct, grid, s, x_plane, w, bias, scale, ws, w_bits, o, g, pl
#define GQ_FORM(TAPS, CB)                                                                                              \
    do {                                                                                                               \
        if (f32) gq_go<TAPS, CB, true>(GQ_ARGS);                                                                       \
        else gq_go<TAPS, CB, false>(GQ_ARGS);                                                                          \
    } while (0)
    if (kh == 1) {
        if (cin_g == 16) GQ_FORM(1, 1);
        else GQ_FORM(1, 2);
    } else {
        if (cin_g == 16) GQ_FORM(9, 1);
        else GQ_FORM(9, 2);
    }
#undef GQ_FORM
#undef GQ_ARGS
    return qt_check_launch();
}

}  // namespace

extern "C" int qt_gmconv2d_codes(const int8_t* x_plane, int64_t ldx_bytes, int64_t in_halo_h, int64_t in_halo_w, float inv_n,
                                 const float* w, const float* bias, const float* alpha, const float* beta, const float* bn_stats,
                                 int relu, int bit_width, int8_t* codes, int64_t ldc_bytes, int64_t out_halo_h, int64_t out_halo_w,
                                 int32_t* overflow, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh,
                                 int kw, int sh, int sw, int ph, int pw, int dh, int dw, const float* w_scale, int w_bits,
                                 qt_stream_t stream) {
    GqOut o{};
    o.alpha = alpha;
    o.beta = beta;
    o.bn_stats = bn_stats;
    o.relu = relu;
    o.codes = codes;
    o.ldc = ldc_bytes;
    o.overflow = overflow;
    return gq_launch(x_plane, ldx_bytes, in_halo_h, in_halo_w, inv_n, w, bias, o, bit_width, out_halo_h, out_halo_w, N, G, cin_g, cout_g,
                     H, W, kh, kw, sh, sw, ph, pw, dh, dw, false, w_scale, w_bits, stream);
}

extern "C" int qt_gmconv2d_codes_f32(const int8_t* x_plane, int64_t ldx_bytes, int64_t in_halo_h, int64_t in_halo_w, float inv_n,
                                     const float* w, const float* bias, const int32_t* overflow, float* y, int64_t N, int64_t G,
                                     int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                                     int pw, int dh, int dw, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w,
                                     const float* w_scale, int w_bits, qt_stream_t stream) {
    GqOut o{};
    o.y = y;
    o.ys = DwStrides{ys_n, ys_c, ys_h, ys_w};
    o.in_flag = overflow;
    return gq_launch(x_plane, ldx_bytes, in_halo_h, in_halo_w, inv_n, w, bias, o, 0, 0, 0, N, G, cin_g, cout_g, H, W, kh, kw, sh, sw, ph,
                     pw, dh, dw, true, w_scale, w_bits, stream);
}
