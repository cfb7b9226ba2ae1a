// What the matrix-core grouped convs of gconv_mfma.hip (fp32 operands, three bf16 terms) and gconv_mfma_h.hip (bf16 / fp16 operands,
// one term) share: the gather's record of a problem, the tile plan with its LDS budget, the spans of a tile's source box and steps
// 1 to 3 of the documented validation order.  The plans (gm_plan; gmw_plan of the weight gradient) take the number of operand
// planes (`terms`) the patch is staged as.
#pragma once
#include "qt_common.h"

namespace {

constexpr int GM_TILE_PIX = 128;                 // destination pixels of a tile: 8 row tiles of 16
constexpr int GM_TILE_COLS = 32;
constexpr int GM_LDS_BYTES = 64 * 1024;          // weights + tables + patch: two workgroups per CU at the worst
constexpr int GM_TARGET_WGS = 1024;
constexpr int GM_MAX_COUT_G = QT_GM_MAX_COUT_G;
constexpr int64_t GM_MAX_ELEMS = (int64_t)1 << 31;

struct GmGeom {
    int N, G;
    int KC, NO;              // reduction / result channels per group
    int Hs, Ws, Hd, Wd;      // source and destination maps
    int s, ph, pw;
    int bwd;                 // 0: forward (src = x), 1: grad_input (src = go)
    int vec;                 // channels-last source, 16-byte aligned: 16-byte loads
};

struct GmPlan {
    int TR, TC, tiles_r, tiles_c;
    int splits;
    int npmax;               // patch pixels per term; pixel npmax is the zero pixel
    int nopad;               // NO padded to the column tile
    int w_bytes, lds_bytes;
};

// bytes of a patch pixel: NCB blocks of 8 two-byte elements, padded to an odd number of 16-byte slots
constexpr int gm_ps(int ncb) { return 16 * (ncb | 1); }

__host__ __device__ inline int gm_min(int a, int b) { return a < b ? a : b; }

// the source rows (columns) a run [d0, d1) of destination rows reads along one axis, clipped to the source: first and count
__device__ __forceinline__ void gm_span(int bwd, int d0, int d1, int s, int p, int k, int S, int& lo, int& cnt) {
    int hi;
    if (!bwd) {
        lo = d0 * s - p;
        hi = (d1 - 1) * s - p + k - 1;
    } else {
        const int a = d0 + p - (k - 1);
        lo = a <= 0 ? 0 : (a + s - 1) / s;
        hi = (d1 - 1 + p) / s;
    }
    lo = lo < 0 ? 0 : lo;
    hi = hi > S - 1 ? S - 1 : hi;
    cnt = hi >= lo ? hi - lo + 1 : 0;
}

// the most gm_span can return for a run of T destination rows
inline int gm_span_cap(int bwd, int T, int s, int k, int S) {
    const int cap = bwd ? (T + k - 2) / s + 1 : (T - 1) * s + k;
    return cap < S ? cap : S;
}

// the tile of the destination map and the LDS it needs: at most 128 pixels, at most 32 columns, the patch (`terms` planes of it)
// inside the budget, then balanced over the map (which only shrinks it).  shrunk (qt_gmconv2d_describe): how often the budget loop
// took a row, a column.
inline GmPlan gm_plan(const GmGeom& g, int taps, int ncb, int terms, int* shrunk = nullptr) {
    GmPlan pl{};
    const int ks = taps == 9 ? 3 : 1, ps = gm_ps(ncb);
    pl.nopad = (g.NO + 15) & ~15;
    pl.w_bytes = (taps * ncb + 3) / 4 * 4 * pl.nopad * 16;
    const int fixed = pl.w_bytes + (taps + 1) * GM_TILE_PIX * 4;
    const int budget = (GM_LDS_BYTES - fixed) / (terms * ps) - 1;     // patch pixels per term, the zero pixel aside
    auto need = [&](int tr, int tc) { return gm_span_cap(g.bwd, tr, g.s, ks, g.Hs) * gm_span_cap(g.bwd, tc, g.s, ks, g.Ws); };
    int tc = gm_min(g.Wd, GM_TILE_COLS);
    pl.tiles_c = (g.Wd + tc - 1) / tc;
    tc = (g.Wd + pl.tiles_c - 1) / pl.tiles_c;
    int tr = gm_min(g.Hd, GM_TILE_PIX / tc);
    int dec[2] = {0, 0};
    while (need(tr, tc) > budget) {                                   // a 1 x 1 tile needs 9 pixels: this ends
        if (tr > 1) --tr, ++dec[0];
        else --tc, ++dec[1];
    }
    if (shrunk) shrunk[0] = dec[0], shrunk[1] = dec[1];
    pl.tiles_c = (g.Wd + tc - 1) / tc;
    pl.tiles_r = (g.Hd + tr - 1) / tr;
    pl.TR = (g.Hd + pl.tiles_r - 1) / pl.tiles_r;
    pl.TC = (g.Wd + pl.tiles_c - 1) / pl.tiles_c;
    pl.npmax = need(pl.TR, pl.TC);
    pl.lds_bytes = fixed + terms * (pl.npmax + 1) * ps;
    const int64_t units = (int64_t)g.N * pl.tiles_r * pl.tiles_c;
    int64_t s = (GM_TARGET_WGS + g.G - 1) / g.G;
    if (s > units) s = units;
    pl.splits = (int)(s < 1 ? 1 : s);
    return pl;
}

// ---- the weight gradient: gmw_kernel (gconv_mfma.hip, three terms) and gwh_kernel (gconv_mfma_h.hip, one term) -----------------

constexpr int GMW_MAX_SPLITS = QT_GM_WGRAD_MAX_SPLITS;

struct GmwPlan {
    int TR, TC, tiles_r, tiles_c;
    int splits;
    int npmax;               // x patch pixels per term; pixel npmax is the zero pixel
    int gpix;                // go tile pixels per term: TR * TC rounded up to the chunk of 32
    int gvec;                // go is channels-last and 16-byte aligned (GmGeom::vec says so for x)
    int lds_bytes;
};

// floats of one (split, group) block of the partials: [tap][oc][ci], then the bias gradient [oc]
__host__ __device__ inline int64_t gmw_block(int taps, int cout_g, int cin_g) { return (int64_t)taps * cout_g * cin_g + cout_g; }

// the tile of the output map and the LDS it needs: as gm_plan, with the go tile beside the x patch (`terms` planes of each) and no
// weights.  A plan of fewer terms never has a smaller tile (the budget loop stops no later), so never more units or splits.
inline GmwPlan gmw_plan(const GmGeom& g, int taps, int ncbx, int rt, int terms, int* shrunk = nullptr) {
    GmwPlan pl{};
    const int ks = taps == 9 ? 3 : 1, psx = gm_ps(ncbx), psg = gm_ps(2 * rt);
    auto need = [&](int tr, int tc) { return gm_span_cap(0, tr, g.s, ks, g.Hs) * gm_span_cap(0, tc, g.s, ks, g.Ws); };
    auto bytes = [&](int tr, int tc) {
        return taps * GM_TILE_PIX * 4 + terms * ((tr * tc + 31) & ~31) * psg + terms * (need(tr, tc) + 1) * psx + 16;
    };
    int tc = gm_min(g.Wd, GM_TILE_COLS);
    pl.tiles_c = (g.Wd + tc - 1) / tc;
    tc = (g.Wd + pl.tiles_c - 1) / pl.tiles_c;
    int tr = gm_min(g.Hd, GM_TILE_PIX / tc);
    int dec[2] = {0, 0};
    while (bytes(tr, tc) > GM_LDS_BYTES) {                            // a 1 x 1 tile needs under 20 KiB: this ends
        if (tr > 1) --tr, ++dec[0];
        else --tc, ++dec[1];
    }
    if (shrunk) shrunk[0] = dec[0], shrunk[1] = dec[1];
    pl.tiles_c = (g.Wd + tc - 1) / tc;
    pl.tiles_r = (g.Hd + tr - 1) / tr;
    pl.TR = (g.Hd + pl.tiles_r - 1) / pl.tiles_r;
    pl.TC = (g.Wd + pl.tiles_c - 1) / pl.tiles_c;
    pl.npmax = need(pl.TR, pl.TC);
    pl.gpix = (pl.TR * pl.TC + 31) & ~31;
    pl.lds_bytes = bytes(pl.TR, pl.TC);
    const int64_t units = (int64_t)g.N * pl.tiles_r * pl.tiles_c;
    int64_t s = (GM_TARGET_WGS + g.G - 1) / g.G;
    if (s > GMW_MAX_SPLITS) s = GMW_MAX_SPLITS;
    if (s > units) s = units;
    pl.splits = (int)s;
    return pl;
}

inline GmGeom gmw_geom(int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int64_t Ho, int64_t Wo, int s, int ph,
                       int pw) {
    GmGeom g{};
    g.N = (int)N; g.G = (int)G; g.KC = (int)cin_g; g.NO = (int)cout_g;
    g.Hs = (int)H; g.Ws = (int)W; g.Hd = (int)Ho; g.Wd = (int)Wo;
    g.s = s; g.ph = ph; g.pw = pw;
    return g;
}

// Steps 1 to 3 of the documented validation order, shared by every entry: the sizes, the empty problem, the limits.  False: the
// call ends with `rc`; true: Ho x Wo is the output map of a problem inside the window.  `wide`: the channel window of
// gconv_wide_mfma.hip (cin_g and cout_g each one of 16, 24, 32, 40, 48, 64) in place of this family's.
inline bool gm_wide_channels(int64_t c) { return c == 16 || c == 24 || c == 32 || c == 40 || c == 48 || c == 64; }

inline bool gm_shape(int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                     int pw, int dh, int dw, int64_t& Ho, int64_t& Wo, int& rc, bool wide = false) {
    rc = QT_ERR_INVALID_ARG;
    if (N < 0 || G < 0 || cin_g < 1 || cout_g < 1 || H < 0 || W < 0 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 ||
        dh < 1 || dw < 1)
        return false;
    rc = QT_ERR_UNSUPPORTED;
    if ((int64_t)kh * kw > QT_DW_MAX_TAPS) return false;
    if (N == 0 || G == 0 || H == 0 || W == 0) {
        rc = QT_OK;
        return false;
    }
    if (wide ? !(gm_wide_channels(cin_g) && gm_wide_channels(cout_g))
             : (cin_g != 16 && cin_g != 24 && cin_g != 32) || (cout_g & 15) || cout_g > GM_MAX_COUT_G)
        return false;
    if (!((kh == 1 && kw == 1) || (kh == 3 && kw == 3)) || sh != sw || sh > 2 || dh != 1 || dw != 1 || ph > 1 || pw > 1) return false;
    if (N >= GM_MAX_ELEMS || G >= GM_MAX_ELEMS || H >= GM_MAX_ELEMS || W >= GM_MAX_ELEMS) return false;
    const int64_t eh = H + 2 * (int64_t)ph - kh, ew = W + 2 * (int64_t)pw - kw;
    if (eh < 0 || ew < 0) {                                       // the kernel does not fit the padded image
        rc = QT_ERR_INVALID_ARG;
        return false;
    }
    Ho = eh / sh + 1;
    Wo = ew / sw + 1;
    return (double)N * (double)(G * cin_g) * (double)H * (double)W < (double)GM_MAX_ELEMS &&
           (double)N * (double)(G * cout_g) * (double)Ho * (double)Wo < (double)GM_MAX_ELEMS &&
           (double)(G * cout_g) <= (double)QT_DW_MAX_CHANNELS;
}

// the gather's record of a problem gm_shape took: the source is x (forward) or go (grad_input); vec is the caller's to set
inline GmGeom gm_geom(bool bwd, int64_t N, int64_t G, int64_t cin_g, int64_t cout_g, int64_t H, int64_t W, int64_t Ho, int64_t Wo, int s,
                      int ph, int pw) {
    GmGeom g{};
    g.N = (int)N; g.G = (int)G;
    g.KC = (int)(bwd ? cout_g : cin_g); g.NO = (int)(bwd ? cin_g : cout_g);
    g.Hs = (int)(bwd ? Ho : H); g.Ws = (int)(bwd ? Wo : W); g.Hd = (int)(bwd ? H : Ho); g.Wd = (int)(bwd ? W : Wo);
    g.s = s; g.ph = ph; g.pw = pw; g.bwd = bwd ? 1 : 0;
    return g;
}

}  // namespace
