// What the streaming convs of dwconv.hip (depthwise) and gconv.hip (grouped) share: the element strides of a dense 4-D tensor, the
// thread map of a 256-thread workgroup over (channel, n, row, column), the weight quantiser of a tap and the host-side layout checks.
#pragma once
#include "qt_common.h"

namespace {

constexpr int DW_THREADS = 256;

struct DwStrides { int64_t n, c, h, w; };

// how the 256 threads of a workgroup and its units cover (channel, n, row, column) of the tensor being walked
struct DwMap {
    int cl;              // 1: channels-last map
    int a_log, b_log;    // NCHW: log2 TW, log2 TH;   channels-last: log2 lanes along C, unused
    int slots;           // channels per workgroup
    int tiles_h, tiles_w;
    int Hm, Wm;          // the plane that is walked (Ho x Wo, or H x W for grad_input)
    int64_t chans;       // channels that are walked (C * m, or C)
    int64_t npix;        // N * Hm * Wm
    int units, splits;
    int64_t cgs;
};

inline int dw_pow2ceil(int64_t v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int dw_log2(int p) {
    int l = 0;
    while ((1 << l) < p) ++l;
    return l;
}

DwMap dw_plan(int cl, int64_t N, int64_t chans, int Hm, int Wm, int target_wgs) {
    DwMap mp{};
    mp.cl = cl;
    mp.Hm = Hm;
    mp.Wm = Wm;
    mp.chans = chans;
    mp.npix = N * Hm * Wm;
    if (cl) {
        const int tc = dw_pow2ceil(chans < 64 ? chans : 64);
        mp.a_log = dw_log2(tc);
        mp.slots = tc;
        const int tpix = DW_THREADS / tc;
        mp.units = (int)((mp.npix + tpix - 1) / tpix);
    } else {
        const int tw = dw_pow2ceil(Wm < 64 ? Wm : 64);
        int th = dw_pow2ceil(Hm);
        if (th > DW_THREADS / tw) th = DW_THREADS / tw;
        mp.a_log = dw_log2(tw);
        mp.b_log = dw_log2(th);
        mp.slots = DW_THREADS / (tw * th);
        mp.tiles_w = (Wm + tw - 1) / tw;
        mp.tiles_h = (Hm + th - 1) / th;
        mp.units = (int)(N * mp.tiles_h * mp.tiles_w);
    }
    mp.cgs = (chans + mp.slots - 1) / mp.slots;
    int64_t s = (target_wgs + mp.cgs - 1) / mp.cgs;
    if (s > mp.units) s = mp.units;
    if (s < 1) s = 1;
    mp.splits = (int)s;
    return mp;
}

__device__ __forceinline__ int dw_slot(const DwMap& mp, int tid) {
    return mp.cl ? (tid & (mp.slots - 1)) : (tid >> (mp.a_log + mp.b_log));
}

// position (n, h, w) that thread `tid` has in unit `u`; false when it lies outside the tensor
__device__ __forceinline__ bool dw_pos(const DwMap& mp, int u, int tid, int& n, int& h, int& w) {
    if (mp.cl) {
        const int64_t pix = (int64_t)u * (DW_THREADS >> mp.a_log) + (tid >> mp.a_log);
        if (pix >= mp.npix) return false;
        const int p = (int)pix;
        const int hw = mp.Hm * mp.Wm;
        n = p / hw;
        const int r = p - n * hw;
        h = r / mp.Wm;
        w = r - h * mp.Wm;
        return true;
    }
    const int per = mp.tiles_h * mp.tiles_w;
    n = u / per;
    const int r = u - n * per;
    const int th = r / mp.tiles_w;
    const int tw = r - th * mp.tiles_w;
    w = (tw << mp.a_log) + (tid & ((1 << mp.a_log) - 1));
    h = (th << mp.b_log) + ((tid >> mp.a_log) & ((1 << mp.b_log) - 1));
    return h < mp.Hm && w < mp.Wm;
}

__device__ __forceinline__ float dw_quant(int kind, float w) {
    return kind == QT_DW_SIGN ? qt_safe_sign(w) : (kind == QT_DW_TERNARY ? qt_ternarize(w) : w);
}

bool dw_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// 0 NCHW-contiguous, 1 channels-last, -1 neither, for a dense [N, C, H, W] tensor with these element strides
int dw_layout(int64_t N, int64_t C, int64_t H, int64_t W, const DwStrides& s) {
    if (s.w == 1 && s.h == W && s.c == H * W && s.n == C * H * W) return 0;
    if (s.c == 1 && s.w == C && s.h == W * C && s.n == H * W * C) return 1;
    return -1;
}

}  // namespace
