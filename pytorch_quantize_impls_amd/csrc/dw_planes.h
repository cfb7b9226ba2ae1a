// What the plane-writing forwards of dwconv.hip (depthwise) and gconv.hip (grouped) share: the geometry record, the output planes of
// a launch, and the writing stage — one 32-channel word of threshold bits of one output pixel -> the word of the sign plane, its
// four nibble words, the pad words of the row — with the walk that zeroes the border of a halo plane and the host-side bounds of
// the planes.  include/qt_hip.h "Depthwise convolution on bit planes" states the formats.
#pragma once
#include <algorithm>
#include "dw_map.h"

namespace {

struct DwGeom {
    int N, C, m, H, W, Ho, Wo;
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int64_t Cout;
};

constexpr int DW_PIX_PER_STEP = DW_THREADS / 32;

struct DwPlaneOut {
    uint32_t* sign;      // [N Ho Wo][ldb] or null
    uint32_t* nib;       // [N (Ho + 2 hy) (Wo + 2 hx)][ldn] or null
    float* y;            // fp32 result by element strides, or null (then the planes are written)
    int64_t ldb, ldn;
    int hy, hx;
};

__device__ __forceinline__ uint32_t dw_spread8(uint32_t b) {
    uint32_t t = b & 0xFFu;
    t = (t | (t << 12)) & 0x000F000Fu;
    t = (t | (t << 6)) & 0x03030303u;
    t = (t | (t << 3)) & 0x11111111u;
    return t;
}

__device__ __forceinline__ void dw_store_zero4(uint32_t* p) { *reinterpret_cast<uint4*>(p) = make_uint4(0, 0, 0, 0); }

// the threshold bits of channels 32 wd ... 32 wd + 31 of output pixel pix = (n, ho, wo), bits of channels >= C m zero: the word of
// the sign plane, its four nibble words, and — with the last live word of a pixel — the pad words of both rows
__device__ __forceinline__ void dw_store_word(const DwPlaneOut& o, const DwGeom& g, int wd, int64_t pix, int n, int ho, int wo,
                                              uint32_t word) {
    const int nw = (int)((g.Cout + 31) >> 5);
    if (o.sign) {
        uint32_t* row = o.sign + pix * o.ldb;
        row[wd] = word;
        if (wd == nw - 1)
            for (int64_t t = nw; t < o.ldb; ++t) row[t] = 0u;
    }
    if (o.nib) {
        const int Hop = g.Ho + 2 * o.hy, Wop = g.Wo + 2 * o.hx;
        const int64_t left = g.Cout - (int64_t)wd * 32;
        const uint32_t mw = left >= 32 ? 0xFFFFFFFFu : ((1u << (int)left) - 1u);
        uint4 q;
        q.x = (dw_spread8(mw) << 1) | (dw_spread8(word) << 3);
        q.y = (dw_spread8(mw >> 8) << 1) | (dw_spread8(word >> 8) << 3);
        q.z = (dw_spread8(mw >> 16) << 1) | (dw_spread8(word >> 16) << 3);
        q.w = (dw_spread8(mw >> 24) << 1) | (dw_spread8(word >> 24) << 3);
        uint32_t* row = o.nib + (((int64_t)n * Hop + ho + o.hy) * Wop + wo + o.hx) * o.ldn;
        *reinterpret_cast<uint4*>(row + wd * 4) = q;
        if (wd == nw - 1)
            for (int64_t t = (int64_t)nw * 4; t < o.ldn; t += 4) dw_store_zero4(row + t);
    }
}

// the border pixels of a halo nibble plane, zeroed by a walk of the whole grid over the plane
__device__ __forceinline__ void dw_zero_border(const DwPlaneOut& o, const DwGeom& g, int tid) {
    if (!o.nib || !(o.hy || o.hx)) return;
    const int Hop = g.Ho + 2 * o.hy, Wop = g.Wo + 2 * o.hx;
    const int64_t groups = o.ldn / 4;
    const int64_t total = (int64_t)g.N * Hop * Wop * groups;
    for (int64_t e = (int64_t)blockIdx.x * DW_THREADS + tid; e < total; e += (int64_t)gridDim.x * DW_THREADS) {
        const int64_t pix = e / groups;
        const int rem = (int)(pix % ((int64_t)Hop * Wop));
        const int r = rem / Wop - o.hy, q = rem % Wop - o.hx;
        if ((unsigned)r >= (unsigned)g.Ho || (unsigned)q >= (unsigned)g.Wo) dw_store_zero4(o.nib + pix * o.ldn + (e - pix * groups) * 4);
    }
}

inline int64_t dw_packed_ld(int64_t K) {
    const int64_t kw = (K + 31) / 32;
    return std::max<int64_t>(4, (kw + 3) / 4 * 4);
}
inline int64_t dw_pixel_ld_nib(int64_t K) { return std::max<int64_t>(4, ((K + 7) / 8 + 3) / 4 * 4); }
bool dw_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr int DW_MAX_HALO = 64;

}  // namespace
