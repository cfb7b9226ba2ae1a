// What the streaming convs of dwconv.hip (depthwise) and gconv.hip (grouped) share: the element strides of a dense 4-D tensor, the
// thread map of a 256-thread workgroup over (channel, n, row, column), the weight quantiser of a tap and the host-side layout checks.
#pragma once
#include <type_traits>
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

// Element types of the "_h" entries (include/qt_hip.h "Depthwise and grouped convolution on half-precision operands").  A kernel
// template reads every operand through dw_ld (the exact upcast to fp32) and writes every result through dw_st (one rounding to
// nearest even), so its float instantiation is the fp32 kernel unchanged and the arithmetic between the two is the same code.
//   bf16: the pattern is the high half of the fp32 pattern; rounded on the integer pattern (a NaN keeps its sign and its high
//         payload bits and gets the quiet bit, so it cannot round to inf), no instruction whose mode could flush a subnormal.
//   fp16: v_cvt_f32_f16 / v_cvt_f16_f32 under hipcc's default modes (round to nearest even, fp16 subnormals kept on both sides).
struct DwBf16 { uint16_t bits; };
using DwF16 = _Float16;

__device__ __forceinline__ float dw_ld(float v) { return v; }
__device__ __forceinline__ float dw_ld(DwBf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }
__device__ __forceinline__ float dw_ld(DwF16 v) { return (float)v; }

__device__ __forceinline__ void dw_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void dw_st(DwBf16* p, float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t r = (u & 0x7fffffffu) > 0x7f800000u ? ((u >> 16) | 0x40u) : ((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    p->bits = (uint16_t)r;
}
__device__ __forceinline__ void dw_st(DwF16* p, float v) { *p = (DwF16)v; }

// Between a batch of T loads of XT elements and their dw_ld conversions.  For the half types hipcc otherwise pairs every 2-byte
// load with its conversion in ONE register — load, wait for it, convert, next load — so the batch is serialised on the memory
// latency (measured: the grouped 3 x 3 bf16 forward at 975 us against 540 us for the fp32 form, 431 us with the barrier).  The
// scheduling barrier keeps the loads of a batch together, as they are in the fp32 instantiation, which gets none and stays the
// code it was.  A batch of ONE load gets none either: there the loads that overlap are those of the unrolled channel loop around
// it, and a loop that holds the (convergent) barrier is not unrolled (measured on the grouped 1 x 1: 45 us without, 60 us with).
template <typename XT, int T>
__device__ __forceinline__ void dw_loads_issued() {
    if constexpr (!std::is_same<XT, float>::value && T > 1) __builtin_amdgcn_sched_barrier(0);
}

bool dw_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
// alignment of a pointer to elements of type T: 4 bytes for float, 2 for the half types
template <typename T>
bool dw_aligned_elt(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (sizeof(T) - 1)) == 0; }

// Runs `f` with a null pointer of the element type a "_h" dtype code names: f(activation type tag, weight type tag).  The weight
// is of the activation's type or fp32 (autocast).  false: the pair is not one the "_h" entries take.
template <typename F>
bool dw_half_types(int dtype, int w_dtype, F&& f) {
    if (dtype != QT_DTYPE_BF16 && dtype != QT_DTYPE_F16) return false;
    if (w_dtype != dtype && w_dtype != QT_DTYPE_F32) return false;
    if (dtype == QT_DTYPE_BF16) {
        if (w_dtype == QT_DTYPE_F32) f((DwBf16*)nullptr, (float*)nullptr);
        else f((DwBf16*)nullptr, (DwBf16*)nullptr);
    } else {
        if (w_dtype == QT_DTYPE_F32) f((DwF16*)nullptr, (float*)nullptr);
        else f((DwF16*)nullptr, (DwF16*)nullptr);
    }
    return true;
}

// 0 NCHW-contiguous, 1 channels-last, -1 neither, for a dense [N, C, H, W] tensor with these element strides
int dw_layout(int64_t N, int64_t C, int64_t H, int64_t W, const DwStrides& s) {
    if (s.w == 1 && s.h == W && s.c == H * W && s.n == C * H * W) return 0;
    if (s.c == 1 && s.w == C && s.h == W * C && s.n == H * W * C) return 1;
    return -1;
}

}  // namespace
