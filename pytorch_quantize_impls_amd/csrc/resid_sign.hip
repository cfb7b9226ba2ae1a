// Residual blocks of the sign chain (include/qt_hip.h "BatchNorm + shortcut + sign"): one streaming pass over the fp32 conv result
//   t = fma(fl(fl(x - mean) * rs), weight, bias);  s = fl(t + r);  v = hardtanh(s);  bit = [v < 0]
// that writes the sum (the next block's shortcut) and the next conv's operand planes.
//
// Thread map.  One lane owns 4 consecutive channels of one NHWC row (a float4 of x, of a channels-last residual and of the sum), so
// neighbouring lanes read neighbouring 16-byte pieces of a row and rows follow each other: every stream is contiguous.  The 8 lanes
// of a 32-channel word lie in one aligned group of 8 lanes of a wave; each lane shifts its 4 bits to their place in the word and
// three xor-shuffles (1, 2, 4) or them together.  The group's first lane hands the word to dw_store_word (dw_planes.h), which writes
// the word of the sign plane, its four nibble words and the pad words — the stage the depthwise and grouped plane convs use.
// The alternative, a wave-level __ballot, yields one bit per LANE: with a lane per channel it gives two words per ballot but every
// lane then loads 4 bytes, not 16; with 4 channels per lane it takes 4 ballots and a bit interleave of the masks.  The per-lane
// assembly keeps the float4 streams and costs 3 cross-lane moves and 3 ors per 4 elements (DESIGN.md "Residual blocks in the sign
// chain" quotes the listing).
//
// An NCHW residual has its channels Ho Wo floats apart.  It goes through an LDS tile: 32 rows x 32 channels are read with the lanes
// ALONG THE PIXELS (32 consecutive floats of one channel plane per half wave), stored transposed, and consumed by the same
// 4-channels-per-lane map.  The tile pitch of 33 floats spreads both the writes and the reads over the banks.  A sum that is wanted
// in NCHW storage (the layout the module graph's own sum has behind an NCHW input) takes the same tile the other way round: every
// lane leaves its 4 values where it found its 4 residuals, and the lanes along the pixels write them out.
#include "qt_common.h"
#include "dw_planes.h"

namespace {

constexpr int RS_TILE = 32;          // rows and channels of the NCHW residual's LDS tile
constexpr int RS_PITCH = RS_TILE + 1;

struct RsArgs {
    const float* x;        // [rows][ldx]
    float* sum;            // [rows][lds], or NCHW (s_tile), or null; rows may be x itself (same pitch)
    const float* r;        // residual
    const float* weight;   // [C]
    const float* bias;     // [C]
    const float* stats;    // [mean | rs], 2 C
    int64_t ldx, lds, ldr; // ldr: row pitch of a channels-last residual
    int64_t rs_n, rs_c;    // NCHW residual: element strides of n and c (rs_h = Wo, rs_w = 1)
    int64_t ss_n, ss_c;    // NCHW sum: the same
    int r_tile, s_tile;    // the residual is read / the sum is written through the LDS tile (NCHW storage)
    int64_t rows;
    int C, nw;             // channels, 32-channel words per row
    int hw, wo;            // Ho * Wo, Wo
    int hardtanh;
    float lo, hi;
};

// BatchNorm constants of a lane's 4 channels: four 16-byte loads on the vector path (the per-channel vectors are 16-byte aligned
// there and C % 4 == 0), element by element otherwise
struct RsConsts { float mean[4], rs[4], w[4], b[4]; };

template <bool VEC>
__device__ __forceinline__ RsConsts rs_consts(const RsArgs& a, int c0, int live) {
    RsConsts k{};
    if (live <= 0) return k;
    if (VEC) {
        const float4 m = *reinterpret_cast<const float4*>(a.stats + c0), q = *reinterpret_cast<const float4*>(a.stats + a.C + c0);
        const float4 w = *reinterpret_cast<const float4*>(a.weight + c0), b = *reinterpret_cast<const float4*>(a.bias + c0);
        k.mean[0] = m.x; k.mean[1] = m.y; k.mean[2] = m.z; k.mean[3] = m.w;
        k.rs[0] = q.x; k.rs[1] = q.y; k.rs[2] = q.z; k.rs[3] = q.w;
        k.w[0] = w.x; k.w[1] = w.y; k.w[2] = w.z; k.w[3] = w.w;
        k.b[0] = b.x; k.b[1] = b.y; k.b[2] = b.z; k.b[3] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < live) {
                k.mean[e] = a.stats[c0 + e]; k.rs[e] = a.stats[a.C + c0 + e]; k.w[e] = a.weight[c0 + e]; k.b[e] = a.bias[c0 + e];
            }
    }
    return k;
}

// the 4 channels c0 ... c0 + 3 of one row, `live` of them inside C (0 ... 4): reads x and the residual — a channels-last one from
// memory, an NCHW one from column rt[e * RS_PITCH] of the LDS tile — writes the sum (rows to memory, an NCHW one to column
// st[e * RS_PITCH] of the tile), returns the 4 threshold bits
template <bool VEC>
__device__ __forceinline__ uint32_t rs_four(const RsArgs& a, const RsConsts& k, int64_t row, int c0, int live, const float* rt,
                                            float* st) {
    if (live <= 0) return 0u;
    float xv[4] = {0.f, 0.f, 0.f, 0.f}, rv[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    const float* xp = a.x + row * a.ldx + c0;
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(xp);
        xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < live) xv[e] = xp[e];
    }
    if (rt) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < live) rv[e] = rt[e * RS_PITCH];
    } else {
        const float* rp = a.r + row * a.ldr + c0;
        if (VEC) {
            const float4 q = *reinterpret_cast<const float4*>(rp);
            rv[0] = q.x; rv[1] = q.y; rv[2] = q.z; rv[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < live) rv[e] = rp[e];
        }
    }
    uint32_t bits = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < live) {
            // every step one rounding, the multiply-add fused: qt_bn_eval_device_f32's expression, then ONE fp32 add
            const float t = __fmaf_rn(__fmul_rn(__fsub_rn(xv[e], k.mean[e]), k.rs[e]), k.w[e], k.b[e]);
            const float s = __fadd_rn(t, rv[e]);
            // torch's hardtanh: a NaN fails both compares and stays
            v[e] = a.hardtanh ? (s < a.lo ? a.lo : (s > a.hi ? a.hi : s)) : s;
            bits |= qt_neg_bit(v[e]) << e;
        }
    }
    if (st) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < live) st[e * RS_PITCH] = v[e];
    } else if (a.sum) {
        float* sp = a.sum + row * a.lds + c0;
        if (VEC) {
            *reinterpret_cast<float4*>(sp) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < live) sp[e] = v[e];
        }
    }
    return bits;
}

// or of the 8 lanes of an aligned group of 8 (every lane of the wave executes this)
__device__ __forceinline__ uint32_t rs_or8(uint32_t w) {
    w |= (uint32_t)__shfl_xor((int)w, 1);
    w |= (uint32_t)__shfl_xor((int)w, 2);
    w |= (uint32_t)__shfl_xor((int)w, 4);
    return w;
}

__device__ __forceinline__ void rs_store(const DwPlaneOut& o, const DwGeom& g, const RsArgs& a, int64_t row, int wd, uint32_t word) {
    const int n = (int)(row / a.hw);
    const int rem = (int)(row - (int64_t)n * a.hw);
    const int ho = rem / a.wo;
    dw_store_word(o, g, wd, row, n, ho, rem - ho * a.wo, word);
}

// channels-last residual: item = (row, word, lane of 8), rows and words in memory order
template <bool VEC>
__global__ __launch_bounds__(DW_THREADS) void rs_rows_kernel(RsArgs a, DwPlaneOut o, DwGeom g) {
    const int tid = threadIdx.x;
    dw_zero_border(o, g, tid);
    const int per = a.nw * 8;
    const int64_t total = a.rows * per;
    const bool small = total < ((int64_t)1 << 32);      // (uniform) a 32-bit division serves
    // 256 lanes are whole rows (1, 2, 4, ... 32 words per row): a lane keeps its 4 channels from step to step, and their constants
    const bool fixed = (DW_THREADS % per) == 0;
    const int jf = tid % per;
    RsConsts kf = rs_consts<VEC>(a, jf * 4, fixed ? (a.C - jf * 4 < 4 ? a.C - jf * 4 : 4) : 0);
    // the loop bound is uniform over the workgroup: every lane takes part in the shuffles
    for (int64_t base = (int64_t)blockIdx.x * DW_THREADS; base < total; base += (int64_t)gridDim.x * DW_THREADS) {
        const int64_t item = base + tid;
        const bool in = item < total;
        const int64_t row = !in ? 0 : (small ? (int64_t)((uint32_t)item / (uint32_t)per) : item / per);
        const int j = in ? (int)(item - row * per) : 0;
        const int c0 = j * 4;
        const int live = in ? (a.C - c0 < 4 ? a.C - c0 : 4) : 0;
        const RsConsts k = fixed ? kf : rs_consts<VEC>(a, c0, live);
        const uint32_t bits = live > 0 ? rs_four<VEC>(a, k, row, c0, live, nullptr, nullptr) : 0u;
        const uint32_t word = rs_or8(bits << ((j & 7) * 4));
        if (in && (j & 7) == 0 && (o.sign || o.nib)) rs_store(o, g, a, row, j >> 3, word);
    }
}

// NCHW residual and / or NCHW sum: unit = (tile of 32 rows, word); r comes in and the sum goes out through an LDS tile
template <bool VEC>
__global__ __launch_bounds__(DW_THREADS) void rs_nchw_kernel(RsArgs a, DwPlaneOut o, DwGeom g) {
    __shared__ float tile[RS_TILE * RS_PITCH];          // [channel in word][row in tile]
    const int tid = threadIdx.x;
    dw_zero_border(o, g, tid);
    const int64_t tiles = (a.rows + RS_TILE - 1) / RS_TILE;
    const int64_t units = tiles * a.nw;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t t = u / a.nw;
        const int wd = (int)(u - t * a.nw);
        const int64_t row0 = t * RS_TILE;
        const int pl = tid & (RS_TILE - 1);        // lanes along the pixels: 32 consecutive rows are consecutive floats of a channel
        const int64_t prow = row0 + pl;            // plane (up to an image boundary)
        const int64_t pn = prow < a.rows ? prow / a.hw : 0;
        if (a.r_tile && prow < a.rows) {
            const float* rp = a.r + pn * a.rs_n + (prow - pn * a.hw);
#pragma unroll
            for (int pass = 0; pass < RS_TILE / 8; ++pass) {
                const int cl = (tid >> 5) + pass * 8;
                const int c = wd * 32 + cl;
                if (c < a.C) tile[cl * RS_PITCH + pl] = rp[(int64_t)c * a.rs_c];
            }
        }
        __syncthreads();
        {
            const int j = tid & 7, p = tid >> 3;
            const int64_t row = row0 + p;
            const bool in = row < a.rows;
            const int c0 = wd * 32 + j * 4;
            float* col = tile + j * 4 * RS_PITCH + p;
            const int live = in ? (a.C - c0 < 4 ? a.C - c0 : 4) : 0;
            const RsConsts k = rs_consts<VEC>(a, c0, live);
            const uint32_t bits = live > 0 ? rs_four<VEC>(a, k, row, c0, live, a.r_tile ? col : nullptr, a.s_tile ? col : nullptr) : 0u;
            const uint32_t word = rs_or8(bits << (j * 4));
            if (in && j == 0 && (o.sign || o.nib)) rs_store(o, g, a, row, wd, word);
        }
        __syncthreads();
        if (a.s_tile) {
            if (prow < a.rows) {
                float* sp = a.sum + pn * a.ss_n + (prow - pn * a.hw);
#pragma unroll
                for (int pass = 0; pass < RS_TILE / 8; ++pass) {
                    const int cl = (tid >> 5) + pass * 8;
                    const int c = wd * 32 + cl;
                    if (c < a.C) sp[(int64_t)c * a.ss_c] = tile[cl * RS_PITCH + pl];
                }
            }
            __syncthreads();
        }
    }
}

bool rs_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int qt_bn_add_sign_f32(const float* x, int64_t ldx, const float* weight, const float* bias, const float* bn_stats,
                                  const float* r, int64_t rs_n, int64_t rs_c, int64_t rs_h, int64_t rs_w, int hardtanh, float lo,
                                  float hi, float* sum, int64_t ss_n, int64_t ss_c, int64_t ss_h, int64_t ss_w, uint32_t* sign_plane,
                                  int64_t ldb, uint32_t* nib_plane, int64_t ldn, int64_t out_halo_h, int64_t out_halo_w, int64_t N,
                                  int64_t C, int64_t Ho, int64_t Wo, qt_stream_t stream) {
    // 1. negative sizes / halos
    if (N < 0 || C < 0 || Ho < 0 || Wo < 0 || out_halo_h < 0 || out_halo_w < 0) return QT_ERR_INVALID_ARG;
    // 2. an empty problem
    if (N == 0 || C == 0 || Ho == 0 || Wo == 0) return QT_OK;
    // 3. the limits
    if (out_halo_h > DW_MAX_HALO || out_halo_w > DW_MAX_HALO) return QT_ERR_UNSUPPORTED;
    const double lim = 2147483648.0;
    if ((double)N * (double)(Ho + 2 * out_halo_h) * (double)(Wo + 2 * out_halo_w) >= lim || (double)C >= lim ||
        (double)Ho * (double)Wo >= lim)
        return QT_ERR_UNSUPPORTED;
    const int64_t rows = N * Ho * Wo;
    // 4. arguments
    if (!x || !weight || !bias || !bn_stats || !r) return QT_ERR_INVALID_ARG;
    if (!sum && !sign_plane && !nib_plane) return QT_ERR_INVALID_ARG;
    if (hardtanh != 0 && hardtanh != 1) return QT_ERR_INVALID_ARG;
    if (hardtanh && !(lo <= hi)) return QT_ERR_INVALID_ARG;
    if (ldx < C) return QT_ERR_INVALID_ARG;
    const bool nchw = rs_w == 1 && rs_h == Wo && rs_c == Ho * Wo && rs_n == C * Ho * Wo;
    const bool cl = rs_c == 1 && rs_w >= C && rs_h == Wo * rs_w && rs_n == Ho * rs_h;
    if (!nchw && !cl) return QT_ERR_INVALID_ARG;
    // the sum: rows with a pitch (the channels-last form, checked first: at Ho Wo == 1 both forms describe rows) or dense NCHW
    const bool s_rows = ss_c == 1 && ss_w >= C && ss_h == Wo * ss_w && ss_n == Ho * ss_h;
    const bool s_nchw = !s_rows && ss_w == 1 && ss_h == Wo && ss_c == Ho * Wo && ss_n == C * Ho * Wo;
    if (sum && !s_rows && !s_nchw) return QT_ERR_INVALID_ARG;
    const int64_t lds = ss_w;
    if (sign_plane && ldb < dw_packed_ld(C)) return QT_ERR_INVALID_ARG;
    if (nib_plane && ldn < dw_pixel_ld_nib(C)) return QT_ERR_INVALID_ARG;
    if (sum) {
        // in place (same pointer, same pitch) or disjoint from x
        const uintptr_t xb = (uintptr_t)x, xe = xb + (uintptr_t)(((rows - 1) * ldx + C) * 4);
        const uintptr_t sb = (uintptr_t)sum, se = sb + (uintptr_t)((s_rows ? (rows - 1) * lds + C : rows * C) * 4);
        const bool same = s_rows && sb == xb && lds == ldx;
        if (!same && sb < xe && xb < se) return QT_ERR_INVALID_ARG;
    }
    // 5. alignment
    if (!rs_aligned4(x) || !rs_aligned4(weight) || !rs_aligned4(bias) || !rs_aligned4(bn_stats) || !rs_aligned4(r) ||
        !rs_aligned4(sum) || !rs_aligned4(sign_plane))
        return QT_ERR_ALIGNMENT;
    if (nib_plane && ((ldn & 3) || !dw_aligned16(nib_plane))) return QT_ERR_ALIGNMENT;

    RsArgs a{};
    a.x = x; a.sum = sum; a.r = r; a.weight = weight; a.bias = bias; a.stats = bn_stats;
    a.ldx = ldx; a.lds = lds; a.ldr = rs_w; a.rs_n = rs_n; a.rs_c = rs_c; a.ss_n = ss_n; a.ss_c = ss_c;
    a.r_tile = nchw ? 1 : 0;
    a.s_tile = (sum && s_nchw) ? 1 : 0;
    a.rows = rows; a.C = (int)C; a.nw = (int)((C + 31) / 32);
    a.hw = (int)(Ho * Wo); a.wo = (int)Wo;
    a.hardtanh = hardtanh; a.lo = lo; a.hi = hi;
    DwPlaneOut o{};
    o.sign = sign_plane; o.ldb = ldb; o.nib = nib_plane; o.ldn = ldn;
    o.hy = (int)out_halo_h; o.hx = (int)out_halo_w;
    DwGeom g{};
    g.N = (int)N; g.Ho = (int)Ho; g.Wo = (int)Wo; g.Cout = C;
    // 16-byte streams: every row piece of 4 channels is one aligned float4 of x, of the sum, of a channels-last residual and of the
    // per-channel constants
    const bool vec = (C & 3) == 0 && (ldx & 3) == 0 && dw_aligned16(x) && dw_aligned16(weight) && dw_aligned16(bias) &&
                     dw_aligned16(bn_stats) &&
                     (!sum || a.s_tile || ((lds & 3) == 0 && dw_aligned16(sum))) && (nchw || ((rs_w & 3) == 0 && dw_aligned16(r)));
    hipStream_t s = (hipStream_t)stream;
    if (a.r_tile || a.s_tile) {
        const int grid = qt_stream_grid((rows + RS_TILE - 1) / RS_TILE * a.nw);
        if (vec) hipLaunchKernelGGL(rs_nchw_kernel<true>, dim3(grid), dim3(DW_THREADS), 0, s, a, o, g);
        else hipLaunchKernelGGL(rs_nchw_kernel<false>, dim3(grid), dim3(DW_THREADS), 0, s, a, o, g);
    } else {
        const int grid = qt_stream_grid((rows * a.nw * 8 + DW_THREADS - 1) / DW_THREADS);
        if (vec) hipLaunchKernelGGL(rs_rows_kernel<true>, dim3(grid), dim3(DW_THREADS), 0, s, a, o, g);
        else hipLaunchKernelGGL(rs_rows_kernel<false>, dim3(grid), dim3(DW_THREADS), 0, s, a, o, g);
    }
    return qt_check_launch();
}
