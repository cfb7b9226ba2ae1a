// Per-tap scaled implicit-GEMM convs: the XNOR-Net family on the matrix cores.
//
//   XNORConv2d (functions/xnor_connect.py:135-146, layers/xnor_layers.py:36-69):  y = conv2d(x, sign(W) * alpha),
//   alpha = mean(|W|, dim = [0, 1], keepdim) -> [1, 1, kh, kw]: ONE scale per filter tap.
//
// For +-1 activations (every layer behind a BinaryConnect) the conv factorises as  y = sum_taps alpha[i, j] * D[i, j]  with D the
// exact integer contraction over the input channels of one tap.  The implicit-GEMM kernel walks K tap-major,
// so the tap sums are formed on the fp4 matrix cores exactly as for BinConv2d and combined in Horner form on the accumulators
// (mfma_gemm_kernel.h, ElemFp4Taps): one fp4 pass + one VALU multiply per accumulator register per tap, instead of the six
// bf16 passes of a real x real conv.  The same holds for the gradient w.r.t. the input (xnor_connect.py:154-155): a real-valued
// gradient (two fp16 terms) against the flipped sign(W), alpha per flipped tap (ElemF16Taps).
//
// Entry points (include/qt_hip.h): qt_conv2d_implicit_taps (fp32 result), qt_conv2d_implicit_taps_bits / _nib (inference
// fusion: BatchNorm-threshold bits, or the next conv's nibble plane), qt_xnor_tap_prep_f32 (alpha + the Horner tables of a weight).
#include <cstdio>
#include "mfma_gemm_kernel.h"
#include "tile_select.h"
#include "xnor_alpha.h"

namespace {

// ---- alpha[c] = mean_r |W[r, c]|: the shared column-sum order of xnor_alpha.h (tap_abs_partial_kernel + tap_alpha_final) ----

// tables[0 .. T]      forward  : [1, rho_1 .. rho_{T-1}, a'_{T-1}],   rho_t = a'_{t-1} / a'_t
// tables[T+1 .. 2T+1] flipped  : the same for the reversed tap order (grad_x convolves with the flipped kernel)
// a' = alpha with zeros replaced by the previous non-zero entry (a tap whose alpha is 0 has all-zero weights: D_t = 0, any factor
// is right), leading zeros by the first non-zero one (or 1).
__global__ __launch_bounds__(1024) void tap_tables_kernel(const float* __restrict__ work, int nblk, float rows, const float* __restrict__ alpha_in,
                                                          int T, float* __restrict__ alpha, float* __restrict__ tables) {
    __shared__ float a[1024];
    __shared__ float stage[TAP_FINAL_STAGE];
    const int t = threadIdx.x;
    float s = 0.0f;
    if (!alpha_in) s = tap_alpha_final(work, nblk, T, t, rows, stage);        // (block-cooperative: every thread calls it)
    if (t < T) {
        if (alpha_in) s = alpha_in[t];
        a[t] = s;
        if (alpha) alpha[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        for (int dir = 0; dir < 2; ++dir) {
            float* tab = tables + dir * (T + 1);
            float first = 1.0f;
            for (int i = 0; i < T; ++i) {
                const float v = a[dir ? T - 1 - i : i];
                if (v != 0.0f) { first = v; break; }
            }
            float prev = first;
            tab[0] = 1.0f;
            for (int i = 0; i < T; ++i) {
                float v = a[dir ? T - 1 - i : i];
                if (!(v != 0.0f)) v = prev;            // zero (or NaN compares unequal: kept, poisons the result like upstream)
                if (i > 0) tab[i] = prev / v;
                prev = v;
            }
            tab[T] = prev;
        }
    }
}

// TileCfg (select_conv_taps, tile_select.h) -> launch: the configurations the per-tap scaled elements are instantiated for.
// A configuration outside this set is QT_ERR_UNSUPPORTED, never another kernel.  a: the arguments of launch_cfg.
template <class E, class... A>
int launch_taps(TileCfg cfg, A&&... a) {
    switch (cfg) {
        case TileCfg::ConvV128x128: return launch_cfg<ConvV128x128<E>>(a...);
        case TileCfg::ConvV128x64: return launch_cfg<ConvV128x64<E>>(a...);
        case TileCfg::ConvVSkinny: return launch_cfg<ConvVSkinny<E>>(a...);
        case TileCfg::ConvVPP256: return launch_cfg<ConvVPP256<E>>(a...);
        case TileCfg::ConvVPP192: return launch_cfg<ConvVPP192<E>>(a...);
        case TileCfg::ConvVPP256x192: return launch_cfg<ConvVPP256x192<E>>(a...);
        case TileCfg::ConvVPP128: return launch_cfg<ConvVPP128<E>>(a...);
        case TileCfg::ConvV64: return launch_cfg<ConvV64<E>>(a...);
        case TileCfg::ConvSkinny: return launch_cfg<ConvSkinny<E>>(a...);
        case TileCfg::Conv128x128: return launch_cfg<Conv128x128<E>>(a...);
        case TileCfg::ConvPP256: return launch_cfg<ConvPP256<E>>(a...);
        case TileCfg::ConvPP192: return launch_cfg<ConvPP192<E>>(a...);
        case TileCfg::ConvPP256x192: return launch_cfg<ConvPP256x192<E>>(a...);
        case TileCfg::ConvPP128: return launch_cfg<ConvPP128<E>>(a...);
        case TileCfg::Conv64: return launch_cfg<Conv64<E>>(a...);
        default: return QT_ERR_UNSUPPORTED;
    }
}

// What conv_taps_impl launches, worked out from the numbers alone (the describe entry point calls this and stops here).
struct TapsPlan {
    ConvArgs cg;
    int64_t M, K;
    TileCfg cfg;
};
int conv_taps_plan(int elem, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph,
                   int64_t pw, int64_t dh, int64_t dw, int64_t ldwp, int64_t ldy, int64_t Cout, EpiArgs& epi, bool has_rho, ConvPtrs ptrs, TapsPlan& pl) {
    if (elem != 0 && elem != 3) return QT_ERR_UNSUPPORTED;        // fp4 nibble planes / fp16 pair planes
    if (!has_rho) return QT_ERR_INVALID_ARG;
    if (Cw <= 0 || (Cw & 7)) return QT_ERR_ALIGNMENT;             // a tap = whole 32-byte MFMA k-steps
    bool valid;
    int64_t kwords, p_offset;
    const int rc = conv_geometry(elem, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, ldwp, ldy, Cout, epi, 0, 0, ptrs, pl.cg, valid, pl.M,
                                 pl.K, kwords, p_offset);
    if (rc != QT_OK) return rc;
    pl.cfg = select_conv_taps(pl.M, Cout, kwords * 4, ldwp, valid, epi.d2s_cout != 0, !epi.alpha && epi.mode == 0);
    return QT_OK;
}

int conv_taps_impl(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh,
                   int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat, int64_t ldwp, const float* bias,
                   float scale, const float* scale_dev, const float* tap_rho, float* Y, int64_t ldy, int64_t Cout, qt_stream_t stream,
                   EpiArgs epi) {
    TapsPlan pl;
    const int rc = conv_taps_plan(elem, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, ldwp, ldy, Cout, epi, tap_rho != nullptr,
                                  conv_check_pointers(P, Wmat, Y), pl);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    epi.tap_rho = tap_rho;
    epi.tap_ksteps = (int)(Cw / 8);
    epi.ntaps = (int)(kh * kw);
    if (elem == 0)
        return launch_taps<ElemFp4Taps>(pl.cfg, P, 0, Wmat, ldwp, bias, scale, scale_dev, Y, ldy, pl.M, Cout, pl.K, stream, pl.cg, epi);
    return launch_taps<ElemF16Taps>(pl.cfg, P, 0, Wmat, ldwp, bias, scale, scale_dev, Y, ldy, pl.M, Cout, pl.K, stream, pl.cg, epi);
}

}  // namespace

extern "C" {

int qt_conv2d_implicit_taps(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw,
                            int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat,
                            int64_t ldwp, const float* bias, float scale, const float* scale_dev, const float* tap_rho, float* Y,
                            int64_t ldy, int64_t Cout, qt_stream_t stream) {
    return conv_taps_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale, scale_dev, tap_rho, Y, ldy,
                          Cout, stream, EpiArgs{});
}

int qt_conv2d_implicit_taps_bits(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw,
                                 int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat,
                                 int64_t ldwp, const float* bias, float scale, const float* scale_dev, const float* tap_rho,
                                 const float* alpha, const float* beta, uint32_t* neg_plane, int64_t ldb, int64_t Cout,
                                 qt_stream_t stream) {
    if (!alpha || !beta) return QT_ERR_INVALID_ARG;
    if (ldb & 3) return QT_ERR_ALIGNMENT;
    EpiArgs epi;
    epi.alpha = alpha;
    epi.beta = beta;
    return conv_taps_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale, scale_dev, tap_rho,
                          reinterpret_cast<float*>(neg_plane), ldb, Cout, stream, epi);
}

int qt_conv2d_implicit_taps_nib(int elem, const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw,
                                int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat,
                                int64_t ldwp, const float* bias, float scale, const float* scale_dev, const float* tap_rho,
                                const float* alpha, const float* beta, uint32_t* nib_plane, int64_t ldn, int64_t Cout,
                                int64_t out_halo_h, int64_t out_halo_w, qt_stream_t stream) {
    if (!alpha || !beta) return QT_ERR_INVALID_ARG;
    if (out_halo_h < 0 || out_halo_w < 0 || out_halo_h > 64 || out_halo_w > 64) return QT_ERR_INVALID_ARG;
    if ((ldn & 3) || !qt_aligned16(nib_plane)) return QT_ERR_ALIGNMENT;
    if (ldn != (Cout + 31) / 32 * 4) return QT_ERR_INVALID_ARG;          // every word of a pixel is written by a column block
    EpiArgs epi;
    epi.alpha = alpha;
    epi.beta = beta;
    epi.mode = 3;
    epi.ohy = (int)out_halo_h;
    epi.ohx = (int)out_halo_w;
    return conv_taps_impl(elem, P, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, Wmat, ldwp, bias, scale, scale_dev, tap_rho,
                          reinterpret_cast<float*>(nib_plane), ldn, Cout, stream, epi);
}

int qt_conv2d_implicit_taps_describe(int elem, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh, int64_t sw,
                                     int64_t ph, int64_t pw, int64_t dh, int64_t dw, int64_t ldwp, int64_t Cout, int64_t in_halo_h,
                                     int64_t in_halo_w, int epilogue, int has_thr, int64_t d2s_cout, int variant, char* out, int cap) {
    // the arguments of qt_conv2d_implicit_describe; the per-tap scaled convs take no input halo, thresholds, depth-to-space or variant
    if (!out || cap < 2) return QT_ERR_INVALID_ARG;
    out[0] = 0;
    if (in_halo_h || in_halo_w || has_thr || d2s_cout || variant) return QT_ERR_INVALID_ARG;
    static const float some = 0.0f;        // "a pointer was given": nothing is read through it
    EpiArgs epi;
    int64_t ldy = Cout;
    if (epilogue == QT_EPI_BITS || epilogue == QT_EPI_NIB) {
        epi.alpha = epi.beta = &some;
        epi.mode = epilogue == QT_EPI_NIB ? 3 : 0;
        ldy = epilogue == QT_EPI_NIB ? (Cout + 31) / 32 * 4 : ((Cout + 31) / 32 + 3) & ~3ll;
    } else if (epilogue != QT_EPI_PLAIN) {
        return QT_ERR_INVALID_ARG;
    }
    TapsPlan pl;
    const int rc = conv_taps_plan(elem, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, ldwp, ldy, Cout, epi, true, ConvPtrs{true, true}, pl);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;      // nothing to do: QT_OK and an empty name
    snprintf(out, (size_t)cap, "%s<%s>", tile_cfg_name(pl.cfg), elem == 0 ? "ElemFp4Taps" : "ElemF16Taps");
    return QT_OK;
}

int qt_conv2d_implicit_taps_rows(const uint32_t* P, int64_t Nimg, int64_t H, int64_t W, int64_t Cw, int64_t kh, int64_t kw, int64_t sh,
                                 int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw, const uint32_t* Wmat, int64_t ldwp,
                                 const float* bias, const float* tap_rho, const float* a_plane, float* Y, int64_t ldy, int64_t Cout,
                                 qt_stream_t stream) {
    if (!tap_rho || !a_plane) return QT_ERR_INVALID_ARG;
    if (Cw <= 0 || (Cw & 7)) return QT_ERR_ALIGNMENT;
    if (kh * kw > 48) return QT_ERR_UNSUPPORTED;                  // (kh kw + 1) x 256 floats of LDS beside the stage buffers
    ConvArgs cg;
    EpiArgs epi;
    bool valid;
    int64_t M, K, kwords;
    int64_t p_offset;
    const int rc = conv_geometry(0, Nimg, H, W, Cw, kh, kw, sh, sw, ph, pw, dh, dw, ldwp, ldy, Cout, epi, 0, 0, conv_check_pointers(P, Wmat, Y),
                                 cg, valid, M, K, kwords, p_offset);
    if (rc != QT_OK) return rc > 0 ? QT_OK : rc;
    epi.tap_rho = tap_rho;
    epi.tap_ksteps = (int)(Cw / 8);
    epi.ntaps = (int)(kh * kw);
    epi.row_A = a_plane;
    epi.aH = (int)H; epi.aW = (int)W; epi.aph = (int)ph; epi.apw = (int)pw;
    // 256 x 128 tiles, double-buffered 128-byte stages, bounds-checked taps (the per-row factors need the accumulators in
    // VALU-addressable registers next to 16 factor registers: the 64-register accumulator tile)
    // (the 256 x 128 ping-pong tile measured slower here: AlexNet conv2 810 vs 752 us for the whole function, conv4 463 vs 444)
    return launch_cfg<Conv128<ElemFp4TapsRows>>(P, 0, Wmat, ldwp, bias, 1.0f, nullptr, Y, ldy, M, Cout, K, stream, cg, epi);
}

int64_t qt_xnor_tap_prep_work_floats(int64_t R, int64_t taps) {
    if (R <= 0 || taps <= 0 || taps > 1024) return 0;
    return (int64_t)tap_alpha_blocks(R, taps, nullptr) * taps;
}

int qt_xnor_tap_prep_f32(const float* w, int64_t R, int64_t taps, const float* alpha_in, float* work, float* alpha,
                         float* tables, qt_stream_t stream) {
    if (taps <= 0 || taps > 1024 || !tables) return QT_ERR_INVALID_ARG;
    int nblk = 0;
    if (!alpha_in) {
        if (!w || R <= 0 || !work) return QT_ERR_INVALID_ARG;
        int64_t rows_per_blk = 0;
        nblk = tap_alpha_blocks(R, taps, &rows_per_blk);
        hipLaunchKernelGGL(tap_abs_partial_kernel, dim3(nblk), dim3(1024), 0, (hipStream_t)stream, w, R, (int)taps, rows_per_blk, work);
    }
    hipLaunchKernelGGL(tap_tables_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, work, nblk, (float)R,
                       alpha_in, (int)taps, alpha, tables);
    return qt_check_launch();
}

}  // extern "C"
