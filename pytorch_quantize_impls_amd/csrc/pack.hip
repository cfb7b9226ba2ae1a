// Bit-pack kernels: fp32 / bf16 / fp16 rows -> uint32 bit planes (include/qt_hip.h "Packed formats").
//
// HBM-bound (reads 4 or 2 B/element, writes 1/8 B/element per plane).  The kernels are templated on the
// encoder (what a bit means) and on the element type (qt_elt.h: how 16 bytes of the row are read and
// classified; the half types are classified on their bit pattern).  Two code paths:
//   * vec  : K % EPV == 0 (EPV = elements per 16-byte load: 4 fp32, 8 half), 16-byte aligned rows.
//            Each lane loads 16 bytes (a wave-load is 1 KiB contiguous), turns them into EPV bits, and
//            the 32 / EPV lanes that share a 32-element word OR their shifted bits together with DPP-class
//            lane exchanges; the first lane of each group stores the word.  Words past ceil(K/32) up to
//            ldp are written as zero by the same pass (the pad-is-zero invariant of the format).
//   * wave : any K / alignment.  Lane i of a wave loads element i of a 64-element chunk
//            (coalesced dwords) and a 64-bit wave ballot yields two words at once.
#include "qt_common.h"
#include "qt_elt.h"

namespace {

struct SignBits {
    static constexpr int NPLANES = 1;
    template <class E>
    __device__ __forceinline__ static void bits(typename E::scalar x, uint32_t& p0, uint32_t& p1) {
        p0 = E::neg(x);
        p1 = 0;
    }
};
struct TernaryBits {  // plane0 = mask (t != 0), plane1 = sign (t < 0)
    static constexpr int NPLANES = 2;
    template <class E>
    __device__ __forceinline__ static void bits(typename E::scalar x, uint32_t& p0, uint32_t& p1) {
        const auto t = E::tern(x);
        p0 = (t != 0) ? 1u : 0u;
        p1 = (t < 0) ? 1u : 0u;
    }
};

template <int LANES>   // OR over aligned groups of 8 (fp32) or 4 (half) lanes
__device__ __forceinline__ uint32_t or_reduce(uint32_t v) {
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    if (LANES == 8) v |= __shfl_xor(v, 4);
    return v;
}

// One row of packed output = ldp words = ldp*LPW 16-byte "slots" (LPW = 32 / EPV lanes per word; slots past
// K/EPV load nothing and contribute zero bits).  Work item = one slot; LPW consecutive slots = LPW consecutive
// lanes = 1 word.  ldp % 4 == 0 guarantees a row's slot count is a multiple of 16, and 64-lane waves start
// at multiples of 64 slots in the flattened (row, slot) index space, so a word never straddles
// two waves.  WRITE_IMG: also write the +-1 image of safeSign in the element type of the input.
template <class Enc, class E, bool WRITE_IMG>
__global__ __launch_bounds__(256) void pack_vec_kernel(const typename E::scalar* __restrict__ x, int64_t ldx,
                                                       uint32_t* __restrict__ p0,
                                                       uint32_t* __restrict__ p1, int64_t ldp,
                                                       typename E::scalar* __restrict__ yf, int64_t ldy,
                                                       int64_t rows, int64_t K) {
    constexpr int EPV = E::EPV, LPW = 32 / EPV;
    const int64_t slots_per_row = ldp * LPW;
    const int64_t total = rows * slots_per_row;
    const int64_t kv = K / EPV;  // K % EPV == 0 on this path
    const int lanew = threadIdx.x & (LPW - 1);
    // total % 16 == 0 and every LPW-lane group starts at a multiple of LPW, so a group is either
    // entirely inside the loop or entirely outside it: the cross-lane OR only ever reads lanes
    // that are active with it.
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total;
         s += (int64_t)gridDim.x * blockDim.x) {
        uint32_t b0 = 0, b1 = 0;
        const int64_t row = s / slots_per_row;
        const int64_t slot = s - row * slots_per_row;
        if (slot < kv) {
            const typename E::vec v = *reinterpret_cast<const typename E::vec*>(x + row * ldx + slot * EPV);
#pragma unroll
            for (int i = 0; i < EPV; ++i) {
                uint32_t a0, a1;
                Enc::template bits<E>(v.e[i], a0, a1);
                b0 |= a0 << i;
                b1 |= a1 << i;
            }
            if (WRITE_IMG) {
                typename E::vec r;
#pragma unroll
                for (int i = 0; i < EPV; ++i) r.e[i] = E::safe_sign(v.e[i]);
                *reinterpret_cast<typename E::vec*>(yf + row * ldy + slot * EPV) = r;
            }
        }
        const uint32_t w0 = or_reduce<LPW>(b0 << (EPV * lanew));
        if (lanew == 0) p0[row * ldp + slot / LPW] = w0;
        if (Enc::NPLANES == 2) {
            const uint32_t w1 = or_reduce<LPW>(b1 << (EPV * lanew));
            if (lanew == 0) p1[row * ldp + slot / LPW] = w1;
        }
    }
}

// Generic path: one wave per (row, 64-element chunk); chunks cover the padded row (ldp*32
// elements) so pad words are zeroed as well.
template <class Enc, class E, bool WRITE_IMG>
__global__ __launch_bounds__(256) void pack_wave_kernel(const typename E::scalar* __restrict__ x, int64_t ldx,
                                                        uint32_t* __restrict__ p0,
                                                        uint32_t* __restrict__ p1, int64_t ldp,
                                                        typename E::scalar* __restrict__ yf, int64_t ldy,
                                                        int64_t rows, int64_t K) {
    const int lane = threadIdx.x & 63;
    const int64_t chunks_per_row = ldp / 2;  // ldp % 4 == 0
    const int64_t total = rows * chunks_per_row;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = wave; c < total; c += nwaves) {
        const int64_t row = c / chunks_per_row;
        const int64_t ch = c - row * chunks_per_row;
        const int64_t k = ch * 64 + lane;
        uint32_t b0 = 0, b1 = 0;
        if (k < K) {
            const typename E::scalar v = x[row * ldx + k];
            Enc::template bits<E>(v, b0, b1);
            if (WRITE_IMG) yf[row * ldy + k] = E::safe_sign(v);
        }
        const unsigned long long m0 = __ballot(b0 != 0);
        if (lane < 2) p0[row * ldp + ch * 2 + lane] = (uint32_t)(m0 >> (32 * lane));
        if (Enc::NPLANES == 2) {
            const unsigned long long m1 = __ballot(b1 != 0);
            if (lane < 2) p1[row * ldp + ch * 2 + lane] = (uint32_t)(m1 >> (32 * lane));
        }
    }
}

template <class Enc, class E, bool WRITE_IMG>
int launch_pack(const typename E::scalar* x, int64_t ldx, uint32_t* p0, uint32_t* p1, int64_t ldp,
                typename E::scalar* yf, int64_t ldy, int64_t rows, int64_t K, qt_stream_t stream) {
    if (rows < 0 || K < 0 || ldx < K || ldp < 0) return QT_ERR_INVALID_ARG;
    if (rows == 0) return QT_OK;
    if (!x && K > 0) return QT_ERR_INVALID_ARG;
    if (!p0 || (Enc::NPLANES == 2 && !p1)) return QT_ERR_INVALID_ARG;
    if (WRITE_IMG && (!yf || ldy < K)) return QT_ERR_INVALID_ARG;
    const int64_t kw = (K + 31) / 32;
    if (ldp < kw || (ldp & 3) != 0) return QT_ERR_ALIGNMENT;
    if (!qt_aligned16(p0) || (Enc::NPLANES == 2 && !qt_aligned16(p1))) return QT_ERR_ALIGNMENT;
    if (ldp == 0) return QT_OK;
    constexpr int EPV = E::EPV;
    const bool vec = (K % EPV == 0) && (ldx % EPV == 0) && qt_aligned16(x) &&
                     (!WRITE_IMG || ((ldy % EPV == 0) && qt_aligned16(yf)));
    if (vec) {
        const int64_t total = rows * ldp * (32 / EPV);
        const int grid = qt_stream_grid((total + 255) / 256);
        hipLaunchKernelGGL((pack_vec_kernel<Enc, E, WRITE_IMG>), dim3(grid), dim3(256), 0,
                           (hipStream_t)stream, x, ldx, p0, p1, ldp, yf, ldy, rows, K);
    } else {
        const int64_t total_waves = rows * (ldp / 2);
        const int grid = qt_stream_grid((total_waves + 3) / 4);
        hipLaunchKernelGGL((pack_wave_kernel<Enc, E, WRITE_IMG>), dim3(grid), dim3(256), 0,
                           (hipStream_t)stream, x, ldx, p0, p1, ldp, yf, ldy, rows, K);
    }
    return qt_check_launch();
}

template <class E>
__global__ __launch_bounds__(256) void check_pm1_kernel(const typename E::scalar* __restrict__ x, int64_t n,
                                                        int32_t* __restrict__ flag) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        bad |= !E::is_pm1(x[i]);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// 16-byte loads (half types: 8 elements per lane); x is 16-byte aligned, the n % EPV tail elements are looked
// at by the first lanes of workgroup 0.
template <class E>
__global__ __launch_bounds__(256) void check_pm1_vec_kernel(const typename E::scalar* __restrict__ x, int64_t n,
                                                            int32_t* __restrict__ flag) {
    constexpr int EPV = E::EPV;
    const int64_t nv = n / EPV;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (int64_t)gridDim.x * blockDim.x) {
        const typename E::vec v = reinterpret_cast<const typename E::vec*>(x)[i];
#pragma unroll
        for (int e = 0; e < EPV; ++e) bad |= !E::is_pm1(v.e[e]);
    }
    if (blockIdx.x == 0 && nv * EPV + threadIdx.x < n) bad |= !E::is_pm1(x[nv * EPV + threadIdx.x]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

template <class E>
int launch_check_pm1(const typename E::scalar* x, int64_t n, int32_t* flag, qt_stream_t stream) {
    if (n < 0 || !flag || (n > 0 && !x)) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    if constexpr (E::EPV == 8) {               // half types: 16-byte loads whenever the base allows them
        if (qt_aligned16(x)) {
            const int grid = qt_stream_grid((n / E::EPV + 1023) / 1024);
            hipLaunchKernelGGL(check_pm1_vec_kernel<E>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, flag);
            return qt_check_launch();
        }
    }
    const int grid = qt_stream_grid((n + 2047) / 2048);   // fp32: the dword-per-lane kernel, as ever
    hipLaunchKernelGGL(check_pm1_kernel<E>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, flag);
    return qt_check_launch();
}

template <class E>
int sign_pack_any(const void* xv, int64_t ldx, uint32_t* sign_plane, int64_t ldp, void* yv, int64_t ldy, int64_t rows,
                  int64_t K, qt_stream_t stream) {
    using S = typename E::scalar;
    const S* x = static_cast<const S*>(xv);
    S* y = static_cast<S*>(yv);
    if (y) return launch_pack<SignBits, E, true>(x, ldx, sign_plane, nullptr, ldp, y, ldy, rows, K, stream);
    return launch_pack<SignBits, E, false>(x, ldx, sign_plane, nullptr, ldp, nullptr, 0, rows, K, stream);
}

}  // namespace

extern "C" {

int qt_sign_pack_f32(const float* x, int64_t ldx, uint32_t* sign_plane, int64_t ldp, float* y_f32,
                     int64_t ldy, int64_t rows, int64_t K, qt_stream_t stream) {
    return sign_pack_any<EltF32>(x, ldx, sign_plane, ldp, y_f32, ldy, rows, K, stream);
}

int qt_ternary_pack_f32(const float* x, int64_t ldx, uint32_t* mask_plane, uint32_t* sign_plane,
                        int64_t ldp, int64_t rows, int64_t K, qt_stream_t stream) {
    return launch_pack<TernaryBits, EltF32, false>(x, ldx, mask_plane, sign_plane, ldp, nullptr, 0, rows, K,
                                                   stream);
}

int qt_check_pm1_f32(const float* x, int64_t n, int32_t* flag, qt_stream_t stream) {
    return launch_check_pm1<EltF32>(x, n, flag, stream);
}

int qt_sign_pack_h(const void* x, int dtype, int64_t ldx, uint32_t* sign_plane, int64_t ldp, void* y, int64_t ldy,
                   int64_t rows, int64_t K, qt_stream_t stream) {
    if (dtype == QT_DTYPE_BF16) return sign_pack_any<EltBf16>(x, ldx, sign_plane, ldp, y, ldy, rows, K, stream);
    if (dtype == QT_DTYPE_F16) return sign_pack_any<EltF16>(x, ldx, sign_plane, ldp, y, ldy, rows, K, stream);
    return QT_ERR_INVALID_ARG;
}

int qt_ternary_pack_h(const void* x, int dtype, int64_t ldx, uint32_t* mask_plane, uint32_t* sign_plane, int64_t ldp,
                      int64_t rows, int64_t K, qt_stream_t stream) {
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    if (dtype == QT_DTYPE_BF16)
        return launch_pack<TernaryBits, EltBf16, false>(xh, ldx, mask_plane, sign_plane, ldp, nullptr, 0, rows, K, stream);
    if (dtype == QT_DTYPE_F16)
        return launch_pack<TernaryBits, EltF16, false>(xh, ldx, mask_plane, sign_plane, ldp, nullptr, 0, rows, K, stream);
    return QT_ERR_INVALID_ARG;
}

int qt_check_pm1_h(const void* x, int dtype, int64_t n, int32_t* flag, qt_stream_t stream) {
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    if (dtype == QT_DTYPE_BF16) return launch_check_pm1<EltBf16>(xh, n, flag, stream);
    if (dtype == QT_DTYPE_F16) return launch_check_pm1<EltF16>(xh, n, flag, stream);
    return QT_ERR_INVALID_ARG;
}

}  // extern "C"
