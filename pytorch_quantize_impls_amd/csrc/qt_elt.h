// Element types of the operand packers: how 16 bytes of a row are read and how one element is classified.
//
//   EltF32  : float, 4 per 16-byte load; IEEE compares (qt_common.h: -0.0 and NaN are not negative, subnormals
//             compare un-flushed).
//   EltBf16 / EltF16 : the 16-bit pattern, 8 per 16-byte load.  Classified with integer compares on the pattern,
//             so the answer does not depend on the kernel's denormal mode (fp16 has subnormals in everyday ranges):
//               x < 0      <=> sign bit set, magnitude in [1, INF]          (-0.0, NaN -> not negative)
//               x >= 0.5   <=> sign bit clear, magnitude >= HALF; x < -0.5 <=> sign bit set, magnitude in (HALF, INF]
//               NaN ternarises to +1 like the fp32 formula (s + safeSign(x - 0.5 s)) / 2 with s = safeSign(NaN) = +1
//               x is +-1   <=> magnitude == ONE
#pragma once
#include "qt_common.h"

struct EltF32 {
    using scalar = float;
    static constexpr int EPV = 4;
    struct alignas(16) vec { float e[4]; };
    __device__ __forceinline__ static uint32_t neg(float x) { return qt_neg_bit(x); }
    __device__ __forceinline__ static float tern(float x) { return qt_ternarize(x); }
    __device__ __forceinline__ static float safe_sign(float x) { return qt_safe_sign(x); }
    __device__ __forceinline__ static bool is_pm1(float x) { return x == 1.0f || x == -1.0f; }
};

template <uint32_t INF, uint32_t HALF, uint32_t ONE>
struct EltHalfBits {
    using scalar = uint16_t;
    static constexpr int EPV = 8;
    struct alignas(16) vec { uint16_t e[8]; };
    __device__ __forceinline__ static uint32_t neg(uint16_t h) {          // pattern in [0x8001, 0x8000 + INF]
        return ((uint32_t)h - 0x8001u) <= (INF - 1u) ? 1u : 0u;
    }
    __device__ __forceinline__ static int tern(uint16_t h) {
        const uint32_t mag = h & 0x7fffu;
        if (mag > INF) return 1;                                          // NaN
        if (h & 0x8000u) return mag > HALF ? -1 : 0;
        return mag >= HALF ? 1 : 0;
    }
    __device__ __forceinline__ static uint16_t safe_sign(uint16_t h) { return (uint16_t)(ONE | (neg(h) << 15)); }
    __device__ __forceinline__ static bool is_pm1(uint16_t h) { return (h & 0x7fffu) == ONE; }
};
using EltBf16 = EltHalfBits<0x7f80u, 0x3f00u, 0x3f80u>;
using EltF16 = EltHalfBits<0x7c00u, 0x3800u, 0x3c00u>;
