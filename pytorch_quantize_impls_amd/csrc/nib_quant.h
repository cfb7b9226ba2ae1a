// fp4-e2m1 nibble codes of the weight / activation quantisers (include/qt_hip.h "nibble planes": +1 = 0x2, -1 = 0xA, 0 = 0x0).
// One definition for every kernel that writes a nibble plane: the operand packers (mfma_gemm.hip) and the training update
// that emits the plane of the weight it has just stored (optim_step.hip).  The half overloads classify the 16-bit pattern
// through the element type E (qt_elt.h).
#pragma once
#include "qt_common.h"

struct NibSign {  // safeSign: +1 -> 0x2, -1 -> 0xA
    __device__ __forceinline__ static uint32_t nib(float x) { return x < 0.0f ? 0xAu : 0x2u; }
    template <class E> __device__ __forceinline__ static uint32_t nib(uint16_t h) { return E::neg(h) ? 0xAu : 0x2u; }
};
struct NibTernary {  // TernaryConnectDeterministic: 0 -> 0x0
    __device__ __forceinline__ static uint32_t nib(float x) {
        const float t = qt_ternarize(x);
        return t == 0.0f ? 0x0u : (t < 0.0f ? 0xAu : 0x2u);
    }
    template <class E> __device__ __forceinline__ static uint32_t nib(uint16_t h) {
        const int t = E::tern(h);
        return t == 0 ? 0x0u : (t < 0 ? 0xAu : 0x2u);
    }
};

struct NibSign0 {  // torch.sign: 0 (and NaN) -> 0x0 — the XNOR-Net weight image sign(W) (functions/xnor_connect.py:141)
    __device__ __forceinline__ static uint32_t nib(float x) { return x > 0.0f ? 0x2u : (x < 0.0f ? 0xAu : 0x0u); }
};
