// Does the fp4 GEMM's MFMA shape change the clock the chip holds under load?  Two loops with the register and LDS
// shape of mfma_gemm.hip's 256x256 ping-pong tile: 8 waves per workgroup (2 per SIMD), one workgroup per CU on every CU,
// a 128x64 wave tile, random +-1 fp4 operands re-read from LDS by ds_read_b128 every 128-element K slice:
//   32x32x64  (v_mfma_scale_f32_32x32x64_f8f6f4):  4 x 2 blocks, 2 k-steps -> 16 MFMAs + 12 fragment reads per slice
//   16x16x128 (v_mfma_scale_f32_16x16x128_f8f6f4): 8 x 4 blocks, 1 k-step  -> 32 MFMAs + 12 fragment reads per slice
// Both do the same FLOP, the same LDS bytes and hold 128 accumulator VGPRs.  After >= 2 s of back-to-back launches of
// one shape, 20 launches are timed by events (wall FLOP/s), and every workgroup stamps s_memtime / s_memrealtime
// around its loop (in-kernel clock = d(memtime) / d(memrealtime) x 100 MHz, median over workgroups).  Stamps go to a
// buffer of their own.  Zero operands are run too, as the control where the two shapes should tie.
// Build: hipcc --offload-arch=gfx950 -O3 mfma_shape_power.hip -o mfma_shape_power ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); exit(1);} } while (0)

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int ROWS = 256, STAGE = 64, NSTAGE = 2;        // 256 rows x 64 bytes (128 fp4) per operand and stage
constexpr int OP_BYTES = ROWS * STAGE, BUF = 2 * OP_BYTES; // [X | W] per stage

// 4 chunks per 64-byte row: the 16 rows of a ds_read_b128 lane group land on 16 distinct 16-byte slots of a 256-byte bank row
__device__ __forceinline__ int swz(int row, int c) { return c ^ ((row >> 2) & 3); }

template <int SHAPE>   // 0 = 32x32x64, 1 = 16x16x128
__global__ __launch_bounds__(512, 1) void k_shape(const uint4* __restrict__ data, float* out, int iters,
                                                  unsigned long long* ts) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[NSTAGE * BUF];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 2, wn = wave & 3;
    for (int i = t; i < NSTAGE * BUF / 16; i += 512) reinterpret_cast<uint4*>(lds)[i] = data[(size_t)blockIdx.x * (NSTAGE * BUF / 16) + i];
    __syncthreads();
    constexpr int TMW = SHAPE == 0 ? 4 : 8, TNW = SHAPE == 0 ? 2 : 4, BR = SHAPE == 0 ? 32 : 16;
    using acc_t = typename std::conditional<SHAPE == 0, v16f, v4f>::type;
    constexpr int NR = SHAPE == 0 ? 16 : 4;
    acc_t c[TMW][TNW];
    for (int i = 0; i < TMW; ++i)
        for (int j = 0; j < TNW; ++j)
            for (int r = 0; r < NR; ++r) c[i][j][r] = 0.f;
    const int lrow = SHAPE == 0 ? (lane & 31) : (lane & 15), lch = SHAPE == 0 ? (lane >> 5) : (lane >> 4);
    __syncthreads();
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), w0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
        const unsigned char* xs = lds + (it & 1) * BUF;
        const unsigned char* ws = xs + OP_BYTES;
        constexpr int KS = SHAPE == 0 ? 2 : 1;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            uint4 a[TMW], b[TNW];
            const int ch = kk * 2 + lch;
#pragma unroll
            for (int i = 0; i < TMW; ++i) {
                const int row = (wm * TMW + i) * BR + lrow;
                a[i] = *reinterpret_cast<const uint4*>(xs + row * STAGE + swz(row, ch) * 16);
            }
#pragma unroll
            for (int j = 0; j < TNW; ++j) {
                const int row = (wn * TNW + j) * BR + lrow;
                b[j] = *reinterpret_cast<const uint4*>(ws + row * STAGE + swz(row, ch) * 16);
            }
#pragma unroll
            for (int i = 0; i < TMW; ++i)
#pragma unroll
                for (int j = 0; j < TNW; ++j) {
                    const v8i av = {(int)a[i].x, (int)a[i].y, (int)a[i].z, (int)a[i].w, 0, 0, 0, 0};
                    const v8i bv = {(int)b[j].x, (int)b[j].y, (int)b[j].z, (int)b[j].w, 0, 0, 0, 0};
                    if constexpr (SHAPE == 0)
                        c[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c[i][j], 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
                    else
                        c[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c[i][j], 4, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
                }
        }
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), w1 = __builtin_amdgcn_s_memrealtime();
    float s = 0;
    for (int i = 0; i < TMW; ++i)
        for (int j = 0; j < TNW; ++j)
            for (int r = 0; r < NR; ++r) s += c[i][j][r];
    out[blockIdx.x * 512 + t] = s;
    if (t == 0) { ts[blockIdx.x * 2] = c1 - c0; ts[blockIdx.x * 2 + 1] = w1 - w0; }
}

template <int SHAPE>
void launch(int blocks, const uint4* d, float* out, int iters, unsigned long long* ts) {
    hipLaunchKernelGGL(k_shape<SHAPE>, dim3(blocks), dim3(512), 0, 0, d, out, iters, ts);
}

int main(int argc, char** argv) {
    const double soak_s = argc > 1 ? atof(argv[1]) : 2.5;
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int blocks = prop.multiProcessorCount;
    printf("device %s, %d CUs; 8 waves / CU, wave tile 128x64, soak %.1f s per case\n", prop.gcnArchName, blocks, soak_s);
    const size_t nvec = (size_t)blocks * NSTAGE * BUF / 16;
    std::vector<uint32_t> h(nvec * 4);
    uint4* d; float* out; unsigned long long* ts;
    CK(hipMalloc(&d, nvec * 16)); CK(hipMalloc(&out, (size_t)blocks * 512 * 4)); CK(hipMalloc(&ts, blocks * 16));
    std::vector<unsigned long long> hts(blocks * 2);
    const int iters = 40000;   // 128-element K slices per launch: ~ 10 ms
    for (int dk = 0; dk < 2; ++dk) {
        uint64_t st = 0x9e3779b97f4a7c15ull;
        for (auto& w : h) {
            if (dk == 0) w = 0;
            else {
                st = st * 6364136223846793005ull + 1442695040888963407ull;
                const uint32_t r = (uint32_t)(st >> 32);
                uint32_t v = 0;
                for (int n = 0; n < 8; ++n) v |= (((r >> n) & 1) ? 0xAu : 0x2u) << (4 * n);
                w = v;
            }
        }
        CK(hipMemcpy(d, h.data(), nvec * 16, hipMemcpyHostToDevice));
        double tf[2] = {0, 0};
        for (int shape = 0; shape < 2; ++shape) {
            auto go = [&]() { if (shape == 0) launch<0>(blocks, d, out, iters, ts); else launch<1>(blocks, d, out, iters, ts); };
            const auto t0 = std::chrono::steady_clock::now();
            int soaked = 0;
            while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < soak_s) {
                for (int i = 0; i < 10; ++i) go();
                CK(hipGetLastError());
                CK(hipDeviceSynchronize());
                soaked += 10;
            }
            hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
            const int reps = 20;
            CK(hipEventRecord(e0));
            for (int i = 0; i < reps; ++i) go();
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(hts.data(), ts, blocks * 16, hipMemcpyDeviceToHost));
            std::vector<double> clk(blocks);
            for (int b = 0; b < blocks; ++b) clk[b] = (double)hts[2 * b] / (double)hts[2 * b + 1] * 100.0;
            std::sort(clk.begin(), clk.end());
            const double per_launch_us = ms * 1e3 / reps;
            const double flop = 2.0 * 256 * 256 * 128 * (double)iters * blocks;   // per launch
            tf[shape] = flop / per_launch_us / 1e6;
            const double cyc = (double)hts[0] / (double)iters;                      // memtime ticks per K slice, block 0
            printf("%-10s %-9s soak %4d launches: %8.1f us/launch  %8.1f TFLOP/s (wall)  in-kernel clock median %.0f MHz (min %.0f max %.0f)  "
                   "memtime ticks / K slice (blk 0) %.1f\n",
                   dk ? "random+-1" : "zeros", shape ? "16x16x128" : "32x32x64", soaked, per_launch_us, tf[shape], clk[blocks / 2],
                   clk[0], clk[blocks - 1], cyc);
            CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
        }
        printf("%-10s 16x16x128 / 32x32x64 wall FLOP/s = %.3f\n", dk ? "random+-1" : "zeros", tf[1] / tf[0]);
    }
    CK(hipFree(d)); CK(hipFree(out)); CK(hipFree(ts));
    return 0;
}
