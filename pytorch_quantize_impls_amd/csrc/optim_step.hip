// Training update: one multi-tensor launch per parameter group (include/qt_hip.h "Training update").
//
// For every tensor of a host table the kernel applies the optimiser recurrence (torch.optim.SGD / torch.optim.Adam,
// one rounding per operation, -ffp-contract=off), clamps the value it is about to store to the tensor's [lo, hi]
// (what the layer's clamp() would do in a second pass) and, for the weight of a deterministic LinearBin / LinearTer,
// writes the fp4 nibble plane of that stored value: the operand the next training forward would otherwise produce by
// reading the whole fp32 weight again.
//
// HBM-bound: 3 (SGD) or 4 (Adam) fp32 streams read, 2 or 3 written, 1/8 of one stream for a plane.  No LDS, no
// cross-lane traffic, plain vector stores.
//
//   * The table travels as a BY-VALUE kernel argument in chunks of QT_OPTIM_CHUNK descriptors: no device allocation
//     and no host-to-device copy per step.  Next to the descriptors a chunk carries the prefix sums of the tensors'
//     UNITS; a workgroup walks units grid-strided and finds its tensor by advancing a (wave-uniform) index along the
//     prefix, so the grid is sized from the whole chunk, not from one tensor.
//   * flat tensors: unit = 4096 consecutive elements.  16-byte loads / stores when every pointer of the tensor is
//     16-byte aligned (full units: four independent dwordx4 per stream and lane in flight; the numel % 4 tail goes
//     to the first lanes of the last unit), a dword-per-lane walk otherwise (views at odd element offsets).
//   * plane tensors ([rows, K] weight, plane [rows, ld] words): unit = 512 plane words, walked by (row, word).  One
//     lane owns the 8 consecutive K elements of one word (two dwordx4 per stream when K % 4 == 0 and the pointers
//     allow it, scalar otherwise) and stores the word; words from ceil(K/8) to ld and the tail nibbles of a row's
//     last word are written as zero, so the plane may be uninitialised memory.
//   * per-step scalars (learning rate; Adam's bias corrections c0, c1) reach the recurrence through a SOURCE type: the
//     by-value entries take them from the argument block / the descriptor, the `_dev` entries (qt_optim_sgd_dev_f32 /
//     qt_optim_adam_dev_f32) from device memory, so that a launch captured in a hipGraph sees the values of the step
//     it is replayed for.  A workgroup reads them once per tensor it walks (a wave-uniform load where the tensor index
//     advances), never per element; the arithmetic is the same template, so equal scalars give equal bits.  Adam's
//     `coef` is indexed by the TABLE index of a tensor: a chunk carries, per slot, the table index relative to its
//     first slot (empty tensors are dropped, later chunks start anywhere) and the launch gets `coef` rebased to that.
//     qt_optim_scalars_f32 is how the host gets them there between replays: a launch whose ARGUMENT BLOCK carries the values
//     (up to 960 floats per launch), stream-ordered like any kernel, with no staging buffer for a later call to overwrite.
//   * the `_dev_guard` entries (qt_optim_sgd_dev_guard_f32 / qt_optim_adam_dev_guard_f32) are the `_dev` entries behind one
//     device word: every workgroup reads *skip once, before it touches a tensor, and leaves when it is non-zero — how a
//     captured training step keeps parameters, state and planes untouched when one of its trusted route verdicts turned out
//     wrong (utils.GraphedTrainStep(recover=True)).  Same body, so *skip == 0 stores the bits of the `_dev` entries.
//     qt_flags_or_i32 folds the step's verdict flags into that word: the flag POINTERS travel by value, 448 per launch.
//   * kernel-argument size: OptimChunk = 32 x 96 (descriptors) + 33 x 4 (unit prefix) + 32 x 4 (table indices) + 4 (n)
//     + 4 (padding) = 3336 bytes; the largest rule (Adam from device memory) adds 32 and the guard
//     pointer 8: 3376 of HIP's 4096 bytes.
#include "qt_common.h"
#include "nib_quant.h"

#define QT_OPTIM_CHUNK 32

namespace {

constexpr int FLAG_FIRST = 1;          // public: first step of an SGD momentum buffer (buf = grad)
constexpr int FLAG_VEC = 1 << 8;       // library-internal: every pointer 16-byte aligned (plane tensors: and K % 4 == 0)
constexpr int FLAT_UNIT = 4096;        // elements
constexpr int PLANE_UNIT = 512;        // plane words = 4096 elements

struct OptimChunk {
    qt_optim_tensor t[QT_OPTIM_CHUNK];
    int32_t ustart[QT_OPTIM_CHUNK + 1];   // units of tensor i: [ustart[i], ustart[i + 1])
    int32_t idx[QT_OPTIM_CHUNK];          // table index of slot i, relative to the table index of slot 0
    int32_t n;
};
static_assert(sizeof(OptimChunk) == 3336, "by-value chunk: see the file header before growing it");

// Where the learning rate of an SGD launch comes from: the argument block, or one float of device memory.
struct LrValue {
    float lr;
    __device__ __forceinline__ float get() const { return lr; }
    LrValue at_base(int64_t) const { return *this; }
};
struct LrDevice {
    const float* lr;
    __device__ __forceinline__ float get() const { return *lr; }
    LrDevice at_base(int64_t) const { return *this; }
};

// torch.optim.SGD (dampening 0): g += wd p ; buf = first ? g : mu buf + g ; g = nesterov ? g + mu buf : buf ; p -= lr g
template <int NS_, class Lr>
struct SgdRule {
    static constexpr int NS = NS_;        // state tensors: 0 (no momentum) or 1
    struct Step { float lr; };            // what a workgroup reads once per tensor
    Lr src;
    float mu, wd;
    int nesterov;
    __device__ __forceinline__ Step step(const qt_optim_tensor&, int) const { return Step{src.get()}; }
    SgdRule at_base(int64_t b) const { return SgdRule{src.at_base(b), mu, wd, nesterov}; }
    __device__ __forceinline__ void operator()(float& p, float g, float& s0, float&, const qt_optim_tensor& t, const Step& st) const {
        if (wd != 0.0f) g = g + wd * p;
        if (NS == 1) {
            const float b = (t.flags & FLAG_FIRST) ? g : s0 * mu + g;
            s0 = b;
            g = nesterov ? g + mu * b : b;
        }
        p = p - st.lr * g;
    }
};

// Where Adam's bias corrections come from: the descriptor (t.c0, t.c1), or coef[table index][2] in device memory.
struct CoefTable {
    __device__ __forceinline__ void get(const qt_optim_tensor& t, int, float& c0, float& c1) const { c0 = t.c0, c1 = t.c1; }
    CoefTable at_base(int64_t) const { return *this; }
};
struct CoefDevice {
    const float* coef;                    // rebased to the table index of the chunk's first slot
    __device__ __forceinline__ void get(const qt_optim_tensor&, int idx, float& c0, float& c1) const {
        c0 = coef[2 * (int64_t)idx], c1 = coef[2 * (int64_t)idx + 1];
    }
    CoefDevice at_base(int64_t b) const { return CoefDevice{coef + 2 * b}; }
};

// torch.optim.Adam (L2 weight decay, no amsgrad).  c0 = lr / (1 - beta1^step), c1 = sqrt(1 - beta2^step): computed by
// the host in double precision from the tensor's own step count.
template <class Coef>
struct AdamRule {
    static constexpr int NS = 2;
    struct Step { float c0, c1; };
    Coef src;
    float b1, omb1, b2, omb2, eps, wd;
    __device__ __forceinline__ Step step(const qt_optim_tensor& t, int idx) const {
        Step st;
        src.get(t, idx, st.c0, st.c1);
        return st;
    }
    AdamRule at_base(int64_t b) const { return AdamRule{src.at_base(b), b1, omb1, b2, omb2, eps, wd}; }
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v, const qt_optim_tensor&, const Step& st) const {
        if (wd != 0.0f) g = g + wd * p;
        m = b1 * m + omb1 * g;
        v = b2 * v + omb2 * (g * g);
        const float denom = sqrtf(v) / st.c1 + eps;
        p = p - st.c0 * (m / denom);
    }
};

// torch.clamp: NaN stays NaN; lo = -inf / hi = +inf leave the value alone
__device__ __forceinline__ float clamp_store(float p, float lo, float hi) { return p < lo ? lo : (p > hi ? hi : p); }

__device__ __forceinline__ float& at(float4& v, int i) { return reinterpret_cast<float*>(&v)[i]; }

template <class Rule>
__device__ __forceinline__ void update4(const Rule& r, const typename Rule::Step& st, const qt_optim_tensor& t, float4& p,
                                        const float4& g, float4& s0, float4& s1) {
    r(p.x, g.x, s0.x, s1.x, t, st);
    r(p.y, g.y, s0.y, s1.y, t, st);
    r(p.z, g.z, s0.z, s1.z, t, st);
    r(p.w, g.w, s0.w, s1.w, t, st);
    p.x = clamp_store(p.x, t.lo, t.hi);
    p.y = clamp_store(p.y, t.lo, t.hi);
    p.z = clamp_store(p.z, t.lo, t.hi);
    p.w = clamp_store(p.w, t.lo, t.hi);
}

template <class Rule>
__device__ __forceinline__ float update1(const Rule& r, const typename Rule::Step& st, const qt_optim_tensor& t, int64_t i) {
    float p = t.p[i], s0 = 0.0f, s1 = 0.0f;
    if (Rule::NS >= 1) s0 = t.s0[i];
    if (Rule::NS >= 2) s1 = t.s1[i];
    r(p, t.g[i], s0, s1, t, st);
    p = clamp_store(p, t.lo, t.hi);
    t.p[i] = p;
    if (Rule::NS >= 1) t.s0[i] = s0;
    if (Rule::NS >= 2) t.s1[i] = s1;
    return p;
}

template <class Rule>
__device__ __forceinline__ void load4(const qt_optim_tensor& t, int64_t i4, float4& p, float4& g, float4& s0, float4& s1) {
    p = reinterpret_cast<const float4*>(t.p)[i4];
    g = reinterpret_cast<const float4*>(t.g)[i4];
    if (Rule::NS >= 1) s0 = reinterpret_cast<const float4*>(t.s0)[i4];
    if (Rule::NS >= 2) s1 = reinterpret_cast<const float4*>(t.s1)[i4];
}

template <class Rule>
__device__ __forceinline__ void store4(const qt_optim_tensor& t, int64_t i4, const float4& p, const float4& s0, const float4& s1) {
    reinterpret_cast<float4*>(t.p)[i4] = p;
    if (Rule::NS >= 1) reinterpret_cast<float4*>(t.s0)[i4] = s0;
    if (Rule::NS >= 2) reinterpret_cast<float4*>(t.s1)[i4] = s1;
}

// unit b of a flat tensor: elements [4096 b, min(numel, 4096 (b + 1)))
template <class Rule>
__device__ __forceinline__ void flat_unit(const Rule& r, const typename Rule::Step& st, const qt_optim_tensor& t, int64_t b) {
    const int tid = threadIdx.x;
    const int64_t base = b * FLAT_UNIT;
    if (!(t.flags & FLAG_VEC)) {
#pragma unroll 4
        for (int j = 0; j < FLAT_UNIT / 256; ++j) {
            const int64_t i = base + j * 256 + tid;
            if (i < t.numel) update1(r, st, t, i);
        }
        return;
    }
    const int64_t i0 = b * (FLAT_UNIT / 4) + tid;
    if (base + FLAT_UNIT <= t.numel) {        // full unit: every load of the lane issued before the first use
        float4 p[4], g[4], s0[4], s1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) load4<Rule>(t, i0 + 256 * j, p[j], g[j], s0[j], s1[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            update4(r, st, t, p[j], g[j], s0[j], s1[j]);
            store4<Rule>(t, i0 + 256 * j, p[j], s0[j], s1[j]);
        }
        return;
    }
    const int64_t n4 = t.numel >> 2;          // the tensor's last unit
    for (int j = 0; j < 4; ++j) {
        const int64_t i4 = i0 + 256 * j;
        if (i4 < n4) {
            float4 p, g, s0, s1;
            load4<Rule>(t, i4, p, g, s0, s1);
            update4(r, st, t, p, g, s0, s1);
            store4<Rule>(t, i4, p, s0, s1);
        }
    }
    const int64_t e = n4 * 4 + tid;           // numel % 4 tail elements (they lie in this unit)
    if (e < t.numel) update1(r, st, t, e);
}

__device__ __forceinline__ uint32_t nib_code(int kind, float x) { return kind == 2 ? NibTernary::nib(x) : NibSign::nib(x); }

// unit b of a plane tensor: plane words [512 b, min(rows ld, 512 (b + 1))) in (row, word) order
template <class Rule>
__device__ __forceinline__ void plane_unit(const Rule& r, const typename Rule::Step& st, const qt_optim_tensor& t, int64_t b) {
    const int64_t total = t.rows * t.ld;
    const bool vec = t.flags & FLAG_VEC;
#pragma unroll
    for (int j = 0; j < PLANE_UNIT / 256; ++j) {
        const int64_t wi = b * PLANE_UNIT + j * 256 + threadIdx.x;
        if (wi >= total) continue;
        const int64_t row = wi / t.ld, col = wi - row * t.ld;
        const int64_t k0 = col * 8;
        uint32_t word = 0;
        if (k0 < t.K) {
            const int64_t e0 = row * t.K + k0;
            const int nk = (int)(t.K - k0 < 8 ? t.K - k0 : 8);
            if (vec) {                          // K % 4 == 0: nk is 4 or 8
                const int64_t i4 = e0 >> 2;
                float4 p0, g0, a0, c0, p1, g1, a1, c1;
                load4<Rule>(t, i4, p0, g0, a0, c0);
                if (nk == 8) load4<Rule>(t, i4 + 1, p1, g1, a1, c1);
                update4(r, st, t, p0, g0, a0, c0);
                store4<Rule>(t, i4, p0, a0, c0);
#pragma unroll
                for (int i = 0; i < 4; ++i) word |= nib_code(t.kind, at(p0, i)) << (4 * i);
                if (nk == 8) {
                    update4(r, st, t, p1, g1, a1, c1);
                    store4<Rule>(t, i4 + 1, p1, a1, c1);
#pragma unroll
                    for (int i = 0; i < 4; ++i) word |= nib_code(t.kind, at(p1, i)) << (16 + 4 * i);
                }
            } else {
                for (int i = 0; i < nk; ++i) word |= nib_code(t.kind, update1(r, st, t, e0 + i)) << (4 * i);
            }
        }
        t.words[wi] = word;
    }
}

template <class Rule>
__device__ __forceinline__ void optim_step_body(const OptimChunk& c, const Rule& r) {
    const int total = c.ustart[c.n];
    int ti = 0, have = -1;
    typename Rule::Step st{};
    for (int u = blockIdx.x; u < total; u += gridDim.x) {
        while (c.ustart[ti + 1] <= u) ++ti;          // u < total = ustart[n]: stops at ti < n
        const qt_optim_tensor& t = c.t[ti];
        if (ti != have) {                            // the per-step scalars of this tensor: once per (workgroup, tensor)
            st = r.step(t, c.idx[ti]);
            have = ti;
        }
        const int64_t b = u - c.ustart[ti];
        if (t.kind != 0) plane_unit(r, st, t, b);
        else flat_unit(r, st, t, b);
    }
}

template <class Rule>
__global__ __launch_bounds__(256) void optim_step_kernel(const OptimChunk c, const Rule r) {
    optim_step_body(c, r);
}

// The guarded form (`_dev_guard` entries): one wave-uniform read of *skip before any tensor is touched; non-zero = the
// whole workgroup leaves, so p, the state and the plane keep their bits.  With *skip == 0 it is the body above.
template <class Rule>
__global__ __launch_bounds__(256) void optim_step_guard_kernel(const OptimChunk c, const Rule r, const int32_t* skip) {
    if (*skip != 0) return;
    optim_step_body(c, r);
}

template <class Rule>
int check_tensor(const qt_optim_tensor& t) {
    if (t.numel < 0) return QT_ERR_INVALID_ARG;
    if (t.kind < 0 || t.kind > 2) return QT_ERR_INVALID_ARG;
    if (t.numel > 0 && (!t.p || !t.g)) return QT_ERR_INVALID_ARG;
    if (t.numel > 0 && ((Rule::NS >= 1 && !t.s0) || (Rule::NS >= 2 && !t.s1))) return QT_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g)) & 3u) return QT_ERR_ALIGNMENT;
    if (Rule::NS >= 1 && (reinterpret_cast<uintptr_t>(t.s0) & 3u)) return QT_ERR_ALIGNMENT;
    if (Rule::NS >= 2 && (reinterpret_cast<uintptr_t>(t.s1) & 3u)) return QT_ERR_ALIGNMENT;
    if (t.kind != 0) {
        if (t.rows < 0 || t.K < 0 || t.ld < 0) return QT_ERR_INVALID_ARG;
        if (t.rows > 0 && t.K > (int64_t)INT64_MAX / t.rows) return QT_ERR_INVALID_ARG;
        if (t.rows * t.K != t.numel) return QT_ERR_INVALID_ARG;
        if (t.rows > 0 && !t.words) return QT_ERR_INVALID_ARG;
        if (t.ld < (t.K + 7) / 8 || (t.ld & 3) != 0 || !qt_aligned16(t.words)) return QT_ERR_ALIGNMENT;
        if (t.rows > 0 && t.ld > (int64_t)INT64_MAX / t.rows) return QT_ERR_INVALID_ARG;
    }
    return QT_OK;
}

int64_t tensor_units(const qt_optim_tensor& t) {
    if (t.kind != 0) return (t.rows * t.ld + PLANE_UNIT - 1) / PLANE_UNIT;
    return (t.numel + FLAT_UNIT - 1) / FLAT_UNIT;
}

// The guard of a launch sequence is a TYPE, so that only the entries that take one instantiate the guarded kernel.
struct NoGuard {};
struct DevGuard { const int32_t* skip; };

template <class Rule>
void enqueue_chunk(const OptimChunk& c, const Rule& r, NoGuard, int grid, hipStream_t s) {
    hipLaunchKernelGGL(optim_step_kernel<Rule>, dim3(grid), dim3(256), 0, s, c, r);
}
template <class Rule>
void enqueue_chunk(const OptimChunk& c, const Rule& r, DevGuard g, int grid, hipStream_t s) {
    hipLaunchKernelGGL(optim_step_guard_kernel<Rule>, dim3(grid), dim3(256), 0, s, c, r, g.skip);
}

template <class Rule, class Guard>
int launch_chunk(const OptimChunk& c, const Rule& r, Guard g, qt_stream_t stream) {
    const int total = c.ustart[c.n];
    if (c.n == 0 || total == 0) return QT_OK;
    enqueue_chunk(c, r, g, qt_stream_grid(total), (hipStream_t)stream);
    return qt_check_launch();
}

template <class Rule, class Guard = NoGuard>
int optim_step(const qt_optim_tensor* tab, int64_t n, const Rule& r, qt_stream_t stream, Guard skip = Guard{}) {
    if (n < 0 || (n > 0 && !tab)) return QT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; ++i) {              // the whole table is checked before anything is enqueued
        const int rc = check_tensor<Rule>(tab[i]);
        if (rc != QT_OK) return rc;
        if (tensor_units(tab[i]) > INT32_MAX) return QT_ERR_UNSUPPORTED;
    }
    OptimChunk c{};
    int64_t base = 0;                              // table index of the chunk's first slot
    for (int64_t i = 0; i < n; ++i) {
        const int64_t units = tensor_units(tab[i]);
        if (units == 0) continue;                  // empty tensor
        if (c.n == QT_OPTIM_CHUNK || (int64_t)c.ustart[c.n] + units > INT32_MAX || (c.n > 0 && i - base > INT32_MAX)) {
            const int rc = launch_chunk(c, r.at_base(base), skip, stream);
            if (rc != QT_OK) return rc;
            c.n = 0;
        }
        if (c.n == 0) base = i;
        c.idx[c.n] = (int32_t)(i - base);
        qt_optim_tensor& t = c.t[c.n];
        t = tab[i];
        bool vec = qt_aligned16(t.p) && qt_aligned16(t.g) && (Rule::NS < 1 || qt_aligned16(t.s0)) &&
                   (Rule::NS < 2 || qt_aligned16(t.s1));
        if (t.kind != 0) vec = vec && (t.K % 4 == 0);
        if (Rule::NS < 1) t.s0 = nullptr;
        if (Rule::NS < 2) t.s1 = nullptr;
        t.flags = (t.flags & FLAG_FIRST) | (vec ? FLAG_VEC : 0);
        c.ustart[c.n + 1] = c.ustart[c.n] + (int32_t)units;
        ++c.n;
    }
    return launch_chunk(c, r.at_base(base), skip, stream);
}

#define QT_SCALARS_CHUNK 960               // 3840 bytes of values + pointer + count: below the 4096-byte argument limit
struct ScalarChunk {
    float v[QT_SCALARS_CHUNK];
};

__global__ __launch_bounds__(256) void optim_scalars_kernel(float* dst, const ScalarChunk c, int n) {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = c.v[i];
}

// the device scalars of a `_dev` entry: looked at only when there is a tensor to update
int check_scalars(const float* s, int64_t n) {
    if (n < 0) return QT_ERR_INVALID_ARG;          // the status optim_step() gives: every table rejection comes first
    if (n > 0 && !s) return QT_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(s) & 3u) return QT_ERR_ALIGNMENT;
    return QT_OK;
}

// the skip word of a `_dev_guard` entry: validated like the device scalars, after them
int check_skip(const int32_t* skip) {
    if (!skip) return QT_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(skip) & 3u) return QT_ERR_ALIGNMENT;
    return QT_OK;
}

#define QT_FLAGS_CHUNK 448                 // 3584 bytes of pointers + guard + count: below the 4096-byte argument limit
struct FlagChunk {
    const int32_t* f[QT_FLAGS_CHUNK];
};

// *guard |= any(*f[i] != 0): every lane ORs its flags, the workgroup votes, lane 0 stores (a plain vector store, and
// only when there is something to raise: a guard that is already set is never cleared).
__global__ __launch_bounds__(256) void flags_or_kernel(const FlagChunk c, int n, int32_t* guard) {
    int any = 0;
    for (int i = threadIdx.x; i < n; i += 256) any |= (*c.f[i] != 0);
    if (__syncthreads_or(any) && threadIdx.x == 0) *guard = 1;
}

}  // namespace

extern "C" {

int qt_optim_chunk_capacity(void) { return QT_OPTIM_CHUNK; }

int qt_optim_scalars_f32(float* dst, const float* values, int64_t n, qt_stream_t stream) {
    if (n < 0 || (n > 0 && (!dst || !values))) return QT_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(dst) & 3u) return QT_ERR_ALIGNMENT;
    ScalarChunk c{};                           // the whole struct travels as the argument block
    for (int64_t done = 0; done < n; done += QT_SCALARS_CHUNK) {
        const int m = (int)(n - done < QT_SCALARS_CHUNK ? n - done : QT_SCALARS_CHUNK);
        for (int i = 0; i < m; ++i) c.v[i] = values[done + i];
        hipLaunchKernelGGL(optim_scalars_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, dst + done, c, m);
        const int rc = qt_check_launch();
        if (rc != QT_OK) return rc;
    }
    return QT_OK;
}

int qt_optim_sgd_f32(const qt_optim_tensor* table, int64_t n, float lr, float momentum, float weight_decay, int nesterov,
                     qt_stream_t stream) {
    if (nesterov && momentum == 0.0f) return QT_ERR_INVALID_ARG;
    if (momentum != 0.0f) return optim_step(table, n, SgdRule<1, LrValue>{{lr}, momentum, weight_decay, nesterov ? 1 : 0}, stream);
    return optim_step(table, n, SgdRule<0, LrValue>{{lr}, 0.0f, weight_decay, 0}, stream);
}

int qt_optim_sgd_dev_f32(const qt_optim_tensor* table, int64_t n, const float* lr, float momentum, float weight_decay,
                         int nesterov, qt_stream_t stream) {
    if (nesterov && momentum == 0.0f) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    const int rc = check_scalars(lr, n);
    if (rc != QT_OK) return rc;
    if (momentum != 0.0f) return optim_step(table, n, SgdRule<1, LrDevice>{{lr}, momentum, weight_decay, nesterov ? 1 : 0}, stream);
    return optim_step(table, n, SgdRule<0, LrDevice>{{lr}, 0.0f, weight_decay, 0}, stream);
}

int qt_optim_adam_f32(const qt_optim_tensor* table, int64_t n, float beta1, float one_minus_beta1, float beta2,
                      float one_minus_beta2, float eps, float weight_decay, qt_stream_t stream) {
    return optim_step(table, n, AdamRule<CoefTable>{{}, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay}, stream);
}

int qt_optim_adam_dev_f32(const qt_optim_tensor* table, int64_t n, const float* coef, float beta1, float one_minus_beta1,
                          float beta2, float one_minus_beta2, float eps, float weight_decay, qt_stream_t stream) {
    if (n == 0) return QT_OK;
    const int rc = check_scalars(coef, n);
    if (rc != QT_OK) return rc;
    return optim_step(table, n, AdamRule<CoefDevice>{{coef}, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay},
                      stream);
}

int qt_optim_sgd_dev_guard_f32(const qt_optim_tensor* table, int64_t n, const float* lr, const int32_t* skip, float momentum,
                               float weight_decay, int nesterov, qt_stream_t stream) {
    if (nesterov && momentum == 0.0f) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    int rc = check_scalars(lr, n);
    if (rc == QT_OK) rc = check_skip(skip);
    if (rc != QT_OK) return rc;
    if (momentum != 0.0f)
        return optim_step(table, n, SgdRule<1, LrDevice>{{lr}, momentum, weight_decay, nesterov ? 1 : 0}, stream, DevGuard{skip});
    return optim_step(table, n, SgdRule<0, LrDevice>{{lr}, 0.0f, weight_decay, 0}, stream, DevGuard{skip});
}

int qt_optim_adam_dev_guard_f32(const qt_optim_tensor* table, int64_t n, const float* coef, const int32_t* skip, float beta1,
                                float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float weight_decay,
                                qt_stream_t stream) {
    if (n == 0) return QT_OK;
    int rc = check_scalars(coef, n);
    if (rc == QT_OK) rc = check_skip(skip);
    if (rc != QT_OK) return rc;
    return optim_step(table, n, AdamRule<CoefDevice>{{coef}, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay},
                      stream, DevGuard{skip});
}

int qt_flags_chunk_capacity(void) { return QT_FLAGS_CHUNK; }

int qt_flags_or_i32(const int32_t* const* flags, int64_t n, int32_t* guard, qt_stream_t stream) {
    if (n < 0 || (n > 0 && (!flags || !guard))) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    if (reinterpret_cast<uintptr_t>(guard) & 3u) return QT_ERR_ALIGNMENT;
    for (int64_t i = 0; i < n; ++i) {              // every pointer is checked before anything is enqueued
        if (!flags[i]) return QT_ERR_INVALID_ARG;
        if (reinterpret_cast<uintptr_t>(flags[i]) & 3u) return QT_ERR_ALIGNMENT;
    }
    FlagChunk c{};                                 // the whole struct travels as the argument block
    for (int64_t done = 0; done < n; done += QT_FLAGS_CHUNK) {
        const int m = (int)(n - done < QT_FLAGS_CHUNK ? n - done : QT_FLAGS_CHUNK);
        for (int i = 0; i < m; ++i) c.f[i] = flags[done + i];
        hipLaunchKernelGGL(flags_or_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, c, m, guard);
        const int rc = qt_check_launch();
        if (rc != QT_OK) return rc;
    }
    return QT_OK;
}

}  // extern "C"
