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
//   * one entry per rule (qt_optim_sgd_f32 / qt_optim_adam_f32) and ONE kernel template.  The three optional inputs of an entry
//     (its `form`: QT_OPTIM_SCALARS_DEV, QT_OPTIM_GSCALE, QT_OPTIM_SKIP) choose the rule's SOURCE types and the skip pointer the
//     kernel gets; the arithmetic is the one template in every form, so equal values give equal bits.
//   * per-step scalars (learning rate; Adam's bias corrections c0, c1) come from the argument block / the descriptor, or, with
//     QT_OPTIM_SCALARS_DEV, from device memory, so that a launch captured in a hipGraph sees the values of the step it is
//     replayed for.  A workgroup reads them once per tensor it walks (a wave-uniform load where the tensor index advances),
//     never per element.  Adam's `coef` is indexed by the TABLE index of a tensor: a chunk carries, per slot, the table index
//     relative to its first slot (empty tensors are dropped, later chunks start anywhere) and the launch gets `coef` rebased to
//     that.  qt_optim_scalars_f32 is how the host gets them there between replays: a launch whose ARGUMENT BLOCK carries the
//     values (up to 960 floats per launch), stream-ordered like any kernel, with no staging buffer for a later call to overwrite.
//   * QT_OPTIM_GSCALE: the gradient is multiplied by one device float first: g = g * (*gscale), a separate fp32 multiplication
//     in front of the weight-decay term, where torch.nn.utils.clip_grad_norm_'s in-place mul_ puts it — but the gradient in
//     memory is not rewritten.  *gscale is read with the other per-step scalars, once per (workgroup, tensor).  Without the
//     bit the scale's source type is NoScale, which compiles to nothing.
//   * QT_OPTIM_SKIP: every workgroup reads *skip once, before it touches a tensor, and leaves when it is non-zero — how a
//     captured training step keeps parameters, state and planes untouched when one of its trusted route verdicts turned out
//     wrong (utils.GraphedTrainStep(recover=True)).  Without the bit the kernel gets a null pointer and does not read it.
//     qt_flags_or_i32 folds the step's verdict flags into that word: the flag POINTERS travel by value, 448 per launch.
//   * the global gradient norm that scale comes from (qt_optim_grad_sumsq_f32 / qt_optim_grad_norm_finalize_f32, below the update):
//     one fp32 partial per 4096-element unit in a caller's workspace, then one workgroup that adds the partials in fp64.  Fixed
//     order everywhere, no atomics, no counter, no buffer that has to be zero before the launch.
//   * kernel-argument size: OptimChunk = 32 x 96 (descriptors) + 33 x 4 (unit prefix) + 32 x 4 (table indices) + 4 (n)
//     + 4 (padding) = 3336 bytes; the largest rule (clipped Adam from device memory: coef and gscale pointers, six floats)
//     adds 40 and the skip pointer 8: 3384 of HIP's 4096 bytes.
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

// What the gradient is multiplied by before the recurrence: nothing, or one float of device memory (the clip coefficient).
// The rules derive from it, so NoScale takes no room in the argument block.
struct NoScale {
    static constexpr bool ON = false;
    __device__ __forceinline__ float get() const { return 1.0f; }
};
struct DevScale {
    static constexpr bool ON = true;
    const float* gscale;
    __device__ __forceinline__ float get() const { return *gscale; }
};

// torch.optim.SGD (dampening 0): g = g gscale ; g += wd p ; buf = first ? g : mu buf + g ; g = nesterov ? g + mu buf : buf ; p -= lr g
template <int NS_, class Lr, class Gs = NoScale>
struct SgdRule : Gs {
    static constexpr int NS = NS_;        // state tensors: 0 (no momentum) or 1
    struct Step { float lr, gs; };        // what a workgroup reads once per tensor
    Lr src;
    float mu, wd;
    int nesterov;
    __device__ __forceinline__ Step step(const qt_optim_tensor&, int) const { return Step{src.get(), Gs::get()}; }
    SgdRule at_base(int64_t b) const { return SgdRule{static_cast<const Gs&>(*this), src.at_base(b), mu, wd, nesterov}; }
    __device__ __forceinline__ void operator()(float& p, float g, float& s0, float&, const qt_optim_tensor& t, const Step& st) const {
        if (Gs::ON) g = g * st.gs;
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
template <class Coef, class Gs = NoScale>
struct AdamRule : Gs {
    static constexpr int NS = 2;
    struct Step { float c0, c1, gs; };
    Coef src;
    float b1, omb1, b2, omb2, eps, wd;
    __device__ __forceinline__ Step step(const qt_optim_tensor& t, int idx) const {
        Step st;
        src.get(t, idx, st.c0, st.c1);
        st.gs = Gs::get();
        return st;
    }
    AdamRule at_base(int64_t b) const {
        return AdamRule{static_cast<const Gs&>(*this), src.at_base(b), b1, omb1, b2, omb2, eps, wd};
    }
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v, const qt_optim_tensor&, const Step& st) const {
        if (Gs::ON) g = g * st.gs;
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

// skip: null, or one device word.  One wave-uniform read before any tensor is touched; non-zero = the whole workgroup leaves,
// so p, the state and the plane keep their bits.
template <class Rule>
__global__ __launch_bounds__(256) void optim_step_kernel(const OptimChunk c, const Rule r, const int32_t* skip) {
    if (skip && *skip != 0) return;
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

template <class Rule>
int launch_chunk(const OptimChunk& c, const Rule& r, const int32_t* skip, qt_stream_t stream) {
    const int total = c.ustart[c.n];
    if (c.n == 0 || total == 0) return QT_OK;
    hipLaunchKernelGGL(optim_step_kernel<Rule>, dim3(qt_stream_grid(total)), dim3(256), 0, (hipStream_t)stream, c, r, skip);
    return qt_check_launch();
}

template <class Rule>
int optim_step(const qt_optim_tensor* tab, int64_t n, const Rule& r, const int32_t* skip, qt_stream_t stream) {
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

// One optional device word of an update entry (per-step scalars, gscale, skip): given exactly when its form bit says so.
int check_word(const void* p, bool flagged) {
    if (flagged != (p != nullptr)) return QT_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(p) & 3u) return QT_ERR_ALIGNMENT;
    return QT_OK;
}

// What both update entries check in front of the table, in the order of include/qt_hip.h.  go = false: n == 0, nothing to do.
int check_form(int form, int64_t n, const float* scalars, const float* gscale, const int32_t* skip, bool& go) {
    go = false;
    if (form & ~QT_OPTIM_FORM_MASK) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    if (n < 0) return QT_ERR_INVALID_ARG;
    int rc = check_word(scalars, form & QT_OPTIM_SCALARS_DEV);
    if (rc == QT_OK) rc = check_word(gscale, form & QT_OPTIM_GSCALE);
    if (rc == QT_OK) rc = check_word(skip, form & QT_OPTIM_SKIP);
    go = rc == QT_OK;
    return rc;
}

// The rule's two source types, chosen from the form: f(scalar source, gradient scale).
template <class Value, class Device, class F>
int with_sources(int form, const Value& value, const Device& device, const float* gscale, F f) {
    const bool dev = form & QT_OPTIM_SCALARS_DEV;
    if (form & QT_OPTIM_GSCALE) return dev ? f(device, DevScale{gscale}) : f(value, DevScale{gscale});
    return dev ? f(device, NoScale{}) : f(value, NoScale{});
}

#define QT_SCALARS_CHUNK 960               // 3840 bytes of values + pointer + count: below the 4096-byte argument limit
struct ScalarChunk {
    float v[QT_SCALARS_CHUNK];
};

__global__ __launch_bounds__(256) void optim_scalars_kernel(float* dst, const ScalarChunk c, int n) {
    for (int i = threadIdx.x; i < n; i += 256) dst[i] = c.v[i];
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

// ---- global gradient norm: sum of squares per unit, then one workgroup that finishes ----

// What the sum-of-squares pass needs of a chunk of the table: gradient pointers and sizes, the unit prefix, one bit per slot for
// the 16-byte walk.  656 bytes of argument block.
struct NormChunk {
    const float* g[QT_OPTIM_CHUNK];
    int64_t numel[QT_OPTIM_CHUNK];
    int32_t ustart[QT_OPTIM_CHUNK + 1];   // units of slot i: [ustart[i], ustart[i + 1])
    uint32_t vec;                         // bit i: g[i] is 16-byte aligned
    int32_t n;
};
static_assert(sizeof(NormChunk) == 656, "by-value chunk of the sum-of-squares pass");

// Sum over the 64 lanes of a wave, a fixed tree: four DPP steps inside each row of 16, then the four row sums in lane order.
// Every step exchanges symmetrically, so the lanes of a row agree bit for bit.
__device__ __forceinline__ float wave_sum_dpp_f32(float v) {
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true));   // row_mirror
    const int i = __float_as_int(v);
    return ((__int_as_float(__builtin_amdgcn_readlane(i, 0)) + __int_as_float(__builtin_amdgcn_readlane(i, 16))) +
            __int_as_float(__builtin_amdgcn_readlane(i, 32))) + __int_as_float(__builtin_amdgcn_readlane(i, 48));
}

__device__ __forceinline__ float sumsq4(float acc, const float4& g) {
    acc = acc + g.x * g.x;
    acc = acc + g.y * g.y;
    acc = acc + g.z * g.z;
    return acc + g.w * g.w;
}

// this lane's share of unit b of a gradient: elements [4096 b, min(numel, 4096 (b + 1))), walked as flat_unit() walks them
__device__ __forceinline__ float lane_sumsq(const float* g, int64_t numel, int64_t b, bool vec) {
    const int tid = threadIdx.x;
    const int64_t base = b * FLAT_UNIT;
    float acc = 0.0f;
    if (!vec) {
#pragma unroll 4
        for (int j = 0; j < FLAT_UNIT / 256; ++j) {
            const int64_t i = base + j * 256 + tid;
            if (i < numel) {
                const float x = g[i];
                acc = acc + x * x;
            }
        }
        return acc;
    }
    const int64_t i0 = b * (FLAT_UNIT / 4) + tid;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    if (base + FLAT_UNIT <= numel) {          // full unit: four independent loads in flight
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = g4[i0 + 256 * j];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = sumsq4(acc, v[j]);
        return acc;
    }
    const int64_t n4 = numel >> 2;            // the gradient's last unit
    for (int j = 0; j < 4; ++j) {
        const int64_t i4 = i0 + 256 * j;
        if (i4 < n4) acc = sumsq4(acc, g4[i4]);
    }
    const int64_t e = n4 * 4 + tid;           // numel % 4 tail elements (they lie in this unit)
    if (e < numel) {
        const float x = g[e];
        acc = acc + x * x;
    }
    return acc;
}

// work[u] = sum of squares of unit u of the chunk: per lane, then the wave tree, then the four waves through LDS in wave order.
// Every unit's word is written by exactly one workgroup with a plain store: nothing has to be zero beforehand.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const NormChunk c, float* __restrict__ work) {
    __shared__ float part[4];
    const int total = c.ustart[c.n];
    int ti = 0;
    for (int u = blockIdx.x; u < total; u += gridDim.x) {
        while (c.ustart[ti + 1] <= u) ++ti;          // u < total = ustart[n]: stops at ti < n
        float acc = lane_sumsq(c.g[ti], c.numel[ti], u - c.ustart[ti], (c.vec >> ti) & 1u);
        acc = wave_sum_dpp_f32(acc);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) work[u] = ((part[0] + part[1]) + part[2]) + part[3];
        __syncthreads();                             // part[] is reused by the next unit
    }
}

// One workgroup: total = sum of work[0, m) in fp64 (lane l adds the words l, l + 256, ... in ascending order, then a fixed
// tree over the lanes), out[0] = norm = (float)sqrt(total), out[1] = coef = min(1, max_norm / (norm + 1e-6f)) in fp32, the
// expression of torch.nn.utils.clip_grad_norm_.  A NaN quotient stays NaN (torch.clamp), an infinite norm gives 0.
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float* __restrict__ work, int64_t m, float max_norm,
                                                                 const float* max_norm_dev, float* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += 256) s += (double)work[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(sh[0]);
        const float mx = max_norm_dev ? *max_norm_dev : max_norm;
        const float q = mx / (norm + 1e-6f);
        out[0] = norm;
        out[1] = q > 1.0f ? 1.0f : q;
    }
}

int check_grad(const qt_optim_tensor& t) {
    if (t.numel < 0) return QT_ERR_INVALID_ARG;
    if (t.numel > 0 && !t.g) return QT_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(t.g) & 3u) return QT_ERR_ALIGNMENT;
    if ((t.numel + FLAT_UNIT - 1) / FLAT_UNIT > INT32_MAX) return QT_ERR_UNSUPPORTED;
    return QT_OK;
}

// units of a gradient in the sum-of-squares pass: flat memory, whatever the parameter's plane
int64_t grad_units(const qt_optim_tensor& t) { return (t.numel + FLAT_UNIT - 1) / FLAT_UNIT; }

// The chunking of the sum-of-squares pass, apart from the launch: emit(chunk, first unit of the chunk in the workspace) for
// every non-empty chunk, in table order.  Returns the number of units, or a negative status of emit.
template <class Emit>
int64_t grad_sumsq_chunks(const qt_optim_tensor* tab, int64_t n, Emit emit) {
    NormChunk c{};
    int64_t first = 0;                             // workspace index of the chunk's unit 0
    for (int64_t i = 0; i < n; ++i) {
        const int64_t units = grad_units(tab[i]);
        if (units == 0) continue;                  // empty tensor
        if (c.n == QT_OPTIM_CHUNK || (int64_t)c.ustart[c.n] + units > INT32_MAX) {
            const int rc = emit(c, first);
            if (rc != QT_OK) return rc;
            first += c.ustart[c.n];
            c = NormChunk{};
        }
        c.g[c.n] = tab[i].g;
        c.numel[c.n] = tab[i].numel;
        if (qt_aligned16(tab[i].g)) c.vec |= 1u << c.n;
        c.ustart[c.n + 1] = c.ustart[c.n] + (int32_t)units;
        ++c.n;
    }
    if (c.n > 0) {
        const int rc = emit(c, first);
        if (rc != QT_OK) return rc;
        first += c.ustart[c.n];
    }
    return first;
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

int qt_optim_sgd_f32(const qt_optim_tensor* table, int64_t n, int form, float lr, const float* lr_dev, const float* gscale,
                     const int32_t* skip, float momentum, float weight_decay, int nesterov, qt_stream_t stream) {
    if (nesterov && momentum == 0.0f) return QT_ERR_INVALID_ARG;
    bool go;
    const int rc = check_form(form, n, lr_dev, gscale, skip, go);
    if (!go) return rc;
    return with_sources(form, LrValue{lr}, LrDevice{lr_dev}, gscale, [&](auto src, auto gs) {
        using Lr = decltype(src);
        using Gs = decltype(gs);
        if (momentum != 0.0f)
            return optim_step(table, n, SgdRule<1, Lr, Gs>{gs, src, momentum, weight_decay, nesterov ? 1 : 0}, skip, stream);
        return optim_step(table, n, SgdRule<0, Lr, Gs>{gs, src, 0.0f, weight_decay, 0}, skip, stream);
    });
}

int qt_optim_adam_f32(const qt_optim_tensor* table, int64_t n, int form, const float* coef, const float* gscale,
                      const int32_t* skip, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                      float weight_decay, qt_stream_t stream) {
    bool go;
    const int rc = check_form(form, n, coef, gscale, skip, go);
    if (!go) return rc;
    return with_sources(form, CoefTable{}, CoefDevice{coef}, gscale, [&](auto src, auto gs) {
        return optim_step(table, n, AdamRule<decltype(src), decltype(gs)>{gs, src, beta1, one_minus_beta1, beta2, one_minus_beta2,
                                                                         eps, weight_decay}, skip, stream);
    });
}

int64_t qt_optim_grad_norm_work_floats(const qt_optim_tensor* table, int64_t n) {
    if (n < 0 || (n > 0 && !table)) return QT_ERR_INVALID_ARG;
    int64_t units = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int rc = check_grad(table[i]);
        if (rc != QT_OK) return rc;
        units += grad_units(table[i]);
    }
    return units;
}

int qt_optim_grad_sumsq_f32(const qt_optim_tensor* table, int64_t n, float* work, qt_stream_t stream) {
    if (n < 0 || (n > 0 && (!table || !work))) return QT_ERR_INVALID_ARG;
    if (n == 0) return QT_OK;
    if (reinterpret_cast<uintptr_t>(work) & 3u) return QT_ERR_ALIGNMENT;
    for (int64_t i = 0; i < n; ++i) {              // the whole table is checked before anything is enqueued
        const int rc = check_grad(table[i]);
        if (rc != QT_OK) return rc;
    }
    const int64_t rc = grad_sumsq_chunks(table, n, [&](const NormChunk& c, int64_t first) {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(qt_stream_grid(c.ustart[c.n])), dim3(256), 0, (hipStream_t)stream, c, work + first);
        return qt_check_launch();
    });
    return rc < 0 ? (int)rc : QT_OK;
}

int qt_optim_grad_norm_finalize_f32(const float* work, int64_t m, float max_norm, const float* max_norm_dev, float* out,
                                    qt_stream_t stream) {
    if (m < 0 || (m > 0 && !work) || !out) return QT_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(work) | reinterpret_cast<uintptr_t>(max_norm_dev) | reinterpret_cast<uintptr_t>(out)) & 3u)
        return QT_ERR_ALIGNMENT;
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, work, m, max_norm, max_norm_dev, out);
    return qt_check_launch();
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
