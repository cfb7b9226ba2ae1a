// Stand-alone host check of the gradient-clipping entries of csrc/optim_step.hip: the chunking of the sum-of-squares pass, its
// workspace offsets, and the argument validation of the norm entries and of the two update entries in every form.  Nothing here launches a kernel or touches device
// memory (every pointer is a made-up address that is only compared and offset), so it runs without a GPU and is meant to be built
// with the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Ipytorch_quantize_impls_amd/csrc \
//         tools/optim_clip_host_check.hip -o /tmp/optim_clip_host_check && /tmp/optim_clip_host_check
//
// The translation unit is included, not linked: the chunk builder lives in its anonymous namespace.
#include "../pytorch_quantize_impls_amd/csrc/optim_step.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static float* fake(uintptr_t a) { return reinterpret_cast<float*>(a); }

static qt_optim_tensor tensor(int64_t numel, uintptr_t base) {
    qt_optim_tensor t{};
    t.p = fake(base);
    t.g = numel ? fake(base + 0x100000) : nullptr;
    t.s0 = fake(base + 0x200000);
    t.s1 = fake(base + 0x300000);
    t.numel = numel;
    t.lo = -INFINITY;
    t.hi = INFINITY;
    return t;
}

// walks a table through grad_sumsq_chunks and checks every chunk against the table: order, unit prefix, workspace offset, the
// alignment bits; returns the number of chunks
static int walk(const std::vector<qt_optim_tensor>& tab) {
    int chunks = 0;
    size_t next = 0;                // table index the next slot must come from
    int64_t units = 0;
    const int64_t got = grad_sumsq_chunks(tab.data(), (int64_t)tab.size(), [&](const NormChunk& c, int64_t first) {
        CHECK(c.n >= 1 && c.n <= QT_OPTIM_CHUNK);
        CHECK(first == units && c.ustart[0] == 0);
        for (int i = 0; i < c.n; ++i) {
            while (next < tab.size() && tab[next].numel == 0) ++next;          // empty tensors take no slot
            CHECK(next < tab.size());
            CHECK(c.g[i] == tab[next].g && c.numel[i] == tab[next].numel);
            CHECK(c.ustart[i + 1] - c.ustart[i] == (tab[next].numel + 4095) / 4096);
            CHECK((((c.vec >> i) & 1u) != 0) == ((reinterpret_cast<uintptr_t>(tab[next].g) & 15u) == 0));
            ++next;
        }
        for (int i = c.n; i < QT_OPTIM_CHUNK; ++i) CHECK(c.g[i] == nullptr && ((c.vec >> i) & 1u) == 0);
        units += c.ustart[c.n];
        ++chunks;
        return (int)QT_OK;
    });
    while (next < tab.size() && tab[next].numel == 0) ++next;
    CHECK(next == tab.size());
    CHECK(got == units);
    CHECK(qt_optim_grad_norm_work_floats(tab.data(), (int64_t)tab.size()) == units);
    return chunks;
}

int main() {
    // ---- chunking ----
    CHECK(walk({}) == 0);
    const int64_t sizes[] = {1, 3, 4095, 4096, 4097, 2 * 4096 + 5, 0, 100};
    for (int n : {1, 7, 31, 32, 33, 64, 65, 100}) {
        std::vector<qt_optim_tensor> tab;
        for (int i = 0; tab.size() < (size_t)n; ++i) {
            const int64_t numel = i == 20 ? 0 : sizes[i % 8];
            tab.push_back(tensor(numel, 0x10000000u + 0x1000000u * (uintptr_t)i + (i % 5 == 2 ? 4 : 0)));     // some 4-byte aligned only
        }
        int nonempty = 0;
        for (const auto& t : tab) nonempty += t.numel != 0;
        CHECK(walk(tab) == (nonempty + QT_OPTIM_CHUNK - 1) / QT_OPTIM_CHUNK);
    }
    {   // only empty tensors: no chunk, no unit
        std::vector<qt_optim_tensor> tab(40, tensor(0, 0x1000));
        CHECK(walk(tab) == 0);
    }
    {   // the unit prefix is int32: three tensors of 2^30 units each do not fit one chunk
        std::vector<qt_optim_tensor> tab(3, tensor((int64_t)4096 << 30, 0x40000000));
        CHECK(walk(tab) == 3);                                         // 2^30 + 2^30 > INT32_MAX: one tensor per chunk
        tab[1].numel = ((int64_t)4096 << 31);                                  // 2^31 units in one tensor
        CHECK(qt_optim_grad_norm_work_floats(tab.data(), 3) == QT_ERR_UNSUPPORTED);
        CHECK(qt_optim_grad_sumsq_f32(tab.data(), 3, fake(0x6000), nullptr) == QT_ERR_UNSUPPORTED);
    }
    {   // an emit that fails stops the walk with its status
        std::vector<qt_optim_tensor> tab(70, tensor(5000, 0x50000000));
        int calls = 0;
        CHECK(grad_sumsq_chunks(tab.data(), 70, [&](const NormChunk&, int64_t) { return ++calls == 2 ? (int)QT_ERR_LAUNCH : (int)QT_OK; }) ==
              QT_ERR_LAUNCH);
        CHECK(calls == 2);
    }

    // ---- validation: every status below is returned before anything is enqueued ----
    std::vector<qt_optim_tensor> tab(40, tensor(5000, 0x50000000));
    float* const dev = fake(0x6000);
    const int32_t* const skip = reinterpret_cast<const int32_t*>(0x7000);
    const int32_t* const skip2 = reinterpret_cast<const int32_t*>(0x7002);       // not 4-byte aligned
    const int DEV = QT_OPTIM_SCALARS_DEV, GS = QT_OPTIM_GSCALE, SK = QT_OPTIM_SKIP;
    CHECK(qt_optim_grad_norm_work_floats(nullptr, 0) == 0 && qt_optim_grad_norm_work_floats(nullptr, 1) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_grad_norm_work_floats(tab.data(), -1) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_grad_sumsq_f32(nullptr, 0, nullptr, nullptr) == QT_OK);
    CHECK(qt_optim_grad_sumsq_f32(tab.data(), 40, nullptr, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_grad_sumsq_f32(nullptr, 40, dev, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_grad_sumsq_f32(tab.data(), 40, fake(0x6002), nullptr) == QT_ERR_ALIGNMENT);
    tab[39].g = fake(0x50100002);                                              // the LAST entry is bad: still nothing is enqueued
    CHECK(qt_optim_grad_sumsq_f32(tab.data(), 40, dev, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, GS, 0.1f, nullptr, dev, nullptr, 0.9f, 0.0f, 0, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_adam_f32(tab.data(), 40, DEV | GS | SK, dev, dev, skip, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_ALIGNMENT);
    tab[39].g = nullptr;
    CHECK(qt_optim_grad_sumsq_f32(tab.data(), 40, dev, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, DEV | GS | SK, 0.1f, dev, dev, skip, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, 0, 0.1f, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(tab.data(), 40, SK, nullptr, nullptr, skip, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    tab[39] = tensor(5000, 0x50000000);
    // a flagged pointer that is null, then one that is not 4-byte aligned
    CHECK(qt_optim_sgd_f32(tab.data(), 40, GS, 0.1f, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, GS, 0.1f, nullptr, fake(0x6002), nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, DEV | GS, 0.1f, fake(0x6002), dev, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, GS | SK, 0.1f, nullptr, dev, skip2, 0.0f, 0.0f, 0, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, DEV, 0.1f, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, DEV | SK, 0.1f, dev, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, GS, 0.1f, nullptr, dev, nullptr, 0.0f, 0.0f, 1, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), -1, GS, 0.1f, nullptr, dev, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(nullptr, 0, GS, 0.1f, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_OK);
    CHECK(qt_optim_adam_f32(tab.data(), 40, GS, nullptr, nullptr, nullptr, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(tab.data(), 40, DEV | GS, fake(0x6002), dev, nullptr, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_adam_f32(nullptr, 0, GS, nullptr, nullptr, nullptr, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_OK);
    // a pointer whose bit is clear must be null, aligned or not: nothing becomes legal by being left over from another form
    CHECK(qt_optim_sgd_f32(tab.data(), 40, 0, 0.1f, dev, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, 0, 0.1f, nullptr, dev, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, 0, 0.1f, nullptr, nullptr, skip, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(tab.data(), 40, GS | SK, dev, dev, skip, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(tab.data(), 40, DEV | SK, dev, fake(0x6002), skip, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(tab.data(), 40, DEV | GS, dev, dev, skip2, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    // bits outside the mask: refused even where there is nothing to do
    CHECK(qt_optim_sgd_f32(nullptr, 0, 0x8, 0.1f, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(nullptr, 0, GS | 0x10, nullptr, dev, nullptr, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(tab.data(), 40, -1, dev, dev, skip, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    // the order: nesterov before n == 0; n < 0 before the pointers; scalars before gscale before skip; all before the table
    CHECK(qt_optim_sgd_f32(nullptr, 0, 0, 0.1f, nullptr, nullptr, nullptr, 0.0f, 0.0f, 1, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), -1, DEV, 0.1f, fake(0x6002), nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, DEV | GS, 0.1f, fake(0x6002), nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, DEV | GS, 0.1f, nullptr, fake(0x6002), nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_adam_f32(tab.data(), 40, GS | SK, nullptr, fake(0x6002), nullptr, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_adam_f32(tab.data(), 40, GS | SK, nullptr, nullptr, skip2, 0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, 0.0f, nullptr) == QT_ERR_INVALID_ARG);
    tab[0].p = nullptr;                                                        // INVALID_ARG from the table ...
    CHECK(qt_optim_sgd_f32(tab.data(), 40, SK, 0.1f, nullptr, nullptr, skip2, 0.0f, 0.0f, 0, nullptr) == QT_ERR_ALIGNMENT);
    tab[0].p = fake(0x50000002);                                               // ... and ALIGNMENT
    CHECK(qt_optim_sgd_f32(tab.data(), 40, SK, 0.1f, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_sgd_f32(tab.data(), 40, SK, 0.1f, nullptr, nullptr, skip, 0.0f, 0.0f, 0, nullptr) == QT_ERR_ALIGNMENT);
    tab[0] = tensor(5000, 0x50000000);
    CHECK(qt_optim_grad_norm_finalize_f32(dev, -1, 1.0f, nullptr, dev, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_grad_norm_finalize_f32(nullptr, 3, 1.0f, nullptr, dev, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_grad_norm_finalize_f32(dev, 3, 1.0f, nullptr, nullptr, nullptr) == QT_ERR_INVALID_ARG);
    CHECK(qt_optim_grad_norm_finalize_f32(dev, 3, 1.0f, fake(0x6002), dev, nullptr) == QT_ERR_ALIGNMENT);
    CHECK(qt_optim_grad_norm_finalize_f32(dev, 3, 1.0f, nullptr, fake(0x6002), nullptr) == QT_ERR_ALIGNMENT);
    std::puts("optim_clip_host_check: ok");
    return 0;
}
