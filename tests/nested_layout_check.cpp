// nested_layout_check.cpp — the work layouts of nested sampling (NestedWork and NestedCull of csrc/draws/octo_draws_layout.h) on host memory;
// tests/test_nested_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (D, ld) as arguments, two numbers a
// shape (the cull's order is laid out for K = ld). For each layout: size it with a null base (which must hand out null pointers), allocate
// exactly that many doubles, lay the parts out, fill every element of every part with the part's own tag, read all of them back, and print
// one JSON line with the size, the number of pointers in the struct and each part's offset, element size, length and position in the struct.
// The lengths are stated here, not taken from the header.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "octo_draws_layout.h"

struct Part {
    const char* name;
    void* p;
    size_t elem;        // bytes of an element
    int64_t len;        // elements
    size_t member;      // offsetof the pointer in its struct
};

#define PART(T, s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(T, m)}

static std::vector<Part> parts_of(const NestedWork& s, int64_t D, int64_t ld) {
    return {PART(NestedWork, s, trial, D * ld), PART(NestedWork, s, gpr, D * ld), PART(NestedWork, s, u, D * ld), PART(NestedWork, s, lp, ld),
            PART(NestedWork, s, L, ld), PART(NestedWork, s, R, ld), PART(NestedWork, s, xp, ld), PART(NestedWork, s, keep, ld),
            PART(NestedWork, s, status, ld), PART(NestedWork, s, j, ld), PART(NestedWork, s, phase, ld), PART(NestedWork, s, s, ld),
            PART(NestedWork, s, J, ld), PART(NestedWork, s, Kr, ld), PART(NestedWork, s, n_eval, ld), PART(NestedWork, s, n_step, ld),
            PART(NestedWork, s, n_shrink, ld), PART(NestedWork, s, n_stuck, ld)};
}
static std::vector<Part> parts_of(const NestedCull& s, int64_t K) { return {PART(NestedCull, s, order, K)}; }

// element k of a part holds the part's tag in its own width (4-byte elements at 4-byte stride, as the kernels index them)
static void fill(const Part& q, int tag) {
    const int64_t t8 = tag; const int32_t t4 = tag;
    for (int64_t k = 0; k < q.len; ++k) std::memcpy((char*)q.p + k * q.elem, q.elem == 4 ? (const void*)&t4 : (const void*)&t8, q.elem);
}
static bool holds(const Part& q, int tag) {
    const int64_t t8 = tag; const int32_t t4 = tag;
    bool ok = true;
    for (int64_t k = 0; k < q.len; ++k) ok = ok && std::memcmp((const char*)q.p + k * q.elem, q.elem == 4 ? (const void*)&t4 : (const void*)&t8, q.elem) == 0;
    return ok;
}

static void report(const char* layout, int64_t D, int64_t ld, int64_t size, size_t members, std::vector<Part>& parts, const double* buf) {
    for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
    std::printf("{\"layout\": \"%s\", \"shape\": [%lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", layout, (long long)D, (long long)ld, (long long)size, members);
    for (size_t k = 0; k < parts.size(); ++k) {
        const Part& q = parts[k];
        std::printf("%s{\"name\": \"%s\", \"offset\": %lld, \"elem\": %zu, \"len\": %lld, \"member\": %zu, \"tag_ok\": %s}", k ? ", " : "", q.name,
                    (long long)((const char*)q.p - (const char*)buf), q.elem, (long long)q.len, q.member, holds(q, (int)k + 1) ? "true" : "false");
    }
    std::printf("]}\n");
}

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2 != 0) return 3;
    for (int a = 1; a + 1 < argc; a += 2) {
        const int64_t D = std::atoll(argv[a]), ld = std::atoll(argv[a + 1]);
        {
            const int64_t size = carve_size(nested_work, D, ld);
            for (const Part& q : parts_of(carve_at(nullptr, nested_work, D, ld), D, ld)) if (q.p) return 2;
            double* buf = new double[size];
            const NestedWork s = carve_at(buf, nested_work, D, ld);
            std::vector<Part> parts = parts_of(s, D, ld);
            report("nested_work", D, ld, size, sizeof(s) / sizeof(void*), parts, buf);
            delete[] buf;
        }
        {
            const int64_t K = ld, size = carve_size(nested_cull, K);
            for (const Part& q : parts_of(carve_at(nullptr, nested_cull, K), K)) if (q.p) return 2;
            double* buf = new double[size];
            const NestedCull s = carve_at(buf, nested_cull, K);
            std::vector<Part> parts = parts_of(s, K);
            report("nested_cull", D, ld, size, sizeof(s) / sizeof(void*), parts, buf);
            delete[] buf;
        }
    }
    return 0;
}
