// de_layout_check.cpp — the work layout of differential evolution (DeWork of csrc/draws/octo_draws_layout.h) on host memory;
// tests/test_de_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (D, ld) as arguments, two numbers a
// shape. For each: size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles, lay the parts
// out, fill every element of every part with the part's own tag, read all of them back, and print one JSON line with the size, the number of
// pointers in the struct and each part's offset, element size, length and position in the struct. The lengths are stated here, not taken
// from the header.
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
    size_t member;      // offsetof the pointer in DeWork
};

#define PART(s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(DeWork, m)}

static std::vector<Part> parts_of(const DeWork& s, int64_t D, int64_t ld) {
    return {PART(s, pop0, D * ld), PART(s, pop1, D * ld), PART(s, trial0, D * ld), PART(s, trial1, D * ld), PART(s, gpr, D * ld), PART(s, lp, ld), PART(s, f0, ld),
            PART(s, f1, ld), PART(s, tlpt0, ld), PART(s, tlpt1, ld), PART(s, lpt, ld), PART(s, F, ld), PART(s, CR, ld), PART(s, Ft, ld), PART(s, CRt, ld),
            PART(s, n_accept, ld), PART(s, improved, ld)};
}

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

int main(int argc, char** argv) {
    if (argc < 3 || (argc - 1) % 2 != 0) return 3;
    for (int a = 1; a + 1 < argc; a += 2) {
        const int64_t D = std::atoll(argv[a]), ld = std::atoll(argv[a + 1]);
        const int64_t size = carve_size(de_work, D, ld);
        for (const Part& q : parts_of(carve_at(nullptr, de_work, D, ld), D, ld)) if (q.p) return 2;
        double* buf = new double[size];
        const DeWork s = carve_at(buf, de_work, D, ld);
        const std::vector<Part> parts = parts_of(s, D, ld);
        for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
        std::printf("{\"layout\": \"de_work\", \"shape\": [%lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)D, (long long)ld, (long long)size,
                    sizeof(s) / sizeof(void*));
        for (size_t k = 0; k < parts.size(); ++k) {
            const Part& q = parts[k];
            std::printf("%s{\"name\": \"%s\", \"offset\": %lld, \"elem\": %zu, \"len\": %lld, \"member\": %zu, \"tag_ok\": %s}", k ? ", " : "", q.name,
                        (long long)((const char*)q.p - (const char*)buf), q.elem, (long long)q.len, q.member, holds(q, (int)k + 1) ? "true" : "false");
        }
        std::printf("]}\n");
        delete[] buf;
    }
    return 0;
}
