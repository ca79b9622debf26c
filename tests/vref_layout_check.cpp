// vref_layout_check.cpp — the reference table of a variational tempering leg (RefTable of csrc/draws/octo_draws_layout.h) on host memory;
// tests/test_vref_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (D, nc, icn) as arguments, three numbers a
// shape. For each: size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles, lay the parts out,
// fill every element of every part with the part's own tag, read all of them back, and print one JSON line with the size, the number of
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
    size_t member;      // offsetof the pointer in RefTable
};

#define PART(s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(RefTable, m)}

static std::vector<Part> parts_of(const RefTable& s, int64_t D, int64_t nc, int64_t icn) {
    return {PART(s, priors, 5 * D), PART(s, pc, nc * D), PART(s, ic, icn * D), PART(s, mean, D), PART(s, sd, D)};      // an octo_prior is 40 bytes
}

static void fill(const Part& q, int tag) {
    const int64_t t8 = tag;
    for (int64_t k = 0; k < q.len; ++k) std::memcpy((char*)q.p + k * q.elem, &t8, q.elem);
}
static bool holds(const Part& q, int tag) {
    const int64_t t8 = tag;
    bool ok = true;
    for (int64_t k = 0; k < q.len; ++k) ok = ok && std::memcmp((const char*)q.p + k * q.elem, &t8, q.elem) == 0;
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) return 3;
    for (int a = 1; a + 2 < argc; a += 3) {
        const int64_t D = std::atoll(argv[a]), nc = std::atoll(argv[a + 1]), icn = std::atoll(argv[a + 2]);
        const int64_t size = carve_size(ref_table, D, nc, icn);
        for (const Part& q : parts_of(carve_at(nullptr, ref_table, D, nc, icn), D, nc, icn)) if (q.p) return 2;
        double* buf = new double[size];
        const RefTable s = carve_at(buf, ref_table, D, nc, icn);
        const std::vector<Part> parts = parts_of(s, D, nc, icn);
        for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
        std::printf("{\"layout\": \"ref_table\", \"shape\": [%lld, %lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)D, (long long)nc,
                    (long long)icn, (long long)size, sizeof(s) / sizeof(void*));
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
