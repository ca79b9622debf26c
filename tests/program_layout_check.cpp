// program_layout_check.cpp — the work arrays of an expression program (ProgWork of csrc/draws/octo_draws_layout.h) on host memory;
// tests/test_program_reference.py compiles this with -fsanitize=address,undefined and runs it with the shapes (D, N, n_in, P, ldw) as
// arguments, five numbers a shape. For each: size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles, lay the parts out,
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
    size_t member;      // offsetof the pointer in ProgWork
};

#define PART(s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(ProgWork, m)}

static std::vector<Part> parts_of(const ProgWork& s, int64_t D, int64_t N, int64_t n_in, int64_t P, int64_t ldw) {
    return {PART(s, vals, N * ldw), PART(s, dx, D * ldw), PART(s, gpd, D * ldw), PART(s, inputs, n_in * ldw), PART(s, g_in, n_in * ldw),
            PART(s, gtp, 7 * P * ldw), PART(s, pp, ldw), PART(s, ll, ldw), PART(s, healed, ldw)};
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
    if (argc < 6 || (argc - 1) % 5 != 0) return 3;
    for (int a = 1; a + 4 < argc; a += 5) {
        const int64_t D = std::atoll(argv[a]), N = std::atoll(argv[a + 1]), n_in = std::atoll(argv[a + 2]), P = std::atoll(argv[a + 3]), ldw = std::atoll(argv[a + 4]);
        const int64_t size = carve_size(prog_work, D, N, n_in, P, ldw);
        for (const Part& q : parts_of(carve_at(nullptr, prog_work, D, N, n_in, P, ldw), D, N, n_in, P, ldw)) if (q.p) return 2;
        double* buf = new double[size];
        const ProgWork s = carve_at(buf, prog_work, D, N, n_in, P, ldw);
        const std::vector<Part> parts = parts_of(s, D, N, n_in, P, ldw);
        for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
        std::printf("{\"layout\": \"prog_work\", \"shape\": [%lld, %lld, %lld, %lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)D,
                    (long long)N, (long long)n_in, (long long)P, (long long)ldw, (long long)size, sizeof(s) / sizeof(void*));
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
