// dense_layout_check.cpp — the block partials of the pooled covariance (CovPartials / cov_partials of csrc/draws/octo_draws_layout.h) on host
// memory; tests/test_dense_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (nblk, K) as arguments, two
// numbers a shape. For each: size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles, lay the
// parts out, fill every element of every part with the part's own tag, read all of them back, and print one JSON line with the size, the number
// of pointers in the struct and each part's offset, element size, length and position in the struct. The lengths are stated here, not taken
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
    size_t member;      // offsetof the pointer in its struct
};

#define PART(T, s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(T, m)}

static std::vector<Part> parts_of(const CovPartials& s, int64_t nblk, int64_t K) {
    return {PART(CovPartials, s, cnt, nblk), PART(CovPartials, s, sum, nblk * K), PART(CovPartials, s, m2, nblk * (K * (K + 1) / 2))};
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
    if (argc < 3 || (argc - 1) % 2 != 0) return 3;
    for (int a = 1; a + 1 < argc; a += 2) {
        const int64_t nblk = std::atoll(argv[a]), K = std::atoll(argv[a + 1]);
        const int64_t size = carve_size(cov_partials, nblk, K);
        for (const Part& q : parts_of(carve_at(nullptr, cov_partials, nblk, K), nblk, K)) if (q.p) return 2;
        double* buf = new double[size];
        const CovPartials s = carve_at(buf, cov_partials, nblk, K);
        std::vector<Part> parts = parts_of(s, nblk, K);
        for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
        std::printf("{\"layout\": \"cov_partials\", \"shape\": [%lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)nblk, (long long)K,
                    (long long)size, sizeof(s) / sizeof(void*));
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
