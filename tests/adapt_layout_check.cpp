// adapt_layout_check.cpp — the block partials of the grouped moments (moments_partials of csrc/draws/octo_draws_layout.h) on host memory
// (tests/test_adapt_layout.py compiles this with -fsanitize=address,undefined and runs it), by the method of draws_layout_check.cpp: size
// the layout with a null base, allocate exactly that many doubles, lay the parts out, fill every element of every part with the part's own
// tag, read all of them back, and print one JSON line a shape. The lengths are stated here, not taken from the header.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "octo_draws_layout.h"

struct Part {
    const char* name;
    double* p;
    int64_t len;        // elements
    size_t member;      // offsetof the pointer in the struct
};

#define PART(s, m, len) Part{#m, (s).m, (len), offsetof(MomentsPartials, m)}

int main() {
    const int64_t shapes[4][3] = {{1, 1, 1}, {3, 5, 2}, {7, 64, 64}, {4, 3, 11}};      // (nblk, G, K)
    for (const auto& sh : shapes) {
        const int64_t nblk = sh[0], G = sh[1], K = sh[2];
        const int64_t size = carve_size(moments_partials, nblk, G, K);
        const MomentsPartials none = carve_at(nullptr, moments_partials, nblk, G, K);
        if (none.cnt || none.sum || none.m2) return 2;      // a null base hands out null pointers
        double* buf = new double[size];
        const MomentsPartials s = carve_at(buf, moments_partials, nblk, G, K);
        const std::vector<Part> parts = {PART(s, cnt, nblk * G), PART(s, sum, nblk * G * K), PART(s, m2, nblk * G * K)};
        for (size_t k = 0; k < parts.size(); ++k)
            for (int64_t j = 0; j < parts[k].len; ++j) parts[k].p[j] = (double)(k + 1);
        std::printf("{\"layout\": \"moments_partials\", \"shape\": [%lld, %lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)nblk, (long long)G,
                    (long long)K, (long long)size, sizeof(s) / sizeof(void*));
        for (size_t k = 0; k < parts.size(); ++k) {
            bool ok = true;
            for (int64_t j = 0; j < parts[k].len; ++j) ok = ok && parts[k].p[j] == (double)(k + 1);
            std::printf("%s{\"name\": \"%s\", \"offset\": %lld, \"elem\": %zu, \"len\": %lld, \"member\": %zu, \"tag_ok\": %s}", k ? ", " : "", parts[k].name,
                        (long long)((const char*)parts[k].p - (const char*)buf), sizeof(double), (long long)parts[k].len, parts[k].member, ok ? "true" : "false");
        }
        std::printf("]}\n");
        delete[] buf;
    }
    return 0;
}
