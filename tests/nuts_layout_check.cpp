// nuts_layout_check.cpp — the trees of a NUTS transition (nuts_work of csrc/draws/octo_draws_layout.h) on host memory (tests/test_nuts_layout.py
// compiles this with -fsanitize=address,undefined and runs it), by the method of adapt_layout_check.cpp: size the layout with a null base,
// allocate exactly that many doubles, lay the parts out, fill every element of every part with the part's own tag, read all of them back, and
// print one JSON line a shape. The lengths are stated here, not taken from the header. A part of int32 elements takes a double's room each.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "octo_draws_layout.h"

struct Part {
    const char* name;
    void* p;
    int64_t len;        // elements
    size_t elem;        // bytes of one
    size_t member;      // offsetof the pointer in the struct
};

#define PART(s, m, len) Part{#m, (s).m, (len), sizeof(*(s).m), offsetof(NutsWork, m)}

int main() {
    const int64_t shapes[5][3] = {{1, 1, 1}, {14, 72, 4}, {5, 65536, 5}, {64, 3, 10}, {3, 257, 2}};      // (D, ld, max_depth)
    for (const auto& sh : shapes) {
        const int64_t D = sh[0], ld = sh[1], md = sh[2], plane = D * ld;
        const int64_t size = carve_size(nuts_work, D, ld, md);
        const NutsWork none = carve_at(nullptr, nuts_work, D, ld, md);
        if (none.trial || none.ck_r || none.ssel) return 2;      // a null base hands out null pointers
        double* buf = new double[size];
        const NutsWork s = carve_at(buf, nuts_work, D, ld, md);
        const std::vector<Part> parts = {
            PART(s, trial, plane), PART(s, pt, plane), PART(s, qL, plane), PART(s, pL, plane), PART(s, gL, plane), PART(s, qR, plane), PART(s, pR, plane),
            PART(s, gR, plane), PART(s, prop, plane), PART(s, sprop, plane), PART(s, rho, plane), PART(s, rho_s, plane), PART(s, gpr, plane), PART(s, glp, plane),
            PART(s, ck_p, md * plane), PART(s, ck_r, md * plane),
            PART(s, lp, ld), PART(s, H0, ld), PART(s, logw, ld), PART(s, logw_s, ld), PART(s, sum_acc, ld), PART(s, prop_lp, ld), PART(s, prop_lpt, ld),
            PART(s, sprop_lp, ld), PART(s, sprop_lpt, ld), PART(s, out_lp, ld), PART(s, out_lpt, ld),
            PART(s, status, ld), PART(s, depth, ld), PART(s, n, ld), PART(s, nleaf, ld), PART(s, v, ld), PART(s, sel, ld), PART(s, ssel, ld)};
        for (size_t k = 0; k < parts.size(); ++k)
            for (int64_t j = 0; j < parts[k].len; ++j) {
                if (parts[k].elem == 8) static_cast<double*>(parts[k].p)[j] = (double)(k + 1);
                else static_cast<int32_t*>(parts[k].p)[j] = (int32_t)(k + 1);
            }
        std::printf("{\"layout\": \"nuts_work\", \"shape\": [%lld, %lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)D, (long long)ld,
                    (long long)md, (long long)size, sizeof(s) / sizeof(void*));
        for (size_t k = 0; k < parts.size(); ++k) {
            bool ok = true;
            for (int64_t j = 0; j < parts[k].len; ++j)
                ok = ok && (parts[k].elem == 8 ? static_cast<double*>(parts[k].p)[j] == (double)(k + 1) : static_cast<int32_t*>(parts[k].p)[j] == (int32_t)(k + 1));
            std::printf("%s{\"name\": \"%s\", \"offset\": %lld, \"elem\": %zu, \"len\": %lld, \"member\": %zu, \"tag_ok\": %s}", k ? ", " : "", parts[k].name,
                        (long long)((const char*)parts[k].p - (const char*)buf), parts[k].elem, (long long)parts[k].len, parts[k].member, ok ? "true" : "false");
        }
        std::printf("]}\n");
        delete[] buf;
    }
    return 0;
}
