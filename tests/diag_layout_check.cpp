// diag_layout_check.cpp — the work layout of the convergence diagnostics (DiagWork of csrc/draws/octo_draws_layout.h) on host memory;
// tests/test_diag_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (K, P, S, M, T, nblk) as arguments, six
// numbers a shape. For each: size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles, lay
// the parts out, fill every element of every part with the part's own tag, read all of them back, and print one JSON line with the size, the
// number of pointers in the struct and each part's offset, element size, length and position in the struct. The lengths are stated here,
// not taken from the header.
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
    size_t member;      // offsetof the pointer in DiagWork
};

#define PART(s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(DiagWork, m)}

static std::vector<Part> parts_of(const DiagWork& s, int64_t K, int64_t P, int64_t S, int64_t M, int64_t T, int64_t nblk) {
    return {PART(s, keys, K * P), PART(s, fkeys, K * P), PART(s, z, K * S), PART(s, zf, K * S), PART(s, mu, 5 * K * M), PART(s, var, 5 * K * M),
            PART(s, part, 4 * K * T * nblk), PART(s, rho, 4 * K * T), PART(s, q, 3 * K), PART(s, bad, K), PART(s, ok, K)};
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
    if (argc < 7 || (argc - 1) % 6 != 0) return 3;
    for (int a = 1; a + 5 < argc; a += 6) {
        int64_t v[6];
        for (int k = 0; k < 6; ++k) v[k] = std::atoll(argv[a + k]);
        const int64_t K = v[0], P = v[1], S = v[2], M = v[3], T = v[4], nblk = v[5];
        const int64_t size = carve_size(diag_work, K, P, S, M, T, nblk);
        for (const Part& q : parts_of(carve_at(nullptr, diag_work, K, P, S, M, T, nblk), K, P, S, M, T, nblk)) if (q.p) return 2;
        double* buf = new double[size];
        const DiagWork s = carve_at(buf, diag_work, K, P, S, M, T, nblk);
        const std::vector<Part> parts = parts_of(s, K, P, S, M, T, nblk);
        for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
        std::printf("{\"layout\": \"diag_work\", \"shape\": [%lld, %lld, %lld, %lld, %lld, %lld], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)K,
                    (long long)P, (long long)S, (long long)M, (long long)T, (long long)nblk, (long long)size, sizeof(s) / sizeof(void*));
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
