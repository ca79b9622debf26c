// gp_layout_check.cpp — the work layouts of the Gaussian-process RV term (GpWork and GpStaging of csrc/draws/octo_draws_layout.h) on host
// memory; tests/test_gp_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (n, n_state, n_planets, ldw, H, K, grad) as
// arguments, seven numbers a shape. For each: size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles,
// lay the parts out, fill every element of every part with the part's own tag, read all of them back, and print one JSON line with the size, the number
// of pointers in the struct and each part's offset, element size, length and position in the struct. The lengths are stated here, not taken from the
// header. The staging layout of (P, H, K, ld = ldw) follows on a line of its own.
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

static std::vector<Part> parts_of(const GpWork& s, int64_t n, int64_t n_state, int64_t n_seg, int64_t n_tasks, int64_t n_sums, int64_t ldw, int64_t grad) {
    return {PART(GpWork, s, res, n * ldw), PART(GpWork, s, ok, ldw), PART(GpWork, s, check, grad * n_seg * n_state * ldw), PART(GpWork, s, seg, grad * 16 * n_state * ldw),
            PART(GpWork, s, part, grad * n_tasks * n_sums * ldw)};
}
static std::vector<Part> parts_of(const GpStaging& s, int64_t P, int64_t H, int64_t K, int64_t ld) {
    return {PART(GpStaging, s, elems, 9 * P * ld), PART(GpStaging, s, g_elems, 9 * P * ld), PART(GpStaging, s, hyper, H * ld), PART(GpStaging, s, g_hyper, H * ld),
            PART(GpStaging, s, beta, K * ld), PART(GpStaging, s, g_beta, K * ld), PART(GpStaging, s, jitter, ld), PART(GpStaging, s, g_jitter, ld), PART(GpStaging, s, ll, ld)};
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

static void report(const char* layout, const std::vector<Part>& parts, const double* buf, int64_t size, size_t members, const int64_t* shape, int n_shape) {
    std::printf("{\"layout\": \"%s\", \"shape\": [", layout);
    for (int k = 0; k < n_shape; ++k) std::printf("%s%lld", k ? ", " : "", (long long)shape[k]);
    std::printf("], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)size, members);
    for (size_t k = 0; k < parts.size(); ++k) {
        const Part& q = parts[k];
        std::printf("%s{\"name\": \"%s\", \"offset\": %lld, \"elem\": %zu, \"len\": %lld, \"member\": %zu, \"tag_ok\": %s}", k ? ", " : "", q.name,
                    (long long)((const char*)q.p - (const char*)buf), q.elem, (long long)q.len, q.member, holds(q, (int)k + 1) ? "true" : "false");
    }
    std::printf("]}\n");
}

int main(int argc, char** argv) {
    if (argc < 8 || (argc - 1) % 7 != 0) return 3;
    for (int a = 1; a + 6 < argc; a += 7) {
        const int64_t n = std::atoll(argv[a]), n_state = std::atoll(argv[a + 1]), P = std::atoll(argv[a + 2]), ldw = std::atoll(argv[a + 3]), H = std::atoll(argv[a + 4]),
                      K = std::atoll(argv[a + 5]), grad = std::atoll(argv[a + 6]);
        const int64_t n_seg = (n + 15) / 16, n_tasks = (n + 7) / 8, n_sums = 4 + 6 * P;
        {
            const int64_t size = carve_size(gp_work, n, n_state, n_seg, (int64_t)16, n_tasks, n_sums, ldw, grad);
            for (const Part& q : parts_of(carve_at(nullptr, gp_work, n, n_state, n_seg, (int64_t)16, n_tasks, n_sums, ldw, grad), n, n_state, n_seg, n_tasks, n_sums, ldw, grad))
                if (q.p) return 2;
            double* buf = new double[size];
            const GpWork s = carve_at(buf, gp_work, n, n_state, n_seg, (int64_t)16, n_tasks, n_sums, ldw, grad);
            const std::vector<Part> parts = parts_of(s, n, n_state, n_seg, n_tasks, n_sums, ldw, grad);
            for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
            const int64_t shape[5] = {n, n_state, P, ldw, grad};
            report("gp_work", parts, buf, size, sizeof(s) / sizeof(void*), shape, 5);
            delete[] buf;
        }
        {
            const int64_t size = carve_size(gp_staging, P, H, K, ldw);
            for (const Part& q : parts_of(carve_at(nullptr, gp_staging, P, H, K, ldw), P, H, K, ldw)) if (q.p) return 2;
            double* buf = new double[size];
            const GpStaging s = carve_at(buf, gp_staging, P, H, K, ldw);
            const std::vector<Part> parts = parts_of(s, P, H, K, ldw);
            for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
            const int64_t shape[4] = {P, H, K, ldw};
            report("gp_staging", parts, buf, size, sizeof(s) / sizeof(void*), shape, 4);
            delete[] buf;
        }
    }
    return 0;
}
