// scan_layout_check.cpp — the work layouts of along-scan absolute astrometry (ScanWork and ScanStaging of csrc/draws/octo_draws_layout.h) on host
// memory; tests/test_scan_layout.py compiles this with -fsanitize=address,undefined and runs it with the shapes (n_tasks, n_sums, ldw, P, K) as
// arguments, five numbers a shape. For each: size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles,
// lay the parts out, fill every element of every part with the part's own tag, read all of them back, and print one JSON line with the size, the number
// of pointers in the struct and each part's offset, element size, length and position in the struct. The lengths are stated here, not taken from the
// header. The staging layout of (P, K, ld = ldw) follows on a line of its own.
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

static std::vector<Part> parts_of(const ScanWork& s, int64_t n_tasks, int64_t n_sums, int64_t ldw) {
    return {PART(ScanWork, s, part, n_tasks * n_sums * ldw), PART(ScanWork, s, marg, 28 * ldw)};
}
static std::vector<Part> parts_of(const ScanStaging& s, int64_t P, int64_t K, int64_t ld) {
    return {PART(ScanStaging, s, elems, 9 * P * ld), PART(ScanStaging, s, g_elems, 9 * P * ld), PART(ScanStaging, s, beta, K * ld), PART(ScanStaging, s, g_beta, K * ld),
            PART(ScanStaging, s, beta_hat, K * ld), PART(ScanStaging, s, jitter, ld), PART(ScanStaging, s, g_jitter, ld), PART(ScanStaging, s, ll, ld)};
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
    if (argc < 6 || (argc - 1) % 5 != 0) return 3;
    for (int a = 1; a + 4 < argc; a += 5) {
        const int64_t n_tasks = std::atoll(argv[a]), n_sums = std::atoll(argv[a + 1]), ldw = std::atoll(argv[a + 2]), P = std::atoll(argv[a + 3]), K = std::atoll(argv[a + 4]);
        {
            const int64_t size = carve_size(scan_work, n_tasks, n_sums, ldw);
            for (const Part& q : parts_of(carve_at(nullptr, scan_work, n_tasks, n_sums, ldw), n_tasks, n_sums, ldw)) if (q.p) return 2;
            double* buf = new double[size];
            const ScanWork s = carve_at(buf, scan_work, n_tasks, n_sums, ldw);
            const std::vector<Part> parts = parts_of(s, n_tasks, n_sums, ldw);
            for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
            const int64_t shape[3] = {n_tasks, n_sums, ldw};
            report("scan_work", parts, buf, size, sizeof(s) / sizeof(void*), shape, 3);
            delete[] buf;
        }
        {
            const int64_t size = carve_size(scan_staging, P, K, ldw);
            for (const Part& q : parts_of(carve_at(nullptr, scan_staging, P, K, ldw), P, K, ldw)) if (q.p) return 2;
            double* buf = new double[size];
            const ScanStaging s = carve_at(buf, scan_staging, P, K, ldw);
            const std::vector<Part> parts = parts_of(s, P, K, ldw);
            for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
            const int64_t shape[3] = {P, K, ldw};
            report("scan_staging", parts, buf, size, sizeof(s) / sizeof(void*), shape, 3);
            delete[] buf;
        }
    }
    return 0;
}
