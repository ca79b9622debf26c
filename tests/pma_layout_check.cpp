// pma_layout_check.cpp — the work layouts of the catalogue proper-motion anomaly (PmaWork and PmaStaging of csrc/draws/octo_draws_layout.h) on host
// memory, and the host-made table algebra of csrc/draws/octo_draws_pma_host.h; tests/test_pma_layout.py compiles this with -fsanitize=address,undefined
// and runs it with the shapes (n_tasks, n_sums, ldw, P, K) as arguments, five numbers a shape, then the word `algebra` and pairs (Q, K). For each shape:
// size the layout with a null base (which must hand out null pointers), allocate exactly that many doubles, lay the parts out, fill every element of
// every part with the part's own tag, read all of them back, and print one JSON line with the size, the number of pointers in the struct and each
// part's offset, element size, length and position in the struct. The lengths are stated here, not taken from the header. The staging layout of
// (P, K, ld = ldw) follows on a line of its own. For each (Q, K): pma_table_build on a Σ = A·Aᵀ + I, an H and a d made here, one JSON line with the inputs
// and every result at 17 digits, and a line with the statuses of an indefinite Σ, an asymmetric Σ and a rank-deficient H. The algebra lines come first.
#include <cmath>
#include <cstdint>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "octo_draws_layout.h"
#include "octo_draws_pma_host.h"

struct Part {
    const char* name;
    void* p;
    size_t elem;        // bytes of an element
    int64_t len;        // elements
    size_t member;      // offsetof the pointer in its struct
};

#define PART(T, s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(T, m)}

static std::vector<Part> parts_of(const PmaWork& s, int64_t n_tasks, int64_t n_sums, int64_t ldw) {
    return {PART(PmaWork, s, part, n_tasks * n_sums * ldw), PART(PmaWork, s, lam, 8 * ldw), PART(PmaWork, s, ok, ldw)};
}
static std::vector<Part> parts_of(const PmaStaging& s, int64_t P, int64_t K, int64_t ld) {
    return {PART(PmaStaging, s, elems, 9 * P * ld), PART(PmaStaging, s, g_elems, 9 * P * ld), PART(PmaStaging, s, gamma, K * ld), PART(PmaStaging, s, g_gamma, K * ld),
            PART(PmaStaging, s, gamma_hat, K * ld), PART(PmaStaging, s, ll, ld)};
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


// ---- the table algebra of octo_draws_pma_host.h at (Q, K): Σ = A·Aᵀ + I and H, d from a fixed recurrence; one JSON line with the inputs and the results
static double next_value(uint64_t& s) {      // a 64-bit LCG's upper bits in (−1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(s >> 11) / 4503599627370496.0 - 1.0;
}
static void print_array(const char* name, const double* x, int rows, int cols, int stride, bool last = false) {
    std::printf("\"%s\": [", name);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) std::printf("%s%.17g", i + j ? ", " : "", x[i * stride + j]);
    std::printf("]%s", last ? "" : ", ");
}
static bool zeros_behind(const PmaTable& t, int Q, int K) {      // the padding the device's fixed-size loops rely on
    bool ok = true;
    for (int m = 0; m < 2; ++m)
        for (int i = 0; i < PMA_Q; ++i)
            for (int j = 0; j < PMA_Q; ++j) ok = ok && ((i < Q && j < Q) || t.M[m][i * PMA_Q + j] == 0.0);
    for (int q = 0; q < PMA_Q; ++q)
        for (int k = 0; k < PMA_K; ++k) ok = ok && ((q < Q && k < K) || (t.H[q * PMA_K + k] == 0.0 && t.G[k * PMA_Q + q] == 0.0));
    for (int q = Q; q < PMA_Q; ++q) ok = ok && t.d[q] == 0.0;
    return ok;
}
static int algebra(int Q, int K) {
    uint64_t s = 1000 * (uint64_t)Q + (uint64_t)K + 17;
    std::vector<double> A((size_t)Q * Q), cov((size_t)Q * Q), H((size_t)Q * (K ? K : 1)), d((size_t)Q);
    for (double& x : A) x = next_value(s);
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j < Q; ++j) {
            double x = i == j ? 1.0 : 0.0;
            for (int k = 0; k < Q; ++k) x += A[i * Q + k] * A[j * Q + k];
            cov[i * Q + j] = x;
        }
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j < i; ++j) cov[i * Q + j] = cov[j * Q + i];      // exactly symmetric whatever the order of the sums
    for (int i = 0; i < Q * K; ++i) H[i] = next_value(s);
    for (double& x : d) x = 3.0 * next_value(s);
    PmaTable t;
    const int rc = pma_table_build(cov.data(), K ? H.data() : nullptr, d.data(), Q, K, &t);
    std::printf("{\"algebra\": [%d, %d], \"rc\": %d, \"marg_ok\": %d, \"padded\": %s, ", Q, K, rc, (int)t.marg_ok, zeros_behind(t, Q, K) ? "true" : "false");
    print_array("cov", cov.data(), Q, Q, Q);
    print_array("H", H.data(), Q, K, K);
    print_array("d_in", d.data(), 1, Q, Q);
    print_array("Sinv", t.M[0], Q, Q, PMA_Q);
    print_array("Pm", t.M[1], Q, Q, PMA_Q);
    print_array("H_out", t.H, Q, K, PMA_K);
    print_array("G", t.G, K, Q, PMA_Q);
    print_array("d", t.d, 1, Q, PMA_Q);
    print_array("cst", t.cst, 1, 2, 2, true);
    std::printf("}\n");
    // refusals: an indefinite Σ (2), an asymmetric one (1); a rank-deficient H is no error but leaves marg_ok = 0
    std::vector<double> bad = cov;
    bad[0] = -bad[0];
    const int rc_indef = pma_table_build(bad.data(), K ? H.data() : nullptr, d.data(), Q, K, &t);
    int rc_asym = 1;
    if (Q > 1) {
        bad = cov;
        bad[1] += 1e-6 * std::sqrt(cov[0] * cov[Q + 1]);
        rc_asym = pma_table_build(bad.data(), K ? H.data() : nullptr, d.data(), Q, K, &t);
    }
    int rc_rank = 0, ok_rank = 0;
    if (K > 1) {
        std::vector<double> Hd = H;
        for (int q = 0; q < Q; ++q) Hd[q * K + K - 1] = 2.0 * Hd[q * K];
        rc_rank = pma_table_build(cov.data(), Hd.data(), d.data(), Q, K, &t);
        ok_rank = t.marg_ok;
    }
    std::printf("{\"refusals\": [%d, %d], \"indefinite\": %d, \"asymmetric\": %d, \"rank_deficient\": [%d, %d]}\n", Q, K, rc_indef, rc_asym, rc_rank, ok_rank);
    return 0;
}

int main(int argc, char** argv) {
    int n_layout = 1;
    while (n_layout < argc && std::strcmp(argv[n_layout], "algebra") != 0) ++n_layout;
    if ((n_layout - 1) % 5 != 0 || (argc > n_layout && (argc - n_layout - 1) % 2 != 0)) return 3;
    for (int a = n_layout + 1; a + 1 < argc; a += 2)
        if (algebra(std::atoi(argv[a]), std::atoi(argv[a + 1]))) return 4;
    for (int a = 1; a + 4 < n_layout; a += 5) {
        const int64_t n_tasks = std::atoll(argv[a]), n_sums = std::atoll(argv[a + 1]), ldw = std::atoll(argv[a + 2]), P = std::atoll(argv[a + 3]), K = std::atoll(argv[a + 4]);
        {
            const int64_t size = carve_size(pma_work, n_tasks, n_sums, ldw);
            for (const Part& q : parts_of(carve_at(nullptr, pma_work, n_tasks, n_sums, ldw), n_tasks, n_sums, ldw)) if (q.p) return 2;
            double* buf = new double[size];
            const PmaWork s = carve_at(buf, pma_work, n_tasks, n_sums, ldw);
            const std::vector<Part> parts = parts_of(s, n_tasks, n_sums, ldw);
            for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
            const int64_t shape[3] = {n_tasks, n_sums, ldw};
            report("pma_work", parts, buf, size, sizeof(s) / sizeof(void*), shape, 3);
            delete[] buf;
        }
        {
            const int64_t size = carve_size(pma_staging, P, K, ldw);
            for (const Part& q : parts_of(carve_at(nullptr, pma_staging, P, K, ldw), P, K, ldw)) if (q.p) return 2;
            double* buf = new double[size];
            const PmaStaging s = carve_at(buf, pma_staging, P, K, ldw);
            const std::vector<Part> parts = parts_of(s, P, K, ldw);
            for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
            const int64_t shape[3] = {P, K, ldw};
            report("pma_staging", parts, buf, size, sizeof(s) / sizeof(void*), shape, 3);
            delete[] buf;
        }
    }
    return 0;
}
