// draws_layout_check.cpp — every layout of csrc/draws/octo_draws_layout.h on host memory (tests/test_draws_layout.py compiles this with
// -fsanitize=address,undefined and runs it). For each layout and shape: size it with a null base, allocate exactly that many doubles,
// lay the parts out, fill every element of every part with the part's own tag, read all of them back, and print one JSON line with the
// size, the number of pointers in the struct and each part's offset, element size, length and position in the struct. The lengths are stated here, not taken from the header.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "octo_draws_layout.h"

struct Part {
    const char* name;
    void* p;
    size_t elem;        // bytes of an element
    int64_t len;        // elements
    size_t member;      // offsetof the pointer in the layout's struct
};

#define PART(s, m, len) Part{#m, (void*)(s).m, sizeof(*(s).m), (len), offsetof(std::remove_cv_t<std::remove_reference_t<decltype(s)>>, m)}

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

static void report(const char* layout, std::vector<int64_t> shape, int64_t size, size_t members, const double* base, const std::vector<Part>& parts) {
    for (size_t k = 0; k < parts.size(); ++k) fill(parts[k], (int)k + 1);
    std::printf("{\"layout\": \"%s\", \"shape\": [", layout);
    for (size_t k = 0; k < shape.size(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)shape[k]);
    std::printf("], \"size\": %lld, \"members\": %zu, \"parts\": [", (long long)size, members);
    for (size_t k = 0; k < parts.size(); ++k) {
        const Part& q = parts[k];
        const bool ok = holds(q, (int)k + 1);
        std::printf("%s{\"name\": \"%s\", \"offset\": %lld, \"elem\": %zu, \"len\": %lld, \"member\": %zu, \"tag_ok\": %s}", k ? ", " : "", q.name,
                    (long long)((const char*)q.p - (const char*)base), q.elem, (long long)q.len, q.member, ok ? "true" : "false");
    }
    std::printf("]}\n");
}

// size with a null base (which must hand out null pointers), then the parts on exactly that many doubles
#define RUN(name, fn, shape_list, parts_of, ...)                                        \
    do {                                                                                \
        const int64_t size = carve_size(fn, __VA_ARGS__);                               \
        const auto none = carve_at(nullptr, fn, __VA_ARGS__);                           \
        for (const Part& q : parts_of(none)) if (q.p) return 2;                         \
        double* buf = new double[size];                                                 \
        const auto s = carve_at(buf, fn, __VA_ARGS__);                                  \
        report(name, shape_list, size, sizeof(s) / sizeof(void*), buf, parts_of(s));                            \
        delete[] buf;                                                                   \
    } while (0)

int main() {
    const int64_t shapes[3][3] = {{1, 1, 1}, {3, 5, 2}, {64, 7, 8}};      // (D, ld, m) of the ten layouts of the optimisers, the HMC step and the drivers
    for (const auto& sh : shapes) {
        const int64_t D = sh[0], ld = sh[1], m = sh[2], plane = D * ld, KW = 5 * ld, P = D * (D + 1) / 2;
        const std::vector<int64_t> dlm = {D, ld, m}, dl = {D, ld};
        auto lbfgs = [&](const LbfgsState& s) {
            return std::vector<Part>{PART(s, trial, plane), PART(s, g, plane), PART(s, dir, plane), PART(s, alpha, plane), PART(s, glp, plane),
                                     PART(s, S, m * plane), PART(s, Y, m * plane), PART(s, sy, m * ld), PART(s, coef, m * ld),
                                     PART(s, lp, ld), PART(s, f, ld), PART(s, t, ld), PART(s, gd, ld), PART(s, gn, ld),
                                     PART(s, status, ld), PART(s, iters, ld), PART(s, evals, ld), PART(s, nbt, ld), PART(s, cnt, ld), PART(s, head, ld)};
        };
        RUN("lbfgs_state", lbfgs_state, dlm, lbfgs, D, ld, m);
        auto coef = [&](const LbfgsCoef& s) { return std::vector<Part>{PART(s, sy, m * ld), PART(s, coef, m * ld)}; };
        RUN("lbfgs_coef", lbfgs_coef, dlm, coef, ld, m);
        auto pf = [&](const PfState& s) {
            return std::vector<Part>{PART(s, mu, 2 * plane), PART(s, sqa, 2 * plane), PART(s, chol, 2 * P * ld), PART(s, logdet, 2 * ld), PART(s, elbo, ld),
                                     PART(s, slot, ld), PART(s, elbo_iter, ld), PART(s, n_fits, ld), PART(s, prev_iters, ld), PART(s, fresh, ld)};
        };
        RUN("pf_state", pf_state, dl, pf, D, ld);
        auto batch = [&](const PfBatch& s) { return std::vector<Part>{PART(s, phi, D * KW), PART(s, lp, KW), PART(s, logq, KW)}; };
        RUN("pf_batch", pf_batch, (std::vector<int64_t>{D, KW}), batch, D, KW);
        auto hmc = [&](const HmcWork& s) {
            return std::vector<Part>{PART(s, q, plane), PART(s, p, plane), PART(s, gpr, plane), PART(s, glp, plane),
                                     PART(s, lp, ld), PART(s, lp0, ld), PART(s, lpt0, ld), PART(s, K0, ld)};
        };
        RUN("hmc_work", hmc_work, dl, hmc, D, ld);
        auto lst = [&](const LbfgsStaging& s) {
            return std::vector<Part>{PART(s, theta_t, plane), PART(s, inv_hess_diag, plane), PART(s, lp, ld), PART(s, gn, ld),
                                     PART(s, status, ld), PART(s, iters, ld), PART(s, evals, ld), PART(s, inv_mass, D)};
        };
        RUN("lbfgs_staging", lbfgs_staging, dl, lst, D, ld);
        auto hst = [&](const HmcStaging& s) {
            return std::vector<Part>{PART(s, theta_t, plane), PART(s, theta_prop, plane), PART(s, beta, ld), PART(s, eps, ld), PART(s, lp, ld),
                                     PART(s, ll, ld), PART(s, dH, ld), PART(s, accepted, ld), PART(s, inv_mass, D)};
        };
        RUN("hmc_staging", hmc_staging, dl, hst, D, ld);
        // the drivers' groups, with ld draws to a chunk, m candidates in the lists, ld draws in m blocks
        auto chunk = [&](const ChunkBufs& s) {
            return std::vector<Part>{PART(s, tt, D * ld), PART(s, lpt, ld), PART(s, clp, m), PART(s, cix, m), PART(s, max, 1)};
        };
        RUN("chunk_bufs", chunk_bufs, dlm, chunk, D, ld, m);
        auto arr = [&](const DrawArrays& s) { return std::vector<Part>{PART(s, lp, ld), PART(s, ll, ld), PART(s, pmax, m), PART(s, cnt, m + 1)}; };
        RUN("draw_arrays", draw_arrays, (std::vector<int64_t>{ld, m}), arr, ld, m);
        auto out = [&](const Outputs& s) { return std::vector<Part>{PART(s, ix, ld), PART(s, ll, ld), PART(s, lp, ld), PART(s, theta, D * ld)}; };
        RUN("outputs", outputs, dl, out, D, ld);
    }
    const int64_t moment_shapes[4][3] = {{1, 1, 1}, {3, 5, 2}, {7, 64, 64}, {4, 3, 11}};      // (nblk, G, K): the block partials of the grouped moments
    for (const auto& sh : moment_shapes) {
        const int64_t nblk = sh[0], G = sh[1], K = sh[2];
        auto mom = [&](const MomentsPartials& s) { return std::vector<Part>{PART(s, cnt, nblk * G), PART(s, sum, nblk * G * K), PART(s, m2, nblk * G * K)}; };
        RUN("moments_partials", moments_partials, (std::vector<int64_t>{nblk, G, K}), mom, nblk, G, K);
    }
    const int64_t nuts_shapes[5][3] = {{1, 1, 1}, {14, 72, 4}, {5, 65536, 5}, {64, 3, 10}, {3, 257, 2}};      // (D, ld, max_depth): the trees of a NUTS transition
    for (const auto& sh : nuts_shapes) {
        const int64_t D = sh[0], ld = sh[1], md = sh[2], plane = D * ld;
        auto tree = [&](const NutsWork& s) {
            return std::vector<Part>{
                PART(s, trial, plane), PART(s, pt, plane), PART(s, qL, plane), PART(s, pL, plane), PART(s, gL, plane), PART(s, qR, plane), PART(s, pR, plane),
                PART(s, gR, plane), PART(s, prop, plane), PART(s, sprop, plane), PART(s, rho, plane), PART(s, rho_s, plane), PART(s, gpr, plane), PART(s, glp, plane),
                PART(s, ck_p, md * plane), PART(s, ck_r, md * plane),
                PART(s, lp, ld), PART(s, H0, ld), PART(s, logw, ld), PART(s, logw_s, ld), PART(s, sum_acc, ld), PART(s, prop_lp, ld), PART(s, prop_lpt, ld),
                PART(s, sprop_lp, ld), PART(s, sprop_lpt, ld), PART(s, out_lp, ld), PART(s, out_lpt, ld),
                PART(s, status, ld), PART(s, depth, ld), PART(s, n, ld), PART(s, nleaf, ld), PART(s, v, ld), PART(s, sel, ld), PART(s, ssel, ld)};
        };
        RUN("nuts_work", nuts_work, (std::vector<int64_t>{D, ld, md}), tree, D, ld, md);
    }
    return 0;
}
