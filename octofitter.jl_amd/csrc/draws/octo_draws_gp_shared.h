// octo_draws_gp_shared.h — what the two units of the Gaussian-process RV term share: octo_draws_gp.hip (the table, the row-parallel passes, the celerite
// recursion, the C ABI) and octo_draws_gpd.hip (the dense kernels: one workgroup a walker). The kernels' argument block, the row record, and the one
// function the first unit calls in the second. Included once by each of the two units, after nothing: it brings octo_draws_common.h itself.
#pragma once
#include "octo_draws_common.h"

namespace gp_dev {      // the companions' device routines under a name of their own: that header and octo_draws_common.h both define a wave_sum
#include "octo_companion_device.h"
}

namespace {

constexpr int GP_ROWS = OCTO_DRAWS_SCAN_ROWS, GP_K = OCTO_DRAWS_GP_MAX_K, GP_J = OCTO_DRAWS_GP_MAX_TERMS, GP_S = OCTO_DRAWS_GP_MAX_SLOTS, GP_G = OCTO_DRAWS_GP_SEGMENT;
constexpr int GROWW = 8;                       // a row record: {t, rv, σ², c[4] (0 behind K), 0}
constexpr int GP_PL = 6;                       // a planet's sums in the work array: GE, GM, GT, GC, GK, GW

struct GpArgs {
    const double* rows;            // [n][GROWW]
    int32_t n, K, P, J, H, accumulate, n_tasks, n_sums, n_seg;
    int32_t term[GP_J], slot[GP_S];
    int32_t orbit_kind[MAXP], has_mass[MAXP];
    DevConsts c;
    const double* elems; int64_t ld, W, ldw;
    const double *hyper, *beta, *jitter;      // [H][ld], [K][ld] or null, [W] or null
    GpWork k;
    double* tri;                   // the dense route's packed triangles [W][n(n+1)/2] of a table with more than OCTO_DRAWS_GP_DENSE_LDS_ROWS rows, or null
    double *ll, *g_elems, *g_hyper, *g_beta, *g_jitter;
    double *eta, *mu; int64_t ld_out;
};

inline bool gp_dense_kind(int kind) { return kind >= OCTO_DRAWS_GP_SE && kind <= OCTO_DRAWS_GP_QUASIPERIODIC; }
inline int gp_dense_n_hyper(int kind) { return kind == OCTO_DRAWS_GP_QUASIPERIODIC ? 4 : (kind == OCTO_DRAWS_GP_PERIODIC ? 3 : 2); }

}  // namespace

// octo_draws_gpd.hip: the dense kernels between k_gp_rows and k_gp_adj on st — ℓ, the validity, α over r (want_alpha), ∂ℓ/∂hyper and ∂ℓ/∂s where a.g_hyper or
// a.g_jitter is set — and what octo_draws_gp_set asks of the device for a dense table of n rows (the workgroup's LDS).
OCTO_DRAWS_INTERNAL int draws_gpd_launch(octo_draws* h, hipStream_t st, const void* gp_args, bool want_ll, bool want_alpha);
OCTO_DRAWS_INTERNAL int draws_gpd_prepare(octo_draws* h, int64_t n);
