// octo_draws_program.hip — liboctofitter_hip_draws.so: derived variables as expression programs (include/octofitter_hip_draws.h, "Derived
// variables"). The reference's @variables block produces a short straight-line list of arithmetic on θ; that list is data, and this unit is
// its interpreter on the device, forward and reverse, so that every ℓπ consumer of the handle (logpost_at, octo_draws_common.h) runs on models
// with derived variables with θ_t, the elements and the gradient staying in HBM. A client of the public ABI like the rest of the library: ℓ and
// ∂ℓ/∂(elements, nuisances) come from octo_eval_device; of the main library's sources it includes the device routines of octo_model.h
// (prior_link_lanes, prior_density_lanes, tperi_campbell), so the prior part and tp are the code the model callback runs.
//
//   k_prog_fwd<GRAD>   lane = walker, one wave a block. Link and logpdf_with_trans of every prior, then the ops in order: the op list is the same
//                      for every lane, so the opcode is read with scalar loads and dispatched with a scalar branch — a wave never diverges on
//                      the program. Node values live in LDS [node][64] (512 B a node; dynamic, sized by the program); with GRAD they are
//                      streamed to the work array as well, lane-contiguous. Then the inputs (a TPERI binding: tperi_campbell) and Σ terms.
//   k_prog_values      the same forward sweep, the chosen nodes written out.
//   k_prog_bwd         ADJOINTS live in LDS, zeroed, then seeded by the inputs' gradient and the terms; the ops in reverse, operand VALUES read
//                      back from the work array (those loads are not on the dependent chain, only the adjoint updates are). No atomics: a lane
//                      owns its column. Then ∂x/∂θ_t, the prior gradient and the finiteness rules of k_model_bwd.
// Measured and not kept: the values staged into LDS beside the adjoints ahead of the reverse sweep, and the next op fetched while the
// current one runs — neither moved the callback's time (tools/program_bench.py: both kernels sit at ~20 µs, a launch and one wave's chain).
#include "octo_draws_common.h"

namespace {

constexpr int TP_SLOTS = 7;      // a TPERI binding's gradient: the angle, then these six element slots
__device__ constexpr int TP_EL[6] = {OCTO_EL_A, OCTO_EL_E, OCTO_EL_I, OCTO_EL_W, OCTO_EL_O, OCTO_EL_M};
constexpr int TP_EL_HOST[6] = {OCTO_EL_A, OCTO_EL_E, OCTO_EL_I, OCTO_EL_W, OCTO_EL_O, OCTO_EL_M};

struct ProgArgs {
    const octo_prior* priors;      // [D] the handle's OWN table
    const double* pc;              // [D][PRIOR_NC]
    const octo_draws_op* ops;      // [n_ops]
    const octo_draws_bind* binds;  // [n_in]
    const int32_t* terms;          // [n_terms]
    int32_t D, n_ops, n_in, n_terms;
    const double* theta_t; int64_t ld, W, ldw;
    ProgWork k;
    double k_yr;
    double* lp_out; double* grad_out;      // k_prog_bwd
};

struct ValuesArgs {
    ProgArgs p;
    double* out; int64_t ld_out;
    int32_t n;
    uint8_t nodes[256];
};

// x_d, the prior part and the node values of this lane's walker into its LDS column L[node·64 + lane]. Every lane of the wave runs it
// (prior_density_lanes votes across the wave), a lane beyond the batch with the last walker's column. Returns whether every θ_t entry is finite.
template <bool GRAD>
__device__ __forceinline__ bool prog_forward(const ProgArgs& a, double* __restrict__ L, int lane, int64_t w, int64_t wl, bool live, double& prior, bool& healed) {
    const int D = a.D;
    bool fin = true;
    prior = 0.0; healed = false;
    for (int d = 0; d < D; ++d) {
        const octo_prior pr = a.priors[d];
        const double y = a.theta_t[(int64_t)d * a.ld + wl];
        fin = fin && isfinite(y);
        double xv, xd, pv, pd;
        prior_link_lanes(pr, y, xv, xd);
        prior_density_lanes(pr, xv, xd, pv, pd, a.pc + PRIOR_NC * d);
        healed = healed || !isfinite(pv);
        prior += pv;
        L[d * WAVE + lane] = xv;
        if constexpr (GRAD) {
            if (live) { a.k.vals[(int64_t)d * a.ldw + w] = xv; a.k.dx[(int64_t)d * a.ldw + w] = xd; a.k.gpd[(int64_t)d * a.ldw + w] = pd; }
        }
    }
    prior = healed ? HEALED : prior;
    for (int j = 0; j < a.n_ops; ++j) {
        const octo_draws_op op = a.ops[j];      // the same for every lane: scalar loads, a scalar branch
        const double va = L[op.a * WAVE + lane], vb = L[op.b * WAVE + lane];
        double r;
        switch (op.op) {
        case OCTO_DRAWS_OP_CONST: r = op.value; break;
        case OCTO_DRAWS_OP_ADD: r = va + vb; break;
        case OCTO_DRAWS_OP_SUB: r = va - vb; break;
        case OCTO_DRAWS_OP_MUL: r = va * vb; break;
        case OCTO_DRAWS_OP_DIV: r = va / vb; break;
        case OCTO_DRAWS_OP_NEG: r = -va; break;
        case OCTO_DRAWS_OP_SQRT: r = sqrt(va); break;
        case OCTO_DRAWS_OP_CBRT: r = cbrt(va); break;
        case OCTO_DRAWS_OP_EXP: r = exp(va); break;
        case OCTO_DRAWS_OP_LOG: r = log(va); break;
        case OCTO_DRAWS_OP_SIN: r = sin(va); break;
        case OCTO_DRAWS_OP_COS: r = cos(va); break;
        case OCTO_DRAWS_OP_ATAN2: r = atan2(va, vb); break;
        case OCTO_DRAWS_OP_POWC: r = pow(va, op.value); break;
        case OCTO_DRAWS_OP_MULC: r = va * op.value; break;
        default: r = va + op.value; break;      // OCTO_DRAWS_OP_ADDC: octo_draws_program_set admits no other
        }
        L[(D + j) * WAVE + lane] = r;
        if constexpr (GRAD) {
            if (live) a.k.vals[(int64_t)(D + j) * a.ldw + w] = r;
        }
    }
    return fin;
}

template <bool GRAD>
__global__ __launch_bounds__(WAVE) void k_prog_fwd(ProgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double L[];      // [N][64] node values
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = w < a.W;
    const int64_t wl = live ? w : a.W - 1;
    double prior;
    bool healed;
    const bool fin = prog_forward<GRAD>(a, L, lane, w, wl, live, prior, healed);
    for (int k = 0; k < a.n_in; ++k) {
        const octo_draws_bind b = a.binds[k];
        double v = L[b.node * WAVE + lane];
        if ((b.kind & 0xFFFF) == OCTO_DRAWS_BIND_TPERI) {
            const int p = k / OCTO_N_EL;      // a TPERI binding sits on the TP slot of an element row: octo_draws_program_set
            double el[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) el[q] = L[a.binds[p * OCTO_N_EL + TP_EL[q]].node * WAVE + lane];
            double g[OCTO_N_EL], g_theta = 0.0;
            v = tperi_campbell<GRAD>(v, b.value, el[5], el[1], el[0], el[2], el[3], el[4], a.k_yr, g, g_theta);
            if constexpr (GRAD) {
                if (live) {
                    double* o = a.k.gtp + (int64_t)p * TP_SLOTS * a.ldw + w;
                    o[0] = g_theta;
#pragma unroll
                    for (int q = 0; q < 6; ++q) o[(int64_t)(q + 1) * a.ldw] = g[TP_EL[q]];
                }
            }
        }
        if (live) a.k.inputs[(int64_t)k * a.ldw + w] = v;
    }
    double t = 0.0;
    for (int i = 0; i < a.n_terms; ++i) t += L[a.terms[i] * WAVE + lane];
    if (live) {
        a.k.pp[w] = fin ? prior + t : -INFINITY;
        a.k.healed[w] = healed ? 1 : 0;
    }
}

__global__ __launch_bounds__(WAVE) void k_prog_values(ValuesArgs v) {
    extern __shared__ __attribute__((aligned(16))) double L[];
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = w < v.p.W;
    const int64_t wl = live ? w : v.p.W - 1;
    double prior;
    bool healed;
    (void)prog_forward<false>(v.p, L, lane, w, wl, live, prior, healed);
    if (!live) return;
    for (int k = 0; k < v.n; ++k) v.out[(int64_t)k * v.ld_out + w] = L[(int)v.nodes[k] * WAVE + lane];
}

// lp = isfinite(pp) ? pp + ℓ : pp, NaN -> −Inf (k_model_bwd); with a gradient: the reverse sweep
__global__ __launch_bounds__(WAVE) void k_prog_bwd(ProgArgs a) {
    extern __shared__ __attribute__((aligned(16))) double A[];      // [N][64] adjoints
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    if (w >= a.W) return;      // nothing below votes across the wave
    const double pp = a.k.pp[w];
    double lp = isfinite(pp) ? pp + a.k.ll[w] : pp;
    if (isnan(lp)) lp = -INFINITY;
    a.lp_out[w] = lp;
    if (!a.grad_out) return;
    const int D = a.D, N = D + a.n_ops;
    for (int n = 0; n < N; ++n) A[n * WAVE + lane] = 0.0;
    for (int k = 0; k < a.n_in; ++k) {
        const octo_draws_bind b = a.binds[k];
        const double g = a.k.g_in[(int64_t)k * a.ldw + w];
        if ((b.kind & 0xFFFF) == OCTO_DRAWS_BIND_TPERI) {
            const int p = k / OCTO_N_EL;
            const double* o = a.k.gtp + (int64_t)p * TP_SLOTS * a.ldw + w;
            A[b.node * WAVE + lane] += g * o[0];
#pragma unroll
            for (int q = 0; q < 6; ++q) A[a.binds[p * OCTO_N_EL + TP_EL[q]].node * WAVE + lane] += g * o[(int64_t)(q + 1) * a.ldw];
        } else {
            A[b.node * WAVE + lane] += g;
        }
    }
    for (int i = 0; i < a.n_terms; ++i) A[a.terms[i] * WAVE + lane] += 1.0;
    const double* __restrict__ V = a.k.vals + w;
    for (int j = a.n_ops - 1; j >= 0; --j) {
        const octo_draws_op op = a.ops[j];
        const double adj = A[(D + j) * WAVE + lane];
        const double va = V[(int64_t)op.a * a.ldw], vb = V[(int64_t)op.b * a.ldw], r = V[(int64_t)(D + j) * a.ldw];
        double* Aa = A + op.a * WAVE + lane;
        double* Ab = A + op.b * WAVE + lane;      // may be Aa: every update below is a read-modify-write of its own
        switch (op.op) {
        case OCTO_DRAWS_OP_CONST: break;
        case OCTO_DRAWS_OP_ADD: *Aa += adj; *Ab += adj; break;
        case OCTO_DRAWS_OP_SUB: *Aa += adj; *Ab -= adj; break;
        case OCTO_DRAWS_OP_MUL: *Aa += adj * vb; *Ab += adj * va; break;
        case OCTO_DRAWS_OP_DIV: { const double q = adj / vb; *Aa += q; *Ab -= q * r; break; }
        case OCTO_DRAWS_OP_NEG: *Aa -= adj; break;
        case OCTO_DRAWS_OP_SQRT: *Aa += adj * (0.5 / r); break;
        case OCTO_DRAWS_OP_CBRT: *Aa += adj / (3.0 * r * r); break;
        case OCTO_DRAWS_OP_EXP: *Aa += adj * r; break;
        case OCTO_DRAWS_OP_LOG: *Aa += adj / va; break;
        case OCTO_DRAWS_OP_SIN: *Aa += adj * cos(va); break;
        case OCTO_DRAWS_OP_COS: *Aa -= adj * sin(va); break;
        case OCTO_DRAWS_OP_ATAN2: { const double ih = adj / (va * va + vb * vb); *Aa += vb * ih; *Ab -= va * ih; break; }
        case OCTO_DRAWS_OP_POWC: *Aa += adj * (op.value * pow(va, op.value - 1.0)); break;
        case OCTO_DRAWS_OP_MULC: *Aa += adj * op.value; break;
        default: *Aa += adj; break;      // OCTO_DRAWS_OP_ADDC
        }
    }
    const bool healed = a.k.healed[w] != 0, ok = isfinite(lp);
    for (int d = 0; d < D; ++d) {
        const double g = fma(A[d * WAVE + lane], a.k.dx[(int64_t)d * a.ldw + w], healed ? 0.0 : a.k.gpd[(int64_t)d * a.ldw + w]);
        a.grad_out[(int64_t)d * a.ld + w] = ok ? g : 0.0;
    }
}

inline size_t prog_lds(const octo_draws* h) { return (size_t)(h->D + h->prog_n_ops) * WAVE * sizeof(double); }

int check_program_call(octo_draws* h, const char* who, const double* d_theta_t, int64_t ld, int64_t W) {
    if (!h->prog_ops || !h->ctx) return fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no program (octo_draws_program_set)");
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    return W == 0 || d_theta_t ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": d_theta_t is NULL");
}

ProgArgs program_args(const octo_draws* h, const double* d_theta_t, int64_t ld, int64_t W, int64_t ldw) {
    ProgArgs a;
    std::memset(&a, 0, sizeof(a));
    a.priors = h->own_priors; a.pc = h->own_pc; a.ops = h->prog_ops; a.binds = h->prog_binds; a.terms = h->prog_terms;
    a.D = h->D; a.n_ops = h->prog_n_ops; a.n_in = h->prog_n_in; a.n_terms = h->prog_n_terms;
    a.theta_t = d_theta_t; a.ld = ld; a.W = W; a.ldw = ldw; a.k_yr = h->prog_k_yr;
    if (h->scan_bound) {      // a bound scan table (octo_draws_scan.hip): the nodes it reads are input rows behind the program's own
        a.binds = (const octo_draws_bind*)h->d_scan_binds; a.n_in += h->scan_n_bind;
    } else if (h->pma_bound) {      // … or a bound catalogue table (octo_draws_pma.hip), the same way: one bound table a handle
        a.binds = (const octo_draws_bind*)h->d_pma_binds; a.n_in += h->pma_n_bind;
    } else if (h->gp_bound) {       // … or a bound Gaussian-process RV table (octo_draws_gp.hip)
        a.binds = (const octo_draws_bind*)h->d_gp_binds; a.n_in += h->gp_n_bind;
    }
    return a;
}

}  // namespace

extern "C" {

int32_t octo_draws_program_clear(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    h->prog_ops = nullptr; h->prog_binds = nullptr; h->prog_terms = nullptr; h->prog_ds = nullptr;
    h->prog_n_ops = h->prog_n_in = h->prog_n_el = h->prog_n_terms = h->prog_planets = 0;
    h->scan_bound = 0; h->scan_n_bind = 0;      // a bound scan table names this program's nodes
    h->pma_bound = 0; h->pma_n_bind = 0;        // … and so does a bound catalogue table
    h->gp_bound = 0; h->gp_n_bind = 0;          // … and a bound Gaussian-process RV table
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->pf_W = 0; h->de_open = false;      // a transition is never resumed on another target
    return OCTO_OK;
}

int32_t octo_draws_program_set(octo_draws* h, const octo_dataset* ds, int32_t n_planets, int32_t n_obs, const octo_draws_op* ops, int32_t n_ops,
                               const octo_draws_bind* binds, int32_t n_binds, const int32_t* terms, int32_t n_terms) {
    const std::string who = "octo_draws_program_set: ";
    if (!h) return OCTO_EINVAL;
    if (h->model) return fail(h, OCTO_EINVAL, who + "the handle has a model: a program goes on a handle created with a context and without one");
    if (!h->ctx) return fail(h, OCTO_EINVAL, who + "the handle has no context");
    if (!ds || !binds || (n_ops > 0 && !ops) || (n_terms > 0 && !terms)) return fail(h, OCTO_EINVAL, who + "null argument");
    if (n_planets < 1 || n_obs < 0 || n_ops < 0 || n_terms < 0) return fail(h, OCTO_EINVAL, who + "need n_planets >= 1 and n_obs, n_ops, n_terms >= 0");
    if (n_ops > OCTO_DRAWS_PROGRAM_MAX_OPS) return fail(h, OCTO_ENOTSUP, who + std::to_string(n_ops) + " ops: more than OCTO_DRAWS_PROGRAM_MAX_OPS");
    const int64_t n_el = (int64_t)n_planets * OCTO_N_EL, n_in = n_el + (int64_t)n_obs * OCTO_N_NUIS;
    if (n_binds != n_in)
        return fail(h, OCTO_EINVAL, who + std::to_string(n_binds) + " bindings: need n_planets*OCTO_N_EL + n_obs*OCTO_N_NUIS = " + std::to_string(n_in));
    const int D = h->D, N = D + n_ops;
    for (int j = 0; j < n_ops; ++j) {
        const octo_draws_op& op = ops[j];
        const std::string opj = who + "op " + std::to_string(j) + ": ";
        if (op.op < 0 || op.op >= OCTO_DRAWS_N_OPS) return fail(h, OCTO_EINVAL, opj + "unknown opcode " + std::to_string(op.op));
        const bool binary = (op.op >= OCTO_DRAWS_OP_ADD && op.op <= OCTO_DRAWS_OP_DIV) || op.op == OCTO_DRAWS_OP_ATAN2;
        const bool reads_a = op.op != OCTO_DRAWS_OP_CONST;
        // an operand the op does not read is still an LDS address of the sweep: it must be a node too
        if (op.a < 0 || op.a >= (reads_a ? D + j : N) || op.b < 0 || op.b >= (binary ? D + j : N))
            return fail(h, OCTO_EINVAL, opj + "operands (" + std::to_string(op.a) + ", " + std::to_string(op.b) + ") must be earlier nodes, below " + std::to_string(D + j) + " (forward reference)");
    }
    for (int k = 0; k < n_binds; ++k) {
        const octo_draws_bind& b = binds[k];
        const std::string bk = who + "binding " + std::to_string(k) + ": ";
        const int kind = b.kind & 0xFFFF;
        if ((kind != OCTO_DRAWS_BIND_NODE && kind != OCTO_DRAWS_BIND_TPERI) || (b.kind & ~(0xFFFF | OCTO_DRAWS_BIND_FLAG_TI)) != 0)
            return fail(h, OCTO_EINVAL, bk + "unknown kind " + std::to_string(b.kind));
        if (b.node < 0 || b.node >= N) return fail(h, OCTO_EINVAL, bk + "node " + std::to_string(b.node) + " out of range");
        if (kind != OCTO_DRAWS_BIND_TPERI) continue;
        if (k >= n_el || k % OCTO_N_EL != OCTO_EL_TP) return fail(h, OCTO_EINVAL, bk + "a TPERI binding goes on the OCTO_EL_TP slot of a planet");
        if (b.kind & OCTO_DRAWS_BIND_FLAG_TI) return fail(h, OCTO_ENOTSUP, bk + "a TPERI binding on a Thiele-Innes planet is not on the program path");
        for (int q = 0; q < 6; ++q) {
            const int s = (k / OCTO_N_EL) * OCTO_N_EL + TP_EL_HOST[q];
            if ((binds[s].kind & 0xFFFF) != OCTO_DRAWS_BIND_NODE) return fail(h, OCTO_EINVAL, bk + "slot " + std::to_string(TP_EL_HOST[q]) + " of its planet must be a NODE binding");
        }
    }
    for (int i = 0; i < n_terms; ++i)
        if (terms[i] < 0 || terms[i] >= N) return fail(h, OCTO_EINVAL, who + "term " + std::to_string(i) + ": node " + std::to_string(terms[i]) + " out of range");
    octo_consts cst;
    if (octo_consts_default(&cst) != OCTO_OK) return fail(h, OCTO_EINVAL, who + "octo_consts_default failed");
    OCHK(h, hipSetDevice(h->device));
    const size_t lds = (size_t)N * WAVE * sizeof(double);
    if (lds > 48 * 1024) {      // beyond the default limit: raised once per program, for the four kernels
        for (const void* fn : {(const void*)k_prog_fwd<true>, (const void*)k_prog_fwd<false>, (const void*)k_prog_values, (const void*)k_prog_bwd})
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, OCTO_ENOTSUP, who + "the program needs more LDS per block than this device gives (512 B a node)");
            }
    }
    // the tables in one allocation: ops (24 B each), binds (16 B), terms (4 B) — every part starts on an 8-byte boundary
    const size_t b_ops = sizeof(octo_draws_op) * (size_t)n_ops, b_binds = sizeof(octo_draws_bind) * (size_t)n_binds, b_terms = sizeof(int32_t) * (size_t)n_terms;
    octo_draws_program_clear(h);
    OCHK(h, hipStreamSynchronize(h->stream));
    if (h->d_prog_tab) { OCHK(h, hipFree(h->d_prog_tab)); h->d_prog_tab = nullptr; }
    OCHK(h, hipMalloc(&h->d_prog_tab, b_ops + b_binds + b_terms + 8));
    char* base = (char*)h->d_prog_tab;
    if (b_ops) OCHK(h, hipMemcpy(base, ops, b_ops, hipMemcpyHostToDevice));
    OCHK(h, hipMemcpy(base + b_ops, binds, b_binds, hipMemcpyHostToDevice));
    if (b_terms) OCHK(h, hipMemcpy(base + b_ops + b_binds, terms, b_terms, hipMemcpyHostToDevice));
    h->prog_ops = (const octo_draws_op*)base; h->prog_binds = (const octo_draws_bind*)(base + b_ops); h->prog_terms = (const int32_t*)(base + b_ops + b_binds);
    h->prog_n_ops = n_ops; h->prog_n_in = (int32_t)n_in; h->prog_n_el = (int32_t)n_el; h->prog_n_terms = n_terms; h->prog_planets = n_planets;
    h->prog_ds = ds; h->prog_k_yr = cst.kepler_year_to_julian_day;
    return OCTO_OK;
}

int32_t octo_draws_program_logpost_device(octo_draws* h, const double* d_theta_t, int64_t ld, int64_t W, double* d_lp, double* d_grad, void* hip_stream) {
    const char* who = "octo_draws_program_logpost_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_program_call(h, who, d_theta_t, ld, W)) return rc;
    if (W == 0) return OCTO_OK;
    if (!d_lp) return fail(h, OCTO_EINVAL, std::string(who) + ": d_lp is NULL");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    ProgArgs a = program_args(h, d_theta_t, ld, W, ldw);
    if (int rc = grow_to(h, h->d_prog, h->cap_prog, a.k, prog_work, (int64_t)h->D, (int64_t)(h->D + h->prog_n_ops), (int64_t)a.n_in, (int64_t)h->prog_planets, ldw)) return rc;
    a.lp_out = d_lp; a.grad_out = d_grad;
    const dim3 grid((unsigned)(ldw / WAVE)), block(WAVE);
    const size_t lds = prog_lds(h);
    if (d_grad) hipLaunchKernelGGL(k_prog_fwd<true>, grid, block, lds, st, a);
    else hipLaunchKernelGGL(k_prog_fwd<false>, grid, block, lds, st, a);
    OCHK(h, hipGetLastError());
    const int n_el = h->prog_n_el, n_nu = h->prog_n_in - n_el;
    if (int rc = main_call(h, octo_eval_device(h->ctx, h->prog_ds, a.k.inputs, n_nu ? a.k.inputs + (int64_t)n_el * ldw : nullptr, ldw, W, a.k.ll,
                                               d_grad ? a.k.g_in : nullptr, d_grad && n_nu ? a.k.g_in + (int64_t)n_el * ldw : nullptr, (void*)st), "octo_eval_device")) return rc;
    if (h->scan_bound)      // ℓ_scan into ℓ, its adjoints into g_in: on the likelihood side of the split, ahead of the reverse sweep
        if (int rc = draws_scan_accumulate(h, st, a.k.inputs, d_grad ? a.k.g_in : nullptr, a.k.ll, ldw, W, h->prog_n_in)) return rc;
    if (h->pma_bound)       // ℓ_pma likewise (octo_draws_pma.hip)
        if (int rc = draws_pma_accumulate(h, st, a.k.inputs, d_grad ? a.k.g_in : nullptr, a.k.ll, ldw, W, h->prog_n_in)) return rc;
    if (h->gp_bound)        // ℓ_gp likewise (octo_draws_gp.hip)
        if (int rc = draws_gp_accumulate(h, st, a.k.inputs, d_grad ? a.k.g_in : nullptr, a.k.ll, ldw, W, h->prog_n_in)) return rc;
    hipLaunchKernelGGL(k_prog_bwd, grid, block, d_grad ? lds : 0, st, a);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_program_values_device(octo_draws* h, const double* d_theta_t, int64_t ld, int64_t W, const int32_t* nodes, int32_t n, double* d_out,
                                         int64_t ld_out, void* hip_stream) {
    const char* who = "octo_draws_program_values_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_program_call(h, who, d_theta_t, ld, W)) return rc;
    if (n < 0 || n > 256 || (n > 0 && !nodes)) return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= n <= 256 node indices");
    if (ld_out < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need ld_out >= W");
    ValuesArgs v;
    std::memset(&v, 0, sizeof(v));
    const int N = h->D + h->prog_n_ops;
    for (int k = 0; k < n; ++k) {
        if (nodes[k] < 0 || nodes[k] >= N) return fail(h, OCTO_EINVAL, std::string(who) + ": node " + std::to_string(nodes[k]) + " out of range");
        v.nodes[k] = (uint8_t)nodes[k];
    }
    if (W == 0 || n == 0) return OCTO_OK;
    if (!d_out) return fail(h, OCTO_EINVAL, std::string(who) + ": d_out is NULL");
    OCHK(h, hipSetDevice(h->device));
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    v.p = program_args(h, d_theta_t, ld, W, ldw);
    v.out = d_out; v.ld_out = ld_out; v.n = n;
    hipLaunchKernelGGL(k_prog_values, dim3((unsigned)(ldw / WAVE)), dim3(WAVE), prog_lds(h), stream_of(h, hip_stream), v);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // extern "C"
