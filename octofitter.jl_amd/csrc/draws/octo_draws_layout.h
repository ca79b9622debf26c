// octo_draws_layout.h — how every work allocation of liboctofitter_hip_draws.so is cut into its parts. One function per layout hands out
// the parts from a Carve in the order its struct declares them; the same function sizes the allocation (a null base only counts) and
// places the pointers, so the two cannot disagree, and a unit that reads another's state (Pathfinder, the L-BFGS's) calls that state's
// function. Plain host C++ on <cstdint> alone: it compiles and is tested by itself (tests/test_draws_layout.py).
#pragma once

#include <cstdint>

// Hands out consecutive parts of `base`, counted in doubles. A part of 4-byte elements takes a double's room per element — the rule
// include/octofitter_hip_draws.h documents — so every part starts on an 8-byte boundary whatever precedes it.
struct Carve {
    double* base;          // null: size only
    int64_t used = 0;      // doubles handed out so far
    template <class T = double>
    T* take(int64_t n) {
        static_assert(sizeof(T) == 8 || sizeof(T) == 4, "a part holds 8-byte elements, or 4-byte ones in a double's room each");
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;      // no pointer is formed from a null base
        used += n;
        return p;
    }
};

// the doubles of layout(c, args…) · its parts on base. The functions below return braced lists: their elements are evaluated in order.
template <class F, class... A> int64_t carve_size(F layout, A... args) { Carve c{nullptr}; layout(c, args...); return c.used; }
template <class F, class... A> auto carve_at(double* base, F layout, A... args) { Carve c{base}; return layout(c, args...); }

// The L-BFGS state of one (ld, m), d_lbf: ((5 + 2m)·D + 2m + 11)·ld
struct LbfgsState {
    double *trial, *g, *dir, *alpha, *glp;                   // [D][ld]; glp = ∇ℓπ
    double *S, *Y;                                           // [m][D][ld]
    double *sy, *coef;                                       // [m][ld]
    double *lp, *f, *t, *gd, *gn;                            // [ld]; lp = ℓπ
    int32_t *status, *iters, *evals, *nbt, *cnt, *head;      // [ld]
};
inline LbfgsState lbfgs_state(Carve& c, int64_t D, int64_t ld, int64_t m) {
    const int64_t plane = D * ld;
    return {c.take(plane), c.take(plane), c.take(plane), c.take(plane), c.take(plane),
            c.take(m * plane), c.take(m * plane),
            c.take(m * ld), c.take(m * ld),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld)};
}

// sᵀy and the first loop's coefficients of the direction call, d_lbd: 2m·ld
struct LbfgsCoef { double *sy, *coef; };      // [m][ld]
inline LbfgsCoef lbfgs_coef(Carve& c, int64_t ld, int64_t m) { return {c.take(m * ld), c.take(m * ld)}; }

// The Pathfinder state of one (ld), d_pf: (D² + 5D + 8)·ld. Two fits per chain — slot[c] names the kept one, the other receives the
// candidate — and the scalars. The kernels take it by value (OpenArgs, ElboArgs): its members and their order are their argument layout.
struct PfState {
    double *mu, *sqa, *chol, *logdet, *elbo;      // μ, √α [2][D][ld] · L̃ packed [2][P][ld], P = D(D+1)/2 · logdet [2][ld] · ELBO [ld]
    int32_t *slot, *elbo_iter, *n_fits, *prev_iters, *fresh;      // [ld]
};
inline PfState pf_state(Carve& c, int64_t D, int64_t ld) {
    return {c.take(2 * D * ld), c.take(2 * D * ld), c.take(D * (D + 1) * ld), c.take(2 * ld), c.take(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld)};
}

// Pathfinder's ELBO batch of KW = n_elbo·W draws, d_pfb: (D + 2)·KW
struct PfBatch { double *phi, *lp, *logq; };      // φ [D][KW] · ℓπ, log q [KW]
inline PfBatch pf_batch(Carve& c, int64_t D, int64_t KW) { return {c.take(D * KW), c.take(KW), c.take(KW)}; }

// The explorer's work arrays, d_hmc: 4·D·ld + 4·ld. q, p, gpr, glp = ∇ℓπ [D][ld] · lp = ℓπ, lp0, lpt0, K0 [ld]
struct HmcWork { double *q, *p, *gpr, *glp, *lp, *lp0, *lpt0, *K0; };
inline HmcWork hmc_work(Carve& c, int64_t D, int64_t ld) {
    return {c.take(D * ld), c.take(D * ld), c.take(D * ld), c.take(D * ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld)};
}

// The trees of one NUTS transition (octo_draws_nuts.hip), d_nuts: ((14 + 2·max_depth)·D + 18)·ld. The kernels take it by value (NutsArgs): its
// members and their order are their argument layout.
struct NutsWork {
    double *trial, *pt;                          // [D][ld] the point of the next log-posterior call and its half-kicked momentum
    double *qL, *pL, *gL, *qR, *pR, *gR;         // [D][ld] the tree's two endpoints: θ_t, p, ∇E
    double *prop, *sprop;                        // [D][ld] the proposal of the tree and of the subtree being built
    double *rho, *rho_s;                         // [D][ld] Σp of the tree and of the subtree
    double *gpr, *glp;                           // [D][ld] ∇ℓprior_t and ∇ℓπ at the point of a launch
    double *ck_p, *ck_r;                         // [max_depth][D][ld] the checkpoints: p′ and ρ_s at the leaf that opened a sub-subtree
    double *lp, *H0, *logw, *logw_s, *sum_acc;   // [ld] ℓπ at the point of a launch · H₀ · log w, log w_s · Σ of the leaves' acceptance statistics
    double *prop_lp, *prop_lpt, *sprop_lp, *sprop_lpt, *out_lp, *out_lpt;      // [ld] ℓπ and ℓprior_t of the two proposals and of θ_t as it stands
    int32_t *status, *depth, *n, *nleaf, *v, *sel, *ssel;      // [ld] stop reason (0: building) · j · leaf of the subtree · leaves made · ±1 · leaf numbers of the proposals
};
inline NutsWork nuts_work(Carve& c, int64_t D, int64_t ld, int64_t max_depth) {
    const int64_t plane = D * ld;
    return {c.take(plane), c.take(plane),
            c.take(plane), c.take(plane), c.take(plane), c.take(plane), c.take(plane), c.take(plane),
            c.take(plane), c.take(plane),
            c.take(plane), c.take(plane),
            c.take(plane), c.take(plane),
            c.take(max_depth * plane), c.take(max_depth * plane),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld)};
}

// The state machines of one slice-sampling transition (octo_draws_slice.hip), d_slice: (2·D + 28)·ld. The kernels take it by value (SliceArgs):
// its members and their order are their argument layout.
struct SliceWork {
    double *trial, *gpr;                         // [D][ld] the point of the next log-posterior call: θ_t but for the coordinate being updated · ∇ℓprior_t (target_at's, not read)
    double *lp, *E0, *out_lp, *out_lpt;          // [ld] ℓπ at the point of a launch · E, ℓπ and ℓprior_t of θ_t as it stands
    double *z, *L, *R, *EL, *ER;                 // [ld] the level · the interval of the update and E at its ends
    double *Lb, *Rb;                             // [ld] L̄, R̄: the shrunk interval
    double *Lh, *Rh, *ELh, *ERh;                 // [ld] L̂, R̂ of the acceptance test and E at them
    double *xp, *Ep, *lpp, *lptp;                // [ld] the proposal x′ and E, ℓπ, ℓprior_t there
    int32_t *status, *j, *phase, *i, *flag;      // [ld] OCTO_DRAWS_SLICE_* · the update number · what the launch's evaluation is · the doubling or shrink number · the test's flag
    int32_t *n_eval, *n_expand, *n_shrink, *n_stuck;      // [ld] the counts
};
inline SliceWork slice_work(Carve& c, int64_t D, int64_t ld) {
    const int64_t plane = D * ld;
    return {c.take(plane), c.take(plane),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take(ld), c.take(ld),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld)};
}

// The state machines of one constrained-prior move of nested sampling (octo_draws_nested.hip), d_nest: (3·D + 15)·ld. The kernels take it by value
// (NestedArgs): its members and their order are their argument layout.
struct NestedWork {
    double *trial, *gpr, *u;                     // [D][ld] θ_t of the point of the next log-posterior call · ∇ℓprior_t (target_at's, not read) · the gathered cube columns (the opening's)
    double *lp, *L, *R, *xp, *keep;              // [ld] ℓπ at the point of a launch · the interval of the update · the proposal x′ · θ_t of the coordinate as it stands
    int32_t *status, *j, *phase, *s, *J, *Kr;    // [ld] OCTO_DRAWS_NESTED_* · the update number · what the launch's evaluation is · the shrink number · the steps left on either side
    int32_t *n_eval, *n_step, *n_shrink, *n_stuck;      // [ld] the counts
};
inline NestedWork nested_work(Carve& c, int64_t D, int64_t ld) {
    const int64_t plane = D * ld;
    return {c.take(plane), c.take(plane), c.take(plane),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld)};
}

// The population of differential evolution (octo_draws_de.hip), d_de: (5·D + 12)·ld. The population and the trial points are kept twice: a
// generation's launch reads one copy of each and writes the other, and so do the two [ld] arrays that other lanes read (f and ℓprior_t of the
// trial). Which copy is current is the parity of the generations made since the opening; octo_draws_de_device hands the kernels the current
// and the next one by name.
struct DeWork {
    double *pop0, *pop1, *trial0, *trial1, *gpr;      // [D][ld] X and the trial points V, twice · ∇ℓprior_t (target_at's, not read)
    double *lp, *f0, *f1, *tlpt0, *tlpt1;             // [ld] ℓπ at the trial points of a launch · f of the population, twice · ℓprior_t of the trial points, twice
    double *lpt, *F, *CR, *Ft, *CRt;                  // [ld] ℓprior_t of the population · (F_i, CR_i) · (F′, CR′) of the trial
    int32_t *n_accept, *improved;                     // [ld] acceptances so far · the last generation accepted
};
inline DeWork de_work(Carve& c, int64_t D, int64_t ld) {
    const int64_t plane = D * ld;
    return {c.take(plane), c.take(plane), c.take(plane), c.take(plane), c.take(plane),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld),
            c.take<int32_t>(ld), c.take<int32_t>(ld)};
}

// The OFTI rejection sampler (octo_draws_ofti.hip). The rows of the table for k_oftis_post, d_oftis_rows: 8·n_rows — a row record of the main
// library, {t, w_rr, w_dd, w_rd, p, q, 0, 0}.
struct OftiRows { double* rows; };      // [n_rows][8]
inline OftiRows ofti_rows(Carve& c, int64_t n_rows) { return {c.take(8 * n_rows)}; }

// The work group of one octo_draws_ofti_rejection call, d_oftis: 10·chunk + N + 2·nblk + 2 + 29·room. Per chunk θ and nl (regenerated, never kept for
// all N); ℓ of all N draws at 8 bytes a draw, the block maxima, the block counts with their total, the maximum; for the `room` stored draws their
// index, ℓ (twice: k_scatter writes two columns), θ, nl and the posterior rows.
struct OftiWork {
    double *theta, *nl;                   // [5][chunk]
    double *ll, *pmax; int64_t* cnt;      // [N] · [nblk] · [nblk + 1]
    double* max;                          // [1]
    uint64_t* ix; double *oll, *olp;      // [room]
    double *otheta, *onl, *post;          // [5][room] · [5][room] · [16][room]
};
inline OftiWork ofti_work(Carve& c, int64_t chunk, int64_t N, int64_t nblk, int64_t room) {
    return {c.take(5 * chunk), c.take(5 * chunk), c.take(N), c.take(nblk), c.take<int64_t>(nblk + 1), c.take(1),
            c.take<uint64_t>(room), c.take(room), c.take(room), c.take(5 * room), c.take(5 * room), c.take(16 * room)};
}

// The order of one cull of nested sampling, d_ncull: K. order[r] = the live slot of rank r, ascending by (ℓ, slot).
struct NestedCull { int32_t* order; };      // [K]
inline NestedCull nested_cull(Carve& c, int64_t K) { return {c.take<int32_t>(K)}; }

// The block partials of the grouped moments (octo_draws_adapt.hip), d_mom: nblk·G·(2K + 1). Per block of 256 chains and group: the number
// of chains it holds · per row their sum and Σ(x − the block's mean)². sum and m2 of a (block, group) with cnt = 0 are never written or read.
struct MomentsPartials { double *cnt, *sum, *m2; };      // [nblk][G] · [nblk][G][K] · [nblk][G][K]
inline MomentsPartials moments_partials(Carve& c, int64_t nblk, int64_t G, int64_t K) {
    return {c.take(nblk * G), c.take(nblk * G * K), c.take(nblk * G * K)};
}

// The block partials of the pooled covariance (octo_draws_dense.hip), on d_mom as well: nblk·(1 + K + K(K+1)/2). Per block of 256 chains: the number
// of chains it holds · per row their sum · per pair i >= j, packed by rows, Σ(x_i − the block's mean_i)(x_j − the block's mean_j). sum and m2 of a
// block with cnt = 0 are never written or read.
struct CovPartials { double *cnt, *sum, *m2; };      // [nblk] · [nblk][K] · [nblk][K(K+1)/2]
inline CovPartials cov_partials(Carve& c, int64_t nblk, int64_t K) { return {c.take(nblk), c.take(nblk * K), c.take(nblk * (K * (K + 1) / 2))}; }

// The block partials of the tempering statistics (octo_draws_pt.hip), on d_mom as well: 7·P·nblk. Per pair of neighbouring slots (P = T − 1) and
// block of 256 chains: Σα · the forward stepping-stone terms' count, maximum and Σ exp(v − maximum) · the backward terms' three. Pair-major, so
// that the merge reads a pair's blocks side by side; m of a (pair, block) without a term is −Inf and its s is 0. The kernels take it by value.
struct PtPartials { double *A, *nf, *mf, *sf, *nb, *mb, *sb; };      // [P][nblk] each
inline PtPartials pt_partials(Carve& c, int64_t P, int64_t nblk) {
    return {c.take(P * nblk), c.take(P * nblk), c.take(P * nblk), c.take(P * nblk), c.take(P * nblk), c.take(P * nblk), c.take(P * nblk)};
}

// The reference table of a variational leg (octo_draws_vref.hip), CALLER-owned: 15·D doubles at D coordinates, PRIOR_NC = IC_N = 4. What a
// handle's three prior arrays hold, side by side, and the fit they were made from: D octo_prior of 40 bytes — REF_PRIOR_DOUBLES doubles —
// each, their constants, and μ and σ. octo_draws_reference_doubles sizes it; octo_draws_use_reference points the handle's active table at its
// first three parts.
constexpr int64_t REF_PRIOR_DOUBLES = 5;      // sizeof(octo_prior)/8: {int32 kind, pad; double p0, p1, lo, hi}
struct RefTable { double *priors, *pc, *ic, *mean, *sd; };      // octo_prior [D] · [D][nc] · [D][icn] · [D] · [D]
inline RefTable ref_table(Carve& c, int64_t D, int64_t nc, int64_t icn) {
    return {c.take(REF_PRIOR_DOUBLES * D), c.take(nc * D), c.take(icn * D), c.take(D), c.take(D)};
}

// The work arrays of an expression program (octo_draws_program.hip), d_prog: (N + 2·D + 2·n_in + 7·P + 3)·ldw. N = D + n_ops nodes, n_in kernel
// inputs, P planets, ldw = the batch rounded up to whole waves. The kernels take it by value: its members and their order are their argument layout.
struct ProgWork {
    double* vals;               // [N][ldw] node values of the forward sweep, what the reverse sweep reads its operands from
    double *dx, *gpd;           // [D][ldw] dx_d/dθ_t · ∂(logpdf_with_trans of prior d)/∂θ_t
    double *inputs, *g_in;      // [n_in][ldw] what octo_eval_device reads (elements, then nuisances) and its gradient
    double* gtp;                // [P][7][ldw] a TPERI binding's ∂tp/∂(angle, a, e, i, ω, Ω, M)
    double *pp, *ll;            // [ldw] prior part + terms · ℓ
    int32_t* healed;            // [ldw] the prior was healed
};
inline ProgWork prog_work(Carve& c, int64_t D, int64_t N, int64_t n_in, int64_t P, int64_t ldw) {
    return {c.take(N * ldw), c.take(D * ldw), c.take(D * ldw), c.take(n_in * ldw), c.take(n_in * ldw), c.take(7 * P * ldw), c.take(ldw), c.take(ldw),
            c.take<int32_t>(ldw)};
}

// Along-scan absolute astrometry (octo_draws_scan.hip), d_scan: (n_tasks·n_sums + 28)·ldw. The partial sums of every task of SCAN_ROWS table rows,
// task-major, and the marginal mode's per-walker solve. n_sums = 9 + 10·P: ℓ, the jitter sum, the marginal mode's Σw²cᵀA⁻¹c, six β sums, ten adjoint
// sums a planet (U1 … U6, GE, GM, GT, GC of the main library's finish); the marginal mode's first pass keeps A (21, packed by rows) and b (6) in the same
// rows, so there n_sums = max(9 + 10·P, 27). The kernels take it by value.
struct ScanWork {
    double* part;      // [n_tasks][n_sums][ldw]
    double* marg;      // [28][ldw] β̂ [6] · A⁻¹ packed by rows [21] · log det A
};
inline ScanWork scan_work(Carve& c, int64_t n_tasks, int64_t n_sums, int64_t ldw) { return {c.take(n_tasks * n_sums * ldw), c.take(28 * ldw)}; }

// The device side of octo_draws_scan_eval, d_scan_hst: (2·P·9 + 3·K + 3)·ld
struct ScanStaging {
    double *elems, *g_elems;           // [P·9][ld]
    double *beta, *g_beta, *beta_hat;  // [K][ld]
    double *jitter, *g_jitter, *ll;    // [ld]
};
inline ScanStaging scan_staging(Carve& c, int64_t P, int64_t K, int64_t ld) {
    return {c.take(9 * P * ld), c.take(9 * P * ld), c.take(K * ld), c.take(K * ld), c.take(K * ld), c.take(ld), c.take(ld), c.take(ld)};
}

// The catalogue proper-motion anomaly (octo_draws_pma.hip), d_pma: (n_tasks·n_sums + 9)·ldw, n_sums = max(8, 10·P). The partial sums of every task of
// SCAN_ROWS table rows, task-major: first the Q sums z_q of k_pma_rows, which k_pma_close consumes, then in the same rows the ten adjoint sums a planet
// of k_pma_adj (U1 … U6, GE, GM, GT, GC of the main library's finish). λ = M·r of every walker (0 behind Q, and for an invalid walker) and its validity
// (1 or 0) stay between k_pma_close and the adjoint kernels. The kernels take it by value.
struct PmaWork {
    double* part;      // [n_tasks][n_sums][ldw]
    double* lam;       // [8][ldw]
    double* ok;        // [ldw]
};
inline PmaWork pma_work(Carve& c, int64_t n_tasks, int64_t n_sums, int64_t ldw) { return {c.take(n_tasks * n_sums * ldw), c.take(8 * ldw), c.take(ldw)}; }

// The device side of octo_draws_pma_eval, d_pma_hst: (2·P·9 + 3·K + 1)·ld
struct PmaStaging {
    double *elems, *g_elems;               // [P·9][ld]
    double *gamma, *g_gamma, *gamma_hat;   // [K][ld]
    double* ll;                            // [ld]
};
inline PmaStaging pma_staging(Carve& c, int64_t P, int64_t K, int64_t ld) {
    return {c.take(9 * P * ld), c.take(9 * P * ld), c.take(K * ld), c.take(K * ld), c.take(K * ld), c.take(ld)};
}

// The Gaussian-process RV term (octo_draws_gp.hip), d_gp: (n + 1 + [grad]·((n_seg + SEGMENT)·n_state + n_tasks·n_sums))·ldw, n_state = R'(R' + 1)/2 + R'
// of the R' = 2, 4 or 8 slots the kernels are instantiated for, n_seg = ⌈n/SEGMENT⌉, n_tasks = ⌈n/SCAN_ROWS⌉, n_sums = 4 + 6·P. The residuals r_i of
// k_gp_rows, which k_gp_back replaces row by row with α_i; every walker's validity (1 or 0) from k_gp_factor; with a gradient the state (S + D·W·Wᵀ packed,
// f + W·z) handed to the first row of every segment, the states handed to each row of the segment k_gp_back is walking, and the partial sums of k_gp_adj,
// task-major: the K <= 4 sums Σ α_i c_i[k], then six a planet (GE, GM, GT, GC, GK, GW of the main library's finish). The kernels take it by value.
struct GpWork {
    double* res;        // [n][ldw]
    double* ok;         // [ldw]
    double* check;      // [ldw/64][n_seg][n_state][64]: a wave's states lie together, so their offsets are constants of the kernel
    double* seg;        // [ldw/64][SEGMENT][n_state][64]
    double* part;       // [n_tasks][n_sums][ldw]
};
inline GpWork gp_work(Carve& c, int64_t n, int64_t n_state, int64_t n_seg, int64_t segment, int64_t n_tasks, int64_t n_sums, int64_t ldw, int64_t grad) {
    return {c.take(n * ldw), c.take(ldw), c.take(grad ? n_seg * n_state * ldw : 0), c.take(grad ? segment * n_state * ldw : 0), c.take(grad ? n_tasks * n_sums * ldw : 0)};
}

// … with dense kernels (octo_draws_gpd.hip), on d_gp as well: (n + 1 + [grad]·n_tasks·n_sums)·ldw + [global]·W·n(n+1)/2. The residuals (then α), the validity and
// the row tasks' sums as above; no checkpoints, no states. A table of more than OCTO_DRAWS_GP_DENSE_LDS_ROWS rows (global) keeps every walker's packed lower
// triangle here, walker-major; a shorter one keeps it in the workgroup's LDS.
struct GpdWork {
    double* res;        // [n][ldw]
    double* ok;         // [ldw]
    double* part;       // [n_tasks][n_sums][ldw]
    double* tri;        // [W][n(n+1)/2]
};
inline GpdWork gpd_work(Carve& c, int64_t n, int64_t n_tasks, int64_t n_sums, int64_t ldw, int64_t W, int64_t global, int64_t grad) {
    return {c.take(n * ldw), c.take(ldw), c.take(grad ? n_tasks * n_sums * ldw : 0), c.take(global ? W * (n * (n + 1) / 2) : 0)};
}

// The device side of octo_draws_gp_eval, d_gp_hst: (2·P·9 + 2·H + 2·K + 3)·ld
struct GpStaging {
    double *elems, *g_elems;       // [P·9][ld]
    double *hyper, *g_hyper;       // [H][ld]
    double *beta, *g_beta;         // [K][ld]
    double *jitter, *g_jitter, *ll;      // [ld]
};
inline GpStaging gp_staging(Carve& c, int64_t P, int64_t H, int64_t K, int64_t ld) {
    return {c.take(9 * P * ld), c.take(9 * P * ld), c.take(H * ld), c.take(H * ld), c.take(K * ld), c.take(K * ld), c.take(ld), c.take(ld), c.take(ld)};
}

// The convergence diagnostics of K rows (octo_draws_diag.hip), d_diag: 2K(P + S) + 10KM + 4K·T·(nblk + 1) + 5K. N draws of M = 2W split chains a row,
// S = M·N used draws, P = the power of two the sort pads them to, T = the lags rounded up to whole blocks of 16, nblk = ⌈M/256⌉. The kernels take it
// by value: its members and their order are their argument layout.
struct DiagWork {
    double *keys, *fkeys;      // [K][P] the used draws of a row and their |x − median|, sorted ascending, +Inf behind the S
    double *z, *zf;            // [K][N][M] the rank-normalised draws, bulk and folded: lane = split chain
    double *mu, *var;          // [K][5][M] the mean and the variance of every split chain: of z, x, 1[x <= q05], 1[x <= q95], z_folded
    double* part;              // [K][4][T][nblk] the block sums of acov_m(t) of the first four
    double* rho;               // [K][4][T] ρ_t, then ρ̂_t
    double* q;                 // [3][K] q05, q50, q95
    int32_t *bad, *ok;         // [K] a used draw is not finite · the row is valid
};
inline DiagWork diag_work(Carve& c, int64_t K, int64_t P, int64_t S, int64_t M, int64_t T, int64_t nblk) {
    return {c.take(K * P), c.take(K * P), c.take(K * S), c.take(K * S), c.take(5 * K * M), c.take(5 * K * M), c.take(4 * K * T * nblk),
            c.take(4 * K * T), c.take(3 * K), c.take<int32_t>(K), c.take<int32_t>(K)};
}

// The device side of the host-buffer twins, both on d_hst. octo_draws_lbfgs: 2·D·ld + 5·ld + D
struct LbfgsStaging {
    double *theta_t, *inv_hess_diag;      // [D][ld]
    double *lp, *gn;                      // [ld]
    int32_t *status, *iters, *evals;      // [ld]
    double* inv_mass;                     // [D]
};
inline LbfgsStaging lbfgs_staging(Carve& c, int64_t D, int64_t ld) {
    return {c.take(D * ld), c.take(D * ld), c.take(ld), c.take(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take<int32_t>(ld), c.take(D)};
}

// octo_draws_hmc_step: 2·D·ld + 6·ld + D
struct HmcStaging {
    double *theta_t, *theta_prop;         // [D][ld]
    double *beta, *eps, *lp, *ll, *dH;    // [ld]
    int32_t* accepted;                    // [ld]
    double* inv_mass;                     // [D]
};
inline HmcStaging hmc_staging(Carve& c, int64_t D, int64_t ld) {
    return {c.take(D * ld), c.take(D * ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take(ld), c.take<int32_t>(ld), c.take(D)};
}

// The three groups of the drivers (octo_draws.hip). The chunk buffers and the candidate lists, d_chunk: fixed for a handle
struct ChunkBufs {
    double *tt, *lpt;                     // θ_t [D][chunk], logprior_t [chunk]
    double* clp; uint64_t* cix;           // [lists] the candidate lists, list 0 = the running list
    double* max;                          // [1]
};
inline ChunkBufs chunk_bufs(Carve& c, int64_t D, int64_t chunk, int64_t lists) {
    return {c.take(D * chunk), c.take(chunk), c.take(lists), c.take<uint64_t>(lists), c.take(1)};
}

// the per-draw arrays of a call of n draws, d_arr: lp, ll [n] · the block maxima [nblk] · the block counts and their total [nblk + 1]
struct DrawArrays { double *lp, *ll, *pmax; int64_t* cnt; };
inline DrawArrays draw_arrays(Carve& c, int64_t n, int64_t nblk) { return {c.take(n), c.take(n), c.take(nblk), c.take<int64_t>(nblk + 1)}; }

// the outputs of a call before they go to the host, d_out: index, ll, lp [n] · θ [D][n]
struct Outputs { uint64_t* ix; double *ll, *lp, *theta; };
inline Outputs outputs(Carve& c, int64_t D, int64_t n) { return {c.take<uint64_t>(n), c.take(n), c.take(n), c.take(D * n)}; }
