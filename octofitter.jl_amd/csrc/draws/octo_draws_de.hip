// octo_draws_de.hip — differential evolution, the fifteenth part of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the generation):
// a population of W points in θ_t climbs ℓπ by DE/rand/1/bin with parents from a ring neighbourhood and self-adapted (F, CR), generational — a
// generation being one FORWARD octo_model_logpost_device call at the W trial points and one k_de_round launch. Lane = individual, SoA with the
// individual's index fastest. The coordinate loop addresses global memory only; nothing of an individual lives in a private array.
//
//   k_de_open     f of the population as the caller gave it, the population plane = θ_t, the trial points of the first generation.
//   k_de_round    the lane's own selection of generation g (the next population plane, f, ℓprior_t, F, CR, the counts) and its trial point of
//                 generation g + 1 from parents AS THAT SELECTION LEAVES THEM: a parent's selection is decided again from its f and its f′, and
//                 its coordinates are read from the old population plane or the old trial plane accordingly. Both are read-only in the launch,
//                 the lane writes the other copy of each (DeWork of octo_draws_layout.h), so no lane waits for another: no grid-wide barrier.
//   k_de_report   the outputs: θ_t, ℓπ, ℓ, the counts, (F, CR), and in block 0 the best individual by a reduction in a fixed order.
// The trial point's ℓprior_t is formed where the trial point is built (target_at on the lane's own column of the next trial plane), so that every
// lane of the next launch can form any parent's f′ from two loads. From octo_draws_common.h: SamplerHead, chain_of, target_at, dead_state,
// check_sampler_call, run_rounds and the Philox routine; the forward callback alone, Target::grad is never called.
#include "octo_draws_common.h"

namespace {

// what the kernels see of DeWork: the copies that are current (read) and the ones the launch writes. run_rounds evaluates ℓπ at s.trial.
struct DeState {
    const double *trial, *pop;        // [D][ld] V and X, read-only in a launch
    double *trial_n, *pop_n, *gpr;    // [D][ld] the next V and X · ∇ℓprior_t (target_at's, not read)
    double* lp;                       // [ld] ℓπ at s.trial, or null without a model
    const double *f, *tlpt;           // [ld] f of X · ℓprior_t of V
    double *f_n, *tlpt_n;             // [ld]
    double *lpt, *F, *CR, *Ft, *CRt;  // [ld]
    int32_t *n_accept, *improved;     // [ld]
};

// SamplerHead: step = the generation the launch builds trial points for; theta_t = the caller's population; beta, eps_w, inv_mass null
struct DeArgs : SamplerHead {
    int32_t n, write_out;             // n = the neighbourhood's size · write_out: run_rounds's, not read (k_de_report writes every output)
    const double *lo, *hi;            // [D] or both null
    const double* fcr_in;             // [2][ld] or null: (F, CR) at the opening
    DeState s;
    double *o_lp, *o_ll, *o_fcr, *o_best_lp;
    int32_t *o_nacc, *o_best, *o_nimp;
};

// f at a point from ℓπ and ℓprior_t there: ℓπ, or ℓprior_t on a handle without a model; −Inf at a dead or non-finite point
__device__ __forceinline__ double value_of(double beta, int32_t has_model, double lp, double lpt) {
    const double f = has_model ? lp : lpt;
    return dead_state(beta, f, lp, lpt) ? -INFINITY : f;
}
// f′ of individual r's trial point of the generation being selected
__device__ __forceinline__ double trial_value(const DeArgs& a, double beta, int64_t r) {
    return value_of(beta, a.has_model, a.has_model ? a.s.lp[r] : 0.0, a.s.tlpt[r]);
}
__device__ __forceinline__ bool accepts(double fp, double f) { return fp > -INFINITY && fp >= f; }

// ⌊u·n⌋, never n
__device__ __forceinline__ int32_t pick(double u, int32_t n) { return min((int32_t)(u * (double)n), n - 1); }

// member k of individual i's neighbourhood of n: (i − ⌊n/2⌋ + k + (k >= ⌊n/2⌋)) mod W
__device__ __forceinline__ int64_t member(int64_t i, int32_t k, int32_t n, int64_t W) {
    const int32_t h = n / 2;
    int64_t m = i + (k - h) + (k >= h ? 1 : 0);
    if (m < 0) m += W;
    if (m >= W) m -= W;
    return m;
}

// The trial point of individual i = c.wl for generation a.step into the next trial plane, and its own point `own` [D][ld] into the next population
// plane. SELECT: the parents are read as the selection of the generation before leaves them (k_de_round); otherwise from `base` alone (k_de_open:
// the caller's population). Fi, CRi: the individual's pair after its own selection. Every operation is rounded by itself.
template <bool SELECT>
__device__ __forceinline__ void build_trial(const DeArgs& a, const Chain& c, const double* own, const double* base, double Fi, double CRi) {
#pragma clang fp contract(off)
    const int64_t i = c.wl, ld = a.ld;
    uint64_t r0[4], r1[4];
    philox4x64(a.seed, KEY1, (uint64_t)i, 0, OCTO_DRAWS_PURPOSE_DE, a.step, r0);
    philox4x64(a.seed, KEY1, (uint64_t)i, 1, OCTO_DRAWS_PURPOSE_DE, a.step, r1);
    const double Ft = u01(r1[0]) < OCTO_DRAWS_DE_TAU_F ? OCTO_DRAWS_DE_F_LOW + OCTO_DRAWS_DE_F_SPAN * u01(r1[1]) : Fi;
    const double CRt = u01(r1[2]) < OCTO_DRAWS_DE_TAU_CR ? u01(r1[3]) : CRi;
    const int32_t n = a.n;
    const int32_t ka = pick(u01(r0[0]), n);
    int32_t kb = pick(u01(r0[1]), n - 1);
    kb += kb >= ka ? 1 : 0;
    int32_t kc = pick(u01(r0[2]), n - 2);
    kc += kc >= min(ka, kb) ? 1 : 0;
    kc += kc >= max(ka, kb) ? 1 : 0;
    const int64_t p1 = member(i, ka, n, a.W), p2 = member(i, kb, n, a.W), p3 = member(i, kc, n, a.W);
    const double *s1 = base, *s2 = base, *s3 = base;
    if (SELECT) {
        if (accepts(trial_value(a, c.beta, p1), a.s.f[p1])) s1 = a.s.trial;
        if (accepts(trial_value(a, c.beta, p2), a.s.f[p2])) s2 = a.s.trial;
        if (accepts(trial_value(a, c.beta, p3), a.s.f[p3])) s3 = a.s.trial;
    }
    const int32_t jrand = pick(u01(r0[3]), a.D);
    for (int d0 = 0; d0 < a.D; d0 += 4) {
        uint64_t rc[4];
        philox4x64(a.seed, KEY1, (uint64_t)i, (uint64_t)(2 + d0 / 4), OCTO_DRAWS_PURPOSE_DE, a.step, rc);
        double v[4], x[4];
        uint32_t out = 0;      // bit q: coordinate d0 + q crosses and lies beyond a bound
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = d0 + q;
            v[q] = x[q] = 0.0;
            if (d < a.D) {
                const int64_t row = (int64_t)d * ld;
                x[q] = own[row + i];
                v[q] = x[q];
                if (d == jrand || u01(rc[q]) < CRt) {
                    const double diff = s1[row + p1] - s2[row + p2];
                    const double step = Ft * diff;
                    v[q] = s3[row + p3] + step;
                    if (a.lo && (v[q] < a.lo[d] || v[q] > a.hi[d])) out |= 1u << q;
                }
            }
        }
        if (out) {      // a crossing coordinate beyond a bound: between the bound and the individual's own value
            uint64_t rb[4];
            philox4x64(a.seed, KEY1, (uint64_t)i, (uint64_t)(18 + d0 / 4), OCTO_DRAWS_PURPOSE_DE, a.step, rb);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = d0 + q;
                if (out & (1u << q)) {
                    const double lo = a.lo[d], hi = a.hi[d], u = u01(rb[q]);
                    if (v[q] < lo) { const double room = x[q] - lo; const double back = u * room; v[q] = lo + back; }
                    else if (v[q] > hi) { const double room = hi - x[q]; const double back = u * room; v[q] = hi - back; }
                }
            }
        }
        if (c.live) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = d0 + q;
                if (d < a.D) {
                    const int64_t o = (int64_t)d * ld + i;
                    a.s.trial_n[o] = v[q];
                    a.s.pop_n[o] = x[q];
                }
            }
        }
    }
    if (c.live) { a.s.Ft[i] = Ft; a.s.CRt[i] = CRt; }
}

__global__ __launch_bounds__(TPB) void k_de_open(DeArgs a) {
    const Chain ch = chain_of(a);
    const int64_t w = ch.w;
    const Target tg = target_at(a, ch, a.theta_t, a.s.lp, nullptr, a.s.gpr);      // every lane: its prior_loop() votes across the wave
    double Fi = OCTO_DRAWS_DE_F0, CRi = OCTO_DRAWS_DE_CR0;
    if (a.fcr_in) { Fi = a.fcr_in[ch.wl]; CRi = a.fcr_in[a.ld + ch.wl]; }
    if (ch.live) {
        a.s.f_n[w] = value_of(ch.beta, a.has_model, tg.lp(w), tg.lpt);
        a.s.lpt[w] = tg.lpt;
        a.s.F[w] = Fi; a.s.CR[w] = CRi;
        a.s.n_accept[w] = 0; a.s.improved[w] = 0;
    }
    build_trial<false>(a, ch, a.theta_t, a.theta_t, Fi, CRi);
    const Target tt = target_at(a, ch, a.s.trial_n, nullptr, nullptr, a.s.gpr);   // the lane's own column, as it has just written it
    if (ch.live) a.s.tlpt_n[w] = tt.lpt;
}

__global__ __launch_bounds__(TPB) void k_de_round(DeArgs a) {
    const Chain ch = chain_of(a);
    const int64_t w = ch.w, i = ch.wl;
    // the lane's own selection of the generation whose ℓπ has arrived
    const double f = a.s.f[i], fp = trial_value(a, ch.beta, i);
    const bool acc = accepts(fp, f);
    const double Fi = acc ? a.s.Ft[i] : a.s.F[i], CRi = acc ? a.s.CRt[i] : a.s.CR[i];
    if (ch.live) {
        a.s.f_n[w] = acc ? fp : f;
        a.s.improved[w] = acc ? 1 : 0;
        if (acc) {
            a.s.lpt[w] = a.s.tlpt[w];
            a.s.F[w] = Fi; a.s.CR[w] = CRi;
            a.s.n_accept[w] += 1;
        }
    }
    // its trial point of the next generation, and its own point into the next population plane
    build_trial<true>(a, ch, acc ? a.s.trial : a.s.pop, a.s.pop, Fi, CRi);
    // every lane; a live lane reads its own column, as it has just written it. A lane beyond the batch reads the last individual's, which that lane may
    // still be writing: what it computes is dropped, and nothing it reads decides an address.
    const Target tt = target_at(a, ch, a.s.trial_n, nullptr, nullptr, a.s.gpr);
    if (ch.live) a.s.tlpt_n[w] = tt.lpt;
}

// After the last launch of a call the copies it wrote are the current ones: the host hands them over as s.pop, s.f.
__global__ __launch_bounds__(TPB) void k_de_report(DeArgs a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w < a.W) {
        for (int d = 0; d < a.D; ++d) a.theta_t[(int64_t)d * a.ld + w] = a.s.pop[(int64_t)d * a.ld + w];
        const double f = a.s.f[w];
        if (a.o_lp) a.o_lp[w] = f;
        if (a.o_ll) {
            const double ll = f - a.s.lpt[w];
            a.o_ll[w] = isfinite(ll) ? ll : -INFINITY;
        }
        if (a.o_nacc) a.o_nacc[w] = a.s.n_accept[w];
        if (a.o_fcr) { a.o_fcr[w] = a.s.F[w]; a.o_fcr[a.ld + w] = a.s.CR[w]; }
    }
    if (blockIdx.x != 0 || !(a.o_best || a.o_best_lp || a.o_nimp)) return;
    // the best individual: each lane over its stride in ascending order, then the halves of the block; a tie goes to the lower index
    __shared__ double sf[TPB];
    __shared__ int32_t si[TPB], sn[TPB];
    double bf = -INFINITY;
    int32_t bi = -1, cnt = 0;
    for (int64_t k = threadIdx.x; k < a.W; k += TPB) {
        const double f = a.s.f[k];
        if (f > bf) { bf = f; bi = (int32_t)k; }
        cnt += a.s.improved[k];
    }
    sf[threadIdx.x] = bf; si[threadIdx.x] = bi; sn[threadIdx.x] = cnt;
    __syncthreads();
    for (int h = TPB / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const double of = sf[threadIdx.x + h];
            const int32_t oi = si[threadIdx.x + h];
            if (oi >= 0 && (of > sf[threadIdx.x] || (of == sf[threadIdx.x] && oi < si[threadIdx.x]))) { sf[threadIdx.x] = of; si[threadIdx.x] = oi; }
            sn[threadIdx.x] += sn[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (a.o_best) *a.o_best = si[0];
        if (a.o_best_lp) *a.o_best_lp = sf[0];
        if (a.o_nimp) *a.o_nimp = sn[0];
    }
}

// the kernels' view of the work array when `flip` generations' worth of swaps have been made
DeState de_state(const DeWork& k, int flip, bool has_model) {
    DeState s;
    s.pop = flip ? k.pop1 : k.pop0;       s.pop_n = flip ? k.pop0 : k.pop1;
    s.trial = flip ? k.trial1 : k.trial0; s.trial_n = flip ? k.trial0 : k.trial1;
    s.f = flip ? k.f1 : k.f0;             s.f_n = flip ? k.f0 : k.f1;
    s.tlpt = flip ? k.tlpt1 : k.tlpt0;    s.tlpt_n = flip ? k.tlpt0 : k.tlpt1;
    s.gpr = k.gpr; s.lp = has_model ? k.lp : nullptr;
    s.lpt = k.lpt; s.F = k.F; s.CR = k.CR; s.Ft = k.Ft; s.CRt = k.CRt; s.n_accept = k.n_accept; s.improved = k.improved;
    return s;
}

}  // namespace

extern "C" {

int64_t octo_draws_de_work_doubles(int32_t D, int64_t ld) { return D < 1 || ld < 0 ? 0 : carve_size(de_work, (int64_t)D, ld); }

int32_t octo_draws_de_device(octo_draws* h, uint64_t seed, uint64_t gen0, int64_t W, int64_t ld, double* d_theta_t, const double* d_lo, const double* d_hi,
                             int32_t radius, int32_t n_gen, int32_t resume, double* d_fcr, double* d_logpost, double* d_loglike, int32_t* d_n_accept,
                             int32_t* d_best, double* d_best_logpost, int32_t* d_n_improved, void* hip_stream) {
    const char* who = "octo_draws_de_device";
    if (!h) return OCTO_EINVAL;
    if (W < 4) return fail(h, OCTO_EINVAL, std::string(who) + ": W >= 4 (three parents beside the individual)");
    if (radius < 0) return fail(h, OCTO_EINVAL, std::string(who) + ": radius >= 0");
    if (n_gen < 0) return fail(h, OCTO_EINVAL, std::string(who) + ": n_gen >= 0");
    if ((d_lo == nullptr) != (d_hi == nullptr)) return fail(h, OCTO_EINVAL, std::string(who) + ": d_lo and d_hi: both or neither");
    const bool has_model = has_target(h);
    // the samplers' checks of the batch and of ℓπ outputs without a model; their step-size check has nothing to look at here
    if (int rc = check_sampler_call(h, who, W, ld, nullptr, 1.0, has_model, d_logpost, d_loglike)) return rc;
    if (!d_theta_t) return fail(h, OCTO_EINVAL, std::string(who) + ": d_theta_t is required");
    if (resume && !(h->de_open && h->de_W == W && h->de_ld == ld && h->de_radius == radius && h->de_seed == seed && h->de_gen == gen0 && h->de_bounds == (d_lo != nullptr)))
        return fail(h, OCTO_EINVAL, std::string(who) + ": resume needs a previous call with the same W, ld, radius, seed and bounds, and gen0 = its gen0 + n_gen");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    if (!resume) {
        h->de_open = false;      // a call that fails below leaves nothing to resume
        h->de_flip = 0;
        if (int rc = grow(h, h->d_de, h->cap_de, carve_size(de_work, (int64_t)h->D, ld))) return rc;
    }
    const DeWork k = carve_at(h->d_de, de_work, (int64_t)h->D, ld);
    DeArgs a{sampler_head(h, has_model, seed, gen0, 0, W, ld, d_theta_t, nullptr, nullptr, 1.0, nullptr)};
    a.n = (int32_t)(radius == 0 ? W - 1 : std::min<int64_t>(std::max<int64_t>(2 * (int64_t)radius, 3), W - 1));      // W <= 2^30; three parents need n >= 3
    a.write_out = 0;
    a.lo = d_lo; a.hi = d_hi; a.fcr_in = d_fcr;
    a.o_lp = d_logpost; a.o_ll = d_loglike; a.o_fcr = d_fcr; a.o_best_lp = d_best_logpost; a.o_nacc = d_n_accept; a.o_best = d_best; a.o_nimp = d_n_improved;
    // k_de_open writes the copies k_de_round then reads: the opening is the first swap
    if (!resume) {
        a.s = de_state(k, 1, has_model);
        if (int rc = run_rounds(h, st, a, has_model, d_theta_t, k.lp, nullptr, 0, false, k_de_open, k_de_round, k_de_report)) return rc;
    }
    for (int32_t g = 0; g < n_gen; ++g) {      // a generation: ℓπ at the current trial points, the selection, the next trial points
        a.s = de_state(k, h->de_flip, has_model);
        a.step = gen0 + (uint64_t)g + 1;
        if (int rc = run_rounds(h, st, a, has_model, d_theta_t, k.lp, nullptr, 1, true, k_de_open, k_de_round, k_de_report)) return rc;
        h->de_flip ^= 1;
    }
    a.s = de_state(k, h->de_flip, has_model);
    if (int rc = run_rounds(h, st, a, has_model, d_theta_t, k.lp, nullptr, 0, true, k_de_open, k_de_round, k_de_report)) return rc;      // k_de_report
    h->de_W = W; h->de_ld = ld; h->de_radius = radius; h->de_seed = seed; h->de_gen = gen0 + (uint64_t)n_gen; h->de_bounds = d_lo != nullptr;
    h->de_open = true;
    return OCTO_OK;
}

}  // extern "C"
