// octo_draws_nested.hip — nested sampling of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the three functions): the unit cube and
// the hypercube transform, the ordered cull of a live set with its evidence bookkeeping, and the constrained-prior move — a coordinate-wise slice
// sampler IN THE CUBE under a hard floor on the likelihood, the B chains in lockstep rounds of one FORWARD log-posterior call, lane = chain.
//
//   k_cube            the uniforms of purpose 0, one launch per Philox block of four coordinates: the numbers k_draw feeds to the quantile.
//   k_from_cube       draw_block (octo_draws_common.h: what k_draw does after its Philox call) on uniforms read from memory; one launch per four
//                     coordinates, as k_draw, and for the same reason: no loop over the coordinates around the quantile's polynomials.
//   k_nested_sort     ONE block: the K (ℓ, slot) pairs, padded to a power of two, sorted in LDS (bitonic); then one lane walks the B running sums
//                     (log volume, log weight, log evidence) in the stated order and writes the state.
//   k_nested_width    one block per coordinate: max − min over the K live points, a fixed-shape reduction.
//   k_nested_scatter  one thread per (dead rank, coordinate): the dead record, and with replace the survivor's copy into the dead slot.
//   k_nested_gather   the B columns named by d_slot, into the work plane the opening's k_from_cube launches read.
//   k_nested_open     every chain's state machine at update 0 and its first trial coordinate.
//   k_nested_round    ℓ at the trial point, received by the chain's phase (a step to the left, to the right, a shrink proposal), and the next trial
//                     coordinate: the one coordinate that changed goes through cube_link at ONE call site, with the lane's own d.
//   k_nested_report   the outputs alone: a resumed call of no rounds.
// From octo_draws_common.h, as the slice sampler: SamplerHead, chain_of, target_at, logpost_at, run_rounds — with no gradient array: Target::grad is
// never called. Nothing of a chain lives in a private array: its state machine sits in the handle's work array (nested_work of octo_draws_layout.h).
#include "octo_draws_common.h"

namespace {

constexpr int SORT_TPB = 1024;
constexpr int32_t NO_SLOT = 0x7fffffff;

// ---- the cube ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_cube(uint64_t seed, uint64_t first, int64_t n, int64_t ld, int32_t D, int32_t d0, double* __restrict__ u) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    uint64_t r[4];
    philox4x64(seed, KEY1, first + (uint64_t)t, (uint64_t)(d0 >> 2), OCTO_DRAWS_PURPOSE_PRIOR, 0, r);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (d0 + q < D) u[(int64_t)(d0 + q) * ld + t] = u01(r[q]);
}

// a.idx, a.seed and a.first are not read. A draw with a coordinate outside (0, 1), in ANY block of four, is bad in every launch: all its outputs are NaN.
__global__ __launch_bounds__(TPB) void k_from_cube(DrawArgs a, const double* __restrict__ cube) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool live = t < a.n;                        // no early exit: prior_density_lanes votes across the wave
    const int64_t tl = live ? t : a.n - 1;
    bool bad = false;
    for (int d = 0; d < a.D; ++d) {
        const double v = cube[(int64_t)d * a.ld + tl];
        bad = bad || !(v > 0.0 && v < 1.0);           // NaN compares false
    }
    double u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = (a.d0 + q < a.D && !bad) ? cube[(int64_t)(a.d0 + q) * a.ld + tl] : 0.5;
    draw_block(a, t, tl, live, u, bad);
}

int launch_from_cube(octo_draws* h, hipStream_t st, int64_t n, int64_t ld, const double* d_u, double* d_theta, double* d_theta_t, double* d_lpt) {
    DrawArgs a;
    std::memset(&a, 0, sizeof(a));
    a.priors = h->d_priors; a.pc = h->d_pc; a.ic = h->d_ic; a.D = h->D;
    a.n = n; a.ld = ld;
    a.theta = d_theta; a.theta_t = d_theta_t; a.lpt = d_lpt;
    for (a.d0 = 0; a.d0 < h->D; a.d0 += 4) hipLaunchKernelGGL(k_from_cube, grid_of(n), dim3(TPB), 0, st, a, d_u);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

// ---- the cull ------------------------------------------------------------------------------------------------------------------------------
// the ordering key: NaN and −Inf count as −Inf
__device__ __forceinline__ double cull_key(double ll) { return ll > -INFINITY ? ll : -INFINITY; }

// max(a, b) + log1p(exp(−|a − b|)); −Inf when both are −Inf
__device__ __forceinline__ double logaddexp(double a, double b) {
    if (a == -INFINITY && b == -INFINITY) return -INFINITY;
    return fmax(a, b) + log1p(exp(-fabs(a - b)));
}

struct CullArgs {
    uint64_t seed, iter;
    int32_t K, B, D, replace;
    int64_t ldK, dead_first, ld_dead;
    double *u_live, *ll_live, *state;
    double *dead_u, *dead_ll, *dead_logvol, *dead_logwt;
    int32_t* slot;
    double* width;
    int32_t* order;
};

__global__ __launch_bounds__(SORT_TPB) void k_nested_sort(CullArgs a) {
    __shared__ double s_key[OCTO_DRAWS_NESTED_MAX_LIVE];
    __shared__ int32_t s_ix[OCTO_DRAWS_NESTED_MAX_LIVE];
    const int K = a.K, B = a.B, tid = threadIdx.x;
    int P = 2;
    while (P < K) P <<= 1;
    for (int i = tid; i < P; i += SORT_TPB) {
        s_key[i] = i < K ? cull_key(a.ll_live[i]) : INFINITY;
        s_ix[i] = i < K ? i : NO_SLOT;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < P; i += SORT_TPB) {
                const int p = i ^ j;
                if (p > i) {
                    const double ki = s_key[i], kp = s_key[p];
                    const int32_t xi = s_ix[i], xp = s_ix[p];
                    const bool after = ki > kp || (ki == kp && xi > xp);      // (ℓ, slot) is a total order: element i sorts after element p
                    if (after == ((i & k) == 0)) { s_key[i] = kp; s_key[p] = ki; s_ix[i] = xp; s_ix[p] = xi; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < K; i += SORT_TPB) a.order[i] = s_ix[i];
    if (tid != 0) return;
    // one lane, rank by rank
    double logZ = a.state[0], logX = a.state[1];
    const double n_dead = a.state[5];
    for (int r = 0; r < B; ++r) {
        const double t = 1.0 / (double)(K - r);
        const double logwt = s_key[r] + logX + log(-expm1(-t));
        logX -= t;
        logZ = logaddexp(logZ, logwt);
        if (a.dead_logvol) a.dead_logvol[a.dead_first + r] = logX;
        if (a.dead_logwt) a.dead_logwt[a.dead_first + r] = logwt;
    }
    const double lmax = s_key[K - 1];
    a.state[0] = logZ;
    a.state[1] = logX;
    a.state[2] = s_key[B - 1];
    a.state[3] = lmax;
    a.state[4] = logZ == -INFINITY ? INFINITY : logaddexp(logZ, lmax + logX) - logZ;
    a.state[5] = n_dead + (double)B;
    a.state[6] = 0.0;
    a.state[7] = 0.0;
}

__global__ __launch_bounds__(TPB) void k_nested_width(CullArgs a) {
    __shared__ double s_lo[TPB / WAVE], s_hi[TPB / WAVE];
    const int d = blockIdx.x;
    double lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < a.K; i += TPB) {
        const double v = a.u_live[(int64_t)d * a.ldK + i];
        lo = fmin(lo, v); hi = fmax(hi, v);
    }
#pragma unroll
    for (int k = WAVE / 2; k >= 1; k >>= 1) { lo = fmin(lo, __shfl_xor(lo, k, WAVE)); hi = fmax(hi, __shfl_xor(hi, k, WAVE)); }
    if ((threadIdx.x & (WAVE - 1)) == 0) { s_lo[threadIdx.x / WAVE] = lo; s_hi[threadIdx.x / WAVE] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TPB / WAVE; ++w) { lo = fmin(lo, s_lo[w]); hi = fmax(hi, s_hi[w]); }
        a.width[d] = hi - lo;
    }
}

// thread (r, d): survivors are only read, dead slots only written — and a dead slot's own value is read by the thread that then overwrites it
__global__ __launch_bounds__(TPB) void k_nested_scatter(CullArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= (int64_t)a.B * a.D) return;
    const int r = (int)(t % a.B), d = (int)(t / a.B);
    const int32_t dead = a.order[r];
    const int64_t o = (int64_t)d * a.ldK + dead;
    if (a.dead_u) a.dead_u[(int64_t)d * a.ld_dead + a.dead_first + r] = a.u_live[o];
    if (d == 0) {
        if (a.dead_ll) a.dead_ll[a.dead_first + r] = cull_key(a.ll_live[dead]);
        a.slot[r] = dead;
    }
    if (!a.replace) return;
    uint64_t x[4];
    philox4x64(a.seed, KEY1, (uint64_t)r, 0, OCTO_DRAWS_PURPOSE_NESTED_SEED, a.iter, x);
    const int32_t n = a.K - a.B;
    int32_t pick = (int32_t)floor(u01(x[0]) * (double)n);
    pick = pick < n - 1 ? pick : n - 1;
    const int32_t src = a.order[a.B + pick];
    a.u_live[o] = a.u_live[(int64_t)d * a.ldK + src];
    if (d == 0) a.ll_live[dead] = a.ll_live[src];
}

// ---- the move ------------------------------------------------------------------------------------------------------------------------------
// what the evaluation of a launch is: inside(L) of the stepping out, inside(R), the shrink proposal x′
enum { PH_L = 0, PH_R = 1, PH_X = 2 };
// where a chain's state machine stands between two evaluations
enum { ST_EVAL = 0, ST_NEXT, ST_OPEN, ST_LEFT, ST_RIGHT, ST_CLIP, ST_PROPOSE, ST_DONE };

// eps of the head is the scalar width, step the iteration, theta_t the trial plane
struct NestedArgs : SamplerHead {
    int32_t n_updates, m, max_shrink, write_out;      // n_updates = n_passes·D
    const double* width;                              // [D] or null = eps
    const double* ic;                                 // [D][IC_N]
    const double* state;                              // the floor ℓ* = state[2]
    const int32_t* slot;                              // [B]
    double *u_live, *ll_live;                         // [D][ldK], [K]
    int64_t ldK;
    int32_t K;
    NestedWork s;
    double* o_tt;
    int32_t *o_eval, *o_step, *o_shrink, *o_stuck, *o_status, *o_nact;
};

__device__ __forceinline__ void nested_uniforms(const NestedArgs& a, int32_t c, int32_t j, int32_t i, double& v0, double& v1, double& v2) {
    uint64_t r[4];
    philox4x64(a.seed, KEY1, (uint64_t)c, (uint64_t)j * 128 + (uint64_t)i, OCTO_DRAWS_PURPOSE_NESTED_MOVE, a.step, r);
    v0 = u01(r[0]); v1 = u01(r[1]); v2 = u01(r[2]);
}

// the live slot of chain w, held inside the live set whatever d_slot holds
__device__ __forceinline__ int32_t slot_of(const int32_t* slot, int64_t w, int32_t K) { return min(max(slot[w], 0), K - 1); }

__device__ __forceinline__ double nested_width_at(const NestedArgs& a, int32_t d) { return a.width ? a.width[d] : a.eps; }

// The chain's state machine from `stage` to its next evaluation, or to DONE: everything between two evaluations, a y outside (0, 1) among it (outside
// without an evaluation, no round). The loop is over these stages, which hold no transcendental; the one trial coordinate then goes through cube_link.
__device__ __forceinline__ void advance(const NestedArgs& a, int64_t w, int32_t c, int32_t stage, int32_t j, double L, double R, double x, int32_t s, int32_t J,
                                        int32_t Kr) {
    int32_t d = j < 0 ? 0 : j % a.D, phase = PH_X;
    int64_t o = (int64_t)d * a.ld + w;
    int32_t n_shrink = a.s.n_shrink[w];
    double y = 0.5, xp = 0.0;
    while (stage != ST_EVAL && stage != ST_DONE) {
        if (stage == ST_NEXT) {
            if (j + 1 == a.n_updates) { stage = ST_DONE; continue; }
            j += 1;
            stage = ST_OPEN;
        }
        if (stage == ST_OPEN) {
            d = j % a.D;
            o = (int64_t)d * a.ld + w;
            const double wd = nested_width_at(a, d);
            double v0, v1, v2;
            nested_uniforms(a, c, j, 0, v0, v1, v2);
            x = a.u_live[(int64_t)d * a.ldK + c];
            L = x - wd * v1;
            R = L + wd;
            J = (int32_t)floor((double)a.m * v2);
            J = J < a.m - 1 ? J : a.m - 1;
            Kr = a.m - 1 - J;
            s = 0;
            a.s.keep[w] = a.s.trial[o];
            stage = ST_LEFT;
        }
        if (stage == ST_LEFT) {
            if (J > 0 && L > 0.0 && L < 1.0) { y = L; phase = PH_L; stage = ST_EVAL; continue; }
            stage = ST_RIGHT;
        }
        if (stage == ST_RIGHT) {
            if (Kr > 0 && R > 0.0 && R < 1.0) { y = R; phase = PH_R; stage = ST_EVAL; continue; }
            stage = ST_CLIP;
        }
        if (stage == ST_CLIP) {
            L = fmax(L, 0.0);
            R = fmin(R, 1.0);
            stage = ST_PROPOSE;
        }
        if (stage == ST_PROPOSE) {
            if (s == a.max_shrink) {      // stuck: the coordinate keeps its value
                a.s.n_stuck[w] += 1;
                a.s.trial[o] = a.s.keep[w];
                stage = ST_NEXT;
                continue;
            }
            double v0, v1, v2;
            nested_uniforms(a, c, j, 64 + s, v0, v1, v2);
            xp = L + v0 * (R - L);
            n_shrink += 1;
            if (xp > 0.0 && xp < 1.0) { y = xp; phase = PH_X; stage = ST_EVAL; continue; }
            if (xp < x) L = xp; else R = xp;      // rounded onto a face of the cube: outside
            s += 1;
        }
    }
    a.s.n_shrink[w] = n_shrink;
    if (stage == ST_DONE) {
        a.s.status[w] = OCTO_DRAWS_NESTED_DONE;
        return;
    }
    a.s.j[w] = j; a.s.phase[w] = phase; a.s.s[w] = s; a.s.J[w] = J; a.s.Kr[w] = Kr;
    a.s.L[w] = L; a.s.R[w] = R; a.s.xp[w] = xp;
    const octo_prior pr = a.priors[d];
    const PriorBounds B = prior_bounds(pr);
    double th;
    a.s.trial[o] = cube_link(pr, B, a.ic + IC_N * d, y, th);
}

__device__ __forceinline__ void report(const NestedArgs& a, int64_t w) {
    const int32_t status = a.s.status[w];
    if (a.o_tt) {
        for (int d = 0; d < a.D; ++d) a.o_tt[(int64_t)d * a.ld + w] = a.s.trial[(int64_t)d * a.ld + w];
        if (status == OCTO_DRAWS_NESTED_ACTIVE) a.o_tt[(int64_t)(a.s.j[w] % a.D) * a.ld + w] = a.s.keep[w];      // the point as it stands, not the trial
    }
    if (a.o_eval) a.o_eval[w] = a.s.n_eval[w];
    if (a.o_step) a.o_step[w] = a.s.n_step[w];
    if (a.o_shrink) a.o_shrink[w] = a.s.n_shrink[w];
    if (a.o_stuck) a.o_stuck[w] = a.s.n_stuck[w];
    if (a.o_status) a.o_status[w] = status;
    if (a.o_nact && status == OCTO_DRAWS_NESTED_ACTIVE) atomicAdd(a.o_nact, 1);      // an integer count: order-free
}

__global__ __launch_bounds__(TPB) void k_nested_gather(const double* __restrict__ u_live, int64_t ldK, const int32_t* __restrict__ slot, int32_t K, int64_t B, int64_t ld, int32_t D,
                                                       double* __restrict__ u) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= B * D) return;
    const int64_t w = t % B, d = t / B;
    u[d * ld + w] = u_live[d * ldK + min(max(slot[w], 0), K - 1)];
}

// the trial plane holds θ_t of the gathered columns (the opening's k_from_cube launches); ℓ of a slot is d_loglike_live's, so the opening call's is not read
__global__ __launch_bounds__(TPB) void k_nested_open(NestedArgs a) {
    const Chain ch = chain_of(a);
    if (!ch.live) return;
    const int64_t w = ch.w;
    a.s.status[w] = OCTO_DRAWS_NESTED_ACTIVE;
    a.s.n_eval[w] = 0; a.s.n_step[w] = 0; a.s.n_shrink[w] = 0; a.s.n_stuck[w] = 0;
    advance(a, w, slot_of(a.slot, w, a.K), ST_NEXT, -1, 0.0, 0.0, 0.0, 0, 0, 0);
    if (a.write_out) report(a, w);
}

__global__ __launch_bounds__(TPB) void k_nested_round(NestedArgs a) {
    const Chain ch = chain_of(a);
    const Target tg = target_at(a, ch, a.s.trial, a.s.lp, nullptr, a.s.gpr);      // every lane: its prior_loop() votes across the wave; a frozen chain: at its point, ignored
    if (!ch.live) return;
    const int64_t w = ch.w;
    if (a.s.status[w] == OCTO_DRAWS_NESTED_ACTIVE) {
        double ll = tg.lp(w) - tg.lpt;      // the rejection driver's likelihood
        ll = isfinite(ll) ? ll : -INFINITY;
        const bool inside = ll > a.state[2];
        const int32_t c = slot_of(a.slot, w, a.K), j = a.s.j[w], d = j % a.D, phase = a.s.phase[w];
        const double wd = nested_width_at(a, d), x = a.u_live[(int64_t)d * a.ldK + c];
        double L = a.s.L[w], R = a.s.R[w];
        int32_t s = a.s.s[w], J = a.s.J[w], Kr = a.s.Kr[w], stage;
        a.s.n_eval[w] += 1;
        if (phase == PH_L) {
            if (inside) { L -= wd; J -= 1; a.s.n_step[w] += 1; stage = ST_LEFT; }
            else stage = ST_RIGHT;
        } else if (phase == PH_R) {
            if (inside) { R += wd; Kr -= 1; a.s.n_step[w] += 1; stage = ST_RIGHT; }
            else stage = ST_CLIP;
        } else {
            const double xp = a.s.xp[w];
            if (inside) {      // the coordinate becomes x′ with what was evaluated there; the trial plane keeps the transformed value
                a.u_live[(int64_t)d * a.ldK + c] = xp;
                a.ll_live[c] = ll;
                stage = ST_NEXT;
            } else {
                if (xp < x) L = xp; else R = xp;
                s += 1;
                stage = ST_PROPOSE;
            }
        }
        advance(a, w, c, stage, j, L, R, x, s, J, Kr);
    }
    if (a.write_out) report(a, w);
}

__global__ __launch_bounds__(TPB) void k_nested_report(NestedArgs a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w < a.W) report(a, w);
}

int check_live(octo_draws* h, const char* who, int32_t K, int64_t ldK, const void* u, const void* ll, const void* state) {
    if (K < 2 || K > OCTO_DRAWS_NESTED_MAX_LIVE) return fail(h, OCTO_EINVAL, std::string(who) + ": K must be 2 ... OCTO_DRAWS_NESTED_MAX_LIVE");
    if (ldK < K) return fail(h, OCTO_EINVAL, std::string(who) + ": need K <= ldK");
    return u && ll && state ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": d_u_live, d_loglike_live and d_state are required");
}

}  // namespace

extern "C" {

int32_t octo_draws_cube_device(octo_draws* h, uint64_t seed, uint64_t first, int64_t n, int64_t ld, double* d_u, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (n < 0 || ld < n || n > MAX_CHAINS) return fail(h, OCTO_EINVAL, "octo_draws_cube_device: need 0 <= n <= ld, n <= 2^30");
    if (first + (uint64_t)n < first) return fail(h, OCTO_EINVAL, "octo_draws_cube_device: first + n overflows the draw index");
    if (n == 0) return OCTO_OK;
    if (!d_u) return fail(h, OCTO_EINVAL, "octo_draws_cube_device: d_u is required");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    for (int32_t d0 = 0; d0 < h->D; d0 += 4) hipLaunchKernelGGL(k_cube, grid_of(n), dim3(TPB), 0, st, seed, first, n, ld, (int32_t)h->D, d0, d_u);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_from_cube_device(octo_draws* h, int64_t n, int64_t ld, const double* d_u, double* d_theta, double* d_theta_t, double* d_logprior_t,
                                    void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (n < 0 || ld < n || n > MAX_CHAINS) return fail(h, OCTO_EINVAL, "octo_draws_from_cube_device: need 0 <= n <= ld, n <= 2^30");
    if (n == 0 || (!d_theta && !d_theta_t && !d_logprior_t)) return OCTO_OK;
    if (!d_u) return fail(h, OCTO_EINVAL, "octo_draws_from_cube_device: d_u is required");
    OCHK(h, hipSetDevice(h->device));
    return launch_from_cube(h, stream_of(h, hip_stream), n, ld, d_u, d_theta, d_theta_t, d_logprior_t);
}

int32_t octo_draws_nested_cull_device(octo_draws* h, uint64_t seed, uint64_t iter, int32_t K, int64_t ldK, double* d_u_live, double* d_loglike_live,
                                      double* d_state, int32_t B, int32_t replace, int64_t dead_first, int64_t ld_dead, double* d_dead_u,
                                      double* d_dead_loglike, double* d_dead_logvol, double* d_dead_logwt, int32_t* d_slot, double* d_width,
                                      void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    const char* who = "octo_draws_nested_cull_device";
    if (int rc = check_live(h, who, K, ldK, d_u_live, d_loglike_live, d_state)) return rc;
    if (replace != 0 && replace != 1) return fail(h, OCTO_EINVAL, std::string(who) + ": replace must be 0 or 1");
    if (replace ? (B < 1 || B > K - 1) : B != K) return fail(h, OCTO_EINVAL, std::string(who) + ": B must be 1 ... K - 1 with replace = 1, and K with replace = 0");
    if (dead_first < 0 || ld_dead < dead_first + B) return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= dead_first and dead_first + B <= ld_dead");
    if (!d_slot) return fail(h, OCTO_EINVAL, std::string(who) + ": d_slot is required");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    NestedCull nc;
    if (int rc = grow_to(h, h->d_ncull, h->cap_ncull, nc, nested_cull, (int64_t)K)) return rc;
    CullArgs a{seed, iter, K, B, (int32_t)h->D, replace, ldK, dead_first, ld_dead, d_u_live, d_loglike_live, d_state,
               d_dead_u, d_dead_loglike, d_dead_logvol, d_dead_logwt, d_slot, d_width, nc.order};
    hipLaunchKernelGGL(k_nested_sort, dim3(1), dim3(SORT_TPB), 0, st, a);
    if (replace && d_width) hipLaunchKernelGGL(k_nested_width, dim3((unsigned)h->D), dim3(TPB), 0, st, a);      // the live points as they stood on entry
    hipLaunchKernelGGL(k_nested_scatter, grid_of((int64_t)B * h->D), dim3(TPB), 0, st, a);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_nested_move_device(octo_draws* h, uint64_t seed, uint64_t iter, int32_t K, int64_t ldK, double* d_u_live, double* d_loglike_live,
                                      const double* d_state, int64_t B, int64_t ld, const int32_t* d_slot, const double* d_width, double w,
                                      int32_t max_steps, int32_t n_passes, int32_t max_shrink, int32_t n_rounds, int32_t resume, double* d_theta_t,
                                      int32_t* d_n_eval, int32_t* d_n_step, int32_t* d_n_shrink, int32_t* d_n_stuck, int32_t* d_status,
                                      int32_t* d_n_active, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    const char* who = "octo_draws_nested_move_device";
    if (!has_target(h)) return fail(h, OCTO_EINVAL, std::string(who) + ": nested sampling needs a likelihood (the handle has neither a model nor a program)");
    if (int rc = check_live(h, who, K, ldK, d_u_live, d_loglike_live, d_state)) return rc;
    if (B < 0 || B > K - 1 || ld < B) return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= B <= K - 1 and B <= ld");
    if (!d_width && !(w > 0.0 && w <= 1.0)) return fail(h, OCTO_EINVAL, std::string(who) + ": w must be in (0, 1] when d_width is NULL");
    if (max_steps < 1 || max_steps > OCTO_DRAWS_NESTED_MAX_STEPS) return fail(h, OCTO_EINVAL, std::string(who) + ": max_steps must be 1 ... OCTO_DRAWS_NESTED_MAX_STEPS");
    if (max_shrink < 1 || max_shrink > OCTO_DRAWS_NESTED_MAX_SHRINK) return fail(h, OCTO_EINVAL, std::string(who) + ": max_shrink must be 1 ... OCTO_DRAWS_NESTED_MAX_SHRINK");
    if (n_passes < 1 || n_passes > OCTO_DRAWS_NESTED_MAX_PASSES) return fail(h, OCTO_EINVAL, std::string(who) + ": n_passes must be 1 ... OCTO_DRAWS_NESTED_MAX_PASSES");
    if (n_rounds < 0) return fail(h, OCTO_EINVAL, std::string(who) + ": n_rounds >= 0");
    if (resume && (h->nest_passes != n_passes || h->nest_steps != max_steps || h->nest_shrink != max_shrink || h->nest_B != B || h->nest_ld != ld || h->nest_K != K ||
                   h->nest_ldK != ldK || h->nest_seed != seed || h->nest_iter != iter))
        return fail(h, OCTO_EINVAL, std::string(who) + ": resume needs a previous call with the same K, ldK, B, ld, max_steps, n_passes, max_shrink, seed and iter");
    if (B == 0) {
        if (!resume) h->nest_passes = 0;
        return OCTO_OK;
    }
    if (!d_slot) return fail(h, OCTO_EINVAL, std::string(who) + ": d_slot is required");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    NestedArgs a{sampler_head(h, true, seed, iter, 0, B, ld, nullptr, nullptr, nullptr, d_width ? 1.0 : w, nullptr)};
    if (!resume) {
        h->nest_passes = 0;      // a call that fails below leaves nothing to resume
        if (int rc = grow(h, h->d_nest, h->cap_nest, carve_size(nested_work, (int64_t)h->D, ld))) return rc;
    }
    a.s = carve_at(h->d_nest, nested_work, (int64_t)h->D, ld);
    a.theta_t = a.s.trial;
    a.n_updates = n_passes * h->D; a.m = max_steps; a.max_shrink = max_shrink;
    a.width = d_width; a.ic = h->d_ic; a.state = d_state; a.slot = d_slot;
    a.u_live = d_u_live; a.ll_live = d_loglike_live; a.ldK = ldK; a.K = K;
    a.o_tt = d_theta_t; a.o_eval = d_n_eval; a.o_step = d_n_step; a.o_shrink = d_n_shrink; a.o_stuck = d_n_stuck; a.o_status = d_status; a.o_nact = d_n_active;
    if (!resume) {      // the opening: the B columns into the work plane, and all D of them to θ_t by the hypercube transform's launches
        hipLaunchKernelGGL(k_nested_gather, grid_of(B * h->D), dim3(TPB), 0, st, (const double*)d_u_live, ldK, d_slot, K, B, ld, (int32_t)h->D, a.s.u);
        if (int rc = launch_from_cube(h, st, B, ld, a.s.u, nullptr, a.s.trial, nullptr)) return rc;
    }
    if (d_n_active) OCHK(h, hipMemsetAsync(d_n_active, 0, sizeof(int32_t), st));      // the last launch of the call counts into it
    if (int rc = run_rounds(h, st, a, true, a.s.trial, a.s.lp, nullptr, n_rounds, resume != 0, k_nested_open, k_nested_round, k_nested_report)) return rc;
    h->nest_B = B; h->nest_ld = ld; h->nest_K = K; h->nest_ldK = ldK; h->nest_passes = n_passes; h->nest_steps = max_steps; h->nest_shrink = max_shrink;
    h->nest_seed = seed; h->nest_iter = iter;
    return OCTO_OK;
}

}  // extern "C"
