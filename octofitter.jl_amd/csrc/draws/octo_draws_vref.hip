// octo_draws_vref.hip — the variational reference leg of parallel tempering, in liboctofitter_hip_draws.so (include/octofitter_hip_draws.h,
// "The variational reference of a tempering leg", states it): a mean-field normal N(μ_d, σ_d) on θ_t as a prior table of kind OCTO_PRIOR_NORMAL,
// made and re-made on the device in caller-owned memory, put under the handle's functions in place of its own table, and the exchange of the
// target replicas of two legs that anneal from different references. No model, no random number, no atomic, no allocation.
//
//   k_vref_table      one wave, lane = coordinate (D <= 64): μ and σ from the caller (set) or from one group's moments (fit); a good coordinate's
//                     octo_prior, its four density constants, its four quantile constants, μ and σ are written; a bad one keeps every byte; the
//                     number of bad ones by a ballot.
//   k_vref_exchange   lane = chain: ℓprior_t of each leg's reference at the OTHER leg's target point (prior_loop, no gradient written), then the
//                     D values of θ_t and ℓπ trade places and each side's swap potential is written. A chain's two columns are its lane's alone.
#include "octo_draws_common.h"

namespace {

static_assert(sizeof(octo_prior) == 8 * REF_PRIOR_DOUBLES, "ref_table gives an octo_prior REF_PRIOR_DOUBLES doubles");

inline RefTable table_at(const double* d_ref, int32_t D) { return carve_at(const_cast<double*>(d_ref), ref_table, (int64_t)D, (int64_t)PRIOR_NC, (int64_t)IC_N); }

struct TableArgs {
    const double *count, *mean, *spread;      // [1] or null (set) · [D] · [D]: σ (set) or M2 (fit)
    double inflate;
    int32_t D;
    RefTable t;
    int32_t* bad;                             // [1]
};

__global__ __launch_bounds__(64) void k_vref_table(TableArgs a) {
    const int d = threadIdx.x;
    const bool in = d < a.D;                  // no early exit: the ballot below
    double mu = NAN, sd = NAN;
    bool ok = false;
    if (in) {
        mu = a.mean[d];
        if (a.count) {
            const double n = a.count[0];
            sd = a.inflate * sqrt(a.spread[d] / (n - 1.0));
            ok = n >= 2.0;
        } else {
            sd = a.spread[d];
            ok = true;
        }
        ok = ok && isfinite(mu) && isfinite(sd) && sd > 0.0;
    }
    const unsigned long long bad = __ballot(in && !ok);
    if (d == 0) a.bad[0] = __popcll(bad);
    if (!ok) return;
    octo_prior pr;
    pr.kind = OCTO_PRIOR_NORMAL; pr.pad = 0; pr.p0 = mu; pr.p1 = sd; pr.lo = -INFINITY; pr.hi = INFINITY;
    reinterpret_cast<octo_prior*>(a.t.priors)[d] = pr;
    double* c = a.t.pc + PRIOR_NC * d;        // octo_draws_create's entries of a Normal: {NaN, 1/(b − a) = 0 with both ends open, −log σ, 1/σ}
    c[0] = NAN; c[1] = 0.0; c[2] = -log(sd); c[3] = 1.0 / sd;
    double* q = a.t.ic + IC_N * d;
#pragma unroll
    for (int k = 0; k < IC_N; ++k) q[k] = 0.0;
    a.t.mean[d] = mu;
    a.t.sd[d] = sd;
}

struct Leg {
    const octo_prior* priors;      // [D] the leg's reference
    const double* pc;              // [D][PRIOR_NC]
    const int32_t* slot2rep;       // [Cn][T]
    double *theta, *lp, *ll;       // [D][ld] · [T·Cn] · [T·Cn]
    int64_t ld;
    int32_t T;
};
struct ExchangeArgs {
    Leg a, b;
    int64_t Cn;
    int32_t D;
};

// the swap potential ℓπ − ℓprior_t of a point under a reference: −Inf where it is not finite or the prior was healed
__device__ __forceinline__ double potential(double lp, double lpt, bool healed) {
    const double v = lp - lpt;
    return isfinite(v) && !healed ? v : -INFINITY;
}

__global__ __launch_bounds__(TPB) void k_vref_exchange(ExchangeArgs x) {
    const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool live = c < x.Cn;                         // no early exit: prior_loop votes across the wave
    const int64_t cl = live ? c : x.Cn - 1;
    const int ra = x.a.slot2rep[cl * x.a.T], rb = x.b.slot2rep[cl * x.b.T];
    const bool go = live && ra >= 0 && ra < x.a.T && rb >= 0 && rb < x.b.T;
    // a chain that exchanges nothing reads replica 0's column of its chain: inside both arrays (ld >= T·Cn)
    const int64_t ca = (go ? (int64_t)ra * x.Cn : 0) + cl, cb = (go ? (int64_t)rb * x.Cn : 0) + cl;
    bool healed_a, healed_b;
    const double lpt_a = prior_loop(x.a.priors, x.a.pc, x.D, x.b.theta, x.b.ld, cb, cb, false, nullptr, healed_a);      // A's reference at θ_b
    const double lpt_b = prior_loop(x.b.priors, x.b.pc, x.D, x.a.theta, x.a.ld, ca, ca, false, nullptr, healed_b);      // B's reference at θ_a
    if (!go) return;
    for (int d = 0; d < x.D; ++d) {
        double* pa = x.a.theta + (int64_t)d * x.a.ld + ca;
        double* pb = x.b.theta + (int64_t)d * x.b.ld + cb;
        const double va = *pa, vb = *pb;
        *pa = vb; *pb = va;
    }
    const double lp_a = x.a.lp[ca], lp_b = x.b.lp[cb];
    x.a.lp[ca] = lp_b; x.b.lp[cb] = lp_a;
    x.a.ll[ca] = potential(lp_b, lpt_a, healed_a);
    x.b.ll[cb] = potential(lp_a, lpt_b, healed_b);
}

int launch_table(octo_draws* h, const double* d_count, const double* d_mean, const double* d_spread, double inflate, double* d_ref,
                 int32_t* d_bad, void* hip_stream) {
    OCHK(h, hipSetDevice(h->device));
    TableArgs a;
    a.count = d_count; a.mean = d_mean; a.spread = d_spread; a.inflate = inflate; a.D = h->D; a.t = table_at(d_ref, h->D); a.bad = d_bad;
    hipLaunchKernelGGL(k_vref_table, dim3(1), dim3(64), 0, stream_of(h, hip_stream), a);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // namespace

extern "C" {

int64_t octo_draws_reference_doubles(int32_t D) { return D >= 1 ? carve_size(ref_table, (int64_t)D, (int64_t)PRIOR_NC, (int64_t)IC_N) : 0; }

int32_t octo_draws_reference_set_device(octo_draws* h, const double* d_mean, const double* d_sd, double* d_ref, int32_t* d_bad, void* hip_stream) {
    const char* who = "octo_draws_reference_set_device";
    if (!h) return OCTO_EINVAL;
    if (!d_mean || !d_sd || !d_ref || !d_bad) return fail(h, OCTO_EINVAL, std::string(who) + ": every array is required");
    return launch_table(h, nullptr, d_mean, d_sd, 1.0, d_ref, d_bad, hip_stream);
}

int32_t octo_draws_reference_fit_device(octo_draws* h, const double* d_count_g, const double* d_mean_g, const double* d_m2_g, double inflate, double* d_ref,
                                        int32_t* d_bad, void* hip_stream) {
    const char* who = "octo_draws_reference_fit_device";
    if (!h) return OCTO_EINVAL;
    if (!d_count_g || !d_mean_g || !d_m2_g || !d_ref || !d_bad) return fail(h, OCTO_EINVAL, std::string(who) + ": every array is required");
    if (!(std::isfinite(inflate) && inflate > 0.0)) return fail(h, OCTO_EINVAL, std::string(who) + ": inflate must be finite and > 0");
    return launch_table(h, d_count_g, d_mean_g, d_m2_g, inflate, d_ref, d_bad, hip_stream);
}

int32_t octo_draws_use_reference(octo_draws* h, const double* d_ref) {
    if (!h) return OCTO_EINVAL;
    if (d_ref) {
        const RefTable t = table_at(d_ref, h->D);
        h->d_priors = reinterpret_cast<octo_prior*>(t.priors); h->d_pc = t.pc; h->d_ic = t.ic;
    } else {
        h->d_priors = h->own_priors; h->d_pc = h->own_pc; h->d_ic = h->own_ic;
    }
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->de_open = false;      // a transition is never resumed on another target
    return OCTO_OK;
}

int32_t octo_draws_reference_exchange_device(octo_draws* h, int64_t Cn, int32_t T_a, const int32_t* d_slot2rep_a, int64_t ld_a, double* d_theta_a,
                                             double* d_lp_a, double* d_ll_a, const double* d_ref_a, int32_t T_b, const int32_t* d_slot2rep_b, int64_t ld_b,
                                             double* d_theta_b, double* d_lp_b, double* d_ll_b, const double* d_ref_b, void* hip_stream) {
    const char* who = "octo_draws_reference_exchange_device";
    if (!h) return OCTO_EINVAL;
    if (!d_slot2rep_a || !d_theta_a || !d_lp_a || !d_ll_a || !d_slot2rep_b || !d_theta_b || !d_lp_b || !d_ll_b)
        return fail(h, OCTO_EINVAL, std::string(who) + ": every array but d_ref_a and d_ref_b is required");
    if (T_a < 2 || T_b < 2 || Cn < 1 || Cn > MAX_CHAINS) return fail(h, OCTO_EINVAL, std::string(who) + ": T_a, T_b >= 2 and 1 <= Cn <= 2^30");
    if (ld_a / T_a < Cn || ld_b / T_b < Cn) return fail(h, OCTO_EINVAL, std::string(who) + ": need ld_a >= T_a·Cn and ld_b >= T_b·Cn");
    if (d_theta_a == d_theta_b) return fail(h, OCTO_EINVAL, std::string(who) + ": the two legs must not share their θ_t array");
    OCHK(h, hipSetDevice(h->device));
    ExchangeArgs x;
    const auto leg = [&](const double* d_ref, const int32_t* s2r, double* theta, double* lp, double* ll, int64_t ld, int32_t T) {
        Leg g;
        if (d_ref) { const RefTable t = table_at(d_ref, h->D); g.priors = reinterpret_cast<const octo_prior*>(t.priors); g.pc = t.pc; }
        else { g.priors = h->own_priors; g.pc = h->own_pc; }
        g.slot2rep = s2r; g.theta = theta; g.lp = lp; g.ll = ll; g.ld = ld; g.T = T;
        return g;
    };
    x.a = leg(d_ref_a, d_slot2rep_a, d_theta_a, d_lp_a, d_ll_a, ld_a, T_a);
    x.b = leg(d_ref_b, d_slot2rep_b, d_theta_b, d_lp_b, d_ll_b, ld_b, T_b);
    x.Cn = Cn; x.D = h->D;
    hipLaunchKernelGGL(k_vref_exchange, grid_of(Cn), dim3(TPB), 0, stream_of(h, hip_stream), x);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // extern "C"
