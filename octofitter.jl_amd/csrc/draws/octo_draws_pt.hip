// octo_draws_pt.hip — what a parallel-tempering driver does between its scans, in liboctofitter_hip_draws.so (include/octofitter_hip_draws.h,
// "Parallel tempering between the scans", states it): per pair of neighbouring ladder slots the Rao-Blackwellised swap acceptance and the two
// stepping-stone sums over every chain of a scan, the tempered restarts of the index process, and once a round the communication barrier Λ, the
// ladder that equalises the rejection rates along it and the log evidence. Lane = chain. No model, no random number, no floating-point atomic:
// every sum has the order of octo_draws_moments_device (wave_sum, waves_total of octo_draws_common.h).
//
//   k_ptadapt_partials   grid (chain blocks × pairs), one block = 256 chains of one pair: α, the forward and the backward term of every chain; Σα by
//                        a butterfly over the wave and the four waves in wave order; each side's count (a ballot), its block maximum (exact) and
//                        Σ exp(v − maximum) the same way. Stores the seven per (pair, block). The blocks of pair 0 also move the restarts of
//                        their chains: one thread a chain.
//   k_ptadapt_merge      one wave per pair, three lanes at work: Σα, the forward and the backward (count, m, s) over the blocks in block order,
//                        then into the held state.
//   k_ptadapt_schedule   one wave: lane t reads pair t; lane 0 sums Λ, fwd and rev in t order; lane k interpolates β*_k.
// The statistics of a scan are 2 launches, the schedule of a round 1 (after a copy of β [T] to the host, which checks it: the one
// synchronisation, once a round).
#include "octo_draws_common.h"

namespace {

constexpr int WAVES = TPB / 64;
constexpr int MAXT = OCTO_DRAWS_MAX_GROUPS;
constexpr int64_t MAX_PT_CHAINS = (int64_t)1 << 24;

struct StatsArgs {
    const double* ll;              // [T][Cn] by replica
    const int32_t* slot2rep;       // [Cn][T]
    const double* beta;            // [T]
    int64_t Cn, nblk;
    int32_t T;
    PtPartials p;
    int32_t *leg, *restarts;       // [Cn][T] by replica, [Cn]; both or neither
};

// the maximum over the 64 lanes, the same bits in every lane (−Inf where a lane has nothing; no NaN is ever passed)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(TPB) void k_ptadapt_partials(StatsArgs a) {
    __shared__ double s_A[WAVES], s_nf[WAVES], s_nb[WAVES], s_mf[WAVES], s_mb[WAVES], s_sf[WAVES], s_sb[WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, t = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * TPB + tid;
    const bool live = c < a.Cn;                         // no early exit: ballots, shuffles and barriers below
    double li = NAN, lj = NAN;                          // a lane beyond the batch, and a replica index outside 0 … T − 1: excluded everywhere
    if (live) {
        const int32_t* s2r = a.slot2rep + c * a.T;
        const int ri = s2r[t], rj = s2r[t + 1];
        if (ri >= 0 && ri < a.T) li = a.ll[(int64_t)ri * a.Cn + c];
        if (rj >= 0 && rj < a.T) lj = a.ll[(int64_t)rj * a.Cn + c];
        if (t == 0 && a.leg) {                          // the restarts: this chain's row of leg and its count are this thread's alone
            const int rc = s2r[a.T - 1];
            if (rc >= 0 && rc < a.T) a.leg[c * a.T + rc] = 1;
            if (ri >= 0 && ri < a.T && a.leg[c * a.T + ri] == 1) {
                a.restarts[c] += 1;
                a.leg[c * a.T + ri] = 0;
            }
        }
    }
    const double bt = a.beta[t], bn = a.beta[t + 1], db = bt - bn;
    const bool fi = isfinite(li), fj = isfinite(lj);
    double alpha = 0.0;
    if (live) alpha = fi && fj ? fmin(1.0, exp(db * (lj - li))) : (fj && !fi && bt > bn ? 1.0 : 0.0);
    // lj = −Inf, a dead prior draw at the cold end, counts in n_f and adds exp(−Inf) = 0: decided before the multiply, db = 0 gives no NaN
    const double vf = fj ? db * lj : -INFINITY, vb = fi ? -db * li : -INFINITY;
    const double wA = wave_sum(alpha), wmf = wave_max(vf), wmb = wave_max(vb);
    const unsigned long long bf = __ballot(fj || lj == -INFINITY), bb = __ballot(fi);
    if (lane == 0) {
        s_A[wave] = wA; s_mf[wave] = wmf; s_mb[wave] = wmb;
        s_nf[wave] = (double)__popcll(bf); s_nb[wave] = (double)__popcll(bb);
    }
    __syncthreads();
    double mf = s_mf[0], mb = s_mb[0];
#pragma unroll
    for (int q = 1; q < WAVES; ++q) { mf = fmax(mf, s_mf[q]); mb = fmax(mb, s_mb[q]); }
    const double wsf = wave_sum(fj ? exp(vf - mf) : 0.0), wsb = wave_sum(fi ? exp(vb - mb) : 0.0);
    if (lane == 0) { s_sf[wave] = wsf; s_sb[wave] = wsb; }
    __syncthreads();
    if (tid != 0) return;
    const int64_t o = (int64_t)t * a.nblk + blockIdx.x;
    a.p.A[o] = waves_total(s_A);
    a.p.nf[o] = waves_total(s_nf); a.p.mf[o] = mf; a.p.sf[o] = waves_total(s_sf);
    a.p.nb[o] = waves_total(s_nb); a.p.mb[o] = mb; a.p.sb[o] = waves_total(s_sb);
}

struct MergeArgs {
    PtPartials p;
    int64_t Cn, nblk;
    double* acc;                   // [T − 1][8]
};

// (n, m, s) merged with (nb, mb, sb): the counts add; a side without a term (m = −Inf) leaves the other's (m, s) untouched
__device__ __forceinline__ void lse_merge(double& n, double& m, double& s, double nb, double mb, double sb) {
    n += nb;
    if (mb == -INFINITY) return;
    if (m == -INFINITY) { m = mb; s = sb; return; }
    const double mm = fmax(m, mb);
    s = s * exp(m - mm) + sb * exp(mb - mm);
    m = mm;
}

__global__ __launch_bounds__(64) void k_ptadapt_merge(MergeArgs a) {
    const int lane = threadIdx.x;
    if (lane > 2) return;
    const int64_t o = (int64_t)blockIdx.x * a.nblk;
    double* acc = a.acc + 8 * (int64_t)blockIdx.x;
    if (lane == 0) {
        double A = 0.0;
        for (int64_t b = 0; b < a.nblk; ++b) A += a.p.A[o + b];
        acc[0] += (double)a.Cn;
        acc[1] += A;
        return;
    }
    const double *pn = lane == 1 ? a.p.nf : a.p.nb, *pm = lane == 1 ? a.p.mf : a.p.mb, *ps = lane == 1 ? a.p.sf : a.p.sb;
    double n = 0.0, m = -INFINITY, s = 0.0;
    for (int64_t b = 0; b < a.nblk; ++b) lse_merge(n, m, s, pn[o + b], pm[o + b], ps[o + b]);
    double* h = acc + (lane == 1 ? 2 : 5);
    double hn = h[0], hm = h[1], hs = h[2];
    lse_merge(hn, hm, hs, n, m, s);
    h[0] = hn; h[1] = hm; h[2] = hs;
}

struct ScheduleArgs {
    double* acc;                   // [T − 1][8]
    const double* beta;            // [T]
    int32_t T, adapt, reset;
    double *beta_out, *rej, *summary;      // [T] (may be beta), [T − 1], [4]
};

__global__ __launch_bounds__(64) void k_ptadapt_schedule(ScheduleArgs a) {
    __shared__ double s_beta[MAXT], s_r[MAXT], s_lam[MAXT], s_f[MAXT], s_b[MAXT];
    const int k = threadIdx.x, T = a.T;
    if (k < T) s_beta[k] = a.beta[k];
    if (k < T - 1) {
        double* q = a.acc + 8 * k;
        const double n = q[0], A = q[1];
        const double r = n > 0.0 ? fmin(fmax(1.0 - A / n, 0.0), 1.0) : NAN;
        s_r[k] = r;
        s_f[k] = q[3] + log(q[4] / q[2]);
        s_b[k] = q[6] + log(q[7] / q[5]);
        a.rej[k] = r;
        if (a.reset) {
            q[0] = 0.0; q[1] = 0.0; q[2] = 0.0; q[3] = -INFINITY; q[4] = 0.0; q[5] = 0.0; q[6] = -INFINITY; q[7] = 0.0;
        }
    }
    __syncthreads();
    if (k == 0) {
        double lam = 0.0, fwd = 0.0, rev = 0.0;
        s_lam[0] = 0.0;
        for (int t = 0; t < T - 1; ++t) {
            lam += s_r[t];
            s_lam[t + 1] = lam;
            fwd += s_f[t];
            rev += s_b[t];
        }
        rev = -rev;
        a.summary[0] = lam; a.summary[1] = fwd; a.summary[2] = rev; a.summary[3] = 0.5 * (fwd + rev);
    }
    __syncthreads();
    if (k >= T) return;
    const double lam = s_lam[T - 1];
    double b = s_beta[k];                               // the end slots, and every slot when no schedule is made, keep their bits
    if (a.adapt && k >= 1 && k <= T - 2 && isfinite(lam) && lam > 0.0) {
        const double g = (double)k * lam / (double)(T - 1);
        int t = 0;
        while (t < T - 2 && !(s_lam[t + 1] >= g)) ++t;  // the first t with Λ_{t+1} >= g: Λ_t < g there, the denominator is positive
        b = s_beta[t] + (s_beta[t + 1] - s_beta[t]) * (g - s_lam[t]) / (s_lam[t + 1] - s_lam[t]);
    }
    a.beta_out[k] = b;
}

inline int check_shape(octo_draws* h, const char* who, int32_t T, int64_t Cn) {
    if (T < 2 || T > OCTO_DRAWS_MAX_GROUPS) return fail(h, OCTO_EINVAL, std::string(who) + ": T must be 2 ... OCTO_DRAWS_MAX_GROUPS");
    return Cn >= 1 && Cn <= MAX_PT_CHAINS ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": Cn must be 1 ... 2^24");
}

}  // namespace

extern "C" {

int32_t octo_draws_pt_stats_device(octo_draws* h, int32_t T, int64_t Cn, const double* d_ll, const int32_t* d_slot2rep, const double* d_beta,
                                   double* d_acc, int32_t* d_leg, int32_t* d_restarts, void* hip_stream) {
    const char* who = "octo_draws_pt_stats_device";
    if (!h) return OCTO_EINVAL;
    if (!d_ll || !d_slot2rep || !d_beta || !d_acc) return fail(h, OCTO_EINVAL, std::string(who) + ": d_ll, d_slot2rep, d_beta and d_acc are required");
    if ((d_leg == nullptr) != (d_restarts == nullptr)) return fail(h, OCTO_EINVAL, std::string(who) + ": d_leg and d_restarts are given together or not at all");
    if (int rc = check_shape(h, who, T, Cn)) return rc;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    StatsArgs a;
    a.ll = d_ll; a.slot2rep = d_slot2rep; a.beta = d_beta; a.Cn = Cn; a.nblk = (Cn + TPB - 1) / TPB; a.T = T; a.leg = d_leg; a.restarts = d_restarts;
    if (int rc = grow_to(h, h->d_mom, h->cap_mom, a.p, pt_partials, (int64_t)(T - 1), a.nblk)) return rc;
    hipLaunchKernelGGL(k_ptadapt_partials, dim3((unsigned)a.nblk, (unsigned)(T - 1)), dim3(TPB), 0, st, a);
    MergeArgs m;
    m.p = a.p; m.Cn = Cn; m.nblk = a.nblk; m.acc = d_acc;
    hipLaunchKernelGGL(k_ptadapt_merge, dim3((unsigned)(T - 1)), dim3(64), 0, st, m);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_pt_schedule_device(octo_draws* h, int32_t T, double* d_acc, const double* d_beta, int32_t adapt, int32_t reset, double* d_beta_out,
                                      double* d_rej, double* d_summary, void* hip_stream) {
    const char* who = "octo_draws_pt_schedule_device";
    if (!h) return OCTO_EINVAL;
    if (!d_acc || !d_beta || !d_beta_out || !d_rej || !d_summary) return fail(h, OCTO_EINVAL, std::string(who) + ": every array is required");
    if (int rc = check_shape(h, who, T, 1)) return rc;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    double beta[MAXT];
    OCHK(h, hipMemcpyAsync(beta, d_beta, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    for (int t = 0; t + 1 < T; ++t)
        if (!(beta[t] >= beta[t + 1])) return fail(h, OCTO_EINVAL, std::string(who) + ": d_beta must be non-increasing from slot 0 (and hold no NaN)");
    ScheduleArgs a;
    a.acc = d_acc; a.beta = d_beta; a.T = T; a.adapt = adapt ? 1 : 0; a.reset = reset ? 1 : 0; a.beta_out = d_beta_out; a.rej = d_rej; a.summary = d_summary;
    hipLaunchKernelGGL(k_ptadapt_schedule, dim3(1), dim3(64), 0, st, a);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // extern "C"
