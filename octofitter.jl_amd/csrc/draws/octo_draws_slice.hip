// octo_draws_slice.hip — the slice sampler of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the transition): W chains update
// their coordinates one at a time by Neal's doubling, shrinkage and acceptance test, in lockstep — a round being one FORWARD
// octo_model_logpost_device call at the trial points of all chains and one k_slice_round launch, which takes every chain's state machine one
// evaluation further. Lane = chain, SoA with the chain index fastest. A chain's coordinate d = j mod D is per lane (the chains advance
// independently) and addresses global memory only: x is read from θ_t, the trial value is written into the trial plane, the width is read from
// d_width. Nothing of a chain lives in a private array: its state machine sits in the handle's work array (slice_work of octo_draws_layout.h).
// The prior loop of target_at runs over all D coordinates of the trial point with d wave-uniform, as everywhere else.
//
//   k_slice_open    the start point: E₀, the dead test, the trial plane = θ_t, the level and the interval of update 0, the first trial value L.
//   k_slice_round   E at the trial point, received by the chain's phase (E_L, E_R, a doubled end, the proposal x′, a midpoint of the test), and
//                   the next trial value; a round writes the one trial coordinate that changed, and the restored one when the chain moves on.
//   k_slice_report  the outputs alone: a resumed call of no rounds.
// The last launch of a call writes the outputs. From octo_draws_common.h, as NUTS: SamplerHead, chain_of, target_at, tempered_energy, dead_state,
// check_sampler_call and run_rounds — with no gradient array: the forward callback, and Target::grad is never called.
#include "octo_draws_common.h"

namespace {

// what the evaluation of a launch is: E_L and E_R of the interval, a doubled end, the proposal, an end of the acceptance test's interval
enum { PH_L = 0, PH_R = 1, PH_GROW_L = 2, PH_GROW_R = 3, PH_X = 4, PH_TEST_L = 5, PH_TEST_R = 6 };
// what a chain does with it, in the order k_slice_round walks them
enum { DO_NOTHING = 0, DO_GROW, DO_TEST, DO_REJECT, DO_SHRINK, DO_ACCEPT, DO_MOVE };

// theta_t is read by both kernels (x of the update) and written where an update accepts; eps of the head is the scalar width
struct SliceArgs : SamplerHead {
    int32_t n_updates, p, max_shrink, write_out;      // n_updates = n_passes·D
    const double* width;                              // [D] or null = eps
    SliceWork s;
    double *o_lp, *o_ll;
    int32_t *o_eval, *o_expand, *o_shrink, *o_stuck, *o_status, *o_nact;
};

// the uniforms of words 0 and 1 of the counter (c, j·128 + i, 9, step)
__device__ __forceinline__ void slice_uniforms(const SliceArgs& a, int64_t w, int32_t j, int32_t i, double& u, double& u1) {
    uint64_t r[4];
    philox4x64(a.seed, KEY1, a.chain0 + (uint64_t)w, (uint64_t)j * 128 + (uint64_t)i, OCTO_DRAWS_PURPOSE_SLICE, a.step, r);
    u = u01(r[0]);
    u1 = u01(r[1]);
}

__device__ __forceinline__ double width_at(const SliceArgs& a, int32_t d) { return a.width ? a.width[d] : a.eps; }

// update j opens: the level, the interval around x, and L as the trial value
__device__ __forceinline__ void open_update(const SliceArgs& a, int64_t w, int32_t j) {
    const int32_t d = j % a.D;
    const int64_t o = (int64_t)d * a.ld + w;
    const double wd = width_at(a, d);
    double u, u1;
    slice_uniforms(a, w, j, 0, u, u1);
    const double L = a.theta_t[o] - wd * u1;
    a.s.z[w] = a.s.E0[w] + log(u);
    a.s.L[w] = L;
    a.s.R[w] = L + wd;
    a.s.trial[o] = L;
    a.s.j[w] = j;
    a.s.phase[w] = PH_L;
}

__device__ __forceinline__ void report(const SliceArgs& a, int64_t w) {
    const int32_t status = a.s.status[w];
    if (a.o_lp) a.o_lp[w] = a.s.out_lp[w];
    if (a.o_ll) {
        const double ll = a.s.out_lp[w] - a.s.out_lpt[w];
        a.o_ll[w] = isfinite(ll) ? ll : -INFINITY;
    }
    if (a.o_eval) a.o_eval[w] = a.s.n_eval[w];
    if (a.o_expand) a.o_expand[w] = a.s.n_expand[w];
    if (a.o_shrink) a.o_shrink[w] = a.s.n_shrink[w];
    if (a.o_stuck) a.o_stuck[w] = a.s.n_stuck[w];
    if (a.o_status) a.o_status[w] = status;
    if (a.o_nact && status == OCTO_DRAWS_SLICE_ACTIVE) atomicAdd(a.o_nact, 1);      // an integer count: order-free
}

__global__ __launch_bounds__(TPB) void k_slice_open(SliceArgs a) {
    const Chain ch = chain_of(a);
    const int64_t w = ch.w;
    if (ch.live)      // the trial plane = θ_t, ahead of the prior loop (copied after it, the kernel is given a private segment for its scalar spills)
        for (int d = 0; d < a.D; ++d) {
            const int64_t o = (int64_t)d * a.ld + w;
            a.s.trial[o] = a.theta_t[o];
        }
    const Target tg = target_at(a, ch, a.theta_t, a.s.lp, nullptr, a.s.gpr);      // every lane: its prior_loop() votes across the wave
    if (!ch.live) return;
    const double lp = tg.lp(w), lpt = tg.lpt;
    const double E0 = tempered_energy(ch.beta, lp, lpt);
    const bool dead = dead_state(ch.beta, E0, lp, lpt);
    a.s.E0[w] = E0; a.s.out_lp[w] = lp; a.s.out_lpt[w] = lpt;
    a.s.status[w] = dead ? OCTO_DRAWS_SLICE_DEAD : OCTO_DRAWS_SLICE_ACTIVE;
    a.s.n_eval[w] = 0; a.s.n_expand[w] = 0; a.s.n_shrink[w] = 0; a.s.n_stuck[w] = 0;
    if (!dead) open_update(a, w, 0);      // j and the phase; a dead chain never reads them, nor does any chain read i or the flag ahead of setting them
    if (a.write_out) report(a, w);
}

__global__ __launch_bounds__(TPB) void k_slice_round(SliceArgs a) {
    const Chain ch = chain_of(a);
    const Target tg = target_at(a, ch, a.s.trial, a.s.lp, nullptr, a.s.gpr);      // every lane: its prior_loop() votes across the wave; a frozen chain: at its θ_t, ignored
    if (!ch.live) return;
    const int64_t w = ch.w;
    if (a.s.status[w] == OCTO_DRAWS_SLICE_ACTIVE) {
        const double lp = tg.lp(w), lpt = tg.lpt;
        double E = tempered_energy(ch.beta, lp, lpt);
        if (dead_state(ch.beta, E, lp, lpt)) E = -INFINITY;
        const int32_t j = a.s.j[w], d = j % a.D, phase = a.s.phase[w];
        const int64_t o = (int64_t)d * a.ld + w;
        const double wd = width_at(a, d), z = a.s.z[w];
        double x = a.theta_t[o];
        int32_t i = a.s.i[w], act = DO_NOTHING;
        a.s.n_eval[w] += 1;
        // 1. the evaluation arrives
        if (phase == PH_L) {
            a.s.EL[w] = E;
            a.s.trial[o] = a.s.R[w];
            a.s.phase[w] = PH_R;
        } else if (phase == PH_R || phase == PH_GROW_L || phase == PH_GROW_R) {
            if (phase == PH_GROW_L) a.s.EL[w] = E; else a.s.ER[w] = E;
            i = phase == PH_R ? 1 : i + 1;
            act = DO_GROW;
        } else if (phase == PH_X) {
            a.s.Ep[w] = E; a.s.lpp[w] = lp; a.s.lptp[w] = lpt;
            if (z < E) {      // a candidate: the acceptance test opens on the whole interval
                a.s.Lh[w] = a.s.L[w]; a.s.Rh[w] = a.s.R[w]; a.s.ELh[w] = a.s.EL[w]; a.s.ERh[w] = a.s.ER[w]; a.s.flag[w] = 0;
                act = DO_TEST;
            } else act = DO_REJECT;
        } else {
            if (phase == PH_TEST_L) a.s.ELh[w] = E; else a.s.ERh[w] = E;
            act = a.s.flag[w] != 0 && z >= a.s.ELh[w] && z >= a.s.ERh[w] ? DO_REJECT : DO_TEST;
        }
        // 2. doubling number i, or the interval stands
        if (act == DO_GROW) {
            const double L = a.s.L[w], R = a.s.R[w];
            if (i <= a.p && (z < a.s.EL[w] || z < a.s.ER[w])) {
                double u, u1;
                slice_uniforms(a, w, j, i, u, u1);
                const bool left = u < 0.5;
                const double e = left ? L - (R - L) : R + (R - L);
                if (left) a.s.L[w] = e; else a.s.R[w] = e;
                a.s.trial[o] = e;
                a.s.phase[w] = left ? PH_GROW_L : PH_GROW_R;
                a.s.i[w] = i;
                a.s.n_expand[w] += 1;
            } else {
                a.s.Lb[w] = L; a.s.Rb[w] = R;
                i = 0;
                act = DO_SHRINK;
            }
        }
        // 3. the next midpoint of the acceptance test, or the candidate has passed
        if (act == DO_TEST) {
            const double Lh = a.s.Lh[w], Rh = a.s.Rh[w];
            if (Rh - Lh > 1.1 * wd) {
                const double M = (Lh + Rh) / 2, xp = a.s.xp[w];
                if ((x < M) != (xp < M)) a.s.flag[w] = 1;
                if (xp < M) a.s.Rh[w] = M; else a.s.Lh[w] = M;
                a.s.trial[o] = M;
                a.s.phase[w] = xp < M ? PH_TEST_R : PH_TEST_L;
            } else act = DO_ACCEPT;
        }
        // 4. a proposal that failed shrinks the interval towards x
        if (act == DO_REJECT) {
            const double xp = a.s.xp[w];
            if (xp < x) a.s.Lb[w] = xp; else a.s.Rb[w] = xp;
            i += 1;
            act = DO_SHRINK;
        }
        // 5. shrink proposal number i, or the update is stuck
        if (act == DO_SHRINK) {
            if (i == a.max_shrink) {
                a.s.n_stuck[w] += 1;
                act = DO_MOVE;
            } else {
                double u, u1;
                slice_uniforms(a, w, j, 64 + i, u, u1);
                const double Lb = a.s.Lb[w], Rb = a.s.Rb[w];
                const double xp = Lb + u * (Rb - Lb);
                a.s.xp[w] = xp;
                a.s.trial[o] = xp;
                a.s.phase[w] = PH_X;
                a.s.i[w] = i;
                a.s.n_shrink[w] += 1;
            }
        }
        // 6. the proposal becomes the coordinate, with what was evaluated there
        if (act == DO_ACCEPT) {
            x = a.s.xp[w];
            a.theta_t[o] = x;
            a.s.E0[w] = a.s.Ep[w]; a.s.out_lp[w] = a.s.lpp[w]; a.s.out_lpt[w] = a.s.lptp[w];
            act = DO_MOVE;
        }
        // 7. the trial point takes the coordinate back; the next update opens, or the chain is done
        if (act == DO_MOVE) {
            a.s.trial[o] = x;
            if (j + 1 == a.n_updates) a.s.status[w] = OCTO_DRAWS_SLICE_DONE;
            else open_update(a, w, j + 1);
        }
    }
    if (a.write_out) report(a, w);
}

__global__ __launch_bounds__(TPB) void k_slice_report(SliceArgs a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w < a.W) report(a, w);
}

}  // namespace

extern "C" {

int32_t octo_draws_slice_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t, const double* d_beta,
                                const double* d_width, double w, int32_t p, int32_t n_passes, int32_t max_shrink, int32_t n_rounds, int32_t resume,
                                double* d_logpost, double* d_loglike, int32_t* d_n_eval, int32_t* d_n_expand, int32_t* d_n_shrink, int32_t* d_n_stuck,
                                int32_t* d_status, int32_t* d_n_active, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (!d_width && !(w > 0.0 && std::isfinite(w))) return fail(h, OCTO_EINVAL, "octo_draws_slice_device: w must be finite and > 0 when d_width is NULL");
    if (p < 0 || p > OCTO_DRAWS_SLICE_MAX_DOUBLINGS) return fail(h, OCTO_EINVAL, "octo_draws_slice_device: p must be 0 ... OCTO_DRAWS_SLICE_MAX_DOUBLINGS");
    if (max_shrink < 1 || max_shrink > OCTO_DRAWS_SLICE_MAX_SHRINK) return fail(h, OCTO_EINVAL, "octo_draws_slice_device: max_shrink must be 1 ... OCTO_DRAWS_SLICE_MAX_SHRINK");
    if (n_passes < 1 || n_passes > OCTO_DRAWS_SLICE_MAX_PASSES) return fail(h, OCTO_EINVAL, "octo_draws_slice_device: n_passes must be 1 ... OCTO_DRAWS_SLICE_MAX_PASSES");
    if (n_rounds < 0) return fail(h, OCTO_EINVAL, "octo_draws_slice_device: n_rounds >= 0");
    const bool has_model = has_target(h);
    // the samplers' checks of the chains and of ℓπ outputs without a model; their step-size check has nothing to look at here (the width stands in the head's ε)
    if (int rc = check_sampler_call(h, "octo_draws_slice_device", W, ld, nullptr, 1.0, has_model, d_logpost, d_loglike)) return rc;
    if (resume && (h->slice_passes != n_passes || h->slice_p != p || h->slice_shrink != max_shrink || h->slice_W != W || h->slice_ld != ld || h->slice_seed != seed ||
                   h->slice_step != step || h->slice_chain0 != chain0))
        return fail(h, OCTO_EINVAL, "octo_draws_slice_device: resume needs a previous call with the same W, ld, p, n_passes, max_shrink, seed, step and chain0");
    if (W == 0) {
        if (!resume) h->slice_passes = 0;
        return OCTO_OK;
    }
    if (!d_theta_t) return fail(h, OCTO_EINVAL, "octo_draws_slice_device: d_theta_t is required");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    if (!resume) {
        h->slice_passes = 0;      // a call that fails below leaves nothing to resume
        int rc = grow(h, h->d_slice, h->cap_slice, carve_size(slice_work, (int64_t)h->D, ld)); if (rc) return rc;
    }
    SliceArgs a{sampler_head(h, has_model, seed, step, chain0, W, ld, d_theta_t, d_beta, nullptr, d_width ? 1.0 : w, nullptr)};
    a.n_updates = n_passes * h->D; a.p = p; a.max_shrink = max_shrink;
    a.width = d_width;
    a.s = carve_at(h->d_slice, slice_work, (int64_t)h->D, ld);
    double* lp = a.s.lp;
    if (!has_model) a.s.lp = nullptr;
    a.o_lp = d_logpost; a.o_ll = d_loglike; a.o_eval = d_n_eval; a.o_expand = d_n_expand; a.o_shrink = d_n_shrink; a.o_stuck = d_n_stuck; a.o_status = d_status;
    a.o_nact = d_n_active;
    if (d_n_active) OCHK(h, hipMemsetAsync(d_n_active, 0, sizeof(int32_t), st));      // the last launch of the call counts into it
    if (int rc = run_rounds(h, st, a, has_model, d_theta_t, lp, nullptr, n_rounds, resume != 0, k_slice_open, k_slice_round, k_slice_report)) return rc;
    h->slice_W = W; h->slice_ld = ld; h->slice_passes = n_passes; h->slice_p = p; h->slice_shrink = max_shrink;
    h->slice_seed = seed; h->slice_step = step; h->slice_chain0 = chain0;
    return OCTO_OK;
}

}  // extern "C"
