// octo_draws_lbfgs.hip — the multi-start L-BFGS of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the algorithm):
// W chains minimise f = −ℓπ over θ_t in lockstep, a round being one octo_model_logpost_device call at the trial points of all chains and
// one k_lbfgs_advance launch. Lane = chain, SoA with the chain index fastest (every load and store coalesced); the coordinate index and
// the pair index are wave-uniform loop variables, accept / reject and the ring position are per lane. Nothing of a chain lives in a
// private array: the history, the two-loop coefficients and every scalar of the state sit in the handle's work arrays, and a lane reaches
// its ring slot through an address it computes.
//
//   k_lbfgs_advance<OPEN>    f, g at the start, the dead test, d = −v⊙g, the first trial point.
//   k_lbfgs_advance<ROUND>   the Armijo test at the trial point; on accept the pair, the Pathfinder diagonal, the convergence tests and the
//                            new direction (lbfgs_two_loop); on reject the halved step. The last launch of a call writes the outputs.
//   k_lbfgs_advance<REPORT>  the outputs alone: a resumed call of no rounds.
//   k_lbfgs_direction        lbfgs_two_loop alone on a caller's history (octo_draws_lbfgs_direction_device).
// LbfgsArgs holds the state as octo_draws_layout.h lays it out (a.s). From octo_draws_common.h: the metric v (inv_mass_at) and run_rounds, the
// round driver shared with NUTS, which makes the log-posterior calls and the three launches in their order.
#include "octo_draws_common.h"

namespace {

enum { LB_OPEN = 0, LB_ROUND = 1, LB_REPORT = 2 };
constexpr double LB_C1 = 1e-4, LB_CURV = 1e-10;
constexpr int LB_MAX_BACKTRACKS = 30;

// The two-loop recursion of chain w over its cnt newest pairs, newest first; the pair k steps back from the newest sits in slot
// (head − 1 − k) mod m. H₀ = γ·diag(v), γ = sᵀy/⟨y,y⟩_v of the newest pair (1 with none). q and r live in dir; coef [m][ld] holds the
// first loop's coefficients. sy [m][ld]: sᵀy of every slot. Every sum over d in index order.
__device__ __forceinline__ void lbfgs_two_loop(int32_t D, int32_t m, int64_t ld, int64_t w, int32_t cnt, int32_t head, const double* __restrict__ S,
                                               const double* __restrict__ Y, const double* __restrict__ sy, const double* __restrict__ g,
                                               const double* __restrict__ inv_mass, double* __restrict__ coef, double* __restrict__ dir) {
    const int64_t plane = (int64_t)D * ld;
    for (int d = 0; d < D; ++d) dir[(int64_t)d * ld + w] = g[(int64_t)d * ld + w];
    for (int k = 0; k < m; ++k) {
        if (k >= cnt) continue;
        int32_t slot = head - 1 - k;
        slot += slot < 0 ? m : 0;
        const double* __restrict__ s = S + slot * plane + w;
        const double* __restrict__ y = Y + slot * plane + w;
        double sq = 0.0;
        for (int d = 0; d < D; ++d) sq += s[(int64_t)d * ld] * dir[(int64_t)d * ld + w];
        const double c = sq / sy[(int64_t)slot * ld + w];
        coef[(int64_t)k * ld + w] = c;
        for (int d = 0; d < D; ++d) dir[(int64_t)d * ld + w] -= c * y[(int64_t)d * ld];
    }
    double gamma = 1.0;
    if (cnt > 0) {
        const int32_t newest = head - 1 + (head < 1 ? m : 0);
        const double* __restrict__ y = Y + newest * plane + w;
        double yy = 0.0;
        for (int d = 0; d < D; ++d) {
            const double yd = y[(int64_t)d * ld];
            yy += yd * yd * inv_mass_at(inv_mass, d);
        }
        gamma = sy[(int64_t)newest * ld + w] / yy;
    }
    for (int d = 0; d < D; ++d) dir[(int64_t)d * ld + w] *= gamma * inv_mass_at(inv_mass, d);
    for (int k = m - 1; k >= 0; --k) {
        if (k >= cnt) continue;
        int32_t slot = head - 1 - k;
        slot += slot < 0 ? m : 0;
        const double* __restrict__ s = S + slot * plane + w;
        const double* __restrict__ y = Y + slot * plane + w;
        double yr = 0.0;
        for (int d = 0; d < D; ++d) yr += y[(int64_t)d * ld] * dir[(int64_t)d * ld + w];
        const double c = coef[(int64_t)k * ld + w] - yr / sy[(int64_t)slot * ld + w];
        for (int d = 0; d < D; ++d) dir[(int64_t)d * ld + w] += c * s[(int64_t)d * ld];
    }
    for (int d = 0; d < D; ++d) dir[(int64_t)d * ld + w] = -dir[(int64_t)d * ld + w];
}

struct DirectionArgs {
    const int32_t *cnt, *head;     // [W]
    const double *S, *Y, *g;       // [m][D][ld], [m][D][ld], [D][ld]
    const double* inv_mass;        // [D] or null = 1
    double *sy, *coef;             // [m][ld] of the handle
    double* dir;                   // [D][ld]
    int64_t W, ld;
    int32_t D, m;
};

__global__ __launch_bounds__(TPB) void k_lbfgs_direction(DirectionArgs a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w >= a.W) return;
    const int32_t cnt = min(max(a.cnt[w], 0), a.m);
    const int32_t head = ((a.head[w] % a.m) + a.m) % a.m;
    const int64_t plane = (int64_t)a.D * a.ld;
    for (int slot = 0; slot < a.m; ++slot) {      // sᵀy of every slot the recursion will read
        int32_t back = head - 1 - slot;
        back += back < 0 ? a.m : 0;
        if (back >= cnt) continue;
        double sy = 0.0;
        for (int d = 0; d < a.D; ++d) sy += a.S[slot * plane + (int64_t)d * a.ld + w] * a.Y[slot * plane + (int64_t)d * a.ld + w];
        a.sy[(int64_t)slot * a.ld + w] = sy;
    }
    lbfgs_two_loop(a.D, a.m, a.ld, w, cnt, head, a.S, a.Y, a.sy, a.g, a.inv_mass, a.coef, a.dir);
}

struct LbfgsArgs {
    const double* inv_mass;        // [D] or null = 1
    int64_t W, ld;
    int32_t D, m, write_out;
    double gtol, ftol;
    double* x;                     // [D][ld] the caller's θ_t: read everywhere, written where a chain accepts
    LbfgsState s;                  // glp, lp: ∇ℓπ and ℓπ at the point of this launch
    double *o_lp, *o_gn, *o_ihd;
    int32_t *o_status, *o_iters, *o_evals;
};

// d = −v⊙g into dir; returns gᵀd
__device__ __forceinline__ double steepest(const LbfgsArgs& a, int64_t w) {
    double gd = 0.0;
    for (int d = 0; d < a.D; ++d) {
        const int64_t o = (int64_t)d * a.ld + w;
        const double gv = a.s.g[o], dv = -inv_mass_at(a.inv_mass, d) * gv;
        a.s.dir[o] = dv;
        gd += gv * dv;
    }
    return gd;
}

__device__ __forceinline__ void set_trial(const LbfgsArgs& a, int64_t w, double t, bool moving) {
    for (int d = 0; d < a.D; ++d) {
        const int64_t o = (int64_t)d * a.ld + w;
        a.s.trial[o] = moving ? a.x[o] + t * a.s.dir[o] : a.x[o];
    }
}

template <int PHASE>
__global__ __launch_bounds__(TPB) void k_lbfgs_advance(LbfgsArgs a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w >= a.W) return;
    const int64_t plane = (int64_t)a.D * a.ld;
    if (PHASE == LB_OPEN) {
        const double f = -a.s.lp[w];
        bool fin = isfinite(f);
        double gg = 0.0, gn = 0.0;
        for (int d = 0; d < a.D; ++d) {
            const int64_t o = (int64_t)d * a.ld + w;
            const double v = inv_mass_at(a.inv_mass, d), gv = -a.s.glp[o];
            fin = fin && isfinite(gv);
            a.s.g[o] = gv;
            a.s.alpha[o] = v;
            gg += v * gv * gv;
            gn = fmax(gn, fabs(gv) * sqrt(v));
        }
        a.s.f[w] = f; a.s.gn[w] = fin ? gn : NAN;
        a.s.iters[w] = 0; a.s.evals[w] = 1; a.s.nbt[w] = 0; a.s.cnt[w] = 0; a.s.head[w] = 0;
        a.s.status[w] = fin ? OCTO_DRAWS_LBFGS_ACTIVE : OCTO_DRAWS_LBFGS_DEAD;
        double t = 0.0, gd = 0.0;
        if (fin) {
            gd = steepest(a, w);
            t = fmin(1.0, 1.0 / sqrt(gg));
        }
        a.s.t[w] = t; a.s.gd[w] = gd;
        set_trial(a, w, t, fin);
    } else if (PHASE == LB_ROUND && a.s.status[w] == OCTO_DRAWS_LBFGS_ACTIVE) {
        const double f = a.s.f[w], t = a.s.t[w], ft = -a.s.lp[w];
        bool fin = isfinite(ft);
        for (int d = 0; d < a.D; ++d) fin = fin && isfinite(a.s.glp[(int64_t)d * a.ld + w]);
        a.s.evals[w] += 1;
        if (fin && ft <= f + LB_C1 * t * a.s.gd[w]) {
            double sy = 0.0, ss = 0.0, yy = 0.0, pa = 0.0, pc = 0.0;
            for (int d = 0; d < a.D; ++d) {
                const int64_t o = (int64_t)d * a.ld + w;
                const double v = inv_mass_at(a.inv_mass, d), al = a.s.alpha[o];
                const double s = a.s.trial[o] - a.x[o], y = -a.s.glp[o] - a.s.g[o];
                sy += s * y; ss += s * s / v; yy += y * y * v; pa += y * y * al; pc += s * s / al;
            }
            const bool store = sy > LB_CURV * sqrt(ss * yy);
            int32_t cnt = a.s.cnt[w], head = a.s.head[w];
            double* __restrict__ Ss = a.s.S + head * plane;
            double* __restrict__ Ys = a.s.Y + head * plane;
            double gn = 0.0;
            for (int d = 0; d < a.D; ++d) {
                const int64_t o = (int64_t)d * a.ld + w;
                const double v = inv_mass_at(a.inv_mass, d);
                const double xt = a.s.trial[o], gt = -a.s.glp[o];
                const double s = xt - a.x[o], y = gt - a.s.g[o];
                if (store) {
                    const double al = a.s.alpha[o];
                    Ss[o] = s; Ys[o] = y;
                    a.s.alpha[o] = 1.0 / (pa / (sy * al) + y * y / sy - pa * s * s / (sy * pc * al * al));
                }
                a.x[o] = xt; a.s.g[o] = gt;
                gn = fmax(gn, fabs(gt) * sqrt(v));
            }
            if (store) {
                a.s.sy[(int64_t)head * a.ld + w] = sy;
                head = head + 1 == a.m ? 0 : head + 1;
                cnt = min(cnt + 1, a.m);
            }
            a.s.f[w] = ft; a.s.gn[w] = gn; a.s.iters[w] += 1; a.s.nbt[w] = 0;
            if (gn <= a.gtol) a.s.status[w] = OCTO_DRAWS_LBFGS_GTOL;      // the trial point is x already: a frozen chain's trial point
            else if (a.ftol > 0.0 && fabs(f - ft) <= a.ftol * fmax(1.0, fabs(ft))) a.s.status[w] = OCTO_DRAWS_LBFGS_FTOL;
            else {
                lbfgs_two_loop(a.D, a.m, a.ld, w, cnt, head, a.s.S, a.s.Y, a.s.sy, a.s.g, a.inv_mass, a.s.coef, a.s.dir);
                double gd = 0.0;
                for (int d = 0; d < a.D; ++d) gd += a.s.g[(int64_t)d * a.ld + w] * a.s.dir[(int64_t)d * a.ld + w];
                if (!(gd < 0.0)) { cnt = 0; head = 0; gd = steepest(a, w); }
                a.s.t[w] = 1.0; a.s.gd[w] = gd;
                set_trial(a, w, 1.0, true);
            }
            a.s.cnt[w] = cnt; a.s.head[w] = head;
        } else {
            const int32_t nbt = a.s.nbt[w] + 1;
            const double th = 0.5 * t;
            a.s.nbt[w] = nbt; a.s.t[w] = th;
            const bool failed = nbt > LB_MAX_BACKTRACKS;
            if (failed) a.s.status[w] = OCTO_DRAWS_LBFGS_LINESEARCH;
            set_trial(a, w, th, !failed);
        }
    }
    if (!a.write_out) return;
    a.o_lp[w] = -a.s.f[w]; a.o_gn[w] = a.s.gn[w];
    a.o_status[w] = a.s.status[w]; a.o_iters[w] = a.s.iters[w]; a.o_evals[w] = a.s.evals[w];
    if (a.o_ihd)
        for (int d = 0; d < a.D; ++d) a.o_ihd[(int64_t)d * a.ld + w] = a.s.alpha[(int64_t)d * a.ld + w];
}

}  // namespace

extern "C" {

int32_t octo_draws_lbfgs_direction_device(octo_draws* h, int64_t W, int64_t ld, int32_t m, const int32_t* d_cnt, const int32_t* d_head, const double* d_S,
                                          const double* d_Y, const double* d_g, const double* d_inv_mass, double* d_dir, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (int rc = check_m(h, "octo_draws_lbfgs_direction_device", m)) return rc;
    if (int rc = check_chains(h, "octo_draws_lbfgs_direction_device", W, ld, MAX_CHAINS, "2^30")) return rc;
    if (W == 0) return OCTO_OK;
    if (!d_cnt || !d_head || !d_S || !d_Y || !d_g || !d_dir) return fail(h, OCTO_EINVAL, "octo_draws_lbfgs_direction_device: only d_inv_mass may be NULL");
    OCHK(h, hipSetDevice(h->device));
    LbfgsCoef c;
    if (int rc = grow_to(h, h->d_lbd, h->cap_lbd, c, lbfgs_coef, ld, (int64_t)m)) return rc;
    DirectionArgs a;
    a.cnt = d_cnt; a.head = d_head; a.S = d_S; a.Y = d_Y; a.g = d_g; a.inv_mass = d_inv_mass; a.sy = c.sy; a.coef = c.coef;
    a.dir = d_dir; a.W = W; a.ld = ld; a.D = h->D; a.m = m;
    hipLaunchKernelGGL(k_lbfgs_direction, grid_of(W), dim3(TPB), 0, stream_of(h, hip_stream), a);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_lbfgs_device(octo_draws* h, int64_t W, int64_t ld, double* d_theta_t, const double* d_inv_mass, int32_t m, int32_t n_rounds, double gtol,
                                double ftol, int32_t resume, double* d_logpost, double* d_gnorm, int32_t* d_status, int32_t* d_iters, int32_t* d_evals,
                                double* d_inv_hess_diag, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (int rc = check_model(h, "octo_draws_lbfgs_device")) return rc;
    if (int rc = check_m(h, "octo_draws_lbfgs_device", m)) return rc;
    if (n_rounds < 0) return fail(h, OCTO_EINVAL, "octo_draws_lbfgs_device: n_rounds >= 0");
    if (int rc = check_chains(h, "octo_draws_lbfgs_device", W, ld, MAX_CHAINS, "2^30")) return rc;
    if (int rc = check_tolerances(h, "octo_draws_lbfgs_device", gtol, ftol)) return rc;
    if (resume && (h->lbf_m == 0 || h->lbf_W != W || h->lbf_ld != ld || h->lbf_m != m))
        return fail(h, OCTO_EINVAL, "octo_draws_lbfgs_device: resume needs a previous call with the same W, ld and m");
    if (W == 0) return OCTO_OK;
    if (!d_theta_t || !d_logpost || !d_gnorm || !d_status || !d_iters || !d_evals)
        return fail(h, OCTO_EINVAL, "octo_draws_lbfgs_device: only d_inv_mass and d_inv_hess_diag may be NULL");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    if (!resume) {
        h->lbf_m = 0;      // a call that fails below leaves nothing to resume
        int rc = grow(h, h->d_lbf, h->cap_lbf, carve_size(lbfgs_state, (int64_t)h->D, ld, (int64_t)m)); if (rc) return rc;
    }
    LbfgsArgs a{};
    a.inv_mass = d_inv_mass; a.W = W; a.ld = ld; a.D = h->D; a.m = m; a.gtol = gtol; a.ftol = ftol;
    a.x = d_theta_t;
    a.s = carve_at(h->d_lbf, lbfgs_state, (int64_t)h->D, ld, (int64_t)m);
    a.o_lp = d_logpost; a.o_gn = d_gnorm; a.o_ihd = d_inv_hess_diag; a.o_status = d_status; a.o_iters = d_iters; a.o_evals = d_evals;
    if (int rc = run_rounds(h, st, a, true, d_theta_t, a.s.lp, a.s.glp, n_rounds, resume != 0, k_lbfgs_advance<LB_OPEN>, k_lbfgs_advance<LB_ROUND>,
                            k_lbfgs_advance<LB_REPORT>)) return rc;
    h->lbf_W = W; h->lbf_ld = ld; h->lbf_m = m;
    return OCTO_OK;
}

int32_t octo_draws_lbfgs(octo_draws* h, int64_t W, int64_t ld, double* theta_t, const double* inv_mass, int32_t m, int32_t n_rounds, double gtol, double ftol,
                         double* logpost, double* gnorm, int32_t* status, int32_t* iters, int32_t* evals, double* inv_hess_diag) {
    if (!h) return OCTO_EINVAL;
    if (W < 0 || ld < W) return fail(h, OCTO_EINVAL, "octo_draws_lbfgs: need 0 <= W <= ld");
    if (W > 0 && (!theta_t || !logpost || !gnorm || !status || !iters || !evals))
        return fail(h, OCTO_EINVAL, "octo_draws_lbfgs: only inv_mass and inv_hess_diag may be NULL");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    const int64_t D = h->D, plane = D * ld;
    LbfgsStaging d;
    if (int rc = grow_to(h, h->d_hst, h->cap_hst, d, lbfgs_staging, D, ld)) return rc;
    if (W > 0) OCHK(h, hipMemcpyAsync(d.theta_t, theta_t, sizeof(double) * plane, hipMemcpyHostToDevice, st));
    if (inv_mass) OCHK(h, hipMemcpyAsync(d.inv_mass, inv_mass, sizeof(double) * D, hipMemcpyHostToDevice, st));
    {
        int rc = octo_draws_lbfgs_device(h, W, ld, d.theta_t, inv_mass ? d.inv_mass : nullptr, m, n_rounds, gtol, ftol, 0, d.lp, d.gn, d.status, d.iters, d.evals,
                                         inv_hess_diag ? d.inv_hess_diag : nullptr, OCTO_STREAM_CTX);
        if (rc) return rc;
    }
    if (W == 0) return OCTO_OK;
    OCHK(h, hipMemcpyAsync(theta_t, d.theta_t, sizeof(double) * plane, hipMemcpyDeviceToHost, st));
    if (inv_hess_diag) OCHK(h, hipMemcpyAsync(inv_hess_diag, d.inv_hess_diag, sizeof(double) * plane, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(logpost, d.lp, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(gnorm, d.gn, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(status, d.status, sizeof(int32_t) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(iters, d.iters, sizeof(int32_t) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(evals, d.evals, sizeof(int32_t) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

}  // extern "C"
