// octo_draws.hip — liboctofitter_hip_draws.so: prior draws on the device and the two batched drivers on top of them
// (include/octofitter_hip_draws.h). A client of the public C ABI: log-posteriors come from octo_model_logpost_device; of the
// main library's sources it includes only the device helpers of octo_model.h (prior_bounds, prior_link_lanes,
// prior_density_lanes), so the prior term it subtracts in the rejection driver is the code the model callback ran.
//
//   k_draw      one thread = one draw, one launch = one Philox block of four coordinates: uniform -> inverse CDF -> link -> density.
//               Store bound: 16·D + 8 bytes per draw, every store coalesced (draw index fastest).
//   k_topk      the `keep` best (log-posterior descending, draw index ascending: a TOTAL order, so the result is a set
//               operation — independent of grid, slab and chunk size) of a slab, by `keep` rounds of a block-wide arg-best:
//               wave shuffles -> LDS -> one partial list per block; the same kernel as ONE block merges the partial lists
//               and the running list. No atomics.
//   k_loglike   ll = lp − logprior_t (non-finite -> −Inf) and the per-block maximum; k_max the maximum of those.
//   k_count / k_scan / k_scatter   accept flags (recomputed, never stored), per-block counts, their exclusive scan, ordered scatter.
// The handle, the counter generator and the prior helpers are in octo_draws_common.h, shared with the other units.
#include "octo_draws_common.h"

namespace {

constexpr int64_t CHUNK = 1 << 18;                    // draws per log-posterior call (a multiple of TPB)
constexpr int SEL_EPT = 17;                           // candidates per thread of k_topk
constexpr int64_t SEL_SLAB = (int64_t)TPB * SEL_EPT;  // 4352 per block: 61 blocks per chunk, and (61 + 1)·64 candidates fit the merging block
constexpr int64_t SEL_BLOCKS = (CHUNK + SEL_SLAB - 1) / SEL_SLAB;
constexpr uint64_t NO_INDEX = ~0ull;
constexpr int64_t SEL_LISTS = (1 + SEL_BLOCKS) * OCTO_DRAWS_MAX_KEEP;      // list 0 = the running list
static_assert(SEL_LISTS <= SEL_SLAB, "the merging block must hold every partial list and the running list");
static_assert(CHUNK % TPB == 0, "chunk boundaries are block boundaries of the rejection pass");

__device__ __forceinline__ double rejection_uniform(uint64_t seed, uint64_t i) {
    uint64_t r[4];
    philox4x64(seed, KEY1, i, 0, OCTO_DRAWS_PURPOSE_UNIFORM, 0, r);
    return u01(r[0]);
}

// One launch = one Philox block of four coordinates [d0, d0 + 4) ∩ [0, D); the host walks the blocks (launch_draw). A loop over the coordinates
// INSIDE the kernel was tried first: the compiler hoists the ~230 polynomial coefficients of normcdfinv / exp / log / log1p / acos out of it into
// registers (480 VGPRs + AGPRs, one wave per SIMD; held to 128 it spilled 348 of them). Without a loop there is nothing to hoist them out of.
// logprior_t is carried through a.lpt from launch to launch, added in declaration order: the model callback's own order of summation.
__global__ __launch_bounds__(TPB) void k_draw(DrawArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool live = t < a.n;                        // no early exit: prior_density_lanes votes across the wave
    const int64_t tl = live ? t : a.n - 1;
    const uint64_t i = a.idx ? a.idx[tl] : a.first + (uint64_t)tl;
    uint64_t r[4];
    philox4x64(a.seed, KEY1, i, (uint64_t)(a.d0 >> 2), OCTO_DRAWS_PURPOSE_PRIOR, 0, r);
    const double u[4] = {u01(r[0]), u01(r[1]), u01(r[2]), u01(r[3])};
    draw_block(a, t, tl, live, u, false);      // octo_draws_common.h: shared with the hypercube transform
}

// ---- selection ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool better(double lp1, uint64_t i1, double lp2, uint64_t i2) { return lp1 > lp2 || (lp1 == lp2 && i1 < i2); }

// Block b lists the `keep` best of candidates [b·SEL_SLAB, min(n, (b+1)·SEL_SLAB)) at out[(out_first + b)·keep …], best first; places without
// a candidate hold (−Inf, NO_INDEX). idx = null: candidate k is draw base + k. A candidate with a non-finite lp is none.
// One block may run in place on out (every candidate is in a register before the first barrier; the first store follows it).
__global__ __launch_bounds__(TPB) void k_topk(const double* lp, const uint64_t* idx, uint64_t base, int64_t n, int32_t keep,
                                              int64_t out_first, double* out_lp, uint64_t* out_idx) {
    __shared__ double s_lp[2][TPB / WAVE];
    __shared__ uint64_t s_ix[2][TPB / WAVE];
    const int64_t lo = (int64_t)blockIdx.x * SEL_SLAB;
    double v[SEL_EPT];
    uint64_t ix[SEL_EPT];
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e) {
        const int64_t k = lo + (int64_t)e * TPB + threadIdx.x;
        const bool in = k < n;
        const double x = in ? lp[k] : NAN;
        v[e] = isfinite(x) ? x : NAN;
        ix[e] = in ? (idx ? idx[k] : base + (uint64_t)k) : NO_INDEX;
    }
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    double prev_lp = INFINITY;
    uint64_t prev_ix = 0;
    for (int r = 0; r < keep; ++r) {
        double b_lp = -INFINITY;
        uint64_t b_ix = NO_INDEX;
#pragma unroll
        for (int e = 0; e < SEL_EPT; ++e) {
            // still to be listed = strictly after the previous winner in the order (NaN compares false: never a candidate)
            const bool cand = better(prev_lp, prev_ix, v[e], ix[e]) && better(v[e], ix[e], b_lp, b_ix);
            b_lp = cand ? v[e] : b_lp;
            b_ix = cand ? ix[e] : b_ix;
        }
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) {
            const double o_lp = __shfl_xor(b_lp, m, WAVE);
            const uint64_t o_ix = (uint64_t)__shfl_xor((unsigned long long)b_ix, m, WAVE);
            const bool take = better(o_lp, o_ix, b_lp, b_ix);
            b_lp = take ? o_lp : b_lp;
            b_ix = take ? o_ix : b_ix;
        }
        const int buf = r & 1;                          // two buffers: one barrier per round
        if (lane == 0) { s_lp[buf][wv] = b_lp; s_ix[buf][wv] = b_ix; }
        __syncthreads();
        b_lp = s_lp[buf][0]; b_ix = s_ix[buf][0];
#pragma unroll
        for (int w = 1; w < TPB / WAVE; ++w) {
            const double o_lp = s_lp[buf][w];
            const uint64_t o_ix = s_ix[buf][w];
            const bool take = better(o_lp, o_ix, b_lp, b_ix);
            b_lp = take ? o_lp : b_lp;
            b_ix = take ? o_ix : b_ix;
        }
        if (threadIdx.x == 0) {
            const int64_t o = (out_first + blockIdx.x) * keep + r;
            out_lp[o] = b_lp; out_idx[o] = b_ix;
        }
        if (b_ix == NO_INDEX) { prev_lp = -INFINITY; prev_ix = NO_INDEX; }      // exhausted: nothing is after this
        else { prev_lp = b_lp; prev_ix = b_ix; }
    }
}

// ---- rejection ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_max(double m, double* s) {
#pragma unroll
    for (int k = WAVE / 2; k >= 1; k >>= 1) m = fmax(m, __shfl_xor(m, k, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = m;
    __syncthreads();
    m = s[0];
#pragma unroll
    for (int w = 1; w < TPB / WAVE; ++w) m = fmax(m, s[w]);
    return m;
}

// ll[k] = lp[k] − lpt[k] (sampling.jl:260-268: non-finite -> −Inf), pmax[block] = its maximum over the block
__global__ __launch_bounds__(TPB) void k_loglike(const double* __restrict__ lp, const double* __restrict__ lpt, int64_t n, double* __restrict__ ll, double* __restrict__ pmax) {
    __shared__ double s[TPB / WAVE];
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double v = -INFINITY;
    if (k < n) {
        v = lp[k] - lpt[k];
        v = isfinite(v) ? v : -INFINITY;
        ll[k] = v;
    }
    v = block_max(v, s);
    if (threadIdx.x == 0) pmax[blockIdx.x] = v;
}

__global__ __launch_bounds__(TPB) void k_max(const double* __restrict__ pmax, int64_t n, double* __restrict__ out) {
    __shared__ double s[TPB / WAVE];
    double v = -INFINITY;
    for (int64_t k = threadIdx.x; k < n; k += TPB) v = fmax(v, pmax[k]);
    v = block_max(v, s);
    if (threadIdx.x == 0) *out = v;
}

// sampling.jl:202-210
__device__ __forceinline__ bool accepted(double ll, double mx, uint64_t seed, uint64_t i) {
    return ll != -INFINITY && rejection_uniform(seed, i) < exp(ll - mx);
}

__global__ __launch_bounds__(TPB) void k_count(const double* __restrict__ ll, int64_t n, const double* __restrict__ mx, uint64_t seed, uint64_t first, int64_t* __restrict__ cnt) {
    __shared__ int s[TPB / WAVE];
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool f = k < n && accepted(ll[k], *mx, seed, first + (uint64_t)k);
    const int c = __popcll(__ballot(f));
    if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < TPB / WAVE; ++w) tot += s[w];
        cnt[blockIdx.x] = tot;
    }
}

// exclusive scan of cnt[0 … n) in place, the total at cnt[n]: one block, a contiguous segment per thread
__global__ __launch_bounds__(TPB) void k_scan(int64_t* cnt, int64_t n) {
    __shared__ int64_t s[TPB];
    const int64_t seg = (n + TPB - 1) / TPB, lo = (int64_t)threadIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    int64_t sum = 0;
    for (int64_t k = lo; k < hi; ++k) sum += cnt[k];
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int step = 1; step < TPB; step <<= 1) {      // Hillis-Steele, inclusive
        const int64_t add = (int)threadIdx.x >= step ? s[threadIdx.x - step] : 0;
        __syncthreads();
        s[threadIdx.x] += add;
        __syncthreads();
    }
    int64_t run = s[threadIdx.x] - sum;
    for (int64_t k = lo; k < hi; ++k) { const int64_t c = cnt[k]; cnt[k] = run; run += c; }
    if (threadIdx.x == TPB - 1) cnt[n] = s[TPB - 1];
}

__global__ __launch_bounds__(TPB) void k_scatter(const double* __restrict__ ll, const double* __restrict__ lp, int64_t n, const double* __restrict__ mx, uint64_t seed,
                                                 uint64_t first, const int64_t* __restrict__ offs, int64_t cap, uint64_t* __restrict__ o_idx,
                                                 double* __restrict__ o_ll, double* __restrict__ o_lp) {
    __shared__ int s[TPB / WAVE];
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const double v = k < n ? ll[k] : -INFINITY;
    const bool f = k < n && accepted(v, *mx, seed, first + (uint64_t)k);
    const unsigned long long mask = __ballot(f);
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    if (lane == 0) s[wv] = __popcll(mask);
    __syncthreads();
    int64_t pos = offs[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) pos += s[w];
    if (f && pos < cap) { o_idx[pos] = first + (uint64_t)k; o_ll[pos] = v; o_lp[pos] = lp[k]; }
}

// The three groups of work arrays, each one allocation laid out by its function of octo_draws_layout.h and kept while it is large enough
// (a failed growth leaves the group empty): the chunk buffers, the per-draw arrays of n draws, the outputs of n draws.
int ensure_chunk(octo_draws* h, ChunkBufs& k) { return grow_to(h, h->d_chunk, h->cap_chunk, k, chunk_bufs, (int64_t)h->D, CHUNK, SEL_LISTS); }
int ensure_draw_arrays(octo_draws* h, int64_t n, DrawArrays& a) { return grow_to(h, h->d_arr, h->cap_arr, a, draw_arrays, n, (n + TPB - 1) / TPB); }
int ensure_outputs(octo_draws* h, int64_t n, Outputs& o) { return grow_to(h, h->d_out, h->cap_out, o, outputs, (int64_t)h->D, n); }

// draws [first, first + n) or the listed ones, enqueued on st in launches of at most 2³⁰ draws
int launch_draw(octo_draws* h, hipStream_t st, uint64_t seed, uint64_t first, const uint64_t* d_idx, int64_t n, int64_t ld,
                double* d_theta, double* d_theta_t, double* d_lpt) {
    constexpr int64_t PIECE = (int64_t)1 << 30;
    for (int64_t o = 0; o < n; o += PIECE) {
        DrawArgs a;
        std::memset(&a, 0, sizeof(a));
        a.priors = h->d_priors; a.pc = h->d_pc; a.ic = h->d_ic; a.D = h->D;
        a.idx = d_idx ? d_idx + o : nullptr;
        a.seed = seed; a.first = first + (uint64_t)o;
        a.n = std::min(PIECE, n - o); a.ld = ld;
        a.theta = d_theta ? d_theta + o : nullptr; a.theta_t = d_theta_t ? d_theta_t + o : nullptr; a.lpt = d_lpt ? d_lpt + o : nullptr;
        for (a.d0 = 0; a.d0 < h->D; a.d0 += 4) hipLaunchKernelGGL(k_draw, grid_of(a.n), dim3(TPB), 0, st, a);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int check_range(octo_draws* h, const char* who, uint64_t first, int64_t N, bool need_model) {
    if (N < 1) return fail(h, OCTO_EINVAL, std::string(who) + ": N >= 1");
    if (first + (uint64_t)N < first) return fail(h, OCTO_EINVAL, std::string(who) + ": first + N overflows the draw index");
    return need_model ? check_model(h, who) : OCTO_OK;
}

double normcdf_host(double z) { return 0.5 * std::erfc(-z * 0.70710678118654752440); }

}  // namespace

// ---- what the OFTI driver (octo_draws_ofti.hip) takes from this unit, declared in octo_draws_common.h: the draw launches and pass 2 of the
// rejection — the kernels of octo_draws_rejection, launched as it launches them
int draws_launch_draw(octo_draws* h, hipStream_t st, uint64_t seed, uint64_t first, const uint64_t* d_idx, int64_t n, int64_t ld, double* d_theta) {
    return launch_draw(h, st, seed, first, d_idx, n, ld, d_theta, nullptr, nullptr);
}

// The two halves of pass 2, written once for octo_draws_rejection and the OFTI driver (a caller sizes its outputs between them). The maximum of the
// block maxima, on the host too, and the refusal when every ℓ is −Inf:
int draws_max_pass(octo_draws* h, hipStream_t st, const double* pmax, int64_t N, double* d_max, double* mx_out) {
    hipLaunchKernelGGL(k_max, dim3(1), dim3(TPB), 0, st, pmax, (N + TPB - 1) / TPB, d_max);
    OCHK(h, hipGetLastError());
    double mx = 0.0;
    OCHK(h, hipMemcpyAsync(&mx, d_max, sizeof(double), hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    if (mx_out) *mx_out = mx;
    if (!std::isfinite(mx))      // sampling.jl:194-197
        return fail(h, OCTO_EINVAL, "All " + std::to_string(N) + " prior samples produced non-finite log-likelihoods. Check your model and priors.");
    return OCTO_OK;
}

// flags -> block counts -> offsets -> ordered scatter of at most `room` accepted draws, and the full count
int draws_accept_pass(octo_draws* h, hipStream_t st, const double* ll, const double* lp, int64_t N, const double* d_max, uint64_t seed, uint64_t first,
                      int64_t* cnt, int64_t room, uint64_t* o_ix, double* o_ll, double* o_lp, int64_t* total_out) {
    const int64_t nblk = (N + TPB - 1) / TPB;
    hipLaunchKernelGGL(k_count, grid_of(N), dim3(TPB), 0, st, ll, N, d_max, seed, first, cnt);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(TPB), 0, st, cnt, nblk);
    hipLaunchKernelGGL(k_scatter, grid_of(N), dim3(TPB), 0, st, ll, lp, N, d_max, seed, first, cnt, room, o_ix, o_ll, o_lp);
    OCHK(h, hipGetLastError());
    OCHK(h, hipMemcpyAsync(total_out, cnt + nblk, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

extern "C" {

int32_t octo_draws_create(octo_ctx* ctx, octo_model* model, const octo_prior* priors, int32_t D, int32_t device_id, octo_draws** out) {
    if (!ctx || !priors || !out) return fail(nullptr, OCTO_EINVAL, "octo_draws_create: null argument");
    *out = nullptr;
    if (D < 1 || D > 64) return fail(nullptr, OCTO_EINVAL, "octo_draws_create: 1 <= D <= 64");
    for (int k = 0; k < D; ++k) {
        const octo_prior& pr = priors[k];
        if (pr.kind < OCTO_PRIOR_UNIFORM || pr.kind > OCTO_PRIOR_SINE) return fail(nullptr, OCTO_EINVAL, "octo_draws_create: unknown prior kind");
        const bool ok = (pr.kind == OCTO_PRIOR_UNIFORM) ? (std::isfinite(pr.p0) && std::isfinite(pr.p1) && pr.p0 < pr.p1)
                      : (pr.kind == OCTO_PRIOR_LOGUNIFORM) ? (std::isfinite(pr.p1) && 0.0 < pr.p0 && pr.p0 < pr.p1)
                      : (pr.kind == OCTO_PRIOR_NORMAL) ? (std::isfinite(pr.p0) && std::isfinite(pr.p1) && pr.p1 > 0.0)
                      : (pr.kind == OCTO_PRIOR_TRUNCNORMAL) ? (std::isfinite(pr.p0) && std::isfinite(pr.p1) && pr.p1 > 0.0 && pr.lo < pr.hi)
                      : true;
        if (!ok) return fail(nullptr, OCTO_EINVAL, "octo_draws_create: prior " + std::to_string(k) + " has no proper support");
    }
    // constants of each prior: pc as octo_model_create forms them for prior_density_lanes (−log(Φ(hi) − Φ(lo)), 1/(b − a),
    // −log(b − a) | log(b/a) | −log σ, 1/σ), ic for prior_quantile
    std::vector<double> pc((size_t)D * PRIOR_NC, std::nan("")), ic((size_t)D * IC_N, 0.0);
    for (int k = 0; k < D; ++k) {
        const octo_prior& pr = priors[k];
        double* c = &pc[(size_t)k * PRIOR_NC];
        double* q = &ic[(size_t)k * IC_N];
        double a = -INFINITY, b = INFINITY;
        if (pr.kind == OCTO_PRIOR_UNIFORM || pr.kind == OCTO_PRIOR_LOGUNIFORM) { a = pr.p0; b = pr.p1; }
        else if (pr.kind == OCTO_PRIOR_TRUNCNORMAL) { a = pr.lo; b = pr.hi; }
        else if (pr.kind == OCTO_PRIOR_SINE) { a = 0.0 + 2.220446049250313e-16; b = PI - 2.220446049250313e-16; }
        c[1] = 1.0 / (b - a);
        if (pr.kind == OCTO_PRIOR_UNIFORM) { c[2] = -std::log(b - a); q[0] = a; q[1] = b - a; }
        else if (pr.kind == OCTO_PRIOR_LOGUNIFORM) { c[2] = std::log(b / a); q[0] = std::log(a); q[1] = std::log(b) - std::log(a); }
        else if (pr.kind == OCTO_PRIOR_NORMAL || pr.kind == OCTO_PRIOR_TRUNCNORMAL) { c[2] = -std::log(pr.p1); c[3] = 1.0 / pr.p1; }
        if (pr.kind == OCTO_PRIOR_TRUNCNORMAL) {
            const double lo = std::isfinite(pr.lo) ? normcdf_host((pr.lo - pr.p0) / pr.p1) : 0.0;
            const double hi = std::isfinite(pr.hi) ? normcdf_host((pr.hi - pr.p0) / pr.p1) : 1.0;
            c[0] = -std::log(hi - lo);
            const double al = (pr.lo - pr.p0) / pr.p1, be = (pr.hi - pr.p0) / pr.p1;      // ±Inf at an open end
            if (al < 0.0) { q[0] = lo; q[1] = hi - lo; q[2] = 0.0; }
            else { q[0] = normcdf_host(-al); q[1] = q[0] - (std::isfinite(be) ? normcdf_host(-be) : 0.0); q[2] = 1.0; }
            if (!(q[1] > 0.0)) return fail(nullptr, OCTO_EINVAL, "octo_draws_create: prior " + std::to_string(k) + ": the truncation leaves no probability in double precision");
        }
    }
    octo_draws* h;
    { int rc = open_device(device_id, "octo_draws_create: ", h); if (rc) return rc; }
    h->ctx = ctx; h->model = model; h->D = D;
    auto bail = [&](int code, const char* msg) { octo_draws_destroy(h); return fail(nullptr, code, msg); };
    if (hipMalloc((void**)&h->own_priors, sizeof(octo_prior) * D) != hipSuccess || hipMalloc((void**)&h->own_pc, sizeof(double) * pc.size()) != hipSuccess ||
        hipMalloc((void**)&h->own_ic, sizeof(double) * ic.size()) != hipSuccess)
        return bail(OCTO_ENOMEM, "octo_draws_create: hipMalloc failed");
    h->d_priors = h->own_priors; h->d_pc = h->own_pc; h->d_ic = h->own_ic;      // the active table: the handle's own until octo_draws_use_reference
    if (hipMemcpy(h->d_priors, priors, sizeof(octo_prior) * D, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_pc, pc.data(), sizeof(double) * pc.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_ic, ic.data(), sizeof(double) * ic.size(), hipMemcpyHostToDevice) != hipSuccess)
        return bail(OCTO_EHIP, "octo_draws_create: upload failed");
    *out = h;
    return OCTO_OK;
}

int32_t octo_draws_destroy(octo_draws* h) {
    if (!h) return OCTO_OK;
    (void)hipSetDevice(h->device);
    (void)octo_draws_ofti_clear(h);      // the OFTI state first: its octo_ofti lives on the context
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        // The context orders a change of stream with an event recorded on the stream of its PREVIOUS call: it must not be left naming a stream
        // that no longer exists. One host-buffer call (a one-element Kepler solve) moves it back to its own stream; if the context refuses it
        // (an evaluation in flight), the stream is kept alive instead of destroyed.
        bool release = true;
        if (h->ctx && h->ctx_on_stream) {
            const double ma = 0.0, e = 0.0;
            double E = 0.0;
            release = octo_kepler_solve(h->ctx, &ma, &e, 1, &E, nullptr, nullptr) == OCTO_OK;
        }
        if (release) (void)hipStreamDestroy(h->stream);
    }
    for (void* p : std::initializer_list<void*>{h->own_priors, h->own_pc, h->own_ic, h->d_chunk, h->d_arr, h->d_out, h->d_hmc, h->d_hst, h->d_lbf, h->d_lbd, h->d_pf, h->d_pfb, h->d_mom, h->d_nuts, h->d_diag, h->d_slice, h->d_prog, h->d_prog_tab, h->d_ncull, h->d_nest, h->d_de, h->d_oftis, h->d_oftis_rows, h->d_scan_rows, h->d_scan, h->d_scan_hst, h->d_scan_binds, h->d_pma_rows, h->d_pma, h->d_pma_hst, h->d_pma_binds, h->d_gp_rows, h->d_gp, h->d_gp_hst, h->d_gp_binds})
        (void)hipFree(p);
    delete h;
    return OCTO_OK;
}

int32_t octo_draws_detach(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    (void)octo_draws_ofti_clear(h);
    h->ctx = nullptr; h->model = nullptr; h->prog_ops = nullptr;
    return OCTO_OK;
}

const char* octo_draws_last_error(const octo_draws* h) { return last_error(h); }

int32_t octo_draws_sample_device(octo_draws* h, uint64_t seed, uint64_t first, int64_t n, int64_t ld, double* d_theta, double* d_theta_t,
                                 double* d_logprior_t, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (n < 0 || ld < n) return fail(h, OCTO_EINVAL, "octo_draws_sample_device: need 0 <= n <= ld");
    if (first + (uint64_t)n < first) return fail(h, OCTO_EINVAL, "octo_draws_sample_device: first + n overflows the draw index");
    if (n == 0 || (!d_theta && !d_theta_t && !d_logprior_t)) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    return launch_draw(h, st, seed, first, nullptr, n, ld, d_theta, d_theta_t, d_logprior_t);
}

int32_t octo_draws_sync(octo_draws* h) { return sync_handle(h); }

int32_t octo_draws_best(octo_draws* h, uint64_t seed, uint64_t first, int64_t N, int32_t keep, double* theta_out, double* logpost_out, uint64_t* index_out) {
    if (!h) return OCTO_EINVAL;
    if (keep < 1 || keep > OCTO_DRAWS_MAX_KEEP) return fail(h, OCTO_EINVAL, "octo_draws_best: 1 <= keep <= 64");
    { int rc = check_range(h, "octo_draws_best", first, N, true); if (rc) return rc; }
    if (keep > N) return fail(h, OCTO_EINVAL, "octo_draws_best: keep <= N");
    if (!theta_out || !logpost_out || !index_out) return fail(h, OCTO_EINVAL, "octo_draws_best: null output");
    OCHK(h, hipSetDevice(h->device));
    ChunkBufs k; DrawArrays a; Outputs o;
    { int rc = ensure_chunk(h, k); if (rc) return rc; }
    { int rc = ensure_draw_arrays(h, std::min(N, CHUNK), a); if (rc) return rc; }
    { int rc = ensure_outputs(h, OCTO_DRAWS_MAX_KEEP, o); if (rc) return rc; }
    const hipStream_t st = h->stream;
    // the running list starts empty: every byte 0xFF = (NaN, NO_INDEX), which k_topk reads as no candidate
    OCHK(h, hipMemsetAsync(k.clp, 0xFF, sizeof(double) * keep, st));
    OCHK(h, hipMemsetAsync(k.cix, 0xFF, sizeof(uint64_t) * keep, st));
    for (int64_t done = 0; done < N; done += CHUNK) {
        const int64_t n = std::min(CHUNK, N - done);
        { int rc = launch_draw(h, st, seed, first + (uint64_t)done, nullptr, n, CHUNK, nullptr, k.tt, nullptr); if (rc) return rc; }
        { int rc = logpost_at(h, st, true, k.tt, CHUNK, n, a.lp, nullptr); if (rc) return rc; }
        const int64_t nb = (n + SEL_SLAB - 1) / SEL_SLAB;
        hipLaunchKernelGGL(k_topk, dim3((unsigned)nb), dim3(TPB), 0, st, a.lp, (const uint64_t*)nullptr, first + (uint64_t)done, n, keep, (int64_t)1, k.clp, k.cix);
        hipLaunchKernelGGL(k_topk, dim3(1), dim3(TPB), 0, st, k.clp, k.cix, (uint64_t)0, (1 + nb) * keep, keep, (int64_t)0, k.clp, k.cix);
        OCHK(h, hipGetLastError());
    }
    OCHK(h, hipMemcpyAsync(logpost_out, k.clp, sizeof(double) * keep, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(index_out, k.cix, sizeof(uint64_t) * keep, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    // places no finite log-posterior took: −Inf and the lowest draw indices not listed yet
    uint64_t next = first;
    for (int r = 0; r < keep; ++r) {
        if (index_out[r] != NO_INDEX) continue;
        for (;; ++next) {
            bool listed = false;
            for (int q = 0; q < keep; ++q) listed = listed || index_out[q] == next;
            if (!listed) break;
        }
        index_out[r] = next++;
        logpost_out[r] = -INFINITY;
    }
    // θ of the winners, from the counter
    OCHK(h, hipMemcpyAsync(o.ix, index_out, sizeof(uint64_t) * keep, hipMemcpyHostToDevice, st));
    { int rc = launch_draw(h, st, seed, 0, o.ix, keep, keep, o.theta, nullptr, nullptr); if (rc) return rc; }
    OCHK(h, hipMemcpyAsync(theta_out, o.theta, sizeof(double) * keep * h->D, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

int32_t octo_draws_rejection(octo_draws* h, uint64_t seed, uint64_t first, int64_t N, int64_t cap, double* theta_out, double* loglike_out,
                             double* logpost_out, uint64_t* index_out, int64_t* n_accepted, double* max_loglike) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_range(h, "octo_draws_rejection", first, N, true); if (rc) return rc; }
    if (cap < 0 || !n_accepted) return fail(h, OCTO_EINVAL, "octo_draws_rejection: cap >= 0 and n_accepted are required");
    if (cap > 0 && (!theta_out || !loglike_out || !logpost_out || !index_out)) return fail(h, OCTO_EINVAL, "octo_draws_rejection: null output with cap > 0");
    OCHK(h, hipSetDevice(h->device));
    ChunkBufs k; DrawArrays a; Outputs o;
    { int rc = ensure_chunk(h, k); if (rc) return rc; }
    { int rc = ensure_draw_arrays(h, N, a); if (rc) return rc; }
    const hipStream_t st = h->stream;
    // pass 1: ll of every draw, chunk by chunk (chunk boundaries are block boundaries), and its maximum
    for (int64_t done = 0; done < N; done += CHUNK) {
        const int64_t n = std::min(CHUNK, N - done);
        { int rc = launch_draw(h, st, seed, first + (uint64_t)done, nullptr, n, CHUNK, nullptr, k.tt, k.lpt); if (rc) return rc; }
        { int rc = logpost_at(h, st, true, k.tt, CHUNK, n, a.lp + done, nullptr); if (rc) return rc; }
        hipLaunchKernelGGL(k_loglike, grid_of(n), dim3(TPB), 0, st, a.lp + done, k.lpt, n, a.ll + done, a.pmax + done / TPB);
        OCHK(h, hipGetLastError());
    }
    *n_accepted = 0;
    { int rc = draws_max_pass(h, st, a.pmax, N, k.max, max_loglike); if (rc) return rc; }
    // pass 2: flags -> block counts -> offsets -> ordered scatter
    { int rc = ensure_outputs(h, std::max<int64_t>(std::min(cap, N), 1), o); if (rc) return rc; }
    const int64_t room = std::min(cap, N);
    int64_t total = 0;
    { int rc = draws_accept_pass(h, st, a.ll, a.lp, N, k.max, seed, first, a.cnt, room, o.ix, o.ll, o.lp, &total); if (rc) return rc; }
    *n_accepted = total;
    const int64_t ns = std::min(total, room);
    if (ns == 0) return OCTO_OK;
    { int rc = launch_draw(h, st, seed, 0, o.ix, ns, ns, o.theta, nullptr, nullptr); if (rc) return rc; }
    OCHK(h, hipMemcpyAsync(index_out, o.ix, sizeof(uint64_t) * ns, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(loglike_out, o.ll, sizeof(double) * ns, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(logpost_out, o.lp, sizeof(double) * ns, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpy2DAsync(theta_out, sizeof(double) * cap, o.theta, sizeof(double) * ns, sizeof(double) * ns, h->D, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

}  // extern "C"
