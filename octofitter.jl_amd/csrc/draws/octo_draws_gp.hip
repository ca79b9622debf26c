// octo_draws_gp.hip — liboctofitter_hip_draws.so, the nineteenth part: a radial-velocity table of the star under a Gaussian process with celerite kernels
// (include/octofitter_hip_draws.h, "The nineteenth"): log N(r; 0, K) of the residuals by the semiseparable recursion and its exact gradient in reverse mode.
// Of the main library's sources it INCLUDES the device routines the likelihood kernels run, as octo_draws_scan.hip does: the orbit constructor, the cold
// Kepler solve, rv_row's arithmetic and the chain rule through the constructor are the code the main library runs.
//
//   k_gp_rows        grid = (walker tiles of 64, tasks of OCTO_DRAWS_SCAN_ROWS rows), one wave a block, lane = walker; the rows are wave-uniform (scalar
//                    loads). η_i = Σ_k c_i[k]·β_k + Σ_p f_p·K_p·V_p(t_i) with one cold Kepler solve per (walker, row, planet), planets added in planet order
//                    in LDS (4 KB); r_i = rv_i − η_i to the work array (and η to the values output).
//   k_gp_factor<R'>  grid = walker tiles, lane = walker, sequential over the rows: the recursion on the state (T, q) = (S + D·W·Wᵀ, f + W·z) in registers
//                    (statically indexed: R' = 2, 4, 8), every slot's (a, b, c, d, rot) in LDS; ℓ, the validity, and with STORE the state handed to the
//                    first row of every segment of OCTO_DRAWS_GP_SEGMENT rows.
//   k_gp_back<R'>    the reverse walk, segment by segment from the last: the segment's states recomputed forward from its checkpoint, each row's record in the
//                    work array handed to the next, then walked backward with the adjoints of T and q in LDS and T streamed from the records; no matrix is
//                    held in registers. α_i replaces r_i; the slots' coefficient adjoints accumulate in LDS and go through the terms' chain rule at the end.
//                    Nothing is divided by φ.
//   k_gp_adj         the grid of k_gp_rows: Σ α_i c_i[k], and per planet a second cold solve and the six sums of rv_row against ∂ℓ/∂η_i = α_i.
//   k_gp_finish      the tasks' sums in task order and planet_finish per planet: ∂ℓ/∂(a, e, i, ω, Ω, tp, M, plx, mass), and ∂ℓ/∂β.
// No atomics, and neither the row partition nor the segments depend on W: a walker's bits depend on its column alone.
// A table under DENSE kernels (the twentieth part) keeps this unit's table, C ABI, k_gp_rows, k_gp_adj and k_gp_finish and puts octo_draws_gpd.hip's kernels
// between them (gp_launch); the argument block GpArgs and the row record are in octo_draws_gp_shared.h.
#include "octo_draws_gp_shared.h"

namespace {
using gp_dev::dev_consts;
using gp_dev::walker_setup;

using FinL = Layout<2, true, false, KM_RVABS>;      // the main library's sums of a planet under an absolute-RV table: U1 … U6 (0 here), GE, GM, GT, GC, GK, GW
static_assert(FinL::PL_N == 12 && FinL::GE == 6 && FinL::GW == 11, "six RV sums behind the six astrometric ones");
enum { SLOT_REAL = 0, SLOT_FIRST, SLOT_SECOND, SLOT_PAD };      // a slot's role: wave-uniform
enum { CO_A = 0, CO_B, CO_C, CO_D, CO_ROT, N_CO };             // a slot's coefficients in LDS, [N_CO][R'][64]

__device__ __forceinline__ bool gp_contributes(const GpArgs& a, int p) {      // wave-uniform
    const int kind = a.orbit_kind[p];
    return (kind == OCTO_ORBIT_VISUAL_KEP || kind == OCTO_ORBIT_RADVEL || kind == OCTO_ORBIT_KEP) && a.has_mass[p] != 0;
}

__global__ __launch_bounds__(WAVE) void k_gp_rows(GpArgs a) {
    __shared__ __attribute__((aligned(16))) double eta_s[GP_ROWS * WAVE];
    const int lane = threadIdx.x, task = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;      // w < ldw: the work array has a column for every lane
    const int64_t wl = w < a.W ? w : a.W - 1;
    const int r0 = task * GP_ROWS, nr = min(GP_ROWS, a.n - r0), P = a.P;
    const double* __restrict__ rows = a.rows + (int64_t)r0 * GROWW;
    double* eta = eta_s + lane;
    {
        double bk[GP_K];
#pragma unroll
        for (int k = 0; k < GP_K; ++k) bk[k] = (!a.beta || k >= a.K) ? 0.0 : a.beta[(int64_t)k * a.ld + wl];
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * GROWW;
            double e = 0.0;
#pragma unroll
            for (int k = 0; k < GP_K; ++k) e = fma(rw[3 + k], bk[k], e);
            eta[r * WAVE] = e;
        }
    }
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        if (!gp_contributes(a, p)) continue;
        double v[NWC];
        (void)walker_setup(a, p, wl, v);
        PC pc;
        load_pc(pc, v, 1, 0, 0);
        const double fK = -pc.mu * pc.K;      // rv_row: gc_p·K_p, gc_p = −m_p/M of an absolute RV
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * GROWW;
            const KSol ks = kepler_solve<2, false>(rw[0], pc);
            const double cnu = (ks.cE - pc.e) * ks.invD, snu = pc.beta * ks.sE * ks.invD;
            const double V = fma(cnu + pc.e, pc.cw, -(snu * pc.sw));
            eta[r * WAVE] = fma(fK, V, eta[r * WAVE]);
        }
    }
    for (int r = 0; r < nr; ++r) {
        const double* __restrict__ rw = rows + r * GROWW;
        a.k.res[(int64_t)(r0 + r) * a.ldw + w] = rw[1] - eta[r * WAVE];
        if (a.eta && w < a.W) a.eta[(int64_t)(r0 + r) * a.ld_out + w] = eta[r * WAVE];
    }
}

// every slot's coefficients of walker wl into co [N_CO][RP][64] (at this lane); returns their validity: finite, and every rate > 0
template <int RP>
__device__ __forceinline__ bool gp_coefficients(const GpArgs& a, int64_t wl, double* co) {
    bool ok = true;
    int r = 0, o = 0;
#pragma unroll 1
    for (int j = 0; j < a.J; ++j) {      // the terms' kinds are wave-uniform
        const int kind = a.term[j];
        const double h0 = a.hyper[(int64_t)o * a.ld + wl], h1 = a.hyper[(int64_t)(o + 1) * a.ld + wl];
        double A0, B0, C0, D0, A1 = 0.0, B1 = 0.0, C1 = 1.0, D1 = 0.0, rot1 = 1.0;
        if (kind == OCTO_DRAWS_GP_REAL) {
            A0 = h0; B0 = 0.0; C0 = h1; D0 = 0.0;
        } else if (kind == OCTO_DRAWS_GP_COMPLEX) {
            const double h2 = a.hyper[(int64_t)(o + 2) * a.ld + wl], h3 = a.hyper[(int64_t)(o + 3) * a.ld + wl];
            A0 = A1 = h0; B0 = B1 = h1; C0 = C1 = h2; D0 = D1 = h3;
        } else {
            const double S0 = h0, Q = h1, w0 = a.hyper[(int64_t)(o + 2) * a.ld + wl];
            const bool over = Q > 0.5;
            const double f = sqrt(over ? fma(4.0 * Q, Q, -1.0) : fma(-4.0 * Q, Q, 1.0));      // 0 at Q = ½: the quotients below are not finite
            const double a0 = S0 * w0 * Q, c0 = w0 / (2.0 * Q), inv = 1.0 / f;
            A0 = over ? a0 : 0.5 * a0 * (1.0 + inv); A1 = over ? a0 : 0.5 * a0 * (1.0 - inv);
            B0 = B1 = over ? a0 * inv : 0.0;
            C0 = over ? c0 : c0 * (1.0 - f); C1 = over ? c0 : c0 * (1.0 + f);
            D0 = D1 = over ? c0 * f : 0.0;
            rot1 = over ? 1.0 : 0.0;
        }
        const int ns = kind == OCTO_DRAWS_GP_REAL ? 1 : 2;
        co[(CO_A * RP + r) * WAVE] = A0; co[(CO_B * RP + r) * WAVE] = B0; co[(CO_C * RP + r) * WAVE] = C0; co[(CO_D * RP + r) * WAVE] = D0;
        co[(CO_ROT * RP + r) * WAVE] = 0.0;
        ok = ok && isfinite(A0) && isfinite(B0) && isfinite(C0) && isfinite(D0) && C0 > 0.0;
        if (ns == 2) {
            co[(CO_A * RP + r + 1) * WAVE] = A1; co[(CO_B * RP + r + 1) * WAVE] = B1; co[(CO_C * RP + r + 1) * WAVE] = C1; co[(CO_D * RP + r + 1) * WAVE] = D1;
            co[(CO_ROT * RP + r + 1) * WAVE] = rot1;
            ok = ok && isfinite(A1) && isfinite(B1) && isfinite(C1) && isfinite(D1) && C1 > 0.0;
        }
        r += ns; o += kind == OCTO_DRAWS_GP_REAL ? 2 : (kind == OCTO_DRAWS_GP_COMPLEX ? 4 : 3);
    }
    for (; r < RP; ++r) {      // a padding slot: Ũ = Ṽ = φ = 0, and no a on the diagonal
        co[(CO_A * RP + r) * WAVE] = 0.0; co[(CO_B * RP + r) * WAVE] = 0.0; co[(CO_C * RP + r) * WAVE] = 0.0; co[(CO_D * RP + r) * WAVE] = 0.0;
        co[(CO_ROT * RP + r) * WAVE] = 1.0;
    }
    return ok;
}

// the row values of every slot at τ = t_i − t_1, Δ = t_i − t_{i−1}: (cx, sx) = rot ? (sin x, −cos x) : (cos x, sin x) of x = d·τ, Ũ = a·cx + b·sx, Ṽ = cx,
// φ = exp(−c·Δ). One sincos a pair: both slots of a pair have the same d in either regime of an SHO.
// A vector of one lane in LDS or in the work array, 64 doubles apart, where the reverse walk keeps what its registers have no room for; the forward pass
// hands the same functions plain arrays. A Sink takes what a caller does not want.
struct LaneVec {
    double* p;
    __device__ __forceinline__ double& operator[](int k) const { return p[k * WAVE]; }
};
// … a record of the work array: a wave-uniform base (in scalar registers) and the lane
struct RecVec {
    double* b; unsigned l;
    __device__ __forceinline__ double& operator[](int k) const { return b[(unsigned)(k * WAVE) + l]; }
};
__device__ __forceinline__ double* uniform_ptr(double* p) {
    const uint64_t x = (uint64_t)p;
    return (double*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x));
}
struct Sink {
    struct Ref { __device__ __forceinline__ void operator=(double) const {} };
    __device__ __forceinline__ Ref operator[](int) const { return {}; }
};

template <int RP, class CX, class SX>
__device__ __forceinline__ void gp_slots(const GpArgs& a, const double* co, double tau, double dt, double (&U)[RP], CX&& cx, SX&& sx, double (&phi)[RP]) {
    double c0 = 1.0, s0 = 0.0;
#pragma unroll
    for (int r = 0; r < RP; ++r) {
        const int role = a.slot[r];
        if (role == SLOT_PAD) { U[r] = 0.0; cx[r] = 0.0; sx[r] = 0.0; phi[r] = 0.0; continue; }
        if (role == SLOT_REAL) { c0 = 1.0; s0 = 0.0; }
        else if (role == SLOT_FIRST) sincos_reduced(co[(CO_D * RP + r) * WAVE] * tau, s0, c0);
        const bool rot = co[(CO_ROT * RP + r) * WAVE] != 0.0;
        const double c = rot ? s0 : c0, sn = rot ? -c0 : s0;
        cx[r] = c;
        sx[r] = sn;
        U[r] = fma(co[(CO_A * RP + r) * WAVE], c, co[(CO_B * RP + r) * WAVE] * sn);
        phi[r] = exp(-co[(CO_C * RP + r) * WAVE] * dt);
    }
}

// Σ_r (rot ? 0 : a_r): what the terms add to the diagonal
template <int RP>
__device__ __forceinline__ double gp_asum(const double* co) {
    double x = 0.0;
#pragma unroll
    for (int r = 0; r < RP; ++r) x += co[(CO_ROT * RP + r) * WAVE] != 0.0 ? 0.0 : co[(CO_A * RP + r) * WAVE];
    return x;
}

constexpr __host__ __device__ int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// One row from the state (T, q) handed to it, T read through `Tin`: S_ab = (φ_a·φ_b)·T_ab, f = φ∘q, SU = S·Ũ, D = A − Ũ·SU, W = (Ṽ − SU)/D, z = r − Ũ·f.
// k_gp_factor and both loops of k_gp_back run this function, so the recomputed states are the forward pass's bits.
template <int RP, class Get, class Q, class V_, class F>
__device__ __forceinline__ void gp_row(Get Tin, Q&& q, const double (&U)[RP], V_&& V, const double (&phi)[RP], double A, double r,
                                       F&& f, double (&SU)[RP], double (&Wv)[RP], double& D, double& iD, double& z) {
    double us = 0.0, uf = 0.0;
#pragma unroll
    for (int i = 0; i < RP; ++i) {
        SU[i] = 0.0;
        const double fi = phi[i] * q[i];
        f[i] = fi;
        uf = fma(U[i], fi, uf);
    }
#pragma unroll
    for (int i = 0; i < RP; ++i) {      // every stored element once, row by row of the packed triangle: a row's loads are not hoisted above the row before
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double S = (phi[i] * phi[j]) * Tin(tri(i, j));
            SU[i] = fma(S, U[j], SU[i]);
            if (j < i) SU[j] = fma(S, U[i], SU[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < RP; ++i) us = fma(U[i], SU[i], us);
    D = A - us;
    iD = 1.0 / D;
    z = r - uf;
#pragma unroll
    for (int i = 0; i < RP; ++i) Wv[i] = (V[i] - SU[i]) * iD;
}

// … and the state it hands on: T = S + D·W·Wᵀ, q = f + W·z, read through Tin and written through Tout (in place in k_gp_factor's registers; from one row's
// record in the work array to the next in k_gp_back)
template <int RP, class Get, class Put, class QO>
__device__ __forceinline__ void gp_hand_on(Get Tin, Put Tout, QO&& qout, const double (&phi)[RP], const double (&f)[RP], const double (&Wv)[RP], double D, double z) {
#pragma unroll
    for (int i = 0; i < RP; ++i) {
        const double dw = D * Wv[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) Tout(tri(i, j), fma(dw, Wv[j], (phi[i] * phi[j]) * Tin(tri(i, j))));
        qout[i] = fma(Wv[i], z, f[i]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int RP, bool STORE>
__global__ __launch_bounds__(WAVE) void k_gp_factor(GpArgs a) {
    constexpr int TRI = RP * (RP + 1) / 2, NS = TRI + RP;
    __shared__ __attribute__((aligned(16))) double co_s[N_CO * RP * WAVE];
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;      // w < ldw
    const int64_t wl = w < a.W ? w : a.W - 1;
    double* co = co_s + lane;
    bool ok = gp_coefficients<RP>(a, wl, co);
    const double s = a.jitter ? a.jitter[wl] : 0.0, s2 = s * s;
    ok = ok && isfinite(s) && s >= 0.0;
    if (a.beta)
        for (int k = 0; k < a.K; ++k) ok = ok && isfinite(a.beta[(int64_t)k * a.ld + wl]);
#pragma unroll 1
    for (int p = 0; p < a.P; ++p) {
        double elv[OCTO_N_EL];
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) elv[k] = a.elems[((int64_t)p * OCTO_N_EL + k) * a.ld + wl];
        const SetupScalars q = setup_scalars<true>(elv, a.c, a.orbit_kind[p], a.has_mass[p]);
        ok = ok && setup_valid<true>(elv, a.orbit_kind[p], a.has_mass[p], q.sma);
    }
    const double asum = gp_asum<RP>(co);
    double T[TRI], q[RP];
#pragma unroll
    for (int k = 0; k < TRI; ++k) T[k] = 0.0;
#pragma unroll
    for (int k = 0; k < RP; ++k) q[k] = 0.0;
    const double t0 = a.rows[0];
    double t_prev = t0, ll = 0.0;
#pragma unroll 1
    for (int i = 0; i < a.n; ++i) {
        asm volatile("" ::: "memory");      // the slots' coefficients are read from LDS where they are used, not hoisted into forty registers
        const double* __restrict__ rw = a.rows + (int64_t)i * GROWW;
        if constexpr (STORE) {
            if (i % GP_G == 0) {
                double* ck = a.k.check + ((int64_t)blockIdx.x * a.n_seg + i / GP_G) * (NS * WAVE) + lane;      // [tile][segment][NS][64]: constant offsets
#pragma unroll
                for (int k = 0; k < TRI; ++k) ck[k * WAVE] = T[k];
#pragma unroll
                for (int k = 0; k < RP; ++k) ck[(TRI + k) * WAVE] = q[k];
            }
        }
        const double t = rw[0];
        double U[RP], cx[RP], sx[RP], phi[RP], f[RP], SU[RP], Wv[RP], D, iD, z;
        gp_slots<RP>(a, co, t - t0, t - t_prev, U, cx, sx, phi);
        t_prev = t;
        gp_row<RP>([&](int k) { return T[k]; }, q, U, cx, phi, (rw[2] + s2) + asum, a.k.res[(int64_t)i * a.ldw + w], f, SU, Wv, D, iD, z);
        gp_hand_on<RP>([&](int k) { return T[k]; }, [&](int k, double x) { T[k] = x; }, q, phi, f, Wv, D, z);
        ok = ok && D > 0.0 && isfinite(D);
        ll += fma(-0.5 * z, z * iD, -0.5 * log(D)) - 0.5 * LOG2PI;
    }
    ok = ok && isfinite(ll) && w < a.W;
    a.k.ok[w] = ok ? 1.0 : 0.0;
    if (w < a.W && a.ll) a.ll[w] = (a.accumulate ? a.ll[w] : 0.0) + (ok ? ll : -INFINITY);
}

template <int RP>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gp_back(GpArgs a) {
    constexpr int TRI = RP * (RP + 1) / 2, NS = TRI + RP;
    extern __shared__ __attribute__((aligned(16))) double L[];      // gp_back_lds<RP>(): 78 KB at R' = 8
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;      // w < ldw
    const int64_t wl = w < a.W ? w : a.W - 1;
    // the slots' coefficients · their adjoints (ga, gb, gc, gd) · the adjoint of T · that of q · a row's cx, sx, S·Ũ, Ũ and φ between its two halves
    double *co = L + lane, *g = co + N_CO * RP * WAVE, *bT = g + 4 * RP * WAVE, *bq = bT + TRI * WAVE, *lcx = bq + RP * WAVE, *lsx = lcx + RP * WAVE, *lsu = lsx + RP * WAVE, *lu = lsu + RP * WAVE, *lphi = lu + RP * WAVE;
    (void)gp_coefficients<RP>(a, wl, co);
    const bool ok = a.k.ok[w] != 0.0;
    const double s = a.jitter ? a.jitter[wl] : 0.0, s2 = s * s;
    const double asum = gp_asum<RP>(co);
#pragma unroll
    for (int k = 0; k < 4 * RP; ++k) g[k * WAVE] = 0.0;
#pragma unroll
    for (int k = 0; k < TRI; ++k) bT[k * WAVE] = 0.0;
    double gs = 0.0;
#pragma unroll
    for (int k = 0; k < RP; ++k) bq[k * WAVE] = 0.0;
    const double t0 = a.rows[0];
#pragma unroll 1
    for (int sg = a.n_seg - 1; sg >= 0; --sg) {
        const int i0 = sg * GP_G, i1 = min(a.n, i0 + GP_G);
        {   // the states handed to the segment's rows, forward from the checkpoint: each row reads its record in the work array and writes the next one's
            const RecVec ck{uniform_ptr(a.k.check + ((int64_t)blockIdx.x * a.n_seg + sg) * (NS * WAVE)), (unsigned)lane};
            const RecVec r0{uniform_ptr(a.k.seg + (int64_t)blockIdx.x * GP_G * (NS * WAVE)), (unsigned)lane};      // [tile][row of the segment][NS][64]
#pragma unroll
            for (int k = 0; k < NS; ++k) r0[k] = ck[k];
            double t_prev = a.rows[(int64_t)max(i0 - 1, 0) * GROWW];
#pragma unroll 1
            for (int i = i0; i + 1 < i1; ++i) {
                asm volatile("" ::: "memory");
                const double* __restrict__ rw = a.rows + (int64_t)i * GROWW;
                const RecVec sp{uniform_ptr(a.k.seg + ((int64_t)blockIdx.x * GP_G + (i - i0)) * (NS * WAVE)), (unsigned)lane}, sn{sp.b + NS * WAVE, sp.l};
                const double t = rw[0];
                double U[RP], phi[RP], f[RP], SU[RP], Wv[RP], D, iD, z;
                gp_slots<RP>(a, co, t - t0, t - t_prev, U, LaneVec{lcx}, Sink{}, phi);
                t_prev = t;
                gp_row<RP>([&](int k) { return sp[k]; }, RecVec{sp.b + TRI * WAVE, sp.l}, U, LaneVec{lcx}, phi, (rw[2] + s2) + asum, a.k.res[(int64_t)i * a.ldw + w], f, SU, Wv,
                           D, iD, z);
                asm volatile("" ::: "memory");      // T is read again, not kept
                gp_hand_on<RP>([&](int k) { return sp[k]; }, [&](int k, double x) { sn[k] = x; }, RecVec{sn.b + TRI * WAVE, sn.l}, phi, f, Wv, D, z);
            }
        }
#pragma unroll 1
        for (int i = i1 - 1; i >= i0; --i) {
            asm volatile("" ::: "memory");      // the slots' coefficients are read from LDS where they are used, not hoisted into forty registers
            const double* __restrict__ rw = a.rows + (int64_t)i * GROWW;
            const RecVec sp{uniform_ptr(a.k.seg + ((int64_t)blockIdx.x * GP_G + (i - i0)) * (NS * WAVE)), (unsigned)lane};
            const double t = rw[0], tau = t - t0, dt = t - a.rows[(int64_t)max(i - 1, 0) * GROWW];
            double U[RP], phi[RP], SU[RP], Wv[RP], D, iD, z;
            gp_slots<RP>(a, co, tau, dt, U, LaneVec{lcx}, LaneVec{lsx}, phi);
            const double white = rw[2] + s2, res = a.k.res[(int64_t)i * a.ldw + w];
            gp_row<RP>([&](int k) { return sp[k]; }, RecVec{sp.b + TRI * WAVE, sp.l}, U, LaneVec{lcx}, phi, white + asum, res, Sink{}, SU, Wv, D, iD, z);
#pragma unroll
            for (int k = 0; k < RP; ++k) { lsu[k * WAVE] = SU[k]; lu[k * WAVE] = U[k]; lphi[k * WAVE] = phi[k]; }
            asm volatile("" ::: "memory");      // T and q are read again below, cx, sx and S·Ũ come back from LDS: none is kept in registers in between
            // ℓ's own terms, and what the next row handed back: bz = ∂/∂z_i, α_i = −bz
            double wq = 0.0;
#pragma unroll
            for (int k = 0; k < RP; ++k) wq = fma(Wv[k], bq[k * WAVE], wq);
            const double bz = fma(-z, iD, wq), alpha = -bz;
            a.k.res[(int64_t)i * a.ldw + w] = ok ? alpha : 0.0;
            if (a.mu && w < a.W) a.mu[(int64_t)i * a.ld_out + w] = fma(-white, alpha, res);
            // y = bT·W, then the adjoints of D, W, Ṽ, SU, Ũ, f. The scheduling barriers keep the loads of one row of bT (and of T below) from being
            // hoisted above the row before: the vectors stay in registers, the matrices pass through.
            double y[RP], wy = 0.0;
#pragma unroll
            for (int m = 0; m < RP; ++m) {
                double x = 0.0;
#pragma unroll
                for (int j = 0; j < RP; ++j) x = fma(bT[tri(m, j) * WAVE], Wv[j], x);
                y[m] = x;
                wy = fma(Wv[m], x, wy);
                __builtin_amdgcn_sched_barrier(0);
            }
            double bD = fma(0.5 * (z * iD), z * iD, -0.5 * iD) + wy, bww = 0.0;
            double bSU[RP], bU[RP], bphi[RP];
#pragma unroll
            for (int k = 0; k < RP; ++k) {
                y[k] = fma(2.0 * D, y[k], bq[k * WAVE] * z);      // the adjoint of W …
                bww = fma(y[k], Wv[k], bww);
            }
            bD = fma(-bww, iD, bD);
            gs += bD;
#pragma unroll
            for (int k = 0; k < RP; ++k) {
                const double bV = y[k] * iD;                // … and of Ṽ, whose only way on is the phase: −bV·sx·τ into ∂ℓ/∂d
                g[(3 * RP + k) * WAVE] = fma(-(bV * lsx[k * WAVE]), tau, g[(3 * RP + k) * WAVE]);
                bSU[k] = -fma(bD, lu[k * WAVE], bV);
                const double qk = sp[TRI + k];
                bU[k] = -fma(bz, lphi[k * WAVE] * qk, bD * lsu[k * WAVE]);      // f = φ∘q
                const double bf = fma(-bz, lu[k * WAVE], bq[k * WAVE]);
                bphi[k] = bf * qk;
                bq[k * WAVE] = lphi[k * WAVE] * bf;                        // handed to the row before
            }
            asm volatile("" ::: "memory");      // bT is read again below, not kept from the product above
            // bS = bT + sym(bSU·Ũᵀ); Ũ's adjoint takes S·bSU, φ's 2·Σ_b bS_ab φ_b T_ab, and φφᵀ∘bS is handed to the row before
#pragma unroll
            for (int m = 0; m < RP; ++m) {
#pragma unroll
                for (int j = 0; j <= m; ++j) {
                    const double pm = lphi[m * WAVE], pj = lphi[j * WAVE];
                    const double Tmj = sp[tri(m, j)], pp = pm * pj, S = pp * Tmj;
                    const double bS = fma(0.5, fma(bSU[m], lu[j * WAVE], lu[m * WAVE] * bSU[j]), bT[tri(m, j) * WAVE]);
                    if (m == j) {
                        bU[m] = fma(S, bSU[m], bU[m]);
                        bphi[m] = fma(2.0 * bS, pm * Tmj, bphi[m]);
                    } else {
                        bU[m] = fma(S, bSU[j], bU[m]);
                        bU[j] = fma(S, bSU[m], bU[j]);
                        bphi[m] = fma(2.0 * bS, pj * Tmj, bphi[m]);
                        bphi[j] = fma(2.0 * bS, pm * Tmj, bphi[j]);
                    }
                    bT[tri(m, j) * WAVE] = pp * bS;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int k = 0; k < RP; ++k) {
                const double ca = co[(CO_A * RP + k) * WAVE], cb = co[(CO_B * RP + k) * WAVE];
                const bool rot = co[(CO_ROT * RP + k) * WAVE] != 0.0;
                const double ck = lcx[k * WAVE], sk = lsx[k * WAVE];
                g[(0 * RP + k) * WAVE] += fma(bU[k], ck, rot ? 0.0 : bD);
                g[(1 * RP + k) * WAVE] = fma(bU[k], sk, g[(1 * RP + k) * WAVE]);
                g[(2 * RP + k) * WAVE] = fma(bphi[k], -dt * lphi[k * WAVE], g[(2 * RP + k) * WAVE]);
                g[(3 * RP + k) * WAVE] = fma(bU[k] * fma(cb, ck, -(ca * sk)), tau, g[(3 * RP + k) * WAVE]);
            }
        }
    }
    if (w >= a.W) return;
    if (a.g_jitter) a.g_jitter[w] = ok ? 2.0 * s * gs : 0.0;
    if (!a.g_hyper) return;
    // the slots' (ga, gb, gc, gd) to the terms' own parameters
    int r = 0, o = 0;
#pragma unroll 1
    for (int j = 0; j < a.J; ++j) {
        const int kind = a.term[j];
        const double ga0 = g[(0 * RP + r) * WAVE], gb0 = g[(1 * RP + r) * WAVE], gc0 = g[(2 * RP + r) * WAVE], gd0 = g[(3 * RP + r) * WAVE];
        double out[4] = {ga0, gc0, 0.0, 0.0};
        int nh = 2, ns = 1;
        if (kind != OCTO_DRAWS_GP_REAL) {
            const double ga1 = g[(0 * RP + r + 1) * WAVE], gb1 = g[(1 * RP + r + 1) * WAVE], gc1 = g[(2 * RP + r + 1) * WAVE], gd1 = g[(3 * RP + r + 1) * WAVE];
            ns = 2;
            if (kind == OCTO_DRAWS_GP_COMPLEX) {
                nh = 4;
                out[0] = ga0 + ga1; out[1] = gb0 + gb1; out[2] = gc0 + gc1; out[3] = gd0 + gd1;
            } else {
                nh = 3;
                const double S0 = a.hyper[(int64_t)o * a.ld + w], Q = a.hyper[(int64_t)(o + 1) * a.ld + w], w0 = a.hyper[(int64_t)(o + 2) * a.ld + w];
                const bool over = Q > 0.5;
                const double f = sqrt(over ? fma(4.0 * Q, Q, -1.0) : fma(-4.0 * Q, Q, 1.0)), inv = 1.0 / f;
                const double a0 = S0 * w0 * Q, c0 = w0 / (2.0 * Q);
                double ab, cb, fb, fp;      // the adjoints of a0, c0 and f, and df/dQ
                if (over) {      // a = a0, b = a0/f, c = c0, d = c0·f
                    const double A = ga0 + ga1, B = gb0 + gb1, C = gc0 + gc1, Dd = gd0 + gd1;
                    ab = fma(B, inv, A); cb = fma(Dd, f, C); fb = fma(Dd, c0, -(B * a0) * (inv * inv)); fp = 4.0 * Q * inv;
                } else {         // a± = ½·a0·(1 ± 1/f), c± = c0·(1 ∓ f): slot r is +, slot r + 1 is −
                    ab = 0.5 * fma(ga0, 1.0 + inv, ga1 * (1.0 - inv)); cb = fma(gc0, 1.0 - f, gc1 * (1.0 + f));
                    fb = fma(0.5 * a0 * (ga1 - ga0), inv * inv, c0 * (gc1 - gc0)); fp = -4.0 * Q * inv;
                }
                out[0] = ab * w0 * Q;
                out[1] = fma(fb, fp, fma(ab, S0 * w0, -(cb * c0) / Q));
                out[2] = fma(ab, S0 * Q, cb / (2.0 * Q));
            }
        }
        for (int k = 0; k < nh; ++k) a.g_hyper[(int64_t)(o + k) * a.ld + w] = ok ? out[k] : 0.0;
        r += ns; o += nh;
    }
}

// Σ α_i c_i[k] and a planet's six sums against ∂ℓ/∂η_i = α_i: the running sums of the main library's rv_row with rvb = α_i, gc = −m/M, on a second cold solve
__global__ __launch_bounds__(WAVE) void k_gp_adj(GpArgs a) {
    const int lane = threadIdx.x, task = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    const int64_t wl = w < a.W ? w : a.W - 1;
    const int r0 = task * GP_ROWS, nr = min(GP_ROWS, a.n - r0), P = a.P;
    const double* __restrict__ rows = a.rows + (int64_t)r0 * GROWW;
    const double* al = a.k.res + (int64_t)r0 * a.ldw + w;
    double* part = a.k.part + (int64_t)task * a.n_sums * a.ldw + w;
    {
        double sb[GP_K];
#pragma unroll
        for (int k = 0; k < GP_K; ++k) sb[k] = 0.0;
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * GROWW;
            const double x = al[(int64_t)r * a.ldw];
#pragma unroll
            for (int k = 0; k < GP_K; ++k) sb[k] = fma(x, rw[3 + k], sb[k]);
        }
#pragma unroll
        for (int k = 0; k < GP_K; ++k) part[(int64_t)k * a.ldw] = sb[k];
    }
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        double gE = 0.0, gM = 0.0, gT = 0.0, gC = 0.0, gK = 0.0, gW = 0.0;
        if (gp_contributes(a, p)) {
            double v[NWC];
            (void)walker_setup(a, p, wl, v);
            PC pc;
            load_pc(pc, v, 1, 0, 0);
            const double gc = -pc.mu, ib2 = 1.0 / (pc.beta * pc.beta);
            for (int r = 0; r < nr; ++r) {
                const double* __restrict__ rw = rows + r * GROWW;
                const double rvb = al[(int64_t)r * a.ldw];
                const KSol ks = kepler_solve<2, false>(rw[0], pc);
                const double cnu = (ks.cE - pc.e) * ks.invD, snu = pc.beta * ks.sE * ks.invD;
                const double V = fma(cnu + pc.e, pc.cw, -(snu * pc.sw));
                gK = fma(gc * V, rvb, gK);
                gC += -(pc.K * V * rvb);
                const double Vb = gc * pc.K * rvb;
                const double S = fma(snu, pc.cw, cnu * pc.sw);      // sin(ν + ω)
                gW = fma(Vb, -fma(pc.e, pc.sw, S), gW);
                const double VS = Vb * S;
                const double Mb = -(VS * pc.beta) * (ks.invD * ks.invD);
                double eb = Vb * pc.cw;
                eb = fma(-(snu * ib2), VS, eb);
                eb = fma(Mb, ks.sE, eb);
                gE += eb;
                gM += Mb;
                gT = fma(Mb, rw[0] - pc.tp, gT);
            }
        }
        double* o = part + (int64_t)(GP_K + p * GP_PL) * a.ldw;
        o[0] = gE; o[a.ldw] = gM; o[2 * a.ldw] = gT; o[3 * a.ldw] = gC; o[4 * a.ldw] = gK; o[5 * a.ldw] = gW;
    }
}

__global__ __launch_bounds__(WAVE) void k_gp_finish(GpArgs a) {
    const int64_t w = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (w >= a.W) return;
    const bool ok = a.k.ok[w] != 0.0;
    if (a.g_beta)
        for (int k = 0; k < a.K; ++k) {
            double x = 0.0;
            for (int t = 0; t < a.n_tasks; ++t) x += a.k.part[((int64_t)t * a.n_sums + k) * a.ldw + w];
            a.g_beta[(int64_t)k * a.ld + w] = ok ? x : 0.0;
        }
    if (!a.g_elems) return;
#pragma unroll 1
    for (int p = 0; p < a.P; ++p) {
        double out[OCTO_N_EL];
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) out[k] = 0.0;
        if (ok && gp_contributes(a, p)) {
            double g[FinL::PL_N];
#pragma unroll
            for (int k = 0; k < FinL::PL_N; ++k) g[k] = 0.0;
            for (int t = 0; t < a.n_tasks; ++t) {
                const double* part = a.k.part + ((int64_t)t * a.n_sums + GP_K + p * GP_PL) * a.ldw + w;
#pragma unroll
                for (int k = 0; k < GP_PL; ++k) g[FinL::GE + k] += part[(int64_t)k * a.ldw];
            }
            double elv[OCTO_N_EL];
#pragma unroll
            for (int k = 0; k < OCTO_N_EL; ++k) elv[k] = a.elems[((int64_t)p * OCTO_N_EL + k) * a.ld + w];
            const SetupOut so = setup_planet_vals<true>(elv, a.c, a.orbit_kind[p], a.has_mass[p]);
            FinPC fp;
            fp.sma = so.v[WC_A]; fp.P_d = rcp_nr<2>(so.v[WC_INVP]); fp.beta = so.v[WC_BETA];
            fp.si = so.v[WC_SINI]; fp.ci = so.v[WC_COSI]; fp.sO = so.v[WC_SINO]; fp.cO = so.v[WC_COSO]; fp.sw = so.v[WC_SINW]; fp.cw = so.v[WC_COSW];
            planet_finish<2, true, false, KM_RVABS>(so.el, out, 1, nullptr, 0, a.c, a.orbit_kind[p], a.has_mass[p], p, g, nullptr, fp, true);
        }
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) {
            double* o = a.g_elems + ((int64_t)p * OCTO_N_EL + k) * a.ld + w;
            *o = (a.accumulate ? *o : 0.0) + out[k];
        }
    }
}

inline int check_gp_table(octo_draws* h, const char* who) {
    return h->gp_n > 0 ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no Gaussian-process RV table (octo_draws_gp_set)");
}

void gp_drop_binding(octo_draws* h) {
    if (!h->gp_bound) return;
    h->gp_bound = 0; h->gp_n_bind = 0;
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->pf_W = 0; h->de_open = false; h->nest_passes = 0;      // a transition is never resumed on another target
}

template <int RP> constexpr size_t gp_back_lds() { return sizeof(double) * WAVE * (size_t)(N_CO * RP + 4 * RP + RP * (RP + 1) / 2 + 6 * RP); }

inline int gp_padded(int R) { return R <= 2 ? 2 : (R <= 4 ? 4 : 8); }

GpArgs gp_args(const octo_draws* h, const double* d_elems, int64_t ld, int64_t W, int64_t ldw) {
    GpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = h->d_gp_rows; a.n = h->gp_n; a.K = h->gp_K; a.P = h->gp_P; a.J = h->gp_J; a.H = h->gp_H;
    for (int j = 0; j < h->gp_J; ++j) a.term[j] = h->gp_term[j];
    for (int r = 0; r < GP_S; ++r) a.slot[r] = h->gp_slot[r];
    for (int p = 0; p < h->gp_P; ++p) { a.orbit_kind[p] = h->gp_kind[p]; a.has_mass[p] = h->gp_mass[p]; }
    a.c = dev_consts(h->gp_consts);
    a.elems = d_elems; a.ld = ld; a.W = W; a.ldw = ldw;
    a.n_tasks = (h->gp_n + GP_ROWS - 1) / GP_ROWS; a.n_seg = (h->gp_n + GP_G - 1) / GP_G; a.n_sums = GP_K + GP_PL * h->gp_P;
    return a;
}

template <int RP>
void gp_sequential(const GpArgs& a, hipStream_t st, bool factor, bool store, bool back) {
    const dim3 tiles((unsigned)(a.ldw / WAVE)), block(WAVE);
    if (factor) {
        if (store) hipLaunchKernelGGL((k_gp_factor<RP, true>), tiles, block, 0, st, a);
        else hipLaunchKernelGGL((k_gp_factor<RP, false>), tiles, block, 0, st, a);
    }
    if (back) hipLaunchKernelGGL((k_gp_back<RP>), tiles, block, gp_back_lds<RP>(), st, a);
}

// the launches of one evaluation on st; the rows of d_hyper, d_beta and their gradients are ld apart. want_mu: the reverse walk for α alone.
int gp_launch(octo_draws* h, hipStream_t st, const double* d_elems, int64_t ld, int64_t W, const double* d_hyper, const double* d_beta, const double* d_jitter,
              double* d_ll, double* d_g_elems, double* d_g_hyper, double* d_g_beta, double* d_g_jitter, int32_t accumulate, double* d_eta, double* d_mu, int64_t ld_out) {
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    GpArgs a = gp_args(h, d_elems, ld, W, ldw);
    const bool grad = d_g_elems || d_g_hyper || d_g_beta || d_g_jitter, back = grad || d_mu, seq = d_ll || back;
    const int RP = h->gp_RP;
    if (h->gp_dense) {      // no checkpoints and no states; the triangles of a long table
        GpdWork d;
        if (int rc = grow_to(h, h->d_gp, h->cap_gp, d, gpd_work, (int64_t)a.n, (int64_t)a.n_tasks, (int64_t)a.n_sums, ldw, W,
                             (int64_t)(a.n > OCTO_DRAWS_GP_DENSE_LDS_ROWS), (int64_t)grad)) return rc;
        a.k = GpWork{d.res, d.ok, nullptr, nullptr, d.part};
        a.tri = d.tri;
    } else if (int rc = grow_to(h, h->d_gp, h->cap_gp, a.k, gp_work, (int64_t)a.n, (int64_t)(RP * (RP + 1) / 2 + RP), (int64_t)a.n_seg, (int64_t)GP_G, (int64_t)a.n_tasks,
                                (int64_t)a.n_sums, ldw, (int64_t)back)) return rc;
    a.hyper = d_hyper; a.beta = d_beta; a.jitter = d_jitter; a.accumulate = accumulate;
    a.ll = d_ll; a.g_elems = d_g_elems; a.g_hyper = d_g_hyper; a.g_beta = d_g_beta; a.g_jitter = d_g_jitter;
    a.eta = d_eta; a.mu = d_mu; a.ld_out = ld_out;
    const dim3 grid((unsigned)(ldw / WAVE), (unsigned)a.n_tasks), tiles((unsigned)(ldw / WAVE)), block(WAVE);
    hipLaunchKernelGGL(k_gp_rows, grid, block, 0, st, a);
    if (h->gp_dense) {
        if (int rc = draws_gpd_launch(h, st, &a, d_ll != nullptr, back)) return rc;
    } else if (seq) {
        if (RP == 2) gp_sequential<2>(a, st, true, back, back);
        else if (RP == 4) gp_sequential<4>(a, st, true, back, back);
        else gp_sequential<8>(a, st, true, back, back);
    }
    if (d_g_elems || d_g_beta) {
        hipLaunchKernelGGL(k_gp_adj, grid, block, 0, st, a);
        hipLaunchKernelGGL(k_gp_finish, tiles, block, 0, st, a);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // namespace

int draws_gp_accumulate(octo_draws* h, hipStream_t st, const double* inputs, double* g_in, double* ll, int64_t ldw, int64_t W, int32_t n_in) {
    const int64_t H = h->gp_H, K = h->gp_K;
    const double* x = inputs + (int64_t)n_in * ldw;
    double* gx = g_in ? g_in + (int64_t)n_in * ldw : nullptr;
    return gp_launch(h, st, inputs, ldw, W, x, K ? x + H * ldw : nullptr, x + (H + K) * ldw, ll, g_in, gx, gx && K ? gx + H * ldw : nullptr,
                     gx ? gx + (H + K) * ldw : nullptr, 1, nullptr, nullptr, 0);
}

extern "C" {

int32_t octo_draws_gp_clear(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    gp_drop_binding(h);
    h->gp_n = 0; h->gp_K = 0; h->gp_P = 0; h->gp_J = 0; h->gp_R = 0; h->gp_RP = 0; h->gp_H = 0; h->gp_dense = 0;
    return OCTO_OK;
}

int32_t octo_draws_gp_set(octo_draws* h, const octo_planet_desc* planets, int32_t n_planets, const octo_consts* consts, const double* t, const double* rv,
                          const double* sigma, const double* c, int32_t K, int64_t n, const int32_t* term_kinds, int32_t n_terms) {
    const std::string who = "octo_draws_gp_set: ";
    if (!h) return OCTO_EINVAL;
    if (n < 1 || n > 65536) return fail(h, OCTO_EINVAL, who + "need 1 <= n <= 65536 rows");
    if (K < 0 || K > GP_K) return fail(h, OCTO_EINVAL, who + "need 0 <= K <= OCTO_DRAWS_GP_MAX_K design columns");
    if (n_planets < 1 || n_planets > OCTO_MAX_PLANETS) return fail(h, OCTO_EINVAL, who + "need 1 <= n_planets <= OCTO_MAX_PLANETS");
    if (n_terms < 1 || n_terms > GP_J) return fail(h, OCTO_EINVAL, who + "need 1 <= n_terms <= OCTO_DRAWS_GP_MAX_TERMS");
    if (!planets || !t || !rv || !sigma || !term_kinds || (K > 0 && !c)) return fail(h, OCTO_EINVAL, who + "null argument");
    for (int p = 0; p < n_planets; ++p) {
        const int kind = planets[p].orbit_kind;
        if (kind != OCTO_ORBIT_VISUAL_KEP && kind != OCTO_ORBIT_RADVEL && kind != OCTO_ORBIT_THIELE_INNES && kind != OCTO_ORBIT_KEP)
            return fail(h, OCTO_EINVAL, who + "planet " + std::to_string(p) + ": unknown orbit kind " + std::to_string(kind));
    }
    int32_t slot[GP_S], R = 0, H = 0, n_dense = 0;
    for (int j = 0; j < n_terms; ++j) {
        const int kind = term_kinds[j];
        if (gp_dense_kind(kind)) { ++n_dense; H += gp_dense_n_hyper(kind); continue; }      // the twentieth part: no slots
        if (kind != OCTO_DRAWS_GP_REAL && kind != OCTO_DRAWS_GP_COMPLEX && kind != OCTO_DRAWS_GP_SHO)
            return fail(h, OCTO_EINVAL, who + "term " + std::to_string(j) + ": unknown kind " + std::to_string(kind));
        if (kind == OCTO_DRAWS_GP_REAL) { slot[R++] = SLOT_REAL; H += 2; }
        else { slot[R++] = SLOT_FIRST; slot[R++] = SLOT_SECOND; H += kind == OCTO_DRAWS_GP_COMPLEX ? 4 : 3; }      // R <= 2·GP_J = GP_S
    }
    static_assert(2 * GP_J <= GP_S, "every term list fits the slots");
    if (n_dense != 0 && n_dense != n_terms) return fail(h, OCTO_EINVAL, who + "a term list is celerite kinds alone or dense kinds alone");
    const bool dense = n_dense != 0;
    if (dense && n > OCTO_DRAWS_GP_DENSE_MAX_N) return fail(h, OCTO_EINVAL, who + "a dense term list needs n <= OCTO_DRAWS_GP_DENSE_MAX_N rows");
    for (int r = R; r < GP_S; ++r) slot[r] = SLOT_PAD;
    std::vector<double> rows((size_t)n * GROWW, 0.0);
    for (int64_t r = 0; r < n; ++r) {
        bool fin = std::isfinite(t[r]) && std::isfinite(rv[r]) && std::isfinite(sigma[r]);
        for (int k = 0; k < K; ++k) fin = fin && std::isfinite(c[(int64_t)k * n + r]);
        if (!fin) return fail(h, OCTO_EINVAL, who + "row " + std::to_string(r) + ": a non-finite entry");
        if (!(sigma[r] > 0.0)) return fail(h, OCTO_EINVAL, who + "row " + std::to_string(r) + ": sigma must be > 0");
        if (r > 0 && t[r] < t[r - 1]) return fail(h, OCTO_EINVAL, who + "row " + std::to_string(r) + ": the epochs must not decrease");
        double* o = rows.data() + r * GROWW;
        o[0] = t[r]; o[1] = rv[r]; o[2] = sigma[r] * sigma[r];
        for (int k = 0; k < K; ++k) o[3 + k] = c[(int64_t)k * n + r];
    }
    for (int p = 0; p < n_planets; ++p)
        if (planets[p].orbit_kind == OCTO_ORBIT_THIELE_INNES && planets[p].has_mass)
            return fail(h, OCTO_ENOTSUP, who + "planet " + std::to_string(p) + ": a ThieleInnesOrbit planet with a mass has no radial velocity on the device path");
    octo_consts cst;
    if (consts) cst = *consts;
    else if (octo_consts_default(&cst) != OCTO_OK) return fail(h, OCTO_EINVAL, who + "octo_consts_default failed");
    OCHK(h, hipSetDevice(h->device));
    if (dense) {
        if (int rc = draws_gpd_prepare(h, n)) return rc;
    } else if (gp_padded(R) == 8 && hipFuncSetAttribute((const void*)k_gp_back<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gp_back_lds<8>()) != hipSuccess) {
        (void)hipGetLastError();      // beyond the default limit of dynamic LDS: raised for the one kernel that needs it
        return fail(h, OCTO_ENOTSUP, who + "eight slots need more LDS per block than this device gives");
    }
    octo_draws_gp_clear(h);
    if (int rc = grow(h, h->d_gp_rows, h->cap_gp_rows, (int64_t)rows.size())) return rc;
    OCHK(h, hipStreamSynchronize(h->stream));
    OCHK(h, hipMemcpy(h->d_gp_rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    h->gp_n = (int32_t)n; h->gp_K = K; h->gp_P = n_planets; h->gp_J = n_terms; h->gp_R = R; h->gp_RP = dense ? 0 : gp_padded(R); h->gp_H = H; h->gp_consts = cst;
    h->gp_dense = dense ? 1 : 0;
    for (int j = 0; j < n_terms; ++j) h->gp_term[j] = term_kinds[j];
    for (int r = 0; r < GP_S; ++r) h->gp_slot[r] = slot[r];
    for (int p = 0; p < n_planets; ++p) { h->gp_kind[p] = planets[p].orbit_kind; h->gp_mass[p] = planets[p].has_mass ? 1 : 0; }
    return OCTO_OK;
}

int64_t octo_draws_gp_work_doubles(int64_t n, int32_t n_slots, int32_t n_planets, int64_t W, int32_t grad) {
    if (n < 1 || n > 65536 || n_slots < 1 || n_slots > GP_S || n_planets < 1 || n_planets > OCTO_MAX_PLANETS || W < 0 || W > MAX_CHAINS) return -1;
    const int64_t RP = gp_padded(n_slots), ldw = (W + WAVE - 1) / WAVE * WAVE;
    return carve_size(gp_work, n, RP * (RP + 1) / 2 + RP, (n + GP_G - 1) / GP_G, (int64_t)GP_G, (n + GP_ROWS - 1) / GP_ROWS, (int64_t)(GP_K + GP_PL * n_planets), ldw,
                      (int64_t)(grad ? 1 : 0));
}

int64_t octo_draws_gp_dense_work_doubles(int64_t n, int32_t n_planets, int64_t W, int32_t grad) {
    if (n < 1 || n > OCTO_DRAWS_GP_DENSE_MAX_N || n_planets < 1 || n_planets > OCTO_MAX_PLANETS || W < 0 || W > MAX_CHAINS) return -1;
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    return carve_size(gpd_work, n, (n + GP_ROWS - 1) / GP_ROWS, (int64_t)(GP_K + GP_PL * n_planets), ldw, W, (int64_t)(n > OCTO_DRAWS_GP_DENSE_LDS_ROWS),
                      (int64_t)(grad ? 1 : 0));
}

int32_t octo_draws_gp_eval_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_hyper, const double* d_beta, const double* d_jitter,
                                  double* d_ll, double* d_g_elems, double* d_g_hyper, double* d_g_beta, double* d_g_jitter, int32_t accumulate, void* hip_stream) {
    const char* who = "octo_draws_gp_eval_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_gp_table(h, who)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    if (W == 0) return OCTO_OK;
    if (!d_elems || !d_hyper || !d_ll) return fail(h, OCTO_EINVAL, std::string(who) + ": d_elems, d_hyper or d_ll is NULL");
    if (h->gp_K > 0 && !d_beta) return fail(h, OCTO_EINVAL, std::string(who) + ": d_beta is NULL (K > 0)");
    OCHK(h, hipSetDevice(h->device));
    return gp_launch(h, stream_of(h, hip_stream), d_elems, ld, W, d_hyper, h->gp_K > 0 ? d_beta : nullptr, d_jitter, d_ll, d_g_elems, d_g_hyper,
                     h->gp_K > 0 ? d_g_beta : nullptr, d_g_jitter, accumulate ? 1 : 0, nullptr, nullptr, 0);
}

int32_t octo_draws_gp_eval(octo_draws* h, const double* elems, int64_t ld, int64_t W, const double* hyper, const double* beta, const double* jitter, double* ll,
                           double* g_elems, double* g_hyper, double* g_beta, double* g_jitter) {
    const char* who = "octo_draws_gp_eval";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_gp_table(h, who)) return rc;
    if (W < 0 || ld < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= W <= ld");
    if (W == 0) return OCTO_OK;
    if (!elems || !hyper || !ll) return fail(h, OCTO_EINVAL, std::string(who) + ": elems, hyper or ll is NULL");
    const int64_t P = h->gp_P, K = h->gp_K, H = h->gp_H, n_el = P * OCTO_N_EL;
    if (K > 0 && !beta) return fail(h, OCTO_EINVAL, std::string(who) + ": beta is NULL (K > 0)");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    GpStaging d;
    if (int rc = grow_to(h, h->d_gp_hst, h->cap_gp_hst, d, gp_staging, P, H, K, ld)) return rc;
    OCHK(h, hipMemcpyAsync(d.elems, elems, sizeof(double) * n_el * ld, hipMemcpyHostToDevice, st));
    OCHK(h, hipMemcpyAsync(d.hyper, hyper, sizeof(double) * H * ld, hipMemcpyHostToDevice, st));
    if (K > 0) OCHK(h, hipMemcpyAsync(d.beta, beta, sizeof(double) * K * ld, hipMemcpyHostToDevice, st));
    if (jitter) OCHK(h, hipMemcpyAsync(d.jitter, jitter, sizeof(double) * W, hipMemcpyHostToDevice, st));
    const bool want_gb = g_beta && K > 0;
    if (int rc = octo_draws_gp_eval_device(h, d.elems, ld, W, d.hyper, K > 0 ? d.beta : nullptr, jitter ? d.jitter : nullptr, d.ll, g_elems ? d.g_elems : nullptr,
                                           g_hyper ? d.g_hyper : nullptr, want_gb ? d.g_beta : nullptr, g_jitter ? d.g_jitter : nullptr, 0, OCTO_STREAM_CTX)) return rc;
    OCHK(h, hipMemcpyAsync(ll, d.ll, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    if (g_elems) OCHK(h, hipMemcpyAsync(g_elems, d.g_elems, sizeof(double) * n_el * ld, hipMemcpyDeviceToHost, st));
    if (g_hyper) OCHK(h, hipMemcpyAsync(g_hyper, d.g_hyper, sizeof(double) * H * ld, hipMemcpyDeviceToHost, st));
    if (want_gb) OCHK(h, hipMemcpyAsync(g_beta, d.g_beta, sizeof(double) * K * ld, hipMemcpyDeviceToHost, st));
    if (g_jitter) OCHK(h, hipMemcpyAsync(g_jitter, d.g_jitter, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

int32_t octo_draws_gp_values_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_hyper, const double* d_beta, const double* d_jitter,
                                    double* d_eta, double* d_mu, int64_t ld_out, void* hip_stream) {
    const char* who = "octo_draws_gp_values_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_gp_table(h, who)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    if (ld_out < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need ld_out >= W");
    if (W == 0) return OCTO_OK;
    if (!d_elems || (!d_eta && !d_mu)) return fail(h, OCTO_EINVAL, std::string(who) + ": d_elems is NULL, or both d_eta and d_mu are");
    if (d_mu && !d_hyper) return fail(h, OCTO_EINVAL, std::string(who) + ": d_mu needs d_hyper");
    OCHK(h, hipSetDevice(h->device));
    return gp_launch(h, stream_of(h, hip_stream), d_elems, ld, W, d_hyper, h->gp_K > 0 ? d_beta : nullptr, d_jitter, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                     d_eta, d_mu, ld_out);
}

int32_t octo_draws_gp_unbind(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    gp_drop_binding(h);
    return OCTO_OK;
}

int32_t octo_draws_gp_bind(octo_draws* h, const octo_draws_bind* binds, int32_t n_binds) {
    const char* who = "octo_draws_gp_bind";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_gp_table(h, who)) return rc;
    if (!h->prog_ops || !h->ctx) return fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no program (octo_draws_program_set)");
    if (h->scan_bound) return fail(h, OCTO_ENOTSUP, std::string(who) + ": a scan table is bound (octo_draws_scan_bind): one bound table a handle");
    if (h->pma_bound) return fail(h, OCTO_ENOTSUP, std::string(who) + ": a catalogue table is bound (octo_draws_pma_bind): one bound table a handle");
    if (h->prog_planets != h->gp_P)
        return fail(h, OCTO_EINVAL, std::string(who) + ": the program has " + std::to_string(h->prog_planets) + " planets, the table " + std::to_string(h->gp_P));
    const int32_t want = h->gp_H + h->gp_K + 1;
    if (n_binds != want || !binds) return fail(h, OCTO_EINVAL, std::string(who) + ": need " + std::to_string(want) + " bindings (H + K + 1)");
    const int N = h->D + h->prog_n_ops;
    for (int k = 0; k < n_binds; ++k) {
        if (binds[k].kind != OCTO_DRAWS_BIND_NODE) return fail(h, OCTO_EINVAL, std::string(who) + ": binding " + std::to_string(k) + " must be an OCTO_DRAWS_BIND_NODE");
        if (binds[k].node < 0 || binds[k].node >= N) return fail(h, OCTO_EINVAL, std::string(who) + ": binding " + std::to_string(k) + ": node out of range");
    }
    OCHK(h, hipSetDevice(h->device));
    gp_drop_binding(h);
    // the program's bindings and the bound nodes behind them, 16 bytes each: two doubles' room
    const int64_t n_all = (int64_t)h->prog_n_in + n_binds;
    if (int rc = grow(h, h->d_gp_binds, h->cap_gp_binds, 2 * n_all)) return rc;
    OCHK(h, hipStreamSynchronize(h->stream));
    octo_draws_bind* d = (octo_draws_bind*)h->d_gp_binds;
    OCHK(h, hipMemcpy(d, h->prog_binds, sizeof(octo_draws_bind) * (size_t)h->prog_n_in, hipMemcpyDeviceToDevice));
    OCHK(h, hipMemcpy(d + h->prog_n_in, binds, sizeof(octo_draws_bind) * (size_t)n_binds, hipMemcpyHostToDevice));
    h->gp_bound = 1; h->gp_n_bind = n_binds;
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->pf_W = 0; h->de_open = false; h->nest_passes = 0;
    return OCTO_OK;
}

}  // extern "C"
