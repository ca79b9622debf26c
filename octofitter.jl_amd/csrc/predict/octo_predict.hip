// octo_predict.hip — liboctofitter_hip_predict.so: posterior-predictive model values on the device (include/octofitter_hip_predict.h).
// Of the main library's sources it INCLUDES the device routines the likelihood kernels run — setup_planet_vals / setup_valid (orbit
// constructors and validity, octo_kernels.h), load_pc / set_starter / the cold kepler_solve / atan2_fast (octo_device.h), sqrt_fast — so a
// prediction is made from the constants the likelihood was made from. It calls one symbol of the main library, octo_consts_default.
// What it shares with the pointwise library (walker_setup, planet_prims, wave_sum, dev_consts) is in companion/octo_companion_device.h, the
// host scaffold of every companion (handle base, fail, OCHK, open_device, grow, ensure_stage) in companion/octo_companion_host.h.
//
//   k_predict_cube<P, WPL>   lane = walker (WPL adjacent walkers per lane), block = 256 lanes × one chunk of epochs. Prologue: the orbit
//                            constructors of the block's walkers, constants in registers. Epoch loop: the epoch (and basis) are wave-uniform
//                            scalar loads; per planet one cold Kepler solve and the three primitives (raoff, decoff, V = radvel / K); per
//                            channel channel_value() and ONE store per lane, contiguous across the wave (8·WPL bytes per lane).
//   k_predict_cube_n         the same for 5 … OCTO_MAX_PLANETS planets: a run-time loop over the planets, block = one wave, the
//                            constants and the primitives in LDS (one column per lane: no barrier).
//   k_predict_part<P> / _n   the band: per (channel, epoch) each wave reduces its 64 values exactly (count by ballot, mean = Σ/n, M2 = Σ(x − mean)²,
//                            min, max: xor butterflies, every lane the same bits), the block's four waves are Chan-merged in wave order
//                            through LDS: one partial per block of 256 walkers.
//   k_predict_merge          one thread per (channel, epoch): Chan merge of the block partials in index order, then sd = √(M2/(n − 1)).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "octo_companion_device.h"
#include "octo_companion_host.h"
#include "octofitter_hip_predict.h"

namespace {
using namespace octo;

constexpr int TPB = 256;               // lanes per block of the templated kernels
constexpr int EPB = 32;                // epochs per block (at least): the prologue's ~350 FP64 instructions per planet are < 10 % of the chunk's
constexpr int MAXC = OCTO_PREDICT_MAX_CHANNELS;
constexpr int NSTAT = 5;               // n_valid, mean, sd | M2, min, max

struct Chan8 { int8_t q, p; };

struct PredictArgs {
    const double* elems; const double* add0; const double* add1;      // [P*9][ld], [C][ld] or null
    const double* epochs; const double* basis;                        // [T], [T] or null
    double* out;                                                      // cube [C*T][ld_out] | block partials [tiles][NSTAT][C*T]
    int64_t ld, W, ld_out, T;
    int32_t epb, P, C, need;
    int32_t orbit_kind[MAXP];
    int32_t has_mass[MAXP];
    DevConsts c;
    Chan8 ch[MAXC];
};

__host__ __device__ __forceinline__ bool is_rv_quantity(int q) { return q == OCTO_PREDICT_RADVEL || q == OCTO_PREDICT_RV_STAR || q == OCTO_PREDICT_RV_REL; }

// One walker's system: the planets' constants and, per epoch, their primitives. REGISTERS for the templated planet counts (every loop over
// the planets unrolls, every index is a constant); LDS columns for the run-time count.
template <int P>
struct RegSys {
    PC pc[P];
    double ra_[P], de_[P], V_[P];
    __device__ __forceinline__ static constexpr int n() { return P; }
    __device__ __forceinline__ double a(int p) const { return pc[p].a; }
    __device__ __forceinline__ double mu(int p) const { return pc[p].mu; }
    __device__ __forceinline__ double K(int p) const { return pc[p].K; }
    __device__ __forceinline__ double ra(int p) const { return ra_[p]; }
    __device__ __forceinline__ double de(int p) const { return de_[p]; }
    __device__ __forceinline__ double V(int p) const { return V_[p]; }
};

constexpr int LDS_PRIM = 3;      // raoff, decoff, V per planet
struct LdsSys {
    const double* wc;            // [P][NWC][WAVE] the block's constants (this lane's column: + lane)
    const double* prim;          // [P][LDS_PRIM][WAVE]
    int np;
    __device__ __forceinline__ int n() const { return np; }
    __device__ __forceinline__ double a(int p) const { return wc[(p * NWC + WC_A) * WAVE]; }
    __device__ __forceinline__ double mu(int p) const { return wc[(p * NWC + WC_MU) * WAVE]; }
    __device__ __forceinline__ double K(int p) const { return wc[(p * NWC + WC_K) * WAVE]; }
    __device__ __forceinline__ double ra(int p) const { return prim[(p * LDS_PRIM + 0) * WAVE]; }
    __device__ __forceinline__ double de(int p) const { return prim[(p * LDS_PRIM + 1) * WAVE]; }
    __device__ __forceinline__ double V(int p) const { return prim[(p * LDS_PRIM + 2) * WAVE]; }
};

// THE value of channel (q, pl) from a system's primitives: every entry point's numbers come from this routine.
//   RV quantities: rv_row's model — fma(add1, basis, add0), then one fma(g_p·K_p, V_p, ·) per planet in planet order, g_p = 1 for the channel's
//   planet, −m/M for every planet (RV_STAR) or for the strictly inner ones (RV_REL), else 0.
//   Astrometric quantities: astrom_row's model — Σ_p f_p·raoff_p in planet order, f_p = 1 for the channel's planet, m/M for the strictly
//   inner ones (ASTROM_*), else 0; ρ = √(x² + y²), PA = atan2(x, y).
// q and pl are wave-uniform: every branch on them is a scalar branch.
template <class S>
__device__ __forceinline__ double channel_value(const S& s, int q, int pl, double add0, double add1, double basis) {
    const int n = s.n();
    double a_this = 0.0;
#pragma unroll
    for (int p = 0; p < n; ++p) a_this = (p == pl) ? s.a(p) : a_this;
    if (is_rv_quantity(q)) {
        double model = fma(add1, basis, add0);
#pragma unroll
        for (int p = 0; p < n; ++p) {
            const double mu = s.mu(p);
            const double g = (q == OCTO_PREDICT_RV_STAR) ? -mu : ((p == pl) ? 1.0 : ((q == OCTO_PREDICT_RV_REL && s.a(p) < a_this) ? -mu : 0.0));
            model = fma(g * s.K(p), s.V(p), model);
        }
        return model;
    }
    const bool composite = q >= OCTO_PREDICT_ASTROM_RA;
    double x = 0.0, y = 0.0;
#pragma unroll
    for (int p = 0; p < n; ++p) {
        const double f = (p == pl) ? 1.0 : ((composite && s.a(p) < a_this) ? s.mu(p) : 0.0);
        x = fma(f, s.ra(p), x);
        y = fma(f, s.de(p), y);
    }
    if (q == OCTO_PREDICT_RAOFF || q == OCTO_PREDICT_ASTROM_RA) return x;
    if (q == OCTO_PREDICT_DECOFF || q == OCTO_PREDICT_ASTROM_DEC) return y;
    if (q == OCTO_PREDICT_SEP || q == OCTO_PREDICT_ASTROM_SEP) return sqrt_fast(fma(x, x, y * y));
    const bool origin = x == 0.0 && y == 0.0;                    // atan2_fast wants a direction: atan(0, 0) = 0
    double pa = atan2_fast(x, origin ? 1.0 : y);
    pa = pa <= -PI ? PI : pa;                                    // (−π, π]
    return pa;
}

// channel c's additive terms of walker wl (RV channels with rows given; otherwise 0)
__device__ __forceinline__ void channel_add(const PredictArgs& a, int c, int q, int64_t wl, double& add0, double& add1) {
    add0 = 0.0; add1 = 0.0;
    if (is_rv_quantity(q)) {
        if (a.add0) add0 = a.add0[(int64_t)c * a.ld + wl];
        if (a.add1 && a.basis) add1 = a.add1[(int64_t)c * a.ld + wl];
    }
}

template <int P, int WPL>
__device__ __forceinline__ void block_setup(const PredictArgs& a, int64_t w0, RegSys<P> (&sys)[WPL], bool (&live)[WPL], bool (&ok)[WPL], int64_t (&wl)[WPL]) {
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
        live[k] = w0 + k < a.W;
        wl[k] = live[k] ? w0 + k : a.W - 1;      // a dead lane repeats the last walker: every load stays inside the arrays
        ok[k] = true;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            double v[NWC];
            ok[k] = walker_setup(a, p, wl[k], v) && ok[k];
            load_pc(sys[k].pc[p], v, 1, 0, 0);
        }
    }
}

// The single-planet kernels are held to 128 registers (four waves per SIMD); with more planets the constants decide.
template <int P, int WPL>
__global__ __launch_bounds__(TPB, (P == 1 ? 4 : 1)) void k_predict_cube(PredictArgs a) {
    const int64_t w0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * WPL;
    RegSys<P> sys[WPL];
    bool live[WPL], ok[WPL];
    int64_t wl[WPL];
    block_setup<P, WPL>(a, w0, sys, live, ok, wl);
    const int64_t j0 = (int64_t)blockIdx.y * a.epb, j1 = j0 + a.epb < a.T ? j0 + a.epb : a.T;
    for (int64_t j = j0; j < j1; ++j) {
        const double t = a.epochs[j];
        const double basis = a.basis ? a.basis[j] : 0.0;
#pragma unroll
        for (int k = 0; k < WPL; ++k)
#pragma unroll
            for (int p = 0; p < P; ++p) planet_prims(sys[k].pc[p], t, a.need, sys[k].ra_[p], sys[k].de_[p], sys[k].V_[p]);
        for (int c = 0; c < a.C; ++c) {
            const int q = a.ch[c].q, pl = a.ch[c].p;
            double v[WPL];
#pragma unroll
            for (int k = 0; k < WPL; ++k) {
                double add0, add1;
                channel_add(a, c, q, wl[k], add0, add1);
                v[k] = channel_value(sys[k], q, pl, add0, add1, basis);
                v[k] = ok[k] ? v[k] : NAN;
            }
            double* o = a.out + ((int64_t)c * a.T + j) * a.ld_out + w0;
            if constexpr (WPL == 2) {
                if (live[1]) *reinterpret_cast<double2*>(o) = make_double2(v[0], v[1]);      // the host takes this variant only for an even ld_out and a 16-byte aligned cube
                else if (live[0]) o[0] = v[0];
            } else {
                if (live[0]) o[0] = v[0];
            }
        }
    }
}

// ---- 5 … OCTO_MAX_PLANETS planets: block = one wave, constants and primitives in LDS -----------------------------------------------------
struct LdsBlock {
    double wc[MAXP * NWC * WAVE];
    double prim[MAXP * LDS_PRIM * WAVE];
};

__device__ __forceinline__ bool lds_setup(const PredictArgs& a, LdsBlock& L, int lane, int64_t wl) {
    bool ok = true;
    for (int p = 0; p < a.P; ++p) {
        double v[NWC];
        ok = walker_setup(a, p, wl, v) && ok;
#pragma unroll
        for (int k = 0; k < NWC; ++k) L.wc[(p * NWC + k) * WAVE + lane] = v[k];
    }
    return ok;
}

__device__ __forceinline__ void lds_prims(const PredictArgs& a, LdsBlock& L, int lane, double t) {
    for (int p = 0; p < a.P; ++p) {
        PC pc;
        load_pc(pc, L.wc, WAVE, p, lane);
        double ra, de, V;
        planet_prims(pc, t, a.need, ra, de, V);
        L.prim[(p * LDS_PRIM + 0) * WAVE + lane] = ra;
        L.prim[(p * LDS_PRIM + 1) * WAVE + lane] = de;
        L.prim[(p * LDS_PRIM + 2) * WAVE + lane] = V;
    }
}

__global__ __launch_bounds__(WAVE) void k_predict_cube_n(PredictArgs a) {
    __shared__ LdsBlock L;
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = w < a.W;
    const int64_t wl = live ? w : a.W - 1;
    const bool ok = lds_setup(a, L, lane, wl);
    const LdsSys sys{L.wc + lane, L.prim + lane, a.P};
    const int64_t j0 = (int64_t)blockIdx.y * a.epb, j1 = j0 + a.epb < a.T ? j0 + a.epb : a.T;
    for (int64_t j = j0; j < j1; ++j) {
        const double t = a.epochs[j];
        const double basis = a.basis ? a.basis[j] : 0.0;
        lds_prims(a, L, lane, t);
        for (int c = 0; c < a.C; ++c) {
            const int q = a.ch[c].q, pl = a.ch[c].p;
            double add0, add1;
            channel_add(a, c, q, wl, add0, add1);
            const double v = channel_value(sys, q, pl, add0, add1, basis);
            if (live) a.out[((int64_t)c * a.T + j) * a.ld_out + w] = ok ? v : NAN;
        }
    }
}

// ---- the band ----------------------------------------------------------------------------------------------------------------------------
struct Stat { double n, mean, m2, mn, mx; };

// Chan, Golub & LeVeque's pairwise update; an empty side leaves the other untouched
__device__ __forceinline__ void stat_merge(Stat& s, const Stat& b) {
    if (b.n == 0.0) return;
    if (s.n == 0.0) { s = b; return; }
    const double nt = s.n + b.n, d = b.mean - s.mean;
    s.mean = fma(d, b.n / nt, s.mean);
    s.m2 = s.m2 + b.m2 + d * d * (s.n * b.n / nt);
    s.n = nt;
    s.mn = fmin(s.mn, b.mn); s.mx = fmax(s.mx, b.mx);
}

// the wave's 64 values, exactly: two passes over registers
__device__ __forceinline__ Stat wave_stat(double x, bool valid) {
    Stat s;
    s.n = (double)__popcll(__ballot(valid));
    s.mean = wave_sum(valid ? x : 0.0) / s.n;                    // n = 0: NaN, never read (stat_merge)
    const double d = valid ? x - s.mean : 0.0;
    s.m2 = wave_sum(d * d);
    double mn = valid ? x : INFINITY, mx = valid ? x : -INFINITY;
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) { mn = fmin(mn, __shfl_xor(mn, m, WAVE)); mx = fmax(mx, __shfl_xor(mx, m, WAVE)); }
    s.mn = mn; s.mx = mx;
    return s;
}

// block partial of (tile, c, j): out[(tile·NSTAT + k)·C·T + c·T + j]
__device__ __forceinline__ void part_store(const PredictArgs& a, int64_t tile, int c, int64_t j, const Stat& s) {
    const int64_t CT = (int64_t)a.C * a.T;
    double* o = a.out + tile * NSTAT * CT + (int64_t)c * a.T + j;
    o[0] = s.n; o[CT] = s.mean; o[2 * CT] = s.m2; o[3 * CT] = s.mn; o[4 * CT] = s.mx;
}

template <int P>
__global__ __launch_bounds__(TPB) void k_predict_part(PredictArgs a) {
    constexpr int NWV = TPB / WAVE;
    __shared__ double sh[2][NWV][MAXC][NSTAT];
    const int64_t w0 = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    RegSys<P> sys[1];
    bool live[1], ok[1];
    int64_t wl[1];
    block_setup<P, 1>(a, w0, sys, live, ok, wl);
    const int64_t j0 = (int64_t)blockIdx.y * a.epb, j1 = j0 + a.epb < a.T ? j0 + a.epb : a.T;
    for (int64_t j = j0; j < j1; ++j) {
        const double t = a.epochs[j];
        const double basis = a.basis ? a.basis[j] : 0.0;
        const int buf = (int)(j & 1);      // two buffers: one barrier per epoch
#pragma unroll
        for (int p = 0; p < P; ++p) planet_prims(sys[0].pc[p], t, a.need, sys[0].ra_[p], sys[0].de_[p], sys[0].V_[p]);
        for (int c = 0; c < a.C; ++c) {
            const int q = a.ch[c].q, pl = a.ch[c].p;
            double add0, add1;
            channel_add(a, c, q, wl[0], add0, add1);
            const double v = channel_value(sys[0], q, pl, add0, add1, basis);
            const Stat s = wave_stat(v, live[0] && ok[0] && v == v);
            if (lane == 0) { double* o = sh[buf][wv][c]; o[0] = s.n; o[1] = s.mean; o[2] = s.m2; o[3] = s.mn; o[4] = s.mx; }
        }
        __syncthreads();
        if ((int)threadIdx.x < a.C) {
            const int c = threadIdx.x;
            Stat s{0.0, 0.0, 0.0, INFINITY, -INFINITY};
#pragma unroll
            for (int w = 0; w < NWV; ++w) { const double* o = sh[buf][w][c]; stat_merge(s, Stat{o[0], o[1], o[2], o[3], o[4]}); }
            part_store(a, blockIdx.x, c, j, s);
        }
    }
}

// 5 … OCTO_MAX_PLANETS planets: block = one wave = one partial of 64 walkers
__global__ __launch_bounds__(WAVE) void k_predict_part_n(PredictArgs a) {
    __shared__ LdsBlock L;
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = w < a.W;
    const int64_t wl = live ? w : a.W - 1;
    const bool ok = lds_setup(a, L, lane, wl);
    const LdsSys sys{L.wc + lane, L.prim + lane, a.P};
    const int64_t j0 = (int64_t)blockIdx.y * a.epb, j1 = j0 + a.epb < a.T ? j0 + a.epb : a.T;
    for (int64_t j = j0; j < j1; ++j) {
        const double t = a.epochs[j];
        const double basis = a.basis ? a.basis[j] : 0.0;
        lds_prims(a, L, lane, t);
        for (int c = 0; c < a.C; ++c) {
            const int q = a.ch[c].q, pl = a.ch[c].p;
            double add0, add1;
            channel_add(a, c, q, wl, add0, add1);
            const double v = channel_value(sys, q, pl, add0, add1, basis);
            Stat s = wave_stat(v, live && ok && v == v);
            if (s.n == 0.0) { s.mean = 0.0; s.m2 = 0.0; }
            if (lane == 0) part_store(a, blockIdx.x, c, j, s);
        }
    }
}

// out [NSTAT][C·T] from part [tiles][NSTAT][C·T]
__global__ __launch_bounds__(TPB) void k_predict_merge(const double* __restrict__ part, int64_t tiles, int64_t CT, double* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (k >= CT) return;
    Stat s{0.0, 0.0, 0.0, INFINITY, -INFINITY};
    for (int64_t b = 0; b < tiles; ++b) {
        const double* o = part + b * NSTAT * CT + k;
        stat_merge(s, Stat{o[0], o[CT], o[2 * CT], o[3 * CT], o[4 * CT]});
    }
    const bool none = s.n == 0.0;
    out[k] = s.n;
    out[CT + k] = none ? NAN : s.mean;
    out[2 * CT + k] = none ? NAN : sqrt(s.m2 / (s.n - 1.0));      // n = 1: 0/0 = NaN
    out[3 * CT + k] = none ? NAN : s.mn;
    out[4 * CT + k] = none ? NAN : s.mx;
}

}  // namespace

struct octo_predict : CompanionStaged {
    int P = 0, C = 0, need = 0, variant = 0;
    int64_t T = 0;
    PredictArgs base;                       // everything of a launch that the handle fixes
    double *d_epochs = nullptr, *d_basis = nullptr;
    // summary: block partials (grown on demand)
    double* d_part = nullptr; int64_t cap_part = 0;
    // host-buffer calls: inputs, cube chunk, summary result (grown on demand)
    double* d_in = nullptr; int64_t cap_in = 0;
    double* d_cube = nullptr; int64_t cap_cube = 0;
    double* d_sum = nullptr;
    int64_t cube_bytes = (int64_t)64 << 20;
};

namespace {

int check_batch(octo_predict* h, const char* who, const void* elems, const void* out, int64_t ld, int64_t W, int64_t w_min) {
    if (W < w_min || ld < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need " + std::to_string(w_min) + " <= W <= ld");
    if (W > 0 && (!elems || !out)) return fail(h, OCTO_EINVAL, std::string(who) + ": null elements or output");
    return OCTO_OK;
}

int32_t epochs_per_block(int64_t T) { return (int32_t)std::max<int64_t>(EPB, (T + 65534) / 65535); }

constexpr int MAXP_WIDE = 2;      // two walkers per lane double the constants in registers: compiled for one and two planets only

void launch_cube(const PredictArgs& a, hipStream_t st, bool wide) {
    const int wpl = wide ? 2 : 1;
    const dim3 grid((unsigned)((a.W + (int64_t)TPB * wpl - 1) / ((int64_t)TPB * wpl)), (unsigned)((a.T + a.epb - 1) / a.epb));
    switch (a.P) {
    case 1: if (wide) hipLaunchKernelGGL((k_predict_cube<1, 2>), grid, dim3(TPB), 0, st, a); else hipLaunchKernelGGL((k_predict_cube<1, 1>), grid, dim3(TPB), 0, st, a); break;
    case 2: if (wide) hipLaunchKernelGGL((k_predict_cube<2, 2>), grid, dim3(TPB), 0, st, a); else hipLaunchKernelGGL((k_predict_cube<2, 1>), grid, dim3(TPB), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_predict_cube<3, 1>), grid, dim3(TPB), 0, st, a); break;
    default: hipLaunchKernelGGL((k_predict_cube<4, 1>), grid, dim3(TPB), 0, st, a); break;
    }
}

int64_t summary_tiles(const octo_predict* h, int64_t W) { return h->P <= MAXP_T ? (W + TPB - 1) / TPB : (W + WAVE - 1) / WAVE; }

}  // namespace

extern "C" {

int32_t octo_predict_create(int32_t device_id, const octo_consts* consts, const octo_planet_desc* planets, int32_t n_planets,
                            const double* epochs, int64_t T, const double* basis, const octo_predict_channel* channels, int32_t n_channels,
                            octo_predict** out) {
    if (!out) return fail(nullptr, OCTO_EINVAL, "octo_predict_create: null out pointer");
    *out = nullptr;
    if (!planets || !epochs || !channels) return fail(nullptr, OCTO_EINVAL, "octo_predict_create: null argument");
    if (n_planets < 1 || n_planets > OCTO_MAX_PLANETS) return fail(nullptr, OCTO_EINVAL, "octo_predict_create: 1 <= n_planets <= OCTO_MAX_PLANETS");
    if (n_channels < 1 || n_channels > OCTO_PREDICT_MAX_CHANNELS) return fail(nullptr, OCTO_EINVAL, "octo_predict_create: 1 <= n_channels <= OCTO_PREDICT_MAX_CHANNELS");
    if (T < 1) return fail(nullptr, OCTO_EINVAL, "octo_predict_create: T >= 1");
    bool any_noplx = false, any_ti = false;
    for (int p = 0; p < n_planets; ++p) {
        const int k = planets[p].orbit_kind;
        if (k != OCTO_ORBIT_VISUAL_KEP && k != OCTO_ORBIT_RADVEL && k != OCTO_ORBIT_THIELE_INNES && k != OCTO_ORBIT_KEP)
            return fail(nullptr, OCTO_EINVAL, "octo_predict_create: unknown orbit kind");
        any_noplx = any_noplx || k == OCTO_ORBIT_RADVEL || k == OCTO_ORBIT_KEP;
        any_ti = any_ti || k == OCTO_ORBIT_THIELE_INNES;
    }
    int need = 0;
    for (int c = 0; c < n_channels; ++c) {
        const int q = channels[c].quantity, pl = channels[c].planet;
        const std::string who = "octo_predict_create: channel " + std::to_string(c);
        if (q < 0 || q >= OCTO_PREDICT_N_QUANTITIES) return fail(nullptr, OCTO_EINVAL, who + ": unknown quantity");
        if (q == OCTO_PREDICT_RV_STAR) { if (pl != -1) return fail(nullptr, OCTO_EINVAL, who + ": RV_STAR takes planet = -1"); }
        else if (pl < 0 || pl >= n_planets) return fail(nullptr, OCTO_EINVAL, who + ": planet index outside the system");
        if (is_rv_quantity(q)) {
            need |= NEED_RV;
            const bool ti = q == OCTO_PREDICT_RADVEL ? planets[pl].orbit_kind == OCTO_ORBIT_THIELE_INNES : any_ti;
            if (ti) return fail(nullptr, OCTO_EINVAL, who + ": an RV quantity with a ThieleInnesOrbit planet");
        } else {
            need |= NEED_AST;
            const int k = planets[pl].orbit_kind;
            if (k == OCTO_ORBIT_RADVEL || k == OCTO_ORBIT_KEP || (q >= OCTO_PREDICT_ASTROM_RA && any_noplx))
                return fail(nullptr, OCTO_EINVAL, who + ": an astrometric quantity with a planet that has no parallax (RadialVelocityOrbit / KepOrbit)");
        }
    }
    for (int64_t j = 0; j < T; ++j)
        if (!std::isfinite(epochs[j]) || (basis && !std::isfinite(basis[j]))) return fail(nullptr, OCTO_EINVAL, "octo_predict_create: non-finite epoch or basis value");
    octo_consts cst;
    if (consts) cst = *consts;
    else if (octo_consts_default(&cst) != OCTO_OK) return fail(nullptr, OCTO_EINVAL, "octo_predict_create: octo_consts_default failed");

    octo_predict* h;
    { int rc = open_device(device_id, "octo_predict_create: ", h); if (rc) return rc; }
    h->P = n_planets; h->C = n_channels; h->T = T; h->need = need;
    h->cube_bytes = env_bytes("OCTO_PREDICT_CUBE_BYTES", h->cube_bytes);
    h->stage_bytes = env_bytes("OCTO_PREDICT_STAGE_BYTES", h->stage_bytes);
    auto bail = [&](int code, const char* msg) { octo_predict_destroy(h); return fail(nullptr, code, msg); };
    if (hipMalloc((void**)&h->d_epochs, sizeof(double) * T) != hipSuccess || (basis && hipMalloc((void**)&h->d_basis, sizeof(double) * T) != hipSuccess) ||
        hipMalloc((void**)&h->d_sum, sizeof(double) * NSTAT * n_channels * T) != hipSuccess)
        return bail(OCTO_ENOMEM, "octo_predict_create: hipMalloc failed");
    if (hipMemcpy(h->d_epochs, epochs, sizeof(double) * T, hipMemcpyHostToDevice) != hipSuccess ||
        (basis && hipMemcpy(h->d_basis, basis, sizeof(double) * T, hipMemcpyHostToDevice) != hipSuccess))
        return bail(OCTO_EHIP, "octo_predict_create: upload failed");
    PredictArgs& a = h->base;
    std::memset(&a, 0, sizeof(a));
    a.epochs = h->d_epochs; a.basis = h->d_basis; a.T = T; a.epb = epochs_per_block(T); a.P = n_planets; a.C = n_channels; a.need = need;
    for (int p = 0; p < n_planets; ++p) { a.orbit_kind[p] = planets[p].orbit_kind; a.has_mass[p] = planets[p].has_mass ? 1 : 0; }
    a.c = dev_consts(cst);
    for (int c = 0; c < n_channels; ++c) { a.ch[c].q = (int8_t)channels[c].quantity; a.ch[c].p = (int8_t)channels[c].planet; }
    *out = h;
    return OCTO_OK;
}

int32_t octo_predict_destroy(octo_predict* h) {
    if (!h) return OCTO_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    (void)hipFree(h->d_epochs); (void)hipFree(h->d_basis); (void)hipFree(h->d_part); (void)hipFree(h->d_in); (void)hipFree(h->d_cube); (void)hipFree(h->d_sum);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    delete h;
    return OCTO_OK;
}

const char* octo_predict_last_error(const octo_predict* h) { return last_error(h); }

int32_t octo_predict_sync(octo_predict* h) { return sync_handle(h); }

int32_t octo_predict_set_variant(octo_predict* h, int32_t variant) {
    if (!h) return OCTO_EINVAL;
    if (variant < 0 || variant > 2) return fail(h, OCTO_EINVAL, "octo_predict_set_variant: 0 <= variant <= 2");
    h->variant = variant;
    return OCTO_OK;
}

int32_t octo_predict_eval_device(octo_predict* h, const double* d_elems, int64_t ld, int64_t W, const double* d_add0, const double* d_add1,
                                 double* d_out, int64_t ld_out, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_predict_eval_device", d_elems, d_out, ld, W, 0); if (rc) return rc; }
    if (ld_out < W) return fail(h, OCTO_EINVAL, "octo_predict_eval_device: need W <= ld_out");
    if (W == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    PredictArgs a = h->base;
    a.elems = d_elems; a.add0 = d_add0; a.add1 = d_add1; a.ld = ld; a.W = W; a.out = d_out; a.ld_out = ld_out;
    if (h->P > MAXP_T) {
        hipLaunchKernelGGL(k_predict_cube_n, dim3((unsigned)((W + WAVE - 1) / WAVE), (unsigned)((a.T + a.epb - 1) / a.epb)), dim3(WAVE), 0, st, a);
    } else {
        // variant 0: wide stores for one planet (128 registers: still four waves per SIMD), narrow otherwise; 2 forces them wherever they are compiled
        const bool can_wide = h->P <= MAXP_WIDE && W >= 2 && (ld_out % 2) == 0 && ((uintptr_t)d_out % 16) == 0;
        const bool wide = can_wide && (h->variant == 2 || (h->variant == 0 && h->P == 1));
        launch_cube(a, st, wide);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_predict_summary_device(octo_predict* h, const double* d_elems, int64_t ld, int64_t W, const double* d_add0, const double* d_add1,
                                    double* d_out, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_predict_summary_device", d_elems, d_out, ld, W, 1); if (rc) return rc; }
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t tiles = summary_tiles(h, W), CT = (int64_t)h->C * h->T;
    { int rc = grow(h, h->d_part, h->cap_part, tiles * NSTAT * CT); if (rc) return rc; }
    PredictArgs a = h->base;
    a.elems = d_elems; a.add0 = d_add0; a.add1 = d_add1; a.ld = ld; a.W = W; a.out = h->d_part; a.ld_out = 0;
    const dim3 grid((unsigned)tiles, (unsigned)((a.T + a.epb - 1) / a.epb));
    switch (h->P) {
    case 1: hipLaunchKernelGGL(k_predict_part<1>, grid, dim3(TPB), 0, st, a); break;
    case 2: hipLaunchKernelGGL(k_predict_part<2>, grid, dim3(TPB), 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_predict_part<3>, grid, dim3(TPB), 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_predict_part<4>, grid, dim3(TPB), 0, st, a); break;
    default: hipLaunchKernelGGL(k_predict_part_n, grid, dim3(WAVE), 0, st, a); break;
    }
    hipLaunchKernelGGL(k_predict_merge, dim3((unsigned)((CT + TPB - 1) / TPB)), dim3(TPB), 0, st, (const double*)h->d_part, tiles, CT, d_out);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

// elems [P*9][ld] and the add rows [C][ld] -> d_in, packed with leading dimension W: elements, then add0, then add1
static int upload_inputs(octo_predict* h, const double* elems, int64_t ld, int64_t W, const double* add0, const double* add1,
                         const double** d_elems, const double** d_add0, const double** d_add1) {
    const int64_t n_el = (int64_t)h->P * OCTO_N_EL, Wp = W + (W & 1);      // an even leading dimension: every row starts 16-byte aligned
    { int rc = grow(h, h->d_in, h->cap_in, (n_el + 2 * h->C) * Wp); if (rc) return rc; }
    double* p = h->d_in;
    OCHK(h, hipMemcpy2DAsync(p, sizeof(double) * Wp, elems, sizeof(double) * ld, sizeof(double) * W, n_el, hipMemcpyHostToDevice, h->stream));
    *d_elems = p; p += n_el * Wp;
    *d_add0 = nullptr; *d_add1 = nullptr;
    if (add0) { OCHK(h, hipMemcpy2DAsync(p, sizeof(double) * Wp, add0, sizeof(double) * ld, sizeof(double) * W, h->C, hipMemcpyHostToDevice, h->stream)); *d_add0 = p; }
    p += (int64_t)h->C * Wp;
    if (add1) { OCHK(h, hipMemcpy2DAsync(p, sizeof(double) * Wp, add1, sizeof(double) * ld, sizeof(double) * W, h->C, hipMemcpyHostToDevice, h->stream)); *d_add1 = p; }
    return OCTO_OK;
}

int32_t octo_predict_eval(octo_predict* h, const double* elems, int64_t ld, int64_t W, const double* add0, const double* add1, double* out, int64_t ld_out) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_predict_eval", elems, out, ld, W, 0); if (rc) return rc; }
    if (ld_out < W) return fail(h, OCTO_EINVAL, "octo_predict_eval: need W <= ld_out");
    if (W == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const double *d_elems, *d_add0, *d_add1;
    { int rc = upload_inputs(h, elems, ld, W, add0, add1, &d_elems, &d_add0, &d_add1); if (rc) return rc; }
    const int64_t Wp = W + (W & 1), rows = (int64_t)h->C * h->T;
    // walkers per chunk: what the device cube buffer and one row of the staging buffer hold; even, so that every chunk starts 16-byte aligned
    int64_t Wc = std::min(h->cube_bytes / (int64_t)(sizeof(double) * rows), h->stage_bytes / (int64_t)sizeof(double));
    Wc = std::max<int64_t>(std::min(Wc, W), 1);
    if (Wc >= 2) Wc &= ~(int64_t)1;
    const int64_t ldc = Wc + (Wc & 1);
    { int rc = grow(h, h->d_cube, h->cap_cube, rows * ldc); if (rc) return rc; }
    { int rc = ensure_stage(h, h->stage_bytes / (int64_t)sizeof(double)); if (rc) return rc; }
    for (int64_t w0 = 0; w0 < W; w0 += Wc) {
        const int64_t n = std::min(Wc, W - w0);
        { int rc = octo_predict_eval_device(h, d_elems + w0, Wp, n, d_add0 ? d_add0 + w0 : nullptr, d_add1 ? d_add1 + w0 : nullptr, h->d_cube, ldc, OCTO_STREAM_CTX); if (rc) return rc; }
        const int64_t rps = std::max<int64_t>(h->cap_stage / n, 1);      // rows per staging pass
        for (int64_t r0 = 0; r0 < rows; r0 += rps) {
            const int64_t nr = std::min(rps, rows - r0);
            OCHK(h, hipMemcpy2DAsync(h->h_stage, sizeof(double) * n, h->d_cube + r0 * ldc, sizeof(double) * ldc, sizeof(double) * n, nr, hipMemcpyDeviceToHost, h->stream));
            OCHK(h, hipStreamSynchronize(h->stream));
            for (int64_t r = 0; r < nr; ++r) std::memcpy(out + (r0 + r) * ld_out + w0, h->h_stage + r * n, sizeof(double) * n);
        }
    }
    return OCTO_OK;
}

int32_t octo_predict_summary(octo_predict* h, const double* elems, int64_t ld, int64_t W, const double* add0, const double* add1, double* out) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_predict_summary", elems, out, ld, W, 1); if (rc) return rc; }
    OCHK(h, hipSetDevice(h->device));
    const double *d_elems, *d_add0, *d_add1;
    { int rc = upload_inputs(h, elems, ld, W, add0, add1, &d_elems, &d_add0, &d_add1); if (rc) return rc; }
    { int rc = octo_predict_summary_device(h, d_elems, W + (W & 1), W, d_add0, d_add1, h->d_sum, OCTO_STREAM_CTX); if (rc) return rc; }
    OCHK(h, hipMemcpyAsync(out, h->d_sum, sizeof(double) * NSTAT * h->C * h->T, hipMemcpyDeviceToHost, h->stream));
    OCHK(h, hipStreamSynchronize(h->stream));
    return OCTO_OK;
}

}  // extern "C"
