// octo_pointwise.hip — liboctofitter_hip_pointwise.so: the per-datum log-likelihood matrix and its WAIC / LOO sums on the device
// (include/octofitter_hip_pointwise.h).
// Of the main library's sources it INCLUDES the device routines the likelihood kernels run — setup_planet_vals / setup_valid (orbit
// constructors and validity, octo_kernels.h), load_pc / set_starter / the cold kepler_solve / atan2_fast / rem_2pi_trunc / rcp_nr / rsqrt_nr
// (octo_device.h), sincos_reduced — so a row is scored from the constants the likelihood was made from. It calls one symbol of the main
// library, octo_consts_default. What it shares with the model-value library (walker_setup, planet_prims, wave_sum, dev_consts) is in
// companion/octo_companion_device.h, the host scaffold of every companion in companion/octo_companion_host.h. The DENSITY is written
// here: astrom_row / rv_row (octo_kernels.h) only accumulate Σ rᵀΣ⁻¹r and Π|Σ| over a table's rows; row_density() below follows their
// rules term by term and closes each row with its own −log 2π − ½ log|Σ|.
//
//   k_pointwise<P, SUM>      lane = walker, block = 256 walkers × one chunk of 32 rows of ONE table. Prologue: the orbit constructors of the
//                            block's walkers (constants in registers), the table's three nuisances and each planet's coefficient in the
//                            table's model. Row loop: the row record is wave-uniform (scalar loads from the constant address space); per
//                            planet the table needs one cold Kepler solve and the primitives (raoff, decoff | V = radvel / K); the model;
//                            row_density(); then
//                              SUM = false  ONE store per lane, contiguous across the wave;
//                              SUM = true   the value into the lane's LDS column; a second loop over the chunk reduces each row at once: wave
//                                           butterflies to (n, max, Σ exp(ll − max), min, Σ exp(min − ll), mean, M2), the block's four waves
//                                           merged in wave order through LDS: one partial per block and row.
//   k_pointwise_n<SUM>       the same for 5 … OCTO_MAX_PLANETS planets: a run-time loop over the planets, block = one wave, the constants in
//                            LDS (one column per lane: no barrier); the solves with the model, the density and the reduction are loops of
//                            their own over the chunk.
//   k_pointwise_merge        one thread per row: the block partials merged in block order, then the seven statistics.
// Every kernel is held to zero SGPR and VGPR spills (tests/test_pointwise_resources.py); DESIGN.md §3d says what that takes.
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
#include "octofitter_hip_pointwise.h"

namespace {
using namespace octo;

constexpr int TPB = 256;               // lanes per block of the templated kernels
constexpr int RPB = 32;                // rows per block: the summary kernels hold a chunk's values in LDS (RPB × 256 doubles = 64 KB); the prologue's ~350 FP64 instructions per planet are < 10 % of the chunk's
constexpr int NSTAT = OCTO_POINTWISE_N_STATS;
constexpr int ROW_N = 8;               // doubles per row record (64 bytes: one line of the scalar cache)
constexpr int FLAG_COR = 1, FLAG_BASIS = 2;

// rows [r0, r1) of one table: what a block's blockIdx.y selects. Wave-uniform: read by scalar loads.
struct RowChunk { int32_t table, kind, planet, flags, mask, r0, r1, pad; };
typedef const int32_t __attribute__((address_space(4))) * cint_t;

struct PwArgs {
    const double* elems; const double* nuis;      // [P*9][ld], [n_obs*3][ld] or null
    const double* rows;                           // [R][ROW_N]: t, y1, y2, s1, s2, cor, basis, 0
    const RowChunk* chunks;
    double* out;                                  // matrix [R][ld_out] | block partials [tiles][R][NSTAT]
    int64_t ld, W, ld_out, R;
    int32_t P, n_chunks;
    int32_t orbit_kind[MAXP];
    int32_t has_mass[MAXP];
    DevConsts c;
};

__device__ __forceinline__ RowChunk load_chunk(const PwArgs& a, int k) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    cint_t p = (cint_t)(a.chunks + k);
#pragma clang diagnostic pop
    RowChunk c;
    c.table = p[0]; c.kind = p[1]; c.planet = p[2]; c.flags = p[3]; c.mask = p[4]; c.r0 = p[5]; c.r1 = p[6]; c.pad = 0;
    return c;
}

// What the row loop reads of its chunk, in ONE scalar register: kind | flags << 4 | mask << 16. row_key() makes it opaque
// once per row, so every wave-uniform test on it (kind, cor, the planet mask) is a compare and a scalar branch INSIDE the loop: left
// loop-invariant, the compiler hoists each test into an SGPR-pair mask of its own, and with the solve's constants they overflow the scalar file.
__device__ __forceinline__ int chunk_key(const RowChunk& c) { return c.kind | (c.flags << 4) | (c.mask << 16); }
__device__ __forceinline__ int row_key(int key) { asm volatile("" : "+s"(key)); return key; }
__device__ __forceinline__ int key_kind(int k) { return k & 15; }
__device__ __forceinline__ int key_flags(int k) { return (k >> 4) & 15; }
__device__ __forceinline__ int key_mask(int k) { return (k >> 16) & 255; }
// The same for a lane's two flags (bit 0: the walker exists, bit 1: every planet's setup_valid passed): kept as ONE vector register and
// tested inside the loop, not as two lane masks in scalar register pairs across it.
__device__ __forceinline__ int lane_flags(int f) { asm volatile("" : "+v"(f)); return f; }
// What the reduction loop needs after the solve loop (the partial buffer and its row count, the walker tile, the chunk's first row) is
// wave-uniform; it is carried across the solve loop in vector registers, where there is room, instead of scalar ones.
template <class T>
__device__ __forceinline__ T in_vgpr(T x) { asm volatile("" : "+v"(x)); return x; }
struct PartDest { double* part; int64_t R; int tile, r0; };

// One walker's system: the planets' constants and, per row, their primitives. REGISTERS for the templated planet counts (every loop over
// the planets unrolls, every index is a constant); LDS columns for the run-time count.
template <int P>
struct RegSys {
    PC pc[P];
    double ra_[P], de_[P], V_[P];
    double cf_[P];               // the table's coefficient of each planet (table_planet_coef), fixed for the block
    __device__ __forceinline__ static constexpr int n() { return P; }
    __device__ __forceinline__ double a(int p) const { return pc[p].a; }
    __device__ __forceinline__ double mu(int p) const { return pc[p].mu; }
    __device__ __forceinline__ double K(int p) const { return pc[p].K; }
    __device__ __forceinline__ double ra(int p) const { return ra_[p]; }
    __device__ __forceinline__ double de(int p) const { return de_[p]; }
    __device__ __forceinline__ double V(int p) const { return V_[p]; }
};

struct LdsSys {
    const double* wc;            // [P][NWC][WAVE] the block's constants (this lane's column: + lane)
    int np;
    __device__ __forceinline__ int n() const { return np; }
    __device__ __forceinline__ double a(int p) const { return wc[(p * NWC + WC_A) * WAVE]; }
    __device__ __forceinline__ double mu(int p) const { return wc[(p * NWC + WC_MU) * WAVE]; }
    __device__ __forceinline__ double K(int p) const { return wc[(p * NWC + WC_K) * WAVE]; }
};

__host__ __device__ __forceinline__ bool is_astrom_kind(int kind) { return kind == OCTO_ASTROM_RADEC || kind == OCTO_ASTROM_SEPPA; }

// a table's nuisances for one walker, read once per block
struct TabCoef {
    double n0, n1, n2;      // astrometry: jitter, platescale, northangle | RV: offset, jitter, trend coefficient (0 without a basis column)
    double j2, sn, cn;      // jitter², sin / cos of the northangle
};

__device__ __forceinline__ TabCoef table_coef(const PwArgs& a, const RowChunk& ch, int64_t wl) {
    TabCoef c;
    const bool astrom = is_astrom_kind(ch.kind);
    c.n0 = 0.0; c.n1 = astrom ? 1.0 : 0.0; c.n2 = 0.0; c.sn = 0.0; c.cn = 1.0;
    if (a.nuis) {
        const double* nu = a.nuis + (int64_t)ch.table * OCTO_N_NUIS * a.ld + wl;
        c.n0 = nu[0]; c.n1 = nu[a.ld]; c.n2 = nu[2 * a.ld];
        if (astrom) sincos_reduced(c.n2, c.sn, c.cn);
        else if (!(ch.flags & FLAG_BASIS)) c.n2 = 0.0;
    }
    const double jit = astrom ? c.n0 : c.n1;
    c.j2 = jit * jit;
    return c;
}

// The coefficient of planet p in the model of a table attached to planet pl, fixed per (walker, table) and so formed ONCE per block:
//   astrometry   f_p = 1 for the table's planet, m/M for the strictly inner ones, else 0                 (astrom_coef_vals)
//   RV           g_p·K_p with g_p = −m/M for every planet (OCTO_RV_ABS), or 1 for the table's planet and −m/M for the strictly inner
//                ones (OCTO_RV_REL)                                                                      (rv_coef_vals: gK)
template <class S>
__device__ __forceinline__ double table_planet_coef(const S& s, int kind, int pl, int p) {
    const int n = s.n();
    double a_this = 0.0;
#pragma unroll
    for (int q = 0; q < n; ++q) a_this = (q == pl) ? s.a(q) : a_this;
    const bool inner = s.a(p) < a_this;
    if (is_astrom_kind(kind)) return (p == pl) ? 1.0 : (inner ? s.mu(p) : 0.0);
    const double g = kind == OCTO_RV_REL ? ((p == pl) ? 1.0 : (inner ? -s.mu(p) : 0.0)) : -s.mu(p);
    return g * s.K(p);
}

// The MODEL of a row, the first half of astrom_row / rv_row:
//   astrometry  (x, y) = Σ_p f_p·(raoff_p, decoff_p) in planet order, from (0, 0)
//   RV          fma(trend, basis, offset), then one fma(g_p·K_p, V_p, ·) per planet in planet order
// model_init / model_add are the only place it is formed: the register kernels call them over their unrolled planets, the run-time-planet
// kernels inside their planet loop.
__device__ __forceinline__ void model_init(const TabCoef& co, int kind, crow_t row, double& m0, double& m1) {
    m0 = is_astrom_kind(kind) ? 0.0 : fma(co.n2, row[6], co.n0);
    m1 = 0.0;
}
__device__ __forceinline__ void model_add(int kind, double cf, double ra, double de, double V, double& m0, double& m1) {
    if (is_astrom_kind(kind)) { m0 = fma(cf, ra, m0); m1 = fma(cf, de, m1); }
    else m0 = fma(cf, V, m0);
}

// THE log-density of one row for one walker from its model (m0, m1) = (x, y) | (rv, ·): every entry point's numbers come from this routine.
// The second half of astrom_row / rv_row:
//   astrometry  platescale and northangle act on the DATA; the sep/PA residual carries Julia's truncated remainder; σ and jitter in
//               quadrature; with a correlation column Σ = [v1, cor·σ1σ2; ·, v2];   ll = −log 2π − ½ log|Σ| − ½ rᵀΣ⁻¹r
//   RV          ll = −½ log 2π − ½ log(σ² + jitter²) − ½ resid²/(σ² + jitter²)
// kind and flags are wave-uniform: every branch on them is a scalar branch, and a field of the row record is loaded on the arm that reads it.
__device__ __forceinline__ double row_density(const TabCoef& co, int kind, int flags, crow_t row, double m0, double m1) {
    const double y1 = row[1], s1 = row[3];
    if (!is_astrom_kind(kind)) {
        const double resid = y1 - m0;
        const double var = fma(s1, s1, co.j2);
        const double iv = rcp_nr<2>(var);
        return fma(-0.5, resid * resid * iv, fma(-0.5, log(var), -0.5 * LOG2PI));
    }
    const double y2 = row[2], s2 = row[4];
    const double x = m0, y = m1;
    const double ps = co.n1, na = co.n2;
    double r1, r2;
    if (kind == OCTO_ASTROM_SEPPA) {
        const double rho2 = fma(x, x, y * y);
        const double irho = rsqrt_nr(rho2);
        const double pa = atan2_fast(x, y);
        double dpa = (y1 + na) - pa + PI;
        dpa = rem_2pi_trunc(dpa) - PI;                 // Julia `%`: truncated remainder
        dpa = dpa < -PI ? dpa + TWO_PI : dpa;
        r1 = dpa;
        r2 = fma(-rho2, irho, y2 * ps);
    } else {
        const double u1 = fma(y1, co.cn, y2 * co.sn);
        const double u2 = fma(y2, co.cn, -(y1 * co.sn));
        r1 = fma(ps, u1, -x);
        r2 = fma(ps, u2, -y);
    }
    const double v1 = fma(s1, s1, co.j2), v2 = fma(s2, s2, co.j2);
    const double v12 = v1 * v2;
    const double iv12 = rcp_nr<2>(v12);
    const double iv1 = iv12 * v2, iv2 = iv12 * v1;
    double a1, a2, det;
    if (flags & FLAG_COR) {
        const double cor = row[5];
        const double omc = 1.0 - cor * cor;
        const double ic = rcp_nr<2>(omc);
        const double is = rsqrt_nr(v12);               // 1/(σ1 σ2)
        a1 = fma(r1, iv1, -(cor * r2 * is)) * ic;
        a2 = fma(r2, iv2, -(cor * r1 * is)) * ic;
        det = v12 * omc;
    } else {
        a1 = r1 * iv1; a2 = r2 * iv2;
        det = v12;
    }
    const double q = fma(r1, a1, r2 * a2);
    return fma(-0.5, q, fma(-0.5, log(det), -LOG2PI));
}

// ---- the reduction over the walkers ------------------------------------------------------------------------------------------------------
struct PStat { double n, mx, s1, mn, s2, mean, m2; };      // s1 = Σ exp(ll − mx), s2 = Σ exp(mn − ll)

// log-sum-exp pairs rescaled to the common extreme — the side that holds it keeps its sum, the other is scaled by ONE exp(−|difference|) —
// and Chan, Golub & LeVeque's pairwise update for mean / M2. Branch-free: an empty side (n = 0, max = −Inf, min = +Inf, sums, mean, M2 = 0)
// leaves the other untouched bit for bit (its sum is scaled by exp(−Inf) = 0, its weight in the mean is 0); two empty sides stay empty.
__device__ __forceinline__ void stat_merge(PStat& s, const PStat& b) {
    const double nt = s.n + b.n;
    const bool any = nt > 0.0;
    const double e1 = exp(-fabs(s.mx - b.mx)), e2 = exp(-fabs(s.mn - b.mn));      // NaN only where both sides are empty: dropped below
    const double s1 = s.mx >= b.mx ? fma(b.s1, e1, s.s1) : fma(s.s1, e1, b.s1);
    const double s2 = s.mn <= b.mn ? fma(b.s2, e2, s.s2) : fma(s.s2, e2, b.s2);
    s.s1 = any ? s1 : 0.0; s.s2 = any ? s2 : 0.0;
    s.mx = fmax(s.mx, b.mx); s.mn = fmin(s.mn, b.mn);
    const double wb = any ? b.n / nt : 0.0, d = b.mean - s.mean;
    s.mean = fma(d, wb, s.mean);
    s.m2 = s.m2 + b.m2 + d * d * (s.n * wb);
    s.n = nt;
}

// the wave's 64 values: every lane ends with the same seven numbers
__device__ __forceinline__ PStat wave_stat(double x, bool valid) {
    PStat s;
    s.n = (double)__popcll(__ballot(valid));
    double mn = valid ? x : INFINITY, mx = valid ? x : -INFINITY;
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) { mn = fmin(mn, __shfl_xor(mn, m, WAVE)); mx = fmax(mx, __shfl_xor(mx, m, WAVE)); }
    s.mn = mn; s.mx = mx;
    s.s1 = wave_sum(valid ? exp(x - mx) : 0.0);
    s.s2 = wave_sum(valid ? exp(mn - x) : 0.0);
    const double mean = wave_sum(valid ? x : 0.0) / s.n;
    s.mean = s.n > 0.0 ? mean : 0.0;                             // an empty wave: the empty statistics stat_merge counts on
    const double d = valid ? x - s.mean : 0.0;
    s.m2 = wave_sum(d * d);
    return s;
}

__device__ __forceinline__ PStat stat_empty() { return PStat{0.0, -INFINITY, 0.0, INFINITY, 0.0, 0.0, 0.0}; }

// block partial of (tile, row r): seven adjacent doubles, out[(tile·R + r)·NSTAT + k] — one address per row
__device__ __forceinline__ void part_store(const PartDest& d, int k, const PStat& s) {
    double* o = d.part + ((int64_t)d.tile * d.R + d.r0 + k) * NSTAT;
    o[0] = s.n; o[1] = s.mx; o[2] = s.s1; o[3] = s.mn; o[4] = s.s2; o[5] = s.mean; o[6] = s.m2;
}

// ---- 1 … 4 planets: constants in registers -----------------------------------------------------------------------------------------------
// The single-planet matrix kernel is held to 128 registers (four waves per SIMD); its summary twin carries the reduction's exp() calls on top
// and takes two; with more planets the constants decide.
template <int P, bool SUM>
__global__ __launch_bounds__(TPB, (P == 1 ? (SUM ? 2 : 4) : 1)) void k_pointwise(PwArgs a) {
    constexpr int NWV = TPB / WAVE;
    __shared__ double sh[SUM ? 2 : 1][NWV][NSTAT];      // two buffers: one barrier per row
    __shared__ double vals[SUM ? RPB * TPB : 1];        // the chunk's values, one column per lane (SUM)
    const int chunk = blockIdx.y + blockIdx.z * gridDim.y;
    if (chunk >= a.n_chunks) return;                    // block-uniform, ahead of every barrier
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool live = w < a.W;
    const int64_t wl = live ? w : a.W - 1;              // a dead lane repeats the last walker: every load stays inside the arrays
    RegSys<P> sys;
    bool ok = true;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        double v[NWC];
        ok = walker_setup(a, p, wl, v) && ok;
        load_pc(sys.pc[p], v, 1, 0, 0);
    }
    const RowChunk ch = load_chunk(a, chunk);      // behind the orbit constructors: nothing of the chunk is parked across them
    const TabCoef co = table_coef(a, ch, wl);
#pragma unroll
    for (int p = 0; p < P; ++p) sys.cf_[p] = table_planet_coef(sys, ch.kind, ch.planet, p);
    const int key0 = chunk_key(ch);
    const int flags0 = (live ? 1 : 0) | (ok ? 2 : 0);
    const crow_t rows = constant_rows(a.rows);
    const int n_rows = ch.r1 - ch.r0;
    const PartDest dest{in_vgpr(a.out), in_vgpr(a.R), in_vgpr((int)blockIdx.x), in_vgpr(ch.r0)};
    for (int k = 0; k < n_rows; ++k) {
        const int r = ch.r0 + k;
        const int key = row_key(key0);
        const int need = is_astrom_kind(key_kind(key)) ? NEED_AST : NEED_RV;
        const crow_t row = rows + (int64_t)r * ROW_N;
        const double t = row[0];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if ((key_mask(key) >> p) & 1) planet_prims(sys.pc[p], t, need, sys.ra_[p], sys.de_[p], sys.V_[p]);
            else { sys.ra_[p] = 0.0; sys.de_[p] = 0.0; sys.V_[p] = 0.0; }
        }
        double m0, m1;
        model_init(co, key_kind(key), row, m0, m1);
#pragma unroll
        for (int p = 0; p < P; ++p) model_add(key_kind(key), sys.cf_[p], sys.ra_[p], sys.de_[p], sys.V_[p], m0, m1);
        double v = row_density(co, key_kind(key), key_flags(key), row, m0, m1);
        const int lf = lane_flags(flags0);
        v = (lf & 2) ? v : -INFINITY;
        if constexpr (!SUM) {
            if (lf & 1) a.out[(int64_t)r * a.ld_out + w] = v;
        } else {
            vals[k * TPB + threadIdx.x] = (lf & 1) ? v : NAN;      // a lane without a walker: not finite, so not counted
        }
    }
    // The reduction is a loop of its own over the chunk's values (each lane reads back its own column: no barrier in between). Fused into
    // the row loop, the reduction's scalar state and the solve's coefficients, which the compiler keeps in scalar registers across a loop
    // that uses them, do not fit the scalar file together.
    if constexpr (SUM) {
        const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
        for (int k = 0; k < n_rows; ++k) {
            const int buf = k & 1;
            const double v = vals[k * TPB + threadIdx.x];
            const PStat s = wave_stat(v, isfinite(v));
            if (lane == 0) { double* o = sh[buf][wv]; o[0] = s.n; o[1] = s.mx; o[2] = s.s1; o[3] = s.mn; o[4] = s.s2; o[5] = s.mean; o[6] = s.m2; }
            __syncthreads();
            if (threadIdx.x == 0) {
                PStat b = stat_empty();
#pragma unroll
                for (int k = 0; k < NWV; ++k) { const double* o = sh[buf][k]; stat_merge(b, PStat{o[0], o[1], o[2], o[3], o[4], o[5], o[6]}); }
                part_store(dest, k, b);
            }
        }
    }
}

// ---- 5 … OCTO_MAX_PLANETS planets: block = one wave, constants in LDS ----------------------------------------------------------------------
// Three loops over the chunk's rows, each lane reading back only its own LDS column (no barrier): the solves and the model; the density;
// (SUM) the reduction. In one loop the solve's and the arctangent's coefficients, the run-time planet loop and the reduction do not fit the
// scalar file together.
struct LdsBlock {
    double wc[MAXP * NWC * WAVE];
    double cf[MAXP * WAVE];
    double m[2 * RPB * WAVE];      // per row the model (m0, m1); the density then overwrites m0 with the value
};

template <bool SUM>
__global__ __launch_bounds__(WAVE) void k_pointwise_n(PwArgs a) {
    __shared__ LdsBlock L;
    const int chunk = blockIdx.y + blockIdx.z * gridDim.y;
    if (chunk >= a.n_chunks) return;
    const int lane = threadIdx.x;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    const bool live = w < a.W;
    const int64_t wl = live ? w : a.W - 1;
    bool ok = true;
    for (int p = 0; p < a.P; ++p) {
        double v[NWC];
        ok = walker_setup(a, p, wl, v) && ok;
#pragma unroll
        for (int k = 0; k < NWC; ++k) L.wc[(p * NWC + k) * WAVE + lane] = v[k];
    }
    const RowChunk ch = load_chunk(a, chunk);
    const LdsSys sys{L.wc + lane, a.P};
    const TabCoef co = table_coef(a, ch, wl);
    for (int p = 0; p < a.P; ++p) L.cf[p * WAVE + lane] = table_planet_coef(sys, ch.kind, ch.planet, p);
    const int key0 = chunk_key(ch);
    const int flags0 = (live ? 1 : 0) | (ok ? 2 : 0);
    const crow_t rows = constant_rows(a.rows);
    const int n_rows = ch.r1 - ch.r0;
    const PartDest dest{in_vgpr(a.out), in_vgpr(a.R), in_vgpr((int)blockIdx.x), in_vgpr(ch.r0)};
    for (int k = 0; k < n_rows; ++k) {
        const int key = row_key(key0);
        const int need = is_astrom_kind(key_kind(key)) ? NEED_AST : NEED_RV;
        const crow_t row = rows + (int64_t)(ch.r0 + k) * ROW_N;
        const double t = row[0];
        double m0, m1;
        model_init(co, key_kind(key), row, m0, m1);
        for (int p = 0; p < a.P; ++p) {
            double ra = 0.0, de = 0.0, V = 0.0;
            if ((key_mask(key) >> p) & 1) {
                PC pc;
                load_pc(pc, L.wc, WAVE, p, lane);
                planet_prims(pc, t, need, ra, de, V);
            }
            model_add(key_kind(key), L.cf[p * WAVE + lane], ra, de, V, m0, m1);
        }
        L.m[(2 * k) * WAVE + lane] = m0;
        L.m[(2 * k + 1) * WAVE + lane] = m1;
    }
    for (int k = 0; k < n_rows; ++k) {
        const int key = row_key(key0);
        const int r = ch.r0 + k;
        const crow_t row = rows + (int64_t)r * ROW_N;
        double v = row_density(co, key_kind(key), key_flags(key), row, L.m[(2 * k) * WAVE + lane], L.m[(2 * k + 1) * WAVE + lane]);
        const int lf = lane_flags(flags0);
        v = (lf & 2) ? v : -INFINITY;
        if constexpr (!SUM) {
            if (lf & 1) a.out[(int64_t)r * a.ld_out + w] = v;
        } else {
            L.m[(2 * k) * WAVE + lane] = (lf & 1) ? v : NAN;      // a lane without a walker: not finite, so not counted
        }
    }
    if constexpr (SUM) {
        for (int k = 0; k < n_rows; ++k) {
            const double v = L.m[(2 * k) * WAVE + lane];
            const PStat s = wave_stat(v, isfinite(v));
            if (lane == 0) part_store(dest, k, s);
        }
    }
}

// out [NSTAT][R] from part [tiles][R][NSTAT]
__global__ __launch_bounds__(TPB) void k_pointwise_merge(const double* __restrict__ part, int64_t tiles, int64_t R, double* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= R) return;
    PStat s = stat_empty();
    for (int64_t b = 0; b < tiles; ++b) {
        const double* o = part + (b * R + r) * NSTAT;
        stat_merge(s, PStat{o[0], o[1], o[2], o[3], o[4], o[5], o[6]});
    }
    const bool none = s.n == 0.0;
    out[OCTO_POINTWISE_N * R + r] = s.n;
    out[OCTO_POINTWISE_LPPD * R + r] = none ? NAN : s.mx + log(s.s1 / s.n);
    out[OCTO_POINTWISE_MEAN * R + r] = none ? NAN : s.mean;
    out[OCTO_POINTWISE_VAR * R + r] = none ? NAN : s.m2 / (s.n - 1.0);      // n = 1: 0/0 = NaN
    out[OCTO_POINTWISE_ELPD_IS_LOO * R + r] = none ? NAN : s.mn - log(s.s2 / s.n);
    out[OCTO_POINTWISE_MIN * R + r] = none ? NAN : s.mn;
    out[OCTO_POINTWISE_MAX * R + r] = none ? NAN : s.mx;
}

}  // namespace

struct octo_pointwise : CompanionStaged {
    int P = 0, n_obs = 0;
    int64_t R = 0;
    int32_t n_chunks = 0;
    PwArgs base;                            // everything of a launch that the handle fixes
    std::vector<int32_t> row_table;
    double* d_rows = nullptr;
    RowChunk* d_chunks = nullptr;
    // summary: block partials (grown on demand)
    double* d_part = nullptr; int64_t cap_part = 0;
    // host-buffer calls: inputs, matrix chunk, summary result (grown on demand)
    double* d_in = nullptr; int64_t cap_in = 0;
    double* d_mat = nullptr; int64_t cap_mat = 0;
    double* d_sum = nullptr;
    int64_t mat_bytes = (int64_t)64 << 20;
};

namespace {

int check_batch(octo_pointwise* h, const char* who, const void* elems, const void* out, int64_t ld, int64_t W, int64_t w_min) {
    if (W < w_min || ld < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need " + std::to_string(w_min) + " <= W <= ld");
    if (W > 0 && h->R > 0 && (!elems || !out)) return fail(h, OCTO_EINVAL, std::string(who) + ": null elements or output");
    return OCTO_OK;
}

const char* kind_name(int kind) {
    switch (kind) {
    case OCTO_RV_ABS_MARG: return "OCTO_RV_ABS_MARG";
    case OCTO_HGCA: return "OCTO_HGCA";
    case OCTO_ONEIL_RADEC: return "OCTO_ONEIL_RADEC";
    case OCTO_ONEIL_SEPPA: return "OCTO_ONEIL_SEPPA";
    default: return "?";
    }
}

template <bool SUM>
void launch_rows(const octo_pointwise* h, const PwArgs& a, hipStream_t st) {
    // chunks over grid.y, and over grid.z beyond its 65 535 (the kernels return for an index past the last chunk)
    const unsigned gy = (unsigned)std::min<int32_t>(h->n_chunks, 65535), gz = (unsigned)((h->n_chunks + 65534) / 65535);
    if (h->P > MAXP_T) {
        hipLaunchKernelGGL(k_pointwise_n<SUM>, dim3((unsigned)((a.W + WAVE - 1) / WAVE), gy, gz), dim3(WAVE), 0, st, a);
        return;
    }
    const dim3 grid((unsigned)((a.W + TPB - 1) / TPB), gy, gz);
    switch (h->P) {
    case 1: hipLaunchKernelGGL((k_pointwise<1, SUM>), grid, dim3(TPB), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_pointwise<2, SUM>), grid, dim3(TPB), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_pointwise<3, SUM>), grid, dim3(TPB), 0, st, a); break;
    default: hipLaunchKernelGGL((k_pointwise<4, SUM>), grid, dim3(TPB), 0, st, a); break;
    }
}

int64_t summary_tiles(const octo_pointwise* h, int64_t W) { return h->P <= MAXP_T ? (W + TPB - 1) / TPB : (W + WAVE - 1) / WAVE; }

}  // namespace

extern "C" {

static int32_t pointwise_create(int32_t device_id, const octo_consts* consts, const octo_obs_desc* obs, int32_t n_obs,
                                const octo_planet_desc* planets, int32_t n_planets, octo_pointwise** out);

// No exception crosses the boundary: the row records of up to 2^31 − 1 rows are host vectors, and their allocation may fail.
int32_t octo_pointwise_create(int32_t device_id, const octo_consts* consts, const octo_obs_desc* obs, int32_t n_obs,
                              const octo_planet_desc* planets, int32_t n_planets, octo_pointwise** out) {
    try {
        return pointwise_create(device_id, consts, obs, n_obs, planets, n_planets, out);
    } catch (const std::bad_alloc&) {      // thrown while the host vectors are built, ahead of the handle: nothing to release
        g_create_error.clear();
        return OCTO_ENOMEM;
    } catch (...) {
        g_create_error.clear();
        return OCTO_EINVAL;
    }
}

static int32_t pointwise_create(int32_t device_id, const octo_consts* consts, const octo_obs_desc* obs, int32_t n_obs,
                                const octo_planet_desc* planets, int32_t n_planets, octo_pointwise** out) {
    const std::string fn = "octo_pointwise_create: ";
    if (!out) return fail(nullptr, OCTO_EINVAL, fn + "null out pointer");
    *out = nullptr;
    if (!planets || n_obs < 0 || (n_obs > 0 && !obs)) return fail(nullptr, OCTO_EINVAL, fn + "null argument");
    if (n_planets < 1 || n_planets > OCTO_MAX_PLANETS) return fail(nullptr, OCTO_EINVAL, fn + "1 <= n_planets <= OCTO_MAX_PLANETS");
    if (n_obs > OCTO_POINTWISE_MAX_TABLES) return fail(nullptr, OCTO_EINVAL, fn + "n_obs <= OCTO_POINTWISE_MAX_TABLES");
    for (int p = 0; p < n_planets; ++p) {
        const int k = planets[p].orbit_kind;
        if (k != OCTO_ORBIT_VISUAL_KEP && k != OCTO_ORBIT_RADVEL && k != OCTO_ORBIT_THIELE_INNES && k != OCTO_ORBIT_KEP)
            return fail(nullptr, OCTO_EINVAL, fn + "unknown orbit kind");
    }
    int64_t R = 0;
    for (int o = 0; o < n_obs; ++o) {
        const octo_obs_desc& d = obs[o];
        const std::string who = fn + "table " + std::to_string(o);
        if (d.kind < 0 || d.kind >= OCTO_N_KINDS) return fail(nullptr, OCTO_EINVAL, who + ": unknown observation kind");
        if (d.kind == OCTO_RV_ABS_MARG || d.kind == OCTO_HGCA || d.kind == OCTO_ONEIL_RADEC || d.kind == OCTO_ONEIL_SEPPA)
            return fail(nullptr, OCTO_ENOTSUP, who + ": " + kind_name(d.kind) + " is not a sum over the table's rows: no pointwise log-likelihood");
        if (d.n_epochs < 0 || d.n_epochs > 0x7fffffff) return fail(nullptr, OCTO_EINVAL, who + ": bad n_epochs");
        const bool astrom = is_astrom_kind(d.kind);
        const bool planet_obs = astrom || d.kind == OCTO_RV_REL;
        if (planet_obs && (d.planet < 0 || d.planet >= n_planets)) return fail(nullptr, OCTO_EINVAL, who + ": planet index outside the system");
        if (d.n_epochs > 0 && (!d.epoch || !d.y1 || !d.s1 || (astrom && (!d.y2 || !d.s2)))) return fail(nullptr, OCTO_EINVAL, who + ": missing column");
        if (astrom && (planets[d.planet].orbit_kind == OCTO_ORBIT_RADVEL || planets[d.planet].orbit_kind == OCTO_ORBIT_KEP))
            return fail(nullptr, OCTO_EINVAL, who + ": astrometry needs a planet with a parallax (Visual{KepOrbit} or ThieleInnesOrbit)");
        if (!astrom)
            for (int p = 0; p < n_planets; ++p)
                if (planets[p].orbit_kind == OCTO_ORBIT_THIELE_INNES && (!planet_obs || p == d.planet || planets[p].has_mass))
                    return fail(nullptr, OCTO_ENOTSUP, who + ": RV tables with a ThieleInnesOrbit planet are not supported");
        if (!planet_obs)
            for (int p = 0; p < n_planets; ++p)
                if (!planets[p].has_mass) return fail(nullptr, OCTO_EINVAL, who + ": absolute RV needs a mass on every planet");
        const bool has_basis = !astrom && d.extra != nullptr && d.n_extra > 0;
        if (has_basis && d.n_extra != d.n_epochs) return fail(nullptr, OCTO_EINVAL, who + ": an RV table's trend basis column (extra) needs n_extra == n_epochs");
        if (astrom && d.extra != nullptr && d.n_extra > 0) return fail(nullptr, OCTO_EINVAL, who + ": astrometry tables take no `extra`");
        for (int64_t r = 0; r < d.n_epochs; ++r) {
            if (!std::isfinite(d.epoch[r]) || !std::isfinite(d.y1[r]) || !(d.s1[r] > 0.0) || !std::isfinite(d.s1[r]) ||
                (astrom && (!std::isfinite(d.y2[r]) || !(d.s2[r] > 0.0) || !std::isfinite(d.s2[r]))) || (has_basis && !std::isfinite(d.extra[r])))
                return fail(nullptr, OCTO_EINVAL, who + " row " + std::to_string(r) + ": epochs and measurements must be finite and uncertainties finite and > 0");
            if (astrom && d.cor && !(std::fabs(d.cor[r]) <= 1.0 - 1e-5))      // relative-astrometry.jl:70-72
                return fail(nullptr, OCTO_EINVAL, who + " row " + std::to_string(r) + ": correlation values may not be well-specified");
        }
        R += d.n_epochs;
        if (R > 0x7fffffff) return fail(nullptr, OCTO_EINVAL, fn + "more than 2^31 - 1 rows");
    }
    octo_consts cst;
    if (consts) cst = *consts;
    else if (octo_consts_default(&cst) != OCTO_OK) return fail(nullptr, OCTO_EINVAL, fn + "octo_consts_default failed");

    // the row records and the chunks of rows the blocks take
    std::vector<double> rows((size_t)std::max<int64_t>(R, 1) * ROW_N, 0.0);
    std::vector<RowChunk> chunks;
    std::vector<int32_t> row_table((size_t)R);
    const int32_t rpb = RPB;
    int64_t r_at = 0;
    for (int o = 0; o < n_obs; ++o) {
        const octo_obs_desc& d = obs[o];
        const bool astrom = is_astrom_kind(d.kind);
        const bool has_basis = !astrom && d.extra != nullptr && d.n_extra > 0;
        int32_t mask = 0;      // the planets whose solution a row of this table can read: its own, and every planet with a mass
        for (int p = 0; p < n_planets; ++p)
            if (planets[p].has_mass || ((astrom || d.kind == OCTO_RV_REL) && p == d.planet)) mask |= 1 << p;
        for (int64_t r = 0; r < d.n_epochs; ++r) {
            double* a = &rows[(size_t)(r_at + r) * ROW_N];
            a[0] = d.epoch[r]; a[1] = d.y1[r]; a[3] = d.s1[r];
            if (astrom) { a[2] = d.y2[r]; a[4] = d.s2[r]; a[5] = d.cor ? d.cor[r] : 0.0; }
            if (has_basis) a[6] = d.extra[r];
            row_table[(size_t)(r_at + r)] = o;
        }
        for (int64_t r0 = 0; r0 < d.n_epochs; r0 += rpb) {
            RowChunk c;
            c.table = o; c.kind = d.kind; c.planet = (astrom || d.kind == OCTO_RV_REL) ? d.planet : -1;
            c.flags = ((astrom && d.cor) ? FLAG_COR : 0) | (has_basis ? FLAG_BASIS : 0);
            c.mask = mask; c.r0 = (int32_t)(r_at + r0); c.r1 = (int32_t)(r_at + std::min<int64_t>(r0 + rpb, d.n_epochs)); c.pad = 0;
            chunks.push_back(c);
        }
        r_at += d.n_epochs;
    }

    octo_pointwise* h;
    { int rc = open_device(device_id, fn, h); if (rc) return rc; }
    h->P = n_planets; h->n_obs = n_obs; h->R = R; h->n_chunks = (int32_t)chunks.size();
    h->row_table = std::move(row_table);
    h->mat_bytes = env_bytes("OCTO_POINTWISE_MATRIX_BYTES", h->mat_bytes);
    h->stage_bytes = env_bytes("OCTO_POINTWISE_STAGE_BYTES", h->stage_bytes);
    auto bail = [&](int code, const std::string& msg) { octo_pointwise_destroy(h); return fail(nullptr, code, msg); };
    const size_t n_ch = std::max<size_t>(chunks.size(), 1);
    if (hipMalloc((void**)&h->d_rows, sizeof(double) * rows.size()) != hipSuccess || hipMalloc((void**)&h->d_chunks, sizeof(RowChunk) * n_ch) != hipSuccess ||
        hipMalloc((void**)&h->d_sum, sizeof(double) * NSTAT * (size_t)std::max<int64_t>(R, 1)) != hipSuccess)
        return bail(OCTO_ENOMEM, fn + "hipMalloc failed");
    if (hipMemcpy(h->d_rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice) != hipSuccess ||
        (!chunks.empty() && hipMemcpy(h->d_chunks, chunks.data(), sizeof(RowChunk) * chunks.size(), hipMemcpyHostToDevice) != hipSuccess))
        return bail(OCTO_EHIP, fn + "upload failed");
    PwArgs& a = h->base;
    std::memset(&a, 0, sizeof(a));
    a.rows = h->d_rows; a.chunks = h->d_chunks; a.R = R; a.P = n_planets; a.n_chunks = h->n_chunks;
    for (int p = 0; p < n_planets; ++p) { a.orbit_kind[p] = planets[p].orbit_kind; a.has_mass[p] = planets[p].has_mass ? 1 : 0; }
    a.c = dev_consts(cst);
    *out = h;
    return OCTO_OK;
}

int32_t octo_pointwise_destroy(octo_pointwise* h) {
    if (!h) return OCTO_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    (void)hipFree(h->d_rows); (void)hipFree(h->d_chunks); (void)hipFree(h->d_part); (void)hipFree(h->d_in); (void)hipFree(h->d_mat); (void)hipFree(h->d_sum);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    delete h;
    return OCTO_OK;
}

const char* octo_pointwise_last_error(const octo_pointwise* h) { return last_error(h); }

int32_t octo_pointwise_sync(octo_pointwise* h) { return sync_handle(h); }

int64_t octo_pointwise_n_rows(const octo_pointwise* h) { return h ? h->R : -1; }

int32_t octo_pointwise_row_table(const octo_pointwise* h, int32_t* out) {
    if (!h) return OCTO_EINVAL;
    if (h->R > 0 && !out) return OCTO_EINVAL;
    if (h->R > 0) std::memcpy(out, h->row_table.data(), sizeof(int32_t) * (size_t)h->R);
    return OCTO_OK;
}

int32_t octo_pointwise_eval_device(octo_pointwise* h, const double* d_elems, int64_t ld, int64_t W, const double* d_nuis,
                                   double* d_out, int64_t ld_out, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_pointwise_eval_device", d_elems, d_out, ld, W, 0); if (rc) return rc; }
    if (ld_out < W) return fail(h, OCTO_EINVAL, "octo_pointwise_eval_device: need W <= ld_out");
    if (W == 0 || h->R == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    PwArgs a = h->base;
    a.elems = d_elems; a.nuis = d_nuis; a.ld = ld; a.W = W; a.out = d_out; a.ld_out = ld_out;
    launch_rows<false>(h, a, st);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_pointwise_summary_device(octo_pointwise* h, const double* d_elems, int64_t ld, int64_t W, const double* d_nuis,
                                      double* d_out, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_pointwise_summary_device", d_elems, d_out, ld, W, 1); if (rc) return rc; }
    if (h->R == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t tiles = summary_tiles(h, W);
    { int rc = grow(h, h->d_part, h->cap_part, tiles * NSTAT * h->R); if (rc) return rc; }
    PwArgs a = h->base;
    a.elems = d_elems; a.nuis = d_nuis; a.ld = ld; a.W = W; a.out = h->d_part; a.ld_out = 0;
    launch_rows<true>(h, a, st);
    hipLaunchKernelGGL(k_pointwise_merge, dim3((unsigned)((h->R + TPB - 1) / TPB)), dim3(TPB), 0, st, (const double*)h->d_part, tiles, h->R, d_out);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

// elems [P*9][ld] and nuis [n_obs*3][ld] -> d_in, packed with leading dimension W: elements, then nuisances
static int upload_inputs(octo_pointwise* h, const double* elems, int64_t ld, int64_t W, const double* nuis, const double** d_elems, const double** d_nuis) {
    const int64_t n_el = (int64_t)h->P * OCTO_N_EL, n_nu = (int64_t)h->n_obs * OCTO_N_NUIS;
    { int rc = grow(h, h->d_in, h->cap_in, (n_el + n_nu) * W); if (rc) return rc; }
    double* p = h->d_in;
    OCHK(h, hipMemcpy2DAsync(p, sizeof(double) * W, elems, sizeof(double) * ld, sizeof(double) * W, n_el, hipMemcpyHostToDevice, h->stream));
    *d_elems = p; p += n_el * W;
    *d_nuis = nullptr;
    if (nuis && n_nu > 0) { OCHK(h, hipMemcpy2DAsync(p, sizeof(double) * W, nuis, sizeof(double) * ld, sizeof(double) * W, n_nu, hipMemcpyHostToDevice, h->stream)); *d_nuis = p; }
    return OCTO_OK;
}

int32_t octo_pointwise_eval(octo_pointwise* h, const double* elems, int64_t ld, int64_t W, const double* nuis, double* out, int64_t ld_out) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_pointwise_eval", elems, out, ld, W, 0); if (rc) return rc; }
    if (ld_out < W) return fail(h, OCTO_EINVAL, "octo_pointwise_eval: need W <= ld_out");
    if (W == 0 || h->R == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const double *d_elems, *d_nuis;
    { int rc = upload_inputs(h, elems, ld, W, nuis, &d_elems, &d_nuis); if (rc) return rc; }
    const int64_t rows = h->R;
    // walkers per chunk: what the device matrix buffer and one row of the staging buffer hold
    int64_t Wc = std::min(h->mat_bytes / (int64_t)(sizeof(double) * rows), h->stage_bytes / (int64_t)sizeof(double));
    Wc = std::max<int64_t>(std::min(Wc, W), 1);
    { int rc = grow(h, h->d_mat, h->cap_mat, rows * Wc); if (rc) return rc; }
    { int rc = ensure_stage(h, std::max<int64_t>(h->stage_bytes / (int64_t)sizeof(double), 1)); if (rc) return rc; }
    for (int64_t w0 = 0; w0 < W; w0 += Wc) {
        const int64_t n = std::min(Wc, W - w0);
        { int rc = octo_pointwise_eval_device(h, d_elems + w0, W, n, d_nuis ? d_nuis + w0 : nullptr, h->d_mat, Wc, OCTO_STREAM_CTX); if (rc) return rc; }
        const int64_t rps = std::max<int64_t>(h->cap_stage / n, 1);      // rows per staging pass
        for (int64_t r0 = 0; r0 < rows; r0 += rps) {
            const int64_t nr = std::min(rps, rows - r0);
            OCHK(h, hipMemcpy2DAsync(h->h_stage, sizeof(double) * n, h->d_mat + r0 * Wc, sizeof(double) * Wc, sizeof(double) * n, nr, hipMemcpyDeviceToHost, h->stream));
            OCHK(h, hipStreamSynchronize(h->stream));
            for (int64_t r = 0; r < nr; ++r) std::memcpy(out + (r0 + r) * ld_out + w0, h->h_stage + r * n, sizeof(double) * n);
        }
    }
    return OCTO_OK;
}

int32_t octo_pointwise_summary(octo_pointwise* h, const double* elems, int64_t ld, int64_t W, const double* nuis, double* out) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_batch(h, "octo_pointwise_summary", elems, out, ld, W, 1); if (rc) return rc; }
    if (h->R == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const double *d_elems, *d_nuis;
    { int rc = upload_inputs(h, elems, ld, W, nuis, &d_elems, &d_nuis); if (rc) return rc; }
    { int rc = octo_pointwise_summary_device(h, d_elems, W, W, d_nuis, h->d_sum, OCTO_STREAM_CTX); if (rc) return rc; }
    OCHK(h, hipMemcpyAsync(out, h->d_sum, sizeof(double) * NSTAT * h->R, hipMemcpyDeviceToHost, h->stream));
    OCHK(h, hipStreamSynchronize(h->stream));
    return OCTO_OK;
}

}  // extern "C"
