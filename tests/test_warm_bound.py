"""
The a-priori bound of k_main's warm Kepler start (octo_device.h: warm_thr): thr = max((WARM_TOL/ΔM³)^(1/5), min(c(e), 0.06)/ΔM) — the parent's
e-blind form or the predictor's third-order term bounded over the orbit, whichever admits more. tests/warm_bound_model.py restates the bound and the
warm step in float64; the CPU tests hold the restatement, the GPU tests the device routine (the hook octo_debug_kepler_warm) and k_main end to end on
the lanes the new bound newly admits (0.6 < e < 0.9 near periastron).
"""
import numpy as np
import pytest

import synth
import warm_bound_model as wm


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_bound_never_below_the_parent_formula():
    """A row the parent runs warm stays warm: warm_thr >= (WARM_TOL/ΔM³)^(1/5) on a grid e ∈ [0, 1 − 1e-9] x |ΔM| ∈ [1e-7, 0.0314], and for invalid /
    NaN eccentricities it IS the parent's; |x| = ΔM·thr stays within the range the rotation's polynomials are exact for."""
    e = np.concatenate([np.linspace(0.0, 1.0, 401)[:-1], 1 - 10.0 ** np.linspace(-9, -1, 200), [1.0 / 6.0, np.nextafter(1.0 / 6.0, 1), wm.WARM_E_MAX, np.nextafter(wm.WARM_E_MAX, 0)]])
    dM = 10.0 ** np.linspace(-7, np.log10(0.0314), 300)
    eg, dg = np.meshgrid(e, dM, indexing="ij")
    new, old = wm.warm_thr(eg, dg), wm.warm_thr_parent(dg)
    assert np.all(np.isfinite(new)) and np.all(new >= old)
    assert np.all(new * dg <= max(wm.WARM_X_CAP, 0.0631) * (1 + 1e-12))          # tol^(1/5)·0.0314^(2/5) = 0.0629: |dE| < 0.066
    assert (new > old).mean() > 0.3                                               # and it is not the parent's bound under another name
    for bad in (1.0, 1.2, -0.1, np.nan):
        assert np.array_equal(wm.warm_thr(np.full(dM.size, bad), dM), wm.warm_thr_parent(dM))
    # the veto is the parent's: a bound >= WARM_MIN_THR exactly where the parent's is
    d2 = np.linspace(0.028, 0.04, 500)
    for ee in (0.0, 0.3, 0.7, 0.95):
        assert np.array_equal(wm.warm_thr(np.full(d2.size, ee), d2) >= wm.WARM_MIN_THR, wm.warm_thr_parent(d2) >= wm.WARM_MIN_THR)


@pytest.fixture(scope="module")
def one_step_sample():
    rng = np.random.default_rng(20261017)
    e, E, dM = wm.draw_samples(rng, 200_000)
    err, invD, conv = wm.one_step_errors(e, E, dM, np.random.default_rng(3))
    return e, E, dM, err, invD, conv


def test_admitted_rows_are_as_accurate_as_the_parents(one_step_sample):
    """2e5 samples (e, E, ΔM): e uniform and log-dense to 1 − 1e-9, every phase, half within |E| < 0.6 of periastron, |ΔM| 1e-7 … 0.0314 both signs; the
    float64 restatement of the warm step (second-order predictor, rotation to dE⁷ / dE⁸, FOURTH-order correction, one ~2^-23 reciprocal) against an 80-bit
    Newton solve, error of (sin E, cos E) weighted by D. Bar: the worst error the PARENT's bound admits in the same restatement x 1.25, and 2e-15.

    Measured (this sample): parent's worst 3.98e-15, the new bound's worst 3.98e-15 — the same sample —, worst of the rows the new bound admits BEYOND
    the parent's (0.50 % of the sample) 2.4e-16; on the device (octo_debug_kepler_warm, 25 000 such rows) 2.5e-16. The parent's worst rows sit in one
    corner — e > 0.9, |ΔM| > 0.012, 1/D within a few per cent of the bound: the fourth-order correction's truncation, ~0.2 ε⁴ at ε = 3.6e-4 (3.9e-15 at
    e = 0.99996, ΔM = −0.0289, E = 1.02 in 40-digit arithmetic; 4.1e-15 on the device) — and outside it the parent's worst is 9.5e-16. So the parent's own
    bound does not hold 2e-15 there, and a bound that is never below the parent's must keep those rows. The 2e-15 bar is therefore asserted on every
    admitted sample outside that corner and on every sample the new bound admits beyond the parent's (inside the corner too), and the corner's samples
    1.25 x the parent's own worst."""
    e, E, dM, err, invD, conv = one_step_sample
    assert conv.mean() > 0.999
    adm_old = (invD < wm.warm_thr_parent(dM)) & conv
    adm_new = (invD < wm.warm_thr(e, dM)) & conv
    assert np.all(adm_new[adm_old])
    newly = adm_new & ~adm_old
    corner = (e > 0.9) & (np.abs(dM) > 0.012)
    w_old, w_new, w_newly = err[adm_old].max(), err[adm_new].max(), err[newly].max()
    print(f"parent's worst {w_old:.3e}  new bound's worst {w_new:.3e}  newly admitted ({newly.mean():.3%} of the sample) worst {w_newly:.3e}  "
          f"parent outside its corner {err[adm_old & ~corner].max():.3e}  new outside the corner {err[adm_new & ~corner].max():.3e}")
    assert newly.mean() > 0.002
    assert w_new <= 1.25 * w_old, (w_new, w_old)
    assert w_newly < 2e-15 and w_newly <= 1.25 * w_old, w_newly
    assert err[adm_new & ~corner].max() < 2e-15, err[adm_new & ~corner].max()


def test_cold_share_of_config_3_walkers_falls_by_a_third():
    """2 048 walkers as config 3 draws them (a ~ LogU(1, 100) AU, e ~ U(0, 0.95)), 1 500 daily rows, tiles of 64 in drawn order: the share of wave-rows
    with a lane whose previous 1/D fails the bound, new against parent's in the same simulation: at most 0.65 (measured 0.50: 7.04 % -> 3.53 %)."""
    el = synth.draw_walkers(np.random.default_rng(2026), 2048)
    t = 50000.0 + np.arange(1500.0)
    w_old, l_old = wm.cold_wave_row_share(el, t, lambda e, d: wm.warm_thr_parent(d), synth.K_YR)
    w_new, l_new = wm.cold_wave_row_share(el, t, wm.warm_thr, synth.K_YR)
    print(f"cold wave-rows: parent {w_old:.3%} -> {w_new:.3%} (ratio {w_new / w_old:.3f}); lane-rows failing {l_old:.3%} -> {l_new:.3%}")
    assert 0.04 < w_old < 0.12, w_old
    assert w_new <= 0.65 * w_old, (w_new, w_old)


# ------------------------------------------------------------------------------------------------------------------------ GPU
def _hook(pkg, M, dM, e):
    import ctypes as C
    capi = pkg.capi
    lib = capi.load_library()
    lib.octo_debug_kepler_warm.restype = C.c_int32
    lib.octo_debug_kepler_warm.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3
    n = M.size
    sE = np.empty(n); cE = np.empty(n); used = np.empty(n)
    ctx = C.c_void_p()
    assert lib.octo_ctx_create(C.byref(ctx), 0) == 0
    try:
        assert lib.octo_debug_kepler_warm(ctx, capi._dptr(M), capi._dptr(dM), capi._dptr(e), n, capi._dptr(sE), capi._dptr(cE), capi._dptr(used)) == 0
    finally:
        lib.octo_ctx_destroy(ctx)
    return sE, cE, used


@pytest.mark.gpu
def test_device_hook_admits_more_and_stays_accurate(pkg):
    """octo_debug_kepler_warm on 64 x 600 samples (the CPU test's distribution), grouped by the NEW bound so that waves are homogeneous: wherever the wave
    took the warm path the D-weighted error against an 80-bit Newton solve is below 2e-15 — the samples within 2 % of the parent's bound in its corner
    (e > 0.9, |ΔM| > 0.012: see test_admitted_rows_are_as_accurate_as_the_parents) are left to the fail group, as the existing domain test leaves them —
    and the used share exceeds that of the same inputs grouped by the parent's formula and bounded by it (a wave of the hook is warm only if all 64 lanes
    pass, so the parent-bounded share is counted per wave of the parent's grouping from the same 1/D)."""
    rng = np.random.default_rng(99)
    n = 64 * 600
    e, Ep, dM = wm.draw_samples(rng, n)
    el, Epl = e.astype(np.longdouble), Ep.astype(np.longdouble)
    M = np.clip((Epl - el * np.sin(Epl)).astype(np.float64), -np.pi, np.pi)
    v = 1.0 / (1.0 - e * np.cos(Ep))
    thr_old, thr_new = wm.warm_thr_parent(dM), wm.warm_thr(e, dM)
    near_parents_edge = (e > 0.9) & (np.abs(dM) > 0.012) & (v >= 0.98 * thr_old)
    g_new = (v < 0.98 * thr_new) & (thr_old > 2.05) & ~near_parents_edge
    g_old = (v < 0.98 * thr_old) & (thr_old > 2.05)
    assert np.all(g_new[g_old]) and g_new.sum() > g_old.sum() + 64
    order = np.argsort(~g_new, kind="stable")
    Ms, dMs, es = (np.ascontiguousarray(x[order]) for x in (M, dM, e))
    sE, cE, used = _hook(pkg, Ms, dMs, es)
    Mn = Ms.astype(np.longdouble) + dMs.astype(np.longdouble)
    els = es.astype(np.longdouble)
    Et = np.arctan2(sE, cE).astype(np.longdouble)
    Et = Et + np.longdouble(2 * np.pi) * np.rint((Mn - Et) / np.longdouble(2 * np.pi))
    for _ in range(60):
        Et = Et - (Et - els * np.sin(Et) - Mn) / (1 - els * np.cos(Et))
    conv = np.abs(Et - els * np.sin(Et) - Mn) < 1e-17
    cond = (1 - els * np.cos(Et)).astype(np.float64)
    err = np.maximum(np.abs(sE - np.sin(Et).astype(np.float64)), np.abs(cE - np.cos(Et).astype(np.float64))) * cond
    w = (used > 0) & conv
    k = int(np.argmax(np.where(w, err, 0.0)))
    print(f"used share {w.mean():.4f} (whole waves of the new grouping {g_new.sum() // 64 * 64 / n:.4f}; of the parent's {g_old.sum() // 64 * 64 / n:.4f})  "
          f"worst used error {err[k]:.3e} at e = {es[k]:.6f}, dM = {dMs[k]:.3e}")
    assert err[w].max() < 2e-15, (err[k], es[k], dMs[k])
    assert err[(used == 0) & conv].max() < 2e-15
    n_full = g_new.sum() // 64 * 64
    assert np.all(used[:n_full] > 0), "a wave that passes the new bound in the restatement did not start warm on the device: the two bounds disagree"
    # the same inputs grouped and bounded by the parent's formula: its whole waves and at most the one mixed wave start warm
    assert (used > 0).sum() > (g_old.sum() // 64 + 1) * 64, "no more rows start warm than under the parent's bound"


def _radec(rng, n, cadence=1.0):
    t = 50000.0 + cadence * np.arange(n)
    ra, dec = synth.truth_radec(t)
    return [dict(kind=0, planet=0, epoch=t, y1=ra + rng.normal(0, 5, n), y2=dec + rng.normal(0, 5, n), s1=np.full(n, 5.0), s2=np.full(n, 7.0), cor=None)]


def _newly_admitted_walkers(rng, W, n_rows):
    """e ~ U(0.6, 0.9), a ~ LogU(1, 3) AU, a periastron passage inside the table for every walker: the rows the parent's bound rejects and the new one admits"""
    el = synth.draw_walkers(rng, W, 1.0, 3.0)
    el[1] = rng.uniform(0.6, 0.9, W)
    el[5] = 50000.0 + rng.uniform(0.1, 0.9, W) * min(n_rows, 360.0)
    return el


@pytest.fixture(scope="module")
def kmain_case():
    rng = np.random.default_rng(606)
    W = 128
    el = _newly_admitted_walkers(rng, W, 512)
    return dict(el=el, obs={n: _radec(np.random.default_rng(607), n) for n in (512, 2048)}, planets=[dict(orbit_kind=0, has_mass=False)],
                act=synth.active_mask(1, 1, mass=False, nuis=False))


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows,sort", [(512, 0), (2048, 0), (512, 1)], ids=["four_waves", "one_round_eight_waves", "tile_sort_forced"])
def test_kmain_on_the_newly_admitted_lanes(pkg, oracle, kmain_case, n_rows, sort):
    """128 walkers the change newly admits x 512 daily rows (and x 2 048: the one-round launch of eight-wave blocks; and with the tile sort forced on):
    the warm loop against the cold loop (OCTO_OPT_WARM_START = 0) at ll 1e-11 / gradient 1e-9 and against the oracle; the two differ in their last bits."""
    from test_gpu_parity import _cmp_oracle, _gpu
    from test_warm_start import _close, _same_bits
    gb, capi = _gpu(), pkg.capi
    c = kmain_case
    obs, el = c["obs"][n_rows], c["el"]
    warm = gb.gpu_eval(obs, c["planets"], el, None, grad=True, small_batch=0, options={capi.OPT_TILE_SORT: sort, capi.OPT_TILE_MIN_WALKERS: 64})
    cold = gb.gpu_eval(obs, c["planets"], el, None, grad=True, small_batch=0, options={capi.OPT_TILE_SORT: 0, capi.OPT_WARM_START: 0})
    assert not _same_bits(warm, cold), "the warm loop did not run"
    _close("newly admitted lanes", warm, cold, ll_tol=1e-11, g_tol=1e-9)
    ll_o, g_o, _ = oracle.oracle_eval(obs, c["planets"], el, None, grad=True, active=c["act"])
    _cmp_oracle("newly admitted lanes, warm vs oracle", warm[0], warm[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)


@pytest.mark.gpu
def test_kmain_batch_invariant_whole_and_split(pkg, kmain_case):
    """OCTO_OPT_BATCH_INVARIANT on the same walkers: the whole batch and its two halves give the same bits."""
    from test_gpu_parity import _gpu
    gb, capi = _gpu(), pkg.capi
    c = kmain_case
    el = c["el"]
    with gb.GpuPath(c["obs"][512], c["planets"], options={capi.OPT_BATCH_INVARIANT: 1}) as g:
        full = g.eval(el, None, grad=True)
        parts = [g.eval(np.ascontiguousarray(el[:, lo:hi]), None, grad=True) for lo, hi in ((0, 50), (50, 128))]
    assert np.isfinite(full[0]).all()
    assert np.array_equal(full[0], np.concatenate([p[0] for p in parts])) and np.array_equal(full[1], np.concatenate([p[1] for p in parts], axis=1))


@pytest.mark.gpu
def test_two_planets_last_planet_on_the_newly_admitted_lanes(pkg, oracle):
    """warm_last_init's path: config 4 in small (RA/Dec on the outer planet + absolute RV at a 4-day cadence, nuisances), the OUTER planet with
    e ~ U(0.6, 0.9), a ~ LogU(3, 6) AU and a periastron inside the table: warm against cold and the oracle, not the same bits."""
    from test_gpu_parity import _cmp_oracle, _gpu
    from test_warm_start import _close, _same_bits
    gb, capi = _gpu(), pkg.capi
    c4 = synth.config_two_planet(n_astrom=300, n_rv=260, n_walkers=128, seed=78)
    obs = [dict(kind=0, planet=1, epoch=c4["astrom"]["epoch"], y1=c4["astrom"]["ra"], y2=c4["astrom"]["dec"], s1=c4["astrom"]["σ_ra"], s2=c4["astrom"]["σ_dec"], cor=None),
           dict(kind=2, planet=-1, epoch=c4["rv"]["epoch"], y1=c4["rv"]["rv"], y2=None, s1=c4["rv"]["σ_rv"], s2=None, cor=None)]
    planets = [dict(orbit_kind=0, has_mass=True)] * 2
    rng = np.random.default_rng(79)
    el, nuis = c4["elems"].copy(), c4["nuis"]
    W = el.shape[1]
    el[9 + 0] = np.exp(rng.uniform(np.log(3.0), np.log(6.0), W))
    el[9 + 1] = rng.uniform(0.6, 0.9, W)
    el[9 + 5] = 50000.0 + rng.uniform(100.0, 1100.0, W)
    warm = gb.gpu_eval(obs, planets, el, nuis, grad=True, small_batch=0, options={capi.OPT_TILE_SORT: 0})
    cold = gb.gpu_eval(obs, planets, el, nuis, grad=True, small_batch=0, options={capi.OPT_TILE_SORT: 0, capi.OPT_WARM_START: 0})
    assert not _same_bits(warm, cold), "the last-planet warm loop did not run"
    _close("two planets, newly admitted lanes", warm, cold, ll_tol=1e-11, g_tol=1e-9)
    ll_o, g_o, gn_o = oracle.oracle_eval(obs, planets, el, nuis, grad=True)
    _cmp_oracle("two planets, newly admitted lanes vs oracle", warm[0], warm[1], warm[2], ll_o, g_o, gn_o, ll_rtol=1e-10, g_rtol=1e-8)
