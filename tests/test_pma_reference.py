"""
The restatement of the catalogue proper-motion anomaly (tests/pma_reference.py) held to third parties, the builder of host/observations.py, and the
build checks of the eighteenth part of liboctofitter_hip_draws.so (csrc/draws/octo_draws_pma.hip). CPU suite: no GPU (hipcc cross-compiles).

  ℓ            against scipy.stats.multivariate_normal.logpdf, the reflex from a brentq Kepler solve and the textbook Thiele-Innes constants
  gradient     against mp central differences of the restated ℓ, both modes
  marginal     K = 1 against scipy.integrate.quad over γ; K = 2 against the closed form by an mp det / lu_solve written separately; γ̂ is the sampled
               mode's stationary point in γ
  builder      a star with no companion that moves linearly in a frame common to both missions: L applied to its scans gives (μα*, μδ) three times
  build        header, library and binding agree; the new kernels have no scratch; the main library's sources are untouched
"""
import math
import re

import mpmath as mp
import numpy as np
import pytest
from scipy import integrate, stats

import companion_checks as cc
import draws_build
import pma_cases as pc
import pma_reference as pref
import scan_cases as sc
import scan_reference as sref
from test_scan_reference import textbook_reflex

KERNELS = ("k_pma_rows", "k_pma_close", "k_pma_adj", "k_pma_finish")
FUNCTIONS = dict(octo_draws_pma_set=14, octo_draws_pma_clear=1, octo_draws_pma_eval_device=12, octo_draws_pma_eval=10, octo_draws_pma_values_device=8,
                 octo_draws_pma_bind=4, octo_draws_pma_unbind=1)
SOURCE = cc.CSRC / "draws" / "octo_draws_pma.hip"


@pytest.fixture(autouse=True)
def working_precision():
    """the tests' own mp arithmetic at the restatement's precision, whatever another module left mpmath's global one at"""
    with mp.workdps(sref.DPS):
        yield


def small(Q=3, K=2, n=6, planets=((sref.VISUAL_KEP, 1), (sref.THIELE_INNES, 1)), W=2, seed=1):
    rng = np.random.default_rng(seed)
    planets = list(planets)
    return dict(tab=pc.draw_table(rng, n, Q, K), planets=planets, elems=sc.draw_elements(rng, planets, W), gamma=rng.normal(size=(K, W)))


def test_the_likelihood_against_scipy():
    x = small(Q=4, K=2, n=9, planets=((sref.VISUAL_KEP, 1), (sref.VISUAL_KEP, 1), (sref.RADVEL, 1), (sref.VISUAL_KEP, 0)), W=3)
    tab = x["tab"]
    r = pref.evaluate(tab, x["planets"], x["elems"], x["gamma"], grad=False)
    for w in range(3):
        rho = np.array([sum(textbook_reflex(x["elems"][p * 9:(p + 1) * 9, w], tab["t"][i], tab["u"][i], tab["v"][i]) for p in (0, 1)) for i in range(9)])
        m = tab["L"] @ rho + tab["H"] @ x["gamma"][:, w]
        ll = stats.multivariate_normal.logpdf(tab["d"], mean=m, cov=tab["cov"])
        assert abs(ll - r["ll"][w]) <= 1e-10 * max(1.0, abs(ll)), (w, ll, r["ll"][w])
        assert np.all(np.abs(m - r["m"][:, w]) <= 1e-10 * np.maximum(1.0, np.abs(m)))
        assert np.all(np.abs(tab["L"] @ rho - r["z"][:, w]) <= 1e-10 * np.maximum(1.0, np.abs(r["z"][:, w])))


@pytest.mark.parametrize("mode", [pref.SAMPLED, pref.MARGINAL])
def test_the_gradient_against_mp_differences(mode):
    x = small()
    tab, planets = x["tab"], x["planets"]
    el, gm = x["elems"][:, :1], x["gamma"][:, :1]
    g = pref.evaluate(tab, planets, el, gm, mode=mode, mp_out=True)[0]
    f = lambda e_, g_: pref.evaluate(tab, planets, e_, g_, mode=mode, grad=False, mp_out=True)[0]["ll"]      # noqa: E731
    h = 2.0 ** -26      # times the input's binade: steps a float64 input takes exactly; the quotient is formed in mp, its error is h²·f‴/6
    def check(fd, an, what):
        assert abs(fd - an) <= 1e-9 * max(1, abs(fd)), (what, fd, an)
    for k in range(el.shape[0]):
        d = h * max(1.0, 2.0 ** math.floor(math.log2(abs(el[k, 0]) + 1e-300)))
        ep, em = el.copy(), el.copy()
        ep[k] += d; em[k] -= d
        check((f(ep, gm) - f(em, gm)) / mp.mpf(float(ep[k, 0] - em[k, 0])), g["g_elems"][k], ("elems", k))
    if mode == pref.SAMPLED:
        for k in range(gm.shape[0]):
            gp, gn = gm.copy(), gm.copy()
            gp[k] += h; gn[k] -= h
            check((f(el, gp) - f(el, gn)) / mp.mpf(2 * h), g["g_gamma"][k], ("gamma", k))


def test_marginal_mode_with_one_parameter_is_the_integral_over_gamma():
    x = small(Q=3, K=1, n=5, planets=((sref.VISUAL_KEP, 1),), W=1)
    tab, planets = x["tab"], x["planets"]
    m = pref.evaluate(tab, planets, x["elems"], None, mode=pref.MARGINAL, grad=False)
    gh = m["gamma_hat"][0, 0]
    f = lambda g: math.exp(pref.evaluate(tab, planets, x["elems"], np.array([[g]]), grad=False)["ll"][0] - m["ll"][0])      # noqa: E731
    H = tab["H"][:, 0]
    sd = 1.0 / math.sqrt(float(H @ np.linalg.solve(tab["cov"], H)))
    val, err = integrate.quad(f, gh - 12 * sd, gh + 12 * sd, epsabs=0, epsrel=1e-12, limit=200)
    assert abs(val - 1.0) <= 1e-10 + 10 * err, (val, err)      # ∫ exp(ℓ(γ)) dγ = exp(ℓ_marg)


def test_marginal_mode_with_two_parameters_is_the_closed_form_and_gamma_hat_is_stationary():
    x = small(Q=6, K=2, n=11, planets=((sref.VISUAL_KEP, 1),), W=1)
    tab, planets = x["tab"], x["planets"]
    m = pref.evaluate(tab, planets, x["elems"], None, mode=pref.MARGINAL, grad=False, mp_out=True)[0]
    # written separately: ℓ_marg = ℓ(γ̂) + (K/2)·log 2π − ½·log det N with γ̂ from the normal equations N γ̂ = HᵀΣ⁻¹(d − z) by lu_solve on Σ and N
    z = pref.evaluate(tab, planets, x["elems"], np.zeros((2, 1)), grad=False, mp_out=True)[0]["z"]
    S = mp.matrix([[mp.mpf(float(v)) for v in row] for row in tab["cov"]])
    H = mp.matrix([[mp.mpf(float(v)) for v in row] for row in tab["H"]])
    rho = mp.matrix([mp.mpf(float(tab["d"][q])) - z[q] for q in range(6)])
    SiH = mp.matrix(6, 2)
    for k in range(2):
        col = mp.lu_solve(S, H[:, k])
        for q in range(6):
            SiH[q, k] = col[q]
    N = H.T * SiH
    gh = mp.lu_solve(N, SiH.T * rho)
    res = rho - H * gh
    ll = -(res.T * mp.lu_solve(S, res))[0] / 2 - (6 * mp.log(2 * mp.pi) + mp.log(mp.det(S))) / 2 + mp.log(2 * mp.pi) - mp.log(mp.det(N)) / 2
    assert abs(ll - m["ll"]) <= mp.mpf("1e-35") * max(1, abs(ll))
    assert all(abs(gh[k] - m["gamma_hat"][k]) <= mp.mpf("1e-35") * max(1, abs(gh[k])) for k in range(2))
    # γ̂ is the stationary point of the sampled mode in γ: ∂ℓ/∂γ at γ̂, formed in mp, vanishes on the scale of its terms |H[q][k]·λ_q|
    gam = np.array([[float(gh[0])], [float(gh[1])]])
    s = pref.evaluate(tab, planets, x["elems"], gam, mp_out=True)[0]
    assert all(abs(s["g_gamma"][k]) <= 1e-13 * max(1.0, float(np.max(np.abs(tab["H"])))) * 6 for k in range(2)), s["g_gamma"]


# ---------------------------------------------------------------------------------------------------- the builder
def scans(rng, nh=40, ng=30):
    yr = np.sort(rng.uniform(1990.0, 1993.0, nh))
    psi_h = rng.uniform(0, 2 * np.pi, nh)
    hip = (yr, np.cos(psi_h), np.sin(psi_h), rng.uniform(0.8, 2.5, nh), rng.uniform(-0.7, 0.7, nh))
    gaia = (np.sort(rng.uniform(56900.0, 57900.0, ng)), rng.uniform(0, 2 * np.pi, ng), rng.uniform(-0.7, 0.7, ng))
    return hip, gaia


HGCA_ROW = dict(epoch_ra_hip=1991.31, epoch_dec_hip=1991.18, epoch_ra_gaia=2016.02, epoch_dec_gaia=2016.11,
                pmra_hip=4.7, pmdec_hip=-6.8, pmra_hip_error=0.6, pmdec_hip_error=0.5, pmra_pmdec_hip=0.2,
                pmra_hg=5.05, pmdec_hg=-7.02, pmra_hg_error=0.02, pmdec_hg_error=0.018, pmra_pmdec_hg=0.1,
                pmra_gaia=5.3, pmdec_gaia=-7.4, pmra_gaia_error=0.05, pmdec_gaia_error=0.04, pmra_pmdec_gaia=-0.15)


def test_the_builder_on_a_star_without_a_companion(pkg):
    rng = np.random.default_rng(8)
    hip, gaia = scans(rng)
    obs = pkg.hgca_obs(HGCA_ROW, hip, gaia, factor=2.0, variables=pkg.variables(pmra=pkg.Normal(0, 10), pmdec=pkg.Normal(0, 10)))
    assert pkg.HGCAObs is pkg.hgca_obs and isinstance(obs, pkg.CatalogueFitObs)
    assert obs.L.shape == (6, 70) and obs.H.shape == (6, 2) and obs.gamma_variables == ("pmra", "pmdec") and obs.mode == "sampled"
    t, u, v = obs.t, obs.u, obs.v
    assert np.array_equal(t[:40], (hip[0] - 2000.0) * 365.25 + 51544.5) and np.array_equal(u[:40], hip[1]) and np.array_equal(v[:40], hip[2])
    assert np.array_equal(u[40:], np.sin(gaia[1])) and np.array_equal(v[40:], np.cos(gaia[1]))
    # a star whose along-scan signal is u·(Δα + μα·(t − T0)) + v·(Δδ + μδ·(t − T0)) + pf·ϖ in a frame COMMON to both missions
    pf = np.concatenate([hip[4], gaia[2]])
    T0, dra, ddec, plx, mua, mud = 51544.5, 3.0, -2.0, 41.0, 5.0, -7.0
    dt = (t - T0) / 365.25
    y = u * (dra + mua * dt) + v * (ddec + mud * dt) + pf * plx
    out = obs.L @ y
    assert np.max(np.abs(out - np.array([mua, mud] * 3))) <= 1e-9, out
    assert not np.any(obs.L[0:2, 40:]) and not np.any(obs.L[4:6, :40]) and np.all(np.any(obs.L[2:4, :40] != 0, axis=1)) and np.all(np.any(obs.L[2:4, 40:] != 0, axis=1))
    # d, Σ and H from the row
    assert np.array_equal(obs.d, [4.7, -6.8, 5.05, -7.02, 5.3, -7.4]) and np.array_equal(obs.H, np.tile(np.eye(2), (3, 1)))
    assert np.allclose(np.diag(obs.cov), (2.0 * np.array([0.6, 0.5, 0.02, 0.018, 0.05, 0.04])) ** 2, rtol=1e-15)
    assert np.isclose(obs.cov[0, 1], 0.2 * 1.2 * 1.0) and np.isclose(obs.cov[4, 5], -0.15 * 0.1 * 0.08) and not np.any(obs.cov[:2, 2:]) and not np.any(obs.cov[2:4, 4:])
    # the restated refit operator (normal equations) gives the same μ rows as the host's (pseudo-inverse)
    FH, _ = pref.refit_operator(t[:40], u[:40], v[:40], hip[4], hip[3])
    FG, _ = pref.refit_operator(t[40:], u[40:], v[40:], gaia[2])
    assert np.allclose(obs.L[0, :40], FH[3], rtol=0, atol=1e-10) and np.allclose(obs.L[5, 40:], FG[4], rtol=0, atol=1e-10)
    # with the barycentre's proper motion in γ and no companion mass the restated likelihood is the catalogue's own density at (μα*, μδ)
    tab = pref.table(t, u, v, obs.L, obs.d, obs.cov, obs.H)
    el = np.array([[5.0, 0.1, 1.0, 1.0, 1.0, 48000.0, 1.0, 41.2, 0.0]]).T      # a companion of mass 0
    r = pref.evaluate(tab, [(sref.VISUAL_KEP, 1)], el, np.array([[mua], [mud]]), grad=False)
    assert abs(r["ll"][0] - stats.multivariate_normal.logpdf(obs.d, mean=[mua, mud] * 3, cov=obs.cov)) <= 1e-9


def test_the_observation_checks(pkg):
    rng = np.random.default_rng(9)
    hip, gaia = scans(rng, 12, 11)
    marg = pkg.hgca_obs(HGCA_ROW, hip, gaia + (np.full(11, 0.3),), mode="marginal")
    assert marg.mode == "marginal" and marg.gamma_variables == ()
    x = pkg.hgca_obs(HGCA_ROW, hip, gaia)
    args = (x.t, x.u, x.v, x.L, x.d, x.cov, x.H)
    for bad in (dict(mode="other"), dict(mode="marginal", variables=pkg.variables(a=1.0)), dict(variables=pkg.variables(a=1.0))):      # two columns need two names
        with pytest.raises(ValueError):
            pkg.CatalogueFitObs(*args, **bad)
    with pytest.raises(ValueError):
        pkg.CatalogueFitObs(*args[:5], -x.cov, x.H)              # not positive definite
    with pytest.raises(ValueError):
        pkg.CatalogueFitObs(*args[:6], None, mode="marginal")   # the marginal mode needs a design
    with pytest.raises(ValueError):
        pkg.CatalogueFitObs(*args[:6], np.ones((6, 5)))          # K > 4
    with pytest.raises(ValueError):
        pkg.hgca_obs(HGCA_ROW, tuple(c[:4] for c in hip), gaia)  # four scans do not determine five parameters


def test_a_system_with_both_tables_is_refused(pkg):
    rng = np.random.default_rng(10)
    hip, gaia = scans(rng, 12, 11)
    V = pkg.variables
    cat = pkg.hgca_obs(HGCA_ROW, hip, gaia, variables=V(pmra=pkg.Normal(0, 10), pmdec=pkg.Normal(0, 10)))
    scan = pkg.AlongScanAstromObs(cat.t, cat.u, cat.v, np.zeros(23), np.ones(23), variables=V(jitter=0.1))
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[],
                   variables=V(a=pkg.LogUniform(2, 10), e=0.1, i=0.9, ω=1.1, Ω=2.3, tp=48000.0, mass=pkg.LogUniform(5.0, 60.0)))
    system = pkg.System(name="both", companions=[b], observations=[cat, scan], variables=V(M=1.1, plx=50.0))
    with pytest.raises(ValueError, match="CatalogueFitObs and an AlongScanAstromObs"):
        pkg.LogDensityModel(system)


# ---------------------------------------------------------------------------------------------------- the build
def test_pma_kernels_are_built_without_scratch():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_pma_")} == set(KERNELS), sorted(built)
    for family in KERNELS:
        assert len(built[family]) == 1, family
        for r in built[family]:
            assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
            assert r["vgpr_count"] + r["agpr_count"] <= 128, (family, r)      # four waves per SIMD at the least, the bar of the samplers' kernels


def test_pma_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_pma.hip")


def test_pma_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for name, n in FUNCTIONS.items():
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported, name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    assert "draws_pma_accumulate" not in exported      # what the expression program takes from the unit stays inside the library
    for f in ("pma_set", "pma_clear", "pma_eval", "pma_eval_host", "pma_values", "pma_bind", "pma_unbind"):
        assert callable(getattr(draws.PriorDraws, f)), f
    assert callable(pkg.CatalogueFitObs) and callable(pkg.hgca_obs) and callable(pkg.HGCAObs)


def test_the_constants_agree_in_the_header_the_binding_and_the_restatement():
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for macro, value in (("PMA_MAX_Q", 8), ("PMA_MAX_K", 4), ("PMA_SAMPLED", 0), ("PMA_MARGINAL", 1)):
        assert ("#define", f"OCTO_DRAWS_{macro}", str(value)) in lines and getattr(draws, macro) == value, macro
    assert (pref.MAX_Q, pref.MAX_K) == (8, 4) and pc.R == draws.SCAN_ROWS == 8 and (pref.SAMPLED, pref.MARGINAL) == (0, 1)
    text = SOURCE.read_text()
    assert "OCTO_DRAWS_SCAN_ROWS" in text and "OCTO_DRAWS_PMA_MAX_Q" in text and "OCTO_DRAWS_PMA_MAX_K" in text      # the header's constants, not literals
    for routine in ("walker_setup(", "kepler_solve<2, false>(", "planet_finish<", "setup_valid<true>(", "grow_to(", "pma_work", "pma_staging", "pma_table_build("):
        assert routine in text, routine
    for absent in ("atomicAdd(", "hipDeviceSynchronize", "hipGraph"):
        assert absent not in text, absent
    assert set(re.findall(r"\bvoid (k_\w+)\(", text)) == set(KERNELS)


def test_the_null_handle_is_refused_first(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    einval = pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_pma_set(None, None, 0, None, None, None, None, None, 0, None, None, None, -1, 0) == einval
    assert lib.octo_draws_pma_clear(None) == einval and lib.octo_draws_pma_unbind(None) == einval
    assert lib.octo_draws_pma_eval_device(None, 5, None, 0, -1, None, None, None, None, None, 0, None) == einval
    assert lib.octo_draws_pma_eval(None, 5, None, 0, -1, None, None, None, None, None) == einval
    assert lib.octo_draws_pma_values_device(None, None, 0, -1, None, None, 0, None) == einval
    assert lib.octo_draws_pma_bind(None, 0, None, 0) == einval
