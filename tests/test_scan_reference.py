"""
The restatement of along-scan absolute astrometry (tests/scan_reference.py) held to third parties, the column builders of host/observations.py, and the
build checks of the seventeenth part of liboctofitter_hip_draws.so (csrc/draws/octo_draws_scan.hip). CPU suite: no GPU (hipcc cross-compiles).

  ℓ            against scipy.stats.norm.logpdf of residuals whose reflex comes from a brentq Kepler solve and the textbook Thiele-Innes constants
  gradient     against mp central differences of the restated ℓ, both modes
  marginal     K = 1 against scipy.integrate.quad over β; K = 5 against the closed form by an mp det / lu_solve written separately
  builders     a star with no companion whose y is built from chosen (Δα*, Δδ, ϖ, μ) has zero residual at those β; RES = 0 with the catalogue's β
  build        header, library and binding agree; the new kernels have no scratch; the main library's sources are untouched
"""
import math
import re

import mpmath as mp
import numpy as np
import pytest
from scipy import integrate, optimize, stats

import companion_checks as cc
import draws_build
import scan_cases as sc
import scan_reference as sref

KERNELS = ("k_scan_rows", "k_scan_solve", "k_scan_finish")
FUNCTIONS = dict(octo_draws_scan_set=12, octo_draws_scan_clear=1, octo_draws_scan_eval_device=14, octo_draws_scan_eval=12, octo_draws_scan_values_device=8,
                 octo_draws_scan_bind=4, octo_draws_scan_unbind=1)
SOURCE = cc.CSRC / "draws" / "octo_draws_scan.hip"


@pytest.fixture(autouse=True)
def working_precision():
    """the tests' own mp arithmetic at the restatement's precision, whatever another module left mpmath's global one at"""
    with mp.workdps(sref.DPS):
        yield


def small(K=2, n=6, planets=((sref.VISUAL_KEP, 1), (sref.THIELE_INNES, 1)), W=2, seed=1):
    rng = np.random.default_rng(seed)
    planets = list(planets)
    return dict(tab=sc.draw_table(rng, n, K), planets=planets, elems=sc.draw_elements(rng, planets, W), beta=rng.normal(size=(K, W)), jitter=rng.uniform(0.2, 1.0, W))


def textbook_reflex(el, t, u, v):
    """a Visual{KepOrbit} planet's star reflex along the scan, float64: brentq on Kepler's equation, the true anomaly, the Thiele-Innes constants"""
    a, e, inc, om, Om, tp, M, plx, mass = el
    P_d = 365.2568983840419 * math.sqrt(a ** 3 / M)
    MA = (2 * math.pi * (t - tp) / P_d) % (2 * math.pi)
    E = optimize.brentq(lambda E: E - e * math.sin(E) - MA, -1.0, 8.0, xtol=1e-15, rtol=1e-15)
    nu = 2 * math.atan2(math.sqrt(1 + e) * math.sin(E / 2), math.sqrt(1 - e) * math.cos(E / 2))
    r = a * (1 - e * math.cos(E))      # AU
    x, y = r * math.cos(nu), r * math.sin(nu)
    A = math.cos(Om) * math.cos(om) - math.sin(Om) * math.sin(om) * math.cos(inc)
    B = math.sin(Om) * math.cos(om) + math.cos(Om) * math.sin(om) * math.cos(inc)
    F = -math.cos(Om) * math.sin(om) - math.sin(Om) * math.cos(om) * math.cos(inc)
    G = -math.sin(Om) * math.sin(om) + math.cos(Om) * math.cos(om) * math.cos(inc)
    dec, ra = plx * (A * x + F * y), plx * (B * x + G * y)      # mas: 1 AU at plx mas subtends plx mas
    return -(mass * 0.0009545942339693249 / M) * (u * ra + v * dec)


def test_the_likelihood_against_scipy():
    x = small(K=3, n=9, planets=((sref.VISUAL_KEP, 1), (sref.VISUAL_KEP, 1), (sref.RADVEL, 1), (sref.VISUAL_KEP, 0)), W=3)
    tab = x["tab"]
    r = sref.evaluate(tab, x["planets"], x["elems"], x["beta"], x["jitter"], grad=False)
    for w in range(3):
        eta = np.array([sum(textbook_reflex(x["elems"][p * 9:(p + 1) * 9, w], tab["t"][i], tab["u"][i], tab["v"][i]) for p in (0, 1)) for i in range(9)])
        eta += tab["c"].T @ x["beta"][:, w]
        ll = stats.norm.logpdf(tab["y"] - eta, scale=np.sqrt(tab["sigma"] ** 2 + x["jitter"][w] ** 2)).sum()
        assert abs(ll - r["ll"][w]) <= 1e-11 * max(1.0, abs(ll)), (w, ll, r["ll"][w])
        assert np.all(np.abs(eta - r["eta"][:, w]) <= 1e-10 * np.maximum(1.0, np.abs(eta)))


@pytest.mark.parametrize("mode", [sref.SAMPLED, sref.MARGINAL])
def test_the_gradient_against_mp_differences(mode):
    x = small()
    tab, planets = x["tab"], x["planets"]
    g = sref.evaluate(tab, planets, x["elems"][:, :1], x["beta"][:, :1], x["jitter"][:1], mode=mode, mp_out=True)[0]
    f = lambda el, b, s: sref.evaluate(tab, planets, el, b, s, mode=mode, grad=False, mp_out=True)[0]["ll"]      # noqa: E731
    el, b, s = x["elems"][:, :1], x["beta"][:, :1], x["jitter"][:1]
    h = 2.0 ** -26      # times the input's binade: steps a float64 input takes exactly; the quotient is formed in mp, its error is h²·f‴/6
    def check(fd, an, what):
        assert abs(fd - an) <= 1e-9 * max(1, abs(fd)), (what, fd, an)
    for k in range(el.shape[0]):
        d = h * max(1.0, 2.0 ** math.floor(math.log2(abs(el[k, 0]) + 1e-300)))
        ep, em = el.copy(), el.copy()
        ep[k] += d; em[k] -= d
        check((f(ep, b, s) - f(em, b, s)) / mp.mpf(float(ep[k, 0] - em[k, 0])), g["g_elems"][k], ("elems", k))
    check((f(el, b, s + h) - f(el, b, s - h)) / mp.mpf(2 * h), g["g_jitter"], "jitter")
    if mode == sref.SAMPLED:
        for k in range(b.shape[0]):
            bp, bm = b.copy(), b.copy()
            bp[k] += h; bm[k] -= h
            check((f(el, bp, s) - f(el, bm, s)) / mp.mpf(2 * h), g["g_beta"][k], ("beta", k))


def test_marginal_mode_with_one_column_is_the_integral_over_beta():
    x = small(K=1, n=5, planets=((sref.VISUAL_KEP, 1),), W=1)
    tab, planets = x["tab"], x["planets"]
    m = sref.evaluate(tab, planets, x["elems"], None, x["jitter"], mode=sref.MARGINAL, grad=False)
    bh = m["beta_hat"][0, 0]
    f = lambda b: math.exp(sref.evaluate(tab, planets, x["elems"], np.array([[b]]), x["jitter"], grad=False)["ll"][0] - m["ll"][0])      # noqa: E731
    w = 1.0 / (tab["sigma"] ** 2 + x["jitter"][0] ** 2)
    sd = 1.0 / math.sqrt(float(np.sum(w * tab["c"][0] ** 2)))
    val, err = integrate.quad(f, bh - 12 * sd, bh + 12 * sd, epsabs=0, epsrel=1e-12, limit=200)
    assert abs(val - 1.0) <= 1e-10 + 10 * err, (val, err)      # ∫ exp(ℓ(β)) dβ = exp(ℓ_marg)


def test_marginal_mode_with_five_columns_is_the_closed_form():
    x = small(K=5, n=11, planets=((sref.VISUAL_KEP, 1),), W=1)
    tab, planets = x["tab"], x["planets"]
    m = sref.evaluate(tab, planets, x["elems"], None, x["jitter"], mode=sref.MARGINAL, grad=False, mp_out=True)[0]
    # written separately: ρ = y − reflex from the sampled mode's η at β = 0; ℓ_marg = −½(ρᵀWρ − bᵀA⁻¹b) + ½Σlog w − (n − K)/2·log 2π − ½ log det A
    eta0 = sref.evaluate(tab, planets, x["elems"], np.zeros((5, 1)), x["jitter"], grad=False, mp_out=True)[0]["eta"]
    n = tab["t"].size
    s = mp.mpf(float(x["jitter"][0]))
    w = [1 / (mp.mpf(float(sg)) ** 2 + s ** 2) for sg in tab["sigma"]]
    rho = [mp.mpf(float(tab["y"][i])) - eta0[i] for i in range(n)]
    C = mp.matrix([[mp.mpf(float(tab["c"][k, i])) for k in range(5)] for i in range(n)])
    Wm = mp.diag(w)
    A, b = C.T * Wm * C, C.T * Wm * mp.matrix(rho)
    bh = mp.lu_solve(A, b)
    ll = -(sum(w[i] * rho[i] ** 2 for i in range(n)) - (b.T * bh)[0]) / 2 + sum(mp.log(wi) for wi in w) / 2 - mp.mpf(n - 5) / 2 * mp.log(2 * mp.pi) - mp.log(mp.det(A)) / 2
    assert abs(ll - m["ll"]) <= mp.mpf("1e-35") * max(1, abs(ll))
    assert all(abs(bh[k] - m["beta_hat"][k]) <= mp.mpf("1e-35") * max(1, abs(bh[k])) for k in range(5))


# ---------------------------------------------------------------------------------------------------- the column builders
def iad(rng, n=40):
    yr = np.sort(rng.uniform(1990.0, 1993.0, n))
    psi = rng.uniform(0, 2 * np.pi, n)
    return yr, rng.uniform(-0.7, 0.7, n), np.cos(psi), np.sin(psi), rng.uniform(0.8, 2.5, n)


def test_the_hipparcos_builder_on_a_star_without_a_companion(pkg):
    rng = np.random.default_rng(3)
    yr, parf, cpsi, spsi, sres = iad(rng)
    cat = dict(plx=42.0, pmra=-13.5, pmdec=7.25)
    truth = np.array([0.8, -1.1, 41.2, -12.0, 6.5])      # Δα*, Δδ, ϖ, μα*, μδ
    dt = yr - 1991.25
    # the residuals the catalogue would report for a star that moves by `truth`: its along-scan position minus the catalogue's model of it
    res = cpsi * truth[0] + spsi * truth[1] + parf * (truth[2] - cat["plx"]) + cpsi * dt * (truth[3] - cat["pmra"]) + spsi * dt * (truth[4] - cat["pmdec"])
    obs = pkg.hipparcos_iad_obs(yr, parf, cpsi, spsi, res, sres, **cat)
    assert obs.columns.shape == (5, 40) and np.array_equal(obs.table["u"], cpsi) and np.array_equal(obs.table["v"], spsi) and np.array_equal(obs.table["sigma"], sres)
    assert np.allclose(obs.table["epoch"], (yr - 2000.0) * 365.25 + 51544.5, rtol=0, atol=1e-9)
    assert np.max(np.abs(obs.table["y"] - obs.columns.T @ truth)) <= 1e-11      # zero residual at those β
    # RES = 0 with the catalogue's β and zero offsets
    obs0 = pkg.hipparcos_iad_obs(yr, parf, cpsi, spsi, np.zeros(40), sres, **cat)
    assert np.max(np.abs(obs0.table["y"] - obs0.columns.T @ np.array([0.0, 0.0, cat["plx"], cat["pmra"], cat["pmdec"]]))) <= 1e-12
    # the restated builder has the same columns
    t, u, v, y, cols = sref.hipparcos_columns(yr, parf, cpsi, spsi, res, **cat)
    assert np.array_equal(t, obs.table["epoch"]) and np.array_equal(y, obs.table["y"]) and np.array_equal(cols, obs.columns)
    # … and the restated likelihood of the companion-free star at `truth` is the normal density of zero residuals
    tab = sref.table(t, u, v, y, sres, cols)
    el = np.array([[5.0, 0.1, 1.0, 1.0, 1.0, 48000.0, 1.0, 41.2, 0.0]]).T      # a companion of mass 0
    r = sref.evaluate(tab, [(sref.VISUAL_KEP, 1)], el, truth[:, None], None, grad=False)
    assert abs(r["ll"][0] - stats.norm.logpdf(np.zeros(40), scale=sres).sum()) <= 1e-9


def test_the_gaia_builder_and_the_observation_checks(pkg):
    rng = np.random.default_rng(4)
    n = 30
    t = np.sort(rng.uniform(56900.0, 58900.0, n))
    psi = rng.uniform(0, 2 * np.pi, n)
    obs = pkg.gaia_epoch_obs(t, psi, rng.uniform(-0.7, 0.7, n), rng.normal(size=n), np.full(n, 0.2), 57388.5, mode="marginal", variables=pkg.variables(jitter=0.1))
    assert obs.mode == "marginal" and obs.beta_variables == () and obs.columns.shape == (5, n)
    assert np.allclose(obs.table["u"], np.sin(psi)) and np.allclose(obs.table["v"], np.cos(psi))
    assert np.allclose(obs.columns[3], np.sin(psi) * (t - 57388.5) / 365.25)
    for bad in (dict(mode="sampled", variables=pkg.variables(a=1.0)),      # five columns need five names
                dict(mode="other"), dict(mode="marginal", variables=pkg.variables(b=1.0))):
        with pytest.raises(ValueError):
            pkg.gaia_epoch_obs(t, psi, np.zeros(n), np.zeros(n), np.full(n, 0.2), 57388.5, **bad)
    with pytest.raises(ValueError):
        pkg.AlongScanAstromObs(t, np.sin(psi), np.cos(psi), np.zeros(n), np.zeros(n))      # σ = 0


# ---------------------------------------------------------------------------------------------------- the build
def test_scan_kernels_are_built_without_scratch():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_scan_")} == set(KERNELS), sorted(built)
    assert len(built["k_scan_rows"]) == 6 and len(built["k_scan_solve"]) == 1 and len(built["k_scan_finish"]) == 1
    for family in KERNELS:
        for r in built[family]:
            assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)


def test_scan_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_scan.hip")


def test_scan_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for name, n in FUNCTIONS.items():
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported, name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    assert "draws_scan_accumulate" not in exported      # what the expression program takes from the unit stays inside the library
    for f in ("scan_set", "scan_clear", "scan_eval", "scan_eval_host", "scan_values", "scan_bind", "scan_unbind"):
        assert callable(getattr(draws.PriorDraws, f)), f
    assert callable(pkg.AlongScanAstromObs) and callable(pkg.hipparcos_iad_obs) and callable(pkg.gaia_epoch_obs)


def test_the_constants_agree_in_the_header_the_binding_and_the_restatement():
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for macro, value in (("SCAN_MAX_K", 6), ("SCAN_ROWS", 8), ("SCAN_SAMPLED", 0), ("SCAN_MARGINAL", 1)):
        assert ("#define", f"OCTO_DRAWS_{macro}", str(value)) in lines and getattr(draws, macro) == value, macro
    assert sref.MAX_K == 6 and sc.R == 8 and (sref.SAMPLED, sref.MARGINAL) == (0, 1)
    text = SOURCE.read_text()
    assert "OCTO_DRAWS_SCAN_ROWS" in text and "OCTO_DRAWS_SCAN_MAX_K" in text      # the kernels read the header's constants, not literals of their own
    for routine in ("walker_setup(", "kepler_solve<2, false>(", "planet_finish<", "setup_valid<true>(", "grow_to(", "scan_work", "scan_staging"):
        assert routine in text, routine
    for absent in ("atomicAdd(", "hipDeviceSynchronize", "hipGraph"):
        assert absent not in text, absent
    assert set(re.findall(r"\bvoid (k_\w+)\(", text)) == set(KERNELS)


def test_the_null_handle_is_refused_first(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    einval = pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_scan_set(None, None, 0, None, None, None, None, None, None, None, -1, 0) == einval
    assert lib.octo_draws_scan_clear(None) == einval and lib.octo_draws_scan_unbind(None) == einval
    assert lib.octo_draws_scan_eval_device(None, 5, None, 0, -1, None, None, None, None, None, None, None, 0, None) == einval
    assert lib.octo_draws_scan_eval(None, 5, None, 0, -1, None, None, None, None, None, None, None) == einval
    assert lib.octo_draws_scan_values_device(None, None, 0, -1, None, None, 0, None) == einval
    assert lib.octo_draws_scan_bind(None, 0, None, 0) == einval
