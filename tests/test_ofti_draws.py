"""
The OFTI rejection sampler on the device (include/octofitter_hip_draws.h, "The sixteenth"; host/draws.py: PriorDraws.ofti_*; host/callers.py:
octofit_ofti_device) against its NumPy restatement (tests/ofti_draws_reference.py) on the cases of tests/ofti_draws_cases.py, whose conditions
tests/test_ofti_draws_reference.py asserts on the CPU: the accepted set EXACTLY, the values at the bars below, invalid lanes and batch shapes
bit for bit, and the meaning of the elements through the main library's own orbit code.

Bars: ℓ at 1e-9·max(1, |ℓ|), test_ofti.py's bar for the device against the restated ofti_linear_solve; the Thiele-Innes rows at 1e-8·‖μ‖ per draw, that
test's bar for the means (cond(S) <= 1e6 by the cases' condition, so a relative error of 1e-15 in S stays below 1e-9 in S⁻¹b and L⁻ᵀz); the elements at
1e-8 relative — they are smooth functions of the draw away from face-on, which the cases exclude. ω and Ω are compared on the circle at 1e-8·|angle|, with
an absolute floor of 1e-10 rad for an angle that happens to lie next to 0: an angle is an atan2 of the draw plus a fold by π or 2π, so its error is ABSOLUTE — the
draw's relative error (whose own bar, 1e-8, would allow 1e-8 rad) and a few ulp of 2π — and does not shrink with the angle; the floor is a hundredth of what
the draw's bar allows and bites only below 0.01 rad.
"""
import math

import numpy as np
import pytest

import hmc_reference as ref
import ofti_draws_cases as oc
import ofti_draws_reference as oref
from draws_device import TRANS_BAR, draws_mod, mirror_priors, rel      # noqa: F401

pytestmark = pytest.mark.gpu

LL_BAR, TI_BAR, EL_BAR = 1e-9, 1e-8, 1e-8
ANGLE_FLOOR = 1e-10      # rad
CASE_IDS = [f"{c[0]}-seed{c[1]}-mode{c[2]}" for c in oc.CASES]


def handle(pkg, draws_mod, name, tp_mode, priors=None):
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, priors or oc.priors_of(tp_mode)))
    pd.ofti_set(*oc.columns(oc.table(name)), tp_mode=tp_mode, t_ref=oc.T_REF)
    return pd


@pytest.fixture(scope="module")
def device_runs(pkg, draws_mod):
    """case -> the device's rejection on it, made once"""
    runs = {}

    def run(case):
        if case not in runs:
            with handle(pkg, draws_mod, case[0], case[2]) as pd:
                runs[case] = pd.ofti_rejection(case[1], oc.N, first=oc.FIRST)
        return runs[case]
    return run


def restated(case):
    r = oc.restated(*case)
    oc.check_conditions(r)
    return r


# ---------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("tp_mode", (0, 1))
def test_nl_is_the_restatements(pkg, draws_mod, tp_mode):
    n, first, seed = 1000, oc.FIRST, 44
    with handle(pkg, draws_mod, "ofti_example", tp_mode) as pd:
        theta, _, _ = pd.sample(seed, first, n, theta_t=False, logprior_t=False)
        nl = pd.ofti_nl(theta).cpu().numpy()
        th = theta.cpu().numpy()
    want_th, _ = ref.prior_sample(oc.priors_of(tp_mode), seed, np.uint64(first) + np.arange(n, dtype=np.uint64))
    want = oref.nl_of(want_th, tp_mode, oc.T_REF, oc.k_yr())
    err = rel(nl, want).max()
    print(f"mode {tp_mode}: nl within {err:.2e} (bar {TRANS_BAR:g})")
    assert err <= TRANS_BAR
    assert np.array_equal(nl[[0, 1, 3, 4]], th[[0, 1, 3, 4]])
    if tp_mode == 0:
        assert np.array_equal(nl[2], th[2])
    else:      # the expression of the likelihood kernel from the device's own θ: a handful of roundings of 1.1e-16 each apart
        assert rel(nl[2], oc.T_REF + th[2] * oc.k_yr() * np.sqrt(th[1] * th[1] * th[1] / th[3])).max() <= 1e-14


# ---------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("case", oc.CASES, ids=CASE_IDS)
def test_the_accepted_set_is_the_restatements(device_runs, case):
    want, got = restated(case), device_runs(case)
    print(f"{case}: accepted {got['n_accepted']} (restated {want['n_accepted']}), max ℓ {got['max_logml']!r} (restated {want['max_logml']!r})")
    assert got["n_accepted"] == want["n_accepted"]
    assert got["index"].dtype == np.uint64 and np.array_equal(got["index"], want["index"])


@pytest.mark.parametrize("case", [oc.CASES[0], oc.CASES[3]], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_a_cap_below_and_above_the_count(pkg, draws_mod, device_runs, case):
    want, full = restated(case), device_runs(case)
    with handle(pkg, draws_mod, case[0], case[2]) as pd:
        for cap in (100, want["n_accepted"] + 50, 0):
            r = pd.ofti_rejection(case[1], oc.N, cap=cap, first=oc.FIRST)
            ns = min(cap, want["n_accepted"])
            assert r["n_accepted"] == want["n_accepted"] and r["max_logml"] == full["max_logml"]
            assert np.array_equal(r["index"], want["index"][:ns])
            for k in ("theta", "nl", "post"):
                assert r[k].shape[1] == ns and np.array_equal(r[k], full[k][:, :ns])


# ---------------------------------------------------------------------------------------------------- c
def circle(a, b):
    d = np.abs(a - b) % (2 * math.pi)
    return np.minimum(d, 2 * math.pi - d)


def angle_excess(got, want):
    """the largest distance on the circle over its bar, EL_BAR·|want| and no less than ANGLE_FLOOR: <= 1 passes"""
    return float((circle(got, want) / np.maximum(EL_BAR * np.abs(want), ANGLE_FLOOR)).max())


@pytest.mark.parametrize("case", oc.CASES, ids=CASE_IDS)
def test_the_values_are_the_restatements(device_runs, case):
    want, got = restated(case), device_runs(case)
    assert np.array_equal(got["index"], want["index"])
    w, g = want["post"], got["post"]
    assert abs(got["max_logml"] - want["max_logml"]) <= LL_BAR * max(1.0, abs(want["max_logml"]))
    e_ll = (np.abs(g[15] - w[15]) / np.maximum(1.0, np.abs(w[15]))).max()
    scale = np.linalg.norm(w[4:8], axis=0)
    e_x, e_mu = (np.abs(g[:4] - w[:4]) / scale).max(), (np.abs(g[4:8] - w[4:8]) / scale).max()
    e_el = max((np.abs(g[k] - w[k]) / np.abs(w[k])).max() for k in (8, 9, 10, 13, 14))
    e_om, e_Om = angle_excess(g[11], w[11]), angle_excess(g[12], w[12])
    e_th = max(rel(got["theta"], want["theta"]).max(), rel(got["nl"], want["nl"]).max())
    print(f"{case}: ℓ {e_ll:.2e} (bar {LL_BAR:g}) · draw {e_x:.2e}, mean {e_mu:.2e} of ‖μ‖ (bar {TI_BAR:g}) · α, a_ti, i, P_d, M_dyn {e_el:.2e} (bar {EL_BAR:g}) · "
          f"ω {e_om:.2e}, Ω {e_Om:.2e} of their bars max({EL_BAR:g}·|angle|, {ANGLE_FLOOR:g} rad) · θ, nl {e_th:.2e} (bar {TRANS_BAR:g})")
    assert e_ll <= LL_BAR and e_x <= TI_BAR and e_mu <= TI_BAR and e_el <= EL_BAR and e_th <= TRANS_BAR
    assert e_om <= 1.0 and e_Om <= 1.0
    assert np.all(g[12] >= 0) and np.all(g[12] < math.pi) and np.all(g[11] >= 0) and np.all(g[11] < 2 * math.pi)


# ---------------------------------------------------------------------------------------------------- d
def test_invalid_lanes_and_batch_shapes_leave_the_other_lanes_their_bits(pkg, draws_mod):
    import torch
    from draws_device import padded_view
    case = oc.CASES[2]
    want = restated(case)
    n = 257
    nl = np.array(want["nl"][:, :n])
    index = np.array(want["index"][:n])
    with handle(pkg, draws_mod, case[0], case[2]) as pd:
        clean = pd.ofti_posterior(case[1], index, padded_view(nl)).cpu().numpy()
        bad = nl.copy()
        lanes = [3, 64, 65, 130, 256]
        bad[4, 3], bad[0, 64], bad[1, 65], bad[0, 130], bad[3, 256] = np.nan, 1.0, -2.0, np.inf, 0.0
        view = padded_view(bad)
        assert view.stride(0) == n + 5
        got = pd.ofti_posterior(case[1], index, view)
        assert got.stride(0) == n + 5
        got = got.cpu().numpy()
        assert np.all(got[15, lanes] == -np.inf) and np.all(np.isnan(got[:15, lanes]))
        good = np.setdiff1d(np.arange(n), lanes)
        assert np.all(np.isfinite(clean)) and np.array_equal(got[:, good], clean[:, good])
        for m in (1, 63):
            part = pd.ofti_posterior(case[1], index[:m], torch.as_tensor(np.ascontiguousarray(nl[:, :m]), device="cuda")).cpu().numpy()
            assert np.array_equal(part, clean[:, :m]), m
        # and the rows are the restatement's
        assert (np.abs(clean[15] - want["post"][15, :n]) / np.maximum(1.0, np.abs(want["post"][15, :n]))).max() <= LL_BAR


# ---------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("case", [oc.CASES[0], oc.CASES[2]], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_the_elements_mean_the_draw_to_the_main_library(pkg, oracle, device_runs, case):
    """The main library's Campbell planet at (a_ti, e, i, ω, Ω, tp, M_dyn, plx) on the same table has the Gaussian log-density of data − D·x, D from
    the oracle's Kepler solve at the period the marginal likelihood was solved with: the angle convention and the M_dyn rule, by meaning."""
    tab, got = oc.table(case[0]), device_runs(case)
    post, nl = got["post"], got["nl"]
    n = post.shape[1]
    table = {"epoch": tab["epochs"], "ra": tab["ra"], "dec": tab["dec"], "σ_ra": tab["s_ra"], "σ_dec": tab["s_dec"]}
    if tab["cor"] is not None:
        table["cor"] = tab["cor"]
    obs = pkg.PlanetRelAstromObs(table, name="astrom")
    planet = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[obs])
    system = pkg.System(name="ofti", companions=[planet], observations=[])
    fn = pkg.make_ln_like(system, dict(M=1.2, plx=50.0, planets=dict(b=dict(a=10.0, e=0.3, i=1.0, ω=0.5, Ω=2.0, tp=50000.0))))
    elems = np.stack([post[9], nl[0], post[10], post[11], post[12], nl[2], post[14], nl[4], np.zeros(n)])
    ll = fn.ln_like_arrays(elems, None, grad=False)
    fn.close()
    # D·x in NumPy: X, Y from the oracle's Kepler solve
    kep = np.vectorize(oracle.load_oracle().octo_oracle_kepler_markley)
    u = (tab["epochs"][None, :] - nl[2][:, None]) / post[13][:, None]
    ma = 2 * math.pi * (u - np.rint(u))
    E = kep(ma, np.broadcast_to(nl[0][:, None], ma.shape))
    X, Y = np.cos(E) - nl[0][:, None], np.sqrt(1 - nl[0][:, None] ** 2) * np.sin(E)
    r_ra = tab["ra"][None, :] - (post[1][:, None] * X + post[3][:, None] * Y)
    r_dec = tab["dec"][None, :] - (post[0][:, None] * X + post[2][:, None] * Y)
    wrr, wdd, wrd, _, _, _, log_det = oref.weights(tab)
    want = -0.5 * ((r_ra * r_ra) @ wrr + (r_dec * r_dec) @ wdd + 2 * (r_ra * r_dec) @ wrd) - 0.5 * log_det - len(tab["epochs"]) * math.log(2 * math.pi)
    err = (np.abs(ll - want) / np.maximum(1.0, np.abs(want))).max()
    print(f"{case}: {n} accepted draws, log-density through the Campbell elements within {err:.2e} (bar 1e-8)")
    assert np.all(np.isfinite(ll)) and err <= 1e-8


# ---------------------------------------------------------------------------------------------------- f
def test_octofit_ofti_device_end_to_end(pkg, draws_mod, device_runs):
    from octofitter_jl_amd.host import predict
    case = oc.CASES[0]
    tab, full = oc.table(case[0]), device_runs(case)
    pri = oc.PRIORS_TAU
    v = pkg.variables(e=pkg.Uniform(pri[0]["p0"], pri[0]["p1"]), a=pkg.LogUniform(pri[1]["p0"], pri[1]["p1"]), τ=pkg.Uniform(0.0, 1.0),
                      M=pkg.truncated(pkg.Normal(pri[3]["p0"], pri[3]["p1"]), lower=pri[3]["lo"]),
                      plx=pkg.truncated(pkg.Normal(pri[4]["p0"], pri[4]["p1"]), lower=pri[4]["lo"]))
    # the driver counts its draws from 0: the case's window starts at FIRST, so this is a run of its own, held to the restatement
    n_draws = 1 << 17
    out = pkg.octofit_ofti_device(*oc.columns(tab), v, draws=n_draws, seed=case[1], t_ref=oc.T_REF)
    want = oref.rejection(tab, pri, case[1], 0, n_draws, 1, oc.T_REF, oc.k_yr())
    assert want["undecided"] == 0 and want["n_accepted"] >= 50
    assert out["n_accepted"] == want["n_accepted"] and np.array_equal(out["index"], want["index"])
    assert set(draws_mod.OFTI_OUTPUTS) | {"e", "a", "τ", "M", "plx", "tp", "index", "n_accepted", "max_logml"} <= set(out)
    # the bars of the values test: ℓ and its maximum, the Thiele-Innes rows per draw, the elements, the angles
    assert abs(out["max_logml"] - want["max_logml"]) <= LL_BAR * max(1.0, abs(want["max_logml"]))
    scale = np.linalg.norm(want["post"][4:8], axis=0)
    for k, name in enumerate(draws_mod.OFTI_OUTPUTS):
        w = want["post"][k]
        if name in ("ω", "Ω"):
            assert angle_excess(out[name], w) <= 1.0, name
        elif name == "logml":
            assert np.all(np.abs(out[name] - w) <= LL_BAR * np.maximum(1.0, np.abs(w))), name
        elif k < 8:
            assert np.all(np.abs(out[name] - w) <= TI_BAR * scale), name
        else:
            assert np.all(np.abs(out[name] - w) <= EL_BAR * np.abs(w)), name
    assert rel(out["tp"], want["nl"][2]).max() <= TRANS_BAR
    for k, name in enumerate(("e", "a", "τ", "M", "plx")):
        assert rel(out[name], want["theta"][k]).max() <= TRANS_BAR, name
    # posterior_predictive on its elements reproduces D·x at the table's epochs
    n = out["n_accepted"]
    elems = np.stack([out["a_ti"], out["e"], out["i"], out["ω"], out["Ω"], out["tp"], out["M_dyn"], out["plx"], np.zeros(n)])
    cube = pkg.posterior_predictive([dict(orbit_kind=0, has_mass=False)], elems, tab["epochs"], [(predict.RAOFF, 0), (predict.DECOFF, 0)], summary=False)
    nl = np.stack([out["e"], out["a"], out["tp"], out["M"], out["plx"]])
    X, Y = oref.design(tab, nl, oc.k_yr())
    ra, dec = out["B"][:, None] * X + out["G"][:, None] * Y, out["A"][:, None] * X + out["F"][:, None] * Y
    scale = out["alpha"][None, :]
    err = max((np.abs(cube[0] - ra.T) / scale).max(), (np.abs(cube[1] - dec.T) / scale).max())
    print(f"octofit_ofti_device: {n} accepted of {n_draws}; posterior_predictive within {err:.2e} of α of D·x (bar 1e-9)")
    assert err <= 1e-9


# ---------------------------------------------------------------------------------------------------- g
def test_refusals(pkg, draws_mod):
    capi = pkg.capi
    tab = oc.table("ofti_example")

    def refused(fn, text):
        with pytest.raises(capi.OctoError) as e:
            fn()
        assert e.value.status == capi.OCTO_EINVAL and text in str(e.value), str(e.value)

    with draws_mod.PriorDraws(priors=mirror_priors(pkg, oc.PRIORS_TAU[:4])) as pd:
        refused(lambda: pd.ofti_set(*oc.columns(tab)), "D = 5")
    with draws_mod.PriorDraws(priors=mirror_priors(pkg, oc.PRIORS_TAU)) as pd:
        refused(lambda: pd.ofti_rejection(41, 1000), "no table is set")
        refused(lambda: pd.ofti_nl(pd.sample(41, 0, 8)[0]), "no table is set")
        refused(lambda: pd.ofti_set(*oc.columns(tab), tp_mode=2), "tp_mode")
        bad = dict(tab, s_ra=np.where(np.arange(8) == 2, 0.0, tab["s_ra"]))
        refused(lambda: pd.ofti_set(*oc.columns(bad)), "octo_ofti_create: row 2")
        refused(lambda: pd.ofti_set(*oc.columns(tab)[:6], -1.0), "sigma_ABFG")
        pd.ofti_set(*oc.columns(tab), tp_mode=1, t_ref=oc.T_REF)
        refused(lambda: pd.ofti_rejection(41, 0), "N >= 1")
        pd.ofti_clear()
        pd.ofti_clear()
        refused(lambda: pd.ofti_rejection(41, 1000), "no table is set")
    # every ℓ = −Inf: the restatement first
    want = oref.rejection(oc.rejecting_table(), oc.PRIORS_NONE, 41, 0, oc.NONE_N, 1, oc.T_REF, oc.k_yr())
    assert np.all(want["ll"] == -np.inf)
    with draws_mod.PriorDraws(priors=mirror_priors(pkg, oc.PRIORS_NONE)) as pd:
        pd.ofti_set(*oc.columns(oc.rejecting_table()), tp_mode=1, t_ref=oc.T_REF)
        refused(lambda: pd.ofti_rejection(41, oc.NONE_N), f"All {oc.NONE_N} prior samples produced non-finite log-likelihoods. Check your model and priors.")
        # the handle is usable afterwards
        pd.ofti_set(*oc.columns(tab), tp_mode=1, t_ref=oc.T_REF)
        assert pd.ofti_rejection(41, 4096, cap=0)["n_accepted"] >= 0
