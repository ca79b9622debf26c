"""
The catalogue proper-motion anomaly on the device (liboctofitter_hip_draws.so: csrc/draws/octo_draws_pma.hip) against its restatement
(tests/pma_reference.py, mpmath at 50 digits) at the project's oracle bar, 1e-8 relative to max(1, |ref|), on the shapes of tests/pma_cases.py and on
one table built by hgca_obs: ℓ, every gradient, the catalogue values m and γ̂ in both modes; the host twin; a walker's bits in any batch; invalid
walkers; the refusals; the table as a term of an expression program; and through the samplers. GPU suite.
"""
import functools

import numpy as np
import pytest

import pma_cases as pc
import pma_reference as pref
import scan_cases as sc
import scan_reference as sref
from draws_device import draws_mod      # noqa: F401  (fixture)
from test_pma_reference import HGCA_ROW, scans
from test_scan import dx_dtheta_t

pytestmark = pytest.mark.gpu

BAR = 1e-8      # the README's oracle bar, relative to max(1, |ref|)
MODES = {"sampled": pref.SAMPLED, "marginal": pref.MARGINAL}


def close(x, ref, what):
    x, ref = np.asarray(x), np.asarray(ref)
    err = np.abs(x - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{what}: max error relative to max(1, |ref|) = {err.max() if err.size else 0.0:.3e}")
    assert np.all(err <= BAR), (what, float(err.max()), np.unravel_index(np.argmax(err), err.shape))


@pytest.fixture(scope="module")
def handle(pkg, draws_mod):
    with draws_mod.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:      # the table needs neither a model nor a program
        yield pd


def dev(pd, x, ld=None):
    """a float64 [rows, W] device tensor with contiguous rows ld apart (default W)"""
    import torch
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    t = pd._out(x.shape[1], x.shape[0], ld)
    t.copy_(torch.as_tensor(x))
    return t


def set_case(pd, x):
    tab = x["tab"]
    pd.pma_set(x["planets"], tab["t"], tab["u"], tab["v"], tab["L"], tab["d"], tab["cov"], tab["H"] if tab["H"].shape[1] else None)


def run(pd, x, mode, grad=True, cols=None, ld=None, accumulate=False, out=None):
    """pma_eval of the case's walkers `cols` (default all) as NumPy arrays"""
    cols = np.arange(x["elems"].shape[1]) if cols is None else np.asarray(cols)
    K = x["gamma"].shape[0]
    ld = ld or len(cols)
    o = pd.pma_eval(dev(pd, x["elems"][:, cols], ld), dev(pd, x["gamma"][:, cols], ld) if K else None, mode=mode, grad=grad, accumulate=accumulate, out=out)
    pd.sync()
    return {k: v.cpu().numpy() for k, v in o.items()}


@functools.lru_cache(maxsize=None)
def hgca_case(pkg):
    """a table built by hgca_obs on 20 + 20 scans, one planet, 16 walkers, with its restated values in both modes"""
    rng = np.random.default_rng(31)
    hip, gaia = scans(rng, 20, 20)
    obs = pkg.hgca_obs(HGCA_ROW, hip, gaia)
    planets = [(sref.VISUAL_KEP, 1)]
    x = dict(tab=pref.table(obs.t, obs.u, obs.v, obs.L, obs.d, obs.cov, obs.H), planets=planets, elems=sc.draw_elements(rng, planets, 16),
             gamma=np.array([[5.0], [-7.0]]) + rng.normal(size=(2, 16)) * 0.3)
    return x, {m: pref.evaluate(x["tab"], planets, x["elems"], x["gamma"], mode=m) for m in (pref.SAMPLED, pref.MARGINAL)}


def case(pkg, name, mode):
    if name == "hgca":
        x, r = hgca_case(pkg)
        return x, r[mode]
    return pc.inputs(name), pc.restated(name, mode)


@pytest.mark.parametrize("name", list(pc.CASES) + ["hgca"])
def test_sampled_mode_against_the_restatement(pkg, handle, name):
    x, r = case(pkg, name, pref.SAMPLED)
    set_case(handle, x)
    o = run(handle, x, "sampled")
    K = x["gamma"].shape[0]
    assert np.all(np.isfinite(r["ll"]))      # every drawn walker is valid by construction
    close(o["ll"], r["ll"], "ll")
    close(o["g_elems"], r["g_elems"], "g_elems")
    if K:
        close(o["g_gamma"], r["g_gamma"], "g_gamma")
    fwd = run(handle, x, "sampled", grad=False)
    assert "g_elems" not in fwd and np.array_equal(fwd["ll"], o["ll"])      # the forward-only call is the gradient call's first two kernels
    if K:
        assert np.array_equal(fwd["g_gamma"], o["g_gamma"])
    m = handle.pma_values(dev(handle, x["elems"]), dev(handle, x["gamma"]) if K else None).cpu().numpy()
    close(m, r["m"], "m")
    z = handle.pma_values(dev(handle, x["elems"])).cpu().numpy()
    close(z, r["z"], "z")
    host = handle.pma_eval_host(x["elems"], x["gamma"], mode="sampled")
    for k in o:
        assert np.array_equal(host[k], o[k]), k      # the host-buffer twin is the same launches


@pytest.mark.parametrize("name", [n for n in pc.CASES if pc.CASES[n][4] > 0] + ["hgca"])
def test_marginal_mode_against_the_restatement(pkg, handle, name):
    x, r = case(pkg, name, pref.MARGINAL)
    set_case(handle, x)
    o = run(handle, x, "marginal")
    close(o["ll"], r["ll"], "ll_marg")
    close(o["gamma_hat"], r["gamma_hat"], "gamma_hat")
    close(o["g_elems"], r["g_elems"], "g_elems")
    host = handle.pma_eval_host(x["elems"], None, mode="marginal")
    for k in o:
        assert np.array_equal(host[k], o[k]), k
    # γ̂ is the stationary point of the sampled mode: |∂ℓ/∂γ_k| <= 1e-8·Σ_q |H[q][k]·λ_q|, the bar on the sum's own scale, with λ = Σ⁻¹(d − m) at γ̂
    s = run(handle, dict(x, gamma=o["gamma_hat"]), "sampled", grad=False)
    m = handle.pma_values(dev(handle, x["elems"]), dev(handle, o["gamma_hat"])).cpu().numpy()
    tab = x["tab"]
    lam = np.linalg.solve(tab["cov"], tab["d"][:, None] - m)
    scale = np.abs(tab["H"]).T @ np.abs(lam)
    print("stationarity: max |g_gamma| / scale =", float(np.max(np.abs(s["g_gamma"]) / np.maximum(scale, 1e-300))))
    assert np.all(np.abs(s["g_gamma"]) <= BAR * scale)


@pytest.mark.parametrize("mode", ["sampled", "marginal"])
def test_a_walkers_bits_do_not_depend_on_its_batch(handle, mode):
    x = pc.inputs("r_plus_1")      # two tasks, five planets, 65 walkers
    set_case(handle, x)
    W = x["elems"].shape[1]
    keys = ("ll", "g_elems") + (("g_gamma",) if mode == "sampled" else ("gamma_hat",))
    full = run(handle, x, mode)
    alone = run(handle, x, mode, cols=[37])
    shard = run(handle, x, mode, cols=np.arange(30, 50))
    perm = np.random.default_rng(5).permutation(W)
    shuffled = run(handle, x, mode, cols=perm)
    wide = run(handle, x, mode, ld=W + 13)
    for k in keys:
        assert np.array_equal(alone[k][..., 0], full[k][..., 37]), k
        assert np.array_equal(shard[k], full[k][..., 30:50]), k
        assert np.array_equal(shuffled[k], full[k][..., perm]), k
        assert np.array_equal(wide[k], full[k]), k
    import torch
    zeros = dict(ll=torch.zeros(W, dtype=torch.float64, device=handle.device), g_elems=torch.zeros((x["elems"].shape[0], W), dtype=torch.float64, device=handle.device))
    acc = run(handle, x, mode, accumulate=True, out=zeros)
    for k in keys:
        assert np.array_equal(acc[k], full[k]), k
    twice = run(handle, x, mode, accumulate=True, out=zeros)      # … and it does add
    assert np.array_equal(twice["ll"], full["ll"] + full["ll"]) and np.array_equal(twice["g_elems"], full["g_elems"] + full["g_elems"])


@pytest.mark.parametrize("mode", ["sampled", "marginal"])
def test_invalid_walkers_are_minus_inf_with_a_zero_gradient_and_touch_no_neighbour(handle, mode):
    x = pc.inputs("r_plus_1")
    set_case(handle, x)
    good = run(handle, x, mode)
    el, gamma = x["elems"].copy(), x["gamma"].copy()
    el[sref.EL_E, 3] = 1.0                       # e = 1
    el[4 * 9 + sref.EL_A, 9] = -2.0              # a < 0 on the fifth planet
    el[9 + sref.EL_M, 40] = np.inf               # an Inf element of the RadialVelocityOrbit planet, which contributes nothing
    el[2 * 9 + sref.EL_PLX, 64] = np.nan         # a NaN element of the planet without a mass, in the second wave
    bad = [3, 9, 40, 64]
    if mode == "sampled":
        gamma[1, 22] = np.nan                    # a NaN γ
        bad.append(22)
    o = run(handle, dict(x, elems=el, gamma=gamma), mode)
    ok = np.setdiff1d(np.arange(el.shape[1]), bad)
    assert np.all(o["ll"][bad] == -np.inf)
    assert not np.any(o["g_elems"][:, bad])
    if mode == "sampled":
        assert not np.any(o["g_gamma"][:, bad])
    for k in ("ll", "g_elems") + (("g_gamma",) if mode == "sampled" else ("gamma_hat",)):
        assert np.array_equal(o[k][..., ok], good[k][..., ok]), k
    r = pref.evaluate(x["tab"], x["planets"], el[:, bad], gamma[:, bad], mode=MODES[mode], grad=False)
    assert np.all(r["ll"] == -np.inf)            # the restatement calls the same walkers invalid


def raises(pkg, status, call):
    with pytest.raises(pkg.capi.OctoError) as e:
        call()
    assert e.value.status == status, e.value


def test_the_refusals_of_the_table_and_of_eval(pkg, handle):
    x = pc.inputs("r_minus_1")      # Q = 8, K = 4
    tab = x["tab"]
    args = (x["planets"], tab["t"], tab["u"], tab["v"], tab["L"], tab["d"])
    einval = pkg.capi.OCTO_EINVAL
    indefinite = tab["cov"] - 2.0 * np.min(np.linalg.eigvalsh(tab["cov"])) * np.eye(8)
    asymmetric = tab["cov"].copy()
    asymmetric[0, 1] += 1e-3
    for bad in (lambda: handle.pma_set(*args, indefinite, tab["H"]),                                   # Σ not positive definite
                lambda: handle.pma_set(*args, asymmetric, tab["H"]),                                   # Σ not symmetric
                lambda: handle.pma_set(args[0], np.where(np.arange(tab["t"].size) == 2, np.nan, tab["t"]), *args[2:], tab["cov"], tab["H"]),
                lambda: handle.pma_set([(7, 1)], *args[1:], tab["cov"], tab["H"]),                     # an unknown orbit kind
                lambda: handle.pma_set(*args, tab["cov"], np.ones((8, 5))),                            # K > OCTO_DRAWS_PMA_MAX_K
                lambda: handle.pma_set(*args[:4], np.ones((9, 7)), np.zeros(9), np.eye(9))):           # Q > OCTO_DRAWS_PMA_MAX_Q
        raises(pkg, einval, bad)
    # a rank-deficient H is accepted by the table and refused by the marginal mode alone
    H = tab["H"].copy()
    H[:, 3] = H[:, 0] - 2.0 * H[:, 1]
    handle.pma_set(*args, tab["cov"], H)
    assert np.all(np.isfinite(run(handle, x, "sampled")["ll"]))
    raises(pkg, einval, lambda: run(handle, x, "marginal"))
    y = pc.inputs("one")      # K = 0: no marginal mode
    set_case(handle, y)
    raises(pkg, einval, lambda: run(handle, y, "marginal"))
    handle.pma_clear()
    handle.pma_shape = (1, 1, 0, 1)      # the binding's record of a table the library no longer holds
    raises(pkg, einval, lambda: run(handle, y, "sampled"))
    handle.pma_shape = None


# ---------------------------------------------------------------------------------------------------- the program route and the samplers
def pma_model(pkg, mode="sampled"):
    """D = 7 (sampled): one Visual{KepOrbit} planet with a, e, i, mass free, the system's plx, and hgca_obs on 20 + 20 scans whose γ are the sampled
    pmra and pmdec of the observation's own block."""
    rng = np.random.default_rng(78)
    hip, gaia = scans(rng, 20, 20)
    V = pkg.variables
    gam = None if mode == "marginal" else V(pmra=pkg.Normal(5.0, 2.0), pmdec=pkg.Normal(-7.0, 2.0))
    obs = pkg.HGCAObs(HGCA_ROW, hip, gaia, mode=mode, variables=gam)
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[],
                   variables=V(a=pkg.LogUniform(2, 10), e=pkg.Uniform(0.0, 0.6), i=pkg.Uniform(0.3, 1.2), ω=1.1, Ω=2.3, tp=48000.0, mass=pkg.LogUniform(5.0, 60.0)))
    system = pkg.System(name="pma", companions=[b], observations=[obs], variables=V(M=1.1, plx=pkg.truncated(pkg.Normal(50.0, 0.5), lower=1.0)))
    return pkg.LogDensityModel(system)


def test_the_table_as_a_term_of_the_program(pkg, draws_mod):
    model = pma_model(pkg)
    try:
        assert model.D == 7 and model.program is not None and model.ln_like.n_obs == 0
        obs, nodes = model._pma
        einval, enotsup = pkg.capi.OCTO_EINVAL, pkg.capi.OCTO_ENOTSUP
        with draws_mod.PriorDraws(model) as pd:
            W = 64
            _, tt, _ = pd.sample(3, 0, W)
            lp_b, g_b = (t.cpu().numpy() for t in pd.program_logpost(tt))
            el_nodes = [n for _k, n, _v in model._binds[:9]]
            elems = pd.program_values(tt, el_nodes).contiguous()
            gamma = pd.program_values(tt, nodes).contiguous()
            s = {k: v.cpu().numpy() for k, v in pd.pma_eval(elems, gamma).items()}
            pd.pma_unbind()
            lp_u, g_u = (t.cpu().numpy() for t in pd.program_logpost(tt))
            assert np.all(np.isfinite(lp_b)) and np.all(np.isfinite(lp_u))
            # bound − unbound = ℓ_pma within 4 ulps of the largest of the three: two roundings of a three-term sum, doubled
            ulp = np.spacing(np.maximum(np.maximum(np.abs(lp_b), np.abs(lp_u)), np.abs(s["ll"])))
            print("bound − unbound − ll_pma, in ulps:", float(np.max(np.abs((lp_b - lp_u) - s["ll"]) / ulp)))
            assert np.all(np.abs((lp_b - lp_u) - s["ll"]) <= 4 * ulp)
            # ∇ℓπ: the unbound gradient + the restated term pushed through the bindings and the links
            tab = pref.table(obs.t, obs.u, obs.v, obs.L, obs.d, obs.cov, obs.H)
            planets = [(sref.VISUAL_KEP, 1)]
            r = pref.evaluate(tab, planets, elems.cpu().numpy(), gamma.cpu().numpy())
            close(s["ll"], r["ll"], "ll_pma")
            gx = np.zeros((model.D, W))      # ∂ℓ_pma/∂(natural parameters): every binding that is a parameter's own node
            for k, node in enumerate(el_nodes):
                if node < model.D:
                    gx[node] += r["g_elems"][k]
            for k, node in enumerate(nodes):
                assert node < model.D
                gx[node] += r["g_gamma"][k]
            want = g_u + gx * dx_dtheta_t(model.priors, tt.cpu().numpy())
            close(g_b, want, "grad logpost")
            # unbind and clear give back the unbound bits; program_set drops a binding
            pd.pma_bind(nodes, "sampled")
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_b)
            pd.pma_clear()
            lp_c, g_c = (t.cpu().numpy() for t in pd.program_logpost(tt))
            assert np.array_equal(lp_c, lp_u) and np.array_equal(g_c, g_u)
            args = (obs.t, obs.u, obs.v, obs.L, obs.d, obs.cov)
            pd.pma_set(planets, *args, obs.H)
            pd.pma_bind(nodes, "sampled")
            pd.program_set(model.program, model._binds)
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_u)
            # the marginal binding takes no nodes and is the marginal ℓ
            pd.pma_bind([], "marginal")
            lp_m = pd.program_logpost(tt, grad=False)[0].cpu().numpy()
            sm = pd.pma_eval(elems, None, mode="marginal", grad=False)["ll"].cpu().numpy()
            ulp = np.spacing(np.maximum(np.maximum(np.abs(lp_m), np.abs(lp_u)), np.abs(sm)))
            assert np.all(np.abs((lp_m - lp_u) - sm) <= 4 * ulp)
            # the refusals of bind: wrong n_binds, both ways; a rank-deficient H and K = 0 in marginal mode; another planet count; one bound table a handle
            raises(pkg, einval, lambda: pd.pma_bind(nodes[:1], "sampled"))
            raises(pkg, einval, lambda: pd.pma_bind(nodes, "marginal"))
            assert np.array_equal(pd.program_logpost(tt, grad=False)[0].cpu().numpy(), lp_m)      # a refused bind leaves the binding as it was
            pd.pma_set(planets, *args, np.tile(np.array([[1.0, 2.0]]), (6, 1)))
            raises(pkg, einval, lambda: pd.pma_bind([], "marginal"))
            pd.pma_bind(nodes, "sampled")      # … which the sampled mode does not mind
            pd.pma_set(planets, *args, None)
            raises(pkg, einval, lambda: pd.pma_bind([], "marginal"))
            pd.pma_bind([], "sampled")
            pd.pma_set(planets * 2, *args, obs.H)
            raises(pkg, einval, lambda: pd.pma_bind(nodes, "sampled"))
            pd.pma_set(planets, *args, obs.H)
            n = obs.t.size
            pd.scan_set(planets, obs.t, obs.u, obs.v, np.zeros(n), np.ones(n))
            const = [nd for _k, nd, _v in model._binds[:9] if nd >= model.D][0]      # a constant's node stands in for the jitter
            pd.scan_bind([const], "sampled")
            raises(pkg, enotsup, lambda: pd.pma_bind(nodes, "sampled"))
            pd.scan_unbind()
            pd.pma_bind(nodes, "sampled")
            raises(pkg, enotsup, lambda: pd.scan_bind([const], "sampled"))
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_b)
    finally:
        model.close()


@pytest.mark.parametrize("mode", ["sampled", "marginal"])
def test_through_the_samplers(pkg, draws_mod, mode):
    import torch
    model = pma_model(pkg, mode)
    try:
        assert model._pma is not None and model.D == (7 if mode == "sampled" else 5)
        with draws_mod.PriorDraws(model) as pd:
            _, init, _ = pd.sample(9, 0, 64)
            r = pkg.octofit_nuts_device(model, n_chains=64, n_warmup=10, n_samples=10, max_depth=5, seed=5, init=init)
            assert r["logpost"].shape == (10, 64) and np.all(np.isfinite(r["logpost"]))
            for k in range(10):
                tt = torch.as_tensor(np.ascontiguousarray(r["samples_t"][k]), device=pd.device)
                assert np.array_equal(pd.program_logpost(tt, grad=False)[0].cpu().numpy(), r["logpost"][k]), k
            # the gradient-free routes
            tt = init.clone()
            o = pd.slice_step(tt, w=1.0, p=2, n_passes=1, seed=13, step=1)
            lp = pd.program_logpost(tt, grad=False)[0]
            assert torch.all(torch.isfinite(lp)) and torch.equal(lp, o["logpost"])
            tt = init.clone()
            o = pd.de_step(tt, n_gen=3, seed=14)
            lp = pd.program_logpost(tt, grad=False)[0]
            assert torch.all(torch.isfinite(lp)) and torch.equal(lp, o["logpost"])
    finally:
        model.close()
