"""
Along-scan absolute astrometry on the device (liboctofitter_hip_draws.so: csrc/draws/octo_draws_scan.hip) against its restatement
(tests/scan_reference.py, mpmath at 50 digits) at the project's oracle bar, 1e-8 relative to max(1, |ref|), on the shapes of tests/scan_cases.py:
ℓ, every gradient, the model values η and β̂ in both modes; the marginal mode's β̂ as the stationary point of the sampled mode; a walker's bits in any
batch; invalid walkers; the table as a term of an expression program; and through the samplers. GPU suite.
"""
import numpy as np
import pytest

import scan_cases as sc
import scan_reference as sref
from draws_device import draws_mod      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BAR = 1e-8      # the README's oracle bar, relative to max(1, |ref|)


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


def dev_vec(pd, x):
    import torch
    return None if x is None else torch.as_tensor(np.asarray(x, dtype=np.float64), device=pd.device)


def set_case(pd, x):
    tab = x["tab"]
    pd.scan_set(x["planets"], tab["t"], tab["u"], tab["v"], tab["y"], tab["sigma"], tab["c"] if tab["c"].shape[0] else None)


def run(pd, x, mode, grad=True, cols=None, ld=None, accumulate=False, out=None):
    """scan_eval of the case's walkers `cols` (default all) as NumPy arrays"""
    cols = np.arange(x["elems"].shape[1]) if cols is None else np.asarray(cols)
    K = x["beta"].shape[0]
    ld = ld or len(cols)
    o = pd.scan_eval(dev(pd, x["elems"][:, cols], ld), dev(pd, x["beta"][:, cols], ld) if K else None,
                     None if x["jitter"] is None else dev_vec(pd, x["jitter"][cols]), mode=mode, grad=grad, accumulate=accumulate, out=out)
    pd.sync()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("name", list(sc.CASES))
def test_sampled_mode_against_the_restatement(handle, name):
    x, r = sc.inputs(name), sc.restated(name, sref.SAMPLED)
    set_case(handle, x)
    o = run(handle, x, "sampled")
    assert np.all(np.isfinite(r["ll"]))      # every drawn walker is valid by construction
    close(o["ll"], r["ll"], "ll")
    close(o["g_elems"], r["g_elems"], "g_elems")
    close(o["g_jitter"], r["g_jitter"], "g_jitter")
    if x["beta"].shape[0]:
        close(o["g_beta"], r["g_beta"], "g_beta")
    fwd = run(handle, x, "sampled", grad=False)
    assert np.array_equal(fwd["ll"], o["ll"])      # the forward-only kernel rounds ℓ as the gradient kernel does
    eta = handle.scan_values(dev(handle, x["elems"]), dev(handle, x["beta"]) if x["beta"].shape[0] else None).cpu().numpy()
    close(eta, r["eta"], "eta")
    host = handle.scan_eval_host(x["elems"], x["beta"], x["jitter"], mode="sampled")
    for k in o:
        assert np.array_equal(host[k], o[k]), k      # the host-buffer twin is the same launches


@pytest.mark.parametrize("name", [n for n in sc.CASES if sc.CASES[n][3] > 0])
def test_marginal_mode_against_the_restatement(handle, name):
    x, r = sc.inputs(name), sc.restated(name, sref.MARGINAL)
    set_case(handle, x)
    o = run(handle, x, "marginal")
    close(o["ll"], r["ll"], "ll_marg")
    close(o["beta_hat"], r["beta_hat"], "beta_hat")
    close(o["g_elems"], r["g_elems"], "g_elems")
    close(o["g_jitter"], r["g_jitter"], "g_jitter")
    # β̂ is the stationary point of the sampled mode: |∂ℓ/∂β_k| <= 1e-8·Σ_i w_i |r_i c_i[k]|, the bar on the sum's own scale
    y = dict(x, beta=o["beta_hat"])
    s = run(handle, y, "sampled")
    tab, W = x["tab"], x["elems"].shape[1]
    jit = np.zeros(W) if x["jitter"] is None else x["jitter"]
    eta = handle.scan_values(dev(handle, x["elems"]), dev(handle, o["beta_hat"])).cpu().numpy()
    w = 1.0 / (tab["sigma"][:, None] ** 2 + jit[None, :] ** 2)
    scale = np.einsum("iw,ki->kw", w * np.abs(tab["y"][:, None] - eta), np.abs(tab["c"]))
    print("stationarity: max |g_beta| / scale =", float(np.max(np.abs(s["g_beta"]) / np.maximum(scale, 1e-300))))
    # With n = K rows the fit is exact: r̂ is identically 0, what the device holds for it is the rounding of y − η, and the bar — a multiple of Σ w|r̂ c| —
    # is 0 in exact arithmetic. The property is asserted where the table leaves a residual, n > K; the n = K shape is held to the restatement above.
    if tab["t"].size > tab["c"].shape[0]:
        assert np.all(np.abs(s["g_beta"]) <= BAR * scale)


def test_a_rank_deficient_table_and_the_other_refusals(pkg, handle):
    x = sc.inputs("r_minus_1")
    tab = x["tab"]
    cols = tab["c"].copy()
    cols[3] = 2.0 * cols[0] - cols[1]
    args = (x["planets"], tab["t"], tab["u"], tab["v"], tab["y"], tab["sigma"])
    for bad in (lambda: handle.scan_set(*args, cols),                                              # CᵀΣ⁻¹C is singular
                lambda: handle.scan_set(*args[:5], -tab["sigma"], tab["c"]),                     # σ <= 0
                lambda: handle.scan_set(args[0], np.where(np.arange(tab["t"].size) == 2, np.nan, tab["t"]), *args[2:], tab["c"]),
                lambda: handle.scan_set([(7, 1)], *args[1:], tab["c"]),                           # an unknown orbit kind
                lambda: handle.scan_set(*args, np.ones((7, tab["t"].size)))):                     # K > OCTO_DRAWS_SCAN_MAX_K
        with pytest.raises(pkg.capi.OctoError) as e:
            bad()
        assert e.value.status == pkg.capi.OCTO_EINVAL
    y = sc.inputs("one")      # K = 0: no marginal mode
    set_case(handle, y)
    with pytest.raises(pkg.capi.OctoError) as e:
        run(handle, y, "marginal")
    assert e.value.status == pkg.capi.OCTO_EINVAL
    handle.scan_clear()
    handle.scan_shape = (1, 0, 1)      # the binding's record of a table the library no longer holds
    with pytest.raises(pkg.capi.OctoError) as e:
        run(handle, y, "sampled")
    assert e.value.status == pkg.capi.OCTO_EINVAL
    handle.scan_shape = None


@pytest.mark.parametrize("mode", ["sampled", "marginal"])
def test_a_walkers_bits_do_not_depend_on_its_batch(handle, mode):
    x = sc.inputs("r_plus_1")      # two tasks, five planets, 65 walkers
    set_case(handle, x)
    W = x["elems"].shape[1]
    keys = ("ll", "g_elems", "g_jitter") + (("g_beta",) if mode == "sampled" else ("beta_hat",))
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
    x = sc.inputs("r_plus_1")
    set_case(handle, x)
    good = run(handle, x, mode)
    el, beta, jit = x["elems"].copy(), x["beta"].copy(), x["jitter"].copy()
    el[sref.EL_E, 3] = 1.0                       # e = 1
    el[4 * 9 + sref.EL_A, 9] = -2.0              # a < 0 on the fifth planet
    jit[17] = -0.5                               # s < 0
    el[9 + sref.EL_M, 40] = np.inf               # an Inf element of the RadialVelocityOrbit planet, which contributes nothing
    el[2 * 9 + sref.EL_PLX, 64] = np.nan         # a NaN element of the planet without a mass, in the second wave
    bad = [3, 9, 17, 40, 64]
    if mode == "sampled":
        beta[1, 22] = np.nan                     # a NaN β
        bad.append(22)
    o = run(handle, dict(x, elems=el, beta=beta, jitter=jit), mode)
    ok = np.setdiff1d(np.arange(el.shape[1]), bad)
    assert np.all(o["ll"][bad] == -np.inf)
    assert not np.any(o["g_elems"][:, bad]) and not np.any(o["g_jitter"][bad])
    if mode == "sampled":
        assert not np.any(o["g_beta"][:, bad])
    for k in ("ll", "g_elems", "g_jitter") + (("g_beta",) if mode == "sampled" else ("beta_hat",)):
        assert np.array_equal(o[k][..., ok], good[k][..., ok]), k
    r = sref.evaluate(x["tab"], x["planets"], el[:, bad], beta[:, bad], jit[bad], mode=sref.SAMPLED if mode == "sampled" else sref.MARGINAL, grad=False)
    assert np.all(r["ll"] == -np.inf)            # the restatement calls the same walkers invalid


# ---------------------------------------------------------------------------------------------------- the program route and the samplers
def scan_model(pkg, mode="sampled"):
    """D = 8 (sampled): one Visual{KepOrbit} planet with a, e, mass free, the system's plx, and a five-column Hipparcos table whose parallax column
    reads the system's plx through a Derived variable; the jitter is a constant."""
    rng = np.random.default_rng(77)
    n = 21
    yr = np.sort(rng.uniform(1990.0, 1993.0, n))
    psi = rng.uniform(0, 2 * np.pi, n)
    V = pkg.variables
    beta = {} if mode == "marginal" else dict(dra=pkg.Normal(0, 5), ddec=pkg.Normal(0, 5), plx=pkg.Derived(lambda obs, system: system.plx),
                                              pmra=pkg.Normal(0, 5), pmdec=pkg.Normal(0, 5))
    obs = pkg.hipparcos_iad_obs(yr, rng.uniform(-0.7, 0.7, n), np.cos(psi), np.sin(psi), rng.normal(size=n) * 1.5, rng.uniform(0.8, 2.0, n), 50.0, 3.0, -2.0,
                                mode=mode, variables=V(**beta, jitter=0.3))
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[],
                   variables=V(a=pkg.LogUniform(2, 10), e=pkg.Uniform(0.0, 0.6), i=0.9, ω=1.1, Ω=2.3, tp=48000.0, mass=pkg.LogUniform(5.0, 60.0)))
    system = pkg.System(name="scan", companions=[b], observations=[obs], variables=V(M=1.1, plx=pkg.truncated(pkg.Normal(50.0, 0.5), lower=1.0)))
    return pkg.LogDensityModel(system)


def dx_dtheta_t(priors, theta_t):
    """d invlink_d/dθ_t at θ_t [D, W] (Bijectors' TruncatedBijector)"""
    out = np.empty_like(theta_t)
    for d, p in enumerate(priors):
        a, b = p.bounds()
        y = theta_t[d]
        if np.isfinite(a) and np.isfinite(b):
            s = 1.0 / (1.0 + np.exp(-y))
            out[d] = (b - a) * s * (1.0 - s)
        elif np.isfinite(a):
            out[d] = np.exp(y)
        elif np.isfinite(b):
            out[d] = -np.exp(y)
        else:
            out[d] = 1.0
    return out


def test_the_table_as_a_term_of_the_program(pkg, draws_mod):
    model = scan_model(pkg)
    try:
        assert model.D == 8 and model.program is not None and model.ln_like.n_obs == 0
        obs, nodes = model._scan
        with draws_mod.PriorDraws(model) as pd:
            W = 64
            _, tt, _ = pd.sample(3, 0, W)
            lp_b, g_b = (t.cpu().numpy() for t in pd.program_logpost(tt))
            el_nodes = [n for _k, n, _v in model._binds[:9]]
            elems = pd.program_values(tt, el_nodes).contiguous()
            extra = pd.program_values(tt, nodes).contiguous()
            beta, jitter = extra[:5].contiguous(), extra[5].contiguous()
            s = {k: v.cpu().numpy() for k, v in pd.scan_eval(elems, beta, jitter).items()}
            pd.scan_unbind()
            lp_u, g_u = (t.cpu().numpy() for t in pd.program_logpost(tt))
            assert np.all(np.isfinite(lp_b)) and np.all(np.isfinite(lp_u))
            # bound − unbound = ℓ_scan within 4 ulps of the largest of the three: two roundings of a three-term sum, doubled
            ulp = np.spacing(np.maximum(np.maximum(np.abs(lp_b), np.abs(lp_u)), np.abs(s["ll"])))
            print("bound − unbound − ll_scan, in ulps:", float(np.max(np.abs((lp_b - lp_u) - s["ll"]) / ulp)))
            assert np.all(np.abs((lp_b - lp_u) - s["ll"]) <= 4 * ulp)
            # ∇ℓπ: the unbound gradient + the restated scan term pushed through the bindings and the links
            tab = sref.table(obs.table["epoch"], obs.table["u"], obs.table["v"], obs.table["y"], obs.table["sigma"], obs.columns)
            r = sref.evaluate(tab, [(sref.VISUAL_KEP, 1)], elems.cpu().numpy(), beta.cpu().numpy(), jitter.cpu().numpy())
            close(s["ll"], r["ll"], "ll_scan")
            gx = np.zeros((model.D, W))      # ∂ℓ_scan/∂(natural parameters): every binding that is a parameter's own node
            for k, node in enumerate(el_nodes):
                if node < model.D:
                    gx[node] += r["g_elems"][k]
            for k, node in enumerate(nodes[:5]):
                assert node < model.D      # the parallax column's Derived is the system's plx itself: the same node as the planet's
                gx[node] += r["g_beta"][k]
            assert nodes[2] == el_nodes[7]
            want = g_u + gx * dx_dtheta_t(model.priors, tt.cpu().numpy())
            close(g_b, want, "grad logpost")
            # unbind and clear give back the unbound bits; program_set drops a binding; a table of another planet count is refused
            pd.scan_bind(nodes, "sampled")
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_b)
            pd.scan_clear()
            lp_c, g_c = (t.cpu().numpy() for t in pd.program_logpost(tt))
            assert np.array_equal(lp_c, lp_u) and np.array_equal(g_c, g_u)
            planets = [(sref.VISUAL_KEP, 1)]
            args = (obs.table["epoch"], obs.table["u"], obs.table["v"], obs.table["y"], obs.table["sigma"], obs.columns)
            pd.scan_set(planets, *args)
            pd.scan_bind(nodes, "sampled")
            pd.program_set(model.program, model._binds)
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_u)
            pd.scan_set(planets * 2, *args)
            with pytest.raises(pkg.capi.OctoError) as e:
                pd.scan_bind(nodes, "sampled")
            assert e.value.status == pkg.capi.OCTO_EINVAL
            with pytest.raises(pkg.capi.OctoError):
                pd.scan_set(planets, *args)
                pd.scan_bind(nodes[:3], "sampled")      # K + 1 bindings
    finally:
        model.close()


@pytest.mark.parametrize("mode", ["sampled", "marginal"])
def test_through_the_samplers(pkg, draws_mod, mode):
    import torch
    model = scan_model(pkg, mode)
    try:
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
