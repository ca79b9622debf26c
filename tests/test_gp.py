"""
The Gaussian-process RV term on the device (liboctofitter_hip_draws.so: csrc/draws/octo_draws_gp.hip) against the dense reference (tests/gp_reference.py,
mpmath at 50 digits: the covariance, its Cholesky factor and ½αᵀ∂Kα − ½tr(K⁻¹∂K), no recursion in it) at the project's oracle bar, 1e-8 relative to
max(1, |ref|), on the shapes of tests/gp_cases.py: ℓ, every gradient, the model values η and the conditional mean μ; a walker's bits in any batch;
invalid walkers; the refusals; the table as a term of an expression program; and a model with a `gaussian_process` closure through the samplers. GPU suite.
"""
import numpy as np
import pytest

import gp_cases as gc
import gp_reference as gref
from draws_device import draws_mod      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BAR = 1e-8      # the README's oracle bar, relative to max(1, |ref|)
KEYS = ("ll", "g_elems", "g_hyper", "g_jitter")


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
    pd.gp_set(x["planets"], tab["t"], tab["rv"], tab["sigma"], tab["c"] if tab["c"].shape[0] else None, x["terms"])


def run(pd, x, grad=True, cols=None, ld=None, accumulate=False, out=None):
    """gp_eval of the case's walkers `cols` (default all) as NumPy arrays"""
    cols = np.arange(x["elems"].shape[1]) if cols is None else np.asarray(cols)
    K = x["beta"].shape[0]
    ld = ld or len(cols)
    o = pd.gp_eval(dev(pd, x["elems"][:, cols], ld), dev(pd, x["hyper"][:, cols], ld), dev(pd, x["beta"][:, cols], ld) if K else None,
                   None if x["jitter"] is None else dev_vec(pd, x["jitter"][cols]), grad=grad, accumulate=accumulate, out=out)
    pd.sync()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("name", list(gc.CASES))
def test_against_the_dense_reference(handle, name):
    x, r = gc.inputs(name), gc.reference(name)
    set_case(handle, x)
    K = x["beta"].shape[0]
    o = run(handle, x)
    assert np.all(np.isfinite(r["ll"]))      # every drawn walker is valid by construction
    close(o["ll"], r["ll"], "ll")
    close(o["g_elems"], r["g_elems"], "g_elems")      # the φ = 0 table's gradient among them: finite and at the bar
    close(o["g_hyper"], r["g_hyper"], "g_hyper")
    close(o["g_jitter"], r["g_jitter"], "g_jitter")
    if K:
        close(o["g_beta"], r["g_beta"], "g_beta")
    fwd = run(handle, x, grad=False)
    assert set(fwd) == {"ll"} and np.array_equal(fwd["ll"], o["ll"])      # the forward-only call has the gradient call's bits
    eta, mu = handle.gp_values(dev(handle, x["elems"]), dev(handle, x["hyper"]), dev(handle, x["beta"]) if K else None, dev_vec(handle, x["jitter"]), mean=True)
    close(eta.cpu().numpy(), r["eta"], "eta")
    close(mu.cpu().numpy(), r["mu"], "mu")
    host = handle.gp_eval_host(x["elems"], x["hyper"], x["beta"], x["jitter"])
    for k in o:
        assert np.array_equal(host[k], o[k]), k      # the host-buffer twin is the same launches
    n, _, P, _, R = handle.gp_shape
    W = x["elems"].shape[1]
    ldw, Rp = -(-W // 64) * 64, (2 if R <= 2 else 4 if R <= 4 else 8)
    ns = Rp * (Rp + 1) // 2 + Rp
    assert handle.gp_work_doubles(W, grad=False) == ldw * (n + 1)
    assert handle.gp_work_doubles(W) == ldw * (n + 1 + (-(-n // gref.SEGMENT) + gref.SEGMENT) * ns + -(-n // gref.ROWS) * (4 + 6 * P))


def test_the_refusals(pkg, handle):
    x = gc.inputs("sho_over")
    tab = x["tab"]
    args = (x["planets"], tab["t"], tab["rv"], tab["sigma"], tab["c"])
    t_bad = tab["t"].copy()
    t_bad[3] = t_bad[1] - 1.0
    for bad in (lambda: handle.gp_set(*args[:3], -tab["sigma"], tab["c"], x["terms"]),                       # σ <= 0
                lambda: handle.gp_set(args[0], t_bad, *args[2:], x["terms"]),                                # epochs that decrease
                lambda: handle.gp_set(args[0], np.where(np.arange(tab["t"].size) == 2, np.nan, tab["t"]), *args[2:], x["terms"]),
                lambda: handle.gp_set([(7, 1)], *args[1:], x["terms"]),                                      # an unknown orbit kind
                lambda: handle.gp_set(*args[:4], np.ones((5, tab["t"].size)), x["terms"]),                   # K > OCTO_DRAWS_GP_MAX_K
                lambda: handle.gp_set(*args, [3]),                                                           # an unknown term kind
                lambda: handle.gp_set(*args, [gref.REAL] * 5),                                               # more than OCTO_DRAWS_GP_MAX_TERMS
                lambda: handle.gp_set(*args, [])):
        with pytest.raises(pkg.capi.OctoError) as e:
            bad()
        assert e.value.status == pkg.capi.OCTO_EINVAL
    with pytest.raises(pkg.capi.OctoError) as e:
        handle.gp_set([(gref.THIELE_INNES, 1)], *args[1:], x["terms"])
    assert e.value.status == pkg.capi.OCTO_ENOTSUP
    handle.gp_set([(gref.THIELE_INNES, 0), (gref.VISUAL_KEP, 1)], *args[1:], x["terms"])      # without a mass it contributes nothing and is accepted
    handle.gp_clear()      # no table: the library itself refuses an evaluation
    assert handle.lib.octo_draws_gp_eval_device(handle._h, None, 1, 1, None, None, None, None, None, None, None, None, 0, None) == pkg.capi.OCTO_EINVAL
    assert handle.lib.octo_draws_gp_clear(None) == pkg.capi.OCTO_EINVAL      # a NULL handle is refused first


def test_a_walkers_bits_do_not_depend_on_its_batch(handle):
    x = gc.inputs("sho_both")      # 130 walkers on both sides of Q = ½, K = 4
    set_case(handle, x)
    W = x["elems"].shape[1]
    keys = KEYS + ("g_beta",)
    full = run(handle, x)
    alone = run(handle, x, cols=[37])
    shard = run(handle, x, cols=np.arange(30, 90))
    perm = np.random.default_rng(5).permutation(W)
    shuffled = run(handle, x, cols=perm)
    wide = run(handle, x, ld=W + 13)
    for k in keys:
        assert np.array_equal(alone[k][..., 0], full[k][..., 37]), k
        assert np.array_equal(shard[k], full[k][..., 30:90]), k
        assert np.array_equal(shuffled[k], full[k][..., perm]), k
        assert np.array_equal(wide[k], full[k]), k
    import torch
    zeros = dict(ll=torch.zeros(W, dtype=torch.float64, device=handle.device), g_elems=torch.zeros((x["elems"].shape[0], W), dtype=torch.float64, device=handle.device))
    acc = run(handle, x, accumulate=True, out=zeros)
    for k in keys:
        assert np.array_equal(acc[k], full[k]), k
    twice = run(handle, x, accumulate=True, out=zeros)      # … and it does add
    assert np.array_equal(twice["ll"], full["ll"] + full["ll"]) and np.array_equal(twice["g_elems"], full["g_elems"] + full["g_elems"])


def test_invalid_walkers_are_minus_inf_with_a_zero_gradient_and_touch_no_neighbour(handle):
    x = gc.inputs("sho_both")
    set_case(handle, x)
    good = run(handle, x)
    el, hy, beta, jit = x["elems"].copy(), x["hyper"].copy(), x["beta"].copy(), x["jitter"].copy()
    el[gref.EL_E, 3] = 1.0            # e = 1
    jit[17] = -0.5                    # s < 0
    hy[2, 9] = -0.2                   # ω0 < 0: the rates are <= 0
    hy[1, 40] = 0.5                   # Q = ½
    hy[0, 64] = np.nan                # a NaN hyperparameter, in the second wave
    hy[0, 22] = -40.0                 # S0 < 0: the kernel is not positive definite
    beta[1, 70] = np.inf
    bad = [3, 9, 17, 22, 40, 64, 70]
    o = run(handle, dict(x, elems=el, hyper=hy, beta=beta, jitter=jit))
    ok = np.setdiff1d(np.arange(el.shape[1]), bad)
    assert np.all(o["ll"][bad] == -np.inf)
    for k in ("g_elems", "g_hyper", "g_beta"):
        assert not np.any(o[k][:, bad]), k
    assert not np.any(o["g_jitter"][bad])
    for k in KEYS + ("g_beta",):
        assert np.array_equal(o[k][..., ok], good[k][..., ok]), k
    r = gref.dense(x["tab"], x["terms"], x["planets"], el[:, bad], hy[:, bad], beta[:, bad], jit[bad], grad=False)
    assert np.all(r["ll"] == -np.inf)            # the reference calls the same walkers invalid


# ---------------------------------------------------------------------------------------------------- the program route
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


def gp_model(pkg):
    """D = 9: one RadialVelocityOrbit planet (a, e, ω, mass free) and the Gaussian process's S0, Q, ω0, the offset and the jitter as the system's free
    parameters; a Derived variable makes the model take the program route."""
    rng = np.random.default_rng(99)
    n = 21
    V = pkg.variables
    b = pkg.Planet(name="b", basis="RadialVelocityOrbit", observations=[],
                   variables=V(a=pkg.LogUniform(0.5, 3.0), e=pkg.Uniform(0.0, 0.5), ω=pkg.Uniform(0.0, 6.28), tp=55010.0, mass=pkg.LogUniform(0.5, 5.0)))
    system = pkg.System(name="gp", companions=[b], observations=[],
                        variables=V(M=1.0, S0=pkg.LogUniform(1.0, 30.0), Q=pkg.Uniform(0.6, 5.0), w0=pkg.LogUniform(0.05, 1.0), off=pkg.Normal(0, 10),
                                    jit=pkg.LogUniform(0.1, 2.0), dummy=pkg.Derived(lambda system: system.S0 + system.Q + system.w0 + system.off + system.jit)))
    tab = gref.table(np.sort(rng.uniform(55000.0, 55080.0, n)), rng.normal(size=n) * 8.0, rng.uniform(0.5, 3.0, n), np.ones((1, n)))
    return pkg.LogDensityModel(system), tab


def test_the_table_as_a_term_of_the_program(pkg, draws_mod):
    model, tab = gp_model(pkg)
    try:
        assert model.program is not None
        with draws_mod.PriorDraws(model) as pd:
            W = 64
            _, tt, _ = pd.sample(3, 0, W)
            nodes = [model._index[("sys", k)] for k in ("S0", "Q", "w0", "off", "jit")]      # a free parameter's node is its θ index
            planets = [(d["orbit_kind"], d["has_mass"]) for d in model.ln_like.planet_desc]
            lp_u, g_u = (t.cpu().numpy() for t in pd.program_logpost(tt))
            pd.gp_set(planets, tab["t"], tab["rv"], tab["sigma"], tab["c"], [gref.SHO])
            pd.gp_bind(nodes)
            lp_b, g_b = (t.cpu().numpy() for t in pd.program_logpost(tt))
            el_nodes = [n for _k, n, _v in model._binds[:9]]
            elems = pd.program_values(tt, el_nodes).contiguous()
            extra = pd.program_values(tt, nodes).contiguous()
            hyper, beta, jitter = extra[:3].contiguous(), extra[3:4].contiguous(), extra[4].contiguous()
            s = {k: v.cpu().numpy() for k, v in pd.gp_eval(elems, hyper, beta, jitter).items()}
            assert np.all(np.isfinite(lp_b)) and np.all(np.isfinite(lp_u))
            ulp = np.spacing(np.maximum(np.maximum(np.abs(lp_b), np.abs(lp_u)), np.abs(s["ll"])))
            print("bound − unbound − ll_gp, in ulps:", float(np.max(np.abs((lp_b - lp_u) - s["ll"]) / ulp)))
            assert np.all(np.abs((lp_b - lp_u) - s["ll"]) <= 4 * ulp)
            r = gref.dense(tab, [gref.SHO], planets, elems.cpu().numpy(), hyper.cpu().numpy(), beta.cpu().numpy(), jitter.cpu().numpy())
            close(s["ll"], r["ll"], "ll_gp")
            gx = np.zeros((model.D, W))
            for k, node in enumerate(el_nodes):
                if node < model.D:
                    gx[node] += r["g_elems"][k]
            for k, node in enumerate(nodes):
                assert node < model.D
                gx[node] += (list(r["g_hyper"]) + list(r["g_beta"]) + [r["g_jitter"]])[k]
            close(g_b, g_u + gx * dx_dtheta_t(model.priors, tt.cpu().numpy()), "grad logpost")
            # unbind and clear give back the unbound bits; program_set drops a binding; the mutual refusals with scan and pma
            pd.gp_unbind()
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_u)
            pd.gp_bind(nodes)
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_b)
            n = tab["t"].size
            pd.scan_set(planets, tab["t"], np.ones(n), np.zeros(n), tab["rv"], tab["sigma"], None)
            with pytest.raises(pkg.capi.OctoError) as e:
                pd.scan_bind([nodes[-1]], "sampled")
            assert e.value.status == pkg.capi.OCTO_ENOTSUP
            pd.gp_unbind()
            pd.scan_bind([nodes[-1]], "sampled")
            with pytest.raises(pkg.capi.OctoError) as e:
                pd.gp_bind(nodes)
            assert e.value.status == pkg.capi.OCTO_ENOTSUP
            pd.scan_clear()
            pd.gp_bind(nodes)
            pd.program_set(model.program, model._binds)
            assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_u)
            pd.gp_bind(nodes)
            pd.gp_clear()
            lp_c, g_c = (t.cpu().numpy() for t in pd.program_logpost(tt))
            assert np.array_equal(lp_c, lp_u) and np.array_equal(g_c, g_u)
            pd.gp_set(planets, tab["t"], tab["rv"], tab["sigma"], tab["c"], [gref.SHO])
            with pytest.raises(pkg.capi.OctoError) as e:
                pd.gp_bind(nodes[:3])      # H + K + 1 bindings
            assert e.value.status == pkg.capi.OCTO_EINVAL
            # through a sampler: the bound term is part of every ℓπ the handle forms
            pd.gp_bind(nodes)
            o = pd.slice_step(tt.clone(), w=1.0, p=2, n_passes=1, seed=13, step=1)
            assert np.all(np.isfinite(o["logpost"].cpu().numpy()))
    finally:
        model.close()


def test_a_gp_model_through_the_samplers(pkg, draws_mod):
    """D = 9: one RadialVelocityOrbit planet (a, e, ω, mass) and an absolute-RV table of 21 rows under an SHO whose S0 is exp(log_S0)."""
    import torch
    from test_gp_host import gp_obs, system_of
    model = pkg.LogDensityModel(system_of(pkg, [gp_obs(pkg)]))
    try:
        assert model.D == 9 and model._gp is not None
        with draws_mod.PriorDraws(model) as pd:
            _, init, _ = pd.sample(9, 0, 64)
            bound = pd.program_logpost(init)[0].cpu().numpy()
            pd.gp_unbind()
            assert np.all(np.isfinite(bound)) and not np.array_equal(pd.program_logpost(init)[0].cpu().numpy(), bound)      # the term is in ℓπ
            pd.gp_bind(model._gp[1])
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
