"""
The Gaussian-process RV term under DENSE kernels on the device (liboctofitter_hip_draws.so: csrc/draws/octo_draws_gpd.hip between the row passes of
octo_draws_gp.hip) against tests/gpd_reference.py at the project's oracle bar, 1e-8 relative to max(1, |ref|), on the shapes of tests/gpd_cases.py: ℓ, every
gradient, η and μ — mpmath at 50 digits up to 17 rows, the float64 NumPy restatement (held to mpmath at 1e-10 by the CPU suite) on the longer tables; the
forward-only call, the host twin and accumulate; a walker's bits in any batch; invalid walkers; the refusals; a celerite table after a dense one; the table
bound to a model's expression program; NUTS on that model. GPU suite.
"""
import numpy as np
import pytest

import gp_cases as gc
import gp_reference as gref
import gpd_cases as dc
import gpd_reference as dref
from draws_device import draws_mod      # noqa: F401  (fixture)
from test_gp import close, dev, dev_vec, dx_dtheta_t, run, set_case

pytestmark = pytest.mark.gpu

KEYS = ("ll", "g_elems", "g_hyper", "g_jitter", "g_beta")


@pytest.fixture(scope="module")
def handle(pkg, draws_mod):
    with draws_mod.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as pd:      # the table needs neither a model nor a program
        yield pd


@pytest.mark.parametrize("name", list(dc.CASES))
def test_against_the_reference(handle, name):
    x, r = dc.inputs(name), dc.reference(name)
    set_case(handle, x)
    K = x["beta"].shape[0]
    o = run(handle, x)
    assert np.all(np.isfinite(r["ll"]))      # every drawn walker is valid by construction
    for k in ("ll", "g_elems", "g_hyper", "g_jitter") + (("g_beta",) if K else ()):
        close(o[k], r[k], f"{name} {k}")
    fwd = run(handle, x, grad=False)
    assert set(fwd) == {"ll"} and np.array_equal(fwd["ll"], o["ll"])      # the forward-only call has the gradient call's bits
    eta, mu = handle.gp_values(dev(handle, x["elems"]), dev(handle, x["hyper"]), dev(handle, x["beta"]) if K else None, dev_vec(handle, x["jitter"]), mean=True)
    close(eta.cpu().numpy(), r["eta"], f"{name} eta")
    close(mu.cpu().numpy(), r["mu"], f"{name} mu")
    host = handle.gp_eval_host(x["elems"], x["hyper"], x["beta"], x["jitter"])
    for k in o:
        assert np.array_equal(host[k], o[k]), k      # the host-buffer twin is the same launches
    n, _, P, H, R = handle.gp_shape
    W = x["elems"].shape[1]
    ldw, tri = -(-W // 64) * 64, (W * n * (n + 1) // 2 if n > dref.LDS_ROWS else 0)
    assert R == 0 and H == dref.n_hyper(x["terms"]) and handle.gp_dense
    assert handle.gp_work_doubles(W, grad=False) == ldw * (n + 1) + tri
    assert handle.gp_work_doubles(W) == ldw * (n + 1 + -(-n // gref.ROWS) * (4 + 6 * P)) + tri


def test_the_refusals(pkg, handle):
    x = dc.inputs("per_wide")
    tab = x["tab"]
    args = (x["planets"], tab["t"], tab["rv"], tab["sigma"], tab["c"])
    n_long = dref.MAX_N + 1
    long_t = 55000.0 + 4.0 * np.arange(n_long)
    for bad in (lambda: handle.gp_set(*args, [dref.QUASIPERIODIC, gref.SHO]),               # mixed kinds
                lambda: handle.gp_set(*args, [gref.REAL, dref.SE]),
                lambda: handle.gp_set(*args, [dref.SE] * 5),                                # five dense terms
                lambda: handle.gp_set(x["planets"], long_t, np.zeros(n_long), np.ones(n_long), None, [dref.SE]),      # n = DENSE_MAX_N + 1
                lambda: handle.gp_set(*args, [3]),
                lambda: handle.gp_set(*args, [21]),
                lambda: handle.gp_set(*args, [15])):
        with pytest.raises(pkg.capi.OctoError) as e:
            bad()
        assert e.value.status == pkg.capi.OCTO_EINVAL
    with pytest.raises(pkg.capi.OctoError) as e:
        handle.gp_set([(gref.THIELE_INNES, 1)], *args[1:], [dref.QUASIPERIODIC])
    assert e.value.status == pkg.capi.OCTO_ENOTSUP
    handle.gp_set(x["planets"], long_t[:-1], np.zeros(n_long - 1), np.ones(n_long - 1), None, [dref.SE])      # DENSE_MAX_N rows are accepted
    handle.gp_clear()


def test_a_walkers_bits_do_not_depend_on_its_batch(handle):
    import torch
    x = dc.inputs("qp_wide")      # 130 walkers, n = 7, two planets
    set_case(handle, x)
    W = x["elems"].shape[1]
    full = run(handle, x)
    alone = run(handle, x, cols=[37])                          # a batch of 1
    shard = run(handle, x, cols=np.arange(30, 97))             # a batch of 67: block index 7 instead of 37
    wide = run(handle, x, ld=W + 13)                           # two values of ld
    wider = run(handle, x, cols=np.arange(30, 97), ld=200)
    hy = x["hyper"].copy()
    hy[1, 36] = 0.0                                            # beside an invalid neighbour
    hy[0, 38] = np.nan
    beside = run(handle, dict(x, hyper=hy))
    assert np.all(beside["ll"][[36, 38]] == -np.inf)
    for k in KEYS:
        assert np.array_equal(alone[k][..., 0], full[k][..., 37]), k
        assert np.array_equal(shard[k], full[k][..., 30:97]), k
        assert np.array_equal(wide[k], full[k]), k
        assert np.array_equal(wider[k], shard[k]), k
        assert np.array_equal(beside[k][..., 37], full[k][..., 37]), k
    zeros = dict(ll=torch.zeros(W, dtype=torch.float64, device=handle.device), g_elems=torch.zeros((x["elems"].shape[0], W), dtype=torch.float64, device=handle.device))
    acc = run(handle, x, accumulate=True, out=zeros)
    for k in KEYS:
        assert np.array_equal(acc[k], full[k]), k      # accumulate = 1 into zeroed outputs gives the store's bits
    twice = run(handle, x, accumulate=True, out=zeros)      # … and it does add
    assert np.array_equal(twice["ll"], full["ll"] + full["ll"]) and np.array_equal(twice["g_elems"], full["g_elems"] + full["g_elems"])


def test_invalid_walkers_are_minus_inf_with_a_zero_gradient_and_leave_their_neighbours_at_the_bar(handle):
    x, r = dc.inputs("qp_wide"), dc.reference("qp_wide")      # hyper rows: a, ℓ, P, r
    set_case(handle, x)
    good = run(handle, x)
    hy, jit = x["hyper"].copy(), x["jitter"].copy()
    hy[1, 3] = 0.0            # ℓ = 0
    hy[2, 9] = -12.0          # P < 0
    hy[3, 40] = 0.0           # r = 0
    hy[0, 64] = np.nan        # a = NaN
    hy[0, 65] = 1e200         # a² is not finite
    jit[17] = -0.5            # s < 0
    bad = [3, 9, 17, 40, 64, 65]
    o = run(handle, dict(x, hyper=hy, jitter=jit))
    ok = np.setdiff1d(np.arange(hy.shape[1]), bad)
    assert np.all(o["ll"][bad] == -np.inf)
    for k in ("g_elems", "g_hyper", "g_beta"):
        assert not np.any(o[k][:, bad]), k
    assert not np.any(o["g_jitter"][bad])
    for k in KEYS:
        assert np.array_equal(o[k][..., ok], good[k][..., ok]), k
        close(o[k][..., ok], r[k][..., ok], f"valid neighbours {k}")
    ref = dref.numpy_dense(x["tab"], x["terms"], x["planets"], x["elems"][:, bad], hy[:, bad], x["beta"][:, bad], jit[bad], grad=False)
    assert np.all(ref["ll"] == -np.inf)      # the reference calls the same walkers invalid


def test_a_celerite_table_after_a_dense_one_keeps_its_bits(pkg, draws_mod, handle):
    c = gc.inputs("sho_over")
    with draws_mod.PriorDraws(priors=[pkg.Uniform(0.0, 1.0)]) as fresh:
        set_case(fresh, c)
        want = run(fresh, c)
        assert not fresh.gp_dense
    for name in ("lds_last", "global_first"):      # both dense routes have used the handle's work array
        d = dc.inputs(name)
        set_case(handle, d)
        run(handle, d)
    set_case(handle, c)
    assert not handle.gp_dense and handle.gp_shape[4] == 2
    got = run(handle, c)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    close(got["ll"], gc.reference("sho_over")["ll"], "sho_over ll")


@pytest.fixture(scope="module")
def qp_model(pkg):
    from test_gp_host import system_of
    from test_gpd_host import qp_obs
    model = pkg.LogDensityModel(system_of(pkg, [qp_obs(pkg, n=20)]))
    yield model
    model.close()


def test_the_bound_table_is_a_term_of_the_models_log_posterior(pkg, draws_mod, qp_model):
    model = qp_model
    obs, nodes = model._gp
    assert model.D == 10 and obs.gp_terms == [dref.QUASIPERIODIC] and len(obs) == 20
    with draws_mod.PriorDraws(model) as pd:
        assert pd.gp_dense and pd.gp_shape == (20, 1, 1, 4, 0)
        W = 64
        _, tt, _ = pd.sample(3, 0, W)
        lp_b, g_b = (t.cpu().numpy() for t in pd.program_logpost(tt))
        pd.gp_unbind()
        lp_u, g_u = (t.cpu().numpy() for t in pd.program_logpost(tt))      # the prior and the main library's likelihood
        pd.gp_bind(nodes)
        assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), lp_b)
        el_nodes = [n for _k, n, _v in model._binds[:9]]
        elems = pd.program_values(tt, el_nodes).contiguous()
        extra = pd.program_values(tt, nodes).contiguous()
        hyper, beta, jitter = extra[:4].contiguous(), extra[4:5].contiguous(), extra[5].contiguous()
        s = {k: v.cpu().numpy() for k, v in pd.gp_eval(elems, hyper, beta, jitter).items()}
        assert np.all(np.isfinite(lp_b)) and np.all(np.isfinite(lp_u)) and np.all(np.isfinite(s["ll"]))
        ulp = np.spacing(np.maximum(np.maximum(np.abs(lp_b), np.abs(lp_u)), np.abs(s["ll"])))
        print("bound − unbound − ll_gp, in ulps:", float(np.max(np.abs((lp_b - lp_u) - s["ll"]) / ulp)))
        assert np.all(np.abs((lp_b - lp_u) - s["ll"]) <= 4 * ulp)
        planets = [(d["orbit_kind"], d["has_mass"]) for d in model.ln_like.planet_desc]
        tab = gref.table(obs.table["epoch"], obs.table["rv"], obs.table["σ_rv"], obs.gp_columns)
        r = dref.dense(tab, obs.gp_terms, planets, elems.cpu().numpy(), hyper.cpu().numpy(), beta.cpu().numpy(), jitter.cpu().numpy())
        for k in ("ll", "g_elems", "g_hyper", "g_beta", "g_jitter"):
            close(s[k], r[k], f"bound {k}")
        # the gradient: the term's adjoints at the nodes, an exp node's through its own value, then the links' dx/dθ_t
        gx = np.zeros((model.D, W))
        for k, node in enumerate(el_nodes):
            if node < model.D:
                gx[node] += r["g_elems"][k]
        ops, vals = model.program.op_names(), extra.cpu().numpy()
        for k, node in enumerate(nodes):
            g = (list(r["g_hyper"]) + list(r["g_beta"]) + [r["g_jitter"]])[k]
            if node < model.D:
                gx[node] += g
            else:
                op, a, _, _ = ops[node - model.D]
                assert op == "EXP" and a < model.D
                gx[a] += g * vals[k]
        close(g_b, g_u + gx * dx_dtheta_t(model.priors, tt.cpu().numpy()), "grad logpost")


def test_nuts_on_the_quasi_periodic_model(pkg, draws_mod, qp_model):
    with draws_mod.PriorDraws(qp_model) as pd:
        _, init, _ = pd.sample(9, 0, 64)
        assert np.all(np.isfinite(pd.program_logpost(init)[0].cpu().numpy()))
    r = pkg.octofit_nuts_device(qp_model, n_chains=64, n_warmup=5, n_samples=5, max_depth=4, seed=5, init=init)
    assert r["logpost"].shape == (5, 64) and np.all(np.isfinite(r["logpost"]))
