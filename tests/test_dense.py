"""
The dense metric on the device (include/octofitter_hip_draws.h, the fourteenth part: octo_draws_cov_device, octo_draws_metric_dense_device,
octo_draws_metric_apply_device, octo_draws_use_metric and the dense kernels of the HMC step and NUTS; host/draws.py: PriorDraws.cov,
metric_dense, metric_apply, use_metric; host/callers.py: metric="dense") against its NumPy restatement (tests/dense_reference.py) fed by the
oracle's callback, and against the conditions tests/test_dense_reference.py establishes for the same inputs on the CPU. The restatement of the
samplers is the TEXTBOOK form (p ~ N(0, Σ⁻¹), Σ in every place the metric occurs); the device carries whitened momenta: the comparison is also
the proof that the two are one transition.

Decisions are compared on DECIDED chains (margin > 1e-6 in the restatement). Tolerances: the co-moments 1e-10·√(M2_ii·M2_jj) (the error of the
two-pass and Chan forms is O(n·2⁻⁵³) of Σ|dx_i·dx_j|, which Cauchy-Schwarz bounds by that scale); L·Lᵀ against Σ 1e-12·√(Σ_ii·Σ_jj) (an entry of Σ
near 0 has no digits of its own); the products 1e-13·Σ|terms|; θ_t, ℓπ, dH and log_accept max(1e-8, 100·s), s the restatement's own sensitivity to
one ulp of the starts (dense_cases.ONE_S, DEEP_S); Kolmogorov-Smirnov at the 0.1 % level.
"""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc
import dense_reference as dref
import draws_cases as cases
import hmc_reference as ref
import nuts_reference as nuts
from draws_device import close, dev, draws_mod, hmc_model, host, mirror_priors, padded, padded_view, same_bits, set_batch_invariant      # noqa: F401

pytestmark = pytest.mark.gpu
OUTPUTS = ("logpost", "loglike", "log_accept", "accepted", "depth", "n_leapfrog", "diverged")


@pytest.fixture(scope="module")
def prior_pd(pkg, draws_mod):
    """a handle without a model on the five priors of the stationarity condition"""
    h = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.STAT_PRIORS))
    yield h
    h.close()


@pytest.fixture(scope="module")
def model_pd(pkg, draws_mod):
    model = hmc_model(pkg)
    pd = draws_mod.PriorDraws(model)
    yield model, pd
    pd.close()
    model.close()


def packed(draws_mod, L):
    import torch
    return draws_mod.pack_lower(torch.as_tensor(np.ascontiguousarray(L), device="cuda"))


# ---------------------------------------------------------------------------------------------------- 1. the co-moments
@pytest.mark.parametrize("K", dc.COV_K)
def test_gpu_cov_against_exact_arithmetic(prior_pd, K):
    import torch
    pd = prior_pd
    for W in dc.COV_W:
        x, exact = dc.cov_case(W, K)
        x = x.copy()                     # the shared case is read-only
        view = padded_view(x)
        got = host(pd.cov(view))
        dc.check_cov(got, exact, f"W {W}, K {K}")
        # the same bits: the call again, another leading dimension with other values beyond column W, other values in the excluded chains
        assert same_bits(got, host(pd.cov(view)))
        assert same_bits(got, host(pd.cov(padded_view(x, 64, float("inf")))))
        if W >= 63:
            x2 = x.copy()
            x2[:K - 1, 5], x2[:K - 1, 7] = 123.0, -4.5e6
            assert same_bits(got, host(pd.cov(padded_view(x2))))
        out = None
        for k, (a, b) in enumerate(cases.thirds(W)):
            out = pd.cov(view[:, a:b], out=out, accumulate=k > 0)
        torch.cuda.synchronize()
        dc.check_cov(host(out), exact, f"W {W}, K {K}, thirds")
        # against the restatement's block / Chan order at the same bar
        want = dref.cov(x)
        dc.check_cov(got, (want[0], want[1], exact[2], exact[3]), f"W {W}, K {K}, restatement")


# ---------------------------------------------------------------------------------------------------- 2. the factor
@pytest.mark.parametrize("K", (1, 2, 11, 64))
def test_gpu_factor_against_the_restatement(prior_pd, draws_mod, K):
    import torch
    pd = prior_pd
    rng = np.random.default_rng(K)
    n = 4 * K + 3
    x = rng.normal(size=(K, n)) * (10.0 ** (np.arange(K) % 4 - 1))[:, None]
    P = K * (K + 1) // 2
    sentinel = np.full(P, -7.0)
    cnt, _mean, m2 = pd.cov(dev(x))
    hc, hm2 = cnt.cpu().numpy(), m2.cpu().numpy()
    for regularize in (False, True):
        chol, info = pd.metric_dense(cnt, m2, dev(sentinel), regularize=regularize)
        want, winfo = dref.factor(hc, hm2, sentinel, regularize)
        assert int(info.item()) == winfo == 0
        L, Lw = dref.unpack(chol.cpu().numpy(), K), dref.unpack(want, K)
        S = dref.unpack(hm2 / (n - 1.0), K)
        S = S + np.tril(S, -1).T
        if regularize:
            S = (n / (n + 5.0)) * S + 1e-3 * (5.0 / (n + 5.0)) * np.eye(K)
        sd = np.sqrt(np.diag(S))
        assert np.all(np.abs(L - Lw) <= 1e-10 * sd[:, None]), (K, regularize)
        assert np.all(np.abs(L @ L.T - S) <= 1e-12 * np.outer(sd, sd)), (K, regularize)
        assert np.array_equal(draws_mod.unpack_lower(chol, K).cpu().numpy(), L) and np.array_equal(draws_mod.pack_lower(dev(L)).cpu().numpy(), chol.cpu().numpy())
    if K >= 2:      # rank-deficient: n = K/2 chains (K = 2: a single chain, which the regularisation cannot mend either)
        c2, _, s2 = pd.cov(dev(x[:, :K // 2]))
        chol, info = pd.metric_dense(c2, s2, dev(sentinel), regularize=False)
        assert int(info.item()) != 0 and np.array_equal(chol.cpu().numpy(), sentinel)
        assert int(info.item()) == dref.factor(c2.cpu().numpy(), s2.cpu().numpy(), sentinel, False)[1]
        chol, info = pd.metric_dense(c2, s2, dev(sentinel), regularize=True)
        assert (int(info.item()) == 0) == (K // 2 >= 2) and np.array_equal(chol.cpu().numpy(), sentinel) == (K // 2 < 2)
    chol, info = pd.metric_dense(dev(np.array([1.0])), dev(np.zeros(P)), dev(sentinel), regularize=True)
    assert int(info.item()) == 1 and np.array_equal(chol.cpu().numpy(), sentinel)
    chol, info = pd.metric_dense(dev(np.array([10.0])), dev(np.full(P, np.nan)), dev(sentinel), regularize=True)      # a pivot that is not finite
    assert int(info.item()) == 1 and np.array_equal(chol.cpu().numpy(), sentinel)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 3. the products
@pytest.mark.parametrize("D", (1, 2, 14, 64))
def test_gpu_metric_apply(pkg, draws_mod, D):
    import torch
    n, ld = 65, 72
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.dim_priors(D)))
    try:
        im = np.array([cases.STAT_INV_MASS[d % 5] for d in range(D)])
        L = dc.factor_of(im)
        x = np.random.default_rng(D).normal(size=(D, n)) * (10.0 ** (np.arange(D) % 3 - 1))[:, None]
        chol = packed(draws_mod, L)
        for transpose in (False, True):
            want = (L.T if transpose else L) @ x
            bar = 1e-13 * dref.product_scale(L, x, transpose)
            buf, view = padded(torch, x, ld)
            out = pd.metric_apply(chol, view, transpose=transpose)
            torch.cuda.synchronize()
            assert tuple(out.shape) == (D, n) and np.all(np.abs(out.cpu().numpy() - want) <= bar), (D, transpose)
            assert np.array_equal(view.cpu().numpy(), x)                         # out of place: x is read only
            obuf, oview = padded(torch, np.zeros((D, n)), ld)
            assert pd.metric_apply(chol, view, transpose=transpose, out=oview) is oview
            assert same_bits([oview.cpu().numpy()], [out.cpu().numpy()]) and bool(torch.isnan(obuf[:, n:]).all())
            assert pd.metric_apply(chol, view, transpose=transpose, out=view) is view      # in place
            torch.cuda.synchronize()
            assert same_bits([view.cpu().numpy()], [out.cpu().numpy()]) and bool(torch.isnan(buf[:, n:]).all())
    finally:
        pd.close()


# ---------------------------------------------------------------------------------------------------- 4. one HMC step
def check_step(got, r, start, what, bar=1e-8):
    lp, ll, dH, acc, prop, out = got
    decided = np.abs(r["dH"] - r["log_u"]) > 1e-6
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)), initial=0.0))      # noqa: E731
    a = acc.astype(bool)
    same = decided & (a == r["accepted"])
    e_prop = rel(prop, r["proposal"])
    e_lp = 0.0 if lp is None else rel(lp[same], r["logpost"][same])
    scale = np.maximum(1.0, np.maximum(np.abs(r["E0"]), np.abs(r["E1"])))
    fin = np.isfinite(r["dH"])
    e_dH = float(np.max(np.abs(dH[fin] - r["dH"][fin]) / scale[fin], initial=0.0))
    print(f"{what}: acceptance {r['accepted'].mean():.3f}; {np.sum(~decided)} undecided; max errors — proposal {e_prop:.3e}, ℓπ {e_lp:.3e}, dH {e_dH:.3e}")
    assert e_prop <= bar and e_lp <= bar and e_dH <= bar, what
    assert np.array_equal(a[decided], r["accepted"][decided]) and set(np.unique(acc)) <= {0, 1}, what
    assert np.array_equal(out[:, ~a], start[:, ~a]) and np.array_equal(out[:, a], prop[:, a])


@pytest.mark.parametrize("n_leapfrog", dc.STEP_LEAPFROGS)
def test_gpu_one_step_against_the_restatement(pkg, oracle, draws_mod, model_pd, n_leapfrog):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    W, ld = dc.STEP_W, dc.STEP_LD
    beta, eps, L = dc.step_inputs()
    start = pd.sample(cases.STEP_SEED, 0, W, theta=False, logprior_t=False)[1]
    r = dref.hmc_step_dense(cases.MODEL_PRIORS, start.cpu().numpy(), beta, eps, n_leapfrog, L, cases.STEP_SEED, cases.STEP_STEP,
                            logpost=cases.oracle_logpost(oracle, cases.oracle_model(oracle)))
    assert np.mean(np.abs(r["dH"] - r["log_u"]) <= 1e-6) <= 0.01 and 0.2 < r["accepted"].mean() < 1.0, "condition on the seed (the reference alone)"
    buf, tt = padded(torch, start, ld)
    with pd.use_metric(packed(draws_mod, L)):
        lp, ll, dH, acc, prop = pd.hmc_step(tt, beta=dev(beta), eps=dev(eps), n_leapfrog=n_leapfrog, seed=cases.STEP_SEED, step=cases.STEP_STEP, want_proposal=True)
        torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, W:]).all())                                  # nothing written beyond column W
    check_step([x.cpu().numpy() for x in (lp, ll, dH, acc, prop, tt)], r, start.cpu().numpy(), f"model, L {n_leapfrog}")


@pytest.mark.parametrize("n_leapfrog", dc.STEP_LEAPFROGS)
def test_gpu_one_step_on_the_prior(prior_pd, draws_mod, n_leapfrog):
    import torch
    pd = prior_pd
    W, ld = dc.STEP_W, dc.STEP_LD
    eps, L = dc.step_prior_inputs()
    start = pd.sample(cases.STEP_SEED, 0, W, theta=False, logprior_t=False)[1]
    r = dref.hmc_step_dense(cases.STAT_PRIORS, start.cpu().numpy(), None, eps, n_leapfrog, L, cases.STEP_SEED, cases.STEP_STEP)
    buf, tt = padded(torch, start, ld)
    with pd.use_metric(packed(draws_mod, L)):
        lp, ll, dH, acc, prop = pd.hmc_step(tt, eps=dev(eps), n_leapfrog=n_leapfrog, seed=cases.STEP_SEED, step=cases.STEP_STEP, want_proposal=True)
        torch.cuda.synchronize()
    assert lp is None and ll is None and bool(torch.isnan(buf[:, W:]).all())
    check_step([None, None] + [x.cpu().numpy() for x in (dH, acc, prop, tt)], r, start.cpu().numpy(), f"prior, L {n_leapfrog}")


# ---------------------------------------------------------------------------------------------------- 5. NUTS
def numpy_outputs(tt, out):
    return [tt.cpu().numpy()] + [None if out[k] is None else out[k].cpu().numpy() for k in OUTPUTS]


def columns(x, sel):
    return [None if a is None else a[..., sel] for a in x]


def against_the_restatement(got, r, start, what, bar):
    """test_nuts.py's comparison: decisions on decided chains, values at the bar, a chain that did not move keeps its bits"""
    tt, lp, ll, la, acc, depth, nleaf, div = got
    decided = r["margin"] > nuts.MARGIN
    for name, mine, theirs in (("accepted", acc != 0, r["accepted"]), ("depth", depth, r["depth"]), ("n_leapfrog", nleaf, r["n_leapfrog"]), ("diverged", div != 0, r["diverged"])):
        assert np.array_equal(mine[decided], theirs[decided]), (what, name, np.nonzero(decided & (mine != theirs))[0])
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)), initial=0.0))      # noqa: E731
    e_tt = rel(tt[:, decided], r["theta_t"][:, decided])
    with np.errstate(invalid="ignore"):
        e_lp = 0.0 if lp is None else rel(lp[decided], r["logpost"][decided])
        fin = decided & np.isfinite(r["loglike"])
        e_ll = 0.0 if ll is None else rel(ll[fin], r["loglike"][fin])
        made = decided & (r["n_leapfrog"] > 0)
        e_la = float(np.max(np.where(la[made] == r["log_accept"][made], 0.0, np.abs(la[made] - r["log_accept"][made])), initial=0.0))
    print(f"{what}: {np.sum(~decided)} of {decided.size} undecided; max errors — θ_t {e_tt:.3e}, ℓπ {e_lp:.3e}, ℓ {e_ll:.3e}; log_accept {e_la:.3e} (bar {bar:.1e})")
    assert e_tt <= bar and e_lp <= bar and e_ll <= bar and e_la <= bar, what
    stay = acc == 0
    assert np.array_equal(tt[:, stay], start[:, stay], equal_nan=True)


def dense_transition(torch, draws_mod, pd, start, beta, eps, L, max_depth, seed, step, ld):
    buf, tt = padded(torch, start, ld)
    with pd.use_metric(packed(draws_mod, L)):
        out = pd.nuts(tt, beta=None if beta is None else dev(beta), eps=dev(eps), max_depth=max_depth, n_rounds=(1 << max_depth) - 1, seed=seed, step=step)
        torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, start.shape[1]:]).all()) and int(out["n_active"].item()) == 0
    return numpy_outputs(tt, out)


def test_gpu_one_transition_against_the_restatement(pkg, oracle, draws_mod, model_pd):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    beta, eps, im = cases.one_inputs()
    start = pd.sample(cases.ONE_SEED, 0, cases.ONE_W, theta=False, logprior_t=False)[1]
    r = dc.one_transition(oracle, start.cpu().numpy())
    cases.check_one_transition_is_decided(r)                                   # the condition on the inputs, before the device runs
    got = dense_transition(torch, draws_mod, pd, start, beta, eps, dc.factor_of(im), cases.ONE_DEPTH, cases.ONE_SEED, dc.ONE_STEP_DENSE, cases.ONE_LD)
    against_the_restatement(got, r, start.cpu().numpy(), "one transition", dc.ONE_BAR)


def test_gpu_deep_transition_against_the_restatement(pkg, oracle, draws_mod, model_pd):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    beta, eps, im = cases.deep_inputs()
    start = pd.sample(cases.ONE_SEED, 0, cases.ONE_W, theta=False, logprior_t=False)[1]
    r = dc.deep_transition(oracle, start.cpu().numpy())
    cases.check_deep_transition_is_decided(r)
    got = dense_transition(torch, draws_mod, pd, start, beta, eps, dc.factor_of(im), cases.DEEP_DEPTH, cases.ONE_SEED, dc.DEEP_STEP_DENSE, cases.ONE_LD)
    against_the_restatement(got, r, start.cpu().numpy(), "deep transition", dc.DEEP_BAR)


@pytest.mark.parametrize("D", cases.DIM_DS)
def test_gpu_dimensions(pkg, draws_mod, D):
    import torch
    priors = cases.dim_priors(D)
    eps, im = cases.dim_inputs(D)
    L = dc.factor_of(im)
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, priors))
    try:
        start = pd.sample(cases.DIM_SEED, 0, cases.DIM_W, theta=False, logprior_t=False)[1]
        r = dref.nuts_transition_dense(priors, start.cpu().numpy(), None, eps, L, cases.DIM_DEPTH, cases.DIM_SEED, cases.DIM_STEP)
        decided = r["margin"] > nuts.MARGIN
        print(f"D {D}: {cases.tree_summary(r)}")
        assert np.mean(~decided) <= cases.ONE_UNDECIDED and len(set(r["depth"][decided])) >= cases.DIM_DEPTHS, "condition on the inputs (the reference alone)"
        got = dense_transition(torch, draws_mod, pd, start, None, eps, L, cases.DIM_DEPTH, cases.DIM_SEED, cases.DIM_STEP, cases.DIM_LD)
        against_the_restatement(got, r, start.cpu().numpy(), f"D {D}", 1e-8)
    finally:
        pd.close()


# ---------------------------------------------------------------------------------------------------- 6. the diagonal factor on the device
def test_gpu_diagonal_factor_is_the_diagonal_path(pkg, oracle, draws_mod, model_pd):
    """use_metric(diag(√im)) against the diagonal kernels with im: on the chains the restatement of the diagonal transition decides, the same
    decisions, and the values within the bar; the HMC step likewise, its flags wherever |log u − dH| > 1e-6"""
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 1)
    try:
        beta, eps, im = cases.one_inputs()
        start = pd.sample(cases.ONE_SEED, 0, cases.ONE_W, theta=False, logprior_t=False)[1]
        tt = start.clone()
        out = pd.nuts(tt, beta=dev(beta), eps=dev(eps), inv_mass=im, max_depth=cases.ONE_DEPTH, n_rounds=(1 << cases.ONE_DEPTH) - 1, seed=cases.ONE_SEED, step=cases.ONE_STEP)
        r = dict(zip(("theta_t",) + OUTPUTS, numpy_outputs(tt, out)))
        r.update(accepted=r["accepted"] != 0, diverged=r["diverged"] != 0, margin=cases.one_transition(oracle, start.cpu().numpy())["margin"])
        assert np.mean(r["margin"] <= nuts.MARGIN) <= cases.ONE_UNDECIDED
        got = dense_transition(torch, draws_mod, pd, start, beta, eps, dc.diagonal_factor(im), cases.ONE_DEPTH, cases.ONE_SEED, cases.ONE_STEP, cases.ONE_LD)
        against_the_restatement(got, r, start.cpu().numpy(), "diagonal factor against the diagonal path", dc.ONE_BAR)
        t1, t2 = start.clone(), start.clone()
        step = dict(beta=dev(beta), eps=dev(eps), n_leapfrog=4, seed=cases.STEP_SEED, step=cases.STEP_STEP, want_proposal=True)
        a = [x.cpu().numpy() for x in pd.hmc_step(t1, inv_mass=im, **step)]
        with pd.use_metric(packed(draws_mod, dc.diagonal_factor(im))):
            b = [x.cpu().numpy() for x in pd.hmc_step(t2, **step)]
        decided = np.abs(np.log(ref.accept_uniforms(cases.STEP_SEED, cases.STEP_STEP, 0, cases.ONE_W)) - a[2]) > 1e-6
        fin = np.isfinite(a[2])
        assert decided.mean() >= 0.99 and np.array_equal(a[3][decided], b[3][decided])
        assert close(b[4], a[4], 1e-8) and close(b[2][fin], a[2][fin], 1e-8) and np.array_equal(b[2][~fin], a[2][~fin], equal_nan=True)
    finally:
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 7. lockstep properties
def run_rounds(torch, pd, start, beta, eps, cuts, chain0=0, ld=None, snapshots=None):
    """the one-transition case cut into calls of `cuts` rounds under the factor that is set: [θ_t, outputs] at the end"""
    W = start.shape[1]
    _buf, tt = padded(torch, start, ld or W)
    args = dict(beta=dev(beta), eps=dev(eps), max_depth=cases.ONE_DEPTH, seed=cases.ONE_SEED, step=dc.ONE_STEP_DENSE, chain0=chain0)
    out = None
    for k, n in enumerate(cuts):
        out = pd.nuts(tt, n_rounds=n, resume=k > 0, out=out, **args)
        if snapshots is not None:
            snapshots.append((numpy_outputs(tt, out), int(out["n_active"].item())))
    return numpy_outputs(tt, out)


def test_gpu_invariance_resume_and_freezing(pkg, draws_mod, model_pd):
    import torch
    model, pd = model_pd
    W, total = cases.ONE_W, (1 << cases.ONE_DEPTH) - 1
    beta, eps, im = cases.one_inputs()
    start = pd.sample(cases.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
    dead = 7
    start[3, dead] = float("nan")                                                # a dead start among the others
    chol, other = packed(draws_mod, dc.factor_of(im)), packed(draws_mod, dc.factor_of(im))
    set_batch_invariant(pkg, model, 1)
    try:
        with pd.use_metric(chol):
            full = run_rounds(torch, pd, start, beta, eps, (total,))
            assert same_bits(full, run_rounds(torch, pd, start, beta, eps, (total,)))
            assert same_bits(full, run_rounds(torch, pd, start, beta, eps, (total,), ld=cases.ONE_LD))
            half = W // 2
            parts = [run_rounds(torch, pd, start[:, a:b].contiguous(), beta[a:b], eps[a:b], (total,), chain0=a) for a, b in ((0, half), (half, W))]
            assert same_bits(columns(full, slice(0, half)), parts[0]) and same_bits(columns(full, slice(half, W)), parts[1])
            snaps = []
            assert same_bits(full, run_rounds(torch, pd, start, beta, eps, (0,) + (1,) * total + (0,), snapshots=snaps))
            assert same_bits(full, run_rounds(torch, pd, start, beta, eps, (3, 0, 5, total - 8)))
            nleaf = full[6]
            assert len(set(nleaf)) >= 3 and nleaf.max() == total
            for rounds, (snap, n_active) in enumerate(snaps[:-1]):
                ended = nleaf <= rounds
                assert same_bits(columns(snap, ended), columns(full, ended)), rounds      # a chain that ended is frozen
                assert n_active == np.sum(~ended), rounds
            assert np.array_equal(full[0][:, dead], start.cpu().numpy()[:, dead], equal_nan=True) and full[6][dead] == 0 and full[4][dead] == 0
            # a resume under another factor pointer, or none, is refused; under the pointer of the opening call it goes on
            _buf, tt = padded(torch, start, W)
            args = dict(beta=dev(beta), eps=dev(eps), max_depth=cases.ONE_DEPTH, seed=cases.ONE_SEED, step=dc.ONE_STEP_DENSE)
            out = pd.nuts(tt, n_rounds=3, **args)
            for factor in (other, None):
                pd.use_metric(factor)
                with pytest.raises(RuntimeError, match="resume needs the dense metric"):
                    pd.nuts(tt, n_rounds=1, resume=True, out=out, **args)
            pd.use_metric(chol)
            out = pd.nuts(tt, n_rounds=total - 3, resume=True, out=out, **args)
            assert same_bits(full, numpy_outputs(tt, out))
        # and the other way round: a diagonal transition is not resumed under a factor
        _buf, tt = padded(torch, start, W)
        out = pd.nuts(tt, n_rounds=3, inv_mass=im, **args)
        with pd.use_metric(chol):
            with pytest.raises(RuntimeError, match="resume needs the dense metric"):
                pd.nuts(tt, n_rounds=1, resume=True, out=out, **args)
    finally:
        pd.use_metric(None)
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 8. the prior is stationary
@pytest.mark.parametrize("sampler", ("hmc", "nuts"))
def test_gpu_prior_is_stationary(prior_pd, draws_mod, sampler):
    import torch
    pd = prior_pd
    eps, n_leapfrog = cases.STAT_SETTINGS[0]
    with pd.use_metric(packed(draws_mod, dc.stationary_factor())):
        for seed in (dc.STAT_SEEDS_HMC if sampler == "hmc" else dc.STAT_SEEDS_NUTS):
            tt = pd.sample(seed, 0, cases.STAT_W, theta=False, logprior_t=False)[1]
            start = tt.clone()
            for step in range(cases.STAT_STEPS):
                if sampler == "hmc":
                    pd.hmc_step(tt, eps=eps, n_leapfrog=n_leapfrog, seed=seed, step=step)
                else:
                    pd.nuts(tt, eps=cases.NUTS_STAT_EPS[0], max_depth=cases.NUTS_STAT_DEPTH, n_rounds=(1 << cases.NUTS_STAT_DEPTH) - 1, seed=seed, step=step)
            torch.cuda.synchronize()
            stat = cases.stationarity_statistics(tt.cpu().numpy())
            moved = float((tt != start).any(dim=0).double().mean())
            print(f"{sampler}, seed {seed}: max D_n {stat:.3e} (bar {cases.STAT_BAR:.3e}); moved {moved:.3f}")
            assert stat < cases.STAT_BAR and moved > 0.9


# ---------------------------------------------------------------------------------------------------- 9. the warm-up, teacher-forced
def test_gpu_warmup_teacher_forced(pkg, prior_pd, draws_mod):
    """every round's cov and every window's factor against the restatement applied to the DEVICE's inputs of that round"""
    import torch
    pd = prior_pd
    D = len(cases.STAT_PRIORS)
    start = pd.sample(cases.LOOP_SEED, 0, cases.LOOP_W, theta=False, logprior_t=False)[1]
    record = []
    out = pkg.hmc_warmup(pd, start.clone(), cases.LOOP_WARMUP, n_leapfrog=cases.LOOP_LEAPFROG, eps=cases.LOOP_EPS, seed=cases.LOOP_SEED, record=record, metric="dense")
    torch.cuda.synchronize()
    assert len(record) == cases.LOOP_WARMUP and getattr(pd, "_active_metric", None) is None
    windows, chol_in = 0, dref.pack(np.eye(D))
    for r, rec in enumerate(record):
        if rec["in_window"]:
            tt = rec["theta_t"].cpu().numpy()
            got = host(rec["mom"])
            want = dref.cov(tt) if rec["first"] else dref.cov(tt, held=host(rec["mom_in"]))
            i, j = np.tril_indices(D)
            diag = np.abs(want[2][[k * (k + 1) // 2 + k for k in range(D)]])
            assert np.array_equal(got[0], want[0]), r
            assert np.all(np.abs(got[1] - want[1]) <= want[0][0] * cases.U * np.maximum(np.max(np.abs(tt), axis=1), np.abs(want[1]))), r
            assert np.all(np.abs(got[2] - want[2]) <= cases.M2_BAR * np.sqrt(diag[i] * diag[j])), r
        if rec["last"]:
            windows += 1
            hm = host(rec["mom"])
            want, info = dref.factor(hm[0], hm[2], chol_in, regularize=True)
            assert int(rec["info"].item()) == info == 0
            Lg, Lw = dref.unpack(rec["chol"].cpu().numpy(), D), dref.unpack(want, D)
            assert np.all(np.abs(Lg - Lw) <= 1e-12 * np.sqrt(np.sum(Lw * Lw, axis=1))[:, None]), r      # relative to √Σ_ii: an entry near 0 has no digits of its own
            chol_in = rec["chol"].cpu().numpy()
    L = out["metric_chol"].cpu().numpy()
    assert windows == 1 and L.shape == (D, D) and np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0) and not np.array_equal(L, np.eye(D))
    assert np.array_equal(dref.pack(L), chol_in)
    assert close(out["inv_mass"].cpu().numpy(), np.sum(L * L, axis=1), 1e-15, scale_one=False)


# ---------------------------------------------------------------------------------------------------- 10. the drivers
@pytest.mark.parametrize("driver", ("nuts", "hmc"))
def test_gpu_drivers(pkg, driver):
    model = hmc_model(pkg)
    try:
        D = model.D
        init = pkg.pathfinder_device(model, n_draws=64, seed=3)["theta_t"]
        fit = (lambda **kw: pkg.octofit_nuts_device(model, max_depth=5, **kw)) if driver == "nuts" else (lambda **kw: pkg.octofit_hmc_device(model, n_leapfrog=4, **kw))
        args = dict(n_chains=64, n_warmup=40, n_samples=10, init=init, seed=3)
        r = fit(metric="dense", **args)
        L = r["metric_chol"]
        assert np.all(np.isfinite(r["samples"])) and r["samples"].shape == (10, D, 64) and np.all(np.isfinite(r["logpost"]))
        assert L.shape == (D, D) and np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
        assert close(r["inv_mass"], np.diag(L @ L.T), 1e-14, scale_one=False)
        assert np.any(np.tril(L, -1) != 0)                                      # the warm-up's window wrote a correlated factor
        plain = fit(**args)
        assert "metric_chol" not in plain and plain["inv_mass"].shape == (D,)
        with pytest.raises(ValueError):
            fit(metric="full", **args)
    finally:
        model.close()


# ---------------------------------------------------------------------------------------------------- 11. argument checks
def test_gpu_argument_checks(pkg, draws_mod, prior_pd):
    import torch
    pd = prior_pd
    lib, h, EINVAL = pd.lib, pd._h, pkg.capi.OCTO_EINVAL
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    W, K = 8, 5
    x = torch.zeros((K, W), dtype=torch.float64, device="cuda")
    bufs = [torch.zeros(64 * 65 // 2, dtype=torch.float64, device="cuda") for _ in range(4)]
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    X, I, (c, m, s, L) = x.data_ptr(), info.data_ptr(), [t.data_ptr() for t in bufs]

    def cov(W_=W, ld=W, K_=K, x_=X, acc=0, c_=c, m_=m, s_=s):
        return lib.octo_draws_cov_device(h, W_, ld, K_, x_, acc, c_, m_, s_, st)
    assert cov() == 0 and cov(W_=0) == 0 and cov(W_=0, x_=None) == 0 and cov(K_=1) == 0
    assert all(r == EINVAL for r in (cov(x_=None), cov(c_=None), cov(m_=None), cov(s_=None), cov(K_=0), cov(K_=65), cov(W_=-1), cov(ld=W - 1),
                                     cov(W_=(1 << 24) + 1, ld=(1 << 24) + 1)))

    def fac(K_=K, c_=c, s_=s, L_=L, i_=I):
        return lib.octo_draws_metric_dense_device(h, K_, c_, s_, 1, L_, i_, st)
    assert fac() == 0 and fac(K_=64) == 0
    assert all(r == EINVAL for r in (fac(K_=0), fac(K_=65), fac(c_=None), fac(s_=None), fac(L_=None), fac(i_=None)))

    def app(n=W, ld=W, L_=L, x_=X, o=X):
        return lib.octo_draws_metric_apply_device(h, n, ld, L_, 0, x_, o, st)
    assert app() == 0 and app(n=0, x_=None, o=None) == 0
    assert all(r == EINVAL for r in (app(L_=None), app(x_=None), app(o=None), app(n=-1), app(ld=W - 1)))
    torch.cuda.synchronize()
    # while a factor is set the samplers refuse an inv_mass, on device and host buffers alike
    chol = draws_mod.pack_lower(torch.eye(5, dtype=torch.float64, device="cuda"))
    tt = pd.sample(1, 0, W, theta=False, logprior_t=False)[1]
    with pd.use_metric(chol):
        for call in (lambda: pd.hmc_step(tt, eps=0.1, inv_mass=np.ones(5)), lambda: pd.nuts(tt, eps=0.1, inv_mass=np.ones(5), max_depth=2, n_rounds=1)):
            with pytest.raises(RuntimeError, match="d_inv_mass must be NULL"):
                call()
        th = np.ascontiguousarray(tt.cpu().numpy())
        acc = np.zeros(W, dtype=np.int32)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
        host_call = lambda im: lib.octo_draws_hmc_step(h, 0, 0, 0, W, W, dp(th), None, None, 0.1, 2, im, None, None, None, None, acc.ctypes.data_as(C.POINTER(C.c_int32)))      # noqa: E731
        assert host_call(dp(np.ones(5))) == EINVAL and host_call(None) == 0
    assert getattr(pd, "_active_metric", None) is None
    pd.hmc_step(tt, eps=0.1, inv_mass=np.ones(5))                                # back on the diagonal metric
    with pytest.raises(ValueError):
        pd.use_metric(chol[:-1])
    with pytest.raises(ValueError):
        pd.cov(x, accumulate=True)
    # D > OCTO_DRAWS_DENSE_MAX_D: octo_draws_create takes at most 64 coordinates, so no handle reaches the check of octo_draws_use_metric; the bound is
    # the same number, and a handle at the bound takes a factor
    assert draws_mod.DENSE_MAX_D == 64
    with pytest.raises(RuntimeError):
        draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.dim_priors(65)))
    top = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.dim_priors(64)))
    try:
        with top.use_metric(draws_mod.pack_lower(torch.eye(64, dtype=torch.float64, device="cuda"))):
            pass
    finally:
        top.close()
