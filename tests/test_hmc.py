"""
The tempered HMC explorer on the device (include/octofitter_hip_draws.h: octo_draws_momentum_device, octo_draws_hmc_step_device,
octo_draws_hmc_step; host/draws.py: PriorDraws.momentum / hmc_step; host/callers.py: octofit_pt_device) against its NumPy restatement
(tests/hmc_reference.py) fed by the oracle's callback, and against the two stationarity conditions that tests/test_hmc_reference.py
establishes for the same seeds on the CPU.

Tolerances: momenta 1e-11 relative to max(1, |ref|), the bar tests/test_prior_draws.py holds the device quantiles to; proposal, ℓπ and ℓ the
project's oracle bar 1e-8 relative to max(1, |ref|); dH 1e-8·max(1, |E|) absolute; Kolmogorov-Smirnov bars at the 0.1 % level.
"""
import ctypes as C
import math

import numpy as np
import pytest

import draws_cases as cases
import hmc_reference as ref
from draws_device import draws_mod, hmc_model, mirror_priors, padded, same_bits, set_batch_invariant      # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- 1. momentum
@pytest.mark.parametrize("D", (1, 4, 5, 11, 64))
def test_gpu_momentum(pkg, draws_mod, D):
    from scipy.special import ndtri
    import torch
    pd = draws_mod.PriorDraws(priors=[pkg.Uniform(0, 1)] * D)
    n, seed = 1000, 20240607
    im = 0.0025 * 4.0 ** (np.arange(D) % 7)
    worst = 0.0
    for chain0 in (0, (1 << 40) + 3):
        for step in (0, 7):
            z = ndtri(ref.momentum_uniforms(seed, step, chain0, n, D))
            for inv_mass in (None, im):
                p = pd.momentum(seed, step, n, inv_mass=inv_mass, chain0=chain0).cpu().numpy()
                got = p if inv_mass is None else p * np.sqrt(im)[:, None]
                err = np.max(np.abs(got - z) / np.maximum(1.0, np.abs(z)))
                worst = max(worst, err)
                assert err <= 1e-11, (D, chain0, step, inv_mass is None, err)
    # a padded leading dimension: nothing written beyond column n
    buf = torch.full((D, n + 5), float("nan"), dtype=torch.float64, device="cuda")
    st = pd.lib.octo_draws_momentum_device(pd._h, seed, 7, 3, n, n + 5, None, buf.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, n:]).all()) and np.array_equal(buf[:, :n].cpu().numpy(), pd.momentum(seed, 7, n, chain0=3).cpu().numpy())
    print(f"D {D}: momentum max rel err {worst:.3e}")
    pd.close()


# ---------------------------------------------------------------------------------------------------- 2. one step against the restatement
STEP_W, STEP_LD, STEP_SEED, step_inputs = cases.STEP_W, cases.STEP_LD, cases.STEP_SEED, cases.step_inputs


@pytest.fixture(scope="module")
def step_model(pkg, draws_mod):
    model = hmc_model(pkg)
    pd = draws_mod.PriorDraws(model)
    yield model, pd
    pd.close()
    model.close()


@pytest.mark.parametrize("n_leapfrog", (1, 3))
def test_gpu_one_step_against_the_restatement(pkg, oracle, draws_mod, step_model, n_leapfrog):
    import torch
    model, pd = step_model
    set_batch_invariant(pkg, model, 0)
    W, ld, seed, step = STEP_W, STEP_LD, STEP_SEED, cases.STEP_STEP
    beta, eps, im = step_inputs()
    start = pd.sample(seed, 0, W, theta=False, logprior_t=False)[1]
    buf, tt = padded(torch, start, ld)
    dev = tt.device
    r = ref.hmc_step(cases.MODEL_PRIORS, start.cpu().numpy(), beta, eps, n_leapfrog, im, seed, cases.STEP_STEP, logpost=cases.oracle_logpost(oracle, cases.oracle_model(oracle)))
    margin = np.abs(r["dH"] - r["log_u"])
    decided = margin > 1e-6
    print(f"L {n_leapfrog}: reference acceptance {r['accepted'].mean():.3f}; {np.sum(~decided)} of {W} chains within 1e-6 of the decision")
    assert np.mean(~decided) <= 0.01, "condition on the seed (the reference alone)"
    assert 0.2 < r["accepted"].mean() < 0.98 and np.all(np.isfinite(r["proposal"]))
    lp, ll, dH, acc, prop = pd.hmc_step(tt, beta=torch.as_tensor(beta, device=dev), eps=torch.as_tensor(eps, device=dev), n_leapfrog=n_leapfrog, inv_mass=im,
                                        seed=seed, step=step, want_proposal=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, W:]).all())                                  # nothing written beyond column W
    lp, ll, dH, acc, prop, out = (x.cpu().numpy() for x in (lp, ll, dH, acc, prop, tt))
    rel = lambda x, y: np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)))      # noqa: E731
    e_prop = rel(prop, r["proposal"])
    same = decided & (acc.astype(bool) == r["accepted"])
    e_lp, e_ll = rel(lp[same], r["logpost"][same]), rel(ll[same], r["loglike"][same])
    scale = np.maximum(1.0, np.maximum(np.abs(r["E0"]), np.abs(r["E1"])))
    e_dH = np.max(np.abs(dH - r["dH"]) / scale)
    print(f"L {n_leapfrog}: max errors — proposal {e_prop:.3e}, logpost {e_lp:.3e}, loglike {e_ll:.3e} (relative to max(1, |ref|)); dH {e_dH:.3e} of max(1, |E|)")
    assert e_prop <= 1e-8 and e_lp <= 1e-8 and e_ll <= 1e-8 and e_dH <= 1e-8
    assert np.array_equal(acc.astype(bool)[decided], r["accepted"][decided])
    assert set(np.unique(acc)) <= {0, 1}
    # a rejected chain keeps its input bit for bit; an accepted one holds its proposal
    a = acc.astype(bool)
    assert np.array_equal(out[:, ~a], start.cpu().numpy()[:, ~a]) and np.array_equal(out[:, a], prop[:, a])


# ---------------------------------------------------------------------------------------------------- 3. β = 0 stationarity
@pytest.mark.parametrize("eps,n_leapfrog", cases.STAT_SETTINGS)
def test_gpu_prior_is_stationary(pkg, draws_mod, eps, n_leapfrog):
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.STAT_PRIORS))
    for seed in cases.STAT_SEEDS:
        tt = pd.sample(seed, 0, cases.STAT_W, theta=False, logprior_t=False)[1]
        start = tt.clone()
        accs = []
        for step in range(cases.STAT_STEPS):
            lp, ll, _dH, acc = pd.hmc_step(tt, eps=eps, n_leapfrog=n_leapfrog, inv_mass=cases.STAT_INV_MASS, seed=seed, step=step)
            assert lp is None and ll is None
            accs.append(float(acc.double().mean()))
        moved = float((tt != start).any(dim=0).double().mean())
        stat = cases.stationarity_statistics(tt.cpu().numpy())
        print(f"seed {seed} (ε {eps}, L {n_leapfrog}): acceptance {np.mean(accs):.3f}, moved {moved:.3f}, max D_n {stat:.3e} (bar {cases.STAT_BAR:.3e})")
        assert stat < cases.STAT_BAR and np.mean(accs) >= 0.6 and moved >= 0.9, (seed, stat, accs, moved)
    pd.close()


# ---------------------------------------------------------------------------------------------------- 4. β = 1 stationarity
@pytest.mark.parametrize("seed", cases.POST_SEEDS)
def test_gpu_posterior_is_stationary(pkg, draws_mod, step_model, seed):
    import torch
    model, pd = step_model
    set_batch_invariant(pkg, model, 0)
    a, b = (model.link(pd.rejection(seed, cases.POST_N, first=first)["samples"]) for first in cases.POST_FIRST)
    im = cases.posterior_inv_mass(b)

    def step_fn(tt, step):
        t = torch.as_tensor(tt, device="cuda").contiguous()
        _lp, _ll, _dH, acc = pd.hmc_step(t, eps=cases.POST_EPS, n_leapfrog=cases.POST_LEAPFROG, inv_mass=im, seed=seed, step=step)
        return t.cpu().numpy(), acc.cpu().numpy()

    cases.check_posterior_stationary(a, b, step_fn, f"seed {seed} (device)")


# ---------------------------------------------------------------------------------------------------- 5. determinism
def run_step(torch, pd, start, beta, eps, im, seed=STEP_SEED, step=2, chain0=0, ld=None, n_leapfrog=3):
    W = start.shape[1]
    _buf, tt = padded(torch, start, ld or W)
    dev = tt.device
    lp, ll, dH, acc = pd.hmc_step(tt, beta=torch.as_tensor(beta, device=dev), eps=torch.as_tensor(eps, device=dev), n_leapfrog=n_leapfrog, inv_mass=im,
                                  seed=seed, step=step, chain0=chain0)
    return [x.cpu().numpy() for x in (tt, lp, ll, dH, acc)]


def test_gpu_determinism(pkg, draws_mod, step_model):
    import torch
    model, pd = step_model
    beta, eps, im = step_inputs()
    start = pd.sample(STEP_SEED, 0, STEP_W, theta=False, logprior_t=False)[1]
    set_batch_invariant(pkg, model, 0)
    assert same_bits(run_step(torch, pd, start, beta, eps, im), run_step(torch, pd, start, beta, eps, im))
    set_batch_invariant(pkg, model, 1)
    try:
        full = run_step(torch, pd, start, beta, eps, im)
        assert same_bits(full, run_step(torch, pd, start, beta, eps, im))
        assert same_bits(full, run_step(torch, pd, start, beta, eps, im, ld=STEP_LD))                       # another leading dimension
        part = run_step(torch, pd, start[:, 64:128].contiguous(), beta[64:128], eps[64:128], im, chain0=64)      # chains 64 … 127 alone
        assert same_bits([x[..., 64:128] for x in full], part)
        assert 0 < part[4].sum() < 64
        # the host-buffer call
        W, D = STEP_W, model.D
        th = np.ascontiguousarray(start.cpu().numpy())
        lp, ll, dH, acc = np.empty(W), np.empty(W), np.empty(W), np.empty(W, dtype=np.int32)
        dp = pkg.capi._dptr
        pd._check(pd.lib.octo_draws_hmc_step(pd._h, STEP_SEED, 2, 0, W, W, dp(th), dp(beta), dp(eps), 0.0, 3, dp(im), None, dp(lp), dp(ll), dp(dH),
                                             acc.ctypes.data_as(C.POINTER(C.c_int32))))
        assert same_bits(full, [th, lp, ll, dH, acc]) and th.shape == (D, W)
    finally:
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 6. dead states
def test_gpu_dead_states(pkg, draws_mod):
    """e ~ Uniform(0, 1.6): an orbit with e >= 1 has ℓπ = −Inf under a finite prior."""
    import torch
    model = hmc_model(pkg, e_prior=pkg.Uniform(0.0, 1.6))
    pd = draws_mod.PriorDraws(model)
    set_batch_invariant(pkg, model, 1)
    W, seed, ie = 64, 43, cases.MODEL_NAMES.index("b_e")
    clean = pd.sample(seed, 0, W, theta=False, logprior_t=False)[1]
    e_link = lambda e: math.log(e / 1.6) - math.log1p(-e / 1.6)      # noqa: E731
    clean[ie] = torch.clamp(clean[ie], max=e_link(0.9))               # every chain of the clean batch starts on a bound orbit
    nan_chain, inf_chains = 5, (9, 10, 11, 12, 13, 14, 15, 16)
    dirty = clean.clone()
    dirty[3, nan_chain] = float("nan")
    dirty[ie, list(inf_chains)] = torch.tensor([e_link(e) for e in (1.001, 1.002, 1.004, 1.008, 1.016, 1.03, 1.06, 1.2)], dtype=torch.float64, device="cuda")
    beta = np.where(np.arange(W) % 2 == 0, 0.3, 1.0)
    eps = np.full(W, 0.05)
    im = step_inputs()[2]
    lp0 = model.ℓπcallback(dirty.cpu().numpy())
    assert np.all(lp0[list(inf_chains)] == -np.inf) and not np.isfinite(lp0[nan_chain])
    tt = dirty.clone()
    lp, ll, dH, acc, prop = pd.hmc_step(tt, beta=torch.as_tensor(beta, device="cuda"), eps=torch.as_tensor(eps, device="cuda"), n_leapfrog=3, inv_mass=im,
                                        seed=seed, step=0, want_proposal=True)
    out, lp, ll, acc, prop = (x.cpu().numpy() for x in (tt, lp, ll, acc, prop))
    # the NaN chain stays NaN and is rejected
    assert acc[nan_chain] == 0 and np.array_equal(out[:, nan_chain], dirty.cpu().numpy()[:, nan_chain], equal_nan=True) and np.isnan(out[3, nan_chain])
    # a chain that starts dead is accepted exactly when its proposal is alive
    lp_prop = model.ℓπcallback(np.where(np.isfinite(prop), prop, 0.0))
    alive = np.isfinite(lp_prop) & np.all(np.isfinite(prop), axis=0)
    idx = list(inf_chains)
    print(f"dead starts: proposals alive {alive[idx].astype(int)}, accepted {acc[idx]}")
    assert np.array_equal(acc[idx].astype(bool), alive[idx])
    assert np.all(np.isfinite(lp[idx][acc[idx] == 1])) and np.all(lp[idx][acc[idx] == 0] == -np.inf) and np.all(ll[idx][acc[idx] == 0] == -np.inf)
    # every other chain of the wave is what it is without those chains
    ref_run = run_step(torch, pd, clean, beta, eps, im, seed=seed, step=0)
    got = run_step(torch, pd, dirty, beta, eps, im, seed=seed, step=0)
    others = np.setdiff1d(np.arange(W), [nan_chain] + idx)
    assert same_bits([x[..., others] for x in ref_run], [x[..., others] for x in got])
    pd.close()
    model.close()


# ---------------------------------------------------------------------------------------------------- 7. the driver
def test_gpu_octofit_pt_device(pkg, draws_mod):
    model = hmc_model(pkg)
    T, Cn, R, seed = 4, 64, 20, 7
    out = pkg.octofit_pt_device(model, T, Cn, R, seed=seed)
    D = model.D
    assert out["samples"].shape == out["samples_t"].shape == (R, D, Cn) and out["logpost"].shape == (R, Cn)
    assert out["hmc_acceptance"].shape == out["eps"].shape == (T,) and out["swap_acceptance"].shape == (T - 1,)
    assert np.all(np.isfinite(out["samples"])) and np.all(np.isfinite(out["samples_t"])) and np.all(np.isfinite(out["logpost"])) and np.all(out["eps"] > 0)
    print(f"HMC acceptance per temperature {out['hmc_acceptance']}, swap acceptance per pair {out['swap_acceptance']}, ε {out['eps']}")
    assert np.all((out["hmc_acceptance"] > 0) & (out["hmc_acceptance"] < 1)) and np.all((out["swap_acceptance"] > 0) & (out["swap_acceptance"] < 1))
    # the recorded ℓπ is the callback's at the recorded states
    lp_cb = model.ℓπcallback(out["samples_t"][-1])
    assert np.all(np.abs(lp_cb - out["logpost"][-1]) <= 1e-8 * np.maximum(1.0, np.abs(lp_cb)))
    # the replicas that sat at β = 0 in the last round hold the prior draws of their indices
    st = out["state"]
    assert st["refreshed_first"] == T * Cn + (R - 1) * Cn and st["refreshed"].shape == (Cn,)
    _, fresh = ref.prior_sample(cases.MODEL_PRIORS, seed, st["refreshed_first"] + np.arange(Cn, dtype=np.uint64))
    got = st["theta_t"][:, st["refreshed"]]
    assert np.max(np.abs(got - fresh) / np.maximum(1.0, np.abs(fresh))) <= 1e-11
    pd = draws_mod.PriorDraws(model)
    assert np.array_equal(got, pd.sample(seed, st["refreshed_first"], Cn, theta=False, logprior_t=False)[1].cpu().numpy())
    pd.close()
    # the same seed, the same output
    again = pkg.octofit_pt_device(model, T, Cn, R, seed=seed)
    for k in ("samples", "samples_t", "logpost", "hmc_acceptance", "swap_acceptance", "eps"):
        assert np.array_equal(out[k], again[k]), k
    assert np.array_equal(st["theta_t"], again["state"]["theta_t"]) and np.array_equal(st["slot2rep"], again["state"]["slot2rep"])
    model.close()


# ---------------------------------------------------------------------------------------------------- arguments
def test_gpu_hmc_argument_checks(pkg, draws_mod, step_model):
    import torch
    model, pd = step_model
    lib, EINVAL, D, W = pd.lib, pkg.capi.OCTO_EINVAL, model.D, 8
    tt = pd.sample(1, 0, W, theta=False, logprior_t=False)[1]
    acc = torch.zeros(W, dtype=torch.int32, device="cuda")
    lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda h, W_, ld, eps, L, d_eps=None, d_lp=None: lib.octo_draws_hmc_step_device(      # noqa: E731
        h, 0, 0, 0, W_, ld, tt.data_ptr(), None, d_eps, eps, L, None, None, d_lp, None, None, acc.data_ptr(), st)
    assert call(None, W, W, 0.1, 1) == EINVAL
    assert call(pd._h, W, W, 0.1, 0) == EINVAL and b"n_leapfrog" in lib.octo_draws_last_error(pd._h)
    assert call(pd._h, -1, W, 0.1, 1) == EINVAL and call(pd._h, W, W - 1, 0.1, 1) == EINVAL
    for eps in (0.0, -0.1, math.inf, math.nan):
        assert call(pd._h, W, W, eps, 1) == EINVAL
    before = tt.clone()
    assert call(pd._h, W, W, math.nan, 1, d_eps=lp.data_ptr()) == 0      # ε per chain: the scalar is not looked at (ε = 0 everywhere: nothing moves)
    assert call(pd._h, 0, 0, 0.1, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(tt, before)
    nomodel = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.MODEL_PRIORS))
    assert call(nomodel._h, W, W, 0.1, 1, d_lp=lp.data_ptr()) == EINVAL and b"no model" in lib.octo_draws_last_error(nomodel._h)
    assert call(nomodel._h, W, W, 0.1, 1) == 0
    assert lib.octo_draws_momentum_device(pd._h, 0, 0, 0, W, W - 1, None, tt.data_ptr(), st) == EINVAL
    with pytest.raises(ValueError):
        pd.hmc_step(tt.t(), eps=0.1)
    torch.cuda.synchronize()
    nomodel.close()
