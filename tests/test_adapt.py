"""
The warm-up statistics on the device (include/octofitter_hip_draws.h: octo_draws_moments_device, octo_draws_metric_device,
octo_draws_hmc_adapt_init_device, octo_draws_hmc_adapt_device, octo_draws_chain_moments_device; host/draws.py: PriorDraws.moments / metric /
adapt_init / adapt_step / chain_moments; host/callers.py: hmc_warmup, octofit_hmc_device, octofit_pt_device(adapt="device")) against exact
arithmetic and the NumPy restatement (tests/adapt_reference.py), on the inputs, bars and seeds of tests/draws_cases.py that
tests/test_adapt_reference.py establishes on the CPU.

Tolerances: the moments' three bars of tests/draws_cases.py; metric 1e-14 relative (arithmetic only); dual-averaging state, acceptance statistic and ε
the project's device-transcendental bar 1e-11 relative to max(1, |ref|); per-chain moments 1e-12 relative; R̂ 1e-10 relative; the free-running
warm-up max(1e-8, 100·s) with the s measured there; Kolmogorov-Smirnov at the 0.1 % level.
"""
import ctypes as C
import math

import numpy as np
import pytest

import adapt_reference as ref
import draws_cases as cases
from draws_device import TRANS_BAR, close, dev, draws_mod, hmc_model, host, mirror_priors, padded_view, set_batch_invariant      # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pd(pkg, draws_mod):
    """a handle without a model on the five priors of the stationarity condition"""
    h = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.STAT_PRIORS))
    yield h
    h.close()


# ---------------------------------------------------------------------------------------------------- 1. moments against the exact reference
@pytest.mark.parametrize("G", cases.MOMENT_G)
@pytest.mark.parametrize("K", cases.MOMENT_K)
def test_gpu_moments_against_exact_arithmetic(pd, K, G):
    import torch
    worst = (0.0, 0.0)
    for W in cases.MOMENT_W:
        x, group = cases.moments_case(W, K, G)
        exact = ref.exact_moments(x, group, G)
        g = None if group is None else dev(group)
        view = padded_view(x)
        got = host(pd.moments(view, g, G))
        w = cases.check_moments(got, exact, (W, K, G))
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
        if G > 1:
            assert got[0][G - 1] == 0 and np.all(got[1][G - 1] == 0) and np.all(got[2][G - 1] == 0)      # the empty group on overwrite
        # the same bits: the call again, another leading dimension with other values beyond column W, other values in excluded chains
        assert all(np.array_equal(a, b) for a, b in zip(got, host(pd.moments(view, g, G))))
        assert all(np.array_equal(a, b) for a, b in zip(got, host(pd.moments(padded_view(x, 64, float("inf")), g, G))))
        if W >= 63:
            x2 = x.copy()
            x2[:K - 1, 5] = 123.0                  # the chain with the NaN in its last row
            x2[:K - 1, 7] = -4.5e6
            if G > 1:
                x2[:, 2], x2[:, 3] = 1e300, -7.0   # the chains with ids −1 and G
            assert all(np.array_equal(a, b) for a, b in zip(got, host(pd.moments(padded_view(x2), g, G))))
        # accumulate: three calls on thirds of the chains against one call on all of them
        out = None
        for k, (a, b) in enumerate(cases.thirds(W)):
            out = pd.moments(view[:, a:b], None if g is None else g[a:b].contiguous(), G, out=out, accumulate=k > 0)
        torch.cuda.synchronize()
        cases.check_moments(host(out), exact, (W, K, G, "thirds"))
    print(f"K {K} G {G}: worst mean error / bar {worst[0]:.3f}, worst M2 relative error {worst[1]:.3e}")


# ---------------------------------------------------------------------------------------------------- 2. metric
def test_gpu_metric(pd):
    import torch
    x, group = cases.moments_case(257, 11, 3)
    cnt, mean, m2 = pd.moments(padded_view(x), dev(group), 3)
    hc, _, hm2 = host((cnt, mean, m2))
    assert hc[1] == 1 and hc[2] == 0
    for reg in (True, False):
        for g in range(3):
            im = torch.full((11,), float("nan"), dtype=torch.float64, device="cuda")
            got = pd.metric(cnt[g:g + 1], mean[g], m2[g], im, regularize=reg).cpu().numpy()
            want = ref.metric(hc[g], hm2[g], np.full(11, np.nan), regularize=reg)
            assert close(got, want, 1e-14, scale_one=False), (reg, g)
            assert np.all(np.isnan(got)) == (g > 0)          # the single-member and the empty group leave every entry untouched
    # n >= 2 with M2 = 0, NaN or Inf: the plain variance is not finite and > 0 there
    c10, m2x = dev(np.array([10.0])), dev(np.array([4.0, 0.0, np.nan, np.inf, 9.0e-4]))
    for reg in (True, False):
        im = torch.full((5,), float("nan"), dtype=torch.float64, device="cuda")
        got = pd.metric(c10, m2x, m2x, im, regularize=reg).cpu().numpy()
        assert close(got, ref.metric(10.0, m2x.cpu().numpy(), np.full(5, np.nan), regularize=reg), 1e-14, scale_one=False)
        assert np.isnan(got[2]) and np.isnan(got[3]) and np.isnan(got[1]) == (not reg)


# ---------------------------------------------------------------------------------------------------- 3. dual averaging
@pytest.mark.parametrize("G", (1, 8))
def test_gpu_dual_averaging(pd, G):
    import torch
    dH0, acc, group = cases.dual_averaging_case(G)
    W = dH0.size
    eps0 = 0.1 if G == 1 else 0.05 * (1 + np.arange(G))
    state = pd.adapt_init(G, eps0 if G == 1 else dev(eps0))
    want = ref.adapt_init(eps0, G)
    assert close(state.cpu().numpy(), want, TRANS_BAR)
    want = state.cpu().numpy()                      # teacher-forced from the device's own start
    first = want.copy()
    g, acc_t = None if group is None else dev(group), dev(acc)
    eps_w = torch.full((W,), -7.0, dtype=torch.float64, device="cuda")
    for k in range(1, 13):
        dH = dH0 + 0.1 * (k - 6)                    # ±Inf and NaN stay what they are
        avg = k % 2 == 0
        a, e = pd.adapt_step(state, dev(dH), acc_t, k, group=g, use_average=avg, eps_w=eps_w)
        want, a_ref = ref.adapt_step(want, dH, acc, k, group)
        assert e is eps_w
        assert close(a.cpu().numpy(), a_ref, TRANS_BAR), (k, a.cpu().numpy(), a_ref)
        assert close(state.cpu().numpy(), want, TRANS_BAR), k
        assert close(eps_w.cpu().numpy(), ref.eps_of(want, group, W, avg, held=np.full(W, -7.0)), TRANS_BAR), k
    got = state.cpu().numpy()
    if G > 1:
        assert np.array_equal(got[G - 2], first[G - 2]) and math.isnan(float(a[G - 2]))      # the empty group: its state bit for bit
        assert eps_w[9] == -7.0 and eps_w[200] == -7.0                                        # excluded chains are not written
    assert np.all(np.isfinite(got)) and not np.array_equal(got[0], first[0])


def test_gpu_argument_checks(pkg, pd):
    import torch
    lib, h, EINVAL = pd.lib, pd._h, pkg.capi.OCTO_EINVAL
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    W, K = 8, 3
    x = torch.zeros((K, W), dtype=torch.float64, device="cuda")
    grp = torch.zeros(W, dtype=torch.int32, device="cuda")
    out = [torch.zeros(4 * 64, dtype=torch.float64, device="cuda") for _ in range(3)]
    X, Gp, (c, m, s) = x.data_ptr(), grp.data_ptr(), [t.data_ptr() for t in out]

    def mom(W_=W, ld=W, K_=K, x_=X, g=Gp, G=2, c_=c, m_=m, s_=s):
        return lib.octo_draws_moments_device(h, W_, ld, K_, x_, g, G, 0, c_, m_, s_, st)
    assert mom() == 0 and mom(W_=0) == 0 and mom(g=None, G=1) == 0
    assert all(r == EINVAL for r in (mom(x_=None), mom(c_=None), mom(m_=None), mom(s_=None), mom(K_=0), mom(K_=65), mom(G=0), mom(G=65), mom(g=None, G=2),
                                     mom(W_=-1), mom(ld=W - 1), mom(W_=(1 << 24) + 1, ld=(1 << 24) + 1)))
    assert b"2^24" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_metric_device(h, K, c, m, s, 1, X, st) == 0
    assert all(lib.octo_draws_metric_device(h, k_, a, b, d, 1, e, st) == EINVAL
               for k_, a, b, d, e in ((0, c, m, s, X), (65, c, m, s, X), (K, None, m, s, X), (K, c, None, s, X), (K, c, m, None, X), (K, c, m, s, None)))
    assert lib.octo_draws_hmc_adapt_init_device(h, 2, None, 0.1, c, st) == 0
    assert all(lib.octo_draws_hmc_adapt_init_device(h, G, None, e, p, st) == EINVAL
               for G, e, p in ((0, 0.1, c), (65, 0.1, c), (2, 0.1, None), (2, 0.0, c), (2, -1.0, c), (2, math.inf, c), (2, math.nan, c)))
    acc = torch.zeros(W, dtype=torch.int32, device="cuda")
    A = acc.data_ptr()

    def da(W_=W, g=Gp, G=2, dH=X, a=A, k=1, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, state=c):
        return lib.octo_draws_hmc_adapt_device(h, W_, g, G, dH, a, k, delta, gamma, t0, kappa, state, None, 0, None, st)
    assert da() == 0 and da(W_=0) == 0 and da(t0=0.0) == 0 and da(g=None, G=1) == 0
    bad = [da(k=0), da(k=-3), da(dH=None), da(a=None), da(state=None), da(G=0), da(G=65), da(g=None, G=2), da(W_=-1), da(W_=(1 << 24) + 1)]
    bad += [da(delta=v) for v in (0.0, 1.0, -0.1, math.nan, math.inf)] + [da(gamma=v) for v in (0.0, -1.0, math.nan, math.inf)]
    bad += [da(t0=v) for v in (-1.0, math.nan, math.inf)] + [da(kappa=v) for v in (0.0, -0.5, math.nan, math.inf)]
    assert all(r == EINVAL for r in bad), bad

    def cm(W_=W, ld=W, K_=K, k=1, x_=X, a=m, b=s):
        return lib.octo_draws_chain_moments_device(h, W_, ld, K_, k, x_, a, b, st)
    assert cm() == 0 and cm(W_=0) == 0
    assert all(r == EINVAL for r in (cm(k=0), cm(x_=None), cm(a=None), cm(b=None), cm(K_=0), cm(K_=65), cm(W_=-1), cm(ld=W - 1), cm(W_=(1 << 24) + 1, ld=(1 << 24) + 1)))
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        pd.moments(x, accumulate=True)


# ---------------------------------------------------------------------------------------------------- 4. per-chain moments and R̂
def test_gpu_chain_moments_and_rhat(pd):
    import torch
    from octofitter_jl_amd.host import callers
    s = cases.rhat_case()
    n, K, W = s.shape
    cmean, cm2 = padded_view(np.zeros((K, W))), padded_view(np.zeros((K, W)))      # NaN everywhere beyond column W, and k = 1 ignores what they hold
    cmean[:] = float("nan")
    rmean = rm2 = None
    for k in range(1, n + 1):
        pd.chain_moments(padded_view(s[k - 1]), k, cmean, cm2)
        rmean, rm2 = ref.chain_moments(s[k - 1], k, rmean, rm2)
        assert close(cmean.cpu().numpy(), rmean, 1e-12, scale_one=False) and close(cm2.cpu().numpy(), rm2, 1e-12, scale_one=False), k
    got = cmean.cpu().numpy()
    assert np.isnan(got[3, 100]) and np.isnan(cm2.cpu().numpy()[3, 100]) and np.isfinite(np.delete(got, 100, axis=1)).all()
    r = callers.rhat_from_chain_moments(pd, cmean, cm2, n).cpu().numpy()
    direct = ref.rhat_direct(s)
    print(f"R̂ {r.min():.4f} … {r.max():.4f}; against the direct formula {np.max(np.abs(r - direct) / direct):.3e}")
    assert np.all(np.abs(r - direct) <= 1e-10 * direct)
    with pytest.raises(ValueError):
        pd.chain_moments(padded_view(s[0]), 1, cmean, torch.zeros((K, W), dtype=torch.float64, device="cuda"))      # another leading dimension


# ---------------------------------------------------------------------------------------------------- 5. the warm-up loop on the prior
@pytest.fixture(scope="module")
def loop(pkg, pd):
    """pkg.hmc_warmup on the handle without a model, every round recorded, and the restatement's own run from the device's start"""
    import torch
    start = pd.sample(cases.LOOP_SEED, 0, cases.LOOP_W, theta=False, logprior_t=False)[1]
    record = []
    out = pkg.hmc_warmup(pd, start.clone(), cases.LOOP_WARMUP, n_leapfrog=cases.LOOP_LEAPFROG, eps=cases.LOOP_EPS, seed=cases.LOOP_SEED, record=record)
    torch.cuda.synchronize()
    own = ref.hmc_warmup(cases.STAT_PRIORS, start.cpu().numpy(), cases.LOOP_WARMUP, cases.LOOP_LEAPFROG, cases.LOOP_EPS, np.ones(5), cases.LOOP_SEED)
    return out, record, own


def test_gpu_warmup_teacher_forced(loop):
    """every round's adapt and moments outputs against the restatement applied to the DEVICE's inputs of that round"""
    out, record, _ = loop
    flags = ref.round_flags(cases.LOOP_WARMUP)
    assert len(record) == cases.LOOP_WARMUP and out["step"] == cases.LOOP_WARMUP
    k, windows = 0, 0
    for r, rec in enumerate(record):
        k += 1
        assert (rec["in_window"], rec["first"], rec["last"]) == flags[r] and rec["k"] == k and rec["use_average"] == (r == cases.LOOP_WARMUP - 1)
        state, a = ref.adapt_step(rec["state_in"].cpu().numpy(), rec["dH"].cpu().numpy(), rec["accepted"].cpu().numpy(), k)
        assert close(rec["state"].cpu().numpy(), state, TRANS_BAR) and close(rec["accept_stat"].cpu().numpy(), a, TRANS_BAR), r
        assert close(rec["eps_w"].cpu().numpy(), np.full(cases.LOOP_W, math.exp(state[0, 1 if rec["use_average"] else 0])), TRANS_BAR), r
        assert close(out["accept_stat"][r].cpu().numpy(), a[0], TRANS_BAR)
        if rec["in_window"]:
            tt = rec["theta_t"].cpu().numpy()
            got = host(rec["mom"])
            if rec["first"]:
                cases.check_moments(got, ref.exact_moments(tt), ("round", r))
            else:                     # the merge: the restatement's Chan step on what the device held, at the same bars
                cnt, mean, m2 = ref.moments(tt, held=host(rec["mom_in"]))
                amax = np.maximum(np.max(np.abs(tt), axis=1), np.abs(mean[0]))
                assert np.array_equal(got[0], cnt) and np.all(np.abs(got[1] - mean) <= cnt[0] * cases.U * amax) and np.all(np.abs(got[2] - m2) <= cases.M2_BAR * m2), r
        if rec["last"]:
            windows += 1
            hm = host(rec["mom"])
            assert close(rec["inv_mass"].cpu().numpy(), ref.metric(hm[0][0], hm[2][0], rec["inv_mass_in"].cpu().numpy(), regularize=True), 1e-14, scale_one=False)
            assert close(rec["state_restart"].cpu().numpy(), ref.adapt_init(np.exp(rec["state"].cpu().numpy()[:, 1])), TRANS_BAR)
            k = 0
    assert windows == 1 and close(out["eps"].cpu().numpy(), record[-1]["eps_w"][:1].cpu().numpy(), 0.0)


def test_gpu_warmup_free_running(loop):
    """ε, inv_mass and the final θ_t against the restatement's own run at max(1e-8, 100·s); every acceptance flag equal"""
    out, record, own = loop
    got = dict(eps=out["eps"].cpu().numpy()[0], inv_mass=out["inv_mass"].cpu().numpy(), theta_t=out["theta_t"].cpu().numpy())
    dev_acc = np.array([rec["accepted"].cpu().numpy() != 0 for rec in record])
    d = cases.loop_deviation(got, own)
    print(f"free-running warm-up: deviation {d:.3e} (bar {cases.LOOP_BAR:.3e}); ε {got['eps']:.6f} (restatement {own['eps']:.6f}); flags differing {np.sum(dev_acc != own['accepted'])}")
    assert np.array_equal(dev_acc, own["accepted"])
    assert d <= cases.LOOP_BAR
    assert not np.allclose(got["inv_mass"], 1.0)


@pytest.mark.parametrize("seed", cases.FROZEN_SEEDS)
def test_gpu_frozen_kernel_is_stationary(pkg, pd, seed):
    """(ε, inv_mass) of a warm-up on chains 0 … 4095, then a fresh batch of 65 536 exact prior draws through six steps"""
    start = pd.sample(seed, 0, cases.FROZEN_WARM_W, theta=False, logprior_t=False)[1]
    wu = pkg.hmc_warmup(pd, start, cases.LOOP_WARMUP, n_leapfrog=cases.LOOP_LEAPFROG, eps=cases.LOOP_EPS, seed=seed)
    eps, im = float(wu["eps"][0]), wu["inv_mass"]
    fresh = pd.sample(seed, cases.FROZEN_WARM_W, cases.FROZEN_W, theta=False, logprior_t=False)[1]

    accs = []
    for j in range(cases.FROZEN_STEPS):
        _, _, _, a = pd.hmc_step(fresh, eps=eps, n_leapfrog=cases.LOOP_LEAPFROG, inv_mass=im, seed=seed, step=cases.LOOP_WARMUP + j, chain0=cases.FROZEN_WARM_W)
        accs.append(float(a.double().mean()))
    acc = float(np.mean(accs))
    stat = cases.stationarity_statistics(fresh.cpu().numpy())
    wu_ref, (stat_ref, acc_ref) = cases.frozen_reference(seed)
    print(f"seed {seed}: device ε {eps:.5f} (restatement {wu_ref['eps']:.5f}); max D_n {stat:.3e} (restatement {stat_ref:.3e}, bar {cases.STAT_BAR:.3e}); "
          f"acceptance {acc:.4f} (restatement {acc_ref:.4f})")
    assert stat < cases.STAT_BAR
    assert abs(acc - acc_ref) <= 3 * 0.5 / math.sqrt(cases.FROZEN_STEPS * cases.FROZEN_W)      # the binomial bound


# ---------------------------------------------------------------------------------------------------- 6. the drivers
@pytest.fixture(scope="module")
def model(pkg):
    m = hmc_model(pkg)
    set_batch_invariant(pkg, m, 1)
    yield m
    m.close()


def test_gpu_octofit_hmc_device(pkg, draws_mod, model):
    Cn, nw, ns, seed, D = 256, 40, 20, 61, model.D
    h = draws_mod.PriorDraws(model)
    init = h.sample(seed, 0, Cn, theta=False, logprior_t=False)[1].cpu().numpy()
    prior_var = h.sample(seed, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).cpu().numpy()
    h.close()
    kw = dict(n_chains=Cn, n_warmup=nw, n_samples=ns, n_leapfrog=3, init=init, seed=seed)
    out = pkg.octofit_hmc_device(model, **kw)
    assert out["samples"].shape == out["samples_t"].shape == (ns, D, Cn) and out["logpost"].shape == (ns, Cn) and out["accept_stat"].shape == (nw + ns,)
    assert out["inv_mass"].shape == out["rhat"].shape == (D,) and out["names"] == list(model.names) and out["state"]["theta_t"].shape == (D, Cn)
    assert out["state"]["step"] == nw + ns and np.array_equal(out["state"]["theta_t"], out["samples_t"][-1])
    assert all(np.all(np.isfinite(out[k])) for k in ("samples", "samples_t", "logpost", "accept_stat", "inv_mass", "rhat"))
    assert math.isfinite(out["eps"]) and out["eps"] > 0 and np.all(out["inv_mass"] > 0)
    assert not np.any(out["inv_mass"] == prior_var)
    again = pkg.octofit_hmc_device(model, **kw)
    assert all(np.array_equal(out[k], again[k]) for k in out if isinstance(out[k], np.ndarray)) and out["eps"] == again["eps"]
    direct = ref.rhat_direct(out["samples_t"])
    print(f"octofit_hmc_device: ε {out['eps']:.4f}, acceptance statistic of the sampling rounds {out['accept_stat'][nw:].mean():.3f}, R̂ {out['rhat'].min():.3f} … "
          f"{out['rhat'].max():.3f}; against the direct formula {np.max(np.abs(out['rhat'] - direct) / direct):.3e}")
    assert np.all(np.abs(out["rhat"] - direct) <= 1e-10 * direct)
    short = pkg.octofit_hmc_device(model, n_chains=Cn, n_warmup=10, n_samples=5, n_leapfrog=3, seed=seed)      # init=None: Pathfinder's draws
    assert short["samples"].shape == (5, D, Cn) and np.all(np.isfinite(short["logpost"])) and short["eps"] > 0 and np.all(np.isfinite(short["rhat"]))
    with pytest.raises(ValueError):
        pkg.octofit_hmc_device(model, n_chains=Cn, init=init[:, :5])


def test_gpu_octofit_pt_device_adapts_on_the_device(pkg, draws_mod, model):
    import torch
    T, Cn, seed = 4, 64, 23
    out = pkg.octofit_pt_device(model, T, Cn, 12, seed=seed, adapt="device")
    assert out["samples"].shape == (12, model.D, Cn) and np.all(np.isfinite(out["eps"])) and np.all(out["eps"] > 0) and not np.allclose(out["eps"], 0.1)
    assert np.all(np.isfinite(out["logpost"]))
    # one round by hand: the ladder starts in order (walker r·n_chains + c in slot r), the metric and the starts are the driver's defaults
    one = pkg.octofit_pt_device(model, T, Cn, 1, seed=seed, n_adapt=1, adapt="device")
    h = draws_mod.PriorDraws(model)
    im = h.sample(seed, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1)
    theta_t = h.sample(seed, 0, T * Cn, theta=False, logprior_t=False)[1]
    slot = torch.arange(T, device="cuda").repeat_interleave(Cn)
    beta = dev(one["betas"])[slot]
    state = h.adapt_init(T, 0.1)
    _, _, dH, acc = h.hmc_step(theta_t, beta=beta, eps=torch.exp(state[:, 0])[slot], n_leapfrog=4, inv_mass=im, seed=seed, step=0)
    h.adapt_step(state, dH, acc, 1, group=slot.int(), want_eps=False)
    by_hand = torch.exp(state[:, 1]).cpu().numpy()
    h.close()
    assert np.array_equal(one["eps"], by_hand), (one["eps"], by_hand)
    with pytest.raises(ValueError):
        pkg.octofit_pt_device(model, T, Cn, 1, adapt="both")
