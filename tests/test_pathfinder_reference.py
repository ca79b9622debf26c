"""
Conditions on the NumPy restatement of Pathfinder (tests/pathfinder_reference.py) that need no device: what the fit means (against dense BFGS
algebra, the paper's compact form, the same function in extended precision, numpy's slogdet and scipy's multivariate normal), the ELBO of an
exactly fitted Gaussian, the selection rule, frozen and dead chains and resume, the argument checks that need no handle, and the condition
the GPU comparison of tests/test_pathfinder.py rests on, from the reference alone.
"""
import functools
import math

import numpy as np
import pytest

import draws_cases as cases
import lbfgs_reference as lref
import pathfinder_reference as ref


# ---------------------------------------------------------------------------------------------------- what the fit means
@pytest.mark.parametrize("D,m", cases.PF_FIT_SHAPES)
def test_sigma_is_the_dense_inverse_bfgs_and_the_compact_form(D, m):
    """Σ of the restatement is lbfgs_reference.dense_inverse_bfgs(pairs, α, 1) and the paper's diag(α) + [αY, S]·γ·[αY, S]ᵀ: in long double
    to 1e-12 of max|Σ| (the bar and the reasoning of test_two_loop_is_the_dense_inverse_bfgs: κ·ε·m·D with κ <= 1e3 is 5e-14 at the largest
    shape), and the float64 restatement is within 1e-10 of the long-double one, so the GPU bar of 1e-8 does not hide the reference's noise."""
    cnt, head, S, Y, x, g, alpha = cases.fit_inputs(D, m)
    Lg = np.longdouble
    assert (cnt == 0).any() and (cnt == m).any() and ((D, m) != (5, 3) or 2 * cnt.max() > D)
    worst = dict(dense=0.0, compact=0.0, f64=0.0)
    for w in range(cases.PF_FIT_W):
        pl = ref.pairs_of(cnt[w], head[w], S.astype(Lg), Y.astype(Lg), w)
        fl = ref.fit_chain(pl, x[:, w].astype(Lg), g[:, w].astype(Lg), alpha[:, w].astype(Lg))
        f64 = ref.fit_chain(ref.pairs_of(cnt[w], head[w], S, Y, w), x[:, w], g[:, w], alpha[:, w])
        assert fl["ok"] and f64["ok"] and fl["H"].dtype == Lg
        sl = ref.sigma(fl)
        scale = float(np.max(np.abs(sl)))
        worst["dense"] = max(worst["dense"], float(np.max(np.abs(sl - lref.dense_inverse_bfgs(pl, alpha[:, w].astype(Lg), Lg(1))))) / scale)
        worst["compact"] = max(worst["compact"], float(np.max(np.abs(sl - ref.compact_sigma(pl, alpha[:, w].astype(Lg))))) / scale)
        worst["f64"] = max(worst["f64"], float(np.max(np.abs(ref.sigma(f64) - sl))) / scale)
        if cnt[w] == 0:
            assert np.allclose(ref.sigma(f64), np.diag(alpha[:, w]), rtol=4e-16, atol=0)      # no pair: Σ = diag(α), (√α)² rounded
    print(f"D {D} m {m}: Σ against dense BFGS {worst['dense']:.3e}, against the compact form {worst['compact']:.3e} (long double), float64 against long double {worst['f64']:.3e}")
    assert worst["dense"] <= 1e-12 and worst["compact"] <= 1e-12 and worst["f64"] <= 1e-10


@pytest.mark.parametrize("D,m", cases.PF_FIT_SHAPES)
def test_square_root_mean_and_logdet(D, m):
    """T = diag(√α)·L̃ is a square root of Σ, μ = x − Σ·g, logdet is numpy's slogdet of Σ: float64 against float64 at 1e-10 of the scale,
    the bar the float64 restatement keeps against long double above."""
    cnt, head, S, Y, x, g, alpha = cases.fit_inputs(D, m)
    worst = dict(tt=0.0, mu=0.0, logdet=0.0)
    for w in range(cases.PF_FIT_W):
        f = ref.fit_chain(ref.pairs_of(cnt[w], head[w], S, Y, w), x[:, w], g[:, w], alpha[:, w])
        sg = ref.sigma(f)
        T = f["sqa"][:, None] * f["L"]
        assert np.array_equal(np.triu(f["L"], 1), np.zeros((D, D))) and np.all(np.diag(f["L"]) > 0)
        worst["tt"] = max(worst["tt"], np.max(np.abs(T @ T.T - sg)) / np.max(np.abs(sg)))
        want = x[:, w] - sg @ g[:, w]
        worst["mu"] = max(worst["mu"], np.max(np.abs(f["mu"] - want)) / max(1.0, np.max(np.abs(want))))
        sign, ld = np.linalg.slogdet(sg)
        assert sign == 1.0
        worst["logdet"] = max(worst["logdet"], abs(f["logdet"] - ld) / max(1.0, abs(ld)))
        assert np.array_equal(ref.unpack(ref.pack(f["L"]), D), f["L"])
    print(f"D {D} m {m}: T·Tᵀ − Σ {worst['tt']:.3e}, μ {worst['mu']:.3e}, logdet {worst['logdet']:.3e}")
    assert max(worst.values()) <= 1e-10


def test_log_q_against_scipy():
    from scipy.stats import multivariate_normal
    D, m = 5, 3
    cnt, head, S, Y, x, g, alpha = cases.fit_inputs(D, m)
    worst = 0.0
    for w in range(cases.PF_FIT_W):
        f = ref.fit_chain(ref.pairs_of(cnt[w], head[w], S, Y, w), x[:, w], g[:, w], alpha[:, w])
        z = ref.final_normals(cases.PF_SEED, cases.PF_CHAIN0 + w, D, 7)
        phi, logq = ref.draw_map(f["mu"], f["sqa"], f["L"], f["logdet"], z)
        want = multivariate_normal(mean=f["mu"], cov=ref.sigma(f)).logpdf(phi.T)
        worst = max(worst, np.max(np.abs(logq - want) / np.maximum(1.0, np.abs(want))))
    print(f"log q against scipy's multivariate normal: {worst:.3e}")
    assert worst <= 1e-10


def test_normals_are_the_momentum_map_on_their_own_streams():
    """purpose 4 at t = iters·32 + k and purpose 5 at t = j: the u -> z map of the momentum kernel with inv_mass = 1, other words than purpose 2's"""
    import hmc_reference as href
    D = 6
    z = ref.elbo_normals(cases.PF_SEED, cases.PF_CHAIN0 + 3, D, iters=2, K=4)
    assert z.shape == (D, 4) and np.array_equal(z[:, 1], ref.normals(cases.PF_SEED, cases.PF_CHAIN0 + 3, D, 4, [2 * 32 + 1])[:, 0])
    assert not np.array_equal(z[:, 1], href.momentum(cases.PF_SEED, 2 * 32 + 1, cases.PF_CHAIN0 + 3, 1, D)[:, 0])
    f = ref.final_normals(cases.PF_SEED, cases.PF_CHAIN0 + 3, D, 3)
    assert np.array_equal(f[:, 2], ref.normals(cases.PF_SEED, cases.PF_CHAIN0 + 3, D, 5, [2])[:, 0]) and not np.array_equal(f[:, :3], z[:, :3])
    assert abs(np.mean(ref.final_normals(cases.PF_SEED, 0, 4, 20000))) < 0.02


def test_elbo_of_an_exactly_fitted_gaussian_is_the_log_normaliser():
    """With D A-conjugate steps on a quadratic the inverse-BFGS matrix is A⁻¹ whatever α, μ is the mode, and ℓπ(φ) − log q(φ) is the log of
    the normaliser at EVERY z: the ELBO has no variance."""
    rng = np.random.default_rng(11)
    D = 4
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    A = (Q * np.array([0.5, 1.0, 3.0, 8.0])) @ Q.T
    a, c0 = rng.normal(size=D), -3.25
    steps = []
    for v in rng.normal(size=(D, D)):
        for s in steps:
            v = v - (s @ A @ v) / (s @ A @ s) * s
        steps.append(v)
    x = rng.normal(size=D)
    alpha = np.exp(rng.uniform(-2, 2, D))
    f = ref.fit_chain([(s, A @ s) for s in steps], x, A @ (x - a), alpha)
    assert f["ok"] and np.allclose(ref.sigma(f), np.linalg.inv(A), rtol=0, atol=1e-12) and np.allclose(f["mu"], a, rtol=0, atol=1e-12)
    log_Z = c0 + 0.5 * D * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(A)[1]
    for seed in (1, 2):
        z = ref.elbo_normals(seed, 5, D, 3, 32)
        phi, logq = ref.draw_map(f["mu"], f["sqa"], f["L"], f["logdet"], z)
        lp = c0 - 0.5 * np.einsum("dk,de,ek->k", phi - a[:, None], A, phi - a[:, None])
        assert np.max(np.abs(lp - logq - log_Z)) <= 1e-11, np.max(np.abs(lp - logq - log_Z))


# ---------------------------------------------------------------------------------------------------- selection, frozen and dead chains, resume
def quartic(th):
    """a cheap non-Gaussian target: ℓπ = −½ Σ θ²/σ² − 0.05 Σ θ⁴"""
    s2 = np.array([0.25, 1.0, 9.0])[:, None]
    return -0.5 * np.sum(th * th / s2, axis=0) - 0.05 * np.sum(th ** 4, axis=0), -th / s2 - 0.2 * th ** 3


def quartic_starts():
    x = np.random.default_rng(3).normal(size=(3, 7)) * 3.0
    x[1, 4] = np.nan
    return x


OUT = ("theta_t", "logpost", "gnorm", "status", "iters", "evals", "inv_hess_diag", "elbo", "elbo_iter", "n_fits")


def test_selection_keeps_the_greatest_elbo_and_the_earliest_of_a_tie():
    r = ref.pathfinder(quartic, quartic_starts(), m=4, n_rounds=12, gtol=1e-9, seed=cases.PF_SEED, chain0=cases.PF_CHAIN0, n_elbo=cases.PF_N_ELBO)
    ps = r["state"]
    live = np.arange(7) != 4
    assert np.all(r["n_fits"][live] == r["iters"][live]) and r["iters"][live].min() >= 3
    for w in np.nonzero(live)[0]:
        its, es = zip(*ps.history[w])
        assert list(its) == list(range(1, r["iters"][w] + 1))                  # every accepted iterate, the opening point not
        assert r["elbo"][w] == max(es) and r["elbo_iter"][w] == its[int(np.argmax(es))]
    # the rule itself: strict comparison — a tie leaves the earlier fit, −Inf and NaN never win
    ps2 = ref.State(ps.lb)
    for e, it in ((-np.inf, 1), (np.nan, 2), (-5.0, 3), (-5.0, 4), (-7.0, 5), (-4.0, 6), (-4.0, 7)):
        if e > ps2.elbo[0]:
            ps2.elbo[0], ps2.elbo_iter[0] = e, it
        assert ps2.elbo_iter[0] == {1: -1, 2: -1, 3: 3, 4: 3, 5: 3, 6: 6, 7: 6}[it]
    # a target that is −Inf wherever a draw lands: candidates are counted, none is kept
    blind = lambda th: quartic(th) if th.shape[1] == 7 else (np.full(th.shape[1], -np.inf), np.zeros_like(th))      # noqa: E731
    rb = ref.pathfinder(blind, quartic_starts(), m=4, n_rounds=6, gtol=1e-9, seed=cases.PF_SEED, chain0=cases.PF_CHAIN0, n_elbo=cases.PF_N_ELBO)
    assert np.all(rb["elbo"] == -np.inf) and np.all(rb["elbo_iter"] == -1) and np.all(rb["n_fits"][live] > 0)


def test_dead_and_frozen_chains_and_resume_in_the_restatement():
    x0 = quartic_starts()
    kw = dict(m=4, gtol=1e-5, seed=cases.PF_SEED, chain0=cases.PF_CHAIN0, n_elbo=cases.PF_N_ELBO)
    one = ref.pathfinder(quartic, x0, n_rounds=30, **kw)
    assert one["status"][4] == lref.DEAD and one["elbo"][4] == -np.inf and one["elbo_iter"][4] == -1 and one["n_fits"][4] == 0
    assert np.array_equal(one["theta_t"][:, 4], x0[:, 4], equal_nan=True)
    half = ref.pathfinder(quartic, x0, n_rounds=11, **kw)
    two = ref.pathfinder(quartic, None, n_rounds=19, state=half["state"], **kw)
    for k in OUT:
        assert np.array_equal(one[k], two[k], equal_nan=True), k
    frozen = one["status"] == lref.GTOL
    assert frozen.sum() >= 3
    more = ref.pathfinder(quartic, None, n_rounds=5, state=one["state"], **kw)
    for k in OUT:
        assert np.array_equal(one[k][..., frozen], more[k][..., frozen]), k
    assert np.all(one["elbo_iter"][frozen] >= 1) and np.all(one["elbo_iter"][frozen] <= one["iters"][frozen])
    # the first n_elbo = 3 draws are the first three of n_elbo = 5: the candidates' counters do not depend on K
    assert np.array_equal(ref.elbo_normals(cases.PF_SEED, 9, 3, 4, 3), ref.elbo_normals(cases.PF_SEED, 9, 3, 4, 5)[:, :3])
    phi, logq, lp = ref.pathfinder_draw(quartic, one["state"], cases.PF_SEED, cases.PF_CHAIN0, 4)
    cols = np.arange(4) * 7 + 4
    assert np.all(np.isnan(logq[cols])) and np.all(lp[cols] == -np.inf) and np.array_equal(phi[:, cols], np.repeat(x0[:, 4:5], 4, axis=1), equal_nan=True)
    others = np.setdiff1d(np.arange(28), cols)
    assert np.all(np.isfinite(logq[others])) and np.all(np.isfinite(lp[others]))


# ---------------------------------------------------------------------------------------------------- argument checks without a device
def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made, so these go through the NULL handle, which is refused before anything else; the same
    arguments on a real handle are in tests/test_pathfinder.py. octo_draws_create admits D <= 64 = OCTO_DRAWS_PF_MAX_D, so no handle can
    carry the D = 65 that OCTO_ENOTSUP is for."""
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    build_draws()
    from octofitter_jl_amd.host import draws
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_pathfinder_fit_device(None, 4, 4, 2, *[None] * 11, 0, None, None, None) == EINVAL
    assert lib.octo_draws_pathfinder_device(None, 1, 0, 4, 4, None, None, 6, 1, 1e-6, 0.0, 5, 0, *[None] * 10) == EINVAL
    assert lib.octo_draws_pathfinder_draw_device(None, 1, 0, 4, 4, None, 8, 32, None, None, None, None) == EINVAL
    assert (draws.PF_MAX_D, draws.PF_MAX_ELBO_DRAWS) == (ref.MAX_D, ref.MAX_ELBO_DRAWS) == (64, 32)
    assert (draws.PURPOSE_ELBO, draws.PURPOSE_PATHFINDER) == (ref.PURPOSE_ELBO, ref.PURPOSE_PATHFINDER) == (4, 5)


# ---------------------------------------------------------------------------------------------------- the condition of the GPU comparison
@functools.lru_cache(maxsize=None)
def reference_rounds(oracle):
    """the restatement's cases.PF_ROUNDS rounds from the 64 starts of cases.reference_case, fed by the oracle — computed once, shared, never modified"""
    starts, _, v, _ = cases.reference_case(oracle)
    return ref.pathfinder(cases.tight_logpost(oracle), starts, v, m=cases.LBFGS_M, n_rounds=cases.PF_ROUNDS, gtol=cases.LBFGS_GRAD_TOL, seed=cases.PF_SEED, chain0=cases.PF_CHAIN0, n_elbo=cases.PF_N_ELBO)


def test_ten_rounds_are_decided_for_most_starts(oracle):
    """tests/test_pathfinder.py compares elbo_iter, n_fits and the ELBO on chains that have a fit and whose two best ELBOs differ by more
    than cases.PF_MARGIN·max(1, |ELBO|), and may leave out at most 1/8 of the 64. With K = 5 draws the ELBOs of neighbouring iterates differ at
    order one, so the reference clears this by far."""
    r = reference_rounds(oracle)
    decided = cases.decided_chains(r)
    gaps = r["margin_elbo"][r["elbo_iter"] >= 0]
    print(f"{decided.sum()} of {cases.LBFGS_N_STARTS} chains decided after {cases.PF_ROUNDS} rounds; fits a chain {r['n_fits'].min()} … {r['n_fits'].max()}; the smallest gap between the "
          f"two best ELBOs {gaps.min():.3e}; best ELBO {r['elbo'].max():.6f}; kept iterates {np.bincount(r['elbo_iter'][r['elbo_iter'] >= 0])}")
    assert decided.sum() >= 7 * cases.LBFGS_N_STARTS // 8
    assert r["n_fits"].max() >= 3 and np.all(r["status"] != lref.DEAD)
