"""
Conditions on the NumPy restatement of the batched L-BFGS (tests/lbfgs_reference.py) that need no device: what the two-loop recursion and
the Pathfinder diagonal mean (against dense BFGS algebra, and against the same recursion in extended precision), the optimiser against
scipy's L-BFGS-B on the oracle's callback, and the conditions the GPU tests of tests/test_lbfgs.py rest on, from the reference alone.

The model is the one of tests/test_hmc_reference.py with the noise its tables were actually drawn with as their σ (60 mas, 30 m/s): a
posterior with one dominant optimum that the scaled L-BFGS reaches from the best prior draws. The scaling v is the variance of prior draws
0 … 4095 in θ_t, the default of the device drivers.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import hmc_reference as href
import lbfgs_reference as ref
import test_hmc_reference as cond

SEED, N_DRAWS, N_STARTS = 77, 65536, 64
M, GTOL, ROUNDS = 6, 1e-6, 800
SHORT_W, SHORT_LD, SHORT_ROUNDS = 67, 71, 4      # one full wave plus three lanes, a padded leading dimension
DECIDED_ROUNDS = 40                              # how far into the full run the decisions of the decided chains are compared
MID_ROUNDS, INPUT_NOISE = 10, 1e-12              # where its Pathfinder diagonal is compared; the level at which device and oracle ℓπ agree
MARGIN = 1e-6
SHORT_FTOLS = (0.0, 0.05)                        # without the ftol test, and with one that stops about half of the chains in the short run
TIGHT_SIGMA_ASTROM, TIGHT_SIGMA_RV = 60.0, 30.0


def tight_tables():
    """cond.model_tables() with σ the noise that was drawn"""
    astrom, rv = cond.model_tables()
    astrom = dict(astrom, σ_ra=np.full(12, TIGHT_SIGMA_ASTROM), σ_dec=np.full(12, TIGHT_SIGMA_ASTROM))
    return astrom, dict(rv, σ_rv=np.full(8, TIGHT_SIGMA_RV))


def tight_logpost(oracle, n_threads=0):
    """logpost(θ_t) -> (ℓπ, ∇ℓπ) of the tight model from the oracle's callback (n_threads = 1 for one θ_t at a time: no thread start a call)"""
    astrom, rv = tight_tables()
    obs = [dict(kind=0, planet=0, epoch=astrom["epoch"], y1=astrom["ra"], y2=astrom["dec"], s1=astrom["σ_ra"], s2=astrom["σ_dec"], cor=None, extra=None),
           dict(kind=2, planet=-1, epoch=rv["epoch"], y1=rv["rv"], y2=None, s1=rv["σ_rv"], s2=None, cor=None, extra=None)]
    _, planets, priors, esrc, nsrc = cond.oracle_model(oracle)
    return lambda th: oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, np.ascontiguousarray(th), grad=True, n_threads=n_threads)


def prior_theta_t(first, n):
    return href.prior_sample(cond.MODEL_PRIORS, SEED, np.uint64(first) + np.arange(n, dtype=np.uint64))[1]


def default_inv_mass(theta_t_4096):
    """the unbiased per-coordinate variance, as torch.var gives the device drivers"""
    return np.var(theta_t_4096, axis=1, ddof=1)


@functools.lru_cache(maxsize=None)
def reference_case(oracle):
    """(starts [D, 64] best first, their ℓπ, v, the restatement's result from them) — computed once, shared, never modified"""
    logpost = tight_logpost(oracle)
    tt = prior_theta_t(0, N_DRAWS)
    lp = np.concatenate([logpost(tt[:, k:k + 8192])[0] for k in range(0, N_DRAWS, 8192)])
    order = np.argsort(-np.where(np.isfinite(lp), lp, -np.inf), kind="stable")[:N_STARTS]
    starts, v = np.ascontiguousarray(tt[:, order]), default_inv_mass(tt[:, :4096])
    res = ref.lbfgs(logpost, starts, v, m=M, n_rounds=ROUNDS, gtol=GTOL)
    for a in (starts, v, *[x for x in res.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return starts, lp[order], v, res


# ---------------------------------------------------------------------------------------------------- what the recursion means
def random_history(rng, m, D, W, dtype=np.float64):
    """s random, y = A·s with A SPD of condition <= 1e3 (one A per chain); cnt cycles through 0 … m, head through 0 … m − 1"""
    S, Y = np.zeros((m, D, W), dtype=dtype), np.zeros((m, D, W), dtype=dtype)
    for w in range(W):
        Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
        A = (Q * np.logspace(0, 3 * rng.uniform(), D)) @ Q.T
        s = rng.normal(size=(m, D))
        S[:, :, w], Y[:, :, w] = s, s @ A.T
    cnt, head = np.arange(W) % (m + 1), (np.arange(W) * 3 + 1) % m
    return cnt, head, S, Y, rng.normal(size=(D, W)).astype(dtype), np.exp(rng.uniform(-3, 3, D)).astype(dtype)


@pytest.mark.parametrize("D,m", [(1, 1), (14, 6), (64, 8), (5, 3)])
def test_two_loop_is_the_dense_inverse_bfgs(D, m):
    """d = −H·g, H the inverse-BFGS updates of γ·diag(v) by the chain's cnt newest pairs; the float64 restatement is within 1e-10·max|d| of
    the same recursion in long double (ε = 1.1e-19), so the GPU bar of 1e-8 does not hide the reference's own noise. The long-double recursion
    and the long-double dense product are the same function: their bar is κ·ε·m·D with κ <= 1e3 — 5e-14 at the largest shape — taken as 1e-12."""
    rng = np.random.default_rng(1000 * D + m)
    W = 23
    cnt, head, S, Y, g, v = random_history(rng, m, D, W)
    d64 = ref.direction(cnt, head, S, Y, g, v)
    L = np.longdouble
    dl = ref.direction(cnt, head, S.astype(L), Y.astype(L), g.astype(L), v.astype(L))
    assert dl.dtype == L and np.finfo(L).eps < 2e-19
    worst64 = worst_dense = 0.0
    for w in range(W):
        pairs = [(S[ref.slot_of(head[w], k, m), :, w].astype(L), Y[ref.slot_of(head[w], k, m), :, w].astype(L)) for k in range(cnt[w] - 1, -1, -1)]
        gamma = L(1) if not pairs else (pairs[-1][0] @ pairs[-1][1]) / np.sum(pairs[-1][1] ** 2 * v.astype(L))
        dense = -ref.dense_inverse_bfgs(pairs, v.astype(L), gamma) @ g[:, w].astype(L)
        scale = float(np.max(np.abs(dense)))
        worst_dense = max(worst_dense, float(np.max(np.abs(dl[:, w] - dense))) / scale)
        worst64 = max(worst64, float(np.max(np.abs(d64[:, w] - dl[:, w]))) / scale)
    print(f"D {D} m {m}: two-loop against dense {worst_dense:.3e}, float64 against long double {worst64:.3e}")
    assert worst_dense <= 1e-12 and worst64 <= 1e-10
    # no pair: d = −v⊙g exactly
    none = cnt == 0
    assert none.any() and np.array_equal(d64[:, none], -(v[:, None] * g[:, none]))


def test_alpha_update_is_the_diagonal_of_the_dense_bfgs_update():
    rng = np.random.default_rng(5)
    D, W = 14, 9
    alpha = np.exp(rng.uniform(-3, 3, (D, W)))
    s = rng.normal(size=(D, W))
    y = s * np.exp(rng.uniform(-1, 1, (D, W)))      # sᵀy > 0
    got = ref.alpha_update(alpha, s, y)
    for w in range(W):
        a, b = np.sum(y[:, w] ** 2 * alpha[:, w]), s[:, w] @ y[:, w]
        B = (a / b) * np.diag(1.0 / alpha[:, w])
        Bs = B @ s[:, w]
        Bn = B - np.outer(Bs, Bs) / (s[:, w] @ Bs) + np.outer(y[:, w], y[:, w]) / b
        assert np.allclose(got[:, w], 1.0 / np.diag(Bn), rtol=1e-12, atol=0.0)
        assert np.all(got[:, w] > 0)


# ---------------------------------------------------------------------------------------------------- against scipy
def test_restatement_against_scipy(oracle):
    from scipy.optimize import minimize
    starts, lp0, v, res = reference_case(oracle)
    logpost = tight_logpost(oracle, n_threads=1)
    conv = res["status"] == ref.GTOL
    print(f"restatement: {conv.sum()} of {N_STARTS} chains at gtol {GTOL} within {ROUNDS} rounds; status counts {np.bincount(res['status'], minlength=5)}; "
          f"evals {res['evals'].min()} … {res['evals'].max()}; best ℓπ {res['logpost'].max():.8f}")
    assert conv.mean() >= 0.75
    assert np.all(res["logpost"] >= lp0)
    sc = np.sqrt(v)

    def fun(z):      # scipy in the scaled variables z = θ_t/√v
        lp, g = logpost((z * sc)[:, None])
        return -float(lp[0]), -g[:, 0] * sc

    worst, n_cmp, its = 0.0, 0, []
    for w in range(N_STARTS):
        r = minimize(fun, starts[:, w] / sc, jac=True, method="L-BFGS-B", options=dict(maxiter=5000, maxfun=20000, ftol=1e-15, gtol=1e-7, maxcor=10))
        its.append(r.nit)
        if conv[w] and r.success and np.max(np.abs(r.jac)) <= 1e-5:
            n_cmp += 1
            worst = max(worst, abs(-r.fun - res["logpost"][w]) / max(1.0, abs(r.fun)))
    print(f"scipy L-BFGS-B: {n_cmp} chains compared, ℓπ differs by at most {worst:.3e} (relative); scipy iterations {min(its)} … {max(its)}")
    assert n_cmp >= 0.75 * N_STARTS and worst <= 1e-8


# ---------------------------------------------------------------------------------------------------- conditions of the GPU tests
@pytest.mark.parametrize("ftol", SHORT_FTOLS)
def test_first_rounds_are_decided_for_the_seed(oracle, ftol):
    """tests/test_lbfgs.py compares decisions on chains whose Armijo margin (and, with ftol > 0, the margin of the ftol test) stays above
    1e-6·max(1, |f|) and may leave out at most 5 %."""
    logpost = tight_logpost(oracle)
    _, _, v, _ = reference_case(oracle)
    r = ref.lbfgs(logpost, prior_theta_t(0, SHORT_W), v, m=M, n_rounds=SHORT_ROUNDS, gtol=GTOL, ftol=ftol)
    close = r["margin"] <= MARGIN
    print(f"ftol {ftol}: {close.sum()} of {SHORT_W} chains within {MARGIN} of a decision in {SHORT_ROUNDS} rounds; accepted steps {r['iters'].min()} … {r['iters'].max()}; "
          f"status counts {np.bincount(r['status'], minlength=5)}")
    assert close.mean() <= 0.05 and np.all(r["status"] != ref.DEAD) and r["iters"].max() >= 2 and (r["decisions"] == -1).any()
    n_ftol = np.sum(r["status"] == ref.FTOL)
    assert (n_ftol == 0) if ftol == 0.0 else (SHORT_W // 4 <= n_ftol <= 3 * SHORT_W // 4)


def test_forty_rounds_are_decided_for_most_starts(oracle):
    """tests/test_lbfgs.py compares the decisions of the full run through DECIDED_ROUNDS rounds on chains whose every decision so far had a
    margin: most of the 64 starts are such chains. (Over the whole run none is: near the optimum f_t − f is rounding noise.)"""
    starts, _, v, res = reference_case(oracle)
    r = ref.lbfgs(tight_logpost(oracle), starts, v, m=M, n_rounds=DECIDED_ROUNDS, gtol=GTOL)
    decided = r["margin"] > MARGIN
    print(f"{decided.sum()} of {N_STARTS} chains keep an Armijo margin above {MARGIN} through {DECIDED_ROUNDS} rounds; over the whole run {(res['margin'] > MARGIN).sum()}")
    assert decided.mean() >= 0.5 and np.all(r["status"] == ref.ACTIVE)


def test_pathfinder_diagonal_is_well_conditioned_for_ten_rounds(oracle):
    """The diagonal is a function of differences of gradients along the path, and the path amplifies a perturbation of ℓπ and ∇ℓπ from round
    to round: with inputs disturbed at INPUT_NOISE (relative), the restatement's own diagonal moves by 1e-9 after 10 rounds, 1e-7 after 20
    and 5e-4 after 40 (decisions unchanged). tests/test_lbfgs.py therefore holds the device's diagonal to 1e-6 after the four rounds of its
    short run and after MID_ROUNDS rounds of the full run, where the restatement's own response stays a factor 100 below that bar."""
    logpost = tight_logpost(oracle)
    starts, _, v, _ = reference_case(oracle)
    rng = np.random.default_rng(0)

    def disturbed(th):
        lp, g = logpost(th)
        return lp * (1.0 + INPUT_NOISE * rng.uniform(-1, 1, lp.shape)), g * (1.0 + INPUT_NOISE * rng.uniform(-1, 1, g.shape))

    a = ref.lbfgs(logpost, starts, v, m=M, n_rounds=MID_ROUNDS, gtol=GTOL)
    b = ref.lbfgs(disturbed, starts, v, m=M, n_rounds=MID_ROUNDS, gtol=GTOL)
    decided = a["margin"] > MARGIN
    assert decided.mean() >= 0.5 and np.array_equal(a["decisions"][:, decided], b["decisions"][:, decided])
    moved = np.max(np.abs(b["inv_hess_diag"][:, decided] / a["inv_hess_diag"][:, decided] - 1.0))
    print(f"after {MID_ROUNDS} rounds with inputs disturbed at {INPUT_NOISE}: {decided.sum()} chains decided, the restatement's diagonal moves by at most {moved:.3e}")
    assert moved <= 1e-8


def test_perturbed_starts_reach_the_same_optimum(oracle):
    logpost = tight_logpost(oracle)
    starts, _, v, res = reference_case(oracle)
    pert = ref.lbfgs(logpost, starts * (1.0 + 1e-9), v, m=M, n_rounds=ROUNDS, gtol=GTOL)
    both = (res["status"] == ref.GTOL) & (pert["status"] == ref.GTOL)
    diff = np.abs(pert["logpost"][both] - res["logpost"][both]) / np.maximum(1.0, np.abs(res["logpost"][both]))
    print(f"{both.sum()} of {N_STARTS} chains converge in both runs; their ℓπ differ by at most {diff.max():.3e}")
    assert both.mean() >= 0.75 and diff.max() <= 1e-8


def test_frozen_chains_and_resume_in_the_restatement(oracle):
    """two segments equal one run, and a converged chain no longer moves"""
    logpost = tight_logpost(oracle)
    starts, _, v, _ = reference_case(oracle)
    x = starts[:, ::4]
    one = ref.lbfgs(logpost, x, v, m=M, n_rounds=500, gtol=GTOL)
    half = ref.lbfgs(logpost, x, v, m=M, n_rounds=400, gtol=GTOL)
    frozen = half["status"] != ref.ACTIVE
    kept = {k: half[k][..., frozen].copy() for k in ("theta_t", "logpost", "inv_hess_diag")}
    two = ref.lbfgs(logpost, None, v, m=M, n_rounds=100, gtol=GTOL, state=half["state"])
    assert all(np.array_equal(two[k][..., frozen], kept[k]) for k in kept)
    for k in ("theta_t", "logpost", "gnorm", "status", "iters", "evals", "inv_hess_diag"):
        assert np.array_equal(one[k], two[k]), k
    assert frozen.any() and not frozen.all()


# ---------------------------------------------------------------------------------------------------- argument checks without a device
def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made, so these go through the NULL handle, which is refused before anything else; the same
    arguments on a real handle are in tests/test_lbfgs.py."""
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    build_draws()
    from octofitter_jl_amd.host import draws
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    th, vec = np.zeros((2, 4)), np.zeros(4)
    ints = [(C.c_int32 * 4)() for _ in range(3)]
    dp = pkg.capi._dptr
    assert lib.octo_draws_lbfgs_direction_device(None, 4, 4, 2, None, None, None, None, None, None, None, None) == EINVAL
    assert lib.octo_draws_lbfgs_device(None, 4, 4, None, None, 6, 1, 1e-6, 0.0, 0, None, None, None, None, None, None, None) == EINVAL
    for m, n_rounds, ld, gtol in ((6, 1, 4, 1e-6), (0, 1, 4, 1e-6), (9, 1, 4, 1e-6), (6, -1, 4, 1e-6), (6, 1, 3, 1e-6), (6, 1, 4, math.nan)):
        assert lib.octo_draws_lbfgs(None, 4, ld, dp(th), None, m, n_rounds, gtol, 0.0, dp(vec), dp(vec), *ints, None) == EINVAL
    assert (draws.LBFGS_ACTIVE, draws.LBFGS_GTOL, draws.LBFGS_FTOL, draws.LBFGS_LINESEARCH, draws.LBFGS_DEAD) == (ref.ACTIVE, ref.GTOL, ref.FTOL, ref.LINESEARCH, ref.DEAD)
    assert draws.LBFGS_MAX_M == ref.MAX_M
