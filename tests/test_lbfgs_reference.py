"""
Conditions on the NumPy restatement of the batched L-BFGS (tests/lbfgs_reference.py) that need no device: what the two-loop recursion and
the Pathfinder diagonal mean (against dense BFGS algebra, and against the same recursion in extended precision), the optimiser against
scipy's L-BFGS-B on the oracle's callback, and the conditions the GPU tests of tests/test_lbfgs.py rest on, from the reference alone.

The tight model, its 64 starts, the scaling v and the settings of the runs are those of tests/draws_cases.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import draws_cases as cases
import lbfgs_reference as ref

INPUT_NOISE = 1e-12      # the level at which device and oracle ℓπ agree


# ---------------------------------------------------------------------------------------------------- what the recursion means
@pytest.mark.parametrize("D,m", [(1, 1), (14, 6), (64, 8), (5, 3)])
def test_two_loop_is_the_dense_inverse_bfgs(D, m):
    """d = −H·g, H the inverse-BFGS updates of γ·diag(v) by the chain's cnt newest pairs; the float64 restatement is within 1e-10·max|d| of
    the same recursion in long double (ε = 1.1e-19), so the GPU bar of 1e-8 does not hide the reference's own noise. The long-double recursion
    and the long-double dense product are the same function: their bar is κ·ε·m·D with κ <= 1e3 — 5e-14 at the largest shape — taken as 1e-12."""
    rng = np.random.default_rng(1000 * D + m)
    W = 23
    cnt, head, S, Y, g, v = cases.random_history(rng, m, D, W)
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
    starts, lp0, v, res = cases.reference_case(oracle)
    logpost = cases.tight_logpost(oracle, n_threads=1)
    conv = res["status"] == ref.GTOL
    print(f"restatement: {conv.sum()} of {cases.LBFGS_N_STARTS} chains at gtol {cases.LBFGS_GRAD_TOL} within {cases.LBFGS_ROUNDS} rounds; status counts {np.bincount(res['status'], minlength=5)}; "
          f"evals {res['evals'].min()} … {res['evals'].max()}; best ℓπ {res['logpost'].max():.8f}")
    assert conv.mean() >= 0.75
    assert np.all(res["logpost"] >= lp0)
    sc = np.sqrt(v)

    def fun(z):      # scipy in the scaled variables z = θ_t/√v
        lp, g = logpost((z * sc)[:, None])
        return -float(lp[0]), -g[:, 0] * sc

    worst, n_cmp, its = 0.0, 0, []
    for w in range(cases.LBFGS_N_STARTS):
        r = minimize(fun, starts[:, w] / sc, jac=True, method="L-BFGS-B", options=dict(maxiter=5000, maxfun=20000, ftol=1e-15, gtol=1e-7, maxcor=10))
        its.append(r.nit)
        if conv[w] and r.success and np.max(np.abs(r.jac)) <= 1e-5:
            n_cmp += 1
            worst = max(worst, abs(-r.fun - res["logpost"][w]) / max(1.0, abs(r.fun)))
    print(f"scipy L-BFGS-B: {n_cmp} chains compared, ℓπ differs by at most {worst:.3e} (relative); scipy iterations {min(its)} … {max(its)}")
    assert n_cmp >= 0.75 * cases.LBFGS_N_STARTS and worst <= 1e-8


# ---------------------------------------------------------------------------------------------------- conditions of the GPU tests
@pytest.mark.parametrize("ftol", cases.LBFGS_SHORT_FTOLS)
def test_first_rounds_are_decided_for_the_seed(oracle, ftol):
    """tests/test_lbfgs.py compares decisions on chains whose Armijo margin (and, with ftol > 0, the margin of the ftol test) stays above
    1e-6·max(1, |f|) and may leave out at most 5 %."""
    logpost = cases.tight_logpost(oracle)
    _, _, v, _ = cases.reference_case(oracle)
    r = ref.lbfgs(logpost, cases.prior_theta_t(0, cases.LBFGS_SHORT_W), v, m=cases.LBFGS_M, n_rounds=cases.LBFGS_SHORT_ROUNDS, gtol=cases.LBFGS_GRAD_TOL, ftol=ftol)
    close = r["margin"] <= cases.LBFGS_MARGIN
    print(f"ftol {ftol}: {close.sum()} of {cases.LBFGS_SHORT_W} chains within {cases.LBFGS_MARGIN} of a decision in {cases.LBFGS_SHORT_ROUNDS} rounds; accepted steps {r['iters'].min()} … {r['iters'].max()}; "
          f"status counts {np.bincount(r['status'], minlength=5)}")
    assert close.mean() <= 0.05 and np.all(r["status"] != ref.DEAD) and r["iters"].max() >= 2 and (r["decisions"] == -1).any()
    n_ftol = np.sum(r["status"] == ref.FTOL)
    assert (n_ftol == 0) if ftol == 0.0 else (cases.LBFGS_SHORT_W // 4 <= n_ftol <= 3 * cases.LBFGS_SHORT_W // 4)


def test_forty_rounds_are_decided_for_most_starts(oracle):
    """tests/test_lbfgs.py compares the decisions of the full run through cases.LBFGS_DECIDED_ROUNDS rounds on chains whose every decision so far had a
    margin: most of the 64 starts are such chains. (Over the whole run none is: near the optimum f_t − f is rounding noise.)"""
    starts, _, v, res = cases.reference_case(oracle)
    r = ref.lbfgs(cases.tight_logpost(oracle), starts, v, m=cases.LBFGS_M, n_rounds=cases.LBFGS_DECIDED_ROUNDS, gtol=cases.LBFGS_GRAD_TOL)
    decided = r["margin"] > cases.LBFGS_MARGIN
    print(f"{decided.sum()} of {cases.LBFGS_N_STARTS} chains keep an Armijo margin above {cases.LBFGS_MARGIN} through {cases.LBFGS_DECIDED_ROUNDS} rounds; over the whole run {(res['margin'] > cases.LBFGS_MARGIN).sum()}")
    assert decided.mean() >= 0.5 and np.all(r["status"] == ref.ACTIVE)


def test_pathfinder_diagonal_is_well_conditioned_for_ten_rounds(oracle):
    """The diagonal is a function of differences of gradients along the path, and the path amplifies a perturbation of ℓπ and ∇ℓπ from round
    to round: with inputs disturbed at INPUT_NOISE (relative), the restatement's own diagonal moves by 1e-9 after 10 rounds, 1e-7 after 20
    and 5e-4 after 40 (decisions unchanged). tests/test_lbfgs.py therefore holds the device's diagonal to 1e-6 after the four rounds of its
    short run and after cases.LBFGS_MID_ROUNDS rounds of the full run, where the restatement's own response stays a factor 100 below that bar."""
    logpost = cases.tight_logpost(oracle)
    starts, _, v, _ = cases.reference_case(oracle)
    rng = np.random.default_rng(0)

    def disturbed(th):
        lp, g = logpost(th)
        return lp * (1.0 + INPUT_NOISE * rng.uniform(-1, 1, lp.shape)), g * (1.0 + INPUT_NOISE * rng.uniform(-1, 1, g.shape))

    a = ref.lbfgs(logpost, starts, v, m=cases.LBFGS_M, n_rounds=cases.LBFGS_MID_ROUNDS, gtol=cases.LBFGS_GRAD_TOL)
    b = ref.lbfgs(disturbed, starts, v, m=cases.LBFGS_M, n_rounds=cases.LBFGS_MID_ROUNDS, gtol=cases.LBFGS_GRAD_TOL)
    decided = a["margin"] > cases.LBFGS_MARGIN
    assert decided.mean() >= 0.5 and np.array_equal(a["decisions"][:, decided], b["decisions"][:, decided])
    moved = np.max(np.abs(b["inv_hess_diag"][:, decided] / a["inv_hess_diag"][:, decided] - 1.0))
    print(f"after {cases.LBFGS_MID_ROUNDS} rounds with inputs disturbed at {INPUT_NOISE}: {decided.sum()} chains decided, the restatement's diagonal moves by at most {moved:.3e}")
    assert moved <= 1e-8


def test_perturbed_starts_reach_the_same_optimum(oracle):
    logpost = cases.tight_logpost(oracle)
    starts, _, v, res = cases.reference_case(oracle)
    pert = ref.lbfgs(logpost, starts * (1.0 + 1e-9), v, m=cases.LBFGS_M, n_rounds=cases.LBFGS_ROUNDS, gtol=cases.LBFGS_GRAD_TOL)
    both = (res["status"] == ref.GTOL) & (pert["status"] == ref.GTOL)
    diff = np.abs(pert["logpost"][both] - res["logpost"][both]) / np.maximum(1.0, np.abs(res["logpost"][both]))
    print(f"{both.sum()} of {cases.LBFGS_N_STARTS} chains converge in both runs; their ℓπ differ by at most {diff.max():.3e}")
    assert both.mean() >= 0.75 and diff.max() <= 1e-8


def test_frozen_chains_and_resume_in_the_restatement(oracle):
    """two segments equal one run, and a converged chain no longer moves"""
    logpost = cases.tight_logpost(oracle)
    starts, _, v, _ = cases.reference_case(oracle)
    x = starts[:, ::4]
    one = ref.lbfgs(logpost, x, v, m=cases.LBFGS_M, n_rounds=500, gtol=cases.LBFGS_GRAD_TOL)
    half = ref.lbfgs(logpost, x, v, m=cases.LBFGS_M, n_rounds=400, gtol=cases.LBFGS_GRAD_TOL)
    frozen = half["status"] != ref.ACTIVE
    kept = {k: half[k][..., frozen].copy() for k in ("theta_t", "logpost", "inv_hess_diag")}
    two = ref.lbfgs(logpost, None, v, m=cases.LBFGS_M, n_rounds=100, gtol=cases.LBFGS_GRAD_TOL, state=half["state"])
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
