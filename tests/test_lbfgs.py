"""
The batched L-BFGS on the device (include/octofitter_hip_draws.h: octo_draws_lbfgs_direction_device, octo_draws_lbfgs_device,
octo_draws_lbfgs; host/draws.py: PriorDraws.lbfgs_direction / lbfgs; host/callers.py: optimize_starting_points_device) against its NumPy
restatement (tests/lbfgs_reference.py) fed by the oracle's callback, on the model and under the conditions that
tests/test_lbfgs_reference.py establishes on the CPU.

Tolerances: the project's oracle bar, 1e-8 relative to max(1, |ref|), for directions, θ_t and ℓπ; 1e-6 relative for the Pathfinder diagonal,
compared after 4 and after 10 rounds, as far as the restatement's own response to disturbed inputs stays below that bar (it grows along the path). Decisions (status, iters, evals) are compared on
chains that the reference alone shows to be decided: an Armijo margin (with ftol > 0 also the ftol test's) above 1e-6·max(1, |f|) in every round.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import draws_cases as cases
import lbfgs_reference as ref
from draws_device import differing, draws_mod, host_outputs, padded, rel, set_batch_invariant, tight_model      # noqa: F401

# tools/lbfgs_bench.py and tools/pathfinder_bench.py read tight_model from this module (test_lbfgs.tight_model): keep the name importable here

pytestmark = pytest.mark.gpu

W, LD, M, GTOL = cases.LBFGS_SHORT_W, cases.LBFGS_SHORT_LD, cases.LBFGS_M, cases.LBFGS_GRAD_TOL
OUT_KEYS = ("logpost", "gnorm", "status", "iters", "evals", "inv_hess_diag")


def same_outputs(a, b):
    return differing(a, b, ("theta_t",) + OUT_KEYS) == []


@pytest.fixture(scope="module")
def case(pkg, oracle, draws_mod):
    """The model, its handle, the default scaling and the 64 device starts with the device's and the restatement's full runs from them —
    computed once, shared by the tests below, never modified."""
    import torch
    model = tight_model(pkg)
    pd = draws_mod.PriorDraws(model)
    v = pd.sample(cases.LBFGS_SEED, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).cpu().numpy()
    θ0, lp0, _ = pd.best(cases.LBFGS_SEED, cases.LBFGS_N_DRAWS, keep=cases.LBFGS_N_STARTS)
    starts = np.ascontiguousarray(model.link(θ0))
    logpost = cases.tight_logpost(oracle)
    tt = torch.as_tensor(starts, device="cuda").clone()
    full = host_outputs(pd.lbfgs(tt, inv_mass=v, m=M, n_rounds=cases.LBFGS_ROUNDS, gtol=GTOL, want_inv_hess_diag=True), tt)
    full_ref = ref.lbfgs(logpost, starts, v, m=M, n_rounds=cases.LBFGS_ROUNDS, gtol=GTOL)
    yield dict(model=model, pd=pd, v=v, starts=starts, lp0=lp0, logpost=logpost, full=full, full_ref=full_ref)
    pd.close()
    model.close()


# ---------------------------------------------------------------------------------------------------- 1. the direction
@pytest.mark.parametrize("D,m", list(itertools.product((1, 14, 64), (1, 6, 8))))
def test_gpu_direction_against_the_restatement(pkg, draws_mod, D, m):
    import torch
    pd = draws_mod.PriorDraws(priors=[pkg.Uniform(0, 1)] * D)
    rng = np.random.default_rng(100 * D + m)
    cnt, head, S, Y, g, v = cases.random_history(rng, m, D, W)
    assert (cnt == 0).any() and (cnt == m).any()
    want = ref.direction(cnt, head, S, Y, g, v)
    worst = 0.0
    for inv_mass in (v, None):
        (_, Sv), (_, Yv), (gbuf, gv) = padded(torch, S, LD), padded(torch, Y, LD), padded(torch, g, LD)
        out = pd.lbfgs_direction(torch.as_tensor(cnt, dtype=torch.int32), torch.as_tensor(head, dtype=torch.int32), Sv, Yv, gv, inv_mass=inv_mass)
        torch.cuda.synchronize()
        assert out.stride(0) == LD or D == 1
        exp = want if inv_mass is not None else ref.direction(cnt, head, S, Y, g, None)
        err = np.max(np.abs(out.cpu().numpy() - exp) / np.maximum(1.0, np.max(np.abs(exp), axis=0)))
        worst = max(worst, err)
        assert bool(torch.isnan(gbuf[:, W:]).all())
    print(f"D {D} m {m}: direction max error {worst:.3e} of max(1, ‖ref‖∞) per chain")
    assert worst <= 1e-8
    pd.close()


# ---------------------------------------------------------------------------------------------------- 2. four rounds
@pytest.mark.parametrize("ftol", cases.LBFGS_SHORT_FTOLS)
def test_gpu_four_rounds_against_the_restatement(pkg, case, ftol):
    import torch
    model, pd, v = case["model"], case["pd"], case["v"]
    set_batch_invariant(pkg, model, 0)
    start = pd.sample(cases.LBFGS_SEED, 0, W, theta=False, logprior_t=False)[1]
    r = ref.lbfgs(case["logpost"], start.cpu().numpy(), v, m=M, n_rounds=cases.LBFGS_SHORT_ROUNDS, gtol=GTOL, ftol=ftol)
    decided = r["margin"] > cases.LBFGS_MARGIN
    print(f"ftol {ftol}: {np.sum(~decided)} of {W} chains within {cases.LBFGS_MARGIN} of a decision; status counts {np.bincount(r['status'], minlength=5)}; reference accepted steps {r['iters'].min()} … {r['iters'].max()}")
    assert np.mean(~decided) <= 0.05, "condition on the seed (the reference alone)"
    buf, tt = padded(torch, start, LD)
    got = host_outputs(pd.lbfgs(tt, inv_mass=v, m=M, n_rounds=cases.LBFGS_SHORT_ROUNDS, gtol=GTOL, ftol=ftol, want_inv_hess_diag=True), tt)
    assert bool(torch.isnan(buf[:, W:]).all())                                  # nothing written beyond column W
    for k in ("status", "iters", "evals"):
        assert np.array_equal(got[k][decided], r[k][decided]), k
    e_th, e_lp = np.max(rel(got["theta_t"][:, decided], r["theta_t"][:, decided])), np.max(rel(got["logpost"][decided], r["logpost"][decided]))
    e_ih = np.max(np.abs(got["inv_hess_diag"][:, decided] / r["inv_hess_diag"][:, decided] - 1.0))
    print(f"four rounds: max errors — θ_t {e_th:.3e}, ℓπ {e_lp:.3e} (relative to max(1, |ref|)); inverse-Hessian diagonal {e_ih:.3e} (relative)")
    assert e_th <= 1e-8 and e_lp <= 1e-8 and e_ih <= 1e-6
    assert got["iters"].max() >= 2 and got["iters"].min() < cases.LBFGS_SHORT_ROUNDS
    assert np.all(got["evals"] == cases.LBFGS_SHORT_ROUNDS + 1) if ftol == 0.0 else np.any(got["status"] == ref.FTOL)


# ---------------------------------------------------------------------------------------------------- 3. the full run
def test_gpu_full_run(pkg, oracle, case):
    import torch
    pd, v, starts, full, r = case["pd"], case["v"], case["starts"], case["full"], case["full_ref"]
    n = cases.LBFGS_N_STARTS
    print(f"device: status counts {np.bincount(full['status'], minlength=5)}, evals {full['evals'].min()} … {full['evals'].max()}, best ℓπ {full['logpost'].max():.8f}; "
          f"restatement: status counts {np.bincount(r['status'], minlength=5)}, best ℓπ {r['logpost'].max():.8f}")
    assert np.all(full["logpost"] >= case["lp0"])                               # Armijo: no chain ends below its start
    lp_o, g_o = case["logpost"](full["theta_t"])
    assert np.max(rel(full["logpost"], lp_o)) <= 1e-8
    conv = full["status"] == ref.GTOL
    gn_o = np.max(np.abs(g_o) * np.sqrt(v)[:, None], axis=0)
    print(f"oracle's scaled gradient at the converged chains: max {gn_o[conv].max():.3e}")
    assert np.all(gn_o[conv] <= 2 * GTOL) and np.all(full["gnorm"][conv] <= GTOL)
    both = conv & (r["status"] == ref.GTOL)
    diff = rel(full["logpost"][both], r["logpost"][both])
    print(f"{both.sum()} of {n} chains converged on both sides; their ℓπ differ by at most {diff.max():.3e}")
    assert both.mean() >= 0.75 and diff.max() <= 1e-8
    assert abs(full["logpost"].max() - r["logpost"].max()) <= 1e-8 * max(1.0, abs(r["logpost"].max()))
    ihd = full["inv_hess_diag"]
    assert np.all(np.isfinite(ihd)) and np.all(ihd > 0)
    # the decisions of every round, from a run in segments of one round (which is the same run, bit for bit)
    tt = torch.as_tensor(starts, device="cuda").clone()
    its, sts = [], []
    for k in range(cases.LBFGS_ROUNDS):
        seg = pd.lbfgs(tt, inv_mass=v, m=M, n_rounds=1, gtol=GTOL, resume=k > 0, want_inv_hess_diag=True)
        its.append(seg["iters"]), sts.append(seg["status"])
        if k + 1 == cases.LBFGS_MID_ROUNDS:
            ihd_mid = seg["inv_hess_diag"].cpu().numpy()
    seg = host_outputs(seg, tt)
    assert same_outputs(seg, full)
    its, sts = torch.stack(its).cpu().numpy(), torch.stack(sts).cpu().numpy()
    active = np.vstack([np.ones((1, n), dtype=bool), sts[:-1] == ref.ACTIVE])
    accepted = np.diff(np.vstack([np.zeros((1, n), dtype=its.dtype), its]), axis=0) > 0
    dec = np.where(active, np.where(accepted, 1, -1), 0)
    dec_ref = np.zeros_like(dec)
    dec_ref[:r["decisions"].shape[0]] = r["decisions"]
    matched = np.all(dec == dec_ref, axis=0)
    first = np.where(matched, cases.LBFGS_ROUNDS, np.argmax(dec != dec_ref, axis=0))
    e_ih = np.max(np.abs(ihd[:, matched] / r["inv_hess_diag"][:, matched] - 1.0)) if matched.any() else 0.0
    print(f"{matched.sum()} of {n} chains made the restatement's decision in every round (the first other decision: round {first.min()} at the earliest, "
          f"median {int(np.median(first))}); their inverse-Hessian diagonals differ by at most {e_ih:.3e} (relative)")
    assert e_ih <= 1e-6
    # … through DECIDED_ROUNDS rounds the decided chains make the restatement's decisions, and after MID_ROUNDS rounds their diagonals agree:
    # as far as the restatement's own response to inputs disturbed at the device's level stays below the bar (tests/test_lbfgs_reference.py)
    for rounds in (cases.LBFGS_DECIDED_ROUNDS, cases.LBFGS_MID_ROUNDS):
        mid = ref.lbfgs(case["logpost"], starts, v, m=M, n_rounds=rounds, gtol=GTOL)
        decided = mid["margin"] > cases.LBFGS_MARGIN
        assert decided.mean() >= 0.5, "condition on the starts (the reference alone)"
        assert np.array_equal(dec[:rounds, decided], mid["decisions"][:, decided])
    e_mid = np.max(np.abs(ihd_mid[:, decided] / mid["inv_hess_diag"][:, decided] - 1.0))
    print(f"after {cases.LBFGS_MID_ROUNDS} rounds: {decided.sum()} of {n} chains decided, their inverse-Hessian diagonals differ by at most {e_mid:.3e} (relative)")
    assert e_mid <= 1e-6


# ---------------------------------------------------------------------------------------------------- 4. batch invariance, 5. resume
def run(torch, pd, x, v, n_rounds, ld=None, **kw):
    _buf, tt = padded(torch, x, ld or x.shape[1])
    return host_outputs(pd.lbfgs(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=n_rounds, want_inv_hess_diag=True, **kw), tt), tt


def test_gpu_batch_invariance_and_resume(pkg, case):
    import torch
    model, pd, v = case["model"], case["pd"], case["v"]
    start = pd.sample(cases.LBFGS_SEED, 0, W, theta=False, logprior_t=False)[1].cpu().numpy()
    set_batch_invariant(pkg, model, 1)
    try:
        whole, _ = run(torch, pd, start, v, 40, ld=LD)
        part, _ = run(torch, pd, np.ascontiguousarray(start[:, 5:9]), v, 40)
        assert same_outputs({k: x[..., 5:9] for k, x in whole.items()}, part)
        assert whole["iters"][5:9].min() >= 5
    finally:
        set_batch_invariant(pkg, model, 0)
    one, _ = run(torch, pd, start, v, 40, ld=LD)
    _, tt = run(torch, pd, start, v, 20, ld=LD)
    two = host_outputs(pd.lbfgs(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=20, resume=True, want_inv_hess_diag=True), tt)
    assert same_outputs(one, two)
    assert np.all(one["evals"] == 41)
    assert same_outputs(two, host_outputs(pd.lbfgs(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=0, resume=True, want_inv_hess_diag=True), tt))      # no round: the outputs alone


# ---------------------------------------------------------------------------------------------------- 6. frozen and dead chains
def test_gpu_frozen_and_dead_chains(pkg, case):
    import torch
    pd, v, starts = case["pd"], case["v"], case["starts"]
    mid, tt = run(torch, pd, starts, v, 400)
    frozen = mid["status"] != ref.ACTIVE
    assert frozen.any() and not frozen.all(), np.bincount(mid["status"], minlength=5)
    more = host_outputs(pd.lbfgs(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=10, resume=True, want_inv_hess_diag=True), tt)
    assert same_outputs({k: x[..., frozen] for k, x in mid.items()}, {k: x[..., frozen] for k, x in more.items()})
    assert np.all(more["evals"][~frozen] > mid["evals"][~frozen])
    dirty = starts.copy()
    dirty[3, 7] = np.nan
    got, _ = run(torch, pd, dirty, v, 12, ld=LD)
    assert got["status"][7] == ref.DEAD and got["iters"][7] == 0 and got["evals"][7] == 1
    assert np.array_equal(got["theta_t"][:, 7], dirty[:, 7], equal_nan=True) and np.isnan(got["theta_t"][3, 7])
    others = np.arange(dirty.shape[1]) != 7
    assert np.all(got["status"][others] != ref.DEAD) and np.all(got["logpost"][others] >= case["lp0"][others])


# ---------------------------------------------------------------------------------------------------- 7. the host twin
def test_gpu_host_twin(pkg, case):
    import torch
    pd, v = case["pd"], case["v"]
    start = pd.sample(cases.LBFGS_SEED, 0, W, theta=False, logprior_t=False)[1].cpu().numpy()
    dev, _ = run(torch, pd, start, v, 30, ld=LD)
    D = start.shape[0]
    th = np.full((D, LD), np.nan)
    th[:, :W] = start
    ihd = np.full((D, LD), np.nan)
    lp, gn = np.empty(W), np.empty(W)
    status, iters, evals = (np.empty(W, dtype=np.int32) for _ in range(3))
    dp, ip = pkg.capi._dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    pd._check(pd.lib.octo_draws_lbfgs(pd._h, W, LD, dp(th), dp(np.ascontiguousarray(v)), M, 30, GTOL, 0.0, dp(lp), dp(gn), ip(status), ip(iters), ip(evals), dp(ihd)))
    twin = dict(theta_t=th[:, :W], logpost=lp, gnorm=gn, status=status, iters=iters, evals=evals, inv_hess_diag=ihd[:, :W])
    assert same_outputs(dev, twin)
    assert np.all(np.isnan(th[:, W:]))


# ---------------------------------------------------------------------------------------------------- 8. arguments
def test_gpu_lbfgs_argument_checks(pkg, draws_mod, case):
    import torch
    model, pd = case["model"], case["pd"]
    lib, EINVAL, n = pd.lib, pkg.capi.OCTO_EINVAL, 8
    tt = pd.sample(1, 0, n, theta=False, logprior_t=False)[1]
    lp, gn = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
    ints = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, W_=n, ld=n, m=M, n_rounds=1, gtol=1e-6, ftol=0.0, resume=0, theta=tt.data_ptr(), status=ints[0].data_ptr()):
        return lib.octo_draws_lbfgs_device(h, W_, ld, theta, None, m, n_rounds, gtol, ftol, resume, lp.data_ptr(), gn.data_ptr(), status,
                                           ints[1].data_ptr(), ints[2].data_ptr(), None, st)

    err = lambda: lib.octo_draws_last_error(pd._h)      # noqa: E731
    assert call(None) == EINVAL
    fresh = draws_mod.PriorDraws(model)
    assert call(fresh._h, resume=1) == EINVAL and b"resume" in lib.octo_draws_last_error(fresh._h)      # no previous call
    fresh.close()
    for m in (0, 9, -1):
        assert call(pd._h, m=m) == EINVAL and b"m must be" in err()
    assert call(pd._h, n_rounds=-1) == EINVAL and b"n_rounds" in err()
    assert call(pd._h, W_=-1) == EINVAL and call(pd._h, ld=n - 1) == EINVAL and b"W <= ld" in err()
    assert call(pd._h, W_=(1 << 30) + 1, ld=(1 << 30) + 1) == EINVAL and b"2^30" in err()
    for bad in (-1e-6, math.inf, math.nan):
        assert call(pd._h, gtol=bad) == EINVAL and b"gtol" in err()
        assert call(pd._h, ftol=bad) == EINVAL and b"ftol" in err()
    assert call(pd._h, theta=None) == EINVAL and call(pd._h, status=None) == EINVAL and b"NULL" in err()
    assert call(pd._h, W_=0, ld=0) == 0
    assert call(pd._h, n_rounds=0) == 0                                         # the opening evaluation alone
    for kw in (dict(W_=n - 1), dict(W_=n - 1, ld=n - 1), dict(m=M - 1)):     # resume with another shape
        assert call(pd._h, resume=1, **kw) == EINVAL and b"resume" in err()
    assert call(pd._h, resume=1) == 0
    torch.cuda.synchronize()
    assert int(ints[2].max()) == 2 and int(ints[2].min()) == 2
    nomodel = draws_mod.PriorDraws(priors=[pkg.Uniform(0, 1)] * model.D)
    assert call(nomodel._h) == EINVAL and b"no model" in lib.octo_draws_last_error(nomodel._h)
    d = torch.zeros((model.D, n), dtype=torch.float64, device="cuda")
    hist = torch.zeros((2, model.D, n), dtype=torch.float64, device="cuda")
    direction = lambda m, W_=n, ld=n, g=d.data_ptr(): lib.octo_draws_lbfgs_direction_device(      # noqa: E731
        nomodel._h, W_, ld, m, ints[0].data_ptr(), ints[1].data_ptr(), hist.data_ptr(), hist.data_ptr(), g, None, d.data_ptr(), st)
    assert direction(0) == EINVAL and direction(9) == EINVAL and direction(2, ld=n - 1) == EINVAL and direction(2, g=None) == EINVAL
    assert direction(2, W_=0) == 0
    with pytest.raises(ValueError):
        pd.lbfgs(tt.t())
    nomodel.close()


# ---------------------------------------------------------------------------------------------------- 9. the driver
def test_gpu_optimize_starting_points_device(pkg, oracle, case, draws_mod):
    model = case["model"]
    out = pkg.optimize_starting_points_device(model, N=cases.LBFGS_N_DRAWS, n_starts=cases.LBFGS_N_STARTS, seed=cases.LBFGS_SEED)
    D, n = model.D, cases.LBFGS_N_STARTS
    assert out["theta"].shape == out["theta_t"].shape == out["inv_hess_diag"].shape == (D, n) and out["names"] == list(model.names)
    assert all(out[k].shape == (n,) for k in ("logpost", "start_logpost", "status", "iters", "evals"))
    print(f"driver: status counts {np.bincount(out['status'], minlength=5)}, evals {out['evals'].min()} … {out['evals'].max()}, best ℓπ {out['logpost'][out['best']]:.8f}")
    assert not np.any(out["status"] == draws_mod.LBFGS_ACTIVE)
    assert np.array_equal(out["start_logpost"], case["lp0"]) and np.all(out["logpost"] >= out["start_logpost"])
    _, lp_guess = pkg.guess_starting_position_device(model, N=cases.LBFGS_N_DRAWS, seed=cases.LBFGS_SEED)
    best = out["logpost"][out["best"]]
    assert best == out["logpost"].max() and best >= lp_guess
    optimum = cases.reference_case(oracle)[3]["logpost"].max()
    assert abs(best - optimum) <= 1e-8 * max(1.0, abs(optimum))
    assert np.max(rel(model.ℓπcallback(out["theta_t"]), out["logpost"])) <= 1e-8 and np.array_equal(model.link(out["theta"]).shape, (D, n))
