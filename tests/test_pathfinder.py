"""
Pathfinder on the device (include/octofitter_hip_draws.h: octo_draws_pathfinder_fit_device, octo_draws_pathfinder_device,
octo_draws_pathfinder_draw_device; host/draws.py: PriorDraws.pathfinder_fit / pathfinder / pathfinder_draw; host/callers.py:
pathfinder_device) against its NumPy restatement (tests/pathfinder_reference.py) fed by the oracle's callback, on the model and under the
condition that tests/test_pathfinder_reference.py establishes on the CPU.

Tolerances: the project's oracle bar, 1e-8 relative to max(1, |ref|), for μ, L̃, logdet, φ, log q, ℓπ and the ELBO. Selections (elbo_iter,
n_fits) and what follows from them are compared on chains that the reference alone shows to be decided: the two best ELBOs more than
1e-6·max(1, |ELBO|) apart and every Armijo margin of the path above 1e-6·max(1, |f|); at most 1/8 of the 64 chains may be left out.
"""
import ctypes as C
import math

import numpy as np
import pytest

import draws_cases as cases
import lbfgs_reference as lref
import pathfinder_reference as ref
from draws_device import differing, draws_mod, host_outputs, padded, rel, set_batch_invariant, tight_model      # noqa: F401

pytestmark = pytest.mark.gpu

SEED, CHAIN0, K, M, GTOL = cases.PF_SEED, cases.PF_CHAIN0, cases.PF_N_ELBO, cases.LBFGS_M, cases.LBFGS_GRAD_TOL
LB_KEYS = ("logpost", "gnorm", "status", "iters", "evals", "inv_hess_diag")
PF_KEYS = LB_KEYS + ("elbo", "elbo_iter", "n_fits")
N_FINAL = 4


def run(torch, pd, x, v, n_rounds, ld=None, chain0=CHAIN0, n_elbo=K, n_final=0, **kw):
    """pathfinder from x (padded to ld) and, with n_final, the final draws: everything on the host, and the device θ_t"""
    _buf, tt = padded(torch, x, ld or x.shape[1])
    out = host_outputs(pd.pathfinder(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=n_rounds, want_inv_hess_diag=True, seed=SEED, chain0=chain0, n_elbo=n_elbo, **kw), tt)
    if n_final:
        phi, logq, lp = pd.pathfinder_draw(tt, n_final, seed=SEED, chain0=chain0)
        W = x.shape[1]
        out.update(phi=phi.cpu().numpy().reshape(-1, n_final, W), logq=logq.cpu().numpy().reshape(n_final, W), draw_logpost=lp.cpu().numpy().reshape(n_final, W))
    return out, tt


DRAW_KEYS = ("phi", "logq", "draw_logpost")


@pytest.fixture(scope="module")
def case(pkg, oracle, draws_mod):
    """The model, its handle, the default scaling, the 64 device starts, the device's ROUNDS rounds with N_FINAL final draws from them, the
    plain L-BFGS of the same arguments, and the restatement's run from the same starts — computed once, shared, never modified."""
    import torch
    model = tight_model(pkg)
    pd = draws_mod.PriorDraws(model)
    v = pd.sample(cases.LBFGS_SEED, 0, 4096, theta=False, logprior_t=False)[1].var(dim=1).cpu().numpy()
    θ0, lp0, _ = pd.best(cases.LBFGS_SEED, cases.LBFGS_N_DRAWS, keep=cases.LBFGS_N_STARTS)
    starts = np.ascontiguousarray(model.link(θ0))
    logpost = cases.tight_logpost(oracle)
    got, _ = run(torch, pd, starts, v, cases.PF_ROUNDS, n_final=N_FINAL)
    tt = torch.as_tensor(starts, device="cuda").clone()
    plain = host_outputs(pd.lbfgs(tt, inv_mass=v, m=M, n_rounds=cases.PF_ROUNDS, gtol=GTOL, want_inv_hess_diag=True), tt)
    r = ref.pathfinder(logpost, starts, v, m=M, n_rounds=cases.PF_ROUNDS, gtol=GTOL, seed=SEED, chain0=CHAIN0, n_elbo=K)
    decided = cases.decided_chains(r) & (r["margin"] > cases.LBFGS_MARGIN)
    yield dict(model=model, pd=pd, v=v, starts=starts, lp0=lp0, logpost=logpost, got=got, plain=plain, ref=r, decided=decided)
    pd.close()
    model.close()


# ---------------------------------------------------------------------------------------------------- 1. the fit
@pytest.mark.parametrize("D,m", cases.PF_FIT_SHAPES)
def test_gpu_fit_against_the_restatement(pkg, draws_mod, D, m):
    import torch
    W, LD, n = cases.PF_FIT_W, cases.PF_FIT_LD, 3
    pd = draws_mod.PriorDraws(priors=[pkg.Uniform(0, 1)] * D)
    cnt, head, S, Y, x, g, alpha = cases.fit_inputs(D, m)
    z = np.random.default_rng(D + m).normal(size=(n, D, W))
    bad = int(np.nonzero(cnt >= 1)[0][1 if D > 1 else 0])      # one chain whose NEWEST pair gets sᵀy < 0: H̃ỹ = s̃ then has ỹᵀH̃ỹ < 0
    Yb = Y.copy()
    Yb[lref.slot_of(head[bad], 0, m), :, bad] *= -1.0
    worst = dict(mu=0.0, chol=0.0, logdet=0.0, phi=0.0)
    for Yin, broken in ((Y, None), (Yb, bad)):
        dev = [padded(torch, a, LD)[1] for a in (S, Yin, x, g, alpha, z)]
        out = pd.pathfinder_fit(torch.as_tensor(cnt, dtype=torch.int32), torch.as_tensor(head, dtype=torch.int32), *dev)
        torch.cuda.synchronize()
        out = {k: t.cpu().numpy() for k, t in out.items()}
        assert np.array_equal(out["ok"], (np.arange(W) != broken).astype(np.int32)) if broken is not None else np.all(out["ok"] == 1)
        for w in range(W):
            if w == broken:
                continue
            f = ref.fit_chain(ref.pairs_of(cnt[w], head[w], S, Yin, w), x[:, w], g[:, w], alpha[:, w])
            phi, _ = ref.draw_map(f["mu"], f["sqa"], f["L"], f["logdet"], z[:, :, w].T)
            for k, a, b in (("mu", out["mu"][:, w], f["mu"]), ("chol", out["chol"][:, w], ref.pack(f["L"])), ("logdet", out["logdet"][w], f["logdet"]),
                            ("phi", out["phi"][:, :, w].T, phi)):
                worst[k] = max(worst[k], float(np.max(rel(a, b))))
    print(f"D {D} m {m}: max errors relative to max(1, |ref|) — μ {worst['mu']:.3e}, L̃ {worst['chol']:.3e}, logdet {worst['logdet']:.3e}, φ {worst['phi']:.3e}")
    assert max(worst.values()) <= 1e-8
    pd.close()


# ---------------------------------------------------------------------------------------------------- 2. ten rounds
def test_gpu_ten_rounds_against_the_restatement(case):
    got, r, decided = case["got"], case["ref"], case["decided"]
    n = cases.LBFGS_N_STARTS
    left = np.nonzero(~decided)[0]
    print(f"{decided.sum()} of {n} chains decided; left out: {left.tolist()} (ELBO gap {r['margin_elbo'][left]}, Armijo margin {r['margin'][left]})")
    assert decided.sum() >= 7 * n // 8, "condition on the starts (the reference alone)"
    assert np.array_equal(got["elbo_iter"][decided], r["elbo_iter"][decided]) and np.array_equal(got["n_fits"][decided], r["n_fits"][decided])
    e = np.max(rel(got["elbo"][decided], r["elbo"][decided]))
    print(f"ELBO: max error {e:.3e} relative to max(1, |ELBO|); device's best {got['elbo'].max():.6f}; fits a chain {got['n_fits'].min()} … {got['n_fits'].max()}; "
          f"kept iterates {np.bincount(got['elbo_iter'][got['elbo_iter'] >= 0])}")
    assert e <= 1e-8
    assert got["n_fits"].max() >= 3 and np.all(got["n_fits"] == got["iters"])      # every accepted iterate gave a candidate
    # the L-BFGS is the L-BFGS: θ_t and its outputs with the bits of PriorDraws.lbfgs, on every chain
    assert differing(got, case["plain"], ("theta_t",) + LB_KEYS) == []


# ---------------------------------------------------------------------------------------------------- 3. the final draws
def test_gpu_draws_from_the_kept_fit(case):
    got, r, decided = case["got"], case["ref"], case["decided"]
    W = cases.LBFGS_N_STARTS
    phi, logq, _ = ref.pathfinder_draw(lambda th: (np.zeros(th.shape[1]), None), r["state"], SEED, CHAIN0, N_FINAL)
    phi, logq = phi.reshape(-1, N_FINAL, W), logq.reshape(N_FINAL, W)
    e_phi, e_q = np.max(rel(got["phi"][:, :, decided], phi[:, :, decided])), np.max(rel(got["logq"][:, decided], logq[:, decided]))
    lp_o = case["logpost"](np.ascontiguousarray(got["phi"].reshape(-1, N_FINAL * W)))[0].reshape(N_FINAL, W)
    fin = np.isfinite(lp_o)
    assert np.array_equal(fin, np.isfinite(got["draw_logpost"])) and fin.mean() > 0.9
    e_lp = np.max(rel(got["draw_logpost"][fin], lp_o[fin]))
    print(f"final draws of {decided.sum()} decided chains: max errors relative to max(1, |ref|) — φ {e_phi:.3e}, log q {e_q:.3e}; ℓπ at the device's φ against the oracle {e_lp:.3e}")
    assert e_phi <= 1e-8 and e_q <= 1e-8 and e_lp <= 1e-8
    assert np.all(np.isfinite(got["logq"])) and got["phi"].std(axis=1).min() > 0


# ---------------------------------------------------------------------------------------------------- 4. invariance
def test_gpu_batch_invariance_resume_and_n_elbo(pkg, case):
    import torch
    model, pd, v = case["model"], case["pd"], case["v"]
    start = case["starts"][:, :24]
    keys = ("theta_t",) + PF_KEYS + DRAW_KEYS
    set_batch_invariant(pkg, model, 1)
    try:
        whole, _ = run(torch, pd, start, v, 8, ld=32, n_final=3)
        assert whole["n_fits"].min() >= 2 and np.all(whole["elbo_iter"] >= 1)
        sub = lambda o, cols: {k: x[..., cols] for k, x in o.items()}      # noqa: E731
        part, _ = run(torch, pd, np.ascontiguousarray(start[:, 5:9]), v, 8, chain0=CHAIN0 + 5, n_final=3)      # a subset, another ld
        assert differing(sub(whole, slice(5, 9)), part, keys) == []
        shifted, _ = run(torch, pd, np.ascontiguousarray(start[:, 3:20]), v, 8, ld=19, chain0=CHAIN0 + 3, n_final=3)      # another position, the same chain0 + c
        assert differing(sub(whole, slice(3, 20)), shifted, keys) == []
        moved, _ = run(torch, pd, np.ascontiguousarray(start[:, 3:20]), v, 8, chain0=CHAIN0 + 4, n_final=3)      # other random numbers: another ELBO
        assert differing(shifted, moved, ("theta_t",) + LB_KEYS) == [] and not np.array_equal(shifted["elbo"], moved["elbo"])
        # a + b rounds in two calls
        _, tt = run(torch, pd, start, v, 3, ld=32)
        two = host_outputs(pd.pathfinder(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=5, resume=True, want_inv_hess_diag=True, seed=SEED, chain0=CHAIN0, n_elbo=K), tt)
        assert differing(whole, two, ("theta_t",) + PF_KEYS) == []
        same = host_outputs(pd.pathfinder(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=0, resume=True, want_inv_hess_diag=True, seed=SEED, chain0=CHAIN0, n_elbo=K), tt)
        assert differing(two, same, ("theta_t",) + PF_KEYS) == []      # no round: the outputs alone
        phi, logq, lp = pd.pathfinder_draw(tt, 3, seed=SEED, chain0=CHAIN0)
        assert np.array_equal(phi.cpu().numpy().reshape(-1, 3, 24), whole["phi"]) and np.array_equal(logq.cpu().numpy().reshape(3, 24), whole["logq"])
        # n_elbo = 3 scores a fit by the first three of the five draws: where the selection stays, the kept fit and its draws are the same
        three, _ = run(torch, pd, start, v, 8, ld=32, n_elbo=3, n_final=3)
        stay = three["elbo_iter"] == whole["elbo_iter"]
        print(f"n_elbo 3 against 5: {stay.sum()} of 24 chains keep their iterate")
        assert differing(whole, three, ("theta_t", "n_fits") + LB_KEYS) == [] and stay.any()
        assert differing(sub(whole, stay), sub(three, stay), DRAW_KEYS) == [] and not np.array_equal(whole["elbo"], three["elbo"])
    finally:
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 5. frozen and dead chains
def test_gpu_frozen_and_dead_chains(case):
    import torch
    pd, v, starts = case["pd"], case["v"], case["starts"]
    mid, tt = run(torch, pd, starts, v, 400, n_final=2)
    frozen = mid["status"] != lref.ACTIVE
    assert frozen.any(), np.bincount(mid["status"], minlength=5)
    more = host_outputs(pd.pathfinder(tt, inv_mass=v, m=M, gtol=GTOL, n_rounds=10, resume=True, want_inv_hess_diag=True, seed=SEED, chain0=CHAIN0, n_elbo=K), tt)
    assert differing({k: x[..., frozen] for k, x in mid.items()}, {k: x[..., frozen] for k, x in more.items()}, ("theta_t",) + PF_KEYS) == []
    assert np.all(more["n_fits"] >= mid["n_fits"]) and np.all(mid["elbo_iter"][frozen] >= 1)
    dirty = starts[:, :16].copy()
    dirty[3, 7] = np.nan
    got, _ = run(torch, pd, dirty, v, 6, ld=19, n_final=2)
    assert got["status"][7] == lref.DEAD and got["elbo"][7] == -np.inf and got["elbo_iter"][7] == -1 and got["n_fits"][7] == 0
    assert np.array_equal(got["theta_t"][:, 7], dirty[:, 7], equal_nan=True) and np.isnan(got["theta_t"][3, 7])      # its column is never written
    assert np.array_equal(got["phi"][:, :, 7], np.repeat(dirty[:, 7:8], 2, axis=1), equal_nan=True)
    assert np.all(np.isnan(got["logq"][:, 7])) and np.all(got["draw_logpost"][:, 7] == -np.inf)
    others = np.arange(16) != 7
    assert np.all(got["elbo_iter"][others] >= 1) and np.all(np.isfinite(got["logq"][:, others])) and np.all(np.isfinite(got["elbo"][others]))


# ---------------------------------------------------------------------------------------------------- 6. arguments
def test_gpu_pathfinder_argument_checks(pkg, draws_mod, case):
    import torch
    model, pd = case["model"], case["pd"]
    lib, EINVAL, n = pd.lib, pkg.capi.OCTO_EINVAL, 8
    tt = pd.sample(1, 0, n, theta=False, logprior_t=False)[1]
    dbl = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3)]
    ints = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(5)]
    out = torch.zeros((model.D + 2, 4 * n), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, W_=n, ld=n, m=M, n_rounds=1, gtol=1e-6, ftol=0.0, n_elbo=K, resume=0, theta=tt.data_ptr(), elbo=dbl[2].data_ptr()):
        return lib.octo_draws_pathfinder_device(h, 1, 0, W_, ld, theta, None, m, n_rounds, gtol, ftol, n_elbo, resume, dbl[0].data_ptr(), dbl[1].data_ptr(),
                                                ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), None, elbo, ints[3].data_ptr(), ints[4].data_ptr(), st)

    def draw(h, W_=n, ld=n, n_draws=4, ld_out=4 * n, phi=out.data_ptr()):
        return lib.octo_draws_pathfinder_draw_device(h, 1, 0, W_, ld, tt.data_ptr(), n_draws, ld_out, phi, out[model.D].data_ptr(), out[model.D + 1].data_ptr(), st)

    err = lambda h=pd: lib.octo_draws_last_error(h._h)      # noqa: E731
    assert call(None) == EINVAL and draw(None) == EINVAL
    fresh = draws_mod.PriorDraws(model)
    assert call(fresh._h, resume=1) == EINVAL and b"resume" in err(fresh)                 # no previous call
    assert draw(fresh._h) == EINVAL and b"previous" in err(fresh)
    tl = tt.clone()
    assert lib.octo_draws_lbfgs_device(fresh._h, n, n, tl.data_ptr(), None, M, 1, 1e-6, 0.0, 0, dbl[0].data_ptr(), dbl[1].data_ptr(), ints[0].data_ptr(),
                                       ints[1].data_ptr(), ints[2].data_ptr(), None, st) == 0
    assert call(fresh._h, resume=1) == EINVAL and b"resume" in err(fresh)                 # an L-BFGS call is no Pathfinder call
    fresh.close()
    for m in (0, 9, -1):
        assert call(pd._h, m=m) == EINVAL and b"m must be" in err()
    for k in (0, 33, -1):
        assert call(pd._h, n_elbo=k) == EINVAL and b"n_elbo" in err()
    assert call(pd._h, n_rounds=-1) == EINVAL and b"n_rounds" in err()
    assert call(pd._h, W_=-1) == EINVAL and call(pd._h, ld=n - 1) == EINVAL and b"W <= ld" in err()
    assert call(pd._h, W_=(1 << 25) + 1, ld=(1 << 25) + 1) == EINVAL and b"2^25" in err()
    for bad in (-1e-6, math.inf, math.nan):
        assert call(pd._h, gtol=bad) == EINVAL and b"gtol" in err()
        assert call(pd._h, ftol=bad) == EINVAL and b"ftol" in err()
    assert call(pd._h, theta=None) == EINVAL and call(pd._h, elbo=None) == EINVAL and b"NULL" in err()
    assert call(pd._h, W_=0, ld=0) == 0
    assert call(pd._h, n_rounds=0) == 0                                                   # the opening evaluation alone
    for kw in (dict(W_=n - 1), dict(W_=n - 1, ld=n - 1), dict(m=M - 1)):               # resume with another shape
        assert call(pd._h, resume=1, **kw) == EINVAL and b"resume" in err()
    assert call(pd._h, resume=1, n_elbo=3) == 0
    assert draw(pd._h) == 0
    torch.cuda.synchronize()
    assert int(ints[2].max()) == 2 and int(ints[2].min()) == 2 and int(ints[4].max()) <= 1
    assert draw(pd._h, n_draws=0) == EINVAL and b"n_draws" in err()
    assert draw(pd._h, ld_out=4 * n - 1) == EINVAL and b"ld_out" in err()
    assert draw(pd._h, W_=n - 1) == EINVAL and b"previous" in err()
    assert draw(pd._h, phi=None) == EINVAL and b"NULL" in err()
    nomodel = draws_mod.PriorDraws(priors=[pkg.Uniform(0, 1)] * model.D)
    assert call(nomodel._h) == EINVAL and b"no model" in err(nomodel) and draw(nomodel._h) == EINVAL and b"no model" in err(nomodel)
    d = torch.zeros((model.D, n), dtype=torch.float64, device="cuda")
    hist = torch.zeros((2, model.D, n), dtype=torch.float64, device="cuda")
    chol = torch.zeros((model.D * (model.D + 1) // 2, n), dtype=torch.float64, device="cuda")
    fit = lambda m, W_=n, ld=n, g=d.data_ptr(), nz=0: lib.octo_draws_pathfinder_fit_device(      # noqa: E731
        nomodel._h, W_, ld, m, ints[0].data_ptr(), ints[1].data_ptr(), hist.data_ptr(), hist.data_ptr(), d.data_ptr(), g, d.data_ptr(), d.data_ptr(), chol.data_ptr(),
        dbl[0].data_ptr(), ints[2].data_ptr(), nz, None, None, st)
    assert fit(0) == EINVAL and fit(9) == EINVAL and fit(2, ld=n - 1) == EINVAL and fit(2, g=None) == EINVAL and fit(2, nz=-1) == EINVAL
    assert fit(2, nz=2) == EINVAL                                                         # draws asked for without z and φ
    assert fit(2, W_=0) == 0
    with pytest.raises(ValueError):
        pd.pathfinder(tt.t())
    nomodel.close()
    # OCTO_ENOTSUP is for D > OCTO_DRAWS_PF_MAX_D = 64, and 64 is as far as octo_draws_create goes: no handle can carry D = 65
    assert draws_mod.PF_MAX_D == 64
    with pytest.raises(pkg.capi.OctoError) as ex:
        draws_mod.PriorDraws(priors=[pkg.Uniform(0, 1)] * 65)
    assert ex.value.status == EINVAL


# ---------------------------------------------------------------------------------------------------- 7. the driver
def test_gpu_pathfinder_device(pkg, case):
    import psis_reference as pr
    model = case["model"]
    kw = dict(N=cases.LBFGS_N_DRAWS, n_paths=cases.LBFGS_N_STARTS, seed=cases.LBFGS_SEED)      # n_draws = 1000 of 256 a path
    out = pkg.pathfinder_device(model, **kw)
    D, n, P = model.D, 1000, cases.LBFGS_N_STARTS
    assert out["theta"].shape == out["theta_t"].shape == (D, n) and out["logpost"].shape == out["path"].shape == (n,) and out["names"] == list(model.names)
    assert all(out[k].shape == (P,) for k in ("elbo", "elbo_iter", "n_fits", "status", "iters", "evals", "gnorm", "start_logpost", "path_logpost"))
    assert out["inv_hess_diag"].shape == out["path_theta_t"].shape == (D, P) and out["log_ratios"].shape == out["log_weights"].shape == (256 * P,)
    assert np.all(np.isfinite(out["logpost"])) and np.all(out["elbo_iter"][out["path"]] >= 0)      # path only names paths with a fit
    assert np.array_equal(out["start_logpost"], case["lp0"]) and not np.any(out["status"] == lref.ACTIVE)
    assert np.max(rel(model.ℓπcallback(out["theta_t"]), out["logpost"])) <= 1e-8
    again = pkg.pathfinder_device(model, **kw)
    assert all(np.array_equal(out[k], again[k], equal_nan=True) for k in out if isinstance(out[k], np.ndarray)) and out["pareto_k"] == again["pareto_k"]
    other = pkg.pathfinder_device(model, **dict(kw, n_elbo=3))
    assert np.array_equal(other["path_theta_t"], out["path_theta_t"]) and not np.array_equal(other["elbo"], out["elbo"])
    want = pr.psis_row(-out["log_ratios"])
    e_k, e_w = abs(out["pareto_k"] - want["pareto_k"]), np.max(rel(out["log_weights"][np.isfinite(want["lw"])], want["lw"][np.isfinite(want["lw"])]))
    print(f"driver: k̂ {out['pareto_k']:.4f}, best ELBO {out['elbo'].max():.6f}, {np.sum(out['elbo_iter'] >= 0)} of {P} paths with a fit, {np.unique(out['path']).size} paths "
          f"among the {n} draws, draws' ℓπ {out['logpost'].min():.3f} … {out['logpost'].max():.3f}; against psis_reference: k̂ {e_k:.3e}, log-weights {e_w:.3e}")
    assert np.array_equal(np.isfinite(out["log_weights"]), np.isfinite(want["lw"])) and e_k <= 1e-8 and e_w <= 1e-8
