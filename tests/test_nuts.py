"""
The no-U-turn sampler on the device (include/octofitter_hip_draws.h: octo_draws_nuts_device; host/draws.py: PriorDraws.nuts / nuts_step;
host/callers.py: hmc_warmup(max_depth=…), octofit_nuts_device) against its NumPy restatement (tests/nuts_reference.py) fed by the oracle's
callback, and against the conditions tests/test_nuts_reference.py establishes for the same seeds on the CPU.

Decisions (depth, n_leapfrog, diverged, accepted) are compared on DECIDED chains — those whose smallest decision margin in the restatement
exceeds 1e-6. Tolerances: θ_t, ℓπ and ℓ the project's oracle bar 1e-8 relative to max(1, |ref|); log_accept 1e-8 absolute; the warm-up's
adaptation outputs the bars of tests/test_adapt.py; Kolmogorov-Smirnov at the 0.1 % level.
"""
import ctypes as C
import math

import numpy as np
import pytest

import adapt_reference as aref
import draws_cases as cases
import nuts_reference as nuts
from draws_device import TRANS_BAR, close, draws_mod, hmc_model, host, mirror_priors, padded, same_bits, set_batch_invariant      # noqa: F401

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


def numpy_outputs(tt, out):
    """[θ_t, the seven outputs] as NumPy arrays (None stays None)"""
    return [tt.cpu().numpy()] + [None if out[k] is None else out[k].cpu().numpy() for k in OUTPUTS]


def columns(x, sel):
    return [None if a is None else a[..., sel] for a in x]


def against_the_restatement(got, r, start, what):
    """decisions on decided chains, values at the oracle bar, a chain that did not move keeps its bits"""
    tt, lp, ll, la, acc, depth, nleaf, div = got
    decided = r["margin"] > nuts.MARGIN
    for name, mine, theirs in (("accepted", acc != 0, r["accepted"]), ("depth", depth, r["depth"]), ("n_leapfrog", nleaf, r["n_leapfrog"]), ("diverged", div != 0, r["diverged"])):
        assert np.array_equal(mine[decided], theirs[decided]), (what, name, np.nonzero(decided & (mine != theirs))[0])
    assert set(np.unique(acc)) <= {0, 1} and set(np.unique(div)) <= {0, 1}
    same = decided
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)), initial=0.0))      # noqa: E731
    e_tt = rel(tt[:, same], r["theta_t"][:, same])
    with np.errstate(invalid="ignore"):
        e_lp = 0.0 if lp is None else rel(lp[same], r["logpost"][same])
        fin = same & np.isfinite(r["loglike"])
        e_ll = 0.0 if ll is None else rel(ll[fin], r["loglike"][fin])
        made = same & (r["n_leapfrog"] > 0)
        e_la = float(np.max(np.where(la[made] == r["log_accept"][made], 0.0, np.abs(la[made] - r["log_accept"][made])), initial=0.0))      # −Inf: every leaf diverged
    print(f"{what}: {np.sum(~decided)} of {decided.size} undecided; max errors — θ_t {e_tt:.3e}, ℓπ {e_lp:.3e}, ℓ {e_ll:.3e} (relative to max(1, |ref|)); log_accept {e_la:.3e}")
    assert e_tt <= 1e-8 and e_lp <= 1e-8 and e_ll <= 1e-8 and e_la <= 1e-8
    assert ll is None or np.array_equal(ll[same & ~fin], r["loglike"][same & ~fin])
    assert np.all(np.isnan(la[r["n_leapfrog"] == 0]))
    stay = acc == 0
    assert np.array_equal(tt[:, stay], start[:, stay], equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 1. one transition against the restatement
def test_gpu_one_transition_against_the_restatement(pkg, oracle, model_pd):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    W, ld = cases.ONE_W, cases.ONE_LD
    beta, eps, im = cases.one_inputs()
    start = pd.sample(cases.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
    r = cases.one_transition(oracle, start.cpu().numpy())
    cases.check_one_transition_is_decided(r)                                   # the condition on the seed, before the device runs
    buf, tt = padded(torch, start, ld)
    out = pd.nuts(tt, beta=torch.as_tensor(beta, device="cuda"), eps=torch.as_tensor(eps, device="cuda"), inv_mass=im, max_depth=cases.ONE_DEPTH,
                  n_rounds=(1 << cases.ONE_DEPTH) - 1, seed=cases.ONE_SEED, step=cases.ONE_STEP)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, W:]).all())                                  # nothing written beyond column W
    assert int(out["n_active"].item()) == 0
    against_the_restatement(numpy_outputs(tt, out), r, start.cpu().numpy(), "one transition")


# ---------------------------------------------------------------------------------------------------- 2. tree shapes
SHAPE_DEPTH, SHAPE_SEED = 3, 5
SHAPE_EPS_SMALL, SHAPE_EPS_LARGE = 0.01, 1.6


def test_gpu_tree_shapes(prior_pd):
    """ε small: every chain reaches max_depth, seven leaves. ε large: turns inside the first subtrees, turns of the tree, divergences."""
    import torch
    pd = prior_pd
    seen = set()
    for W in (1, 64, 257):
        start = pd.sample(SHAPE_SEED, 0, W, theta=False, logprior_t=False)[1]
        for eps in (SHAPE_EPS_SMALL, SHAPE_EPS_LARGE):
            r = nuts.nuts_transition(cases.STAT_PRIORS, start.cpu().numpy(), None, eps, cases.STAT_INV_MASS, SHAPE_DEPTH, SHAPE_SEED, 2)
            tt = start.clone()
            out = pd.nuts(tt, eps=eps, inv_mass=cases.STAT_INV_MASS, max_depth=SHAPE_DEPTH, n_rounds=(1 << SHAPE_DEPTH) - 1, seed=SHAPE_SEED, step=2)
            assert out["logpost"] is None and out["loglike"] is None and int(out["n_active"].item()) == 0
            got = numpy_outputs(tt, out)
            against_the_restatement(got, r, start.cpu().numpy(), f"W {W}, ε {eps}")
            depth, nleaf, div = got[5], got[6], got[7]
            if eps == SHAPE_EPS_SMALL:
                assert np.all(nleaf == 7) and np.all(depth == SHAPE_DEPTH) and not div.any() and np.all(got[4] == 1)
            else:
                decided = r["margin"] > nuts.MARGIN
                seen |= set(r["stop"][decided])
                assert np.all(nleaf >= 1) and np.all(nleaf <= 7)
                if W == 257:
                    assert np.any((depth == 1) & (div == 0))      # a turn at depth 1
    assert {nuts.STOP_TURN_SUBTREE, nuts.STOP_TURN_TREE, nuts.STOP_DIVERGED} <= seen, seen      # with ε small: STOP_MAX_DEPTH, the fourth


# ---------------------------------------------------------------------------------------------------- 3. invariance, resume and freezing
def run_rounds(torch, pd, start, beta, eps, im, cuts, chain0=0, ld=None, max_depth=cases.ONE_DEPTH, snapshots=None):
    """the transition of cases.ONE_SEED cut into calls of `cuts` rounds: [θ_t, outputs] at the end; snapshots: the same after every call"""
    W = start.shape[1]
    _buf, tt = padded(torch, start, ld or W)
    args = dict(beta=torch.as_tensor(beta, device="cuda"), eps=torch.as_tensor(eps, device="cuda"), inv_mass=im, max_depth=max_depth, seed=cases.ONE_SEED,
                step=cases.ONE_STEP, chain0=chain0)
    out = None
    for k, n in enumerate(cuts):
        out = pd.nuts(tt, n_rounds=n, resume=k > 0, out=out, **args)
        if snapshots is not None:
            snapshots.append((numpy_outputs(tt, out), int(out["n_active"].item())))
    return numpy_outputs(tt, out)


def test_gpu_invariance_resume_and_freezing(pkg, model_pd):
    import torch
    model, pd = model_pd
    W, total = cases.ONE_W, (1 << cases.ONE_DEPTH) - 1
    beta, eps, im = cases.one_inputs()
    start = pd.sample(cases.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
    dead = 7
    start[3, dead] = float("nan")                                                # a dead start among the others
    set_batch_invariant(pkg, model, 1)
    try:
        full = run_rounds(torch, pd, start, beta, eps, im, (total,))
        assert same_bits(full, run_rounds(torch, pd, start, beta, eps, im, (total,)))
        assert same_bits(full, run_rounds(torch, pd, start, beta, eps, im, (total,), ld=cases.ONE_LD))       # another leading dimension
        part = run_rounds(torch, pd, start[:, 20:41].contiguous(), beta[20:41], eps[20:41], im, (total,), chain0=20)      # chains 20 … 40 alone
        assert same_bits(columns(full, slice(20, 41)), part)
        snaps = []
        cut = run_rounds(torch, pd, start, beta, eps, im, (0,) + (1,) * total + (0,), snapshots=snaps)        # 0 + 1 + 1 + … + 0 rounds
        assert same_bits(full, cut)
        assert same_bits(full, run_rounds(torch, pd, start, beta, eps, im, (3, 0, 5, total - 8)))
        # a chain of m leaves ended in round m: from there on it is frozen, θ_t and every output keep their bits while the others build
        nleaf = full[6]
        assert len(set(nleaf)) >= 3 and nleaf.max() == total
        for rounds, (snap, n_active) in enumerate(snaps[:-1]):
            ended = nleaf <= rounds                                              # the dead start: from the opening on
            assert same_bits(columns(snap, ended), columns(full, ended)), rounds
            assert n_active == np.sum(~ended), rounds
        assert snaps[-1][1] == 0 and snaps[0][1] == W - 1
        # the dead start: its column is never written, no leaf, not accepted
        assert np.array_equal(full[0][:, dead], start.cpu().numpy()[:, dead], equal_nan=True) and np.isnan(full[0][3, dead])
        assert full[4][dead] == 0 and full[6][dead] == 0 and full[5][dead] == 0 and np.isnan(full[3][dead]) and full[7][dead] == 0
        # the other chains are what they are without it
        clean = start.clone()
        clean[3, dead] = 0.1
        others = np.arange(W) != dead
        assert same_bits(columns(full, others), columns(run_rounds(torch, pd, clean, beta, eps, im, (total,)), others))
    finally:
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 4. nuts_step and the warm-up
def test_gpu_nuts_step_reads_the_count_or_runs_every_round(pkg, model_pd):
    import torch
    model, pd = model_pd
    beta, eps, im = cases.one_inputs()
    start = pd.sample(cases.ONE_SEED, 0, cases.ONE_W, theta=False, logprior_t=False)[1]
    set_batch_invariant(pkg, model, 1)
    try:
        runs = []
        for check_from in (3, None, 0):
            tt = start.clone()
            res = pd.nuts_step(tt, beta=torch.as_tensor(beta, device="cuda"), eps=torch.as_tensor(eps, device="cuda"), inv_mass=im, max_depth=6, seed=cases.ONE_SEED,
                               step=cases.ONE_STEP, check_from=check_from)
            assert len(res) == 7
            runs.append([tt.cpu().numpy()] + [x.cpu().numpy() for x in res])
        assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])
        assert runs[0][6].max() > 7      # a tree beyond the first check
    finally:
        set_batch_invariant(pkg, model, 0)


WARM_W, WARM_ROUNDS, WARM_DEPTH, WARM_EPS, WARM_SEED = 192, 30, 4, 0.2, 77


def test_gpu_warmup_with_nuts_teacher_forced(pkg, prior_pd):
    """hmc_warmup(max_depth=4) on the prior: every round's adaptation outputs against tests/adapt_reference.py applied to the DEVICE's inputs
    of that round (the method of tests/test_adapt.py), the round's log_accept standing where dH stood."""
    import torch
    pd = prior_pd
    start = pd.sample(WARM_SEED, 0, WARM_W, theta=False, logprior_t=False)[1]
    record = []
    out = pkg.hmc_warmup(pd, start.clone(), WARM_ROUNDS, eps=WARM_EPS, seed=WARM_SEED, record=record, max_depth=WARM_DEPTH)
    torch.cuda.synchronize()
    flags = aref.round_flags(WARM_ROUNDS)
    assert len(record) == WARM_ROUNDS and out["step"] == WARM_ROUNDS and out["tree"].shape == (WARM_ROUNDS, 3)
    k, windows = 0, 0
    for r, rec in enumerate(record):
        k += 1
        assert (rec["in_window"], rec["first"], rec["last"]) == flags[r] and rec["k"] == k and rec["use_average"] == (r == WARM_ROUNDS - 1)
        la = rec["dH"].cpu().numpy()
        assert np.all(la[~np.isnan(la)] <= 0.0)                                 # the log of a mean of min(1, ·)
        state, a = aref.adapt_step(rec["state_in"].cpu().numpy(), la, rec["accepted"].cpu().numpy(), k)
        assert close(rec["state"].cpu().numpy(), state, TRANS_BAR) and close(rec["accept_stat"].cpu().numpy(), a, TRANS_BAR), r
        assert close(rec["eps_w"].cpu().numpy(), np.full(WARM_W, math.exp(state[0, 1 if rec["use_average"] else 0])), TRANS_BAR), r
        assert close(out["accept_stat"][r].cpu().numpy(), a[0], TRANS_BAR)
        if rec["in_window"] and rec["first"]:
            cases.check_moments(host(rec["mom"]), aref.exact_moments(rec["theta_t"].cpu().numpy()), ("round", r))
        if rec["last"]:
            windows += 1
            hm = host(rec["mom"])
            assert close(rec["inv_mass"].cpu().numpy(), aref.metric(hm[0][0], hm[2][0], rec["inv_mass_in"].cpu().numpy(), regularize=True), 1e-14, scale_one=False)
            assert close(rec["state_restart"].cpu().numpy(), aref.adapt_init(np.exp(rec["state"].cpu().numpy()[:, 1])), TRANS_BAR)
            k = 0
    tree = out["tree"].cpu().numpy()
    print(f"warm-up with NUTS: ε {WARM_EPS} -> {float(out['eps'][0]):.4f}; mean depth {tree[:, 0].mean():.2f}, mean leaves {tree[:, 1].mean():.2f}, divergences {int(tree[:, 2].sum())}")
    assert windows == 1 and np.all(tree[:, 0] <= WARM_DEPTH) and np.all(tree[:, 1] <= (1 << WARM_DEPTH) - 1) and not np.allclose(out["inv_mass"].cpu().numpy(), 1.0)


# ---------------------------------------------------------------------------------------------------- 5. stationarity on the device
@pytest.mark.parametrize("seed", cases.STAT_SEEDS)
def test_gpu_prior_is_stationary(prior_pd, seed):
    pd = prior_pd
    eps = cases.NUTS_STAT_EPS[0]
    tt = pd.sample(seed, 0, cases.STAT_W, theta=False, logprior_t=False)[1]
    start = tt.clone()
    leaves = []
    for step in range(cases.STAT_STEPS):
        _lp, _ll, _la, _acc, _depth, nleaf, _div = pd.nuts_step(tt, eps=eps, inv_mass=cases.STAT_INV_MASS, max_depth=cases.NUTS_STAT_DEPTH, seed=seed, step=step)
        leaves.append(float(nleaf.double().mean()))
    moved = float((tt != start).any(dim=0).double().mean())
    stat = cases.stationarity_statistics(tt.cpu().numpy())
    print(f"seed {seed} (ε {eps}, depth <= {cases.NUTS_STAT_DEPTH}): mean leaves {np.mean(leaves):.2f}, moved {moved:.3f}, max D_n {stat:.3e} (bar {cases.STAT_BAR:.3e})")
    assert stat < cases.STAT_BAR and moved >= 0.9, (seed, stat, moved)


# ---------------------------------------------------------------------------------------------------- 6. the driver and the arguments
def test_gpu_octofit_nuts_device(pkg, draws_mod, model_pd):
    model, pd = model_pd
    Cn, nw, ns, seed, D = 256, 40, 40, 61, model.D
    init = pd.sample(seed, 0, Cn, theta=False, logprior_t=False)[1].cpu().numpy()
    out = pkg.octofit_nuts_device(model, n_chains=Cn, n_warmup=nw, n_samples=ns, max_depth=5, init=init, seed=seed)
    assert out["samples"].shape == out["samples_t"].shape == (ns, D, Cn) and out["logpost"].shape == (ns, Cn)
    for k in ("accept_stat", "depth", "n_leapfrog", "diverged"):
        assert out[k].shape == (nw + ns,), k
    assert out["rhat"].shape == out["inv_mass"].shape == (D,) and np.all(np.isfinite(out["rhat"])) and np.all(out["inv_mass"] > 0) and out["eps"] > 0
    assert np.all(np.isfinite(out["samples_t"])) and np.all(np.isfinite(out["logpost"])) and out["state"]["step"] == nw + ns
    assert np.all((out["depth"] >= 0) & (out["depth"] <= 5)) and np.all((out["n_leapfrog"] >= 1) & (out["n_leapfrog"] <= 31)) and np.all(out["diverged"] >= 0)
    print(f"NUTS driver: ε {out['eps']:.4f}; sampling rounds — mean depth {out['depth'][nw:].mean():.2f}, mean leaves {out['n_leapfrog'][nw:].mean():.2f}, "
          f"divergences {int(out['diverged'][nw:].sum())} (warm-up {int(out['diverged'][:nw].sum())}), acceptance statistic {out['accept_stat'][nw:].mean():.3f}; "
          f"R̂ {out['rhat'].min():.3f} … {out['rhat'].max():.3f}")
    lp_cb = model.ℓπcallback(out["samples_t"][-1])                               # the recorded ℓπ is the callback's at the recorded states
    assert np.all(np.abs(lp_cb - out["logpost"][-1]) <= 1e-8 * np.maximum(1.0, np.abs(lp_cb)))


def test_gpu_nuts_argument_checks(pkg, draws_mod, model_pd, prior_pd):
    import torch
    model, pd = model_pd
    lib, EINVAL, W = pd.lib, pkg.capi.OCTO_EINVAL, 8
    tt = pd.sample(1, 0, W, theta=False, logprior_t=False)[1]
    before = tt.clone()
    acc = torch.zeros(W, dtype=torch.int32, device="cuda")
    lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, W_=W, ld=W, eps=0.1, depth=3, rounds=0, resume=0, d_eps=None, d_lp=None, d_tt=tt.data_ptr(), d_acc=acc.data_ptr(), seed=0):
        return lib.octo_draws_nuts_device(h, seed, 0, 0, W_, ld, d_tt, None, d_eps, eps, None, depth, rounds, resume, d_lp, None, None, d_acc, None, None, None, None, st)

    assert call(None) == EINVAL
    assert call(pd._h, depth=0) == EINVAL and b"max_depth" in lib.octo_draws_last_error(pd._h)
    assert call(pd._h, depth=11) == EINVAL and call(pd._h, rounds=-1) == EINVAL
    assert call(pd._h, W_=-1) == EINVAL and call(pd._h, ld=W - 1) == EINVAL
    for eps in (0.0, -0.1, math.inf, math.nan):
        assert call(pd._h, eps=eps) == EINVAL
    assert call(pd._h, d_tt=None) == EINVAL and call(pd._h, d_acc=None) == EINVAL
    fresh = draws_mod.PriorDraws(model)
    assert call(fresh._h, resume=1) == EINVAL and b"resume" in lib.octo_draws_last_error(fresh._h)      # nothing to resume
    fresh.close()
    assert call(pd._h, eps=math.nan, d_eps=lp.data_ptr()) == 0      # ε per chain: the scalar is not looked at (ε = 0 everywhere: nothing moves)
    assert call(pd._h, eps=math.nan, d_eps=lp.data_ptr(), rounds=2, resume=1) == 0
    for other in (dict(depth=4), dict(W_=W - 1), dict(seed=1)):      # resume with another shape or another transition
        assert call(pd._h, resume=1, **other) == EINVAL
    assert call(pd._h, W_=0, ld=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(tt, before) and int(acc.sum()) == 0
    nomodel = prior_pd
    t5 = nomodel.sample(1, 0, W, theta=False, logprior_t=False)[1]
    assert call(nomodel._h, d_lp=lp.data_ptr(), d_tt=t5.data_ptr()) == EINVAL and b"no model" in lib.octo_draws_last_error(nomodel._h)
    assert call(nomodel._h, d_tt=t5.data_ptr(), rounds=7) == 0
    with pytest.raises(ValueError):
        pd.nuts_step(tt.t(), eps=0.1)
    with pytest.raises(ValueError):
        pd.nuts_step(tt)
    torch.cuda.synchronize()
