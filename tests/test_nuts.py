"""
The no-U-turn sampler on the device (include/octofitter_hip_draws.h: octo_draws_nuts_device; host/draws.py: PriorDraws.nuts / nuts_step;
host/callers.py: hmc_warmup(max_depth=…), octofit_nuts_device) against its NumPy restatement (tests/nuts_reference.py) fed by the oracle's
callback, and against the conditions tests/test_nuts_reference.py establishes for the same seeds on the CPU.

Decisions (depth, n_leapfrog, diverged, accepted) are compared on DECIDED chains — those whose smallest decision margin in the restatement
exceeds 1e-6. Tolerances: θ_t, ℓπ and ℓ the project's oracle bar 1e-8 relative to max(1, |ref|); log_accept 1e-8 absolute; the deep transition
(1023 leapfrogs) cases.DEEP_BAR = max(1e-8, 100·s), s the restatement's own sensitivity to one ulp of the starts; the warm-up's adaptation
outputs the bars of tests/test_adapt.py; Kolmogorov-Smirnov at the 0.1 % level.
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


def against_the_restatement(got, r, start, what, bar=1e-8):
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
    assert e_tt <= bar and e_lp <= bar and e_ll <= bar and e_la <= bar
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


def test_gpu_deep_transition_against_the_restatement(pkg, oracle, model_pd):
    """max_depth = 10, ε scaled per chain so that every depth from 2 to 10 occurs: subtrees of up to 512 leaves, every checkpoint slot
    popc(n >> 1) = 0 … 8 stored and walked back, leaf numbers up to 1023 in the generator's counter, 1023 rounds in one call."""
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    W, ld, total = cases.ONE_W, cases.ONE_LD, (1 << cases.DEEP_DEPTH) - 1
    beta, eps, im = cases.deep_inputs()
    start = pd.sample(cases.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
    r = cases.deep_transition(oracle, start.cpu().numpy())
    cases.check_deep_transition_is_decided(r)                                  # the conditions on the seed, before the device runs
    buf, tt = padded(torch, start, ld)
    out = pd.nuts(tt, beta=torch.as_tensor(beta, device="cuda"), eps=torch.as_tensor(eps, device="cuda"), inv_mass=im, max_depth=cases.DEEP_DEPTH,
                  n_rounds=total, seed=cases.ONE_SEED, step=cases.ONE_STEP)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, W:]).all())                                  # nothing written beyond column W
    assert int(out["n_active"].item()) == 0
    against_the_restatement(numpy_outputs(tt, out), r, start.cpu().numpy(), "deep transition", bar=cases.DEEP_BAR)


def without(r, col):
    """the restatement's result without one chain"""
    return {k: (np.delete(v, col, axis=-1) if isinstance(v, np.ndarray) else v) for k, v in r.items()}


@pytest.mark.parametrize("route", ("fused", "throughput"))
def test_gpu_one_transition_at_577_chains(pkg, oracle, draws_mod, route):
    """W = 577 with the model, on both kernel families of the callback. What decides the route is small_eligible (csrc/octo_api.hip): the
    fused launch k_small<MODEL> takes a batch with W·P <= the limit, and the limit of a whole single-planet callback is
    max(small_w, small_w_model) = max(512, 768) — so 577 chains of the one-planet test model take the FUSED launch by default, not the
    throughput kernels. An explicit octo_ctx_set_small_batch holds for the callback too (small_w_model = 0): with the limit 0 every call goes
    through k_model_fwd, k_main and k_finish. Both run here, on a model of the test's own (the limit cannot be taken back).
    Chain BIG_DEAD starts with a NaN coordinate: its column is not written and it makes no leaf."""
    import torch
    model = hmc_model(pkg)
    pd = None
    try:
        if route == "throughput":
            fn = model.ln_like
            fn._check(fn.lib.octo_ctx_set_small_batch(fn._ctx, 0), "octo_ctx_set_small_batch")
        pd = draws_mod.PriorDraws(model)
        W, ld, dead, total = cases.BIG_W, cases.BIG_LD, cases.BIG_DEAD, (1 << cases.BIG_DEPTH) - 1
        beta, eps, im = cases.one_inputs(W)
        start = pd.sample(cases.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
        start[3, dead] = float("nan")
        start_h = start.cpu().numpy()
        r = nuts.nuts_transition(cases.MODEL_PRIORS, start_h, beta, eps, im, cases.BIG_DEPTH, cases.ONE_SEED, cases.ONE_STEP,
                                 logpost=cases.oracle_logpost(oracle, cases.oracle_model(oracle)))
        print(f"W {W} ({route}): {cases.tree_summary(r)}")
        assert np.mean(r["margin"] <= nuts.MARGIN) <= cases.ONE_UNDECIDED and r["stop"][dead] == nuts.STOP_DEAD, "condition on the seed (the reference alone)"
        buf, tt = padded(torch, start, ld)
        out = pd.nuts(tt, beta=torch.as_tensor(beta, device="cuda"), eps=torch.as_tensor(eps, device="cuda"), inv_mass=im, max_depth=cases.BIG_DEPTH,
                      n_rounds=total, seed=cases.ONE_SEED, step=cases.ONE_STEP)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:, W:]).all()) and int(out["n_active"].item()) == 0
        got = numpy_outputs(tt, out)
        others = np.arange(W) != dead
        against_the_restatement(columns(got, others), without(r, dead), start_h[:, others], f"W {W} ({route})")
        # the dead start: its column is never written, no leaf, not accepted
        assert np.array_equal(got[0][:, dead], start_h[:, dead], equal_nan=True) and np.isnan(got[0][3, dead])
        assert got[4][dead] == 0 and got[6][dead] == 0 and got[5][dead] == 0 and np.isnan(got[3][dead]) and got[7][dead] == 0
    finally:
        if pd is not None:
            pd.close()
        model.close()


# ---------------------------------------------------------------------------------------------------- 2. tree shapes
SHAPE_DEPTH, SHAPE_SEED = 3, 5
SHAPE_EPS_SMALL, SHAPE_EPS_LARGE = 0.01, 1.6


SHAPE_DEPTHS = (1, 2, SHAPE_DEPTH)      # at depth 1 the first leaf completes the tree


def test_gpu_tree_shapes(prior_pd):
    """ε small: every chain reaches max_depth, 2^max_depth − 1 leaves (1, 3, 7). ε large: turns inside the first subtrees, turns of the tree,
    divergences."""
    import torch
    pd = prior_pd
    seen = set()
    for W in (1, 64, 257):
        start = pd.sample(SHAPE_SEED, 0, W, theta=False, logprior_t=False)[1]
        for max_depth in SHAPE_DEPTHS:
            total = (1 << max_depth) - 1
            for eps in (SHAPE_EPS_SMALL, SHAPE_EPS_LARGE):
                r = nuts.nuts_transition(cases.STAT_PRIORS, start.cpu().numpy(), None, eps, cases.STAT_INV_MASS, max_depth, SHAPE_SEED, 2)
                tt = start.clone()
                out = pd.nuts(tt, eps=eps, inv_mass=cases.STAT_INV_MASS, max_depth=max_depth, n_rounds=total, seed=SHAPE_SEED, step=2)
                assert out["logpost"] is None and out["loglike"] is None and int(out["n_active"].item()) == 0
                got = numpy_outputs(tt, out)
                against_the_restatement(got, r, start.cpu().numpy(), f"W {W}, depth <= {max_depth}, ε {eps}")
                depth, nleaf, div = got[5], got[6], got[7]
                if eps == SHAPE_EPS_SMALL:
                    assert np.all(nleaf == total) and np.all(depth == max_depth) and not div.any() and np.all(got[4] == 1)
                else:
                    decided = r["margin"] > nuts.MARGIN
                    assert np.all(nleaf >= 1) and np.all(nleaf <= total)
                    if max_depth == SHAPE_DEPTH:
                        seen |= set(r["stop"][decided])
                        if W == 257:
                            assert np.any((depth == 1) & (div == 0))      # a turn at depth 1
    assert {nuts.STOP_TURN_SUBTREE, nuts.STOP_TURN_TREE, nuts.STOP_DIVERGED} <= seen, seen      # with ε small: STOP_MAX_DEPTH, the fourth


@pytest.mark.parametrize("D", cases.DIM_DS)
def test_gpu_dimensions_and_a_null_mass(pkg, draws_mod, D):
    """D = 1 and D = 64 (the largest a handle takes), each with a metric and with inv_mass = None (= 1), to depth 7"""
    import torch
    priors = cases.dim_priors(D)
    eps, im = cases.dim_inputs(D)
    W, ld, total = cases.DIM_W, cases.DIM_LD, (1 << cases.DIM_DEPTH) - 1
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, priors))
    try:
        start = pd.sample(cases.DIM_SEED, 0, W, theta=False, logprior_t=False)[1]
        assert tuple(start.shape) == (D, W)
        for mass in (im, None):
            what = f"D {D}, inv_mass {'given' if mass is not None else 'None'}"
            r = nuts.nuts_transition(priors, start.cpu().numpy(), None, eps, mass, cases.DIM_DEPTH, cases.DIM_SEED, cases.DIM_STEP)
            decided = r["margin"] > nuts.MARGIN
            print(f"{what}: {cases.tree_summary(r)}")
            assert np.mean(~decided) <= cases.ONE_UNDECIDED and len(set(r["depth"][decided])) >= cases.DIM_DEPTHS, "condition on the seed (the reference alone)"
            buf, tt = padded(torch, start, ld)
            out = pd.nuts(tt, eps=torch.as_tensor(eps, device="cuda"), inv_mass=mass, max_depth=cases.DIM_DEPTH, n_rounds=total, seed=cases.DIM_SEED, step=cases.DIM_STEP)
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[:, W:]).all()) and int(out["n_active"].item()) == 0
            against_the_restatement(numpy_outputs(tt, out), r, start.cpu().numpy(), what)
    finally:
        pd.close()


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


DEEP_CUTS = ((500, 523), (0, 16, 1, 1006, 0))      # a cut inside the subtree of 256 leaves; an empty opening call, a cut one leaf into the subtree of 16, the next a round on, an empty last call


def test_gpu_deep_resume_and_freezing(pkg, model_pd):
    """the deep transition of test_gpu_deep_transition_against_the_restatement cut into calls, and a slice of its chains alone: the same bits"""
    import torch
    model, pd = model_pd
    W, total = cases.ONE_W, (1 << cases.DEEP_DEPTH) - 1
    beta, eps, im = cases.deep_inputs()
    start = pd.sample(cases.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
    deep = dict(ld=cases.ONE_LD, max_depth=cases.DEEP_DEPTH)
    set_batch_invariant(pkg, model, 1)
    try:
        full = run_rounds(torch, pd, start, beta, eps, im, (total,), **deep)
        nleaf = full[6]
        assert nleaf.max() == total and len(set(nleaf)) >= 8
        for cuts in DEEP_CUTS:
            assert sum(cuts) == total
            snaps = []
            assert same_bits(full, run_rounds(torch, pd, start, beta, eps, im, cuts, snapshots=snaps, **deep)), cuts
            # a chain of m leaves ended in round m: from there on θ_t and every output keep their bits while the others build
            for rounds, (snap, n_active) in zip(np.cumsum(cuts), snaps):
                ended = nleaf <= rounds
                assert same_bits(columns(snap, ended), columns(full, ended)), (cuts, rounds)
                assert n_active == np.sum(~ended), (cuts, rounds)
        part = run_rounds(torch, pd, start[:, 20:41].contiguous(), beta[20:41], eps[20:41], im, (total,), chain0=20, max_depth=cases.DEEP_DEPTH)      # chains 20 … 40 alone
        assert same_bits(columns(full, slice(20, 41)), part)
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
