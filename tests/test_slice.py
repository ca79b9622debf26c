"""
The slice sampler on the device (include/octofitter_hip_draws.h: octo_draws_slice_device; host/draws.py: PriorDraws.slice / slice_step;
host/callers.py: octofit_pt_device(explorer="slice")) against its NumPy restatement (tests/slice_reference.py) fed by the oracle's callback,
and against the conditions tests/test_slice_reference.py establishes for the same seeds on the CPU (tests/slice_cases.py states them).

The counts and the status are compared on DECIDED chains — those whose smallest comparison margin in the restatement exceeds 1e-6.
Tolerances: with the model θ_t, ℓπ and ℓ at the project's oracle bar 1e-8 relative to max(1, |ref|); on handles without a model θ_t at the
device-transcendental bar TRANS_BAR = 1e-11; Kolmogorov-Smirnov at the 0.1 % level.
"""
import ctypes as C
import math

import numpy as np
import pytest

import draws_cases as cases
import slice_cases as sc
import slice_reference as sl
from draws_device import TRANS_BAR, differing, draws_mod, hmc_model, mirror_priors, padded, set_batch_invariant      # noqa: F401

pytestmark = pytest.mark.gpu
KEYS = ("theta_t",) + sc.OUTPUTS


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


def on_host(tt, out):
    """θ_t and the seven outputs by name as NumPy arrays (None stays None)"""
    return dict(theta_t=tt.cpu().numpy(), **{k: None if out[k] is None else out[k].cpu().numpy() for k in sc.OUTPUTS})


def same(a, b, cols=slice(None)):
    """the keys under which two results do not hold the same bits in the columns cols (None equal to None)"""
    return differing({k: v for k, v in a.items() if v is not None}, b, [k for k in KEYS if a[k] is not None], cols) + [k for k in KEYS if (a[k] is None) != (b[k] is None)]


def against_the_restatement(got, r, start, what, bar):
    """the counts and the status on decided chains, the values at the bar, a coordinate that did not move keeps its bits"""
    decided = r["margin"] > sl.MARGIN
    for k in sc.COUNTS:
        assert np.array_equal(got[k][decided], r[k][decided]), (what, k, np.nonzero(decided & (got[k] != r[k]))[0])
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)), initial=0.0))      # noqa: E731
    alive = decided & (r["status"] != sl.DEAD)
    e_tt = rel(got["theta_t"][:, alive], r["theta_t"][:, alive])
    e_lp = e_ll = 0.0
    if got["logpost"] is not None:
        with np.errstate(invalid="ignore"):
            e_lp = rel(got["logpost"][alive], r["logpost"][alive])
            fin = alive & np.isfinite(r["loglike"])
            e_ll = rel(got["loglike"][fin], r["loglike"][fin])
            assert np.array_equal(got["loglike"][alive & ~fin], r["loglike"][alive & ~fin])
    print(f"{what}: {np.sum(~decided)} of {decided.size} undecided; max errors — θ_t {e_tt:.3e}, ℓπ {e_lp:.3e}, ℓ {e_ll:.3e} (relative to max(1, |ref|), bar {bar:.0e})")
    assert e_tt <= bar and e_lp <= bar and e_ll <= bar
    stay = decided[None, :] & ((r["theta_t"] == start) | np.isnan(start))
    assert np.array_equal(got["theta_t"][stay], start[stay], equal_nan=True)
    dead = decided & (r["status"] == sl.DEAD)
    assert np.array_equal(got["theta_t"][:, dead], start[:, dead], equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 1. two transitions against the restatement
def test_gpu_two_transitions_against_the_restatement(pkg, oracle, model_pd):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    W, ld = sc.ONE_W, sc.ONE_LD
    assert ld == W + 5
    beta = torch.as_tensor(sc.one_betas(), device="cuda")
    start = pd.sample(sc.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
    r1 = sc.first_transition(oracle, start.cpu().numpy())
    print(f"first transition: {sc.summary(r1)}")
    assert sc.undecided(r1) <= cases.ONE_UNDECIDED, "condition on the seed (the reference alone)"      # before the device runs
    buf, tt = padded(torch, start, ld)
    out = pd.slice_step(tt, beta=beta, w=sc.DEFAULT_W, p=sc.DEFAULT_P, n_passes=1, seed=sc.ONE_SEED, step=sc.ONE_STEP)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, W:]).all())                                  # nothing written beyond column W
    assert int(out["n_active"].item()) == 0
    against_the_restatement(on_host(tt, out), r1, start.cpu().numpy(), "first transition (defaults)", 1e-8)
    # the second transition: per-coordinate widths of a fraction of the prior draws' deviation, from where the device stands
    start2 = tt.clone()
    r2 = sc.second_transition(oracle, start2.cpu().numpy())
    sc.check_model_transitions(r1, r2)                                          # the conditions on the seed, before the device runs again
    out2 = pd.slice_step(tt, beta=beta, w=sc.narrow_widths().copy(), p=sc.DEFAULT_P, n_passes=1, seed=sc.ONE_SEED, step=sc.ONE_STEP + 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:, W:]).all()) and int(out2["n_active"].item()) == 0
    against_the_restatement(on_host(tt, out2), r2, start2.cpu().numpy(), "second transition (narrow widths)", 1e-8)


# ---------------------------------------------------------------------------------------------------- 2. the edges, on handles without a model
@pytest.mark.parametrize("name", sc.EDGES)
def test_gpu_edges_against_the_restatement(pkg, draws_mod, name):
    """W = 1, 63, 65 and 257, D = 1 and 64, p = 0, max_shrink = 2, one width per coordinate, a start with a NaN coordinate"""
    import torch
    D, W, _w, p, n_passes, max_shrink, nan_chain, _shows = sc.EDGES[name]
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, sc.edge_priors(name)))
    try:
        start = pd.sample(sc.EDGE_SEED, 0, W, theta=False, logprior_t=False)[1]
        assert tuple(start.shape) == (D, W)
        start_h = sc.with_nan(start.cpu().numpy(), nan_chain, D)
        r = sc.edge_transition(name, start_h)
        sc.check_edge(name, r)                                                  # the conditions on the seed, before the device runs
        buf, tt = padded(torch, start_h, W + 5)
        out = pd.slice_step(tt, w=sc.edge_width(name), p=p, n_passes=n_passes, max_shrink=max_shrink, seed=sc.EDGE_SEED, step=sc.EDGE_STEP)
        torch.cuda.synchronize()
        assert out["logpost"] is None and out["loglike"] is None and int(out["n_active"].item()) == 0
        assert bool(torch.isnan(buf[:, W:]).all())
        got = on_host(tt, out)
        against_the_restatement(got, r, start_h, name, TRANS_BAR)
        if nan_chain is not None:      # the dead start: its column is never written, nothing is counted
            assert got["status"][nan_chain] == sl.DEAD and got["n_eval"][nan_chain] == 0 and np.isnan(got["theta_t"][D // 2, nan_chain])
        if max_shrink == 2:
            assert got["n_stuck"].sum() > 0
    finally:
        pd.close()


# ---------------------------------------------------------------------------------------------------- 3. invariance, resume and freezing
TOTAL = 400      # rounds: more than the longest chain of the first transition takes (the restatement's count is asserted below)


def run_rounds(torch, pd, start, beta, cuts, chain0=0, ld=None, snapshots=None):
    """the first transition of sc.ONE_SEED cut into calls of `cuts` rounds: the result at the end; snapshots: (result, n_active) after every call"""
    W = start.shape[1]
    _buf, tt = padded(torch, start, ld or W)
    args = dict(beta=torch.as_tensor(beta, device="cuda"), w=sc.DEFAULT_W, p=sc.DEFAULT_P, n_passes=1, seed=sc.ONE_SEED, step=sc.ONE_STEP, chain0=chain0)
    out = None
    for k, n in enumerate(cuts):
        out = pd.slice(tt, n_rounds=n, resume=k > 0, out=out, **args)
        if snapshots is not None:
            snapshots.append((on_host(tt, out), int(out["n_active"].item())))
    return on_host(tt, out)


def test_gpu_invariance_resume_and_freezing(pkg, model_pd):
    import torch
    model, pd = model_pd
    W = sc.ONE_W
    beta = sc.one_betas()
    start = pd.sample(sc.ONE_SEED, 0, W, theta=False, logprior_t=False)[1]
    dead = 7
    start[3, dead] = float("nan")                                                # a dead start among the others
    set_batch_invariant(pkg, model, 1)
    try:
        full = run_rounds(torch, pd, start, beta, (TOTAL,))
        assert np.all(full["status"][np.arange(W) != dead] == sl.DONE) and full["n_eval"].max() < TOTAL and full["status"][dead] == sl.DEAD
        assert not same(full, run_rounds(torch, pd, start, beta, (TOTAL,)))                                   # run to run
        assert not same(full, run_rounds(torch, pd, start, beta, (TOTAL,), ld=sc.ONE_LD))                     # another leading dimension
        part = run_rounds(torch, pd, start[:, 20:41].contiguous(), beta[20:41], (TOTAL,), chain0=20)          # chains 20 … 40 alone
        assert not [k for k in KEYS if not np.array_equal(part[k], full[k][..., 20:41], equal_nan=True)]
        assert not same(full, run_rounds(torch, pd, start, beta, (150, 250)))                                 # a + b
        cuts = (0, 1, 1, 37, 0, 61) + (50,) * 6
        assert sum(cuts) == TOTAL
        snaps = []
        assert not same(full, run_rounds(torch, pd, start, beta, cuts, snapshots=snaps))
        # a chain of m evaluations ended in round m: from there on it is frozen, θ_t and every output keep their bits while the others go on
        assert len(set(full["n_eval"])) >= 10
        for rounds, (snap, n_active) in zip(np.cumsum(cuts), snaps):
            ended = full["n_eval"] <= rounds                                     # the dead start: from the opening on
            ended[dead] = True
            assert not same(snap, full, ended), rounds
            assert np.all(snap["status"][~ended] == sl.ACTIVE) and n_active == np.sum(~ended), rounds
        assert snaps[0][1] == W - 1 and snaps[-1][1] == 0
        # the dead start: its column is never written, nothing counted
        assert np.array_equal(full["theta_t"][:, dead], start.cpu().numpy()[:, dead], equal_nan=True) and full["n_eval"][dead] == 0 and full["n_shrink"][dead] == 0
        # the other chains are what they are without it
        clean = start.clone()
        clean[3, dead] = 0.1
        others = np.arange(W) != dead
        assert not same(full, run_rounds(torch, pd, clean, beta, (TOTAL,)), others)
    finally:
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 4. stationarity on the device
@pytest.mark.parametrize("w", (sc.STAT_WIDTH, sc.DEFAULT_W))
@pytest.mark.parametrize("seed", cases.STAT_SEEDS)
def test_gpu_prior_is_stationary(prior_pd, seed, w):
    pd = prior_pd
    tt = pd.sample(seed, 0, cases.STAT_W, theta=False, logprior_t=False)[1]
    start = tt.clone()
    evals = []
    for step in range(sc.STAT_TRANSITIONS):
        out = pd.slice_step(tt, w=w, p=sc.DEFAULT_P, n_passes=1, seed=seed, step=step)
        assert int(out["n_active"].item()) == 0 and int(out["n_stuck"].sum()) == 0
        evals.append(float(out["n_eval"].double().mean()))
    moved = float((tt != start).all(dim=0).double().mean())
    stat = cases.stationarity_statistics(tt.cpu().numpy())
    print(f"seed {seed}, w {w}: mean evaluations {np.mean(evals):.1f} a transition, moved in every coordinate {moved:.3f}, max D_n {stat:.3e} (bar {cases.STAT_BAR:.3e})")
    assert stat < cases.STAT_BAR and moved >= 0.99, (seed, stat, moved)


@pytest.mark.parametrize("seed", cases.POST_SEEDS)
def test_gpu_posterior_is_stationary(pkg, model_pd, seed):
    """β = 1: a batch of rejection samples pushed through slice transitions stays within the two-sample bar of a second batch. The widths
    are twice the posterior deviation of the second batch (two digits, as cases.posterior_inv_mass rounds its variances)."""
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    a, b = (model.link(pd.rejection(seed, cases.POST_N, first=first)["samples"]) for first in cases.POST_FIRST)
    widths = 2.0 * np.sqrt(cases.posterior_inv_mass(b))

    def step_fn(tt, step):
        t = torch.as_tensor(tt, device="cuda").contiguous()
        out = pd.slice_step(t, w=widths, p=sc.DEFAULT_P, n_passes=1, seed=seed, step=step)
        assert int(out["n_active"].item()) == 0
        return t.cpu().numpy(), (out["status"] == sl.DONE).cpu().numpy()

    cases.check_posterior_stationary(a, b, step_fn, f"seed {seed} (device, slice)")


# ---------------------------------------------------------------------------------------------------- 5. the driver and the arguments
def test_gpu_octofit_pt_device_with_the_slice_explorer(pkg, model_pd):
    import torch
    model, _pd = model_pd
    T, Cn, R, D = 4, 8, 4, model.D
    set_batch_invariant(pkg, model, 1)
    try:
        runs = [pkg.octofit_pt_device(model, T, Cn, R, explorer="slice", slice_w=2.0, slice_p=3, n_passes=1, seed=5) for _ in range(2)]
    finally:
        set_batch_invariant(pkg, model, 0)
    a, b = runs
    assert set(a) == {"samples", "samples_t", "logpost", "slice_evals", "swap_acceptance", "betas", "names", "state"}
    for k in ("samples", "samples_t", "logpost", "slice_evals", "swap_acceptance"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.array_equal(a["state"]["theta_t"], b["state"]["theta_t"]) and np.array_equal(a["state"]["slot2rep"], b["state"]["slot2rep"])
    assert a["samples_t"].shape == (R, D, Cn) and a["logpost"].shape == (R, Cn) and a["slice_evals"].shape == (T,)
    assert np.all(np.isfinite(a["slice_evals"])) and np.all(a["slice_evals"] > 0)
    print(f"PT with the slice explorer: evaluations per replica per round by temperature {np.round(a['slice_evals'], 1)}; swap acceptance {np.round(a['swap_acceptance'], 2)}")
    for r in range(R):      # the recorded ℓπ is the callback's at the recorded states
        lp = model.logpost_device(torch.as_tensor(a["samples_t"][r], device="cuda").contiguous(), grad=False)[0].cpu().numpy()
        assert np.all(np.abs(lp - a["logpost"][r]) <= 1e-8 * np.maximum(1.0, np.abs(lp))), r
    default = pkg.octofit_pt_device(model, T, Cn, 2, seed=5)
    assert list(default) == ["samples", "samples_t", "logpost", "hmc_acceptance", "swap_acceptance", "eps", "betas", "names", "state"]
    with pytest.raises(ValueError):
        pkg.octofit_pt_device(model, T, Cn, 2, explorer="walk")


def test_gpu_slice_argument_checks(pkg, draws_mod, model_pd, prior_pd):
    import torch
    model, pd = model_pd
    lib, EINVAL, W = pd.lib, pkg.capi.OCTO_EINVAL, 8
    tt = pd.sample(1, 0, W, theta=False, logprior_t=False)[1]
    lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    width = torch.full((model.D,), 0.5, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, W_=W, ld=W, w=1.0, p=3, passes=1, shrink=8, rounds=0, resume=0, d_w=None, d_lp=None, d_tt=tt.data_ptr(), seed=0, step=0, chain0=0):
        return lib.octo_draws_slice_device(h, seed, step, chain0, W_, ld, d_tt, None, d_w, w, p, passes, shrink, rounds, resume, d_lp, None, None, None, None, None, None, None, st)

    assert call(None) == EINVAL
    for w in (0.0, -1.0, math.inf, math.nan):
        assert call(pd._h, w=w) == EINVAL and b"w must be" in lib.octo_draws_last_error(pd._h)
    assert call(pd._h, p=-1) == EINVAL and call(pd._h, p=9) == EINVAL and b"p must be" in lib.octo_draws_last_error(pd._h)
    assert call(pd._h, shrink=0) == EINVAL and call(pd._h, shrink=65) == EINVAL and b"max_shrink" in lib.octo_draws_last_error(pd._h)
    assert call(pd._h, passes=0) == EINVAL and call(pd._h, passes=1025) == EINVAL and call(pd._h, rounds=-1) == EINVAL
    assert call(pd._h, W_=-1) == EINVAL and call(pd._h, ld=W - 1) == EINVAL and call(pd._h, d_tt=None) == EINVAL
    fresh = draws_mod.PriorDraws(model)
    assert call(fresh._h, resume=1) == EINVAL and b"resume" in lib.octo_draws_last_error(fresh._h)      # nothing to resume
    fresh.close()
    assert call(pd._h, w=math.nan, d_w=width.data_ptr()) == 0      # a width per coordinate: the scalar is not looked at
    assert call(pd._h, w=math.nan, d_w=width.data_ptr(), rounds=3, resume=1) == 0
    for other in (dict(p=2), dict(W_=W - 1), dict(ld=W + 1), dict(passes=2), dict(shrink=9), dict(seed=1), dict(step=1), dict(chain0=1)):      # another shape or another transition
        assert call(pd._h, w=math.nan, d_w=width.data_ptr(), resume=1, **other) == EINVAL, other
    assert call(pd._h, W_=0, ld=0) == 0
    assert call(pd._h, resume=1) == EINVAL                         # the empty call left nothing to resume
    nomodel = prior_pd
    t5 = nomodel.sample(1, 0, W, theta=False, logprior_t=False)[1]
    assert call(nomodel._h, d_lp=lp.data_ptr(), d_tt=t5.data_ptr()) == EINVAL and b"no model" in lib.octo_draws_last_error(nomodel._h)
    assert call(nomodel._h, d_tt=t5.data_ptr(), rounds=5) == 0
    with pytest.raises(ValueError):
        pd.slice_step(tt.t())
    with pytest.raises(ValueError):
        pd.slice_step(tt, rounds_per_call=0)
    torch.cuda.synchronize()
