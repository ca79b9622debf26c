"""
The parallel-tempering statistics on the device (include/octofitter_hip_draws.h: octo_draws_pt_stats_device, octo_draws_pt_schedule_device;
host/draws.py: PriorDraws.pt_state / pt_stats / pt_schedule; host/callers.py: octofit_pigeons_device) against their NumPy restatement
(tests/pt_reference.py), which tests/test_pt_reference.py pins by meaning on the CPU; tests/pt_cases.py holds the inputs and the bars.

Counts, maxima, leg and restarts are compared exactly; the sums, the rates, Λ, β* and the log evidence at the project's device-transcendental
bar TRANS_BAR = 1e-11 relative to max(1, |ref|) — the restatement sums in the device's order, so what is left is the last bits of exp and
log. The schedule cases keep their decision margins (test_pt_reference.py asserts it), so the interval a target falls in is decided.
"""
import ctypes as C
import math

import numpy as np
import pytest

import draws_cases as cases
import pt_cases as pc
import pt_reference as pt
from draws_device import TRANS_BAR, draws_mod, hmc_model, mirror_priors, set_batch_invariant      # noqa: F401

pytestmark = pytest.mark.gpu
EXACT = (pt.N, pt.NF, pt.MF, pt.NB, pt.MB)
SUMS = (pt.A, pt.SF, pt.SB)


@pytest.fixture(scope="module")
def prior_pd(pkg, draws_mod):
    """a handle without a model: the two calls need none"""
    h = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.STAT_PRIORS))
    yield h
    h.close()


@pytest.fixture(scope="module")
def model(pkg):
    m = hmc_model(pkg)
    yield m
    m.close()


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def near(got, want):
    """the largest |got − want|/max(1, |want|) over the finite entries of want; the others (NaN, ±Inf) must be the same values"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (got[~fin], want[~fin])
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])), initial=0.0))


def run_device(pd, T, Cn, swapped=False, alias=True):
    """the sequence of pt_cases.reference on the device: everything it returns, by the same names, as NumPy arrays"""
    beta = dev(pc.ladder(T, Cn))
    state = pd.pt_state(T, Cn)
    accs, legs, counts, sched = [], [], [], None
    for k, (ll, s2r) in enumerate(pc.scans(T, Cn, swapped)):
        if k == pc.N_CALLS - 1:
            before = beta.clone()
            s = pd.pt_schedule(state, beta, adapt=True, reset=True, beta_out=beta if alias else None)
            sched = {name: s[name].cpu().numpy() for name in ("beta", "rejection", "summary")}
            sched["acc"] = state["acc"].cpu().numpy()
            assert alias or np.array_equal(beta.cpu().numpy(), before.cpu().numpy())      # without the alias the input is not written
            beta = s["beta"]
        pd.pt_stats(dev(ll), dev(s2r), beta, state)
        accs.append(state["acc"].cpu().numpy())
        legs.append(state["leg"].cpu().numpy())
        counts.append(state["restarts"].cpu().numpy())
    held = state["acc"].clone()
    s = pd.pt_schedule(state, beta, adapt=False, reset=False)
    last = {name: s[name].cpu().numpy() for name in ("beta", "rejection", "summary")}
    assert np.array_equal(state["acc"].cpu().numpy(), held.cpu().numpy(), equal_nan=True)      # reset = 0 leaves the state
    return dict(accs=accs, legs=legs, counts=counts, schedule=sched, last=last, beta_in=beta.cpu().numpy())


def same_bits(a, b):
    """the names under which two run_device results differ in a bit"""
    out = [f"{k}[{i}]" for k in ("accs", "legs", "counts") for i, (x, y) in enumerate(zip(a[k], b[k])) if not np.array_equal(x, y, equal_nan=True)]
    return out + [f"{k}.{n}" for k in ("schedule", "last") for n in a[k] if not np.array_equal(a[k][n], b[k][n], equal_nan=True)]


# ---------------------------------------------------------------------------------------------------- 1. the two calls on synthetic ℓ
@pytest.mark.parametrize("T,Cn", pc.SHAPES)
def test_gpu_the_two_calls_against_the_restatement(prior_pd, T, Cn):
    ref = pc.reference(T, Cn)
    got = run_device(prior_pd, T, Cn)
    worst = 0.0
    for k in range(pc.N_CALLS):
        for col in EXACT:
            assert np.array_equal(got["accs"][k][:, col], ref["accs"][k][:, col]), (k, col)
        assert np.array_equal(got["legs"][k], ref["legs"][k]) and np.array_equal(got["counts"][k], ref["counts"][k]), k
        worst = max(worst, max(near(got["accs"][k][:, col], ref["accs"][k][:, col]) for col in SUMS))
    sched, want = got["schedule"], ref["schedule"]
    e = dict(A_s=worst, r=near(sched["rejection"], want["rej"]), summary=near(sched["summary"], want["summary"]), beta=near(sched["beta"], want["beta"]),
             last=max(near(got["last"]["rejection"], ref["last"]["rej"]), near(got["last"]["summary"], ref["last"]["summary"])))
    print(f"T = {T}, Cn = {Cn}: largest errors relative to max(1, |ref|): " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()) + f" (bar {TRANS_BAR:.0e}); "
          f"Λ = {want['summary'][0]:.4f}, log Z fwd/rev = {want['summary'][1]:.4f} / {want['summary'][2]:.4f}, restarts {int(ref['counts'][-1].sum())}")
    assert all(v <= TRANS_BAR for v in e.values()), e
    assert np.array_equal(sched["acc"], pt.new_acc(T))                                       # reset: every m = −Inf, the rest 0
    assert sched["beta"][0] == ref["beta"][0] and sched["beta"][-1] == ref["beta"][-1]      # the end slots keep their bits
    assert np.array_equal(got["last"]["beta"], got["beta_in"])                               # adapt = 0 copies β through
    assert ref["counts"][-1].sum() > 0 or Cn < 3


@pytest.mark.parametrize("T,Cn", [(3, 63), (8, 257)])
def test_gpu_the_same_bits_from_run_to_run_on_a_used_handle_and_whatever_the_excluded_terms_hold(pkg, draws_mod, prior_pd, T, Cn):
    fresh = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.STAT_PRIORS))
    try:
        first = run_device(fresh, T, Cn)
    finally:
        fresh.close()
    run_device(prior_pd, 64, 1000)                      # the work array has held a larger shape
    again = run_device(prior_pd, T, Cn)
    assert same_bits(first, again) == []
    assert same_bits(first, run_device(prior_pd, T, Cn, alias=False)) == []
    assert same_bits(first, run_device(prior_pd, T, Cn, swapped=True)) == []      # the NaN and the +Inf trade places


def test_gpu_pt_argument_checks(pkg, prior_pd):
    import torch
    pd = prior_pd
    lib, EINVAL, T, Cn = pd.lib, pkg.capi.OCTO_EINVAL, 4, 5
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    state = pd.pt_state(T, Cn)
    ll, s2r, beta = torch.zeros(T * Cn, dtype=torch.float64, device="cuda"), dev(np.tile(np.arange(T, dtype=np.int32), (Cn, 1))), dev(np.linspace(1.0, 0.0, T))
    out, rej, summ = torch.empty(T, dtype=torch.float64, device="cuda"), torch.empty(T - 1, dtype=torch.float64, device="cuda"), torch.empty(4, dtype=torch.float64, device="cuda")
    acc, leg, rst = state["acc"].data_ptr(), state["leg"].data_ptr(), state["restarts"].data_ptr()

    def stats(h=pd._h, T_=T, Cn_=Cn, d_ll=ll.data_ptr(), d_s2r=s2r.data_ptr(), d_beta=beta.data_ptr(), d_acc=acc, d_leg=leg, d_rst=rst):
        return lib.octo_draws_pt_stats_device(h, T_, Cn_, d_ll, d_s2r, d_beta, d_acc, d_leg, d_rst, st)

    def schedule(h=pd._h, T_=T, d_acc=acc, d_beta=beta.data_ptr(), d_out=out.data_ptr(), d_rej=rej.data_ptr(), d_sum=summ.data_ptr()):
        return lib.octo_draws_pt_schedule_device(h, T_, d_acc, d_beta, 1, 1, d_out, d_rej, d_sum, st)

    assert stats(h=None) == EINVAL and schedule(h=None) == EINVAL
    for bad in (dict(d_ll=None), dict(d_s2r=None), dict(d_beta=None), dict(d_acc=None), dict(d_leg=None), dict(d_rst=None)):
        assert stats(**bad) == EINVAL, bad
    assert b"together" in lib.octo_draws_last_error(pd._h)
    for bad in (dict(T_=1), dict(T_=65), dict(Cn_=0), dict(Cn_=(1 << 24) + 1)):
        assert stats(**bad) == EINVAL, bad
    assert b"2^24" in lib.octo_draws_last_error(pd._h)
    for bad in (dict(d_acc=None), dict(d_beta=None), dict(d_out=None), dict(d_rej=None), dict(d_sum=None), dict(T_=1), dict(T_=65)):
        assert schedule(**bad) == EINVAL, bad
    for ladder in ([1.0, 0.5, 0.6, 0.0], [0.0, 0.3, 0.6, 1.0], [1.0, math.nan, 0.2, 0.0]):
        bad_beta = dev(np.array(ladder))
        assert schedule(d_beta=bad_beta.data_ptr()) == EINVAL and b"non-increasing" in lib.octo_draws_last_error(pd._h), ladder
    assert stats() == 0 and stats(d_leg=None, d_rst=None) == 0 and schedule() == 0
    flat = dev(np.array([1.0, 0.5, 0.5, 0.0]))
    assert schedule(d_beta=flat.data_ptr()) == 0      # equal neighbours are a ladder
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        pd.pt_stats(ll.float(), s2r, beta, state)
    with pytest.raises(ValueError):
        pd.pt_stats(ll, s2r, beta, dict(state, leg=None))
    with pytest.raises(ValueError):
        pd.pt_schedule(pd.pt_state(T + 1, Cn), beta)
    with pytest.raises(ValueError):
        pd.pt_state(1, Cn)


# ---------------------------------------------------------------------------------------------------- 2. α is the swap kernel's probability
def test_gpu_alpha_is_the_acceptance_probability_of_the_swap_kernel(pkg, prior_pd, model):
    """fixed ℓ, 200 swap steps from the identity: per pair the accepted swaps against Σα over the scans that tried the pair"""
    import torch
    T, Cn, steps = pc.SWAP_T, pc.SWAP_CN, pc.SWAP_STEPS
    ll_h, beta_h = pc.swap_inputs()
    swap = pkg.TemperedSwap(model.ln_like, T, Cn, device=torch.device("cuda", 0), seed=pc.SWAP_SEED, betas=beta_h)
    ll = dev(ll_h.reshape(-1))
    by_parity = [prior_pd.pt_state(T, Cn), prior_pd.pt_state(T, Cn)]
    seen = torch.empty((steps, Cn, T), dtype=torch.int32, device="cuda")
    for step in range(steps):
        seen[step] = swap.slot2rep                      # the slot2rep the swap step is about to see
        prior_pd.pt_stats(ll, swap.slot2rep, swap.beta, by_parity[step % 2])
        swap.swap_step(ll, step)
    accepted = swap.accepted.cpu().numpy()
    seen = seen.cpu().numpy()
    acc = [s["acc"].cpu().numpy() for s in by_parity]
    total, var = np.zeros(T - 1), np.zeros(T - 1)
    for step in range(steps):
        alpha = pt.pair_terms(ll_h, seen[step], beta_h)[0]
        tried = np.arange(step % 2, T - 1, 2)
        total[tried] += alpha[tried].sum(axis=1)
        var[tried] += (alpha[tried] * (1.0 - alpha[tried])).sum(axis=1)
    for t in range(T - 1):
        A, n = acc[t % 2][t, pt.A], acc[t % 2][t, pt.N]
        print(f"pair {t}: accepted {accepted[t]} of {int(n)}, Σα = {A:.2f}, 4·√Σα(1 − α) = {4 * math.sqrt(var[t]):.2f}")
        assert n == (steps // 2) * Cn and abs(A - total[t]) <= TRANS_BAR * max(1.0, total[t])
        assert abs(accepted[t] - A) <= 4.0 * math.sqrt(var[t]), t
    assert np.all(var > 10.0) and np.all(np.sort(seen[-1], axis=1) == np.arange(T))      # the probabilities are inside (0, 1): the check has something to see


# ---------------------------------------------------------------------------------------------------- 3. the driver
DRIVER_KEYS = {"samples", "samples_t", "logpost", "swap_acceptance", "betas", "names", "state", "log_evidence", "betas_by_round", "rejection_by_round",
               "barrier_by_round", "restarts", "n_scans"}


def start_ladder(T):
    """TemperedSwap's default ladder, as torch rounds it (pt.cubic_ladder is NumPy's: the last bits differ)"""
    import torch
    return (torch.linspace(1.0, 0.0, T, dtype=torch.float64) ** 3).numpy()


def check_structure(out, T, Cn, R, D, explored):
    n_scans, n_keep = 2 ** (R + 1) - 2, 2 ** R
    assert set(out) == DRIVER_KEYS | explored and out["n_scans"] == n_scans
    assert out["samples"].shape == out["samples_t"].shape == (n_keep, D, Cn) and out["logpost"].shape == (n_keep, Cn) and np.all(np.isfinite(out["logpost"]))
    assert out["betas_by_round"].shape == (R + 1, T) and out["rejection_by_round"].shape == (R, T - 1) and out["barrier_by_round"].shape == (R,)
    b = out["betas_by_round"]
    assert np.all(b[:, 0] == 1.0) and np.all(b[:, -1] == 0.0) and np.all(np.diff(b, axis=1) < 0.0)      # strictly decreasing, the ends exactly 1 and 0
    assert np.array_equal(b[0], start_ladder(T)) and np.array_equal(b[-1], b[-2]) and np.array_equal(out["betas"], b[-1])      # no adaptation in the last round
    assert not np.array_equal(b[1], b[0])
    ev = out["log_evidence"]
    assert np.all(ev["n"] == n_keep * Cn) and np.all(ev["n_fwd"] == n_keep * Cn) and np.all(ev["n_rev"] == n_keep * Cn)      # scans × chains of the last round
    assert np.all((out["rejection_by_round"] >= 0.0) & (out["rejection_by_round"] <= 1.0))
    assert np.allclose(out["barrier_by_round"], out["rejection_by_round"].sum(axis=1), rtol=1e-12)
    assert out["restarts"]["per_chain"].shape == (Cn,) and out["restarts"]["total"] == out["restarts"]["per_chain"].sum()
    assert out["swap_acceptance"].shape == (T - 1,) and np.all((out["swap_acceptance"] >= 0.0) & (out["swap_acceptance"] <= 1.0))


@pytest.mark.parametrize("seed", pc.DRIVER_SEEDS)
def test_gpu_octofit_pigeons_device_with_the_hmc_explorer(pkg, model, seed):
    T, Cn, R = pc.DRIVER_T, pc.DRIVER_CN, pc.DRIVER_ROUNDS
    out = pkg.octofit_pigeons_device(model, T, Cn, R, explorer="hmc", seed=seed)
    check_structure(out, T, Cn, R, model.D, {"hmc_acceptance", "eps"})
    first, last = pc.spread(out["rejection_by_round"][0]), pc.spread(out["rejection_by_round"][-1])
    ev = out["log_evidence"]
    print(f"seed {seed}: Λ = {out['barrier_by_round'][-1]:.3f}; spread of the rejection rates, round 1 {first:.3f}, round {R} {last:.3f}; restarts "
          f"{out['restarts']['total']}; log Z fwd {ev['fwd']:.4f}, rev {ev['rev']:.4f}, mean {ev['mean']:.4f} against {pc.MODEL_LOGZ} (bar {pc.DRIVER_BAR:.3f} on "
          f"{pc.DRIVER_STATISTIC}); ε {np.round(out['eps'], 3)}; ladder {np.round(out['betas'], 4)}")
    assert last < first
    assert out["restarts"]["total"] > 0
    assert abs(ev[pc.DRIVER_STATISTIC] - pc.MODEL_LOGZ) <= pc.DRIVER_BAR
    assert np.all(np.isfinite(out["eps"])) and np.all(out["eps"] > 0) and out["hmc_acceptance"].shape == (T,)


def test_gpu_octofit_pigeons_device_with_the_slice_explorer(pkg, model):
    T, Cn, R = 4, 8, pc.SLICE_ROUNDS
    set_batch_invariant(pkg, model, 1)
    try:
        a, b = (pkg.octofit_pigeons_device(model, T, Cn, R, slice_w=2.0, slice_p=3, n_passes=1, seed=5) for _ in range(2))      # explorer="slice" is the default
    finally:
        set_batch_invariant(pkg, model, 0)
    check_structure(a, T, Cn, R, model.D, {"slice_evals"})
    for k in ("samples_t", "logpost", "slice_evals", "swap_acceptance", "betas_by_round", "rejection_by_round", "barrier_by_round"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["log_evidence"].keys() == b["log_evidence"].keys() and all(np.array_equal(a["log_evidence"][k], b["log_evidence"][k], equal_nan=True) for k in a["log_evidence"])
    assert np.array_equal(a["restarts"]["per_chain"], b["restarts"]["per_chain"]) and np.array_equal(a["state"]["slot2rep"], b["state"]["slot2rep"])
    with pytest.raises(ValueError):
        pkg.octofit_pigeons_device(model, T, Cn, R, explorer="walk")
    with pytest.raises(ValueError):
        pkg.octofit_pigeons_device(model, T, Cn, 0)


def test_gpu_octofit_pt_device_is_not_changed_by_a_pigeons_run(pkg, model):
    """the existing driver after an octofit_pigeons_device run on the same model gives the bits it gives alone"""
    T, Cn, R = 4, 16, 6
    alone = pkg.octofit_pt_device(model, T, Cn, R, seed=9)
    pkg.octofit_pigeons_device(model, T, Cn, 3, explorer="hmc", seed=9)
    after = pkg.octofit_pt_device(model, T, Cn, R, seed=9)
    for k in ("samples", "samples_t", "logpost", "hmc_acceptance", "swap_acceptance", "eps", "betas"):
        assert np.array_equal(alone[k], after[k], equal_nan=True), k
    assert np.array_equal(alone["state"]["theta_t"], after["state"]["theta_t"]) and np.array_equal(alone["state"]["slot2rep"], after["state"]["slot2rep"])
    assert np.array_equal(alone["betas"], start_ladder(T))
