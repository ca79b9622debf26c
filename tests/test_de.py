"""
Differential evolution on the device (include/octofitter_hip_draws.h: octo_draws_de_device; host/draws.py: PriorDraws.de / de_step;
host/callers.py: global_search_device, initialize_device) against its NumPy restatement (tests/de_reference.py) fed by the oracle's callback,
and against the conditions tests/test_de_reference.py establishes for the same seeds on the CPU (tests/de_cases.py states them).

A generation is compared from the device's OWN state before it: the restatement builds the trial points of generation g from the population and
the pairs the device left after generation g − 1, so one undecided selection cannot spread. Decisions are compared on DECIDED individuals — those
whose selection margin in the restatement exceeds 1e-6. An accepted individual's θ_t IS its trial point: without a model it holds the
restatement's bits. Tolerances: with the model θ_t, ℓπ and ℓ at the project's oracle bar 1e-8 relative to max(1, |ref|); on handles without a
model the best ℓπ at the device-transcendental bar TRANS_BAR = 1e-11.
"""
import ctypes as C

import numpy as np
import pytest

import de_cases as dc
import de_reference as de
import draws_cases as cases
from draws_device import TRANS_BAR, draws_mod, hmc_model, mirror_priors, padded, rel, set_batch_invariant      # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_pd(pkg, draws_mod):
    model = hmc_model(pkg)
    pd = draws_mod.PriorDraws(model)
    yield model, pd
    pd.close()
    model.close()


@pytest.fixture(scope="module")
def prior_pd(pkg, draws_mod):
    h = draws_mod.PriorDraws(priors=mirror_priors(pkg, cases.STAT_PRIORS))
    yield h
    h.close()


def host(out):
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def state_of(priors, tt, F, CR, n_accept, f=None, lpt=None, logpost=None):
    """the restatement's state at the device's population: f from the device where it reports it, the restatement's own otherwise"""
    s = de.de_open(priors, tt, logpost=logpost if f is None else None, fcr=(F, CR))
    if f is not None:
        s["f"] = np.array(f)
    if lpt is not None:
        s["lpt"] = np.array(lpt)
    s["n_accept"] = np.array(n_accept, dtype=np.int64)
    return s


# ---------------------------------------------------------------------------------------------------- 1. six generations against the restatement
def test_gpu_generations_against_the_restatement_with_the_model(pkg, oracle, model_pd):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    W, ld, priors, logpost = dc.MODEL_W, dc.MODEL_LD, cases.MODEL_PRIORS, dc.model_logpost(oracle)
    assert ld == W + 5
    start = pd.sample(dc.MODEL_SEED, 0, W, theta=False, logprior_t=False)[1].cpu().numpy()
    lo, hi = dc.model_bounds(start)
    buf, tt = padded(torch, start, ld)
    fbuf = torch.full((2, ld), float("nan"), dtype=torch.float64, device="cuda")
    fcr = fbuf[:, :W]
    fcr[0], fcr[1] = de.F0, de.CR0
    args = dict(lo=lo, hi=hi, radius=dc.DEFAULT_RADIUS, seed=dc.MODEL_SEED)
    out = pd.de(tt, n_gen=0, gen0=dc.MODEL_GEN0, fcr=fcr, **args)
    got = host(out)
    assert np.array_equal(tt.cpu().numpy(), start) and np.all(got["n_accept"] == 0) and int(got["n_improved"][0]) == 0      # the opening moves nothing
    f0, _lp, lpt0 = de.evaluate(priors, start, logpost)
    assert np.all(rel(got["logpost"], f0) <= 1e-8) and np.all(rel(got["loglike"], f0 - lpt0) <= 1e-8)
    errs = dict(theta_t=0.0, logpost=0.0, loglike=0.0)
    for g in range(dc.MODEL_GENS):
        before, pop = got, tt.cpu().numpy()
        s = state_of(priors, pop, before["fcr"][0], before["fcr"][1], before["n_accept"], f=before["logpost"], lpt=before["logpost"] - before["loglike"])
        s1, rec = de.de_generation(priors, s, dc.MODEL_SEED, dc.MODEL_GEN0 + g, dc.DEFAULT_RADIUS, lo, hi, logpost)
        dc.check_model_generation(g, rec)                                       # the condition on the seed, before the device is compared
        out = pd.de(tt, n_gen=1, gen0=dc.MODEL_GEN0 + g, resume=True, out=out, **args)
        got, now = host(out), tt.cpu().numpy()
        assert bool(torch.isnan(buf[:, W:]).all()) and bool(torch.isnan(fbuf[:, W:]).all())      # nothing written beyond column W
        decided = rec["margin"] > de.MARGIN
        acc = got["n_accept"] - before["n_accept"]
        assert np.array_equal(acc[decided], rec["accepted"][decided].astype(acc.dtype)), (g, np.nonzero(decided & (acc != rec["accepted"]))[0])
        assert np.array_equal(got["n_accept"][decided], s1["n_accept"][decided])
        assert np.array_equal(got["fcr"][0][decided], s1["F"][decided]) and np.array_equal(got["fcr"][1][decided], s1["CR"][decided])
        stay, moved = decided & ~rec["accepted"], decided & rec["accepted"]
        assert np.array_equal(now[:, stay], pop[:, stay]) and np.array_equal(got["logpost"][stay], before["logpost"][stay])      # the same bits
        assert np.array_equal(now[:, moved], rec["trial"][:, moved])            # the trial point the restatement built from the same population
        errs["theta_t"] = max(errs["theta_t"], float(np.max(rel(now[:, moved], s1["theta_t"][:, moved]), initial=0.0)))
        errs["logpost"] = max(errs["logpost"], float(np.max(rel(got["logpost"][moved], s1["f"][moved]), initial=0.0)))
        errs["loglike"] = max(errs["loglike"], float(np.max(rel(got["loglike"][moved], de.loglike(s1)[moved]), initial=0.0)))
        assert int(got["n_improved"][0]) == int(acc.sum())
        assert int(got["best"][0]) == de.best(dict(f=got["logpost"]))[0] and got["best_logpost"][0] == got["logpost"][got["best"][0]]
    print(f"max errors over {dc.MODEL_GENS} generations — θ_t {errs['theta_t']:.3e}, ℓπ {errs['logpost']:.3e}, ℓ {errs['loglike']:.3e} (bar 1e-08)")
    assert max(errs.values()) <= 1e-8


# ---------------------------------------------------------------------------------------------------- 2. the edges, on handles without a model
@pytest.mark.parametrize("name", dc.EDGES)
def test_gpu_edges_against_the_restatement(pkg, draws_mod, name):
    import torch
    D, W, radius, _bounds, nan_at, fcr_kind, outputs = dc.EDGES[name]
    priors = dc.edge_priors(name)
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, priors))
    try:
        drawn = pd.sample(dc.EDGE_SEED, 0, W, theta=False, logprior_t=False)[1]
        assert tuple(drawn.shape) == (D, W)
        start, lo, hi = dc.edge_population(name, drawn.cpu().numpy())
        buf, tt = padded(torch, start, W + 5)
        F, CR = (dc.edge_fcr(name) if fcr_kind == "given" else (np.full(W, de.F0), np.full(W, de.CR0)))
        fcr = False if fcr_kind is None else None
        if fcr_kind == "given":
            fcr = padded(torch, np.stack([F, CR]), tt.stride(0) if D > 1 else W)[1]
        n_acc = np.zeros(W, dtype=np.int64)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lo_t, hi_t = (None, None) if lo is None else (torch.as_tensor(lo, device="cuda"), torch.as_tensor(hi, device="cuda"))
        ld = tt.stride(0) if D > 1 else W
        out = None
        for g in range(-1, dc.EDGE_GENS):      # −1: the opening
            pop = tt.cpu().numpy()
            if g >= 0:
                s = state_of(priors, pop, F, CR, n_acc)
                s1, rec = de.de_generation(priors, s, dc.EDGE_SEED, dc.EDGE_GEN0 + g, radius, lo, hi)
                dc.check_edge_generation(name, g, rec)                          # the condition on the seed, before the device is compared
            if outputs:
                out = pd.de(tt, lo=lo, hi=hi, radius=radius, seed=dc.EDGE_SEED, n_gen=min(g + 1, 1), gen0=dc.EDGE_GEN0 + max(g, 0), resume=g >= 0, fcr=fcr, out=out)
                got = host(out)
                assert got["logpost"] is None and got["loglike"] is None
            else:                                                               # every optional output NULL: the raw call
                rc = pd.lib.octo_draws_de_device(pd._h, dc.EDGE_SEED, dc.EDGE_GEN0 + max(g, 0), W, ld, tt.data_ptr(), lo_t.data_ptr(), hi_t.data_ptr(), radius,
                                                 min(g + 1, 1), 1 if g >= 0 else 0, None, None, None, None, None, None, None, st)
                assert rc == 0, pd.lib.octo_draws_last_error(pd._h)
                got = None
            torch.cuda.synchronize()
            now = tt.cpu().numpy()
            assert bool(torch.isnan(buf[:, W:]).all())
            if g < 0:
                assert np.array_equal(now, start, equal_nan=True)
                continue
            # an individual either keeps its bits or holds its trial point's: the trial planes are the restatement's, bit for bit
            kept = np.all((now == pop) | (np.isnan(now) & np.isnan(pop)), axis=0)
            took = np.all(now == rec["trial"], axis=0)
            assert np.all(kept | took), (name, g, np.nonzero(~(kept | took))[0])
            decided = rec["margin"] > de.MARGIN
            same_point = np.all(rec["trial"] == pop, axis=0)                    # a trial that crossed nowhere new: either answer leaves the same bits
            acc_dev = took & ~(same_point & kept)
            check = decided & ~same_point
            assert np.array_equal(acc_dev[check], rec["accepted"][check]), (name, g, np.nonzero(check & (acc_dev != rec["accepted"]))[0])
            if got is not None:
                acc = got["n_accept"] - n_acc
                assert np.array_equal(acc[decided], rec["accepted"][decided].astype(acc.dtype)) and int(got["n_improved"][0]) == int(acc.sum())
                kb, fb = de.best(s1)
                if np.all(decided):
                    assert int(got["best"][0]) == kb and abs(got["best_logpost"][0] - fb) <= TRANS_BAR * max(1.0, abs(fb)), (got["best_logpost"][0], fb)
                n_acc = got["n_accept"].astype(np.int64)
                if got["fcr"] is not None:
                    assert np.array_equal(got["fcr"][0][decided], s1["F"][decided]) and np.array_equal(got["fcr"][1][decided], s1["CR"][decided])
                    F, CR = got["fcr"][0], got["fcr"][1]
                else:
                    F, CR = np.where(acc > 0, rec["Ft"], F), np.where(acc > 0, rec["CRt"], CR)
            else:
                n_acc = n_acc + acc_dev
                F, CR = np.where(acc_dev, rec["Ft"], F), np.where(acc_dev, rec["CRt"], CR)
            if nan_at is not None:      # it never wins, and it is replaced only by a finite trial
                assert got["best"][0] != nan_at or np.all(np.isfinite(now[:, nan_at]))
                if acc_dev[nan_at]:
                    assert np.all(np.isfinite(now[:, nan_at]))
                else:
                    assert np.array_equal(now[:, nan_at], pop[:, nan_at], equal_nan=True)
    finally:
        pd.close()


# ---------------------------------------------------------------------------------------------------- 3. resume and reuse
def run(torch, pd, start, cuts, ld=None, **kw):
    """the search of dc.MODEL_SEED from `start` cut into calls of `cuts` generations after its opening: (θ_t, outputs) at the end"""
    W = start.shape[1]
    _buf, tt = padded(torch, start, ld or W)
    out, done = pd.de(tt, n_gen=0, gen0=dc.MODEL_GEN0, seed=dc.MODEL_SEED, **kw), 0
    for n in cuts:
        out = pd.de(tt, n_gen=n, gen0=dc.MODEL_GEN0 + done, seed=dc.MODEL_SEED, resume=True, out=out, **kw)
        done += n
    return tt.cpu().numpy(), host(out)


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and all(np.array_equal(a[1][k], b[1][k], equal_nan=True) for k in a[1])


def test_gpu_resume_and_reuse(pkg, model_pd, draws_mod):
    import torch
    model, pd = model_pd
    W = dc.MODEL_W
    start = pd.sample(dc.MODEL_SEED, 0, W, theta=False, logprior_t=False)[1].cpu().numpy()
    lo, hi = dc.model_bounds(start)
    kw = dict(lo=lo, hi=hi, radius=dc.DEFAULT_RADIUS)
    set_batch_invariant(pkg, model, 1)
    try:
        full = run(torch, pd, start, (5,), **kw)
        assert full[1]["n_accept"].sum() > 0
        assert same(full, run(torch, pd, start, (2, 3), **kw))                   # a + b
        assert same(full, run(torch, pd, start, (5,), **kw))                     # the same call twice
        assert same(full, run(torch, pd, start, (1, 0, 1, 3), **kw))
        other = run(torch, pd, start[:, :40].copy(), (2,), ld=45, **kw)          # another (W, ld) on the same handle
        assert other[0].shape == (model.D, 40)
        tt = torch.as_tensor(start, device="cuda").contiguous()
        with pytest.raises(pkg.capi.OctoError, match="resume"):                  # … is not what a call of this (W, ld) resumes
            pd.de(tt, n_gen=1, gen0=dc.MODEL_GEN0 + 2, seed=dc.MODEL_SEED, resume=True, **kw)
        assert same(full, run(torch, pd, start, (4, 1), **kw))                   # and is right with resume = 0
        # n_gen = 0, resume = 0: θ_t keeps its bits and d_logpost is the population's ℓπ
        tt0, out0 = run(torch, pd, start, (), **kw)
        assert np.array_equal(tt0, start)
        lp = model.logpost_device(torch.as_tensor(start, device="cuda").contiguous(), grad=False)[0].cpu().numpy()
        assert np.all(np.abs(out0["logpost"] - lp) <= 1e-8 * np.maximum(1.0, np.abs(lp)))
    finally:
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 4. properties
def test_gpu_properties_over_the_generations(model_pd):
    _model, pd = model_pd
    W = dc.MODEL_W
    start = pd.sample(dc.MODEL_SEED + 1, 0, W, theta=False, logprior_t=False)[1]
    lo, hi = dc.model_bounds(start.cpu().numpy())
    tt = start.clone()
    out = pd.de(tt, lo=lo, hi=hi, n_gen=0, seed=9)
    prev = host(out)
    for g in range(8):
        out = pd.de(tt, lo=lo, hi=hi, n_gen=1, gen0=g, seed=9, resume=True, out=out)
        got = host(out)
        assert np.all(got["logpost"] >= prev["logpost"])                          # per individual, exactly
        fin = np.where(np.isfinite(got["logpost"]), got["logpost"], -np.inf)
        assert int(got["best"][0]) == int(np.argmax(fin)) and got["best_logpost"][0] == fin.max()
        assert int(got["n_improved"][0]) == int(got["n_accept"].sum() - prev["n_accept"].sum())
        prev = got
    assert prev["n_accept"].sum() > 0


def test_gpu_best_takes_the_lower_index_of_a_tie(prior_pd):
    pd = prior_pd
    tt = pd.sample(3, 0, 300, theta=False, logprior_t=False)[1]
    tt[:, 290] = tt[:, 7]
    tt[:, 100] = tt[:, 7]
    out = pd.de(tt, n_gen=0, seed=1)
    b = int(out["best"].item())
    lpt = pd.sample(3, 0, 300, theta=False, theta_t=False)[2].cpu().numpy()
    lpt[290] = lpt[100] = lpt[7]
    assert b == int(np.argmax(lpt)) and (b != 100 and b != 290)
    tt[:, 0] = tt[:, int(np.argmax(lpt))]      # the best, copied in front of itself
    tt[:, 299] = tt[:, 0]
    assert int(pd.de(tt, n_gen=0, seed=1)["best"].item()) == 0
    tt[:] = float("nan")
    out = pd.de(tt, n_gen=2, seed=1)
    assert int(out["best"].item()) == -1 and float(out["best_logpost"].item()) == -np.inf and int(out["n_accept"].sum()) == 0


# ---------------------------------------------------------------------------------------------------- 5. it optimises
def test_gpu_reaches_the_analytic_maximum_of_eight_normal_priors(pkg, draws_mod):
    pd = draws_mod.PriorDraws(priors=mirror_priors(pkg, dc.OPT_PRIORS))
    try:
        ref_gap = dc.opt_reference_gap()
        assert 0.0 <= ref_gap < dc.OPT_GAP, "condition on the seed (the reference alone)"
        tt = pd.sample(dc.OPT_SEED, 0, dc.OPT_W, theta=False, logprior_t=False)[1]
        out = pd.de_step(tt, radius=dc.DEFAULT_RADIUS, n_gen=dc.OPT_GENS, seed=dc.OPT_SEED)
        gap = dc.OPT_MAX - float(out["best_logpost"].item())
        print(f"gap to the analytic maximum after {dc.OPT_GENS} generations: device {gap:.3e}, restatement {ref_gap:.3e}")
        assert -1e-12 <= gap <= dc.OPT_FACTOR * ref_gap
    finally:
        pd.close()


# ---------------------------------------------------------------------------------------------------- 6. the callers
def test_gpu_global_search_device(pkg, model_pd):
    import torch
    model, _pd = model_pd
    r = pkg.global_search_device(model, **dc.SEARCH)
    assert r["n_gen"] == dc.SEARCH["max_gen"] and list(r["generations"]) == [0, 10, 20, 30, 40] and r["names"] == list(model.names)
    assert np.all(np.diff(r["history"]) >= 0) and r["best_logpost"] == r["history"][-1] >= r["history"][0]      # exactly
    assert r["logpost"][r["best"]] == r["best_logpost"] == np.max(r["logpost"])
    lp = model.logpost_device(torch.as_tensor(r["theta_t"], device="cuda").contiguous(), grad=False)[0].cpu().numpy()
    assert np.all(np.abs(lp - r["logpost"]) <= 1e-8 * np.maximum(1.0, np.abs(lp)))
    print(f"global search: best ℓπ by segment {np.round(r['history'], 3)}")


def test_gpu_initialize_device(pkg, model_pd):
    model, _pd = model_pd
    r = pkg.initialize_device(model, n_starts=dc.INIT_STARTS, max_rounds=100, **dc.SEARCH)
    assert r["theta_t"].shape == (model.D, dc.INIT_STARTS) and r["search"]["theta_t"].shape == (model.D, dc.SEARCH["n_pop"])
    assert np.array_equal(r["start_logpost"], np.sort(r["start_logpost"])[::-1])
    assert np.all(np.abs(r["start_logpost"] - r["search"]["logpost"][r["search_index"]]) <= 1e-8 * np.abs(r["start_logpost"]))
    assert np.all(r["logpost"] >= r["start_logpost"])      # every start's L-BFGS ℓπ >= its start's
    print(f"initialize: search best {r['search']['best_logpost']:.4f}, L-BFGS best {r['logpost'][r['best']]:.4f}")


def test_gpu_default_starts_keep_every_bit(pkg, model_pd):
    model, pd = model_pd
    kw = dict(N=4096, n_starts=8, seed=2, max_rounds=60)
    a = pkg.optimize_starting_points_device(model, **kw)
    θ0, _lp, _ = pd.best(kw["seed"], kw["N"], keep=kw["n_starts"])
    b = pkg.optimize_starting_points_device(model, starts=model.link(θ0), **kw)
    assert set(a) == set(b)
    for k in a:
        if k == "start_logpost":      # the prior search's ℓπ against the callback's at the same points
            assert np.all(np.abs(a[k] - b[k]) <= 1e-8 * np.maximum(1.0, np.abs(a[k])))
        elif k != "names":
            assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---------------------------------------------------------------------------------------------------- 7. the arguments
def test_gpu_de_argument_checks(pkg, draws_mod, model_pd, prior_pd):
    import torch
    model, pd = model_pd
    lib, EINVAL, W = pd.lib, pkg.capi.OCTO_EINVAL, 8
    tt = pd.sample(1, 0, W, theta=False, logprior_t=False)[1]
    lp = torch.zeros(W, dtype=torch.float64, device="cuda")
    bound = torch.zeros(model.D, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(h, W_=W, ld=W, radius=8, n_gen=0, resume=0, d_lo=None, d_hi=None, d_lp=None, d_tt=tt.data_ptr(), seed=0, gen0=0):
        return lib.octo_draws_de_device(h, seed, gen0, W_, ld, d_tt, d_lo, d_hi, radius, n_gen, resume, None, d_lp, None, None, None, None, None, st)

    def refused(text, **kw):
        h = kw.pop("h", pd._h)
        return call(h, **kw) == EINVAL and text in lib.octo_draws_last_error(h)

    assert call(None) == EINVAL
    assert refused(b"W >= 4", W_=3, ld=3) and refused(b"W <= ld", ld=W - 1) and refused(b"2^30", W_=(1 << 30) + 1, ld=(1 << 30) + 1)
    assert refused(b"radius", radius=-1) and refused(b"n_gen", n_gen=-1)
    assert refused(b"both or neither", d_lo=bound.data_ptr()) and refused(b"both or neither", d_hi=bound.data_ptr())
    assert refused(b"d_theta_t", d_tt=None)
    fresh = draws_mod.PriorDraws(model)
    assert refused(b"resume", h=fresh._h, resume=1)                             # nothing to resume
    fresh.close()
    assert call(pd._h, n_gen=2) == 0
    assert call(pd._h, n_gen=1, gen0=2, resume=1) == 0
    for other in (dict(gen0=2), dict(gen0=4), dict(W_=W - 1), dict(ld=W + 1), dict(radius=7), dict(seed=1), dict(d_lo=bound.data_ptr(), d_hi=bound.data_ptr())):
        assert refused(b"resume", resume=1, **{"gen0": 3, **other}), other
    assert call(pd._h, n_gen=0, gen0=3, resume=1) == 0
    nomodel = prior_pd
    t5 = nomodel.sample(1, 0, W, theta=False, logprior_t=False)[1]
    assert refused(b"no model", h=nomodel._h, d_lp=lp.data_ptr(), d_tt=t5.data_ptr())
    assert call(nomodel._h, d_tt=t5.data_ptr(), n_gen=3) == 0
    with pytest.raises(ValueError):
        pd.de(tt.t())
    with pytest.raises(ValueError):
        pd.de(tt, lo=np.zeros(model.D))
    with pytest.raises(ValueError):
        pd.de_step(tt, gens_per_call=0)
    torch.cuda.synchronize()
