"""
The variational reference of a tempering leg on the device (csrc/draws/octo_draws_vref.hip; host/draws.py: PriorDraws.reference_table …
reference_exchange; host/callers.py: octofit_pigeons_device(n_temps_variational=…)) against its NumPy restatement (tests/vref_reference.py):
the table bit for bit, the handle's functions under a reference against a twin handle created with the same Normal priors, the exchange,
and the two-legged driver on the suites' test model. The inputs and bars are in tests/vref_cases.py.
"""
import ctypes as C
import types

import numpy as np
import pytest

import hmc_reference as ref
import pt_cases as pc
import vref_cases as vc
import vref_reference as vr
from draws_device import TRANS_BAR, draws_mod, hmc_model, rel      # noqa: F401

pytestmark = pytest.mark.gpu

PRIOR_DTYPE = np.dtype([("kind", np.int32), ("pad", np.int32), ("p0", np.float64), ("p1", np.float64), ("lo", np.float64), ("hi", np.float64)])


def dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def near(got, want, bar=TRANS_BAR):
    """the non-finite entries of want (NaN, ±Inf) are the same values in got, the finite ones within bar·max(1, |want|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return np.array_equal(got[~fin], want[~fin], equal_nan=True) and bool(np.all(np.abs(got[fin] - want[fin]) <= bar * np.maximum(1.0, np.abs(want[fin]))))


def table_parts(t, D):
    """the parts of a table tensor on the host: priors as records, pc [D][4], ic [D][4], mean, sd"""
    raw = t.cpu().numpy()
    out = {name: raw[o:o + n] for name, (o, n) in vr.parts(D).items()}
    out["priors"] = out["priors"].view(PRIOR_DTYPE)
    out["pc"], out["ic"] = out["pc"].reshape(D, vr.PRIOR_NC), out["ic"].reshape(D, vr.IC_N)
    return out


@pytest.fixture(scope="module")
def model(pkg):
    m = hmc_model(pkg)
    yield m
    m.close()


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("D", vc.TABLE_D)
def test_gpu_the_table_against_the_rule(pkg, draws_mod, D):
    mean, sd = vc.table_inputs(D)
    with draws_mod.PriorDraws(priors=[pkg.Normal(0.0, 1.0)] * D) as pd:
        t = pd.reference_table()
        assert t.numel() == vr.table_doubles(D) == 15 * D
        assert int(pd.reference_set(t, dev(mean), dev(sd)).item()) == 0
        got, want = table_parts(t, D), vr.table(mean, sd)
        p = got["priors"]
        assert np.all(p["kind"] == ref.NORMAL) and np.all(p["pad"] == 0) and np.all(p["lo"] == -np.inf) and np.all(p["hi"] == np.inf)
        assert np.array_equal(bits(p["p0"]), bits(mean)) and np.array_equal(bits(p["p1"]), bits(sd))
        assert np.array_equal(bits(got["mean"]), bits(mean)) and np.array_equal(bits(got["sd"]), bits(sd))
        assert np.all(np.isnan(got["pc"][:, 0])) and np.array_equal(bits(got["pc"][:, 1]), bits(np.zeros(D))) and np.all(got["ic"] == 0.0)
        assert np.array_equal(bits(got["pc"][:, 3]), bits(1.0 / sd))                                   # an IEEE division
        err = rel(got["pc"][:, 2], want["pc"][:, 2]).max()
        print(f"D = {D}: −log σ within {err:.2e} (bar {TRANS_BAR:g})")
        assert err <= TRANS_BAR
        # a bad coordinate is counted and keeps its bytes; the others are written
        clean = t.cpu().numpy().copy()
        j = D // 2
        for what in ("mean", "sd"):
            m2, s2 = mean + 1.0, sd * 2.0
            if what == "mean":
                m2[j] = np.nan
            else:
                s2[j] = 0.0
            t.copy_(dev(clean))
            assert int(pd.reference_set(t, dev(m2), dev(s2)).item()) == 1
            after, before = table_parts(t, D), table_parts(dev(clean), D)
            for name in ("priors", "pc", "ic", "mean", "sd"):
                assert after[name][j].tobytes() == before[name][j].tobytes(), (what, name)
            others = np.arange(D) != j
            assert np.array_equal(after["mean"][others], m2[others]) and np.array_equal(after["sd"][others], s2[others])
        # the fit is the set of (mean, inflate·√(M2/(n − 1))); n = 1 is bad in every coordinate and writes nothing
        count, mu, msq = vc.moments_inputs(D)
        f_mean, f_sd, _ = vr.fit(count, mu, msq, inflate=1.5)
        a, b = pd.reference_table(), pd.reference_table()
        assert int(pd.reference_fit(a, dev(count), dev(mu), dev(msq), inflate=1.5).item()) == 0
        assert int(pd.reference_set(b, dev(f_mean), dev(f_sd)).item()) == 0
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        held = a.cpu().numpy().copy()
        bad = pd.reference_fit(a, dev(np.array([1.0])), dev(mu + 1.0), dev(msq), bad=dev(np.array([77], dtype=np.int32)))
        assert int(bad.item()) == D and a.cpu().numpy().tobytes() == held.tobytes()                    # written, not accumulated
        for inflate in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(pkg.capi.OctoError):
                pd.reference_fit(a, dev(count), dev(mu), dev(msq), inflate=inflate)
        with pytest.raises(ValueError):
            pd.reference_set(t[:-1], dev(mean), dev(sd))


# ---------------------------------------------------------------------------------------------------- draws and explorers under a reference
def twin_handle(draws_mod, pkg, model, mean, sd):
    """a handle CREATED with the priors Normal(mean_d, sd_d) on the same device model and context"""
    c_priors = (pkg.capi.OctoPrior * model.D)()
    for k in range(model.D):
        c_priors[k].kind, c_priors[k].p0, c_priors[k].p1, c_priors[k].lo, c_priors[k].hi = ref.NORMAL, mean[k], sd[k], -np.inf, np.inf
    proxy = types.SimpleNamespace(D=model.D, ln_like=model.ln_like, _m=model._m, _c_priors=c_priors)
    return draws_mod.PriorDraws(proxy)


def reference_point(model):
    """an arbitrary (μ [D], σ [D]) in θ_t: means of either sign, spreads on both sides of 1"""
    rng = np.random.default_rng(42)
    return rng.standard_normal(model.D) * 0.5, rng.uniform(0.3, 2.0, model.D)


def test_gpu_sample_under_a_reference_against_the_restatement(draws_mod, model):
    mean, sd = reference_point(model)
    priors = vr.normal_priors(mean, sd)
    with draws_mod.PriorDraws(model) as pd:
        t = pd.reference_table()
        assert int(pd.reference_set(t, dev(mean), dev(sd)).item()) == 0
        with pd.reference(t):
            th, tt, lpt = (x.cpu().numpy() for x in pd.sample(11, 1000, 300))
            assert int(pd.reference_set(t, dev(mean + 1.0), dev(sd)).item()) == 0      # re-made in place while it is active: the next call reads it
            moved = pd.sample(11, 1000, 300)[1].cpu().numpy()
        idx = np.uint64(1000) + np.arange(300, dtype=np.uint64)
        want_th, want_tt = ref.prior_sample(priors, 11, idx)
        want_lpt, _ = ref.logprior_t(priors, want_tt)
        errs = rel(th, want_th).max(), rel(tt, want_tt).max(), rel(lpt, want_lpt).max()
        print("sample under a reference: θ, θ_t, ℓprior_t within", errs)
        assert max(errs) <= TRANS_BAR and np.array_equal(th, tt)      # the link of a Normal is the identity
        assert rel(moved, ref.prior_sample(vr.normal_priors(mean + 1.0, sd), 11, idx)[1]).max() <= TRANS_BAR


@pytest.mark.parametrize("W", [1, 65, 300])
def test_gpu_a_reference_is_a_handle_created_with_those_priors(pkg, draws_mod, model, W):
    """σ = 1 makes −log σ and 1/σ exact: the handle under the reference and the twin created with Normal(μ, 1) run the same kernels on the same
    constants, so every output holds the same bits"""
    import torch
    mean, _ = reference_point(model)
    sd = np.ones(model.D)
    with draws_mod.PriorDraws(model) as pd, twin_handle(draws_mod, pkg, model, mean, sd) as twin, draws_mod.PriorDraws(model) as fresh:
        t = pd.reference_table()
        assert int(pd.reference_set(t, dev(mean), dev(sd)).item()) == 0
        beta = dev(np.linspace(1.0, 0.0, W) if W > 1 else np.array([0.5]))

        def calls(h):
            out = {}
            th, tt, lpt = h.sample(5, 40, W)
            out.update(theta=th, theta_t=tt.clone(), lpt=lpt)
            x = tt.clone()
            lp, ll, dH, acc = h.hmc_step(x, beta=beta, eps=0.05, n_leapfrog=3, seed=5, step=1)
            out.update(hmc_x=x, hmc_lp=lp, hmc_ll=ll, hmc_dH=dH, hmc_acc=acc)
            x = tt.clone()
            r = h.nuts_step(x, beta=beta, eps=0.05, max_depth=3, seed=5, step=2)
            out.update(nuts_x=x, **{f"nuts_{k}": v for k, v in enumerate(r)})
            x = tt.clone()
            r = h.slice_step(x, beta=beta, w=1.0, p=2, n_passes=1, seed=5, step=3)
            out.update(slice_x=x, **{f"slice_{k}": v for k, v in r.items()})
            torch.cuda.synchronize()
            return {k: v.cpu().numpy() for k, v in out.items()}

        with pd.reference(t):
            under = calls(pd)
        created = calls(twin)
        differ = [k for k in created if not np.array_equal(under[k], created[k], equal_nan=True)]
        assert not differ, differ
        assert np.isfinite(under["hmc_ll"]).any() and (W == 1 or not np.array_equal(under["hmc_x"], under["theta_t"]))      # the β = 0 chain moves
        # after use_reference(NULL) the handle is a fresh handle again
        back, new = calls(pd), calls(fresh)
        differ = [k for k in new if not np.array_equal(back[k], new[k], equal_nan=True)]
        assert not differ, differ
        assert not np.array_equal(back["theta_t"], under["theta_t"])


def test_gpu_a_transition_is_not_resumed_across_use_reference(pkg, draws_mod, model):
    mean, sd = reference_point(model)
    with draws_mod.PriorDraws(model) as pd:
        t = pd.reference_table()
        assert int(pd.reference_set(t, dev(mean), dev(sd)).item()) == 0
        x = pd.sample(3, 0, 33)[1]
        args = dict(eps=0.05, max_depth=4, n_rounds=1, seed=1, step=0)
        out = pd.nuts(x, **args)
        pd.nuts(x, resume=True, out=out, **args)                       # resumable while the target stays
        pd.use_reference(t)
        with pytest.raises(pkg.capi.OctoError):
            pd.nuts(x, resume=True, out=out, **args)
        args = dict(w=1.0, p=2, n_passes=1, n_rounds=1, seed=1, step=0)
        so = pd.slice(x, **args)                                        # opened under the reference
        pd.slice(x, resume=True, out=so, **args)
        pd.use_reference(None)
        with pytest.raises(pkg.capi.OctoError):
            pd.slice(x, resume=True, out=so, **args)


# ---------------------------------------------------------------------------------------------------- the exchange
def run_exchange(pd, Cn, a, b, ref_a=True, ref_b=True):
    """the device call on copies of two vref_cases legs; ref_*: under the leg's own fit, or (False) NULL = the handle's prior"""
    legs, tables = [], []
    for g, use in ((a, ref_a), (b, ref_b)):
        t = None
        if use:
            t = pd.reference_table()
            assert int(pd.reference_set(t, dev(g["mean"]), dev(g["sd"])).item()) == 0
        tables.append(t)
        legs.append(dict(s2r=dev(g["slot2rep"]), theta=dev(g["theta"]), lp=dev(g["lp"]), ll=dev(g["ll"])))
    (A, B), (ta, tb) = legs, tables
    pd.reference_exchange(A["s2r"], A["theta"], A["lp"], A["ll"], ta, B["s2r"], B["theta"], B["lp"], B["ll"], tb)
    return [{k: v.cpu().numpy() for k, v in g.items()} for g in legs]


@pytest.fixture(scope="module")
def exchange_pd(pkg, draws_mod):
    h = draws_mod.PriorDraws(priors=[pkg.Normal(0.5, 1.5)] * vc.EXCHANGE_D)
    yield h
    h.close()


@pytest.mark.parametrize("shape", vc.EXCHANGE_SHAPES)
def test_gpu_the_exchange_against_the_restatement(exchange_pd, shape):
    Cn, T_a, T_b = shape
    a0, b0 = vc.exchange_inputs(*shape)
    want = vc.exchange_reference(*shape)
    got = run_exchange(exchange_pd, Cn, a0, b0)
    again = run_exchange(exchange_pd, Cn, a0, b0)
    c = np.arange(Cn)
    for g0, g, w, r in zip((a0, b0), got, want, again):
        cols = g0["slot2rep"][:, 0] * Cn + c
        rest = np.setdiff1d(np.arange(g0["lp"].size), cols)
        assert np.array_equal(bits(g["theta"]), bits(w["theta"])) and np.array_equal(bits(g["lp"]), bits(w["lp"]))      # swapped bit for bit, the rest kept
        assert np.array_equal(bits(g["theta"][:, rest]), bits(g0["theta"][:, rest])) and np.array_equal(bits(g["lp"][rest]), bits(g0["lp"][rest]))
        assert np.array_equal(bits(g["ll"][rest]), bits(g0["ll"][rest])) and np.array_equal(g["s2r"], g0["slot2rep"])
        assert near(g["ll"][cols], w["ll"][cols])                                                                           # −Inf where the restatement says
        assert all(np.array_equal(bits(g[k]), bits(r[k])) for k in ("theta", "lp", "ll"))                                # the same bits from run to run
    ca, cb = a0["slot2rep"][:, 0] * Cn + c, b0["slot2rep"][:, 0] * Cn + c
    assert got[1]["ll"][cb[0]] == -np.inf and got[0]["ll"][ca[Cn - 1]] == -np.inf      # ℓπ = −Inf moved to leg B; the NaN coordinate healed leg A's reference
    # both references NULL: the two legs share the handle's prior, and a point's potential moves with it
    both = run_exchange(exchange_pd, Cn, a0, b0, ref_a=False, ref_b=False)
    priors = vr.normal_priors(np.full(vc.EXCHANGE_D, 0.5), np.full(vc.EXCHANGE_D, 1.5))
    wa, wb = vr.exchange(Cn, dict(a0, priors=priors), dict(b0, priors=priors))
    assert near(both[0]["ll"][ca], wa["ll"][ca]) and near(both[1]["ll"][cb], wb["ll"][cb])
    fin = np.isfinite(wa["ll"][ca]) & np.isfinite(wb["ll"][cb])
    before_a = vr.potential(a0["lp"][ca], *vr.log_q(priors, a0["theta"][:, ca]))
    before_b = vr.potential(b0["lp"][cb], *vr.log_q(priors, b0["theta"][:, cb]))
    assert near(both[0]["ll"][ca][fin], before_b[fin]) and near(both[1]["ll"][cb][fin], before_a[fin])      # they trade places


def test_gpu_a_slot_outside_the_ladder_exchanges_nothing(exchange_pd):
    shape = (63, 3, 5)
    Cn = shape[0]
    a0, b0 = (dict(g) for g in vc.exchange_inputs(*shape))
    a0["slot2rep"], b0["slot2rep"] = a0["slot2rep"].copy(), b0["slot2rep"].copy()
    a0["slot2rep"][5, 0], b0["slot2rep"][9, 0], a0["slot2rep"][62, 0] = -1, 5, 3
    got = run_exchange(exchange_pd, Cn, a0, b0)
    want = vr.exchange(Cn, a0, b0)
    for g, w, g0 in zip(got, want, (a0, b0)):
        assert np.array_equal(bits(g["theta"]), bits(w["theta"])) and np.array_equal(bits(g["lp"]), bits(w["lp"]))
        for ch in (5, 9, 62):
            cols = np.arange(g0["T"]) * Cn + ch
            assert all(np.array_equal(bits(g[k][..., cols]), bits(g0[k][..., cols])) for k in ("theta", "lp", "ll")), ch


def test_gpu_exchange_argument_checks(pkg, exchange_pd):
    pd, lib, E = exchange_pd, exchange_pd.lib, pkg.capi.OCTO_EINVAL
    Cn, T_a, T_b = 4, 3, 2
    import torch
    s_a, s_b = (torch.zeros((Cn, T), dtype=torch.int32, device="cuda") for T in (T_a, T_b))
    th_a, th_b = (torch.zeros((vc.EXCHANGE_D, T * Cn), dtype=torch.float64, device="cuda") for T in (T_a, T_b))
    v = [torch.zeros(T * Cn, dtype=torch.float64, device="cuda") for T in (T_a, T_a, T_b, T_b)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(Cn=Cn, T_a=T_a, s_a=s_a.data_ptr(), ld_a=T_a * Cn, th_a=th_a.data_ptr(), lp_a=v[0].data_ptr(), ll_a=v[1].data_ptr(), T_b=T_b, s_b=s_b.data_ptr(),
             ld_b=T_b * Cn, th_b=th_b.data_ptr(), lp_b=v[2].data_ptr(), ll_b=v[3].data_ptr(), h=pd._h):
        return lib.octo_draws_reference_exchange_device(h, Cn, T_a, s_a, ld_a, th_a, lp_a, ll_a, None, T_b, s_b, ld_b, th_b, lp_b, ll_b, None, st)
    assert call() == pkg.capi.OCTO_OK
    assert call(h=None) == E
    for name in ("s_a", "th_a", "lp_a", "ll_a", "s_b", "th_b", "lp_b", "ll_b"):
        assert call(**{name: None}) == E, name
    assert call(T_a=1) == E and call(T_b=1) == E and call(Cn=0) == E
    assert call(ld_a=T_a * Cn - 1) == E and call(ld_b=T_b * Cn - 1) == E
    assert call(th_b=th_a.data_ptr()) == E
    assert b"share" in lib.octo_draws_last_error(pd._h)
    with pytest.raises(ValueError):
        pd.reference_exchange(s_a, th_a, v[0], v[1], None, s_b[:3], th_b, v[2], v[3], None)      # the legs' chain counts differ
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the driver
@pytest.mark.parametrize("seed", pc.DRIVER_SEEDS)
def test_gpu_octofit_pigeons_device_with_a_variational_leg(pkg, model, seed):
    T, Cn, R = pc.DRIVER_T, pc.DRIVER_CN, pc.DRIVER_ROUNDS
    out = pkg.octofit_pigeons_device(model, T, Cn, R, explorer="hmc", seed=seed, n_temps_variational=T, first_tuning_round=vc.DRIVER_FIRST_TUNING_ROUND)
    var = out["variational"]
    n_keep = 2 ** R
    ev, ev_v = out["log_evidence"], var["log_evidence"]
    lam, lam_v = out["barrier_by_round"][-1], var["barrier_by_round"][-1]
    print(f"seed {seed}: prior leg log Z fwd {ev['fwd']:.4f} rev {ev['rev']:.4f} Λ {lam:.3f} restarts {out['restarts']['total']}; variational leg log Z fwd "
          f"{ev_v['fwd']:.4f} rev {ev_v['rev']:.4f} mean {ev_v['mean']:.4f} Λ {lam_v:.3f} restarts {var['restarts']['total']} against {pc.MODEL_LOGZ} "
          f"(bars {pc.DRIVER_BAR:.4f}, {vc.DRIVER_VAR_BAR:.4f}); bad {var['bad_by_round']}; ladder {np.round(var['betas'], 4)}")
    assert abs(ev_v["fwd"] - pc.MODEL_LOGZ) <= vc.DRIVER_VAR_BAR
    assert abs(ev[pc.DRIVER_STATISTIC] - pc.MODEL_LOGZ) <= pc.DRIVER_BAR      # the exchange does not disturb the first leg
    m, s = var["mean_by_round"], var["sd_by_round"]
    first = vc.DRIVER_FIRST_TUNING_ROUND - 2                                   # round 3 is the first that ends with a fit
    assert m.shape == s.shape == (R, model.D) and np.isnan(m[:first]).all() and np.isnan(s[:first]).all()
    assert np.isfinite(m[first:]).all() and np.isfinite(s[first:]).all() and np.all(s[first:] > 0.0)
    assert np.all(var["bad_by_round"] == 0)
    assert var["samples"].shape == var["samples_t"].shape == (n_keep, model.D, Cn) and var["logpost"].shape == (n_keep, Cn) and np.all(np.isfinite(var["logpost"]))
    assert var["betas_by_round"].shape == (R + 1, T) and var["rejection_by_round"].shape == (R, T - 1) and var["barrier_by_round"].shape == (R,)
    assert var["restarts"]["per_chain"].shape == (Cn,) and var["restarts"]["total"] > 0 and out["restarts"]["total"] > 0
    if vc.DRIVER_BARRIER_ASSERTED:
        assert lam_v < lam


def test_gpu_the_variational_leg_with_the_slice_explorer_and_the_default_without_it(pkg, model):
    T, Tv, Cn, R = 4, 3, 8, pc.SLICE_ROUNDS
    out = pkg.octofit_pigeons_device(model, T, Cn, R, slice_w=2.0, slice_p=3, n_passes=1, seed=5, n_temps_variational=Tv, first_tuning_round=2)
    var = out["variational"]
    assert out["samples_t"].shape == var["samples_t"].shape == (2 ** R, model.D, Cn) and np.all(np.isfinite(out["logpost"])) and np.all(np.isfinite(var["logpost"]))
    assert var["betas_by_round"].shape == (R + 1, Tv) and out["betas_by_round"].shape == (R + 1, T) and var["slice_evals"].shape == (Tv,)
    assert np.all(np.isfinite(var["barrier_by_round"])) and np.isfinite(var["log_evidence"]["fwd"]) and np.isfinite(out["log_evidence"]["fwd"])
    assert np.isfinite(var["mean_by_round"][0:]).all() and np.all(var["sd_by_round"] > 0.0) and np.all(var["bad_by_round"] == 0)
    plain = pkg.octofit_pigeons_device(model, T, Cn, 2, slice_w=2.0, slice_p=3, n_passes=1, seed=5)
    assert "variational" not in plain
    with pytest.raises(ValueError):
        pkg.octofit_pigeons_device(model, T, Cn, R, n_temps_variational=1)
    with pytest.raises(ValueError):
        pkg.octofit_pigeons_device(model, T, Cn, R, n_temps_variational=2, inflate=0.0)
