"""
Nested sampling on the device (include/octofitter_hip_draws.h: octo_draws_cube_device, octo_draws_from_cube_device,
octo_draws_nested_cull_device, octo_draws_nested_move_device; host/draws.py: PriorDraws.cube … nested_step; host/callers.py:
octofit_nested_device) against its NumPy restatement (tests/nested_reference.py) fed by the oracle's callback, and against brute force from the
rejection driver. tests/nested_cases.py states the cases.

What holds bit for bit: from_cube(cube(…)) against sample; the cull's order, seeds, copies, widths and dead u / ℓ; a chain's result whatever
B, ld, its position in d_slot and the cut of the rounds. At TRANS_BAR = 1e-11: the cull's log volumes, log weights and state. With the model,
u, θ_t and ℓ at the project's oracle bar 1e-8 relative to max(1, |ref|), the counts and the status on DECIDED chains.
"""
import math

import numpy as np
import pytest

import draws_cases as cases
import nested_cases as nc
import nested_reference as nr
from draws_device import TRANS_BAR, close, draws_mod, hmc_model, mirror_priors, set_batch_invariant      # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def model_pd(pkg, draws_mod):
    model = hmc_model(pkg)
    pd = draws_mod.PriorDraws(model)
    yield model, pd
    pd.close()
    model.close()


@pytest.fixture(scope="module")
def prior_pds(pkg, draws_mod):
    """handles without a model at D = 1, 5 (cases.STAT_PRIORS), 14 and 64: STAT_PRIORS in turn"""
    hs = {D: draws_mod.PriorDraws(priors=mirror_priors(pkg, [cases.STAT_PRIORS[k % 5] for k in range(D)])) for D in (1, 5, 14, 64)}
    yield hs
    for h in hs.values():
        h.close()


def nan_matrix(torch, rows, n, extra=5):
    """(buffer, view): a [rows, n] view of leading dimension n + extra of a NaN-filled buffer"""
    buf = torch.full((rows, n + extra), NAN, dtype=torch.float64, device="cuda")
    return buf, buf[:, :n]


# ---------------------------------------------------------------------------------------------------- 1. from_cube(cube(…)) = sample
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_gpu_from_cube_of_cube_is_sample_byte_for_byte(prior_pds, model_pd, n):
    import torch
    handles = [("D = 1", prior_pds[1]), ("the five priors", prior_pds[5]), ("D = 64", prior_pds[64]), ("the model's 14", model_pd[1])]
    for what, pd in handles:
        D, seed, first = pd.D, 19, 1000 + n
        want = pd.sample(seed, first, n)
        ubuf, u = nan_matrix(torch, D, n)
        pd.cube(seed, first, n, out=u)
        bufs = [nan_matrix(torch, D, n), nan_matrix(torch, D, n)]
        lbuf = torch.full((n + 5,), NAN, dtype=torch.float64, device="cuda")
        pd.from_cube(u, out=(bufs[0][1], bufs[1][1], lbuf[:n]))
        torch.cuda.synchronize()
        uh = u.cpu().numpy()
        assert np.array_equal(uh, nr.cube(seed, first, n, D)), what                 # the cube is the restatement's, bit for bit
        for got, ref_t, name in ((bufs[0][1], want[0], "theta"), (bufs[1][1], want[1], "theta_t"), (lbuf[:n], want[2], "logprior_t")):
            assert torch.equal(got, ref_t), (what, n, name)
        for buf in (ubuf, bufs[0][0], bufs[1][0]):
            assert bool(torch.isnan(buf[:, n:]).all()), what                         # nothing written beyond column n
        assert bool(torch.isnan(lbuf[n:]).all())
        # single outputs, and a u of 0, 1, NaN: that draw's outputs are NaN, the others keep their bits
        only_t = pd.from_cube(u, theta=False, logprior_t=False)
        assert only_t[0] is None and only_t[2] is None and torch.equal(only_t[1], want[1])
        if n >= 63:
            bad = {3: 0.0, 40: 1.0, n - 1: NAN, 7: -0.25, 8: 1.5}
            u2 = u.clone()
            for col, v in bad.items():
                u2[(col * 5) % D, col] = v
            th, tt, lp = pd.from_cube(u2)
            torch.cuda.synchronize()
            cols = sorted(bad)
            keep = np.setdiff1d(np.arange(n), cols)
            assert bool(torch.isnan(th[:, cols]).all()) and bool(torch.isnan(tt[:, cols]).all()) and bool(torch.isnan(lp[cols]).all()), what
            assert torch.equal(th[:, keep], want[0][:, keep]) and torch.equal(tt[:, keep], want[1][:, keep]) and torch.equal(lp[keep], want[2][keep]), what


# ---------------------------------------------------------------------------------------------------- 2. the cull
def device_cull(torch, pd, u, ll, state, B, replace, seed, it, dead_first=3):
    """one cull on padded device arrays; returns the host copies and asserts that nothing was written beyond the stated extents"""
    D, K = u.shape
    ubuf, uv = nan_matrix(torch, D, K)
    uv[:] = torch.as_tensor(u, device="cuda")
    lbuf = torch.full((K + 5,), NAN, dtype=torch.float64, device="cuda")
    lbuf[:K] = torch.as_tensor(ll, device="cuda")
    st = torch.as_tensor(np.asarray(state, dtype=np.float64), device="cuda").clone()
    n = dead_first + B + 4
    dead = dict(u=torch.full((D, n), NAN, dtype=torch.float64, device="cuda"), **{k: torch.full((n,), NAN, dtype=torch.float64, device="cuda")
                                                                                 for k in ("loglike", "logvol", "logwt")})
    slot = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    width = torch.full((D,), NAN, dtype=torch.float64, device="cuda")
    pd.nested_cull(uv, lbuf[:K], st, B, replace=replace, seed=seed, iter=it, dead=dead, dead_first=dead_first, slot=slot, width=width)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ubuf[:, K:]).all()) and bool(torch.isnan(lbuf[K:]).all())
    rec = slice(dead_first, dead_first + B)
    for k, t in dead.items():
        h = t.cpu().numpy()
        assert np.all(np.isnan(h[..., :dead_first])) and np.all(np.isnan(h[..., dead_first + B:])), k
    assert slot[B:].tolist() == [-7, -7]
    if not replace:
        assert bool(torch.isnan(width).all())
    return dict(u_live=uv.cpu().numpy(), ll_live=lbuf[:K].cpu().numpy(), state=st.cpu().numpy(), slot=slot[:B].cpu().numpy(), width=width.cpu().numpy(),
                dead_u=dead["u"][:, rec].cpu().numpy(), dead_ll=dead["loglike"][rec].cpu().numpy(), dead_logvol=dead["logvol"][rec].cpu().numpy(),
                dead_logwt=dead["logwt"][rec].cpu().numpy())


def close_with_infinities(got, want, bar):
    """draws_device.close on the finite entries; an infinite entry must be the same infinity"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isinf(want)
    return np.array_equal(got[inf], want[inf]) and close(got[~inf], want[~inf], bar)


def cull_agrees(got, want, replace, what):
    for k in ("slot", "dead_u", "dead_ll", "u_live", "ll_live") + (("width",) if replace else ()):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)                  # bitwise
    for k in ("dead_logvol", "dead_logwt", "state"):
        assert close_with_infinities(got[k], want[k], TRANS_BAR), (what, k, got[k][:4], want[k][:4])


@pytest.mark.parametrize("kind", nc.CULL_B)
@pytest.mark.parametrize("K", nc.CULL_K)
def test_gpu_cull_against_the_restatement(prior_pds, K, kind):
    import torch
    B, replace = nc.cull_batch(K, kind)
    for D in nc.cull_dims(K):
        for variant in nc.CULL_VARIANTS:
            what = (K, kind, D, variant)
            u, ll = nc.cull_live(K, D, B, variant)
            state = np.array(nr.STATE0)
            with np.errstate(all="ignore"):
                if not replace:      # the flush follows an iteration: the state is not the initial one
                    first = nr.cull(u, ll, state, 1, True, nc.CULL_SEED, 0)
                    got1 = device_cull(torch, prior_pds[D], u, ll, state, 1, True, nc.CULL_SEED, 0)
                    cull_agrees(got1, first, True, what + ("first",))
                    u, ll, state = first["u_live"], first["ll_live"], first["state"]
                want = nr.cull(u, ll, state, B, replace, nc.CULL_SEED, 1)
            got = device_cull(torch, prior_pds[D], u, ll, state, B, replace, nc.CULL_SEED, 1)
            cull_agrees(got, want, replace, what)
            assert got["state"][5] == want["state"][5] and got["state"][6] == got["state"][7] == 0.0
            if replace:      # the second iteration, chained through the state and the live set the device left
                with np.errstate(all="ignore"):
                    want2 = nr.cull(got["u_live"], got["ll_live"], got["state"], B, True, nc.CULL_SEED, 2)
                got2 = device_cull(torch, prior_pds[D], got["u_live"], got["ll_live"], got["state"], B, True, nc.CULL_SEED, 2)
                cull_agrees(got2, want2, True, what + ("second",))


# ---------------------------------------------------------------------------------------------------- 3. the move against the restatement
@pytest.fixture(scope="module")
def move_setup(oracle):
    loglike = nc.model_loglike(oracle)
    u, ll = nc.move_live(loglike)
    return loglike, u, ll


def live_on_device(torch, u, ll):
    return torch.as_tensor(np.array(u), device="cuda").contiguous(), torch.as_tensor(np.array(ll), device="cuda").contiguous()


@pytest.mark.parametrize("B", nc.MOVE_B)
def test_gpu_move_against_the_restatement(pkg, model_pd, move_setup, B):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 0)
    loglike, u, ll = move_setup
    D, K = u.shape
    c = nr.cull(u, ll, nr.STATE0, B, True, nc.MOVE_SEED, nc.MOVE_ITER)
    r = nr.move(loglike, c["u_live"], c["ll_live"], float(c["state"][2]), c["slot"], c["width"], nc.MOVE_STEPS, nc.MOVE_PASSES, nr.MAX_SHRINK, nc.MOVE_SEED, nc.MOVE_ITER)
    print(f"B = {B}: {nc.summary(r)}")
    assert nc.undecided(r) <= cases.ONE_UNDECIDED, "condition on the seed (the reference alone)"      # before the device runs
    assert np.all(r["status"] == nr.DONE)
    ud, ld_ = live_on_device(torch, u, ll)
    state = pd.nested_state()
    out = pd.nested_step(ud, ld_, state, B, max_steps=nc.MOVE_STEPS, n_passes=nc.MOVE_PASSES, seed=nc.MOVE_SEED, iter=nc.MOVE_ITER, want_theta_t=True)
    torch.cuda.synchronize()
    assert int(out["n_active"].item()) == 0
    slot = out["slot"].cpu().numpy()
    assert np.array_equal(slot, c["slot"]) and np.array_equal(out["width"].cpu().numpy(), c["width"]) and close_with_infinities(state.cpu().numpy(), c["state"], TRANS_BAR)
    decided = r["margin"] > nr.MARGIN
    for k in nc.COUNTS:
        g = out[k].cpu().numpy()
        assert np.array_equal(g[decided], r[k][decided]), (k, np.nonzero(decided & (g != r[k]))[0])
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)), initial=0.0))      # noqa: E731
    got_u, got_ll, got_tt = ud.cpu().numpy(), ld_.cpu().numpy(), out["theta_t"].cpu().numpy()
    s = slot[decided]
    want_tt = nr.from_cube(cases.MODEL_PRIORS, r["u_live"][:, slot])[1]
    e_u, e_ll, e_tt = rel(got_u[:, s], r["u_live"][:, s]), rel(got_ll[s], r["ll_live"][s]), rel(got_tt[:, decided], want_tt[:, decided])
    print(f"B = {B}: max errors on decided chains — u {e_u:.3e}, ℓ {e_ll:.3e}, θ_t {e_tt:.3e} (relative to max(1, |ref|), bar 1e-08)")
    assert e_u <= 1e-8 and e_ll <= 1e-8 and e_tt <= 1e-8
    stay = decided[None, :] & (r["u_live"][:, slot] == c["u_live"][:, slot])                   # a coordinate that did not move keeps its bits
    assert np.array_equal(got_u[:, slot][stay], c["u_live"][:, slot][stay])
    keep = np.setdiff1d(np.arange(K), slot)                                                     # survivors are only read
    assert np.array_equal(got_u[:, keep], u[:, keep]) and np.array_equal(got_ll[keep], ll[keep])
    assert np.all(got_ll[slot] > c["state"][2]) and np.all((got_u > 0) & (got_u < 1))


# ---------------------------------------------------------------------------------------------------- 4. invariance, bitwise
def run_move(torch, pd, u, ll, state, slot, cuts=(None,), ld=None, **kw):
    """one transition of `slot` on fresh copies of the live set, the rounds cut as `cuts` (None: all that finish every chain); returns host copies"""
    ud, ld_ = live_on_device(torch, u, ll)
    st = torch.as_tensor(np.asarray(state), device="cuda").clone()
    sl = torch.as_tensor(np.asarray(slot, dtype=np.int32), device="cuda")
    B, D = sl.numel(), ud.shape[0]
    args = dict(dict(w=0.5, max_steps=4, n_passes=1, max_shrink=nr.MAX_SHRINK, seed=nc.MOVE_SEED, iter=nc.MOVE_ITER), **kw)
    most = args["n_passes"] * D * (args["max_steps"] - 1 + args["max_shrink"])
    i32 = lambda n: torch.full((n,), -3, dtype=torch.int32, device="cuda")      # noqa: E731
    tbuf, tv = nan_matrix(torch, D, B, extra=0 if ld is None else ld - B)
    out = dict(theta_t=tv, n_eval=i32(B), n_step=i32(B), n_shrink=i32(B), n_stuck=i32(B), status=i32(B), n_active=i32(1))
    frozen = None
    for k, n in enumerate(cuts):
        pd.nested_move(ud, ld_, st, sl, n_rounds=most if n is None else n, resume=k > 0, out=out, **args)
        if k == 0 and len(cuts) > 1:
            torch.cuda.synchronize()
            frozen = {key: v.clone() for key, v in out.items()}, ud.clone(), ld_.clone()
    torch.cuda.synchronize()
    assert bool(torch.isnan(tbuf[:, B:]).all())
    res = dict(u=ud.cpu().numpy()[:, slot], ll=ld_.cpu().numpy()[slot], **{k: v.cpu().numpy() for k, v in out.items()})
    return res, frozen, (ud, ld_)


def same_chains(a, b, ia=slice(None), ib=slice(None)):
    return [k for k in ("u", "ll", "theta_t", "n_eval", "n_step", "n_shrink", "n_stuck", "status") if not np.array_equal(a[k][..., ia], b[k][..., ib])]


def test_gpu_a_chains_result_depends_on_its_slot_alone(pkg, model_pd, move_setup):
    import torch
    model, pd = model_pd
    set_batch_invariant(pkg, model, 1)
    try:
        _loglike, u, ll = move_setup
        c = nr.cull(u, ll, nr.STATE0, 65, True, nc.MOVE_SEED, nc.MOVE_ITER)
        slot, state = c["slot"], c["state"]
        base, _, _ = run_move(torch, pd, c["u_live"], c["ll_live"], state, slot)
        assert base["n_active"][0] == 0 and np.all(base["status"] == nr.DONE) and base["n_step"].sum() > 0 and base["n_shrink"].min() >= 14
        # B and the position in d_slot: seven of the chains, in another order; ld: a padded θ_t
        pick = np.array([40, 3, 64, 0, 17, 33, 8])
        few, _, _ = run_move(torch, pd, c["u_live"], c["ll_live"], state, slot[pick], ld=12)
        assert same_chains(few, base, ib=pick) == []
        perm = np.random.default_rng(1).permutation(65)
        mixed, _, _ = run_move(torch, pd, c["u_live"], c["ll_live"], state, slot[perm], ld=70)
        assert same_chains(mixed, base, ib=perm) == []
        # the cut of the rounds: 0 + 9 + the rest against one call; chains frozen at the first cut keep their bits across resume
        cut, frozen, _ = run_move(torch, pd, c["u_live"], c["ll_live"], state, slot, cuts=(0, 9, None, 4))
        assert same_chains(cut, base) == [] and cut["n_active"][0] == 0
        early, frozen, _ = run_move(torch, pd, c["u_live"], c["ll_live"], state, slot, cuts=(33, None))
        done = (frozen[0]["status"] == nr.DONE).cpu().numpy()
        print(f"{done.sum()} of 65 chains done after 33 rounds")
        assert 0 < done.sum() < 65 and same_chains(early, base) == []
        assert np.array_equal(frozen[1].cpu().numpy()[:, slot[done]], base["u"][:, done]) and np.array_equal(frozen[2].cpu().numpy()[slot[done]], base["ll"][done])
        for k in ("n_eval", "n_step", "n_shrink", "n_stuck"):
            assert np.array_equal(frozen[0][k].cpu().numpy()[done], base[k][done]), k
        # scalar against per-coordinate widths
        per, _, _ = run_move(torch, pd, c["u_live"], c["ll_live"], state, slot, w=np.full(14, 0.5))
        assert same_chains(per, base) == []
        # m = 1: no stepping out
        m1, _, _ = run_move(torch, pd, c["u_live"], c["ll_live"], state, slot, max_steps=1)
        assert m1["n_step"].sum() == 0 and np.all(m1["status"] == nr.DONE) and np.all(m1["n_eval"] <= m1["n_shrink"])
        # max_shrink = 1 under a floor above every ℓ: every update is stuck after one proposal, u and ℓ are the seeds'
        high = state.copy()
        high[2] = 1e300
        stuck, _, _ = run_move(torch, pd, c["u_live"], c["ll_live"], high, slot, max_shrink=1)
        assert np.all(stuck["n_stuck"] == 14) and np.all(stuck["n_shrink"] == 14) and np.all(stuck["status"] == nr.DONE)
        assert np.array_equal(stuck["u"], c["u_live"][:, slot]) and np.array_equal(stuck["ll"], c["ll_live"][slot])
    finally:
        set_batch_invariant(pkg, model, 0)


# ---------------------------------------------------------------------------------------------------- 5. errors
def test_gpu_every_einval_with_its_message(pkg, draws_mod, model_pd, prior_pds):
    import torch
    model, pd = model_pd
    OctoError = pkg.capi.OctoError
    u = pd.cube(1, 0, 8)
    ll = torch.zeros(8, dtype=torch.float64, device="cuda")
    st = pd.nested_state()
    slot = torch.zeros(2, dtype=torch.int32, device="cuda")

    def refused(text, fn, *a, **kw):
        with pytest.raises(OctoError, match=text) as e:
            fn(*a, **kw)
        assert e.value.status == pkg.capi.OCTO_EINVAL

    big = torch.zeros((14, 4097), dtype=torch.float64, device="cuda")
    refused("K must be 2", pd.nested_cull, big, torch.zeros(4097, dtype=torch.float64, device="cuda"), st, 1)
    refused("K must be 2", pd.nested_cull, u[:, :1], ll[:1], st, 1)
    refused("B must be 1 ... K - 1 with replace = 1", pd.nested_cull, u, ll, st, 8)
    refused("B must be 1 ... K - 1 with replace = 1", pd.nested_cull, u, ll, st, 0)
    refused("and K with replace = 0", pd.nested_cull, u, ll, st, 7, replace=False)
    refused("dead_first", pd.nested_cull, u, ll, st, 2, dead_first=-1)
    lib, h, p = pd.lib, pd._h, lambda t: t.data_ptr()      # noqa: E731
    assert lib.octo_draws_nested_cull_device(h, 0, 0, 8, 7, p(u), p(ll), p(st), 1, 1, 0, 1, None, None, None, None, p(slot), None, None) == pkg.capi.OCTO_EINVAL
    assert b"K <= ldK" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_nested_cull_device(h, 0, 0, 8, 8, None, p(ll), p(st), 1, 1, 0, 1, None, None, None, None, p(slot), None, None) == pkg.capi.OCTO_EINVAL
    assert b"are required" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_nested_cull_device(h, 0, 0, 8, 8, p(u), p(ll), p(st), 1, 2, 0, 1, None, None, None, None, p(slot), None, None) == pkg.capi.OCTO_EINVAL
    assert b"replace must be 0 or 1" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_nested_cull_device(h, 0, 0, 8, 8, p(u), p(ll), p(st), 1, 1, 0, 1, None, None, None, None, None, None, None) == pkg.capi.OCTO_EINVAL
    assert b"d_slot is required" in lib.octo_draws_last_error(h)
    # the move
    refused("nested sampling needs a likelihood", prior_pds[14].nested_move, u, ll, st, slot)
    refused("w must be in \\(0, 1\\]", pd.nested_move, u, ll, st, slot, w=0.0)
    refused("w must be in \\(0, 1\\]", pd.nested_move, u, ll, st, slot, w=1.5)
    refused("w must be in \\(0, 1\\]", pd.nested_move, u, ll, st, slot, w=NAN)
    refused("max_steps must be 1 ... OCTO_DRAWS_NESTED_MAX_STEPS", pd.nested_move, u, ll, st, slot, max_steps=0)
    refused("max_steps must be 1 ... OCTO_DRAWS_NESTED_MAX_STEPS", pd.nested_move, u, ll, st, slot, max_steps=65)
    refused("max_shrink must be 1 ... OCTO_DRAWS_NESTED_MAX_SHRINK", pd.nested_move, u, ll, st, slot, max_shrink=0)
    refused("max_shrink must be 1 ... OCTO_DRAWS_NESTED_MAX_SHRINK", pd.nested_move, u, ll, st, slot, max_shrink=65)
    refused("n_passes must be 1 ... OCTO_DRAWS_NESTED_MAX_PASSES", pd.nested_move, u, ll, st, slot, n_passes=0)
    refused("n_passes must be 1 ... OCTO_DRAWS_NESTED_MAX_PASSES", pd.nested_move, u, ll, st, slot, n_passes=1025)
    refused("n_rounds >= 0", pd.nested_move, u, ll, st, slot, n_rounds=-1)
    refused("B <= K - 1", pd.nested_move, u, ll, st, torch.zeros(8, dtype=torch.int32, device="cuda"))
    refused("K must be 2", pd.nested_move, u[:, :1], ll[:1], st, slot[:0])
    move = lambda B, ld, *tail: lib.octo_draws_nested_move_device(h, 0, 0, 8, 8, p(u), p(ll), p(st), B, ld, p(slot), None, 0.5, 2, 1, 4, 0, *tail)      # noqa: E731
    assert move(2, 1, 0, *[None] * 8) == pkg.capi.OCTO_EINVAL and b"B <= ld" in lib.octo_draws_last_error(h)
    refused("resume needs a previous call", pd.nested_move, u, ll, st, slot, resume=True)
    pd.nested_cull(u, ll, st, 2, slot=slot)
    out = pd.nested_move(u, ll, st, slot, w=0.5, n_rounds=1)
    refused("resume needs a previous call", pd.nested_move, u, ll, st, slot, w=0.5, n_rounds=1, resume=True, out=out, iter=1)
    refused("resume needs a previous call", pd.nested_move, u, ll, st, slot, w=0.5, n_rounds=1, resume=True, out=out, n_passes=2)
    pd.nested_move(u, ll, st, slot, w=0.5, n_rounds=1, resume=True, out=out)      # the matching resume is taken
    # the cube
    assert lib.octo_draws_cube_device(h, 0, 0, 4, 3, p(u), None) == pkg.capi.OCTO_EINVAL and b"0 <= n <= ld" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_cube_device(h, 0, 2 ** 64 - 2, 4, 4, p(u), None) == pkg.capi.OCTO_EINVAL and b"overflows" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_cube_device(h, 0, 0, 4, 4, None, None) == pkg.capi.OCTO_EINVAL and b"d_u is required" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_from_cube_device(h, 4, 3, p(u), p(u), None, None, None) == pkg.capi.OCTO_EINVAL and b"0 <= n <= ld" in lib.octo_draws_last_error(h)
    assert lib.octo_draws_from_cube_device(h, 4, 4, None, p(u), None, None, None) == pkg.capi.OCTO_EINVAL and b"d_u is required" in lib.octo_draws_last_error(h)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 6. end to end
def test_gpu_nested_sampling_against_brute_force_from_the_rejection_driver(pkg, model_pd):
    """logZ_bf = max ℓ + log(n_accepted/N) from the rejection driver on N = 2²⁰ prior draws, standard error 1/√n_accepted (draws_cases.POST_LEAST = 2000 is
    the floor on n_accepted). Measured on the MI355X (nested seed 5, rejection seed 31): logZ −274.5027 against −274.5116 from 2 898 accepted draws, a
    difference of +0.0089 with H = 4.235 against the bar 4·√(H/K + 1/n_accepted) = 0.268; θ_t means within 2.6 combined standard errors."""
    model, pd = model_pd
    N = cases.POST_N
    rej = pd.rejection(cases.POST_SEEDS[0], N)
    n_acc = rej["n_accepted"]
    assert n_acc >= cases.POST_LEAST, n_acc
    logz_bf = rej["max_loglike"] + math.log(n_acc / N)
    r = pkg.octofit_nested_device(model, seed=5)
    bar = 4.0 * math.sqrt(r["information"] / 1024 + 1.0 / n_acc)
    print(f"logZ {r['logz']:+.4f} ± {r['logz_err']:.4f} (H {r['information']:.3f}); brute force {logz_bf:+.4f} from {n_acc} accepted of {N}; "
          f"difference {r['logz'] - logz_bf:+.4f}, bar {bar:.4f}; {r['n_iter']} iterations, {r['n_evals']} evaluations, {r['n_stuck']} stuck, ESS {r['ess']:.0f}")
    assert r["n_iter"] < 2000 and r["theta"].shape == (14, r["n_iter"] * 256 + 1024) and r["samples"].shape == (14, 4096)
    assert abs(r["weights"].sum() - 1.0) < 1e-9 and np.all(np.isfinite(r["theta_t"]))
    assert abs(r["logz"] - logz_bf) <= bar
    tt_rej = model.link(rej["samples"])
    n_eff = min(r["ess"], r["samples_t"].shape[1])
    se = np.sqrt(tt_rej.var(axis=1) / n_acc + r["samples_t"].var(axis=1) / n_eff)
    z = (r["samples_t"].mean(axis=1) - tt_rej.mean(axis=1)) / se
    print("θ_t means, nested − rejection, in combined standard errors:", np.round(z, 2))
    assert np.all(np.abs(z) <= 4.0), z


# ---------------------------------------------------------------------------------------------------- 7. a handle carrying a program
def bare_model(pkg):
    """The test model with every kernel input a bare parameter or a constant: ω, Ω and tp have priors of their own in place of UniformCircular
    variables, so that a program that is the identity on the model's inputs holds constants and bindings and not one arithmetic op."""
    astrom_t, rv_t = cases.model_tables()
    astrom = pkg.PlanetRelAstromObs(astrom_t, name="sim")
    rv = pkg.StarAbsoluteRVObs(rv_t, name="rv", variables=pkg.variables(offset=pkg.Normal(0, 20), jitter=pkg.LogUniform(0.1, 20.0)))
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom],
                   variables=pkg.variables(a=pkg.LogUniform(5, 20), e=pkg.Uniform(0.0, 0.6), i=pkg.Sine(), ω=pkg.Uniform(0.0, 2 * math.pi), Ω=pkg.Uniform(0.0, 2 * math.pi),
                                           tp=pkg.Uniform(49000.0, 51000.0), mass=pkg.LogUniform(1.0, 50.0)))
    sys_ = pkg.System(name="sim", companions=[b], observations=[rv],
                      variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.05), lower=0.1), plx=pkg.truncated(pkg.Normal(50.0, 0.1), lower=0.1)))
    return pkg.LogDensityModel(sys_)


def one_step_on_both_handles(torch, pkg, draws_mod, model, pd, tp):
    """one nested_step of 65 of 320 live points on the plain handle and on a handle carrying the model's identity program, everything on the host"""
    tape, binds, terms = tp.identity_program(pkg, model)
    u = pd.cube(nc.MOVE_SEED, 0, nc.MOVE_K)
    _, tt, lpt = pd.from_cube(u, theta=False)
    ll = model.logpost_device(tt, grad=False)[0] - lpt
    ll = torch.where(torch.isfinite(ll), ll, torch.full_like(ll, -float("inf"))).contiguous()
    results = []
    for handle in (pd, draws_mod.PriorDraws(model, program=(tp.as_program(pkg, tape, terms), binds))):
        try:
            ud, ld_, state = u.clone(), ll.clone(), handle.nested_state()
            out = handle.nested_step(ud, ld_, state, 65, max_steps=nc.MOVE_STEPS, n_passes=1, seed=nc.MOVE_SEED, iter=nc.MOVE_ITER, want_theta_t=True)
            torch.cuda.synchronize()
            results.append(dict(u=ud.cpu().numpy(), ll=ld_.cpu().numpy(), state=state.cpu().numpy(), **{k: v.cpu().numpy() for k, v in out.items()}))
        finally:
            if handle is not pd:
                handle.close()
    a, b = results
    assert a["n_active"][0] == 0 and a["n_eval"].min() >= a["u"].shape[0]      # every chain made its D updates
    worst = float(np.max(np.abs(a["ll"] - b["ll"]) / np.maximum(1.0, np.abs(a["ll"]))))
    return [k for k in a if not np.array_equal(a[k], b[k])], worst, tape


def test_gpu_an_identity_program_gives_the_bits_of_the_plain_handle(pkg, draws_mod, model_pd):
    """A program that is the identity on the model's inputs — bindings and constants, no arithmetic of its own — gives the bits of the plain handle
    in every output of one nested_step. On the test model itself, whose UniformCircular variables the program turns into angles with its own
    atan2 and multiplication, the decisions, u, θ_t and the counts are still the plain handle's bits, and the stored ℓ agree to a few ulp
    (measured on the MI355X: 3.7e-16 relative), which is the agreement tests/test_program.py holds the two evaluators to (1e-12)."""
    import torch
    import test_program as tp
    model = bare_model(pkg)
    pd = draws_mod.PriorDraws(model)
    try:
        diff, worst, tape = one_step_on_both_handles(torch, pkg, draws_mod, model, pd, tp)
        print(f"bare model, program against plain handle: keys that differ {diff}; largest relative difference of ℓ {worst:.3e}; ops {[op for op in tape.ops][:3]} … ({len(tape.ops)})")
        assert diff == []
    finally:
        pd.close()
        model.close()
    model, pd = model_pd
    diff, worst, _ = one_step_on_both_handles(torch, pkg, draws_mod, model, pd, tp)
    print(f"test model (circular variables), program against plain handle: keys that differ {diff}; largest relative difference of ℓ {worst:.3e}")
    assert set(diff) <= {"ll"} and worst <= 1e-12
