"""
The restatement of nested sampling (tests/nested_reference.py) by itself, on the CPU: the two new purposes of the counter generator collide
with none of purposes 0 - 9; the lockstep restatement of the move gives the bits and counts of the plainest statement (chain by chain, nested
loops); the cull matches a plain np.lexsort statement on tie blocks, −Inf and NaN entries, B = 1, B = K − 1 and the flush; and the algorithm
as stated is right: on uniform priors with a normalised Gaussian likelihood, whose evidence is analytic, every seed at the driver's defaults
gives |logZ − exact| <= 4·√(H/K) and resampled coordinate means within 4 standard errors of ½. tests/nested_cases.py states the cases.
"""
import math

import numpy as np
import pytest

import hmc_reference as ref
import nested_cases as nc
import nested_reference as nr


def test_the_new_purposes_collide_with_no_other():
    assert (nr.PURPOSE_NESTED_SEED, nr.PURPOSE_NESTED_MOVE) == (10, 11)
    assert nr.seed_counter(3, 9)[2] == 10 and nr.move_counter(3, 2, 64, 9)[2] == 11
    # the purpose is counter word 2 in every stream of the library: purposes 0 … 9 never produce these counters, and the words differ
    seen = {}
    for purpose in range(12):
        for c0, c1, c3 in ((0, 0, 0), (5, 1, 7), (2 ** 40, 64 * 128 + 127, 3)):
            words = ref.philox_int((123, ref.KEY1), (c0, c1, purpose, c3))
            assert words not in seen, (purpose, seen.get(words))
            seen[words] = purpose
    vec = nr.move_uniforms(123, 7, np.array([5]), np.array([1]), np.array([3]))
    words = ref.philox_int((123, ref.KEY1), nr.move_counter(5, 1, 3, 7))
    assert [float(v[0]) for v in vec] == [nr._u01_int(w) for w in words[:3]]


# ---------------------------------------------------------------------------------------------------- the move: lockstep against plain
@pytest.fixture(scope="module")
def gauss_live():
    """64 live points under the analytic likelihood and the cull of 24 of them: what the move cases start from (shared, never modified)"""
    u = nr.cube(11, 0, 64, nc.GAUSS_D)
    c = nr.cull(u, nc.gauss_loglike(u), nr.STATE0, 24, True, seed=11, it=2)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("name,w,m,passes,shrink", [("defaults", None, 8, 2, 64), ("no stepping out", None, 1, 2, 64), ("every update stuck", 0.3, 4, 1, 1),
                                                    ("scalar width", 1.0, 3, 1, 64), ("narrow scalar width", 0.01, 64, 1, 3)])
def test_the_lockstep_move_gives_the_bits_and_counts_of_the_plain_statement(gauss_live, name, w, m, passes, shrink):
    c = gauss_live
    width = c["width"] if w is None else w
    floor = 1e300 if shrink == 1 else float(c["state"][2])      # a floor above every ℓ: nothing is inside
    args = (nc.gauss_loglike, c["u_live"], c["ll_live"], floor, c["slot"], width, m, passes, shrink, 11, 2)
    a, b = nr.move(*args), nr.move_plain(*args)
    print(f"{name}: {nc.summary(a)}")
    for k in ("u_live", "ll_live") + nc.COUNTS:
        assert np.array_equal(a[k], b[k]), (name, k)
    assert (shrink == 1 or np.all(a["ll_live"][c["slot"]] > floor)) and np.all((a["u_live"] > 0) & (a["u_live"] < 1))
    others = np.setdiff1d(np.arange(64), c["slot"])
    assert np.array_equal(a["u_live"][:, others], c["u_live"][:, others])      # survivors are only read
    if shrink == 1:      # every update is stuck after its one proposal: u and ℓ are the seeds'
        assert np.all(a["n_stuck"] == passes * nc.GAUSS_D) and np.all(a["n_shrink"] == passes * nc.GAUSS_D) and a["n_step"].sum() == 0
        assert np.array_equal(a["u_live"], c["u_live"]) and np.array_equal(a["ll_live"], c["ll_live"])
    if m == 1:
        assert a["n_step"].sum() == 0
    if m == 64:
        assert a["n_step"].max() > 3
    # the rounds may be cut anywhere: the chains that are done by then hold their final bits
    cut = nr.move(*args, max_rounds=5)
    done = cut["status"] == nr.DONE
    assert np.array_equal(cut["u_live"][:, c["slot"][done]], a["u_live"][:, c["slot"][done]])


# ---------------------------------------------------------------------------------------------------- the cull against np.lexsort
def cull_plain(u, ll, state, B, replace, seed, it):
    K = ll.size
    key = np.where(np.isnan(ll) | (ll == -np.inf), -np.inf, ll)
    order = np.lexsort((np.arange(K), key))
    t = 1.0 / (K - np.arange(B))
    logvol = state[1] - np.cumsum(t)
    before = np.concatenate([[state[1]], logvol[:-1]])
    logwt = key[order[:B]] + before + np.log(-np.expm1(-t))
    logz = np.logaddexp.reduce(np.concatenate([[state[0]], logwt]))
    out = dict(order=order, slot=order[:B], dead_ll=key[order[:B]], dead_u=u[:, order[:B]], dead_logvol=logvol, dead_logwt=logwt, logz=logz,
               floor=key[order[B - 1]], lmax=np.max(key))
    if replace:
        v = np.array([nr._u01_int(ref.philox_int((seed, ref.KEY1), nr.seed_counter(r, it))[0]) for r in range(B)])
        out["src"] = order[B + np.minimum(K - B - 1, np.floor(v * (K - B)).astype(int))]
        out["width"] = np.nanmax(u, axis=1) - np.nanmin(u, axis=1)
    return out


@pytest.mark.parametrize("K", [2, 5, 64, 257])
@pytest.mark.parametrize("kind", nc.CULL_B)
def test_the_cull_matches_a_plain_lexsort_statement(K, kind):
    B, replace = nc.cull_batch(K, kind)
    for variant in nc.CULL_VARIANTS:
        u, ll = nc.cull_live(K, 3, B, variant)
        state = np.array(nr.STATE0)
        state[:2] = (-3.0, -0.25)
        with np.errstate(all="ignore"):
            got, want = nr.cull(u, ll, state, B, replace, seed=5, it=3), cull_plain(u, ll, state, B, replace, 5, 3)
        what = (K, kind, variant)
        assert np.array_equal(got["order"], want["order"]) and np.array_equal(got["slot"], want["slot"]), what
        assert np.array_equal(got["dead_ll"], want["dead_ll"]) and np.array_equal(got["dead_u"], want["dead_u"]), what
        assert np.allclose(got["dead_logvol"], want["dead_logvol"], rtol=0, atol=1e-12), what
        fin = np.isfinite(want["dead_logwt"])
        assert np.array_equal(got["dead_logwt"][~fin], want["dead_logwt"][~fin]) and np.allclose(got["dead_logwt"][fin], want["dead_logwt"][fin], rtol=1e-13, atol=1e-12), what
        st = got["state"]
        assert math.isclose(st[0], want["logz"], rel_tol=1e-13, abs_tol=1e-12) and math.isclose(st[1], want["dead_logvol"][-1], abs_tol=1e-12), what
        assert st[2] == want["floor"] and st[3] == want["lmax"] and st[5] == B and st[6] == st[7] == 0.0, what
        assert math.isclose(st[4], np.logaddexp(st[0], st[3] + st[1]) - st[0], rel_tol=1e-12, abs_tol=1e-12), what
        if replace:
            assert np.array_equal(got["src"], want["src"]) and np.array_equal(got["width"], want["width"]), what
            assert np.array_equal(got["u_live"][:, got["slot"]], u[:, want["src"]]) and np.array_equal(got["ll_live"][got["slot"]], ll[want["src"]], equal_nan=True), what
            keep = np.setdiff1d(np.arange(K), got["slot"])
            assert np.array_equal(got["u_live"][:, keep], u[:, keep]) and np.array_equal(got["ll_live"][keep], ll[keep], equal_nan=True), what
            assert not np.intersect1d(want["src"], got["slot"]).size, what      # a seed is a survivor
        else:
            assert np.array_equal(got["u_live"], u) and got["width"] is None and sorted(got["slot"]) == list(range(K)), what
        if variant == "ties" and K > 2:      # the tie block straddles rank B: the lower slots die
            block = np.nonzero(ll == got["dead_ll"][-1])[0]
            dead_of_block = np.intersect1d(block, got["slot"])
            assert np.array_equal(dead_of_block, block[:dead_of_block.size]), what


def test_the_initial_state_and_the_volume_of_a_whole_run():
    """from the initial state, culls of B until the flush remove every point once, and the shells' volumes telescope: Σ exp(logwt − ℓ) = 1 − X at the end"""
    K, B = 64, 16
    u = nr.cube(3, 0, K, 2)
    ll = np.zeros(K)      # ℓ = 0: logwt is the log of the volume of the shell, and Z = 1
    state, lw = np.array(nr.STATE0), []
    for it in range(5):
        c = nr.cull(u, ll, state, B, True, 3, it)
        u, ll, state = c["u_live"], c["ll_live"], c["state"]
        lw.append(c["dead_logwt"])
        assert state[5] == B * (it + 1)
    c = nr.cull(u, ll, state, K, False, 3, 5)
    lw.append(c["dead_logwt"])
    left = math.exp(c["state"][1])      # the volume inside the last dead point, which the flush's rule leaves out: about X/(1.78·K)
    assert abs(np.sum(np.exp(np.concatenate(lw))) - (1.0 - left)) < 1e-12 and abs(c["state"][0] - math.log1p(-left)) < 1e-12 and left < 0.01


# ---------------------------------------------------------------------------------------------------- the algorithm is right
@pytest.fixture(scope="module")
def gauss_runs():
    return {seed: nr.run(nc.gauss_loglike, nc.GAUSS_D, seed=seed) for seed in nc.GAUSS_SEEDS}


def test_the_evidence_of_a_gaussian_at_the_drivers_defaults(gauss_runs):
    exact = nc.gauss_logz()
    for seed, r in gauss_runs.items():
        print(f"seed {seed}: logZ {r['logz']:+.4f} (exact {exact:+.2e}), √(H/K) {r['logz_err']:.4f}, H {r['information']:.3f}, {r['n_iter']} iterations, "
              f"{r['n_evals']} evaluations, {r['n_stuck']} stuck, ESS {r['ess']:.0f}; error {(r['logz'] - exact) / r['logz_err']:+.2f} σ")
        assert r["state"][4] < nr.DEFAULTS["dlogz"] and r["n_iter"] < nr.DEFAULTS["max_iter"]
        assert abs(r["logz"] - exact) <= 4.0 * r["logz_err"], seed
        assert r["u"].shape[1] == r["n_iter"] * nr.DEFAULTS["batch"] + nr.DEFAULTS["n_live"] == r["state"][5]
        assert abs(r["weights"].sum() - 1.0) < 1e-9


def test_the_resampled_draws_have_the_exact_means(gauss_runs):
    for seed, r in gauss_runs.items():
        s = r["samples_u"]
        assert s.shape == (nc.GAUSS_D, nr.DEFAULTS["n_samples"])
        se = nc.GAUSS_SIGMA / math.sqrt(min(r["ess"], s.shape[1]))      # the draws carry no more information than the weighted set
        z = (s.mean(axis=1) - 0.5) / se
        print(f"seed {seed}: resampled means − ½ = {s.mean(axis=1) - 0.5} ({z} standard errors of {se:.2e}); sd {s.std(axis=1)}")
        assert np.all(np.abs(z) <= 4.0), (seed, z)
        assert np.all(np.abs(s.std(axis=1) / nc.GAUSS_SIGMA - 1.0) < 0.1)
