"""
The per-datum log-likelihood matrix and its WAIC / LOO sums on the device (include/octofitter_hip_pointwise.h, host/pointwise.py) — GPU suite.

The reference is always the oracle on ONE-ROW sub-tables (every column sliced, `extra` included, with the table's three nuisance rows): never
the device's own output. Bars:
  values, closure   1e-11 · max(1, |ll_ref|) per entry: the bar tests/test_model.py holds `pointwise_like` to;
  invariance        bitwise;
  summary           with δ = the largest per-entry bar of the row and n = its valid count:
                    lppd, elpd_is_loo, mean, min, max within δ + n · 2⁻⁵² · max(1, |ref|) (a log-mean-exp moves by at most the largest move of
                    its inputs; the rest is the rounding of n fixed-order additions), the variance within
                    4 · sd_ref · δ + δ² + n · 2⁻⁵² · var_ref (first order in the inputs' error), n exact.
The observed maxima are printed (tools/pointwise_bench.py writes them to profiles/pointwise_throughput.txt).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pointwise_reference import (NROWS, RVO, TI, KEP, V, check_summary, check_values, five_planets, head, random_nuis,  # noqa: E402
                                 random_table, reference_matrix, table_values)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def padded(a, pad=5):
    """The same rows inside a wider array: a leading dimension larger than the batch."""
    buf = np.full((a.shape[0], a.shape[1] + pad), np.nan)
    buf[:, :a.shape[1]] = a
    return buf


def device_matrix(pkg, pw, elems, nuis, pad=5):
    """The matrix through the C ABI's host-buffer call with ld > W and ld_out > W."""
    import ctypes as C
    capi = pkg.capi
    W = elems.shape[1]
    el = padded(elems, pad)
    nu = None if nuis is None else padded(nuis, pad)
    out = np.full((pw.n_rows, W + pad + 2), 123.0)
    st = pw.lib.octo_pointwise_eval(pw._h, capi._dptr(el), W + pad, W, capi._dptr(nu), capi._dptr(out), W + pad + 2)
    assert st == capi.OCTO_OK, (st, pw.lib.octo_pointwise_last_error(pw._h))
    assert np.all(out[:, W:] == 123.0)      # nothing written past the batch
    return np.ascontiguousarray(out[:, :W])


@pytest.fixture(scope="module")
def two_planets(oracle):
    """Two planets with masses; RA/Dec + cor on the outer, sep/PA on the inner, RV_ABS with a basis column, RV_REL on the outer: 7 rows each,
    W = 600 random walkers (either planet may be the inner one), every nuisance non-trivial. The oracle's matrices are computed once."""
    import predict_reference as ref
    tabs, planets, elems, nuis, _ = ref.two_planet_system(seed=11, W=600)
    tabs = [head(t) for t in tabs]
    return dict(tabs=tabs, planets=planets, elems=elems, nuis=nuis,
                ref_nu=reference_matrix(oracle, tabs, planets, elems, nuis),
                ref_130_none=reference_matrix(oracle, tabs, planets, elems[:, :130], None))


def test_values_two_planets(pkg, oracle, two_planets):
    s = two_planets
    W = 130      # two waves and a partial one
    el, nu = np.ascontiguousarray(s["elems"][:, :W]), np.ascontiguousarray(s["nuis"][:, :W])
    pw = pkg.Pointwise(s["tabs"], s["planets"])
    try:
        assert pw.n_rows == 4 * NROWS and np.array_equal(pw.row_table, np.repeat(np.arange(4), NROWS))
        got_nu = device_matrix(pkg, pw, el, nu)
        got_none = device_matrix(pkg, pw, el, None)
    finally:
        pw.close()
    check_values("two planets, nuisances", got_nu, s["ref_nu"][:, :W])
    check_values("two planets, nuis = None", got_none, s["ref_130_none"])
    assert np.any((el[0] < el[9])) and np.any((el[0] > el[9]))      # both orders of the two planets are among the walkers
    # closure: the rows of a table summed are the oracle's value of the whole table
    for nuis_, got in ((nu, got_nu), (None, got_none)):
        whole = table_values(oracle, s["tabs"], s["planets"], el, nuis_)
        sums = got.reshape(4, NROWS, W).sum(axis=1)
        err = np.abs(sums - whole) / np.maximum(1.0, np.abs(whole))
        print(f"closure ({'nuisances' if nuis_ is not None else 'None'}): max err = {err.max():.3e}")
        assert err.max() <= 1e-11, err.max()


def test_values_seppa_with_cor(pkg, oracle):
    """With a correlation the density is not even in the PA residual, so the wrap point of the residual must stay out of reach: data from a
    truth orbit, walkers near it, and the oracle-side PA of every walker within 1 rad of its datum (asserted)."""
    capi = pkg.capi
    rng = np.random.default_rng(3)
    planets = [dict(orbit_kind=V, has_mass=0)]
    truth = np.array([7.0, 0.25, 0.9, 0.6, 2.4, 58200.0, 1.1, 40.0, 0.0])
    W = 130
    elems = truth[:, None] * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, (9, W)))
    elems[5] = truth[5] + rng.uniform(-30.0, 30.0, W)      # tp within a month, not within 2 % of its MJD
    elems[8] = 0.0
    epoch = np.sort(rng.uniform(57000.0, 60000.0, NROWS))
    ra = np.array([oracle.oracle_orbitsolve(truth, t)["raoff"] for t in epoch])
    dec = np.array([oracle.oracle_orbitsolve(truth, t)["decoff"] for t in epoch])
    s_pa, s_sep = rng.uniform(0.01, 0.03, NROWS), rng.uniform(1.0, 3.0, NROWS)
    tab = dict(kind=capi.ASTROM_SEPPA, planet=0, epoch=epoch, y1=np.arctan2(ra, dec) + s_pa * rng.standard_normal(NROWS),
               y2=np.hypot(ra, dec) + s_sep * rng.standard_normal(NROWS), s1=s_pa, s2=s_sep, cor=rng.uniform(-0.6, 0.6, NROWS), extra=None)
    nuis = np.stack([rng.uniform(0.001, 0.01, W), rng.uniform(0.99, 1.01, W), rng.uniform(-0.01, 0.01, W)])
    for w in range(W):
        for j, t in enumerate(epoch):
            o = oracle.oracle_orbitsolve(np.ascontiguousarray(elems[:, w]), t)
            d = tab["y1"][j] + nuis[2, w] - np.arctan2(o["raoff"], o["decoff"])
            assert abs(np.pi - np.mod(np.pi - d, 2.0 * np.pi)) < 1.0
    pw = pkg.Pointwise([tab], planets)
    try:
        got = device_matrix(pkg, pw, elems, nuis)
        got0 = device_matrix(pkg, pw, elems, None)
    finally:
        pw.close()
    check_values("sep/PA with cor, nuisances", got, reference_matrix(oracle, [tab], planets, elems, nuis))
    check_values("sep/PA with cor, nuis = None", got0, reference_matrix(oracle, [tab], planets, elems, None))


@pytest.mark.parametrize("orbit,kind", [(V, "ASTROM_RADEC"), (RVO, "RV_ABS"), (TI, "ASTROM_SEPPA"), (KEP, "RV_REL")], ids=["visual", "radvel", "ti", "kep"])
def test_values_each_orbit_kind(pkg, oracle, orbit, kind):
    import predict_reference as ref
    capi = pkg.capi
    kind = getattr(capi, kind)
    planets = [dict(orbit_kind=orbit, has_mass=1)]
    W = 20
    elems = ref.random_elements(planets, W, seed=40 + orbit, e_max=0.95)
    tabs = [random_table(capi, kind, -1 if kind == capi.RV_ABS else 0, seed=60 + orbit, cor=True, basis=True)]
    nuis = random_nuis(tabs, W, seed=70 + orbit)
    pw = pkg.Pointwise(tabs, planets)
    try:
        got = device_matrix(pkg, pw, elems, nuis)
    finally:
        pw.close()
    check_values(f"orbit kind {orbit}", got, reference_matrix(oracle, tabs, planets, elems, nuis))


def test_values_five_planets(pkg, oracle):
    """The run-time route (5 … OCTO_MAX_PLANETS planets): RA/Dec on planet 3 plus an absolute RV table; a wave and a partial one."""
    tabs, planets, elems, nuis = five_planets(pkg, 70)
    pw = pkg.Pointwise(tabs, planets)
    try:
        got = device_matrix(pkg, pw, elems, nuis)
        s = pw.summary(elems, nuis)
    finally:
        pw.close()
    refm = reference_matrix(oracle, tabs, planets, elems, nuis)
    check_values("five planets", got, refm)
    whole = table_values(oracle, tabs, planets, elems, nuis)
    err = np.abs(got.reshape(2, NROWS, -1).sum(axis=1) - whole) / np.maximum(1.0, np.abs(whole))
    assert err.max() <= 1e-11, err.max()
    check_summary("five planets", s, refm)


def test_summary_against_the_oracle_matrix(pkg, oracle, two_planets):
    """W = 600: three blocks, the last partial."""
    s = two_planets
    pw = pkg.Pointwise(s["tabs"], s["planets"])
    try:
        a = pw.summary(s["elems"], s["nuis"])
        b = pw.summary(s["elems"], s["nuis"])
    finally:
        pw.close()
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k      # the summary twice: bitwise
    assert np.all(a["n"] == 600)
    check_summary("two planets, W = 600", a, s["ref_nu"])


def test_invariance_bitwise(pkg, two_planets):
    import torch
    s = two_planets
    W = 130
    el, nu = np.ascontiguousarray(s["elems"][:, :W]), np.ascontiguousarray(s["nuis"][:, :W])
    pw = pkg.Pointwise(s["tabs"], s["planets"])
    try:
        full = pw.values(el, nu)
        # a walker alone, and in a shuffled batch
        for w in (0, 64, 129):
            alone = pw.values(el[:, w:w + 1], nu[:, w:w + 1])
            assert np.array_equal(bits(alone[:, 0]), bits(full[:, w])), w
        perm = np.random.default_rng(0).permutation(W)
        shuf = pw.values(np.ascontiguousarray(el[:, perm]), np.ascontiguousarray(nu[:, perm]))
        assert np.array_equal(bits(shuf), bits(full[:, perm]))
        # the device-buffer call against the host-buffer call
        dev = pw.values(torch.from_numpy(el).cuda(), torch.from_numpy(nu).cuda())
        torch.cuda.synchronize()
        assert np.array_equal(bits(dev.cpu().numpy()), bits(full))
        sd = pw.summary(torch.from_numpy(el).cuda(), torch.from_numpy(nu).cuda())
        sh = pw.summary(el, nu)
        torch.cuda.synchronize()
        for k in sh:
            assert np.array_equal(bits(sd[k].cpu().numpy()), bits(sh[k])), k
    finally:
        pw.close()
    # the host-buffer call with both buffers shrunk: 40 walkers per chunk (four chunks), two rows per staging pass
    old = {k: os.environ.get(k) for k in ("OCTO_POINTWISE_MATRIX_BYTES", "OCTO_POINTWISE_STAGE_BYTES")}
    os.environ["OCTO_POINTWISE_MATRIX_BYTES"] = str(4 * NROWS * 8 * 40)
    os.environ["OCTO_POINTWISE_STAGE_BYTES"] = str(8 * 100)
    try:
        small = pkg.Pointwise(s["tabs"], s["planets"])
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        chunked = small.values(el, nu)
    finally:
        small.close()
    assert np.array_equal(bits(chunked), bits(full))


def test_edges(pkg, two_planets):
    s = two_planets
    W = 130
    el, nu = np.ascontiguousarray(s["elems"][:, :W]), np.ascontiguousarray(s["nuis"][:, :W])
    el[1, 7] = 1.2             # e = 1.2: the likelihood scores the walker −Inf
    nu[[0, 3, 7, 10], 90] = np.nan      # a NaN jitter in every table
    pw = pkg.Pointwise(s["tabs"], s["planets"])
    try:
        m = pw.values(el, nu)
        sm = pw.summary(el, nu)
        assert np.all(np.isneginf(m[:, 7])) and np.all(np.isnan(m[:, 90]))
        keep = np.ones(W, dtype=bool); keep[[7, 90]] = False
        assert np.isfinite(m[:, keep]).all()
        assert np.array_equal(bits(m[:, keep]), bits(pw.values(np.ascontiguousarray(el[:, keep]), np.ascontiguousarray(nu[:, keep]))))
        assert np.all(sm["n"] == W - 2)
        assert np.array_equal(sm["min"], m[:, keep].min(axis=1)) and np.array_equal(sm["max"], m[:, keep].max(axis=1))
        # W = 1: a variance of one value is NaN; the other statistics are the value
        one = pw.summary(el[:, :1], nu[:, :1])
        assert np.all(one["n"] == 1) and np.all(np.isnan(one["var"]))
        for k in ("lppd", "mean", "elpd_is_loo", "min", "max"):
            assert np.array_equal(bits(one[k]), bits(m[:, 0])), k
        # no valid walker at all: n = 0 and NaN in the rest
        none = pw.summary(el[:, 7:8], nu[:, 7:8])
        assert np.all(none["n"] == 0) and all(np.all(np.isnan(none[k])) for k in ("lppd", "mean", "var", "elpd_is_loo", "min", "max"))
    finally:
        pw.close()
    # a table of 0 rows beside a table of 3
    empty = head(s["tabs"][2], 0)
    three = head(s["tabs"][0], 3)
    pw = pkg.Pointwise([empty, three], s["planets"])
    try:
        assert pw.n_rows == 3 and np.array_equal(pw.row_table, [1, 1, 1])
        nu2 = np.ascontiguousarray(np.concatenate([nu[6:9], nu[0:3]]))
        got = pw.values(el, nu2)
        assert got.shape == (3, W) and np.array_equal(bits(got), bits(m[:3]))
    finally:
        pw.close()
    pw = pkg.Pointwise([empty], s["planets"])
    try:
        assert pw.n_rows == 0 and pw.values(el, nu[6:9]).shape == (0, W)
    finally:
        pw.close()


def test_callers(pkg, oracle):
    import synth
    capi = pkg.capi
    rng = np.random.default_rng(17)
    t = 50000.0 + 90.0 * np.arange(6)
    ra, dec = synth.truth_radec(t)
    table = dict(epoch=t, ra=ra + rng.normal(0, 60.0, 6), dec=dec + rng.normal(0, 60.0, 6), σ_ra=np.full(6, 60.0), σ_dec=np.full(6, 60.0))
    rvt = dict(epoch=t[:5] + 7.0, rv=rng.normal(0, 30, 5), σ_rv=np.full(5, 8.0))

    def build(rv_obs):
        astrom = pkg.PlanetRelAstromObs(table, name="sim", variables=pkg.variables(jitter=pkg.LogUniform(0.1, 30.0)))
        b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom],
                       variables=pkg.variables(a=pkg.LogUniform(5, 20), e=pkg.Uniform(0.0, 0.6), i=pkg.Sine(), ω=pkg.UniformCircular(),
                                               Ω=pkg.UniformCircular(), θ=pkg.UniformCircular(), tp=pkg.θ_at_epoch_to_tperi("θ", 50000),
                                               mass=pkg.LogUniform(1.0, 50.0)))
        return pkg.LogDensityModel(pkg.System(name="sim", companions=[b], observations=[rv_obs],
                                              variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.05), lower=0.1),
                                                                      plx=pkg.truncated(pkg.Normal(50.0, 0.1), lower=0.1))))

    model = build(pkg.StarAbsoluteRVObs(rvt, name="rv", variables=pkg.variables(offset=pkg.Normal(0, 20), jitter=pkg.LogUniform(0.1, 20.0))))
    try:
        draws = model.sample_priors(rng, 200)
        fn = model.ln_like
        LL, labels = pkg.pointwise_like_rows(model, draws)
        assert LL.shape == (200, 11) and labels == [("sim", j) for j in range(6)] + [("rv", j) for j in range(5)]
        elems, nuis = model.kernel_inputs(draws)
        refm = reference_matrix(oracle, fn.obs_tables, fn.planet_desc, elems, nuis)
        check_values("pointwise_like_rows", np.ascontiguousarray(LL.T), refm)
        w = pkg.waic(model, draws)
        assert w["n_samples"] == 200 and w["labels"] == labels and np.all(w["n_valid"] == 200)
        assert np.array_equal(w["elpd_waic"], w["lppd"] - w["p_waic"])
        for k in ("lppd", "p_waic", "elpd_waic", "elpd_is_loo"):
            assert w[k].shape == (11,) and w[k + "_total"] == float(np.sum(w[k]))
            assert w[k + "_se"] == float(np.sqrt(11 * np.var(w[k], ddof=1)))
        check_summary("waic", dict(n=w["n_valid"], lppd=w["lppd"], var=w["p_waic"], elpd_is_loo=w["elpd_is_loo"]), refm,
                      keys=("lppd", "elpd_is_loo", "var"))
    finally:
        model.close()
    marg = build(pkg.MarginalizedStarAbsoluteRVObs(rvt, name="rv", variables=pkg.variables(jitter=pkg.LogUniform(0.1, 20.0))))
    try:
        draws = marg.sample_priors(rng, 8)
        for call in (pkg.pointwise_like_rows, pkg.waic):
            with pytest.raises(capi.OctoError) as ex:
                call(marg, draws)
            assert ex.value.status == capi.OCTO_ENOTSUP
    finally:
        marg.close()
