"""
PSIS-LOO on the device (include/octofitter_hip_psis.h, host/psis.py, callers.loo) — GPU suite.

The device and the reference get the SAME matrix bits, so only the PSIS arithmetic is under test. The reference is the 40-digit restatement
of the algorithm (psis_reference.psis_row_mp), never the device's own output; the one row that reaches the log(DBL_MIN) cut-off is compared
with the float64 restatement. Bars:
  elpd_loo, lppd, log-weights   1e-11 · max(1, |ref|): the project's pointwise bar;
  n, tail_len                   exact; ±Inf, NaN and the −Inf weights of excluded entries exact;
  k̂ (absolute), ess (relative)  100 × the float64 restatement's own largest gap to the 40-digit reference over the cases of the generator
                                (computed here and printed; 7.4e-12 and 6.0e-13): the margin covers another summation order and the
                                device's exp / log / log1p;
  invariance                    bitwise.
The edge rows (psis_reference.EDGE_ROWS: a gather at every pass of the select and never, tails of 8 … 4096 = MAX_TAIL with m = 94 = MAX_GRID,
tie blocks, sparse rows, offsets; above S = 120 001 against psis_row_hybrid) keep these bars. Only the rows built to gather late have their
tail within 1e-2 … 1e-8 of the cut-off, where y = exp(x) − exp(x_c) cancels: there a field's bar is max(the bar above, 100 × the restatement's
gap on that row), k̂'s capped at 1e-5, and tests/test_psis_reference.py shows on the reference alone that a tail wrong by one entry moves k̂
by at least ten such bars.
The observed maxima are printed (tools/psis_bench.py writes them to profiles/psis_throughput.txt).
"""
import ctypes as C
import os
import types

import numpy as np
import pytest

import psis_reference as pr

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in pr.FIELDS + ("lw",))


def as_result(out, lw):
    res = {k: out[i].copy() for i, k in enumerate(pr.FIELDS)}
    res["lw"] = lw
    return res


def device_loo(pkg, ps, LL, pad=5, pad_w=3, weights=True):
    """The device call through the C ABI with ld = S + pad and ld_w = S + pad_w. The matrix's padding holds a FINITE value (read, it would
    count: n is exact), the weights' padding a sentinel that must survive. weights=False is the statistics-only call (d_lw = NULL): the
    weights returned are then the untouched sentinel."""
    import torch
    R, S = LL.shape
    buf = np.full((R, S + pad), 50.0)
    buf[:, :S] = LL
    d_ll = torch.from_numpy(buf).cuda()
    d_out = torch.full((ps_n_stats(pkg), R), 777.0, dtype=torch.float64, device="cuda")
    d_lw = torch.full((R, S + pad_w), 123.0, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    st = ps.lib.octo_psis_loo_device(ps._h, d_ll.data_ptr(), S + pad, R, S, d_out.data_ptr(), d_lw.data_ptr() if weights else None, S + pad_w if weights else 0, stream)
    assert st == pkg.capi.OCTO_OK, (st, ps.lib.octo_psis_last_error(ps._h))
    torch.cuda.synchronize()
    lw = d_lw.cpu().numpy()
    assert weights or np.all(lw == 123.0)
    assert np.all(lw[:, S:] == 123.0)                                  # nothing written past S
    assert np.array_equal(bits(d_ll.cpu().numpy()), bits(buf))        # the input is untouched
    return as_result(d_out.cpu().numpy(), np.ascontiguousarray(lw[:, :S]))


def ps_n_stats(pkg):
    return pkg.psis.N_STATS


def host_loo(pkg, ps, LL, pad=5, pad_w=3):
    """The host-buffer call with ld > S and ld_w > S."""
    capi = pkg.capi
    R, S = LL.shape
    buf = np.full((R, S + pad), 50.0)
    buf[:, :S] = LL
    out = np.full((ps_n_stats(pkg), R), 777.0)
    lw = np.full((R, S + pad_w), 123.0)
    st = ps.lib.octo_psis_loo(ps._h, capi._dptr(buf), S + pad, R, S, capi._dptr(out), capi._dptr(lw), S + pad_w)
    assert st == capi.OCTO_OK, (st, ps.lib.octo_psis_last_error(ps._h))
    assert np.all(lw[:, S:] == 123.0)
    return as_result(out, np.ascontiguousarray(lw[:, :S]))


@pytest.fixture(scope="module")
def ps(pkg):
    h = pkg.Psis()
    yield h
    h.close()


@pytest.fixture(scope="module")
def bars():
    """k̂ and ess: 100 × the float64 restatement's largest gap to the 40-digit reference over every case of the generator."""
    worst = dict(pareto_k=0.0, ess=0.0)
    for name in pr.CASES:
        LL, ref = pr.case(name)
        g = pr.gaps(pr.psis_matrix(LL), ref)
        worst = {k: max(v, g[k]) for k, v in worst.items()}
    print(f"restatement's largest gap to the 40-digit reference: k̂ {worst['pareto_k']:.3e} (absolute), ess {worst['ess']:.3e} (relative); the device's bars are 100 × these")
    assert 0.0 < worst["pareto_k"] < 1e-11 and 0.0 < worst["ess"] < 1e-11      # the restatement's own bar (tests/test_psis_reference.py)
    return dict(pareto_k=100.0 * worst["pareto_k"], ess=100.0 * worst["ess"], elpd_loo=1e-11, lppd=1e-11, lw=1e-11)


def check(name, got, ref, bars):
    g = pr.gaps(got, ref)      # n, tail_len, ±Inf, NaN and the excluded entries' −Inf: exact
    print(f"{name}: k̂ {g['pareto_k']:.3e} (bar {bars['pareto_k']:.1e})  ess {g['ess']:.3e} (bar {bars['ess']:.1e})  "
          f"elpd_loo {g['elpd_loo']:.3e}  lppd {g['lppd']:.3e}  lw {g['lw']:.3e} (bar 1e-11)")
    for k, v in g.items():
        assert v <= bars[k], (name, k, v, bars[k])
    return g


@pytest.mark.parametrize("name", list(pr.CASES))
def test_against_40_digits(pkg, ps, bars, name):
    LL, ref = pr.case(name)
    check(name, device_loo(pkg, ps, LL), ref, bars)


def test_ties(pkg, ps, bars):
    """ll on a grid of 0.25: ties at the cut-off stay out of the tail (tail_len < M) and ties inside it go by sample index, so the weights must
    match the reference entry by entry; the second row is an index permutation of the first."""
    row = np.round(pr.student_rows(1000, 1, 1.0, 5.0, 31)[0] * 4.0) / 4.0
    LL = np.stack([row, row[np.random.default_rng(5).permutation(row.size)]])
    ref = pr.psis_matrix(LL, pr.psis_row_mp)
    assert np.all(ref["tail_len"] < pr.tail_len(1000)) and np.all(ref["tail_len"] > 4) and ref["tail_len"][0] == ref["tail_len"][1]
    got = device_loo(pkg, ps, LL)
    check("ties", got, ref, bars)
    # equal values inside the tail got DIFFERENT weights, in index order
    for r in range(2):
        order = pr.tail_order(LL[r])
        ties = [i for i in range(len(order) - 1) if LL[r][order[i]] == LL[r][order[i + 1]]]
        assert len(order) == ref["tail_len"][r] and ties, "the case holds no tie inside the tail"
        for i in ties:
            assert order[i] < order[i + 1] and got["lw"][r][order[i]] < got["lw"][r][order[i + 1]] and ref["lw"][r][order[i]] < ref["lw"][r][order[i + 1]]


def test_non_finite_entries(pkg, ps, bars):
    rng = np.random.default_rng(77)
    LL = pr.student_rows(300, 5, 1.0, 5.0, 77)
    LL[0, rng.choice(300, 40, replace=False)] = -np.inf
    LL[0, rng.choice(300, 10, replace=False)] = np.nan
    LL[1, ::3] = np.inf
    LL[1, 1::17] = np.nan
    LL[2, :] = np.nan                      # n = 0
    LL[2, 5] = -np.inf
    LL[3, :] = -np.inf                     # n = 1
    LL[3, 200] = -4.25
    ref = pr.psis_matrix(LL, pr.psis_row_mp)
    assert ref["n"][2] == 0 and ref["n"][3] == 1 and ref["n"][4] == 300
    got = device_loo(pkg, ps, LL)
    check("non-finite", got, ref, bars)
    assert np.all(got["lw"][~np.isfinite(LL)] == -np.inf)
    assert got["n"][2] == 0 and all(np.isnan(got[k][2]) for k in pr.FIELDS[1:])
    assert got["pareto_k"][3] == np.inf and got["tail_len"][3] == 0 and got["elpd_loo"][3] == -4.25 and got["lw"][3, 200] == 0.0
    # the same through the host-buffer call
    assert same_bits(host_loo(pkg, ps, LL), got)


def test_underflow_clamp(pkg, ps, bars):
    """A spread of 3000 in ll: fewer than M + 1 entries lie above log(DBL_MIN), so the cut-off is the clamp and the tail the 20 entries
    above it. Compared with the float64 restatement (the reference of this one row), tail_len exact."""
    rng = np.random.default_rng(123)
    row = rng.normal(-2.0, 1.0, 1000)
    low = rng.choice(1000, 20, replace=False)
    row[low] = -3000.0 + rng.uniform(0.0, 10.0, 20)
    LL = row[None, :]
    assert LL.max() - LL.min() > 2990.0
    ref = pr.psis_matrix(LL)
    assert ref["tail_len"][0] == 20 and np.isfinite(ref["pareto_k"][0])
    check("clamp", device_loo(pkg, ps, LL), ref, bars)


def test_invariance_bitwise(pkg, ps):
    import torch
    LL, _ = pr.case("S130_R70")
    a = device_loo(pkg, ps, LL)
    assert same_bits(device_loo(pkg, ps, LL), a)                                   # the same call twice
    for r in (0, 69):                                                              # a row alone against the same row inside R = 70, at either end
        one = device_loo(pkg, ps, LL[r:r + 1], pad=0, pad_w=0)
        assert all(bits(one[k])[0] == bits(a[k])[r] for k in pr.FIELDS) and np.array_equal(bits(one["lw"][0]), bits(a["lw"][r])), r
    assert same_bits(host_loo(pkg, ps, LL), a)                                     # the device call against the host-buffer call
    # the Python face: torch in, torch out; NumPy in, NumPy out
    t = ps.loo(torch.from_numpy(LL).cuda(), weights=True)
    assert all(torch.is_tensor(v) and v.is_cuda for v in t.values())
    assert same_bits({**{k: t[k].cpu().numpy() for k in pr.FIELDS}, "lw": t["log_weights"].cpu().numpy()}, a)
    h = ps.loo(LL, weights=True)
    assert same_bits({**{k: h[k] for k in pr.FIELDS}, "lw": h["log_weights"]}, a) and "log_weights" not in ps.loo(LL)
    # the host-buffer call in three chunks of rows (a device buffer of 30 rows), through a staging buffer of 3 rows, then of half a row
    big = pr.case("S4103_c0.3_nu30")[0]
    b = device_loo(pkg, ps, big)
    keep = {k: os.environ.get(k) for k in ("OCTO_PSIS_MATRIX_BYTES", "OCTO_PSIS_STAGE_BYTES")}
    try:
        for stage in (3 * 130 * 8 + 16, 65 * 8):
            os.environ["OCTO_PSIS_MATRIX_BYTES"], os.environ["OCTO_PSIS_STAGE_BYTES"] = str(30 * 130 * 8), str(stage)
            small = pkg.Psis()
            try:
                assert same_bits(host_loo(pkg, small, LL), a), stage
                assert same_bits(host_loo(pkg, small, LL, pad=0, pad_w=0), a), stage
                # a row larger than the device buffer: OCTO_ENOMEM with a message, nothing computed
                out = np.zeros((6, 1))
                st = small.lib.octo_psis_loo(small._h, pkg.capi._dptr(big), 4103, 1, 4103, pkg.capi._dptr(out), None, 0)
                assert st == pkg.capi.OCTO_ENOMEM and b"OCTO_PSIS_MATRIX_BYTES" in small.lib.octo_psis_last_error(small._h)
            finally:
                small.close()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert same_bits(host_loo(pkg, ps, big), b)


@pytest.mark.parametrize("name", list(pr.EDGE_ROWS))
def test_edge_rows_against_the_reference(pkg, ps, bars, name):
    """The routes no case of the generator takes (psis_reference.EDGE_ROWS): tails of 8 … 4096 with and without sort padding, a gather at
    every pass 0 … 7 and never, constant rows, tie blocks, few finite entries in a long row, values far from 0. What edge_case asserts on the
    CPU (gather_pass among it) is the evidence that the row takes its route; the bars are the cases' — for the rows whose fit is
    ill-conditioned by construction the per-row rule of psis_reference.edge_bars — and never the device's output."""
    LL, ref, gather = pr.edge_case(name)
    row_bars, gap = pr.edge_bars(name, bars)
    print(f"{name}: S {LL.shape[1]}  n {ref['n'][0]:.0f}  gather_pass {gather}  tail_len {ref['tail_len'][0]:.0f}  k̂ {ref['pareto_k'][0]:.4f}  "
          f"restatement's k̂ gap {gap['pareto_k']:.2e}")
    got = device_loo(pkg, ps, LL)
    check(name, got, ref, row_bars)
    if name.startswith("const"):
        assert got["pareto_k"][0] == np.inf and got["tail_len"][0] == 0
    if name.startswith("dup10"):
        # what test_ties asserts: equal values inside the tail got DIFFERENT weights, in index order — except where the smoothed value is
        # capped at x = 0 (k̂ = 0.08: the top 3 of the 420 quantiles lie above the largest ratio), which both sides must cap alike
        order = pr.tail_order(LL[0])
        ties = [i for i in range(len(order) - 1) if LL[0][order[i]] == LL[0][order[i + 1]]]
        assert len(order) == ref["tail_len"][0] < pr.tail_len(LL.shape[1]) and len(ties) == 9 * len(order) // 10
        g, f = got["lw"][0][order], ref["lw"][0][order]
        capped = f == ref["lw"].max()
        assert np.array_equal(capped, g == got["lw"].max()) and 0 < capped.sum() <= 3 and np.all(capped[-capped.sum():])
        for i in ties:
            assert order[i] < order[i + 1] and ((g[i] < g[i + 1] and f[i] < f[i + 1]) or (capped[i] and capped[i + 1])), i


@pytest.mark.parametrize("name", ["S130_R70", "never_tieblock", pr.LIMIT_ROW])
def test_statistics_only_call_is_bit_identical(pkg, ps, name):
    """d_lw = NULL changes what is stored, not what is computed: the six statistics keep their bits."""
    LL = pr.case(name)[0] if name in pr.CASES else pr.edge_case(name)[0]
    a, b = device_loo(pkg, ps, LL), device_loo(pkg, ps, LL, weights=False)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in pr.FIELDS), name


def test_limit_row_through_the_host_buffer_call(pkg, ps):
    """S = octo_psis_max_samples() through octo_psis_loo: one row of 15 MB in the default 64 MiB device buffer, then through a staging buffer
    of 1 MB — fifteen pieces, the last a short one — with the device call's bits both times."""
    LL = pr.edge_case(pr.LIMIT_ROW)[0]
    S = LL.shape[1]
    assert S == ps.lib.octo_psis_max_samples() and (S * 8) % 1_000_000 != 0
    a = device_loo(pkg, ps, LL)
    assert same_bits(host_loo(pkg, ps, LL), a)
    keep = os.environ.get("OCTO_PSIS_STAGE_BYTES")
    os.environ["OCTO_PSIS_STAGE_BYTES"] = "1000000"
    try:
        small = pkg.Psis()
        try:
            assert same_bits(host_loo(pkg, small, LL), a)
        finally:
            small.close()
    finally:
        if keep is None:
            os.environ.pop("OCTO_PSIS_STAGE_BYTES", None)
        else:
            os.environ["OCTO_PSIS_STAGE_BYTES"] = keep


def test_late_gather_row_keeps_its_bits_in_a_matrix(pkg, ps):
    """gather6 (the select gathers at pass 6) as row 0 and as row 69 of 70 rows of S = 20 000 whose other rows gather at pass 2, and alone."""
    row = pr.edge_case("gather6")[0][0]
    LL = pr.student_rows(20000, 70, 0.3, 30.0, 70)
    LL[0], LL[69] = row, row
    assert pr.gather_pass(LL[0]) == pr.gather_pass(LL[69]) == 6 and pr.gather_pass(LL[1]) == pr.gather_pass(LL[68]) == 2
    a = device_loo(pkg, ps, LL)
    one = device_loo(pkg, ps, row[None, :], pad=0, pad_w=0)
    for r in (0, 69):
        assert all(bits(one[k])[0] == bits(a[k])[r] for k in pr.FIELDS) and np.array_equal(bits(one["lw"][0]), bits(a["lw"][r])), r


class TableModel:
    """What loo() / pointwise_like_rows() read of a LogDensityModel, over given tables: θ = the element rows, then the nuisance rows."""

    def __init__(self, tabs, planets, n_el):
        self.D = n_el + 3 * len(tabs)
        self.n_el = n_el
        self.ln_like = types.SimpleNamespace(obs_tables=tabs, planet_desc=planets, device_index=0,
                                             obs_entries=[(None, t["planet"], None, f"table{i}") for i, t in enumerate(tabs)])

    def kernel_inputs(self, θ):
        return np.ascontiguousarray(θ[:self.n_el]), np.ascontiguousarray(θ[self.n_el:])


def test_loo_end_to_end(pkg, bars):
    """loo(model, θ) on the two-planet system of tests/pointwise_reference.py (four tables of 7 rows, W = 130 walkers near the truth) against the
    40-digit reference applied to pointwise_like_rows(model, θ)."""
    import predict_reference as ref_sys
    from pointwise_reference import head
    tabs, planets, elems, nuis, _ = ref_sys.two_planet_system(seed=11, W=130, spread=0.01)
    tabs = [head(t) for t in tabs]
    model = TableModel(tabs, planets, elems.shape[0])
    θ = np.vstack([elems, nuis])
    LL, labels = pkg.pointwise_like_rows(model, θ)
    assert LL.shape == (130, 28)
    ref = pr.psis_matrix(np.ascontiguousarray(LL.T), pr.psis_row_mp)
    out = pkg.loo(model, θ, weights=True)
    got = dict(n=out["n_valid"], tail_len=out["tail_len"], pareto_k=out["pareto_k"], elpd_loo=out["elpd_loo"], lppd=out["lppd"], ess=out["ess"],
               lw=out["log_weights"])
    check("loo()", got, ref, bars)
    assert out["labels"] == labels and out["n_samples"] == 130 and out["log_weights"].shape == (28, 130)
    assert np.array_equal(out["p_loo"], out["lppd"] - out["elpd_loo"])
    for k in ("elpd_loo", "p_loo"):
        assert out[k + "_total"] == float(np.sum(out[k])) and out[k + "_se"] == float(np.sqrt(28 * np.var(out[k], ddof=1)))
    assert out["n_bad_k"] == int(np.count_nonzero(out["pareto_k"] > 0.7)) == int(np.count_nonzero(ref["pareto_k"] > 0.7))
    assert "log_weights" not in pkg.loo(model, θ)


def test_loo_refuses_a_marginalised_rv_table(pkg):
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

    # a model of the package's own: the caller's path from θ to the dict
    model = build(pkg.StarAbsoluteRVObs(rvt, name="rv", variables=pkg.variables(offset=pkg.Normal(0, 20), jitter=pkg.LogUniform(0.1, 20.0))))
    try:
        draws = model.sample_priors(rng, 200)
        out = pkg.loo(model, draws)
        LL, labels = pkg.pointwise_like_rows(model, draws)
        assert out["labels"] == labels and out["elpd_loo"].shape == (11,) and np.array_equal(out["n_valid"], np.isfinite(LL).sum(axis=0))
    finally:
        model.close()
    marg = build(pkg.MarginalizedStarAbsoluteRVObs(rvt, name="rv", variables=pkg.variables(jitter=pkg.LogUniform(0.1, 20.0))))
    try:
        with pytest.raises(capi.OctoError) as ex:
            pkg.loo(marg, marg.sample_priors(rng, 8))
        assert ex.value.status == capi.OCTO_ENOTSUP
    finally:
        marg.close()
