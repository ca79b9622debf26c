"""
OCTO_OPT_BATCH_INVARIANT (include/octofitter_hip.h) on every kernel path the planner can choose: with the option set, a walker's ll and gradient
are the same bits in whatever batch it is evaluated — the full batch, a shard, a permutation, one θ alone, 64 and 65 walkers, a strided sub-view
(pointer offset, leading dimension = the full batch), forward-only — for one to eight planets, every observation kind, per-walker nuisances,
the model callback (octo_model_logpost), octo_eval_multi and OFTI (octo_ofti_eval). The invariant results are held to the oracle on a
subsample, and the default mode (option 0) to the invariant results at rounding (test_tile_sort._close's bars).

WHY THE TABLES ARE LONG (do not shorten them): every case has >= 3000 rows on a daily-ish cadence. Below ~150 rows per table get_tasks makes ONE
task per table whatever the batch size, so every partition — the batch-size-driven one (plan_key / plan_key_mainp) and the fixed one of the
invariant mode — is the same and a partition that follows W goes unnoticed. At these lengths W = 1 and W ~ 2000 get different row partitions
(beyond four planets ~32 rows per task against hundreds), get_tasks cuts several tasks per table, and in default mode the warm-started loop and
the tile sort are active (one and two planets).
"""
import ctypes as C

import numpy as np
import pytest

import stress_parity as sp
import synth
from conftest import rel_err
from test_gpu_parity import _cmp_oracle, _gpu

pytestmark = pytest.mark.gpu

HGCA_ROWS = np.array([(48348.0, 0, 0), (48414.0, 1, 0), (48200.0, 0, 0), (57408.0, 0, 1), (57470.0, 1, 1), (57600.0, 1, 1)])
HGCA_VALS = np.array([4.71, -1.86, 0.61, 0.49, 0.21, 4.352, -2.013, 0.031, 0.024, -0.12, 4.61, -1.72, 0.052, 0.041, 0.33])


# ------------------------------------------------------------------------------------------------ tables and walkers
def _days(rng, n, t0=50000.0):
    return t0 + np.arange(n, dtype=np.float64) + rng.uniform(0.0, 0.25, n)


def _astrom(rng, kind, planet, t, cor=False):
    """kind 0 / 5: RA/Dec (O'Neil wrapper: 5); kind 1 / 6: sep/PA (O'Neil wrapper: 6)."""
    n = len(t)
    ra, dec = rng.normal(0, 300, n), rng.normal(0, 300, n)
    if kind in (1, 6):
        return dict(kind=kind, planet=planet, epoch=t, y1=np.arctan2(ra, dec), y2=np.hypot(ra, dec), s1=np.full(n, 0.03), s2=rng.uniform(3, 12, n), cor=None)
    return dict(kind=kind, planet=planet, epoch=t, y1=ra, y2=dec, s1=rng.uniform(3, 12, n), s2=rng.uniform(3, 12, n),
                cor=rng.uniform(-0.6, 0.6, n) if cor else None)


def _rv(rng, kind, t, planet=-1, trend=False):
    """kind 2: absolute RV, 3: marginalised absolute RV, 4: relative RV of `planet`."""
    n = len(t)
    amp, sig = (500.0, (20, 80)) if kind == 4 else (30.0, (1, 8))
    d = dict(kind=kind, planet=planet, epoch=t, y1=rng.normal(0, amp, n), y2=None, s1=rng.uniform(*sig, n), s2=None, cor=None)
    if trend:
        d["extra"] = (t - t.mean()) / 1000.0
    return d


def _hgca():
    return dict(kind=7, planet=-1, epoch=HGCA_ROWS[:, 0], y1=HGCA_ROWS[:, 1], y2=HGCA_ROWS[:, 2], s1=None, s2=None, cor=None, extra=HGCA_VALS)


def _nuis(rng, obs, W):
    nz = np.zeros((3 * len(obs), W))
    for o, ob in enumerate(obs):
        k = ob["kind"]
        if k in (0, 1, 5, 6):      # jitter, plate scale, north angle
            nz[3 * o] = rng.uniform(0, 4, W); nz[3 * o + 1] = rng.normal(1, 0.01, W); nz[3 * o + 2] = rng.normal(0, 0.02, W)
        elif k in (2, 3, 4):       # offset, jitter [, trend]
            nz[3 * o] = rng.normal(0, 10, W); nz[3 * o + 1] = np.exp(rng.uniform(np.log(0.1), np.log(10), W))
            if ob.get("extra") is not None:
                nz[3 * o + 2] = rng.normal(0, 2, W)
        else:                      # HGCA: pmra, pmdec
            nz[3 * o] = rng.normal(4.3, 0.3, W); nz[3 * o + 1] = rng.normal(-2.0, 0.3, W)
    return nz


def _walkers(rng, W, ranges):
    if len(ranges) == 1:
        return synth.draw_walkers(rng, W, *ranges[0], with_mass=True)
    el = np.concatenate([sp.planet_elems(rng, W, 0, lo, hi) for lo, hi in ranges])
    for p in range(1, len(ranges)):
        el[p * 9 + 6] = el[6]; el[p * 9 + 7] = el[7]      # one system mass, one parallax
    return el


def _spoil(el, W):
    """Invalid walkers — e > 1, a NaN element, a < 0 (one of them in the ragged last tile) — and, with several planets, a few walkers whose
    planets are out of order. Returns the indices that must come back -Inf."""
    P = el.shape[0] // 9
    bad = np.array([3, W // 2 + 1, W - 5])
    el[1, bad[0]] = 1.3
    el[9 * (P - 1) + 5, bad[1]] = np.nan
    el[9 * (P - 1) + 0, bad[2]] = -1.0
    if P > 1:
        el[0, 40:52] = el[9, 40:52] * 1.7
    return bad


def _case(name):
    """(obs, planets, elems, nuis, invalid walkers, ll bar against the oracle) of one row of the matrix; >= 3000 rows each (module docstring)."""
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)
    pl = lambda n: [dict(orbit_kind=0, has_mass=True) for _ in range(n)]
    ll_rtol = 1e-10
    nuis = True
    if name == "p1_kinds":      # k_main<1> fused / wide prologue, nuisance gradients
        W, P = 2011, 1
        t = _days(rng, 1600)
        obs = [_astrom(rng, 0, 0, t, cor=True), _astrom(rng, 1, 0, t[:900] + 0.5), _rv(rng, 2, _days(rng, 1200, 50100.0), trend=True)]
        el = _walkers(rng, W, [(1.0, 60.0)])
    elif name == "p1_marg_hgca":      # k_marg two-pass gradient route, k_hgca -> extra
        W, P = 2011, 1
        obs = [_rv(rng, 3, _days(rng, 3200), trend=True), _hgca()]
        el = _walkers(rng, W, [(1.0, 60.0)])
        ll_rtol = 1e-9
    elif name == "p2_config4":      # k_main<2>, the last planet's unconditional warm step in default mode
        W, P = 2011, 2
        t = _days(rng, 1500)
        obs = [_astrom(rng, 0, 1, t), _astrom(rng, 0, 0, t[:500] + 0.3), _rv(rng, 2, _days(rng, 1300, 50050.0))]
        el = _walkers(rng, W, [(1.0, 5.0), (6.0, 30.0)])
    elif name == "p3_radec_rv":      # k_main<3>, a kind set whose last planet starts warm
        W, P = 2011, 3
        obs = [_astrom(rng, 0, 2, _days(rng, 1800)), _rv(rng, 2, _days(rng, 1400, 50020.0))]
        el = _walkers(rng, W, [(1.0, 5.0), (6.0, 12.0), (15.0, 40.0)])
    elif name == "p3_marg_oneil":      # k_main<3> with KM_MARG / KM_ONEIL
        W, P = 2011, 3
        obs = [_rv(rng, 3, _days(rng, 2000), trend=True), _astrom(rng, 5, 1, _days(rng, 1200, 50010.0), cor=True)]
        el = _walkers(rng, W, [(1.0, 5.0), (6.0, 12.0), (15.0, 40.0)])
        ll_rtol = 1e-9
    elif name == "p4_kinds":      # k_mainp<4> -> k_finish<4> (MAINP in launch_all)
        W, P = 2011, 4
        t = _days(rng, 1500)
        obs = [_astrom(rng, 0, 3, t), _astrom(rng, 1, 1, t[:900] + 0.4), _rv(rng, 4, _days(rng, 900, 50030.0), planet=2)]
        el = _walkers(rng, W, [(1.5 + 4 * i, 4.5 + 4 * i) for i in range(4)])
        nuis = False
    elif name in ("p5_kinds", "p5_kinds_no_nuis"):      # dispatch_many (k_mainp -> k_finishp)
        W, P = 1733, 5
        t = _days(rng, 900)
        obs = [_astrom(rng, 0, 4, t, cor=True), _astrom(rng, 1, 1, t[:700] + 0.5), _astrom(rng, 0, 0, t[:400] + 0.2),
               _rv(rng, 2, _days(rng, 1000, 50040.0), trend=True), _rv(rng, 4, _days(rng, 600, 50060.0), planet=3)]
        el = _walkers(rng, W, [(1.5 + 4 * i, 4.5 + 4 * i) for i in range(5)])
        nuis = name == "p5_kinds"
    elif name == "p6_marg":      # dispatch_many's k_marg pre-pass over its tasks
        W, P = 1733, 6
        obs = [_rv(rng, 3, _days(rng, 2400), trend=True), _astrom(rng, 0, 5, _days(rng, 700, 50005.0)), _astrom(rng, 1, 2, _days(rng, 400, 50015.0))]
        el = _walkers(rng, W, [(0.05 + 0.4 * i, 0.3 + 0.4 * i) for i in range(6)])
        ll_rtol = 1e-9
    elif name == "p8_oneil_hgca":      # k_hgcap, k_finishp's O'Neil adjoints, a RadialVelocityOrbit planet
        W, P = 1555, 8
        obs = [_hgca(), _astrom(rng, 5, 7, _days(rng, 1500), cor=True), _astrom(rng, 6, 1, _days(rng, 500, 50025.0)),
               _rv(rng, 2, _days(rng, 1200, 50035.0))]
        el = _walkers(rng, W, [(2.0 + 5 * i, 5.0 + 5 * i) for i in range(8)])
        ll_rtol = 1e-9
    else:
        raise KeyError(name)
    planets = pl(P)
    if name == "p8_oneil_hgca":
        planets[2] = dict(orbit_kind=1, has_mass=True)
    assert sum(len(o["epoch"]) for o in obs if o["kind"] != 7) >= 3000
    bad = _spoil(el, W)
    nz = _nuis(rng, obs, W) if nuis else None
    return obs, planets, el, nz, bad, ll_rtol


# ------------------------------------------------------------------------------------------------ the harness
def _at(a, off):
    """A pointer `off` columns into a [rows, ld] row-major buffer (NULL for None)."""
    capi = _gpu().capi
    return capi._dptr(None) if a is None else C.cast(C.c_void_p(a.ctypes.data + 8 * off), capi.c_double_p)


def _strided(g, el, nz, off, Ws):
    """octo_eval on columns [off, off + Ws) of the full buffers: pointer offsets, leading dimension = the full batch. The gradient buffers are
    the full arrays, pre-filled with NaN: nothing outside the view may be written."""
    capi = _gpu().capi
    W = el.shape[1]
    ll = np.full(Ws, np.nan)
    ge = np.full_like(el, np.nan)
    gn = None if nz is None else np.full_like(nz, np.nan)
    g._chk(g.lib.octo_eval(g.ctx, g.ds, _at(el, off), _at(nz, off), W, Ws, capi._dptr(ll), _at(ge, off), _at(gn, off)))
    out = np.ones(W, bool); out[off:off + Ws] = False
    assert np.isnan(ge[:, out]).all() and (gn is None or np.isnan(gn[:, out]).all()), "a strided call wrote outside its columns"
    return ll, ge[:, off:off + Ws], None if gn is None else gn[:, off:off + Ws]


def _shapes(W, seed):
    """(name, the full batch's columns it holds) — a shard starting off a tile boundary, a permutation, one θ, 64 and 65 walkers (one lane in a
    second tile), each away from a multiple of 64."""
    rng = np.random.default_rng(seed)
    k = int(rng.integers(64, W - 64))
    return [("shard", np.arange(5 * 64 + 37, W - 211)), ("permuted", rng.permutation(W)), ("one θ", np.array([k])),
            ("W = 64", np.arange(3 * 64 + 5, 4 * 64 + 5)), ("W = 65", np.arange(7 * 64 + 50, 8 * 64 + 51))]


STRIDED = (2 * 64 + 19, 1000)      # (first column, walkers) of the strided sub-view


def _sub(x, cols):
    return None if x is None else np.ascontiguousarray(x[:, cols])


def _evaluate(g, el, nz, shapes):
    """{name: (columns, (ll, g_elems, g_nuis))} for the full batch, every shape and the strided view; + the forward-only ll of the full batch."""
    W = el.shape[1]
    out = {"full": (np.arange(W), g.eval(el, nz, grad=True))}
    fwd = g.eval(el, nz, grad=False)[0]
    for name, cols in shapes:
        out[name] = (cols, g.eval(_sub(el, cols), _sub(nz, cols), grad=True))
    off, Ws = STRIDED
    out["strided view"] = (np.arange(off, off + Ws), _strided(g, el, nz, off, Ws))
    return out, fwd


def _diff(a, b):
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    if not bad.any():
        return "equal"
    x, y = a[bad], b[bad]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(x - y) / np.maximum(np.abs(y), 1e-300)
    return f"{int(bad.sum())} of {a.size} values differ, worst relative {np.nanmax(r):.3g}"


def _bitwise(name, r, full, cols):
    ref = (full[0][cols], full[1][:, cols], None if full[2] is None else full[2][:, cols])
    assert np.array_equal(r[0], ref[0]), (name, "ll not bit-identical to the full batch", _diff(r[0], ref[0]))
    assert np.array_equal(r[1], ref[1]), (name, "g_elems not bit-identical to the full batch", _diff(r[1], ref[1]))
    if ref[2] is not None:
        assert np.array_equal(r[2], ref[2]), (name, "g_nuis not bit-identical to the full batch", _diff(r[2], ref[2]))


def _row_scale(gr, ok):
    return None if gr is None else np.maximum(np.abs(gr[:, ok]).max(axis=1, keepdims=True), 1e-300)


def _close(name, r, full, cols, scales):
    """test_tile_sort._close's bars (ll 1e-12, gradient 1e-9 of the row's scale over the full batch)."""
    ok = np.isfinite(full[0][cols])
    assert np.array_equal(np.isfinite(r[0]), ok) and np.isneginf(r[0][~ok]).all(), (name, "validity")
    err = rel_err(r[0][ok], full[0][cols][ok], 1.0)
    assert np.all(err < 1e-12), (name, "ll", err.max(initial=0.0))
    for gi, sc in ((1, scales[0]), (2, scales[1])):
        if r[gi] is None:
            continue
        d = np.abs(r[gi][:, ok] - full[gi][:, cols][:, ok]) / sc
        assert np.all(d < 1e-9), (name, "gradient", d.max(initial=0.0))
        assert np.all(r[gi][:, ~ok] == 0.0), (name, "an invalid walker's gradient is zero")


def _oracle_cols(W, bad, seed):
    """12-24 walkers: the first and last columns, the ragged last tile, random picks, the invalid ones."""
    rng = np.random.default_rng(seed)
    tail = W - W % 64
    idx = np.concatenate([[0, 1, 63, 64, W - 2, W - 1, tail, (tail + W) // 2], rng.choice(W, 10, replace=False), bad])
    return np.unique(idx)


def _check_invariance(pkg, oracle, obs, planets, el, nz, bad, ll_rtol, tag, seed):
    gb = _gpu()
    capi = pkg.capi
    W = el.shape[1]
    shapes = _shapes(W, seed)
    res, fwd = {}, {}
    for inv in (1, 0):
        with gb.GpuPath(obs, planets, options={capi.OPT_BATCH_INVARIANT: inv}) as g:
            res[inv], fwd[inv] = _evaluate(g, el, nz, shapes)
    k = shapes[2][1]
    with gb.GpuPath(obs, planets, options={capi.OPT_BATCH_INVARIANT: 1}) as g:      # one θ on a context that has seen nothing else
        lone = g.eval(_sub(el, k), _sub(nz, k), grad=True)
    full = res[1]["full"][1]
    ll, ge, gn = full
    ok = np.isfinite(ll)
    assert np.isneginf(ll[bad]).all(), (tag, "invalid walkers must be -Inf")
    assert np.isneginf(ll[~ok]).all() and np.all(ge[:, ~ok] == 0.0) and (gn is None or np.all(gn[:, ~ok] == 0.0)), tag
    assert ok.sum() >= 0.9 * W, (tag, int(ok.sum()))
    # the invariant results against the oracle
    idx = _oracle_cols(W, bad, seed + 1)
    ll_o, g_o, gn_o = oracle.oracle_eval(obs, planets, el[:, idx], _sub(nz, idx), grad=True)
    _cmp_oracle(f"{tag}: invariant vs oracle", ll[idx], ge[:, idx], None if gn is None else gn[:, idx], ll_o, g_o, gn_o, ll_rtol=ll_rtol, g_rtol=1e-8)
    # option 1: every shape bit for bit
    assert np.array_equal(fwd[1], ll), (tag, "forward-only ll != the ll returned with the gradient", _diff(fwd[1], ll))
    for name, (cols, r) in res[1].items():
        _bitwise(f"{tag}, {name}", r, full, cols)
    _bitwise(f"{tag}, one θ on a fresh context", lone, full, k)
    # option 0: every shape to rounding of the invariant results
    scales = (_row_scale(ge, ok), _row_scale(gn, ok))
    assert np.array_equal(fwd[0], res[0]["full"][1][0]), (tag, "default mode: forward-only ll != the ll returned with the gradient")
    for name, (cols, r) in res[0].items():
        _close(f"{tag}, default mode, {name}", r, full, cols, scales)


CASES = ["p1_kinds", "p1_marg_hgca", "p2_config4", "p3_radec_rv", "p3_marg_oneil", "p4_kinds", "p5_kinds", "p5_kinds_no_nuis", "p6_marg", "p8_oneil_hgca"]


@pytest.mark.parametrize("name", CASES)
def test_batch_invariant_every_kernel_family(pkg, oracle, name):
    """One row of the matrix per planet count and kernel family (module docstring): the same walkers in every batch shape, bitwise with the
    option, to rounding without it, and against the oracle."""
    obs, planets, el, nz, bad, ll_rtol = _case(name)
    _check_invariance(pkg, oracle, obs, planets, el, nz, bad, ll_rtol, name, seed=CASES.index(name) + 11)


def test_batch_invariant_eval_multi_five_planets(pkg):
    """octo_eval_multi over three contexts on device 0, every one with the option set: the split equals the unsplit evaluation bit for bit
    (a 1-GPU against an N-GPU rerun of one chain) beyond four planets."""
    gb = _gpu()
    capi = pkg.capi
    lib = capi.load_library()
    obs, planets, el, nz, bad, _ = _case("p5_kinds")
    opts = {capi.OPT_BATCH_INVARIANT: 1}
    ref = gb.gpu_eval(obs, planets, el, nz, grad=True, options=opts)
    paths = [gb.GpuPath(obs, planets, device=0, options=opts) for _ in range(3)]
    try:
        ctxs = (C.c_void_p * 3)(*[p.ctx for p in paths]); dss = (C.c_void_p * 3)(*[p.ds for p in paths])
        el = np.ascontiguousarray(el); nz = np.ascontiguousarray(nz); W = el.shape[1]
        ll = np.full(W, np.nan); g = np.full_like(el, np.nan); gn = np.full_like(nz, np.nan)
        assert lib.octo_eval_multi(ctxs, dss, 3, capi._dptr(el), capi._dptr(nz), W, W, capi._dptr(ll), capi._dptr(g), capi._dptr(gn)) == 0
    finally:
        for p in paths:
            p.close()
    assert np.isneginf(ll[bad]).all()
    _bitwise("octo_eval_multi, 5 planets, 3 contexts", (ll, g, gn), ref, np.arange(W))


def _model(pkg, P, rng):
    """A LogDensityModel of P planets (relative astrometry on each) + an absolute-RV table with offset and jitter: >= 3000 rows in all."""
    n_ast = 3000 if P == 1 else 600
    planets = []
    for k in range(P):
        t = 50000.0 + k * 0.2 + np.arange(n_ast) + rng.uniform(0, 0.1, n_ast)
        tab = dict(epoch=t, ra=rng.normal(0, 200, n_ast), dec=rng.normal(0, 200, n_ast), σ_ra=np.full(n_ast, 30.0), σ_dec=np.full(n_ast, 30.0))
        obs = [pkg.PlanetRelAstromObs(tab, name=f"astrom{k}", variables=pkg.variables(jitter=pkg.LogUniform(0.1, 30.0)) if k == P // 2 else None)]
        lo, hi = (1.0, 60.0) if P == 1 else (1.0 + 3 * k, 3.0 + 3 * k)
        planets.append(pkg.Planet(name=f"p{k}", basis="Visual{KepOrbit}", observations=obs,
                                  variables=pkg.variables(a=pkg.LogUniform(lo, hi), e=pkg.Uniform(0.0, 0.9), i=pkg.Sine(), ω=pkg.UniformCircular(),
                                                          Ω=pkg.UniformCircular(), θ=pkg.UniformCircular(), tp=pkg.θ_at_epoch_to_tperi("θ", 50000),
                                                          mass=pkg.LogUniform(0.5, 30.0))))
    t = 50000.3 + np.arange(1000) * 1.5
    rv = pkg.StarAbsoluteRVObs(dict(epoch=t, rv=rng.normal(0, 40, 1000), σ_rv=np.full(1000, 6.0)), name="rv",
                               variables=pkg.variables(offset=pkg.Normal(0, 20), jitter=pkg.LogUniform(0.1, 20.0)))
    sys_ = pkg.System(name=f"inv{P}", companions=planets, observations=[rv],
                      variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.05), lower=0.1), plx=pkg.truncated(pkg.Normal(50.0, 0.1), lower=0.1)))
    return pkg.LogDensityModel(sys_)


@pytest.mark.parametrize("P", [1, 5])
def test_batch_invariant_model_callback(pkg, oracle, P):
    """The whole callback (octo_model_logpost: k_model_fwd -> the epoch loop -> k_finish[p] with the model's tail) with the option set: the full,
    a shard, a permuted and a one-θ_t batch give the same bits, and match the oracle's callback."""
    capi = pkg.capi
    rng = np.random.default_rng(600 + P)
    model = _model(pkg, P, rng)
    try:
        fn = model.ln_like
        assert fn.lib.octo_ctx_set_option(fn._ctx, capi.OPT_BATCH_INVARIANT, 1) == 0
        v = C.c_int64(-1)
        assert fn.lib.octo_ctx_get_option(fn._ctx, capi.OPT_BATCH_INVARIANT, C.byref(v)) == 0 and v.value == 1
        W = 1501
        th = model.link(model.sample_priors(rng, W))
        th[3, 17] = np.nan
        lp, g = model.logdensity_and_gradient(th)
        assert np.isneginf(lp[17]) and np.all(g[:, 17] == 0.0) and np.isfinite(lp).sum() >= 0.9 * W
        idx = _oracle_cols(W, np.array([17]), 700 + P)
        lp_o, g_o = oracle.oracle_model_logpost(fn.obs_tables, fn.planet_desc, model._c_priors, model._c_esrc, model._c_nsrc, th[:, idx], grad=True)
        ok = np.isfinite(lp_o)
        assert np.array_equal(np.isfinite(lp[idx]), ok)
        assert np.all(np.abs(lp[idx][ok] - lp_o[ok]) <= 1e-11 * np.abs(lp_o[ok])), np.max(np.abs(lp[idx][ok] - lp_o[ok]) / np.abs(lp_o[ok]))
        sc = np.maximum(np.abs(g_o[:, ok]).max(axis=1, keepdims=True), 1e-300)
        assert np.all(np.abs(g[:, idx][:, ok] - g_o[:, ok]) / sc < 1e-9), (np.abs(g[:, idx][:, ok] - g_o[:, ok]) / sc).max()
        assert np.array_equal(model(th), lp), "the forward-only callback returns the gradient callback's value"
        perm = np.random.default_rng(3).permutation(W)
        for name, cols in (("shard", np.arange(333, 1200)), ("permuted", perm), ("one θ_t", np.array([1234]))):
            lp_s, g_s = model.logdensity_and_gradient(np.ascontiguousarray(th[:, cols]))
            assert np.array_equal(lp_s, lp[cols]), (P, name, "lp", _diff(lp_s, lp[cols]))
            assert np.array_equal(g_s, g[:, cols]), (P, name, "∇θ_t", _diff(g_s, g[:, cols]))
    finally:
        model.close()


def test_batch_invariant_ofti_long_table(pkg, oracle):
    """octo_ofti_eval with the option set on a table of 4 000 rows (several tasks, and a row chunk that plan_key would size differently for one
    draw than for 20 000): one draw, a shard, a permutation and the full batch give the same bits for logml and A/B/F/G; a subsample matches
    the oracle at test_ofti.py's bar."""
    capi = pkg.capi
    rng = np.random.default_rng(808)
    n = 4000
    t = _days(rng, n)
    cols = [t, rng.normal(0, 300, n), rng.normal(0, 300, n), rng.uniform(3, 12, n), rng.uniform(3, 12, n), rng.uniform(-0.5, 0.5, n)]
    W = 20_000
    M = np.abs(rng.normal(1.2, 0.1, W)) + 0.1; plx = rng.normal(50.0, 0.5, W)
    e = rng.uniform(0, 0.99, W); a = np.exp(rng.uniform(0, np.log(100.0), W))
    tp = 50000.0 + rng.uniform(0, 1, W) * np.sqrt(a ** 3 / M) * 365.2568983840419
    e[5] = 1.2; a[6] = 0.0; M[7] = -1.0; tp[8] = np.inf
    nl = np.stack([e, a, tp, M, plx])
    solver = pkg.OftiLinearSolver(*cols, 1000.0)
    try:
        assert solver.lib.octo_ctx_set_option(solver._ctx, capi.OPT_BATCH_INVARIANT, 1) == 0
        full = solver(*nl)
        perm = np.random.default_rng(9).permutation(W)
        shapes = [("one draw", np.array([4321])), ("shard", np.arange(1234, 5679)), ("permuted", perm)]
        got = {name: solver(*nl[:, c]) for name, c in shapes}
    finally:
        solver.close()
    lm = full["log_marginal_likelihood"]
    assert np.all(np.isneginf(lm[5:9])) and np.isfinite(lm).sum() == W - 4
    for name, c in shapes:
        for q in ("log_marginal_likelihood", "A", "B", "F", "G"):
            assert np.array_equal(got[name][q], full[q][c], equal_nan=True), (name, q, _diff(got[name][q], full[q][c]))
    idx = _oracle_cols(W, np.arange(5, 9), 810)
    abfg_o, lm_o = oracle.oracle_ofti(*cols, 1000.0, nl[:, idx])
    ok = np.isfinite(lm_o)
    assert np.array_equal(np.isfinite(lm[idx]), ok)
    assert np.all(np.abs(lm[idx][ok] - lm_o[ok]) <= 1e-8 * np.maximum(1, np.abs(lm_o[ok]))), np.max(np.abs(lm[idx][ok] - lm_o[ok]) / np.maximum(1, np.abs(lm_o[ok])))


@pytest.mark.parametrize("name", ["p1_kinds", "p5_kinds"])
def test_batch_invariant_set_on_a_live_context(pkg, name):
    """The option set on a context that has already evaluated in default mode — two batch sizes, which fill its task-table cache, the tile-sort
    probe (one planet, W >= 2048) and the occupancy cache — gives the bits of a fresh invariant context; get_option reads it back."""
    gb = _gpu()
    capi = pkg.capi
    obs, planets, el, nz, bad, _ = _case(name)
    el = np.concatenate([el, el[:, :700]], axis=1)      # W >= 2048: the tile-sort probe runs on the one-planet context
    nz = None if nz is None else np.concatenate([nz, nz[:, :700]], axis=1)
    sh = np.arange(100, 1100)
    with gb.GpuPath(obs, planets, options={capi.OPT_BATCH_INVARIANT: 1}) as g:
        fresh = g.eval(el, nz, grad=True)
        fresh_sh = g.eval(_sub(el, sh), _sub(nz, sh), grad=True)
    with gb.GpuPath(obs, planets) as g:
        v = C.c_int64(-1)
        assert g.lib.octo_ctx_get_option(g.ctx, capi.OPT_BATCH_INVARIANT, C.byref(v)) == 0 and v.value == 0
        for _ in range(2):
            g.eval(el, nz, grad=True)
            g.eval(_sub(el, sh), _sub(nz, sh), grad=True)
        if len(planets) == 1:
            assert g.tile_state()[1] >= 1, "the tile-sort probe did not run: the test would not see stale tile state"
        assert g.lib.octo_ctx_set_option(g.ctx, capi.OPT_BATCH_INVARIANT, 1) == 0
        assert g.lib.octo_ctx_get_option(g.ctx, capi.OPT_BATCH_INVARIANT, C.byref(v)) == 0 and v.value == 1
        live = g.eval(el, nz, grad=True)
        live_sh = g.eval(_sub(el, sh), _sub(nz, sh), grad=True)
    W = el.shape[1]
    _bitwise(f"{name}: set on a live context, full batch", live, fresh, np.arange(W))
    _bitwise(f"{name}: set on a live context, shard", live_sh, fresh_sh, np.arange(len(sh)))
    _bitwise(f"{name}: fresh invariant context, shard vs full", fresh_sh, fresh, sh)
