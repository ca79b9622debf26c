"""
Model values on the device (include/octofitter_hip_predict.h, host/predict.py) against the oracle — GPU suite.

Bars. Primitives and composite channels: the project's 1e-8, relative to the quantity's natural scale per walker (a·plx·(1 + e) mas for offsets
and separations, the oracle's K·(1 + e) for velocities; a position angle as the wrapped angle difference weighted by ρ / scale); the observed
maxima are printed (tools/predict_bench.py writes them to profiles/predict_throughput.txt). Closure: 1e-11 of max(1, |ll|), the bar of
tests/test_model.py's caller parity. Invariance: bitwise. Summary against NumPy statistics of the device's own cube: n_valid exact, the rest
within 1e-12·(|mean| + sd + scale·1e-16).
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V, RVO, TI, KEP = 0, 1, 2, 3      # orbit kinds


def planets_of(kinds, masses=None):
    return [dict(orbit_kind=k, has_mass=int(bool(masses[i])) if masses else 0) for i, k in enumerate(kinds)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def grid(seed, T, tp_far=True):
    """An unsorted grid with repeated epochs and epochs 1e5 days away from every tp (tp is drawn in 50000 … 60000)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(50000.0, 62000.0, T)
    if T >= 4:
        t[1] = t[0]; t[T - 1] = t[2]
    if tp_far and T >= 6:
        t[3] = 160000.0 + rng.uniform(0, 10); t[5] = -45000.0
    return t


def all_channels(pkg, planets):
    p_ = pkg.predict
    ch = []
    for i, pl in enumerate(planets):
        if pl["orbit_kind"] in (V, TI):
            ch += [(p_.RAOFF, i), (p_.DECOFF, i), (p_.SEP, i), (p_.PA, i)]
        if pl["orbit_kind"] != TI:
            ch += [(p_.RADVEL, i)]
    return ch


@pytest.mark.parametrize("kinds", [(V,), (RVO,), (TI,), (KEP,), (V, TI), (V, RVO, KEP, V), (V, V, TI, V, KEP, V)], ids=lambda k: "kinds" + "".join(map(str, k)))
def test_primitives_against_oracle(pkg, oracle, kinds):
    import predict_reference as ref
    planets = planets_of(kinds)
    W, T = 20, 12
    elems = ref.random_elements(planets, W, seed=100 + len(kinds))
    epochs = grid(3, T)
    ch = all_channels(pkg, planets)[:pkg.predict.MAX_CHANNELS]
    pr = pkg.Predictor(planets, epochs, ch)
    try:
        cube = pr.values(elems)
    finally:
        pr.close()
    assert np.isfinite(cube).all()
    errs, _ = ref.channel_errors(planets, elems, epochs, ch, cube)
    print("primitives", kinds, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-8, errs


def composite_channels(pkg, P):
    p_ = pkg.predict
    ch = [(p_.RV_STAR, -1)]
    for i in range(P):
        ch += [(p_.ASTROM_RA, i), (p_.ASTROM_DEC, i), (p_.ASTROM_SEP, i), (p_.ASTROM_PA, i), (p_.RV_REL, i)]
    return ch


@pytest.mark.parametrize("P", [2, 4])
def test_composite_channels_against_reference(pkg, oracle, P):
    import predict_reference as ref
    planets = planets_of((V,) * P, masses=(1, 1, 0, 1)[:P])
    W, T = 18, 10
    elems = ref.random_elements(planets, W, seed=7 + P, e_max=0.95)
    # a walker pair that swaps which planet is the inner one: the same orbits with the semi-major axes of planets 0 and 1 exchanged
    elems[:, 3] = elems[:, 2]
    elems[0, 3], elems[9, 3] = elems[9, 2], elems[0, 2]
    assert (elems[0, 2] < elems[9, 2]) != (elems[0, 3] < elems[9, 3])
    epochs = grid(5, T)
    ch = composite_channels(pkg, P)
    rng = np.random.default_rng(1)
    add0, add1, basis = rng.normal(0, 30.0, (len(ch), W)), rng.normal(0, 0.01, (len(ch), W)), epochs - 57000.0
    pr = pkg.Predictor(planets, epochs, ch, basis=basis)
    try:
        cube = pr.values(elems, add0=add0, add1=add1)
    finally:
        pr.close()
    errs, refcube = ref.channel_errors(planets, elems, epochs, ch, cube, add0, add1, basis)
    print("composite", P, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) < 1e-8, errs
    # the reflex terms are really there: the composite differs from the bare offset wherever an inner planet has a mass
    bare = ref.channel_values(planets, elems, epochs, [(pkg.predict.RAOFF, 1)])[0]
    inner0 = elems[0] < elems[9]
    assert np.all(np.abs(refcube[ch.index((pkg.predict.ASTROM_RA, 1))] - bare)[:, inner0] > 0)


def test_closure_simulate_tables_gives_the_likelihood(pkg, oracle):
    import gpu_binding
    import predict_reference as ref
    tabs, planets, elems, nuis, _ = ref.two_planet_system(seed=5, W=32, spread=1e-3)
    models = pkg.simulate_tables(tabs, planets, elems, nuis)
    ll = ref.tables_loglike(tabs, models, nuis)
    ll_o, _, _ = oracle.oracle_eval(tabs, planets, elems, nuis, grad=False)
    ll_g, _, _ = gpu_binding.gpu_eval(tabs, planets, elems, nuis, grad=False)
    assert np.isfinite(ll).all() and np.isfinite(ll_o).all() and np.isfinite(ll_g).all()
    assert 1e2 < np.abs(ll_o).max() < 1e4
    e_o = np.abs(ll - ll_o) / np.maximum(1.0, np.abs(ll_o))
    e_g = np.abs(ll - ll_g) / np.maximum(1.0, np.abs(ll_g))
    print(f"closure: vs oracle_eval {e_o.max():.3e}, vs octo_eval {e_g.max():.3e}, |ll| up to {np.abs(ll_o).max():.1f}")
    assert e_o.max() < 1e-11 and e_g.max() < 1e-11, (e_o.max(), e_g.max())


def test_simulate_tables_kinds_and_hgca(pkg, oracle):
    import predict_reference as ref
    capi = pkg.capi
    tabs, planets, elems, nuis, _ = ref.two_planet_system(seed=5, W=5, spread=1e-3)
    marg = dict(tabs[2]); marg["kind"] = capi.RV_ABS_MARG
    oneil = dict(tabs[0]); oneil["kind"] = capi.ONEIL_RADEC
    oneil2 = dict(tabs[1]); oneil2["kind"] = capi.ONEIL_SEPPA
    tabs2 = [marg, oneil, oneil2]
    nu2 = np.ascontiguousarray(np.concatenate([nuis[6:9], nuis[0:3], nuis[3:6]]))
    got = pkg.simulate_tables(tabs2, planets, elems, nu2)
    want = ref.table_models(tabs2, planets, elems, nu2)
    base = ref.table_models([tabs[2]], planets, elems, nuis[6:9])[0]["rv"]
    assert np.allclose(want[0]["rv"] + nuis[6][None, :], base, rtol=0, atol=1e-9)      # the marginalised table's model carries no offset
    for g, w in zip(got, want):
        for k in w:
            assert np.allclose(g[k], w[k], rtol=1e-9, atol=1e-9), k
    hg = dict(kind=capi.HGCA, planet=-1, epoch=np.array([55000.0]), y1=np.zeros(1), y2=np.zeros(1), s1=None, s2=None, cor=None, extra=np.zeros(15))
    with pytest.raises(capi.OctoError) as ex:
        pkg.simulate_tables([hg], planets, elems, None)
    assert ex.value.status == capi.OCTO_ENOTSUP


def test_invariance_is_bitwise(pkg):
    import torch
    import predict_reference as ref
    planets = planets_of((V, V), masses=(1, 1))
    ch = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 0)] + composite_channels(pkg, 2)
    Wmax, T = 1000, 9
    elems = ref.random_elements(planets, Wmax, seed=42)
    epochs = grid(8, T)
    rng = np.random.default_rng(2)
    add0, basis = rng.normal(0, 10.0, (len(ch), Wmax)), epochs - 57000.0
    add1 = rng.normal(0, 0.01, (len(ch), Wmax))
    pr = pkg.Predictor(planets, epochs, ch, basis=basis)
    perm_t = rng.permutation(T)
    pr_perm = pkg.Predictor(planets, epochs[perm_t], ch, basis=basis[perm_t])
    try:
        full = pr.values(elems, add0, add1)
        for W in (1, 63, 64, 65):                                   # the batch size
            sub = pr.values(elems[:, :W], add0[:, :W], add1[:, :W])
            assert np.array_equal(bits(sub), bits(full[:, :, :W])), W
        perm = rng.permutation(Wmax)                                # the walker's index
        moved = pr.values(elems[:, perm], add0[:, perm], add1[:, perm])
        assert np.array_equal(bits(moved), bits(full[:, :, perm]))
        g = pr_perm.values(elems, add0, add1)                       # the grid order
        assert np.array_equal(bits(g), bits(full[:, perm_t, :]))
        for variant in (1, 2):                                      # the store width
            pr.set_variant(variant)
            assert np.array_equal(bits(pr.values(elems, add0, add1)), bits(full)), variant
            assert np.array_equal(bits(pr.values(elems[:, :65], add0[:, :65], add1[:, :65])), bits(full[:, :, :65])), variant
        pr.set_variant(0)
        dev = torch.device("cuda", 0)                               # host buffers against device buffers
        d = pr.values(torch.from_numpy(elems).to(dev), torch.from_numpy(add0).to(dev), torch.from_numpy(add1).to(dev))
        torch.cuda.synchronize()
        assert np.array_equal(bits(d.cpu().numpy()), bits(full))
    finally:
        pr.close(); pr_perm.close()


@pytest.mark.parametrize("P", [1, 2, 6])
def test_invalid_walkers_give_nan_columns(pkg, P):
    import predict_reference as ref
    planets = planets_of((V,) * P, masses=(1,) * P)
    ch = [(pkg.predict.RAOFF, 0), (pkg.predict.RADVEL, P - 1), (pkg.predict.RV_STAR, -1), (pkg.predict.ASTROM_PA, P - 1)]
    W, T = 130, 7
    elems = ref.random_elements(planets, W, seed=9)
    epochs = grid(4, T)
    bad = elems.copy()
    p9 = (P - 1) * 9
    cases = {3: (p9 + 3, np.nan), 17: (1, 1.0), 64: (p9 + 1, -0.1), 65: (0, 0.0), 66: (p9 + 0, -2.0), 100: (6, 0.0), 129: (p9 + 6, -1.0), 70: (5, np.inf)}
    for w, (row, val) in cases.items():
        bad[row, w] = val
    pr = pkg.Predictor(planets, epochs, ch)
    try:
        good_cube = pr.values(elems)
        cube = pr.values(bad)                                       # OCTO_OK: no exception
    finally:
        pr.close()
    assert np.isfinite(good_cube).all()
    mask = np.zeros(W, dtype=bool); mask[list(cases)] = True
    assert np.isnan(cube[:, :, mask]).all()
    assert np.array_equal(bits(cube[:, :, ~mask]), bits(good_cube[:, :, ~mask]))      # the neighbours are untouched


@pytest.mark.parametrize("P,W", [(1, 1 << 17), (2, 5000), (6, 700), (1, 257)])
def test_summary_against_numpy_on_the_devices_cube(pkg, P, W):
    import predict_reference as ref
    planets = planets_of((V,) * P, masses=(1,) * P)
    ch = [(pkg.predict.RAOFF, 0), (pkg.predict.DECOFF, P - 1), (pkg.predict.RADVEL, 0), (pkg.predict.RV_STAR, -1), (pkg.predict.ASTROM_SEP, P - 1)]
    T = 6
    elems = ref.random_elements(planets, W, seed=31, e_max=0.9)
    rng = np.random.default_rng(4)
    n_bad = max(W // 100, 1)                                        # 1 % invalid walkers
    badw = rng.choice(W, n_bad, replace=False)
    elems[1, badw] = 1.5
    epochs = grid(6, T)
    pr = pkg.Predictor(planets, epochs, ch)
    try:
        cube = pr.values(elems)
        s1 = pr.summary(elems)
        s2 = pr.summary(elems)
    finally:
        pr.close()
    for k in s1:
        assert np.array_equal(bits(s1[k]), bits(s2[k])), k         # run to run
    ok = ~np.isnan(cube)
    assert np.array_equal(ok.sum(axis=2), np.full((len(ch), T), W - n_bad))
    assert np.array_equal(s1["n_valid"], ok.sum(axis=2).astype(np.float64))
    valid = cube[:, :, ok[0, 0]]
    mean, sd = valid.mean(axis=2), valid.std(axis=2, ddof=1)
    scale = np.abs(valid).max(axis=2)
    tol = 1e-12 * (np.abs(mean) + sd + scale * 1e-16)
    for name, want in (("mean", mean), ("sd", sd), ("min", valid.min(axis=2)), ("max", valid.max(axis=2))):
        err = np.abs(s1[name] - want)
        print(f"summary P={P} W={W} {name}: max err/tol {np.max(err / tol):.3e}")
        assert np.all(err <= tol), (name, np.max(err / tol))


def test_summary_edge_counts(pkg):
    import predict_reference as ref
    planets = planets_of((V,))
    ch = [(pkg.predict.RAOFF, 0), (pkg.predict.RADVEL, 0)]
    epochs = grid(1, 5)
    elems = ref.random_elements(planets, 300, seed=3)
    pr = pkg.Predictor(planets, epochs, ch)
    try:
        one = pr.summary(elems[:, 5:6])                             # W = 1: sd is NaN (the sample variance of one value, 0/0), documented in the header
        cube1 = pr.values(elems[:, 5:6])
        assert np.array_equal(one["n_valid"], np.ones((2, 5))) and np.isnan(one["sd"]).all()
        for k in ("mean", "min", "max"):
            assert np.array_equal(bits(one[k]), bits(cube1[:, :, 0])), k
        dead = elems.copy(); dead[1] = 1.0                          # every walker invalid
        none = pr.summary(dead)
        assert np.array_equal(none["n_valid"], np.zeros((2, 5)))
        assert all(np.isnan(none[k]).all() for k in ("mean", "sd", "min", "max"))
        lone = dead.copy(); lone[1, 299] = elems[1, 299]            # one valid walker in the last block
        s = pr.summary(lone)
        assert np.array_equal(s["n_valid"], np.ones((2, 5))) and np.array_equal(bits(s["mean"]), bits(pr.values(elems[:, 299:300])[:, :, 0]))
    finally:
        pr.close()


def test_shapes_and_leading_dimensions(pkg):
    import torch
    import predict_reference as ref
    capi, predict = pkg.capi, pkg.predict
    planets = planets_of((V, V), masses=(1, 0))
    elems = ref.random_elements(planets, 37, seed=12)
    # 32 channels
    ch32 = (all_channels(pkg, planets) + composite_channels(pkg, 2)) * 2
    ch32 = ch32[:32]
    epochs = grid(2, 11)
    pr = pkg.Predictor(planets, epochs, ch32)
    try:
        full = pr.values(elems)
        assert full.shape == (32, 11, 37) and np.isfinite(full).all()
        n_unique = len(set(ch32))
        for c, key in enumerate(ch32):
            assert np.array_equal(bits(full[c]), bits(full[ch32.index(key)]))
        assert n_unique >= 15
        # W = 1
        assert np.array_equal(bits(pr.values(elems[:, 4:5])), bits(full[:, :, 4:5]))
        # ld > W and ld_out > W through the C ABI: host buffers …
        lib = predict.load_library()
        W, ld, ldo = 21, 37, 29
        out = np.full((32 * 11, ldo), -7.0)
        assert lib.octo_predict_eval(pr._h, capi._dptr(elems), ld, W, None, None, capi._dptr(out), ldo) == capi.OCTO_OK
        assert np.array_equal(bits(out[:, :W].reshape(32, 11, W)), bits(full[:, :, :W])) and np.all(out[:, W:] == -7.0)
        # … and device buffers (an odd ld_out: the 8-byte store path)
        dev = torch.device("cuda", 0)
        d_el = torch.from_numpy(elems).to(dev)
        d_out = torch.full((32 * 11, ldo), -7.0, dtype=torch.float64, device=dev)
        st = lib.octo_predict_eval_device(pr._h, d_el.data_ptr(), ld, W, None, None, d_out.data_ptr(), ldo, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert st == capi.OCTO_OK
        torch.cuda.synchronize()
        o = d_out.cpu().numpy()
        assert np.array_equal(bits(o[:, :W].reshape(32, 11, W)), bits(full[:, :, :W])) and np.all(o[:, W:] == -7.0)
        # bad sizes
        assert lib.octo_predict_eval(pr._h, capi._dptr(elems), 20, W, None, None, capi._dptr(out), ldo) == capi.OCTO_EINVAL
        assert lib.octo_predict_eval(pr._h, capi._dptr(elems), ld, W, None, None, capi._dptr(out), 20) == capi.OCTO_EINVAL
        assert b"W" in lib.octo_predict_last_error(pr._h)
    finally:
        pr.close()
    # T = 1
    pr1 = pkg.Predictor(planets, epochs[4:5], ch32[:3])
    try:
        assert np.array_equal(bits(pr1.values(elems)), bits(full[:3, 4:5, :]))
    finally:
        pr1.close()


def test_host_cube_larger_than_the_staging_buffer(pkg):
    import predict_reference as ref
    planets = planets_of((V,))
    ch = [(pkg.predict.RAOFF, 0), (pkg.predict.DECOFF, 0), (pkg.predict.RADVEL, 0)]
    epochs = grid(7, 40)
    elems = ref.random_elements(planets, 333, seed=77)
    pr = pkg.Predictor(planets, epochs, ch)
    old = {k: os.environ.get(k) for k in ("OCTO_PREDICT_CUBE_BYTES", "OCTO_PREDICT_STAGE_BYTES")}
    # device cube buffer 3·40·8 B·50 walkers, staging 17 rows of a chunk: 333 walkers cross six chunk boundaries, each chunk several staging passes
    os.environ["OCTO_PREDICT_CUBE_BYTES"] = str(3 * 40 * 8 * 50)
    os.environ["OCTO_PREDICT_STAGE_BYTES"] = str(17 * 50 * 8)
    try:
        small = pkg.Predictor(planets, epochs, ch)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        want = pr.values(elems)
        got = small.values(elems)
        assert np.isfinite(want).all() and np.array_equal(bits(got), bits(want))
    finally:
        pr.close(); small.close()


def test_callers_stream_orders_the_device_call(pkg):
    import torch
    import predict_reference as ref
    planets = planets_of((V,))
    ch = [(pkg.predict.RAOFF, 0), (pkg.predict.RADVEL, 0)]
    epochs = grid(9, 16)
    elems = ref.random_elements(planets, 4096, seed=5)
    dev = torch.device("cuda", 0)
    pr = pkg.Predictor(planets, epochs, ch)
    try:
        want = pr.values(elems)
        src = torch.from_numpy(elems).to(dev)
        d_el = torch.full_like(src, float("nan"))
        a = torch.randn(4096, 4096, device=dev)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            for _ in range(8):                                      # work ahead of the producer, so that the producer has not run when the call is enqueued
                a = a @ a * 1e-3
            d_el.copy_(src * 1.0)                                   # the producer kernel on the caller's stream
            got = pr.values(d_el, stream=s.cuda_stream)
            band = pr.summary(d_el, stream=s.cuda_stream)
        s.synchronize()
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert np.array_equal(band["n_valid"].cpu().numpy(), np.full((2, 16), 4096.0))
    finally:
        pr.close()


def test_posterior_predictive_caller(pkg):
    import predict_reference as ref
    planets = planets_of((V,))
    ch = [("RAOFF", 0), ("DECOFF", 0), ("RADVEL", 0)]
    epochs = np.linspace(57000.0, 60000.0, 50)
    elems = ref.random_elements(planets, 500, seed=8, e_max=0.8)
    band = pkg.posterior_predictive(planets, elems, epochs, ch)
    cube = pkg.posterior_predictive(planets, elems, epochs, ch, summary=False)
    assert cube.shape == (3, 50, 500) and band["mean"].shape == (3, 50)
    assert np.allclose(band["mean"], cube.mean(axis=2), rtol=1e-12, atol=1e-12 * np.abs(cube).max())
    assert np.array_equal(band["max"], cube.max(axis=2)) and np.array_equal(band["min"], cube.min(axis=2))
