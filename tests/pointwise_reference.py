"""Reference side of the pointwise tests (a helper, not a test; tools/pointwise_bench.py uses it too): the oracle on ONE-ROW sub-tables
(every column sliced, `extra` included, with the table's three nuisance rows), the statistics of its matrix by scipy / NumPy, the bars of
tests/test_pointwise.py as checks that print the observed maxima, and the random tables of its cases."""
import numpy as np

V, RVO, TI, KEP = 0, 1, 2, 3      # orbit kinds
EPS = 2.0 ** -52
NROWS = 7


def one_row(t, j):
    """Row j of a table as a table of its own: every column sliced, `extra` included."""
    out = dict(kind=t["kind"], planet=t["planet"])
    for k in ("epoch", "y1", "y2", "s1", "s2", "cor", "extra"):
        v = t.get(k)
        out[k] = None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64)[j:j + 1])
    return out


def reference_matrix(oracle, tabs, planets, elems, nuis):
    """[R, W] from oracle_eval on one-row sub-tables, rows in table order then row order."""
    rows = []
    for io, t in enumerate(tabs):
        nu = None if nuis is None else np.ascontiguousarray(nuis[io * 3:(io + 1) * 3])
        for j in range(len(t["epoch"])):
            ll, _, _ = oracle.oracle_eval([one_row(t, j)], planets, elems, nu, grad=False)
            rows.append(ll)
    return np.array(rows).reshape(len(rows), elems.shape[1])


def table_values(oracle, tabs, planets, elems, nuis):
    """[n_obs, W]: the oracle's value of each whole table."""
    return np.array([oracle.oracle_eval([t], planets, elems, None if nuis is None else np.ascontiguousarray(nuis[io * 3:(io + 1) * 3]), grad=False)[0]
                     for io, t in enumerate(tabs)])


def head(t, n=NROWS):
    """The first n rows of a table."""
    out = dict(t)
    for k in ("epoch", "y1", "y2", "s1", "s2", "cor", "extra"):
        if out.get(k) is not None:
            out[k] = np.ascontiguousarray(out[k][:n])
    return out


def check_values(name, got, ref):
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    assert fin.all(), name
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"values {name}: max err / max(1, |ll|) = {err.max():.3e}, |ll| up to {np.abs(ref).max():.3e}")
    assert err.max() <= 1e-11, (name, err.max())
    return float(err.max())


def random_table(capi, kind, planet, seed, n=NROWS, cor=False, basis=False):
    rng = np.random.default_rng(seed)
    epoch = np.sort(rng.uniform(55000.0, 60000.0, n))
    if kind == capi.ASTROM_RADEC:
        return dict(kind=kind, planet=planet, epoch=epoch, y1=rng.normal(0, 200.0, n), y2=rng.normal(0, 200.0, n), s1=rng.uniform(1.0, 5.0, n),
                    s2=rng.uniform(1.0, 5.0, n), cor=rng.uniform(-0.7, 0.7, n) if cor else None, extra=None)
    if kind == capi.ASTROM_SEPPA:
        return dict(kind=kind, planet=planet, epoch=epoch, y1=rng.uniform(-3.0, 3.0, n), y2=rng.uniform(50.0, 400.0, n), s1=rng.uniform(0.01, 0.05, n),
                    s2=rng.uniform(1.0, 5.0, n), cor=None, extra=None)
    return dict(kind=kind, planet=planet, epoch=epoch, y1=rng.normal(0, 60.0, n), y2=None, s1=rng.uniform(2.0, 9.0, n), s2=None, cor=None,
                extra=(epoch - 57000.0) if basis else None)


def random_nuis(tabs, W, seed):
    rng = np.random.default_rng(seed)
    nu = np.empty((3 * len(tabs), W))
    for io, t in enumerate(tabs):
        if t["kind"] < 2:
            nu[io * 3:(io + 1) * 3] = [rng.uniform(0.1, 2.0, W), rng.uniform(0.98, 1.02, W), rng.uniform(-0.05, 0.05, W)]
        else:
            nu[io * 3:(io + 1) * 3] = [rng.normal(0, 20.0, W), rng.uniform(0.5, 6.0, W), rng.normal(0, 0.01, W)]
    return nu


def five_planets(pkg, W, seed=9):
    import predict_reference as ref
    capi = pkg.capi
    planets = [dict(orbit_kind=V, has_mass=1) for _ in range(5)]
    elems = ref.random_elements(planets, W, seed=seed, e_max=0.9)
    tabs = [random_table(capi, capi.ASTROM_RADEC, 3, seed=21, cor=True), random_table(capi, capi.RV_ABS, -1, seed=22, basis=True)]
    return tabs, planets, elems, random_nuis(tabs, W, seed=23)


def summary_reference(refm):
    from scipy.special import logsumexp
    out = {k: np.full(refm.shape[0], np.nan) for k in ("lppd", "mean", "var", "elpd_is_loo", "min", "max")}
    out["n"] = np.zeros(refm.shape[0])
    for r, row in enumerate(refm):
        x = row[np.isfinite(row)]
        out["n"][r] = x.size
        if x.size == 0:
            continue
        out["lppd"][r] = logsumexp(x) - np.log(x.size)
        out["elpd_is_loo"][r] = -(logsumexp(-x) - np.log(x.size))
        out["mean"][r], out["min"][r], out["max"][r] = x.mean(), x.min(), x.max()
        out["var"][r] = x.var(ddof=1) if x.size > 1 else np.nan
    return out


def check_summary(name, s, refm, keys=("lppd", "elpd_is_loo", "mean", "min", "max", "var")):
    """The device's summary against logsumexp / NumPy on the ORACLE's matrix, at the bars of the module's docstring."""
    want = summary_reference(refm)
    assert np.array_equal(s["n"], want["n"]), (name, s["n"], want["n"])
    worst = {}
    for r in range(refm.shape[0]):
        x = refm[r][np.isfinite(refm[r])]
        n = x.size
        if n == 0:
            continue
        delta = 1e-11 * max(1.0, np.abs(x).max())
        for k in [k for k in keys if k != "var"]:
            bar = delta + n * EPS * max(1.0, abs(want[k][r]))
            err = abs(s[k][r] - want[k][r])
            worst[k] = max(worst.get(k, 0.0), err / bar)
            assert err <= bar, (name, k, r, s[k][r], want[k][r], err, bar)
        if n > 1 and "var" in keys:
            bar = 4.0 * np.sqrt(want["var"][r]) * delta + delta * delta + n * EPS * want["var"][r]
            err = abs(s["var"][r] - want["var"][r])
            worst["var"] = max(worst.get("var", 0.0), err / bar)
            assert err <= bar, (name, "var", r, s["var"][r], want["var"][r], err, bar)
    print(f"summary {name}: largest error / bar " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    return worst
