"""The reference helper of the model-value tests (tests/predict_reference.py) against oracle_eval ALONE (CPU): model values composed from
the oracle's orbitsolve primitives, pushed through the helper's host-side Gaussian log-likelihoods, must give the oracle's log-likelihood.
This leaves the device as the only unknown of tests/test_predict.py's closure test."""
import numpy as np


def test_helper_loglike_matches_oracle_eval(oracle):
    import predict_reference as ref
    tabs, planets, elems, nuis, _ = ref.two_planet_system(seed=11, W=48)
    a0, a1 = elems[0], elems[9]
    assert (a0 < a1).any() and (a1 < a0).any()      # either planet is the inner one for some walker
    assert elems[1].max() > 0.9 or elems[10].max() > 0.9
    models = ref.table_models(tabs, planets, elems, nuis)
    ll = ref.tables_loglike(tabs, models, nuis)
    ll_o, _, _ = oracle.oracle_eval(tabs, planets, elems, nuis, grad=False)
    assert np.isfinite(ll_o).all() and np.isfinite(ll).all()
    err = np.abs(ll - ll_o) / np.maximum(1.0, np.abs(ll_o))
    print(f"helper vs oracle_eval: max rel err {err.max():.3e}")
    assert err.max() < 1e-12, err.max()


def test_helper_loglike_near_the_truth_is_moderate(oracle):
    import predict_reference as ref
    tabs, planets, elems, nuis, truth = ref.two_planet_system(seed=5, W=16, spread=1e-3)
    assert np.array_equal(elems[:, 0], truth)
    ll = ref.tables_loglike(tabs, ref.table_models(tabs, planets, elems, nuis), nuis)
    ll_o, _, _ = oracle.oracle_eval(tabs, planets, elems, nuis, grad=False)
    assert np.isfinite(ll_o).all()
    assert 1e2 < np.abs(ll_o).max() < 1e4 and 1e2 < np.abs(ll_o[0]) < 1e4, ll_o
    assert (np.abs(ll - ll_o) / np.maximum(1.0, np.abs(ll_o))).max() < 1e-12
