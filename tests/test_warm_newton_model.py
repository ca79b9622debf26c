"""The premise and the accuracy of k_main's Newton-only warm rows (octo_device.h: kepler_warm_newton), on its float64 restatement
(tests/warm_newton_model.py) against an 80-bit Newton reference. No GPU.

Sample: config 3's first 64·16 walkers (synth.config_astrom(cfg=3)), three chains of 156 daily rows — the chunk one wave of the flagship launch
walks — at three offsets into the table."""
import numpy as np
import pytest

import synth
import warm_bound_model as wbm
import warm_newton_model as wnm


@pytest.fixture(scope="module")
def chains():
    cfg = synth.config_astrom(n_epochs=10_000, n_walkers=64 * 16, cfg=3)
    el = cfg["elems"]
    rng = np.random.default_rng(5)
    return [wnm.simulate(el, cfg["table"]["epoch"][lo:lo + 156], synth.K_YR, rng) for lo in (0, 3120, 7956)]


def test_newton_only_rows_are_as_accurate_as_the_parents_step(chains):
    """D-weighted error of (sin E, cos E) after one step from an exact previous state, on the Newton-only rows: at most 1.25 x the worst of the
    parent's step (warm_bound_model.warm_arm) on the same rows; 1/D within the adjoints' bar."""
    worst_new = worst_par = worst_inv = 0.0
    for c in chains:
        m = c["lane_cls"] == 2
        assert m.any()
        assert np.isfinite(c["err_new"][m]).all() and np.isfinite(c["err_parent"][m]).all()
        worst_new = max(worst_new, c["err_new"][m].max()); worst_par = max(worst_par, c["err_parent"][m].max())
        worst_inv = max(worst_inv, c["invd_rel"][m].max())
    print(f"Newton-only rows: D-weighted error {worst_new:.3e} (parent's step on the same rows {worst_par:.3e}), 1/D relative {worst_inv:.3e}")
    assert worst_new <= 1.25 * worst_par, (worst_new, worst_par)
    assert worst_inv <= 1.4e-14, worst_inv


def test_newton_only_share_of_wave_rows(chains):
    """The premise: most wave-rows of config 3 are Newton-only (every wave-row of the chain counts, its cold first row included)."""
    cls = np.concatenate([c["cls"] for c in chains], axis=0)
    share = {k: float((cls == k).mean()) for k in (0, 1, 2)}
    print(f"wave-rows: Newton-only {share[2]:.3f}, fourth order {share[1]:.3f}, cold {share[0]:.3f}")
    assert share[2] >= 0.6, share


def test_fourth_order_rows_start_within_warm_tol(chains):
    """A row sent to the fourth-order arm has |δ| <= WARM_TOL in every lane: kepler_correct<., FOURTH_ORDER> is calibrated for starts that good."""
    for c in chains:
        m = c["lane_cls"] == 1
        ok = np.isfinite(c["delta"][m])
        assert np.all(c["delta"][m][ok] <= wbm.WARM_TOL)
        # … and a Newton-only row within the lane's τ
        m2 = c["lane_cls"] == 2
        assert np.all(c["delta"][m2] <= np.broadcast_to(c["tau"][:, None], c["delta"].shape)[m2])


def test_tau_edge_cases():
    t = wnm.tau(np.array([0.0, 1e-12, 0.5, 0.999999, 1.0, 1.2, np.nan]))
    assert t[0] == wnm.WARM_NEWTON_CAP and t[1] == wnm.WARM_NEWTON_CAP and t[5] == wnm.WARM_NEWTON_CAP and t[6] == wnm.WARM_NEWTON_CAP
    assert t[4] == 0.0 and 0.0 < t[3] < t[2] <= wnm.WARM_NEWTON_CAP
    assert abs(t[3] ** 2 * 0.999999 / np.sqrt(1 - 0.999999 ** 2) - wnm.WARM_NEWTON_TOL) < 1e-22
