"""The premise and the accuracy of the middle arm of k_main's Newton-only warm rows (octo_device.h: kepler_warm_newton — one Halley step for a wave-row
whose lanes all start within τ₂(e) of the root), on its float64 restatement (tests/warm_newton_mid_model.py) against an 80-bit Newton reference. No GPU.

Sample: test_warm_newton_model.py's — config 3's first 64·16 walkers (synth.config_astrom(cfg=3)), three chains of 156 daily rows at three offsets
into the table. Measured with it: D-weighted error of (sin E, cos E) on the middle rows 2.16e-16 for the arm (2.16e-16 for the fourth-order arm from the
same start, 4.43e-16 for the parent's warm step), 1/D 1.33e-15 relative; 0.1756 of all wave-rows take the arm."""
import numpy as np
import pytest

import synth
import warm_newton_mid_model as wmm
import warm_newton_model as wnm

OFFSETS = (0, 3120, 7956)


@pytest.fixture(scope="module")
def sample():
    cfg = synth.config_astrom(n_epochs=10_000, n_walkers=64 * 16, cfg=3)
    return cfg["elems"], [cfg["table"]["epoch"][lo:lo + 156] for lo in OFFSETS]


@pytest.fixture(scope="module")
def chains(sample):
    el, ts = sample
    rng = np.random.default_rng(5)
    return [wmm.simulate(el, t, synth.K_YR, rng) for t in ts]


def test_middle_rows_are_as_accurate_as_the_parents_step(chains):
    """D-weighted error of (sin E, cos E) after one step from an exact previous state, on the rows the middle arm takes: at most 1.25 x the worst of the
    parent's step (warm_bound_model.warm_arm) on the same rows — test_warm_newton_model's criterion; 1/D within the adjoints' bar."""
    worst_mid = worst_4 = worst_par = worst_inv = 0.0
    for c in chains:
        m = c["lane_cls"] == wmm.MIDDLE
        assert m.any()
        for k in ("err_mid", "err_fourth", "err_parent", "invd_rel_mid"):
            assert np.isfinite(c[k][m]).all(), k
        worst_mid = max(worst_mid, c["err_mid"][m].max()); worst_4 = max(worst_4, c["err_fourth"][m].max())
        worst_par = max(worst_par, c["err_parent"][m].max()); worst_inv = max(worst_inv, c["invd_rel_mid"][m].max())
    print(f"middle rows: D-weighted error {worst_mid:.3e} (fourth-order arm from the same start {worst_4:.3e}, parent's step {worst_par:.3e}), "
          f"1/D relative {worst_inv:.3e}")
    assert worst_mid <= 1.25 * worst_par, (worst_mid, worst_par)
    assert worst_inv <= 1.4e-14, worst_inv


def test_middle_rows_start_within_tau2(chains):
    """Every lane of a middle row has τ-or-more somewhere in its wave and |δ| <= τ₂(e) itself; a fourth-order row |δ| <= WARM_TOL."""
    for c in chains:
        t2 = np.broadcast_to(c["tau2"][:, None], c["delta"].shape)
        m = c["lane_cls"] == wmm.MIDDLE
        assert np.all(c["delta"][m] <= t2[m])
        assert np.all(c["tau2"] >= c["tau"])
        m4 = c["lane_cls"] == wmm.FOURTH
        assert np.all(c["delta"][m4] <= wnm.wbm.WARM_TOL)
        # a middle wave-row is not a Newton-only one: some lane of the wave is beyond its τ
        over = (c["delta"] > c["tau"][:, None]).reshape(-1, 64, c["delta"].shape[1]).any(axis=1)
        assert np.all(over[c["cls"] == wmm.MIDDLE])


def test_middle_share_of_wave_rows(chains):
    """The premise: the arm takes a good part of ALL wave-rows (every wave-row of the chain counts, its cold first row included)."""
    cls = np.concatenate([c["cls"] for c in chains], axis=0)
    share = {k: float((cls == k).mean()) for k in (wmm.COLD, wmm.FOURTH, wmm.NEWTON, wmm.MIDDLE)}
    print(f"wave-rows: Newton-only {share[wmm.NEWTON]:.4f}, middle {share[wmm.MIDDLE]:.4f}, fourth order {share[wmm.FOURTH]:.4f}, cold {share[wmm.COLD]:.4f}")
    assert share[wmm.MIDDLE] >= 0.12, share


def test_routing_is_warm_newton_models_with_the_fourth_order_class_split(sample, chains):
    """With the middle class folded back into the fourth-order one the routing is warm_newton_model.simulate's, row for row (the same draws)."""
    el, ts = sample
    rng = np.random.default_rng(5)
    for t, c in zip(ts, chains):
        ref = wnm.simulate(el, t, synth.K_YR, rng)["cls"]
        assert np.array_equal(np.where(c["cls"] == wmm.MIDDLE, wmm.FOURTH, c["cls"]), ref)


def test_tau2_edge_cases():
    cap, tol = wmm.WARM_NEWTON_MID_CAP, wmm.WARM_NEWTON_MID_TOL
    t = wmm.tau2(np.array([0.0, 1e-12, 0.5, 0.999999, 1.0, 1.2, np.nan]))
    assert t[0] == cap and t[1] == cap and t[5] == cap and t[6] == cap
    assert t[4] == 0.0 and 0.0 < t[3] < t[2] <= cap
    assert abs(t[3] ** 3 * wmm.kappa(0.999999) - tol) < 1e-22
    # the cap binds where κ <= tol/cap³ = 0.39 (κ(0.5) = 0.33, κ(0.6) = 0.53), and τ₂ is never below τ
    e = np.linspace(0.0, 0.999999, 20001)
    assert np.all(wmm.tau2(e) >= wnm.tau(e))
    assert wmm.tau2(np.array([0.5]))[0] == cap and wmm.tau2(np.array([0.6]))[0] < cap
