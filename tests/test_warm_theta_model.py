"""The premise and the accuracy of k_main's θ-loop (octo_device.h: kepler_warm_theta — the whole Kepler step extrapolated from four recorded steps, on tiles whose
lanes all have ΔM/(1 − e) < WARM_THETA_X0) on its float64 restatement (tests/warm_theta_model.py) against an 80-bit Newton reference. No GPU.

Sample: test_warm_newton_mid_model.py's — config 3's first 64·16 walkers, three chains of 156 daily rows at three offsets into the table — in the order the
device's key gives (warm_theta_model.sorted_order: one segment).

Measured with it (the values this file prints): sorted, 12 of 16 tiles qualify (0 of 16 as drawn); on the qualifying tiles 0.9679 of the θ-loop's wave-rows are
Newton-only — every row of a chain counts: its cold first row (0.0064) and its four start-up rows (0.0256) are the rest, no row leaves by the middle or the
fourth-order arm; with the per-tile rule 0.8706 of ALL sorted wave-rows are Newton-only (middle 0.0576, cold 0.0430) against 0.7350 (0.1756, 0.0644) for today's
loop on the tiles as drawn. D-weighted error of (sin E, cos E) on the θ-loop's Newton-only rows 2.155e-16, the parent's warm step on the same rows 2.155e-16;
1/D 2.0e-15 relative."""
import numpy as np
import pytest

import synth
import warm_newton_mid_model as wmm
import warm_theta_model as wtm
from test_warm_newton_mid_model import OFFSETS

H = 1.0      # the table's step [days]


@pytest.fixture(scope="module")
def sample():
    cfg = synth.config_astrom(n_epochs=10_000, n_walkers=64 * 16, cfg=3)
    el = cfg["elems"]
    order = wtm.sorted_order(el, H, synth.K_YR)
    return el, order, [cfg["table"]["epoch"][lo:lo + 156] for lo in OFFSETS]


@pytest.fixture(scope="module")
def chains(sample):
    el, order, ts = sample
    rng = np.random.default_rng(5)
    els = el[:, order]
    return [dict(theta=wtm.simulate(els, t, synth.K_YR, rng), newton=wmm.simulate(els, t, synth.K_YR, rng), drawn=wmm.simulate(el, t, synth.K_YR, rng)) for t in ts]


def test_the_key_is_a_permutation_that_puts_slow_lanes_first(sample):
    el, order, _ = sample
    assert np.array_equal(np.sort(order), np.arange(el.shape[1]))
    key = wtm.sort_key(el, H, synth.K_YR)
    assert np.all(np.diff(key[order]) >= 0)
    sl = wtm.slow(el, H, synth.K_YR)
    never = key < wtm.TILE_XK
    # among the lanes that never fail the a-priori test, every slow one sits ahead of every other (the class boundary is X0 itself)
    assert key[never & sl].max() < key[never & ~sl].min()
    # with theta off the key is the one class it was: the order of those lanes is the order given
    off = wtm.sorted_order(el, H, synth.K_YR, theta=False)
    n0 = int((wtm.sort_key(el, H, synth.K_YR, theta=False) == 0).sum())
    assert n0 == int(never.sum()) and np.all(np.diff(off[:n0]) > 0)


def test_tiles_qualify_sorted_and_not_as_drawn(sample):
    el, order, _ = sample
    drawn = wtm.qualifying_tiles(el, H, synth.K_YR)
    srt = wtm.qualifying_tiles(el, H, synth.K_YR, order)
    print(f"qualifying tiles: {int(drawn.sum())} of {drawn.size} as drawn, {int(srt.sum())} of {srt.size} sorted")
    assert drawn.mean() <= 0.05, "as drawn no more than a few percent of the tiles qualify: an unsorted batch keeps today's loop"
    assert srt.mean() >= 0.70, "the issue's run: 75 % of the sorted tiles below 0.012"


def test_newton_only_share_on_qualifying_tiles(sample, chains):
    """the issue's run: 0.84 of all sorted wave-rows Newton-only with the θ-loop, against 0.78 as drawn today; a margin of 0.02 for the draws of the reciprocal's error"""
    el, order, _ = sample
    qual = wtm.qualifying_tiles(el, H, synth.K_YR, order)
    th = np.concatenate([c["theta"]["cls"][qual] for c in chains], axis=0)
    rule = np.concatenate([wtm.per_tile_rule(c["theta"]["cls"], c["newton"]["cls"], qual) for c in chains], axis=0)
    drawn = np.concatenate([c["drawn"]["cls"] for c in chains], axis=0)
    share = lambda a, k: float((a == k).mean())
    print(f"theta-loop on qualifying tiles: Newton-only {share(th, wtm.NEWTON):.4f}, middle {share(th, wtm.MIDDLE):.4f}, fourth order {share(th, wtm.FOURTH):.4f}, "
          f"start-up {share(th, wtm.STARTUP):.4f}, cold {share(th, wtm.COLD):.4f}")
    print(f"all sorted tiles, per-tile rule: Newton-only {share(rule, wtm.NEWTON):.4f}, middle {share(rule, wtm.MIDDLE):.4f}, cold {share(rule, wtm.COLD):.4f}; "
          f"as drawn, today's loop: Newton-only {share(drawn, wmm.NEWTON):.4f}, middle {share(drawn, wmm.MIDDLE):.4f}, cold {share(drawn, wmm.COLD):.4f}")
    assert share(th, wtm.NEWTON) >= 0.84 - 0.02
    assert share(rule, wtm.NEWTON) >= 0.84 - 0.02


def test_theta_rows_are_as_accurate_as_the_parents_step(sample, chains):
    """the existing criterion (test_warm_newton_model): the worst D-weighted error of (sin E, cos E) on the Newton-only rows at most 1.25 x the parent's step on the same rows"""
    el, order, _ = sample
    qual = np.repeat(wtm.qualifying_tiles(el, H, synth.K_YR, order), 64)
    worst = worst_par = worst_inv = 0.0
    for c in chains:
        r = c["theta"]
        m = (r["lane_cls"] == wtm.NEWTON) & qual[:, None]
        assert m.any() and np.isfinite(r["err_theta"][m]).all() and np.isfinite(r["err_parent"][m]).all()
        worst = max(worst, r["err_theta"][m].max()); worst_par = max(worst_par, r["err_parent"][m].max()); worst_inv = max(worst_inv, r["invd_rel"][m].max())
        # an accepted row started within τ of the root, and every non-cold row within WARM_TOL
        assert np.all(r["delta"][m] <= np.broadcast_to(r["tau"][:, None], r["delta"].shape)[m])
    print(f"theta-loop Newton-only rows: D-weighted error {worst:.3e} (parent's step {worst_par:.3e}), 1/D relative {worst_inv:.3e}")
    assert worst <= 1.25 * worst_par, (worst, worst_par)
    assert worst_inv <= 1.4e-14, worst_inv
