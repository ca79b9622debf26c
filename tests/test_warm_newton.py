"""
k_main's Newton-only warm rows (octo_device.h: kepler_warm_newton): on an evenly sampled RA/Dec table the gap between the second-order predictor and
the root is extrapolated from the rows behind, and a row whose start then lies within τ(e) of the root in every lane of the wave takes ONE Newton
step; the others take the fourth-order correction from the same start, or the cold solve. The root is unique, so the loop must agree with the warm
loop it replaces (OCTO_WARM_NEWTON=0: the same library without it), with the cold loop (OCTO_WARM=0) and with the oracle — at the bars
tests/test_warm_start.py holds the warm loop to (its _close: 1e-12 on ll, 1e-10 on the gradient against the other loop; 1e-10 / 1e-8 against the oracle).

One planet, 700 daily RA/Dec epochs (past two WARM_RESTARTs, several tasks, a short last chunk), 192 walkers in three tiles:
  tile 0   slow walkers (a >= 20 AU, e <= 0.5): every warm row Newton-only;
  tile 1   as drawn, plus one walker at a = 1 AU, e = 0.93: fourth-order and cold rows for the whole wave around its periastron;
  tile 2   as drawn, with an invalid walker (e = 1.2) and a NaN element.
"""
import os

import numpy as np
import pytest

import synth
from test_gpu_parity import _cmp_oracle, _gpu
from test_warm_start import _close, _same_bits

pytestmark = pytest.mark.gpu

PLANETS = [dict(orbit_kind=0, has_mass=False)]
ACT = synth.active_mask(1, 1, mass=False, nuis=False)
N, W = 700, 192
INVALID = (140, 171)      # e = 1.2; a NaN element


def _eval(gb, obs, elems, grad=True, newton=True, warm=True, env=None):
    env = dict(env or {}, OCTO_WARM="1" if warm else "0", OCTO_WARM_NEWTON="1" if newton else "0")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return gb.gpu_eval(obs, PLANETS, elems, None, grad=grad, small_batch=0)      # the throughput kernels whatever the batch size
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _table(t, rng, cor=False):
    ra, dec = synth.truth_radec(t)
    n = t.size
    return [dict(kind=0, planet=0, epoch=t, y1=ra + rng.normal(0, 5, n), y2=dec + rng.normal(0, 5, n), s1=np.full(n, 5.0), s2=np.full(n, 7.0),
                 cor=rng.uniform(-0.6, 0.6, n) if cor else None)]


def _walkers(rng):
    el = synth.draw_walkers(rng, W, 1.5, 100.0)
    el[0, :64] = np.exp(rng.uniform(np.log(20.0), np.log(100.0), 64)); el[1, :64] = rng.uniform(0.0, 0.5, 64)
    el[5, :64] = 50000.0 + rng.uniform(0.0, 1.0, 64) * synth.K_YR * np.sqrt(el[0, :64] ** 3 / el[6, :64])
    el[0, 100] = 1.0; el[1, 100] = 0.93; el[5, 100] = 50000.0 + 150.0      # periastron passages inside the table (P = 333 d)
    el[1, INVALID[0]] = 1.2; el[3, INVALID[1]] = np.nan
    return el


@pytest.fixture(scope="module")
def case(oracle):
    """the dataset, its walkers, the oracle's answer and the three device answers every test below reads (computed once, never modified)"""
    gb = _gpu()
    rng = np.random.default_rng(91)
    t = 50000.0 + 1.0 * np.arange(N)
    obs = _table(t, rng)
    el = _walkers(rng)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    on = _eval(gb, obs, el)
    off = _eval(gb, obs, el, newton=False)
    cold = _eval(gb, obs, el, warm=False)
    return dict(gb=gb, t=t, obs=obs, el=el, ll_o=ll_o, g_o=g_o, on=on, off=off, cold=cold)


def test_newton_rows_against_the_oracle_the_warm_loop_and_the_cold_loop(case):
    on, off, cold = case["on"], case["off"], case["cold"]
    _cmp_oracle("newton", on[0], on[1], None, case["ll_o"], case["g_o"], None, ll_rtol=1e-10, g_rtol=1e-8)
    _close("newton vs warm", on, off)
    _close("newton vs cold", on, cold)
    # the evidence that the path ran: on the slow tile the two warm loops differ in their last bits (and both differ from the cold loop)
    sl = slice(0, 64)
    assert not (np.array_equal(on[0][sl], off[0][sl]) and np.array_equal(on[1][:, sl], off[1][:, sl])), "the Newton-only loop did not run on the slow tile"
    assert not (np.array_equal(off[0][sl], cold[0][sl]) and np.array_equal(off[1][:, sl], cold[1][:, sl]))


def test_forward_value_and_repeat_are_bit_identical(case):
    gb, on = case["gb"], case["on"]
    fwd = _eval(gb, case["obs"], case["el"], grad=False)
    assert np.array_equal(fwd[0], on[0], equal_nan=True), "forward-only and gradient launches of the Newton-only loop disagree"
    assert _same_bits(_eval(gb, case["obs"], case["el"]), on), "run-to-run determinism"


def test_invalid_walkers_and_their_tile_mates(case):
    on = case["on"]
    bad = list(INVALID)
    assert np.isneginf(on[0][bad]).all() and np.all(on[1][:, bad] == 0.0)
    assert np.isfinite(on[0]).sum() == W - len(bad)
    mates = np.setdiff1d(np.arange(128, W), bad)
    _cmp_oracle("tile-mates of the invalid walkers", on[0][mates], on[1][:, mates], None, case["ll_o"][mates], case["g_o"][:, mates], None, ll_rtol=1e-10, g_rtol=1e-8)


def test_an_uneven_table_keeps_the_warm_loop_it_had(case):
    """ONE step doubled: the table is not evenly sampled, the Newton-only loop is not taken, and the knob changes nothing."""
    gb = case["gb"]
    t = case["t"].copy(); t[333:] += 1.0
    obs = _table(t, np.random.default_rng(92))
    on = _eval(gb, obs, case["el"]); off = _eval(gb, obs, case["el"], newton=False)
    assert _same_bits(on, off)
    assert not _same_bits(on, _eval(gb, obs, case["el"], warm=False)), "the uneven table must still take the warm loop"


def test_partial_last_tile(case, oracle):
    el = case["el"][:, 58:128]      # W = 70: six slow walkers, the drawn tile with its fast eccentric walker
    on = _eval(case["gb"], case["obs"], el)
    ll_o, g_o, _ = oracle.oracle_eval(case["obs"], PLANETS, el, None, grad=True, active=ACT)
    _cmp_oracle("W = 70", on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    assert not _same_bits(on, _eval(case["gb"], case["obs"], el, newton=False))


def test_newton_chain_does_not_drift(oracle):
    """2 500 daily rows, 64 slow low-e walkers that never fall back: the bar of test_warm_start.test_warm_chain_does_not_drift_over_a_long_chunk
    (1e-11 on ll, 1e-9 on the gradient against the cold loop; the oracle at the default bars) over the longest chains the Newton-only loop
    walks — it is only taken within WARM_RESTART rows per wave, the planner's own chunks."""
    gb = _gpu()
    rng = np.random.default_rng(93)
    n = 2500
    obs = _table(50000.0 + 1.0 * np.arange(n), rng)
    el = synth.draw_walkers(rng, 64, 3.0, 100.0)
    el[1] = rng.uniform(0.0, 0.4, 64)
    on = _eval(gb, obs, el); off = _eval(gb, obs, el, newton=False); cold = _eval(gb, obs, el, warm=False)
    assert not _same_bits(on, off)
    _close("long table, newton vs cold", on, cold, ll_tol=1e-11, g_tol=1e-9)
    _close("long table, newton vs warm", on, off, ll_tol=1e-11, g_tol=1e-9)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    _cmp_oracle("long table", on[0], on[1], None, ll_o, g_o, None)


def test_newton_rows_with_correlated_errors(case, oracle):
    """the same epochs and walkers with a correlation column: k_main<1, ·, false, RADEC|COR>"""
    gb = case["gb"]
    obs = _table(case["t"], np.random.default_rng(94), cor=True)
    on = _eval(gb, obs, case["el"]); off = _eval(gb, obs, case["el"], newton=False)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, case["el"], None, grad=True, active=ACT)
    _cmp_oracle("cor", on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close("cor, newton vs warm", on, off)
    assert not (np.array_equal(on[0][:64], off[0][:64]) and np.array_equal(on[1][:, :64], off[1][:, :64]))
    assert np.array_equal(_eval(gb, obs, case["el"], grad=False)[0], on[0], equal_nan=True)
