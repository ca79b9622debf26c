"""
The middle arm of k_main's Newton-only warm rows (octo_device.h: kepler_warm_newton): a wave-row that misses τ(e) but whose lanes all start within τ₂(e)
of the root takes ONE Halley step — a series in the Newton δ with the reciprocal already taken — instead of the fourth-order correction. The root is
unique, so the loop must agree with the same library without the arm (OCTO_WARM_NEWTON_MID=0: τ₂ = 0, the parent's arithmetic bit for bit), without the
Newton-only rows (OCTO_WARM_NEWTON=0), with the cold loop (OCTO_WARM=0) and with the oracle, at the bars of tests/test_warm_newton.py, whose dataset,
walkers and helpers these tests take:

  tile 0   slow walkers (a >= 20 AU, e <= 0.5): every warm row Newton-only — the switch changes no bit;
  tile 1   as drawn, plus one walker at a = 1 AU, e = 0.93: middle, fourth-order and cold rows for the whole wave around its periastron;
  tile 2   as drawn, with an invalid walker (e = 1.2) and a NaN element.
"""
import numpy as np
import pytest

import synth
from test_gpu_parity import _cmp_oracle, _gpu
from test_warm_newton import ACT, INVALID, PLANETS, W, _eval, _table, _walkers, N
from test_warm_start import _close, _same_bits

pytestmark = pytest.mark.gpu

OFF = {"OCTO_WARM_NEWTON_MID": "0"}
ON = {"OCTO_WARM_NEWTON_MID": "1"}


def _tile_bits_equal(a, b, sl):
    return np.array_equal(a[0][sl], b[0][sl], equal_nan=True) and np.array_equal(a[1][:, sl], b[1][:, sl], equal_nan=True)


@pytest.fixture(scope="module")
def mid_case(oracle):
    """test_warm_newton's dataset and walkers (the same seed), the oracle's answer and the four device answers the tests below read (computed once)"""
    gb = _gpu()
    rng = np.random.default_rng(91)
    t = 50000.0 + 1.0 * np.arange(N)
    obs = _table(t, rng)
    el = _walkers(rng)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    on = _eval(gb, obs, el, env=ON)
    off = _eval(gb, obs, el, env=OFF)
    warm = _eval(gb, obs, el, newton=False, env=ON)
    cold = _eval(gb, obs, el, warm=False, env=ON)
    return dict(gb=gb, t=t, obs=obs, el=el, ll_o=ll_o, g_o=g_o, on=on, off=off, warm=warm, cold=cold)


def test_middle_arm_against_the_oracle_and_the_three_other_loops(mid_case):
    on = mid_case["on"]
    _cmp_oracle("mid", on[0], on[1], None, mid_case["ll_o"], mid_case["g_o"], None, ll_rtol=1e-10, g_rtol=1e-8)
    _close("mid on vs off", on, mid_case["off"])
    _close("mid vs warm", on, mid_case["warm"])
    _close("mid vs cold", on, mid_case["cold"])


def test_the_arm_runs_where_rows_leave_the_newton_only_arm_and_nowhere_else(mid_case):
    on, off = mid_case["on"], mid_case["off"]
    assert _tile_bits_equal(on, off, slice(0, 64)), "the slow tile has no row beyond τ: the switch must change no bit there"
    assert not _tile_bits_equal(on, off, slice(64, 128)), "the middle arm did not run on the tile of the a = 1 AU, e = 0.93 walker"
    # the default is the arm on
    assert _same_bits(_eval(mid_case["gb"], mid_case["obs"], mid_case["el"]), on)


def test_forward_value_and_repeat_are_bit_identical(mid_case):
    gb, on = mid_case["gb"], mid_case["on"]
    fwd = _eval(gb, mid_case["obs"], mid_case["el"], grad=False, env=ON)
    assert np.array_equal(fwd[0], on[0], equal_nan=True), "forward-only and gradient launches disagree with the middle arm on"
    assert _same_bits(_eval(gb, mid_case["obs"], mid_case["el"], env=ON), on), "run-to-run determinism"


def test_a_tile_that_crosses_all_three_bounds(mid_case, oracle):
    """128 walkers at a = 1.5-3 AU, e = 0.6-0.9 whose periastron passages lie inside the table: around each passage the wave's |δ| climbs through τ, τ₂ and
    WARM_TOL and comes back (tests/warm_newton_mid_model.py on these walkers: every class of wave-row occurs)."""
    gb = mid_case["gb"]
    rng = np.random.default_rng(95)
    el = synth.draw_walkers(rng, 128, 1.5, 3.0)
    el[1] = rng.uniform(0.6, 0.9, 128)
    el[5] = 50000.0 + rng.uniform(50.0, N - 50.0, 128)
    on = _eval(gb, mid_case["obs"], el, env=ON); off = _eval(gb, mid_case["obs"], el, env=OFF)
    ll_o, g_o, _ = oracle.oracle_eval(mid_case["obs"], PLANETS, el, None, grad=True, active=ACT)
    _cmp_oracle("crossing tile", on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close("crossing tile, mid on vs off", on, off)
    _close("crossing tile, mid vs cold", on, _eval(gb, mid_case["obs"], el, warm=False, env=ON))
    assert not _same_bits(on, off), "the middle arm did not run on the crossing tile"


def test_an_uneven_table_keeps_the_warm_loop_it_had(mid_case):
    """ONE step doubled: the Newton-only loop is not taken, and neither of its switches changes a bit."""
    gb = mid_case["gb"]
    t = mid_case["t"].copy(); t[333:] += 1.0
    obs = _table(t, np.random.default_rng(92))
    on = _eval(gb, obs, mid_case["el"], env=ON)
    assert _same_bits(on, _eval(gb, obs, mid_case["el"], env=OFF))
    assert _same_bits(on, _eval(gb, obs, mid_case["el"], newton=False, env=OFF))


def test_invalid_walkers_and_their_tile_mates(mid_case):
    on = mid_case["on"]
    bad = list(INVALID)
    assert np.isneginf(on[0][bad]).all() and np.all(on[1][:, bad] == 0.0)
    assert np.isfinite(on[0]).sum() == W - len(bad)
    mates = np.setdiff1d(np.arange(128, W), bad)
    _cmp_oracle("tile-mates of the invalid walkers", on[0][mates], on[1][:, mates], None, mid_case["ll_o"][mates], mid_case["g_o"][:, mates], None,
                ll_rtol=1e-10, g_rtol=1e-8)
    _close("tile-mates, mid on vs off", tuple(None if x is None else x[..., mates] for x in on), tuple(None if x is None else x[..., mates] for x in mid_case["off"]))


def test_partial_last_tile(mid_case, oracle):
    el = mid_case["el"][:, 58:128]      # W = 70: six slow walkers, the drawn tile with its fast eccentric walker
    on = _eval(mid_case["gb"], mid_case["obs"], el, env=ON); off = _eval(mid_case["gb"], mid_case["obs"], el, env=OFF)
    ll_o, g_o, _ = oracle.oracle_eval(mid_case["obs"], PLANETS, el, None, grad=True, active=ACT)
    _cmp_oracle("W = 70", on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close("W = 70, mid on vs off", on, off)
    assert not _same_bits(on, off)


def test_middle_arm_with_correlated_errors(mid_case, oracle):
    """the same epochs and walkers with a correlation column: k_main<1, ·, false, RADEC|COR>"""
    gb = mid_case["gb"]
    obs = _table(mid_case["t"], np.random.default_rng(94), cor=True)
    on = _eval(gb, obs, mid_case["el"], env=ON); off = _eval(gb, obs, mid_case["el"], env=OFF)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, mid_case["el"], None, grad=True, active=ACT)
    _cmp_oracle("cor", on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close("cor, mid on vs off", on, off)
    assert _tile_bits_equal(on, off, slice(0, 64)) and not _tile_bits_equal(on, off, slice(64, 128))
    assert np.array_equal(_eval(gb, obs, mid_case["el"], grad=False, env=ON)[0], on[0], equal_nan=True)
