"""
k_main's θ-loop (octo_device.h: kepler_warm_theta; octo_kernels.h: the loop behind warm_theta_init): on an exactly even RA/Dec table a wave whose 64 lanes are all slow
— every lane's ΔM/(1 − e) below WARM_THETA_X0, no invalid or NaN lane — extrapolates the whole Kepler step from four recorded steps instead of the analytic predictor
plus the FP32 extrapolation of its miss — in a SORTED launch (octo_tile.h): an unsorted evaluation keeps the Newton-only loop and returns what it returned, byte for
byte (asserted below; tests/test_even_table.py and the other files of the warm loops hold it, unsorted, to the loop it had). OCTO_WARM_THETA=0 at context creation
gives the Newton-only loop every such tile had, and the sort's key as it was, from the same library. The batches here are 130-200 walkers with the sort forced
(OCTO_OPT_TILE_SORT = 1, OCTO_OPT_TILE_MIN_WALKERS = 64); which walkers then share a tile is restated by tests/warm_theta_model.sorted_order, and asserted to be the
same with the loop off wherever a tile's bytes are compared between the two.

The root is unique, so the θ-loop is held to the bars tests/test_even_table.py holds the exactly even loop to (imported through the same helpers: the oracle at
1e-10 / 1e-8, test_warm_start._close at 1e-12 / 1e-10 against the other loops), a tile that does not qualify to EVERY byte of OCTO_WARM_THETA=0's, and the walker-tile
sort's key and price for the loop (octo_tile.h) to a NumPy count.

Which arm a row takes cannot be read from outside the kernel: the exits' cases below put a lane of e = 0.9 and one of e = 0.995 — both slower than X0 — on their
periastra inside the table, one day later per case so that every phase of the four-row trip is met. By the bounds of octo_device.h the e = 0.9 lane's extrapolated
step misses by more than τ(0.9) = 1.4e-8 around periastron (rows leave by the |δ| exits), and the e = 0.995 lane (ΔM = 4e-5: above WARM_E_MAX the bound is
(WARM_TOL/ΔM³)^(1/5) = 110) reaches 1/D = 200: the a-priori test rejects some twenty rows around periastron — cold rows, then four start-up rows, then θ rows again.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import synth
from test_even_table import _dm_exact
from test_gpu_parity import _cmp_oracle, _gpu
import warm_theta_model as wtm
from test_warm_newton import ACT, PLANETS, _table
from test_warm_start import _close, _same_bits

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * np.pi
X0 = 0.012                                # octo_device.h: WARM_THETA_X0
WPB = 4
THETA_OFF = {"OCTO_WARM_THETA": "0"}
W3 = 150                                  # two tiles and a partial one of 22
# table lengths: one task (the kernel with the finish inside: no Newton-only loop at all), then several tasks whose chunks cover every residue mod 4, chunks of at
# most four rows (the history's depth: they keep the Newton-only rows) and chunks just above it
LENGTHS = (5, 75, 85, 133, 151, 700)


def _chunk_lengths(n):
    """rows per wave of the throughput launch on one table of n rows (octo_api.hip: get_tasks; tests/test_warm_newton_unroll._chunks without its conditions)"""
    rows_min = min(32, max(8, n // (32 * WPB)))
    t = max(1, n // (rows_min * WPB))
    chunk = -(-(-(-n // t)) // WPB)
    out = []
    for r0 in range(0, n, chunk * WPB):
        nrows = min(chunk * WPB, n - r0)
        out += [min(chunk, nrows - wv * chunk) for wv in range(WPB) if nrows - wv * chunk > 0]
    return out, t


def _x(el, h=1.0):
    """ΔM/(1 − e) of every walker at a table step of h days"""
    return TWO_PI * h / (synth.K_YR * np.sqrt(el[0] ** 3 / el[6])) / (1.0 - el[1])


def _slow(rng, W):
    """a in [20, 100] AU, e <= 0.5: x <= 4e-4"""
    el = synth.draw_walkers(rng, W, 20.0, 100.0)
    el[1] = rng.uniform(0.0, 0.5, W)
    assert np.all(_x(el) < 0.1 * X0)
    return el


def test_the_tables_meet_the_conditions_on_the_inputs():
    """host only"""
    lens, multi = set(), set()
    for n in LENGTHS:
        ch, t = _chunk_lengths(n)
        assert sum(ch) == n
        if t > 1:
            multi |= set(ch)
        lens |= set(ch)
    assert _chunk_lengths(LENGTHS[0])[1] == 1 and all(_chunk_lengths(n)[1] > 1 for n in LENGTHS[1:])
    long_ = {c for c in multi if c > 4}
    assert {c % 4 for c in long_} == {0, 1, 2, 3}, multi
    assert any(c <= 4 for c in multi) and 5 in multi, multi


@pytest.fixture(scope="module")
def gb():
    return _gpu()


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _eval(gb, obs, elems, grad=True, newton=True, warm=True, env=None, sort=1):
    """test_warm_newton._eval with the walker-tile sort forced (sort = 1) or off (0): the throughput kernels whatever the batch size"""
    capi = gb.pkg.capi
    env = dict(env or {}, OCTO_WARM="1" if warm else "0", OCTO_WARM_NEWTON="1" if newton else "0")
    with _env(**env):
        return gb.gpu_eval(obs, PLANETS, elems, None, grad=grad, small_batch=0, options={capi.OPT_TILE_SORT: sort, capi.OPT_TILE_MIN_WALKERS: 64})


def _tiles(el, h):
    """[(walkers of the tile, every one of them slow)] of the sorted launch; the order is the same with the loop's key off (asserted)"""
    perm = wtm.sorted_order(el, h, synth.K_YR)
    assert np.array_equal(perm, wtm.sorted_order(el, h, synth.K_YR, theta=False)), "these walkers must sort alike with OCTO_WARM_THETA=0"
    sl = wtm.slow(el, h, synth.K_YR)
    return [(perm[i:i + 64], bool(sl[perm[i:i + 64]].all())) for i in range(0, perm.size, 64)]


def _check(gb, oracle, obs, el, name, takes=True, h=1.0, env=None):
    """the bars of test_even_table._check for the θ-loop against the loops it replaces, sorted; takes: the launch has a chunk the loop is for — then every tile whose
    walkers are all slow must have taken it (its bytes differ from OCTO_WARM_THETA=0's) and every other tile must be OCTO_WARM_THETA=0's byte for byte. Returns
    (loop on, loop off, the tiles)."""
    e_on = dict(env or {}); e_off = dict(e_on, **THETA_OFF)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    on = _eval(gb, obs, el, env=e_on)
    off = _eval(gb, obs, el, env=e_off)
    cold = _eval(gb, obs, el, warm=False, env=e_on)
    _cmp_oracle(name + ", theta", on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close(name + ", theta vs OCTO_WARM_THETA=0", on, off)
    _close(name + ", theta vs OCTO_WARM_NEWTON=0", on, _eval(gb, obs, el, newton=False, env=e_on))
    _close(name + ", theta vs OCTO_WARM=0", on, cold)
    assert np.array_equal(_eval(gb, obs, el, grad=False, env=e_on)[0], on[0], equal_nan=True), name + ": forward-only and gradient launches disagree"
    assert _same_bits(_eval(gb, obs, el, env=e_on), on), name + ": run-to-run determinism"
    tiles = _tiles(el, h)
    for k, (sl, slow) in enumerate(tiles):
        same = np.array_equal(on[0][sl], off[0][sl], equal_nan=True) and np.array_equal(on[1][:, sl], off[1][:, sl], equal_nan=True)
        assert same != (takes and slow), (name, k, "the θ-loop did not run" if takes and slow else "a tile that does not qualify moved")
    return on, off, tiles


@pytest.mark.parametrize("n", LENGTHS)
def test_qualifying_tiles(gb, oracle, n):
    rng = np.random.default_rng(1000 + n)
    t = 50000.0 + 1.0 * np.arange(n)
    assert _dm_exact(t) != 0.0
    ch, tasks = _chunk_lengths(n)
    takes = tasks > 1 and max(ch) > 4      # a launch of several tasks with a chunk longer than the history
    _, _, tiles = _check(gb, oracle, _table(t, rng), _slow(rng, W3), f"n = {n}", takes=takes)
    assert [q for _, q in tiles] == [True, True, True]


def test_correlated_errors_and_a_half_day_cadence(gb, oracle):
    rng = np.random.default_rng(1101)
    t = 50000.0 + 0.5 * np.arange(163)
    assert _dm_exact(t) == TWO_PI * 0.5
    _check(gb, oracle, _table(t, rng, cor=True), _slow(rng, W3), "cor, h = 0.5", h=0.5)


def test_an_unsorted_launch_keeps_todays_loop(gb):
    """the same slow walkers as drawn, sort off and the library's default (auto, below its 2 048 walkers): every byte OCTO_WARM_THETA=0's"""
    rng = np.random.default_rng(1108)
    obs = _table(50000.0 + 1.0 * np.arange(163), rng)
    el = _slow(rng, W3)
    assert _same_bits(_eval(gb, obs, el, sort=0), _eval(gb, obs, el, sort=0, env=THETA_OFF))
    assert _same_bits(_eval(gb, obs, el, sort=2), _eval(gb, obs, el, sort=2, env=THETA_OFF))
    assert not _same_bits(_eval(gb, obs, el, sort=1), _eval(gb, obs, el, sort=1, env=THETA_OFF)), "sorted, the θ-loop must run"


def test_a_chunk_past_the_restart_keeps_the_checked_loop(gb):
    """OCTO_CHUNK=300 > WARM_RESTART: no Newton-only loop, no θ-loop — every byte OCTO_WARM_THETA=0's"""
    rng = np.random.default_rng(1102)
    obs = _table(50000.0 + 1.0 * np.arange(700), rng)
    el = _slow(rng, W3)
    env = {"OCTO_CHUNK": "300"}
    assert _same_bits(_eval(gb, obs, el, env=env), _eval(gb, obs, el, env=dict(env, **THETA_OFF)))


def test_a_tile_with_one_fast_lane_keeps_todays_loop(gb, oracle):
    rng = np.random.default_rng(1103)
    obs = _table(50000.0 + 1.0 * np.arange(163), rng)
    el = _slow(rng, W3)
    el[0, 70] = 1.0; el[1, 70] = 0.9; el[5, 70] = 50000.0 + 60.0
    assert _x(el)[70] > X0
    _, _, tiles = _check(gb, oracle, obs, el, "one fast lane")
    # the key puts the fast lane last: its tile, the partial one, keeps today's loop, the two full tiles of slow walkers take the θ-loop
    assert [q for _, q in tiles] == [True, True, False] and 70 in tiles[2][0]


def test_a_nan_eccentricity_keeps_todays_loop(gb, oracle):
    """the tile of the NaN lane: every byte OCTO_WARM_THETA=0's; its other lanes agree with the same batch without the NaN (which takes the θ-loop there) at _close's bars"""
    rng = np.random.default_rng(1104)
    obs = _table(50000.0 + 1.0 * np.arange(163), rng)
    clean = _slow(rng, W3)
    el = clean.copy(); el[1, 20] = np.nan
    on, _, tiles = _check(gb, oracle, obs, el, "NaN e")
    assert [q for _, q in tiles] == [True, True, False] and 20 in tiles[2][0]
    assert np.isneginf(on[0][20]) and np.all(on[1][:, 20] == 0.0)
    ref = _eval(gb, obs, clean)
    keep = np.setdiff1d(np.arange(W3), [20])
    _close("NaN e: the other lanes", tuple(None if x is None else (x[keep] if x.ndim == 1 else x[:, keep]) for x in on),
           tuple(None if x is None else (x[keep] if x.ndim == 1 else x[:, keep]) for x in ref))
    # an invalid e likewise
    el = clean.copy(); el[1, 140] = 1.2
    _, _, tiles = _check(gb, oracle, obs, el, "e = 1.2")
    assert [q for _, q in tiles] == [True, True, False] and 140 in tiles[2][0]


@pytest.mark.parametrize("k", range(4))
def test_exits_from_the_theta_row_on_every_phase(gb, oracle, k):
    """lanes of e = 0.9 (a = 8 AU) and e = 0.995 (ΔM = 4e-5), both below X0, with their periastra on table day 40 + k and 100 + k: rows that leave by the |δ| exits, cold rows
    (the a-priori test rejects the e = 0.995 lane where 1/D > 110), start-up rows, θ rows again — on every phase over the four cases"""
    rng = np.random.default_rng(1105)
    n = 163
    obs = _table(50000.0 + 1.0 * np.arange(n), rng)
    el = _slow(rng, W3)
    el[0, 10] = 8.0; el[1, 10] = 0.9; el[5, 10] = 50000.0 + 40.0 + k
    el[0, 80] = ((TWO_PI / 4.0e-5 / synth.K_YR) ** 2 * el[6, 80]) ** (1.0 / 3.0); el[1, 80] = 0.995; el[5, 80] = 50000.0 + 100.0 + k
    x = _x(el)
    assert x.max() < X0 and x[10] > 0.5 * X0 and x[80] > 0.5 * X0
    assert 1.0 / (1.0 - el[1, 80]) > 1.5 * (1.0e-3 / 4.0e-5 ** 3) ** 0.2      # the periastron lies well beyond the a-priori bound
    # (the key may place these two lanes differently with the loop off; every tile qualifies, so no tile's bytes are compared with OCTO_WARM_THETA=0's and the
    # three tiles are checked as a whole)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    on = _eval(gb, obs, el); off = _eval(gb, obs, el, env=THETA_OFF); cold = _eval(gb, obs, el, warm=False)
    _cmp_oracle(f"exits, k = {k}", on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close(f"exits, k = {k}, theta vs OCTO_WARM_THETA=0", on, off)
    _close(f"exits, k = {k}, theta vs OCTO_WARM=0", on, cold)
    assert np.array_equal(_eval(gb, obs, el, grad=False)[0], on[0], equal_nan=True)
    assert not _same_bits(on, off), "the θ-loop did not run"


def test_theta_chain_does_not_drift_over_a_long_chunk(gb, oracle):
    """test_warm_start.test_warm_chain_does_not_drift_over_a_long_chunk's bar (1e-11, 1e-9 against the cold loop) on the longest chains the loop walks: OCTO_CHUNK=256"""
    rng = np.random.default_rng(1106)
    obs = _table(50000.0 + 1.0 * np.arange(2500), rng)
    el = _slow(rng, 64)
    env = {"OCTO_CHUNK": "256"}
    on = _eval(gb, obs, el, env=env); off = _eval(gb, obs, el, env=dict(env, **THETA_OFF)); cold = _eval(gb, obs, el, warm=False, env=env)
    assert not _same_bits(on, off), "the θ-loop did not run"
    _close("long chunk, theta vs cold", on, cold, ll_tol=1e-11, g_tol=1e-9)
    _close("long chunk, theta vs OCTO_WARM_THETA=0", on, off, ll_tol=1e-11, g_tol=1e-9)
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    _cmp_oracle("long chunk", on[0], on[1], None, ll_o, g_o, None)


# ---------------------------------------------------------------------------------------------------------------- the sort: key, count, price
def _tile_theta(g):
    f = g.lib.octo_debug_tile_theta
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    a, b = C.c_int64(), C.c_int64()
    assert f(g.ctx, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _count_tiles(slow, seg=1024):
    """tiles all of whose walkers are slow, as given and with every segment's slow walkers first (what the key does where the others are clearly fast)"""
    given = sorted_ = 0
    for s0 in range(0, slow.size, seg):
        s = slow[s0:s0 + seg]
        given += sum(bool(s[i:i + 64].all()) for i in range(0, s.size, 64))
        ns = int(s.sum())
        sorted_ += ns // 64 + (1 if (ns == s.size and ns % 64) else 0)
    return given, sorted_


def test_sort_forced_off_and_auto(gb, oracle):
    """2 048 + 70 walkers, slow (x < X0/10) and fast (ΔM in [0.02, 0.028], e in [0.3, 0.5]: x > 2 X0, no veto, no lane ever fails the a-priori test, so the θ-loop's
    term is the whole price) alternating: no tile qualifies as drawn, 16 of 34 sorted. 100 000 half-day rows, so that the probe's price (16 tiles x 1e5 rows x
    TILE_THETA_ROW_US / 1 024 SIMDs) clears the launch with room; OCTO_CHUNK=250 keeps the waves' chunks within WARM_RESTART, where the planner's own would be longer
    for so few tiles and the launch would take the checked warm loop. Every walker's numbers at its own column (the oracle on a sample of columns), the probe's counts, and auto on /
    off for the batch as drawn / already ordered."""
    pkg = gb.pkg
    capi = pkg.capi
    rng = np.random.default_rng(1107)
    W, n = 2048 + 70, 100_000
    t = 50000.0 + 0.5 * np.arange(n)
    assert _dm_exact(t) != 0.0
    obs = _table(t, rng)
    el = _slow(rng, W)
    fast = np.arange(W) % 2 == 1
    p_d = np.pi / rng.uniform(0.02, 0.028, int(fast.sum()))      # ΔM = 2π·0.5/P
    el[0, fast] = ((p_d / synth.K_YR) ** 2 * el[6, fast]) ** (1.0 / 3.0); el[1, fast] = rng.uniform(0.3, 0.5, int(fast.sum()))
    el[5, fast] = 50000.0 + rng.uniform(0.0, 1.0, int(fast.sum())) * p_d
    x = _x(el, 0.5)
    assert np.all(x[fast] > 2.0 * X0) and np.all(x[~fast] < 0.1 * X0) and np.all(TWO_PI * 0.5 / (synth.K_YR * np.sqrt(el[0] ** 3 / el[6])) < 0.03)
    cols = np.unique(np.concatenate([[0, 1, 63, 64, 1023, 1024, 2047, 2048, W - 1], rng.choice(W, 8, replace=False)]))
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el[:, cols], None, grad=True, active=ACT)
    res = {}
    for mode in (1, 0, 2):
        with _env(OCTO_CHUNK="250"), gb.GpuPath(obs, PLANETS, small_batch=0, options={capi.OPT_TILE_SORT: mode, capi.OPT_TILE_MIN_WALKERS: 2048}) as g:
            res[mode] = g.eval(el, None, grad=True)
            state = g.tile_state()
            if mode == 2:
                assert state[2] and state[0] == 1, ("auto must turn the sort on for this batch", state)
                assert _tile_theta(g) == _count_tiles(~fast)
        _cmp_oracle(f"sort mode {mode}", res[mode][0][cols], res[mode][1][:, cols], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close("sorted vs as drawn", res[1], res[0])
    assert _same_bits(res[2], res[1]), "auto, once on, is the forced sort"
    assert not _same_bits(res[1], res[0]), "sorted tiles must take the θ-loop"
    # the same walkers already in order: nothing for the sort to gain
    order = np.concatenate([np.flatnonzero(~fast), np.flatnonzero(fast)])
    with _env(OCTO_CHUNK="250"), gb.GpuPath(obs, PLANETS, small_batch=0, options={capi.OPT_TILE_SORT: 2, capi.OPT_TILE_MIN_WALKERS: 2048}) as g:
        g.eval(el[:, order], None, grad=True)
        state = g.tile_state()
        given, sorted_ = _tile_theta(g)
    assert not state[2] and state[0] == 0, state
    assert given == _count_tiles((~fast)[order])[0] and sorted_ <= given + 1
