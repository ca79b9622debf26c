"""
Exactly even tables in k_main's Newton-only warm loop (octo_kernels.h: the loop behind warm_newton_init; octo_api.hip: Task::dm_exact). Where every epoch difference of
a table is exact and has the same bit pattern, the loop forms ΔM = dm·(1/P) once per wave instead of once per row (part A: no output bit moves), and sums
Σ Mb·(t − tp) — the sum ∂/∂P is derived from — by prefix, without t − tp in the row (part B: only the outputs that read that sum move, in their last digits).
OCTO_WARM_EVEN=0 at context creation gives the loop every evenly sampled task has, OCTO_WARM_EVEN=1 part A alone, from the same library.

Which outputs read the sum (octo_kernels.h: planet_finish): Pb = −2π/P²·GT feeds ∂/∂a and ∂/∂M_tot — rows 0 and 6 of the element gradient. ∂/∂tp itself is
−2π/P·Σ Mb: it does NOT read the sum and stays bit for bit, with ll and the other rows.

Walkers and tables are those of tests/test_warm_newton_unroll.py: 192 walkers in three tiles (all-Newton; the a = 1 AU, e = 0.93 walker that forces middle, fourth-order
and cold rows; an invalid and a NaN walker) and their 70-walker slice, on tables of 696 … 703 epochs, so that every remainder mod 4 and a chunk shorter than four rows occur
(asserted on the host as that file does; a chunk of at most four rows keeps the rows every evenly sampled task has: tests/even_sum_model.py).
"""
import numpy as np
import pytest

from test_gpu_parity import _cmp_oracle, _gpu
from test_warm_newton import ACT, INVALID, PLANETS, _eval, _table
from test_warm_newton_unroll import LENGTHS, _case_walkers, _chunks, test_the_partition_meets_the_conditions_on_the_inputs as _partition_conditions
from test_warm_start import _close, _same_bits

TWO_PI = 2.0 * np.pi
READS_GT = [0, 6]                        # ∂/∂a, ∂/∂M_tot (through ∂/∂P)
NOT_GT = [1, 2, 3, 4, 5, 7, 8]           # e, i, ω, Ω, tp, plx, mass
EVEN_OFF = {"OCTO_WARM_EVEN": "0"}
EVEN_A = {"OCTO_WARM_EVEN": "1"}


# ---------------------------------------------------------------------------------------------------------------- the flag, restated (octo_api.hip)
def _dm_exact(t):
    """Task::dm_exact of a table with epochs t: 2π·(t₁ − t₀) where every difference t_j − t_{j−1} is exact (TwoSum's error term is zero), positive and the same bit pattern
    — and with it every 2π·(t_j − t_{j−1}) — and the table is evenly sampled at all (dm_uniform); else 0."""
    t = np.asarray(t, dtype=np.float64)
    if t.size < 2 or not _dm_uniform(t):
        return 0.0
    a, b = t[1:], t[:-1]
    h = a - b
    bb = h - a
    err = (a - (h - bb)) + (-b - bb)
    dm = TWO_PI * h
    same = np.all(h.view(np.int64) == h.view(np.int64)[0]) and np.all(dm.view(np.int64) == dm.view(np.int64)[0])
    return float(dm[0]) if (np.all(np.isfinite(dm)) and np.all(h > 0.0) and np.all(err == 0.0) and same) else 0.0


def _dm_uniform(t):
    """Task::dm_uniform != 0: every step of the table within 1e-7 relative of every other"""
    s = np.abs(TWO_PI * np.diff(np.asarray(t, dtype=np.float64)))
    return bool(s.size > 0 and np.all(np.isfinite(s)) and s.min() > 0.0 and s.max() - s.min() <= 1.0e-7 * s.max())


def _thirds(n):
    return 50000.0 + np.arange(n) / 3.0


def _one_ulp(n):
    t = 50000.0 + 1.0 * np.arange(n)
    t[n // 2] = np.nextafter(t[n // 2], np.inf)
    return t


def test_the_flag():
    """host only"""
    j = np.arange(700)
    for t in (50000.0 + 1.0 * j, 50000.0 + 0.5 * j, 50000.0 + j * 2.0 ** -3, j * 2.0 ** -3):
        assert _dm_exact(t) == TWO_PI * (t[1] - t[0]) != 0.0
    # even to 1e-16, steps not bit-equal: asserted first
    t = _thirds(700)
    steps = np.diff(t)
    assert len(set(steps.view(np.int64).tolist())) > 1 and np.ptp(steps) <= 1e-10 * steps.max()
    assert _dm_uniform(t) and _dm_exact(t) == 0.0
    t = _one_ulp(700)
    assert _dm_uniform(t) and _dm_exact(t) == 0.0
    t = 50000.0 + 1.0 * j; t[333:] += 1.0      # one gap
    assert not _dm_uniform(t) and _dm_exact(t) == 0.0
    assert _dm_exact(np.array([50000.0])) == 0.0


def test_the_partition_meets_the_conditions_on_the_inputs():
    """host only: every remainder mod 4, a chunk shorter than four rows, the fast walker's periastron on every phase (test_warm_newton_unroll's conditions),
    and chunks long enough to take the even loop"""
    _partition_conditions()
    lens = {rows for n in LENGTHS for _, rows in _chunks(n)}
    assert max(lens) >= 5 and min(lens) <= 4, lens


# ---------------------------------------------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def gb():
    return _gpu()


def _rows_equal(a, b, rows):
    return np.array_equal(a[1][rows], b[1][rows], equal_nan=True)


def _check(gb, oracle, obs, el, name):
    """every bar of the issue on one (table, walkers) pair; returns (even on, even off)"""
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    on = _eval(gb, obs, el)
    off = _eval(gb, obs, el, env=EVEN_OFF)
    a_only = _eval(gb, obs, el, env=EVEN_A)
    nonewton = _eval(gb, obs, el, newton=False)
    cold = _eval(gb, obs, el, warm=False)
    for tag, r in (("even on", on), ("even off", off)):
        _cmp_oracle(f"{name}, {tag}", r[0], r[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
        _close(f"{name}, {tag} vs OCTO_WARM_NEWTON=0", r, nonewton)
        _close(f"{name}, {tag} vs OCTO_WARM=0", r, cold)
    _close(f"{name}, even on vs OCTO_WARM_EVEN=0", on, off)
    # both halves of the statement: ll and every row that does not read the sum stay bit for bit; the rows that read it moved (the path ran)
    assert np.array_equal(on[0], off[0], equal_nan=True), name + ": ll moved"
    assert _rows_equal(on, off, NOT_GT), name + ": a gradient row that does not read the sum moved"
    assert not _rows_equal(on, off, READS_GT), name + ": the even loop's prefix sum did not run"
    # part A alone: every output bit for bit the loop's without it
    assert _same_bits(a_only, off), name + ": the hoisted ΔM moved an output bit"
    for env in (None, EVEN_OFF):
        ref = on if env is None else off
        assert np.array_equal(_eval(gb, obs, el, grad=False, env=env)[0], ref[0], equal_nan=True), name + ": forward-only and gradient launches disagree"
    assert _same_bits(_eval(gb, obs, el), on), name + ": run-to-run determinism"
    return on, off


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_every_remainder_on_a_daily_table(gb, oracle, k):
    n = LENGTHS[k]
    t = 50000.0 + 1.0 * np.arange(n)
    assert _dm_exact(t) != 0.0
    obs = _table(t, np.random.default_rng(391 + k))
    el = _case_walkers(k)
    on, _ = _check(gb, oracle, obs, el, f"n = {n}")
    bad = list(INVALID)
    assert np.isneginf(on[0][bad]).all() and np.all(on[1][:, bad] == 0.0)
    _check(gb, oracle, obs, el[:, 58:128], f"n = {n}, W = 70")


@pytest.mark.gpu
def test_periastron_inside_the_table_and_far_away(gb, oracle):
    """tp a few days from the epochs of the walker's own chunks (the prefix form's worst conditioning) and 1e5 days away (where the term (t_last − tp)·ΣMb carries the sum)"""
    k = 2
    n = LENGTHS[k]
    el = _case_walkers(k)
    rng = np.random.default_rng(491)
    el[5, :32] = 50000.0 + rng.uniform(0.0, n, 32)
    el[5, 32:48] = 50000.0 + 1.0e5 + rng.uniform(0.0, 1.0, 16)
    el[5, 48:64] = 50000.0 - 1.0e5 - rng.uniform(0.0, 1.0, 16)
    _check(gb, oracle, _table(50000.0 + 1.0 * np.arange(n), rng), el, "tp inside and 1e5 days away")


@pytest.mark.gpu
def test_half_day_cadence(gb, oracle):
    k = 5
    t = 50000.0 + 0.5 * np.arange(LENGTHS[k])
    assert _dm_exact(t) == TWO_PI * 0.5
    _check(gb, oracle, _table(t, np.random.default_rng(591)), _case_walkers(k), "h = 0.5")


@pytest.mark.gpu
def test_correlated_errors(gb, oracle):
    """k_main<1, ·, false, RADEC|COR>"""
    k = 3
    _check(gb, oracle, _table(50000.0 + 1.0 * np.arange(LENGTHS[k]), np.random.default_rng(691), cor=True), _case_walkers(k), "cor")


@pytest.mark.gpu
@pytest.mark.parametrize("make", (_thirds, _one_ulp), ids=("thirds", "one_ulp"))
def test_tables_the_flag_keeps_out(gb, make):
    """even to 1e-16 but not exactly: the Newton-only loop as it was, every output bit for bit OCTO_WARM_EVEN=0's — and the loop did run"""
    k = 1
    t = make(LENGTHS[k])
    assert _dm_uniform(t) and _dm_exact(t) == 0.0
    obs = _table(t, np.random.default_rng(791))
    el = _case_walkers(k)
    on = _eval(gb, obs, el)
    assert _same_bits(on, _eval(gb, obs, el, env=EVEN_OFF))
    assert _same_bits(on, _eval(gb, obs, el, env=EVEN_A))
    assert not _same_bits(on, _eval(gb, obs, el, newton=False)), "the table must still take the Newton-only loop"
