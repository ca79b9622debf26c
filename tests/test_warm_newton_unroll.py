"""
The Newton-only warm loop of k_main walks FOUR rows per trip, one per phase of a four-slot history ring (octo_device.h: kepler_warm_newton<., PH>;
octo_kernels.h: the loop behind `warm_newton_init`), and takes a chunk's remainder at the front: a wave whose chunk has n rows leaves the first
skip = (4 − n mod 4) mod 4 slots of its first trip empty, so row i of the chunk falls on phase (i + skip) mod 4. What can go wrong is the remainder, a chunk
shorter than one trip, and a row that leaves the Newton-only arm (middle, fourth-order, cold: the cold arm clears the history) on each of the four phases.

The cases are eight consecutive table lengths, 696 … 703 daily RA/Dec epochs, with the walkers of tests/test_warm_newton.py (192 in three tiles: all-Newton;
one a = 1 AU, e = 0.93 walker that forces middle, fourth-order and cold rows on its whole wave around periastron; an invalid and a NaN walker) and their
70-walker slice. The fast walker's periastron moves by one day per case. The planner's partition of these tables is restated below (octo_api.hip: get_tasks) and
the conditions on it are asserted on the host before the device is asked:
  - the waves' chunk lengths cover every residue mod 4;
  - a chunk shorter than four rows occurs;
  - the fast walker's periastron row falls on each of the four phases in some case.
Every case is held to the bars of tests/test_warm_newton.py: the oracle at 1e-10 on ll and 1e-8 on the gradient; test_warm_start._close (1e-12, 1e-10)
against OCTO_WARM_NEWTON=0 and OCTO_WARM=0; the forward launch's value and a repeat bitwise equal; OCTO_WARM_NEWTON_MID=0 runs and meets the same bars.
"""
import numpy as np
import pytest

import synth
from test_gpu_parity import _cmp_oracle, _gpu
from test_warm_newton import ACT, INVALID, N, PLANETS, _eval, _table, _walkers
from test_warm_start import _close, _same_bits

LENGTHS = tuple(range(696, 704))
WPB = 4            # waves per block of the four-wave kernels (octo_kernels.h)
FAST = 100         # the a = 1 AU, e = 0.93 walker (test_warm_newton._walkers)
TP0 = 150.0        # its periastron, days after the first epoch, in the first case; + 1 day per case
MID_OFF = {"OCTO_WARM_NEWTON_MID": "0"}


def _chunks(n):
    """[(first row, rows)] of every wave of the throughput launch on ONE table of n rows, as get_tasks cuts it for a target of `key` tasks:
    rows_min = min(32, max(8, n // (32·WPB))) where the table has fewer than 32 tasks of 32·WPB rows, t = min(key, n // (rows_min·WPB)) tasks,
    chunk = ceil(ceil(n / t) / WPB) rows per wave, tasks of WPB·chunk rows, the last one short. plan_key's target for at most three walker tiles is
    at least 256 // 3 = 85 on any device (its capacity floor), and n // (rows_min·WPB) = 21 here: the partition does not depend on the device."""
    assert n // (32 * WPB) < 32
    rows_min = min(32, max(8, n // (32 * WPB)))
    t = max(1, n // (rows_min * WPB))
    assert t <= 85
    chunk = -(-(-(-n // t)) // WPB)
    span = chunk * WPB
    out = []
    for r0 in range(0, n, span):
        nrows = min(span, n - r0)
        for wv in range(WPB):
            lo = min(wv * chunk, nrows); hi = min(lo + chunk, nrows)
            if hi > lo:
                out.append((r0 + lo, hi - lo))
    assert sum(c for _, c in out) == n and len({r0 // span for r0, _ in out}) > 1      # (more than one task: not the one-task kernel with the finish inside)
    return out


def _phase(n, row):
    """the phase of the trip that table row `row` falls on"""
    for first, rows in _chunks(n):
        if first <= row < first + rows:
            return (row - first + (4 - rows % 4) % 4) % 4
    raise AssertionError(row)


def _case_walkers(k):
    """test_warm_newton's walkers (its seed, drawn behind its table), the fast walker's periastron moved to day TP0 + k"""
    rng = np.random.default_rng(91)
    _table(50000.0 + 1.0 * np.arange(N), rng)
    el = _walkers(rng)
    el[5, FAST] = 50000.0 + TP0 + k
    return el


def _periastron_rows(el, n):
    period = synth.K_YR * np.sqrt(el[0, FAST] ** 3 / el[6, FAST])
    tp = el[5, FAST] - 50000.0
    return [int(round(tp + j * period)) for j in range(-3, 4) if 0 <= round(tp + j * period) < n]


def test_the_partition_meets_the_conditions_on_the_inputs():
    """host only (no device is asked): what the cases below rely on"""
    lens = {rows for n in LENGTHS for _, rows in _chunks(n)}
    assert {c % 4 for c in lens} == {0, 1, 2, 3}, lens
    assert min(lens) < 4, lens
    phases = set()
    for k, n in enumerate(LENGTHS):
        rows = _periastron_rows(_case_walkers(k), n)
        assert rows, "the fast walker's periastron lies outside the table"
        phases |= {_phase(n, r) for r in rows}
    assert phases == {0, 1, 2, 3}, phases


@pytest.fixture(scope="module")
def gb():
    return _gpu()


def _check(gb, oracle, obs, el, name):
    ll_o, g_o, _ = oracle.oracle_eval(obs, PLANETS, el, None, grad=True, active=ACT)
    on = _eval(gb, obs, el)
    off = _eval(gb, obs, el, newton=False)
    cold = _eval(gb, obs, el, warm=False)
    _cmp_oracle(name, on[0], on[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close(name + ", newton vs warm", on, off)
    _close(name + ", newton vs cold", on, cold)
    assert not _same_bits(on, off), name + ": the Newton-only loop did not run"
    assert np.array_equal(_eval(gb, obs, el, grad=False)[0], on[0], equal_nan=True), name + ": forward-only and gradient launches disagree"
    assert _same_bits(_eval(gb, obs, el), on), name + ": run-to-run determinism"
    nomid = _eval(gb, obs, el, env=MID_OFF)
    _cmp_oracle(name + ", middle arm off", nomid[0], nomid[1], None, ll_o, g_o, None, ll_rtol=1e-10, g_rtol=1e-8)
    _close(name + ", middle arm off vs warm", nomid, off)
    _close(name + ", middle arm off vs cold", nomid, cold)
    return on, off


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_every_remainder_and_every_phase(gb, oracle, k):
    n = LENGTHS[k]
    test_the_partition_meets_the_conditions_on_the_inputs()
    obs = _table(50000.0 + 1.0 * np.arange(n), np.random.default_rng(191 + k))
    el = _case_walkers(k)
    on, off = _check(gb, oracle, obs, el, f"n = {n}")
    # the slow tile took the Newton-only loop (its last bits differ from the warm loop's), and the invalid walkers stay what they are
    assert not (np.array_equal(on[0][:64], off[0][:64]) and np.array_equal(on[1][:, :64], off[1][:, :64])), "the Newton-only loop did not run on the slow tile"
    bad = list(INVALID)
    assert np.isneginf(on[0][bad]).all() and np.all(on[1][:, bad] == 0.0)
    # W = 70: six slow walkers and the drawn tile with its fast walker, a partial last tile
    _check(gb, oracle, obs, el[:, 58:128], f"n = {n}, W = 70")


@pytest.mark.gpu
def test_correlated_errors(gb, oracle):
    """the same with a correlation column: k_main<1, ·, false, RADEC|COR>"""
    k = 3
    n = LENGTHS[k]
    obs = _table(50000.0 + 1.0 * np.arange(n), np.random.default_rng(291), cor=True)
    _check(gb, oracle, obs, _case_walkers(k), f"cor, n = {n}")
