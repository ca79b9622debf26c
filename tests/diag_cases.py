"""
The inputs of the diagnostics' GPU suite (tests/test_diag.py), shared with tests/test_diag_reference.py — which establishes on the CPU that every
one of them keeps its decision margins — and with tools/diag_bench.py, which records the long-double gaps the bars are written from. Every case is
a pure function of its fixed seed. A plain module, not a test module.
"""
import functools
import itertools

import numpy as np

import diag_reference as ref


def ar1(rng, n, K, W, phi):
    """stationary AR(1) chains of unit variance, [n, K, W]; phi: a number or one value per row"""
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), (K,))[:, None]
    e = rng.standard_normal((n, K, W))
    x = np.empty((n, K, W))
    x[0] = e[0]
    for i in range(1, n):
        x[i] = phi * x[i - 1] + np.sqrt(1.0 - phi * phi) * e[i]
    return x


def _smallest(rng):
    return ar1(rng, 8, 1, 1, 0.0)


def _odd(rng):
    return ar1(rng, 9, 2, 3, 0.0)


def _two_blocks(rng):
    return ar1(rng, 35, 3, 257, (0.0, 0.5, -0.3)) * np.array([1.0, 10.0, 0.1])[:, None] + np.array([0.0, -3.0, 1e3])[:, None]


def _geyer_far(rng):
    return ar1(rng, 400, 2, 64, (0.9, 0.5))


def _global_passes(rng):
    return ar1(rng, 130, 1, 1100, 0.3)


def _widest(rng):
    return ar1(rng, 16, 64, 2, np.linspace(-0.4, 0.6, 64))


def _ties(rng):
    return rng.integers(0, 7, size=(20, 2, 5)).astype(np.float64)


def _signed_zero(rng):
    return rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0]), size=(16, 1, 3))


def _constant_row(rng):
    x = ar1(rng, 12, 3, 4, 0.0)
    x[:, 1] = 2.5
    return x


def _finite_twin(rng):
    return ar1(rng, 12, 4, 4, 0.0)


def _nan_and_inf(rng):
    x = _finite_twin(rng)
    x[3, 1, 2] = np.nan
    x[9, 3, 0] = np.inf
    return x


def _long_chain(rng):
    return ar1(rng, 2082, 2, 3, (0.9995, 0.5))


def _censored(rng):
    x = ar1(rng, 80, 2, 64, (0.0, 0.3))
    x[:, 0] = np.clip(x[:, 0], -0.2, 0.2)
    x[:, 1] = np.minimum(x[:, 1], 1.0)
    return x


def _stuck_chain(rng):
    x = ar1(rng, 24, 2, 5, (0.0, 0.4))
    x[:, 1, 2] = 0.7
    return x


def _edge(rng, n, W):
    return ar1(rng, n, 2, W, (0.0, 0.6))


# The exact edges of the blocks: N on, one below and one above a multiple of the 16-lag window (an odd N drops a middle sample besides), M = 2W of
# exactly one wave (64) and one chain block (256) and two chains more. S = 2048 (N 32, W 32), 4096 (N 16, W 128) and 8192 (N 32, W 128) are powers
# of two: no +Inf behind the keys, and at 4096 the first global pass of the sort with a full last block. (name, seed, (n, W, K)).
EDGES = tuple((f"edge_N{N}_W{W}", 41 + i, (2 * N + N % 2, W, 2))
              for i, (N, W) in enumerate(itertools.product((15, 16, 17, 31, 32, 33), (32, 33, 128, 129))))

# name -> (builder, seed, (n, W, K)). The first six, long_chain and the edges are the shapes on which the kernels can go wrong; the others one case of
# each kind of value.
CASES = {
    "smallest": (_smallest, 11, (8, 1, 1)),
    "odd_n": (_odd, 12, (9, 3, 2)),                       # the middle sample is dropped
    "two_blocks": (_two_blocks, 13, (35, 257, 3)),        # two 256-chain blocks per half, N = 17 across a lag block, S not a power of two
    "geyer_far": (_geyer_far, 14, (400, 64, 2)),          # φ = 0.9: Geyer runs far
    "global_passes": (_global_passes, 15, (130, 1100, 1)),      # S = 143 000: the sort makes 28 global passes
    "widest_K": (_widest, 16, (16, 2, 64)),
    "ties": (_ties, 17, (20, 5, 2)),
    "signed_zero": (_signed_zero, 18, (16, 3, 1)),
    "constant_row": (_constant_row, 19, (12, 4, 3)),
    "nan_and_inf": (_nan_and_inf, 20, (12, 4, 4)),
    "long_chain": (_long_chain, 21, (2082, 3, 2)),        # T = 1056 lags > 1024: ρ_t in the work array; row 0's Geyer loop runs past lag 1024, row 1's stops early
    "stuck_chain": (_stuck_chain, 31, (24, 5, 2)),        # one chain of row 1 never moves: zero variance, N tied ranks, a constant indicator in one lane
    "censored": (_censored, 32, (80, 64, 2)),             # tie runs longer than a sort block, from key 0 and up to key S; q95 = the maximum: ess_tail alone is NaN
    **{name: (functools.partial(_edge, n=shape[0], W=shape[1]), seed, shape) for name, seed, shape in EDGES},
}
# nan_and_inf without its two poisoned entries: what a handle is given after a cube that flagged rows. Not a case of the parametrised tests.
TWINS = {"nan_and_inf_finite": (_finite_twin, 20, (12, 4, 4))}
INVALID_ROWS = {"constant_row": [1], "nan_and_inf": [1, 3]}
STATISTICS = ("rhat", "ess_bulk", "ess_tail", "rhat_basic", "ess_basic")      # the five with a bar; the quantiles are bit for bit
MARGIN_BAR = 1e-6


@functools.lru_cache(maxsize=None)
def draws(name):
    build, seed, (n, W, K) = CASES[name] if name in CASES else TWINS[name]
    x = build(np.random.default_rng(seed))
    assert x.shape == (n, K, W) and x.dtype == np.float64, (name, x.shape)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 restatement of the case, computed once and shared"""
    return ref.diagnose(draws(name))


def gaps(name):
    """statistic -> the largest gap, relative to max(1, |long double|), between the float64 restatement and the same in np.longdouble"""
    lo, hi = reference(name)["stats"], ref.diagnose(draws(name), dtype=np.longdouble)["stats"]
    out = {}
    for s in STATISTICS:
        a, b = lo[getattr(ref, s.upper())].astype(np.longdouble), hi[getattr(ref, s.upper())]
        ok = ~np.isnan(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (name, s)
        out[s] = float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(1, np.abs(b[ok])), initial=0.0))
    return out


# The largest long-double gap of each statistic over CASES, as tools/diag_bench.py measured and profiles/diag_throughput.txt records them
# (tests/test_diag_reference.py holds the two together). The bar of a statistic in tests/test_diag.py is max(TRANS_BAR, 100 × its gap).
LONG_DOUBLE_GAP = {
    "rhat": 1.7474833878483988e-16,
    "ess_bulk": 2.344377615116149e-14,
    "ess_tail": 6.264700271968548e-15,
    "rhat_basic": 6.2313977762518125e-15,
    "ess_basic": 9.51236505730538e-14,
}
