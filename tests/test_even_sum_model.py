"""The rounding of k_main's prefix form of Σ_i Mb_i·(t_i − tp) on an exactly even chunk (octo_kernels.h: astrom_row<…, WEVEN = 2>, even_gt_finish) next to the
parent's row-by-row FMA sum, both in float64 (tests/even_sum_model.py) against long double. No GPU.

Inputs: 4 096 lanes x 156 rows (the chunk one wave of the flagship launch walks), h = 1 day; smooth, sign-changing and random Mb; |t₀ − tp| up to 3, 80, 1e3 and 1e5
days (tp inside the chunk for the first two); chunks of 1, 2, 3 and 157 rows; h = 0.5 and 2. Errors are relative to Σ |Mb·dt|.

The bar, on every input set: the error of what the kernel computes (even_sum_model.device_sum) is at most 16 x the parent form's worst error on the same inputs, and
never above 1e-13 (three orders under the device's gradient bar, test_warm_start._close's 1e-10).

The kernel takes the prefix form on chunks of at least five rows (the shortest on which a Newton-only row can occur) and keeps the parent's rows on shorter ones, because
the BARE prefix form does not meet the bar on a chunk of two rows: random Mb, tp between the two epochs, 49 x the parent's error with this seed (9.0e-15 against 1.8e-16)
and up to 420 x over six other seeds, where Mb₀ + Mb₁ cancels and the sum itself is small; 12 x at most at three rows, 7.5 x from four rows on. That figure is kept as a
test of its own below (the reason for the rule), and a chunk of five rows is added to the cases.

Measured (seed 11): worst ratio 4.7 (random Mb, five rows, |t₀ − tp| <= 3; 3.0 on the chunks of 156 and 157 rows); prefix form at most 3.0e-15, parent's form at most
1.7e-15; from |t₀ − tp| ~ 1e3 days on the two agree to within a factor 2."""
import numpy as np
import pytest

import even_sum_model as esm

LANES = 4096
KINDS = ("smooth", "sign", "random")
SPANS = (3.0, 80.0, 1.0e3, 1.0e5)
# (rows, h)
SHAPES = ((156, 1.0), (1, 1.0), (2, 1.0), (3, 1.0), (5, 1.0), (157, 1.0), (156, 0.5), (156, 2.0))


@pytest.fixture(scope="module")
def table():
    """{(kind, span, rows, h): (worst prefix error, worst parent error)}, computed once"""
    out = {}
    rng = np.random.default_rng(11)
    for n, h in SHAPES:
        t = esm.epochs(50000.0 + 4000.0, h, n)
        for kind in KINDS:
            mb = esm.adjoints(kind, LANES, n, rng)
            for span in SPANS:
                tp = t[0] + rng.uniform(-span, span, LANES)
                out[(kind, span, n, h)] = esm.errors(mb, t, tp)
    return out


def test_the_model_fma_is_an_fma():
    """the restated FMA keeps what a separate product would round away"""
    a = np.array([1.0 + 2.0 ** -30]); b = np.array([1.0 - 2.0 ** -30]); c = np.array([-1.0])
    assert esm.fma(a, b, c)[0] == -2.0 ** -60 and (a * b + c)[0] == 0.0


def test_prefix_form_against_the_parents_sum(table):
    worst_ratio, worst_new, worst_par, at = 0.0, 0.0, 0.0, None
    for key, (e_new, e_par) in table.items():
        print(f"{key}: prefix {e_new:.3e}  parent {e_par:.3e}  ratio {e_new / e_par if e_par > 0 else float('nan'):.2f}")
        assert e_new <= 1.0e-13, (key, e_new)
        assert e_new <= 16.0 * e_par, (key, e_new, e_par)
        worst_new = max(worst_new, e_new); worst_par = max(worst_par, e_par)
        if e_par > 0.0 and e_new / e_par > worst_ratio:
            worst_ratio, at = e_new / e_par, key
    print(f"worst ratio {worst_ratio:.2f} at {at}; prefix form at most {worst_new:.3e}, parent's form at most {worst_par:.3e}")


def test_short_chunks_keep_the_parents_rows_and_why():
    """chunks below MIN_ROWS: the kernel's sum IS the parent's; the bare prefix form on two rows misses the 16 x bar (printed), which is why"""
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4):
        t = esm.epochs(54000.0, 1.0, n)
        mb = esm.adjoints("random", LANES, n, rng)
        tp = t[0] + rng.uniform(-3.0, 3.0, LANES)
        assert n < esm.MIN_ROWS and np.array_equal(esm.device_sum(mb, t, tp), esm.parent_sum(mb, t, tp))
        e_bare, e_par = esm.errors(mb, t, tp, form=esm.prefix_sum)
        print(f"{n} rows, bare prefix form {e_bare:.3e}, parent {e_par:.3e}, ratio {e_bare / e_par:.1f}")
        assert e_bare <= 1.0e-13      # (even there three orders under the device bar: the rule is about the ratio)
    assert esm.MIN_ROWS == 5


def test_a_chunk_of_one_row_is_the_rows_own_product(table):
    """h = 0 there: (t − tp)·Mb, what fma(Mb, t − tp, 0) gives — bit for bit"""
    rng = np.random.default_rng(12)
    t = esm.epochs(54000.0, 1.0, 1)
    mb = esm.adjoints("random", LANES, 1, rng)
    tp = t[0] + rng.uniform(-80.0, 80.0, LANES)
    assert np.array_equal(esm.prefix_sum(mb, t, tp), esm.parent_sum(mb, t, tp))


def test_far_periastron_the_two_forms_agree(table):
    """from |t₀ − tp| ~ 1e3 days the term (t_last − tp)·GM carries the sum and the two forms have the same error to a small factor"""
    for (kind, span, n, h), (e_new, e_par) in table.items():
        if span >= 1.0e3 and n >= 156:
            assert e_new <= 3.0 * e_par + 2.3e-16, (kind, span, n, h, e_new, e_par)
