"""
The cases of the OFTI rejection sampler's tests (tests/test_ofti_draws_reference.py on the CPU, tests/test_ofti_draws.py on the device) and the
conditions a case has to meet ON THE RESTATEMENT ALONE before a device comparison uses it. A plain module, not a conftest and not a test module.
Every restated run is made once a session (lru_cache) and shared; nobody writes into it.

The tables are the two of tests/golden/ofti.json: ofti_example (8 rows, no cor, σ_ABFG = 1000) and ofti_cor_37 (37 rows with cor, σ_ABFG = 300).
The priors are the example's (examples/ofti_rejection_sampling.jl:67-82) with the parallax prior narrowed: τ ~ Uniform(0, 1) at t_ref = 50000 (tp_mode 1),
and a second set with tp ~ Uniform(40000, 50000) (tp_mode 0). N = 2¹⁹ + 37 draws from first = 2²⁰ + 3: two chunk boundaries, a partial last block.
"""
import functools
import json
import math
from pathlib import Path

import numpy as np

import hmc_reference as ref
import ofti_draws_reference as oref

GOLDEN = Path(__file__).resolve().parent / "golden" / "ofti.json"
TABLES = ("ofti_example", "ofti_cor_37")
SEEDS = (41, 42)
FIRST = (1 << 20) + 3
N = (1 << 19) + 37
T_REF = 50000.0
PRIORS_TAU = [ref.prior(ref.UNIFORM, 0.0, 0.95), ref.prior(ref.LOGUNIFORM, 2.0, 100.0), ref.prior(ref.UNIFORM, 0.0, 1.0),
              ref.prior(ref.TRUNCNORMAL, 1.2, 0.1, lo=0.1), ref.prior(ref.TRUNCNORMAL, 50.0, 0.02, lo=0.1)]
PRIORS_TP = PRIORS_TAU[:2] + [ref.prior(ref.UNIFORM, 40000.0, 50000.0)] + PRIORS_TAU[3:]
# (table, seed, tp_mode): both tables and both seeds in mode 1; mode 0 once
CASES = [(t, s, 1) for t in TABLES for s in SEEDS] + [("ofti_example", 41, 0)]
# the conditions
LEAST_ACCEPTED = 200
COND_BAR = 1e6
# every ℓ = −Inf: uncertainties so small that the weights 1/σ² overflow — the table rejects every draw, whatever the priors
PRIORS_NONE = [ref.prior(ref.UNIFORM, 0.999, 0.9999), ref.prior(ref.LOGUNIFORM, 1e-3, 2e-3)] + PRIORS_TAU[2:]
NONE_N = 1000


@functools.lru_cache(maxsize=None)
def golden():
    return json.loads(GOLDEN.read_text())


def k_yr():
    return golden()["consts"]["kepler_year_to_julian_day"]


def table(name):
    case = next(c for c in golden()["cases"] if c["name"] == name)
    return dict(epochs=np.asarray(case["epochs"]), ra=np.asarray(case["ra"]), dec=np.asarray(case["dec"]), s_ra=np.asarray(case["s_ra"]),
                s_dec=np.asarray(case["s_dec"]), cor=None if case["cor"] is None else np.asarray(case["cor"]), sigma_abfg=float(case["sigma_abfg"]))


def rejecting_table():
    t = table("ofti_example")
    t["s_ra"] = np.full_like(t["s_ra"], 1e-160)
    t["s_dec"] = np.full_like(t["s_dec"], 1e-160)
    return t


def columns(tab):
    """the table in the order of octo_draws_ofti_set / OftiLinearSolver"""
    return [tab[k] for k in ("epochs", "ra", "dec", "s_ra", "s_dec", "cor")] + [tab["sigma_abfg"]]


def priors_of(tp_mode):
    return PRIORS_TAU if tp_mode else PRIORS_TP


@functools.lru_cache(maxsize=None)
def restated(name, seed, tp_mode):
    """the restated driver on a case; read-only"""
    r = oref.rejection(table(name), priors_of(tp_mode), seed, FIRST, N, tp_mode, T_REF, k_yr())
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def check_conditions(r):
    """the conditions of a case, on the restatement alone"""
    assert r["n_accepted"] >= LEAST_ACCEPTED, r["n_accepted"]
    assert r["undecided"] == 0, r["undecided"]
    assert float(np.max(r["cond"])) <= COND_BAR, float(np.max(r["cond"]))
    assert r["n_face_on"] == 0, r["n_face_on"]
    assert math.isfinite(r["max_logml"])
