"""
The device-side helpers the GPU suites of liboctofitter_hip_draws.so share (tests/test_prior_draws.py, test_hmc.py, test_lbfgs.py,
test_pathfinder.py, test_adapt.py, test_nuts.py): the loaded binding as a fixture, the test model through the mirror, padded device views
and the comparisons of outputs. A plain module, not a conftest and not a test module; a test module imports what it uses by name, the
fixture included (a module-scoped fixture is instantiated once per importing module). The inputs and bars are in tests/draws_cases.py.
"""
import math

import numpy as np
import pytest

import draws_cases as cases
import hmc_reference as ref

TRANS_BAR = 1e-11      # the project's device-transcendental bar, relative to max(1, |ref|)


@pytest.fixture(scope="module")
def draws_mod(pkg):
    from octofitter_jl_amd.host import draws
    draws.load_library()
    return draws


# ---------------------------------------------------------------------------------------------------- models
def mirror_priors(pkg, priors):
    """host/priors.py priors of the restatement's dicts"""
    out = []
    for p in priors:
        k = p["kind"]
        out.append(pkg.Uniform(p["p0"], p["p1"]) if k == ref.UNIFORM else pkg.LogUniform(p["p0"], p["p1"]) if k == ref.LOGUNIFORM
                   else pkg.Normal(p["p0"], p["p1"]) if k == ref.NORMAL else pkg.Sine() if k == ref.SINE
                   else pkg.truncated(pkg.Normal(p["p0"], p["p1"]), lower=None if p["lo"] == -math.inf else p["lo"], upper=None if p["hi"] == math.inf else p["hi"]))
    return out


def hmc_model(pkg, e_prior=None, tables=None):
    """The test model through the mirror (tables: cases.model_tables() unless given); its priors and sources are the ones
    cases.oracle_model hands the oracle."""
    astrom_t, rv_t = tables or cases.model_tables()
    astrom = pkg.PlanetRelAstromObs(astrom_t, name="sim")
    rv = pkg.StarAbsoluteRVObs(rv_t, name="rv", variables=pkg.variables(offset=pkg.Normal(0, 20), jitter=pkg.LogUniform(0.1, 20.0)))
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom],
                   variables=pkg.variables(a=pkg.LogUniform(5, 20), e=e_prior or pkg.Uniform(0.0, 0.6), i=pkg.Sine(), ω=pkg.UniformCircular(),
                                           Ω=pkg.UniformCircular(), θ=pkg.UniformCircular(), tp=pkg.θ_at_epoch_to_tperi("θ", 50000),
                                           mass=pkg.LogUniform(1.0, 50.0)))
    sys_ = pkg.System(name="sim", companions=[b], observations=[rv],
                      variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.05), lower=0.1), plx=pkg.truncated(pkg.Normal(50.0, 0.1), lower=0.1)))
    model = pkg.LogDensityModel(sys_)
    assert model.names == cases.MODEL_NAMES, model.names
    if e_prior is None:
        for k, p in enumerate(cases.MODEL_PRIORS):
            c = model._c_priors[k]
            lo, hi = ref.support(p) if p["kind"] != ref.NORMAL else (-math.inf, math.inf)
            assert (c.kind, c.p0, c.p1) == (p["kind"], p["p0"], p["p1"]) and (p["kind"] != ref.TRUNCNORMAL or (c.lo, c.hi) == (lo, hi)), (k, p)
    assert [tuple(t) for t in model._esrc] == cases.MODEL_ESRC and [tuple(t) for t in model._nsrc] == cases.MODEL_NSRC, (model._esrc, model._nsrc)
    return model


def tight_model(pkg):
    """The test model on the tight tables of the L-BFGS and Pathfinder suites."""
    return hmc_model(pkg, tables=cases.tight_tables())


def set_batch_invariant(pkg, model, on=1):
    fn = model.ln_like
    fn._check(fn.lib.octo_ctx_set_option(fn._ctx, pkg.capi.OPT_BATCH_INVARIANT, on), "octo_ctx_set_option")


# ---------------------------------------------------------------------------------------------------- device arrays
def dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda") if dtype is None else torch.as_tensor(np.ascontiguousarray(x), device="cuda", dtype=dtype)


def padded(torch, x, ld):
    """(buffer, view): a view with leading dimension ld of a NaN-filled buffer holding x, an array or a tensor (the chain index last)."""
    buf = torch.full(tuple(x.shape[:-1]) + (ld,), float("nan"), dtype=torch.float64, device="cuda")
    buf[..., :x.shape[-1]] = torch.as_tensor(x, device="cuda")
    return buf, buf[..., :x.shape[-1]]


def padded_view(x, extra=5, fill=float("nan")):
    """A [K, W] view with leading dimension W + extra of a buffer filled with `fill` beyond column W."""
    import torch
    x = dev(x)
    buf = torch.full((x.shape[0], x.shape[1] + extra), fill, dtype=torch.float64, device="cuda")
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]]


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


def host_outputs(r, tt):
    """θ_t and every output a call returned, by name, on the host"""
    return dict(theta_t=tt.cpu().numpy(), **{k: v.cpu().numpy() for k, v in r.items() if v is not None})


# ---------------------------------------------------------------------------------------------------- comparisons
def same_bits(x, y):
    """two lists of arrays, entry by entry, NaN equal to NaN (None equal to None)"""
    return all((a is None and b is None) or np.array_equal(a, b, equal_nan=True) for a, b in zip(x, y))


def differing(a, b, keys, cols=slice(None)):
    """the keys under which two dicts of arrays do not hold the same bits in the columns cols"""
    return [k for k in keys if not np.array_equal(a[k][..., cols], b[k][..., cols], equal_nan=True)]


def rel(x, y):
    return np.abs(x - y) / np.maximum(1.0, np.abs(y))


def close(got, want, bar, scale_one=True):
    """|got − want| <= bar·max(1, |want|) (scale_one) or bar·|want|, NaN equal to NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    den = np.maximum(1.0, np.abs(want[ok])) if scale_one else np.abs(want[ok])
    return bool(np.all(np.abs(got[ok] - want[ok]) <= bar * den))
