"""
The host side of the Gaussian-process RV observation (host/gp.py, host/observations.py, host/model.py): the traced `gaussian_process` closure, the
nodes it gives the model, and the refusals. The constructors' tests need no GPU; a LogDensityModel opens a device context, so the two tests that build
one are marked gpu.
"""
import numpy as np
import pytest

import gp_reference as gref


def rv_table(n=21, seed=3):
    rng = np.random.default_rng(seed)
    return dict(epoch=np.sort(rng.uniform(55000.0, 55080.0, n)), rv=rng.normal(size=n) * 8.0, σ_rv=rng.uniform(0.5, 3.0, n))


def gp_obs(pkg, closure=None, trend=None, **more):
    V, d = pkg.variables, pkg.derived
    closure = closure or (lambda θ: pkg.Celerite(pkg.SHOTerm(S0=d.exp(θ.log_S0), Q=θ.Q, w0=θ.w0)))
    return pkg.StarAbsoluteRVObs(rv_table(), name="hires", trend_function=trend, gaussian_process=closure,
                                 variables=V(offset=pkg.Normal(0, 10), jitter=pkg.LogUniform(0.1, 2.0), log_S0=pkg.Uniform(0.0, 3.4), Q=pkg.Uniform(0.6, 5.0),
                                             w0=pkg.LogUniform(0.05, 1.0), **more))


def system_of(pkg, observations):
    V = pkg.variables
    b = pkg.Planet(name="b", basis="RadialVelocityOrbit", observations=[],
                   variables=V(a=pkg.LogUniform(0.5, 3.0), e=pkg.Uniform(0.0, 0.5), ω=pkg.Uniform(0.0, 6.28), tp=55010.0, mass=pkg.LogUniform(0.5, 5.0)))
    return pkg.System(name="gp", companions=[b], observations=observations, variables=V(M=1.0))


def test_the_traced_closure_gives_the_term_kinds(pkg):
    obs = gp_obs(pkg)
    assert obs.gp_terms == [gref.SHO] and callable(obs.gaussian_process)
    d = pkg.derived
    mixed = gp_obs(pkg, lambda θ: pkg.RealTerm(d.exp(θ.log_S0), 0.1) + pkg.ComplexTerm(θ.Q, 0.0, θ.w0, 0.3) + pkg.Celerite(pkg.SHOTerm(2.0, θ.Q, θ.w0)))
    assert mixed.gp_terms == [gref.REAL, gref.COMPLEX, gref.SHO]
    assert (pkg.gp.REAL, pkg.gp.COMPLEX, pkg.gp.SHO) == (gref.REAL, gref.COMPLEX, gref.SHO)


@pytest.mark.gpu
def test_the_model_binds_the_expected_nodes(pkg):
    obs = gp_obs(pkg, trend=lambda θ, t: θ.slope * (t - 55040.0), slope=pkg.Normal(0, 1))
    model = pkg.LogDensityModel(system_of(pkg, [obs]))
    try:
        assert model.D == 10 and model.program is not None and model.ln_like.n_obs == 0      # the table is left out of the main library's dataset
        o, nodes = model._gp
        assert o is obs and len(nodes) == 3 + 2 + 1
        scope = ("sysobs", id(obs))
        ix = {k: model._index[scope + (k,)] for k in ("offset", "jitter", "log_S0", "Q", "w0", "slope")}
        ops = model.program.op_names()
        op, a, _, _ = ops[nodes[0] - model.D]
        assert nodes[0] >= model.D and op == "EXP" and a == ix["log_S0"]      # S0 = exp(log_S0): an exp node of the program
        assert nodes[1:] == [ix["Q"], ix["w0"], ix["offset"], ix["slope"], ix["jitter"]]
        assert obs.gp_columns.shape == (2, 21) and np.all(obs.gp_columns[0] == 1.0)
        assert np.array_equal(obs.gp_columns[1], obs.table["epoch"] - 55040.0)
    finally:
        model.close()


def test_what_is_not_a_celerite_kernel_is_refused_as_before(pkg):
    tab = rv_table()
    for closure in (lambda θ: None, lambda θ: object(), lambda θ: {"kernel": "Matern52"}, "not callable"):
        with pytest.raises(NotImplementedError):
            pkg.StarAbsoluteRVObs(tab, name="x", gaussian_process=closure)
    sho = lambda θ: pkg.Celerite(pkg.SHOTerm(2.0, 1.0, 0.3))      # noqa: E731
    assert pkg.StarAbsoluteRVObs(tab, name="x", gaussian_process=sho).gp_terms == [gref.SHO]
    for cls in (pkg.MarginalizedStarAbsoluteRVObs, pkg.PlanetRelativeRVObs):
        with pytest.raises(NotImplementedError):
            cls(tab, name="x", gaussian_process=sho)
    with pytest.raises(TypeError):
        pkg.Celerite()
    with pytest.raises(TypeError):
        pkg.Celerite(3.0)


@pytest.mark.gpu
def test_a_second_gp_observation_is_refused(pkg):
    with pytest.raises(NotImplementedError):
        pkg.LogDensityModel(system_of(pkg, [gp_obs(pkg), gp_obs(pkg)]))
