"""
The host side of a Gaussian-process RV observation under DENSE kernels (host/gp.py, host/observations.py, host/model.py): the traced closure that returns
`GP(QuasiPeriodicTerm(…))`, the nodes it gives the model, and the refusals that stay. The constructors' tests need no GPU; a LogDensityModel opens a device
context, so the test that builds one is marked gpu.
"""
import numpy as np
import pytest

import gp_reference as gref
import gpd_reference as dref
from test_gp_host import rv_table, system_of


def qp_obs(pkg, n=20, **more):
    """an absolute-RV table of n rows under the quasi-periodic kernel, its amplitude and period log-parameterised as the reference's tutorial has them"""
    V, d = pkg.variables, pkg.derived
    closure = lambda θ: pkg.GP(pkg.QuasiPeriodicTerm(a=d.exp(θ.log_a), l=θ.ell, P=d.exp(θ.log_P), r=θ.r))      # noqa: E731
    return pkg.StarAbsoluteRVObs(rv_table(n=n), name="harps", gaussian_process=closure,
                                 variables=V(offset=pkg.Normal(0, 10), jitter=pkg.LogUniform(0.1, 2.0), log_a=pkg.Uniform(0.0, 2.0), ell=pkg.Uniform(2.0, 40.0),
                                             log_P=pkg.Uniform(1.6, 4.0), r=pkg.Uniform(0.3, 2.0), **more))


def test_the_traced_closure_gives_the_dense_kinds(pkg):
    obs = qp_obs(pkg)
    assert obs.gp_terms == [dref.QUASIPERIODIC] and callable(obs.gaussian_process)
    d = pkg.derived
    V = pkg.variables(a=pkg.Uniform(1, 8), l=pkg.Uniform(2, 40), P=pkg.Uniform(5, 60), r=pkg.Uniform(0.3, 2))
    each = pkg.StarAbsoluteRVObs(rv_table(), name="x", variables=V, gaussian_process=lambda θ: pkg.SqExpTerm(θ.a, θ.l) + pkg.Matern32Term(d.exp(θ.a), 3.0)
                                 + pkg.DenseKernel(pkg.Matern52Term(θ.a, θ.l)) + pkg.PeriodicTerm(θ.a, θ.P, θ.r))
    assert each.gp_terms == [dref.SE, dref.MATERN32, dref.MATERN52, dref.PERIODIC]
    g = pkg.gp
    assert (g.SE, g.MATERN32, g.MATERN52, g.PERIODIC, g.QUASIPERIODIC) == (16, 17, 18, 19, 20)
    kernel = g.probe(lambda θ: pkg.GP(pkg.QuasiPeriodicTerm(θ.a, θ.l, θ.P, θ.r) + pkg.Matern32Term(θ.a, θ.l)), list(V))
    assert isinstance(kernel, pkg.DenseKernel) and kernel.kinds == [20, 17] and len(kernel.params) == 6
    assert isinstance(g.probe(lambda θ: pkg.SHOTerm(2.0, θ.a, θ.l), list(V)), pkg.Celerite)      # probe returns either class


def test_a_celerite_term_does_not_add_to_a_dense_one(pkg):
    sho, se = pkg.SHOTerm(2.0, 1.0, 0.3), pkg.SqExpTerm(1.0, 2.0)
    for bad in (lambda: sho + se, lambda: se + sho, lambda: pkg.Celerite(sho) + pkg.DenseKernel(se), lambda: pkg.DenseKernel(se) + pkg.Celerite(sho),
                lambda: pkg.DenseKernel(), lambda: pkg.DenseKernel(3.0), lambda: pkg.GP(3.0), lambda: pkg.QuasiPeriodicTerm(1.0, 2.0, 3.0)):
        with pytest.raises(TypeError):
            bad()
    assert pkg.GP(se).kinds == [dref.SE] and pkg.GP(sho).kinds == [gref.SHO]
    with pytest.raises(NotImplementedError):      # inside a closure the mixed sum is not a kernel of the HIP path
        pkg.StarAbsoluteRVObs(rv_table(), name="x", gaussian_process=lambda θ: sho + se)


def test_the_old_refusals_still_refuse(pkg):
    tab = rv_table()
    for closure in (lambda θ: None, lambda θ: object(), lambda θ: {"kernel": "Matern52"}, "not callable"):
        with pytest.raises(NotImplementedError):
            pkg.StarAbsoluteRVObs(tab, name="x", gaussian_process=closure)
    qp = lambda θ: pkg.GP(pkg.QuasiPeriodicTerm(2.0, 10.0, 25.0, 0.5))      # noqa: E731
    assert pkg.StarAbsoluteRVObs(tab, name="x", gaussian_process=qp).gp_terms == [dref.QUASIPERIODIC]
    for cls in (pkg.MarginalizedStarAbsoluteRVObs, pkg.PlanetRelativeRVObs):
        with pytest.raises(NotImplementedError):
            cls(tab, name="x", gaussian_process=qp)


@pytest.mark.gpu
def test_the_model_binds_the_expected_nodes(pkg):
    obs = qp_obs(pkg)
    model = pkg.LogDensityModel(system_of(pkg, [obs]))
    try:
        assert model.D == 10 and model.program is not None and model.ln_like.n_obs == 0
        o, nodes = model._gp
        assert o is obs and len(nodes) == 4 + 1 + 1      # H + K + 1
        scope = ("sysobs", id(obs))
        ix = {k: model._index[scope + (k,)] for k in ("offset", "jitter", "log_a", "ell", "log_P", "r")}
        ops = model.program.op_names()
        for node, name in ((nodes[0], "log_a"), (nodes[2], "log_P")):      # a log-parameterised variable arrives as an exp node
            op, a, _, _ = ops[node - model.D]
            assert node >= model.D and op == "EXP" and a == ix[name]
        assert [nodes[1], nodes[3], nodes[4], nodes[5]] == [ix["ell"], ix["r"], ix["offset"], ix["jitter"]]
        assert obs.gp_columns.shape == (1, 20) and np.all(obs.gp_columns[0] == 1.0)
    finally:
        model.close()
