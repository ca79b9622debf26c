"""
Derived variables on the device: the expression programs of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, "Derived variables")
against the oracle's model callback, the device model and the NumPy restatement tests/program_reference.py, and every consumer of the handle
routed through them. The bars are the ones tests/test_model.py::_check holds the device model to: ℓπ within 1e-12·max(1, |ℓπ|), the gradient
within 1e-9·|g| + 1e-12·(the row's largest |g|); node values at rtol 1e-12 (test_gpu_model_reference_style's bar for invlink). The programs
the restatement evaluates are written here by hand (program_reference.Tape); where a model's tracer (host/derived.py) produced the device's
program, agreement holds the tracer to them as well. Sizes: a partial wave, a wave edge, several blocks (W <= 256), 1 and 256 nodes.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest

import hmc_reference as hr
import program_reference as pref
import test_model as tm

pytestmark = pytest.mark.gpu
EINVAL, ENOTSUP = 1, 5


def within_bars(lp, g, lp_ref, g_ref):
    """tests/test_model.py::_check against an array reference; non-finite ℓπ must agree exactly and carry an all-zero gradient row"""
    fin = np.isfinite(lp_ref)
    assert np.array_equal(fin, np.isfinite(lp)), (np.nonzero(fin != np.isfinite(lp))[0][:8])
    assert np.all(lp[~fin] == lp_ref[~fin]) and np.all(g[:, ~fin] == 0.0)
    err = np.abs(lp[fin] - lp_ref[fin]) / np.maximum(1, np.abs(lp_ref[fin]))
    assert np.all(err <= 1e-12), err.max()
    gr, gg = g_ref[:, fin], g[:, fin]
    tol = 1e-9 * np.abs(gr) + 1e-12 * np.abs(gr).max(axis=1, keepdims=True)
    assert np.all(np.abs(gg - gr) <= tol), np.max(np.abs(gg - gr) / np.maximum(tol, 1e-300))


def as_program(pkg, tape, terms=()):
    """a hand-written tape as the Program PriorDraws takes"""
    prog = pkg.derived.Program(tape.D)
    prog.ops, prog.terms = list(tape.ops), [int(t) for t in terms]
    return prog


def identity_program(pkg, model):
    """The standard model `model` written as a program: THETA sources are bare nodes, UniformCircular is ATAN2 + MULC + a UnitLength term in
    primitives, tp is a TPERI binding. Returns (tape, binds, terms)."""
    cap = pkg.capi
    t, binds, terms, angle = pref.Tape(model.D), [], [], {}
    for kind, i0, i1, flags, value in list(model._esrc) + list(model._nsrc):
        if kind == cap.SRC_CONST:
            binds.append((pref.BIND_NODE, t.const(value), 0.0))
        elif kind == cap.SRC_THETA:
            binds.append((pref.BIND_NODE, i0, 0.0))
        else:
            if (i0, i1) not in angle:
                angle[(i0, i1)] = t.atan2(i1, i0)
            if flags & cap.SRC_FLAG_UNITLEN:
                terms.append(t.unit_length(i0, i1))
            binds.append((pref.BIND_NODE, t.mulc(angle[(i0, i1)], value * (1.0 / (2 * math.pi))), 0.0) if kind == cap.SRC_CIRCULAR
                         else (pref.BIND_TPERI, angle[(i0, i1)], value))
    return t, binds, terms


@pytest.fixture(scope="module")
def golden(pkg, oracle):
    """The golden D = 11 model: the device model, its identity program on a handle of its own, 256 points around the fixture's θ_t and the
    oracle's ℓπ and ∇ℓπ there (computed once)."""
    from octofitter_jl_amd.host.draws import PriorDraws
    case = json.loads((tm.ROOT / "tests" / "golden" / "model.json").read_text())["cases"][0]
    model = pkg.LogDensityModel(tm._reference_test_model(pkg))
    tape, binds, terms = identity_program(pkg, model)
    pd = PriorDraws(model, program=(as_program(pkg, tape, terms), binds))
    base = np.asarray(case["theta_t"])
    rng = np.random.default_rng(5)
    th = np.tile(base, (1, 256 // base.shape[1] + 1))[:, :256] + 0.05 * rng.normal(size=(11, 256))
    th[:, :base.shape[1]] = base
    obs, planets = tm._tables(case)
    lp_o, g_o = oracle.oracle_model_logpost(obs, planets, model._c_priors, model._c_esrc, None, th)
    yield dict(case=case, model=model, pd=pd, tape=tape, binds=binds, terms=terms, th=th, lp=lp_o, g=g_o, obs=obs, planets=planets)
    pd.close()
    model.close()


# ---------------------------------------------------------------------------------------------------- 1. identity program = standard model
@pytest.mark.parametrize("W,ld", [(1, 1), (63, 63), (64, 64), (65, 65), (200, 256)])
def test_identity_program_is_the_standard_model(golden, W, ld):
    import torch
    g = golden
    buf = torch.full((11, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :W] = torch.as_tensor(g["th"][:, :W], device="cuda")
    tt = buf[:, :W]
    lp_buf = torch.full((ld,), float("nan"), dtype=torch.float64, device="cuda")
    g_buf = torch.full((11, ld), float("nan"), dtype=torch.float64, device="cuda")
    g["pd"].program_logpost(tt, out=(lp_buf[:W], g_buf[:, :W]))
    lp_m, g_m = g["model"].logpost_device(tt.contiguous())
    torch.cuda.synchronize()
    lp, gr = lp_buf[:W].cpu().numpy(), g_buf[:, :W].cpu().numpy()
    within_bars(lp, gr, g["lp"][:W], g["g"][:, :W])
    within_bars(lp, gr, lp_m.cpu().numpy(), g_m.cpu().numpy())
    assert bool(torch.isnan(lp_buf[W:]).all()) and bool(torch.isnan(g_buf[:, W:]).all())      # nothing beyond W is written
    lp_f, none = g["pd"].program_logpost(tt, grad=False)
    assert none is None and np.array_equal(lp_f.cpu().numpy(), lp)      # the forward-only instantiation rounds the value path identically
    if W == 1:
        within_bars(lp, gr, np.asarray(g["case"]["lp"])[:1], np.asarray(g["case"]["grad"])[:, :1])      # the 60-digit fixture itself


# ---------------------------------------------------------------------------------------------------- 2. the period parameterisation
T_REF = 58000.0


def period_tables():
    rng = np.random.default_rng(23)
    t_rv = T_REF + 25.0 * np.arange(40)
    t_as = T_REF + 180.0 * np.arange(12)
    astrom = dict(epoch=t_as, ra=rng.normal(0, 150.0, 12), dec=rng.normal(0, 150.0, 12), σ_ra=np.full(12, 400.0), σ_dec=np.full(12, 400.0))
    rv = dict(epoch=t_rv, rv=rng.normal(0, 40, 40), σ_rv=np.full(40, 80.0))
    return astrom, rv


def period_model(pkg, tperi_binding):
    """One planet, 40 absolute-RV rows and 12 RA/Dec rows, a = cbrt(M·P²); tp = τ·P·365.25 + t_ref, or θ_at_epoch_to_tperi whose a is derived."""
    d = pkg.derived
    astrom_t, rv_t = period_tables()
    astrom = pkg.PlanetRelAstromObs(astrom_t, name="sim")
    rv = pkg.StarAbsoluteRVObs(rv_t, name="rv", variables=pkg.variables(offset=pkg.Normal(0, 20), jitter=pkg.LogUniform(0.1, 20.0)))
    last = dict(θ=pkg.UniformCircular(), mass=pkg.LogUniform(1.0, 50.0), a=pkg.Derived(lambda b, system: d.cbrt(system.M * b.P ** 2)),
                tp=pkg.θ_at_epoch_to_tperi("θ", T_REF)) if tperi_binding else \
        dict(τ=pkg.UniformCircular(1.0), mass=pkg.LogUniform(1.0, 50.0), a=pkg.Derived(lambda b, system: d.cbrt(system.M * b.P ** 2)),
             tp=pkg.Derived(lambda b: b.τ * b.P * 365.25 + T_REF))
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom],
                   variables=pkg.variables(P=pkg.Uniform(5.0, 40.0), e=pkg.Uniform(0.0, 0.6), i=pkg.Sine(), ω=pkg.UniformCircular(), Ω=pkg.UniformCircular(), **last))
    sys_ = pkg.System(name="period", companions=[b], observations=[rv],
                      variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.05), lower=0.1), plx=pkg.truncated(pkg.Normal(50.0, 0.1), lower=0.1)))
    return pkg.LogDensityModel(sys_)


PERIOD_NAMES = ["M", "plx", "rv_offset", "rv_jitter", "b_P", "b_e", "b_i", "b_ωx", "b_ωy", "b_Ωx", "b_Ωy", "b_τx", "b_τy", "b_mass"]


def period_program(tperi_binding):
    """the same model by hand: (tape, binds, terms, node of a, node of tp or None)"""
    t = pref.Tape(14)
    M, plx, off, jit, P, e, i, wx, wy, Ox, Oy, tx, ty, mass = range(14)
    terms = []
    w = t.mulc(t.atan2(wy, wx), 1.0); terms.append(t.unit_length(wx, wy))
    O = t.mulc(t.atan2(Oy, Ox), 1.0); terms.append(t.unit_length(Ox, Oy))
    ang = t.atan2(ty, tx)
    tau = t.mulc(ang, 1.0 if tperi_binding else 1.0 * (1.0 / (2 * math.pi))); terms.append(t.unit_length(tx, ty))
    a = t.cbrt(t.mul(M, t.powc(P, 2.0)))
    tp = None if tperi_binding else t.addc(t.mulc(t.mul(tau, P), 365.25), T_REF)
    node = lambda n: (pref.BIND_NODE, n, 0.0)      # noqa: E731
    c0, c1 = t.const(0.0), t.const(1.0)
    binds = [node(a), node(e), node(i), node(w), node(O), (pref.BIND_TPERI, ang, T_REF) if tperi_binding else node(tp), node(M), node(plx), node(mass),
             node(c0), node(c1), node(c0), node(off), node(jit), node(c0)]
    return t, binds, terms, a, tp


def period_points(model, W, seed):
    rng = np.random.default_rng(seed)
    return model.link(model.sample_priors(rng, W))


@pytest.mark.parametrize("tperi_binding", [False, True], ids=["tp_derived", "tp_binding_on_derived_a"])
def test_period_parameterisation(pkg, oracle, tperi_binding):
    import torch
    model = period_model(pkg, tperi_binding)
    try:
        assert model.D == 14 and model._m is None and model.program is not None
        assert [n.replace("θ", "τ") for n in model.names] == PERIOD_NAMES
        assert model.derived_names == (["b_a"] if tperi_binding else ["b_a", "b_tp"])
        tape, binds, terms, _a, _tp = period_program(tperi_binding)
        th = period_points(model, 200, 3)
        lp_r, g_r, inputs = pref.logpost(oracle, model.ln_like.obs_tables, model.ln_like.planet_desc, model.priors, tape.ops, binds, terms, th)
        assert np.isfinite(lp_r).sum() >= 150
        lp, g = model.logpost_device(torch.as_tensor(th, device="cuda"))
        within_bars(lp.cpu().numpy(), g.cpu().numpy(), lp_r, g_r)
        lp_h, g_h = model.logdensity_and_gradient(th[:, :3])      # the host-buffer callbacks take the same route
        assert np.array_equal(lp_h, lp.cpu().numpy()[:3]) and np.array_equal(g_h, g.cpu().numpy()[:, :3])
        el, nu = model.kernel_inputs(model.invlink(th))
        assert np.allclose(np.concatenate([el, nu]), inputs, rtol=1e-9, atol=0, equal_nan=True)
    finally:
        model.close()


# ---------------------------------------------------------------------------------------------------- 3. e = h² + k², ω = atan(h, k)
def test_domain_error_costs_one_walker_alone(pkg, oracle):
    """e = h² + k² >= 1 is −Inf with an all-zero gradient row; the neighbours of such walkers hold the bits they have in a batch without
    them. The context runs batch-invariant (OCTO_OPT_BATCH_INVARIANT), which is what makes ℓ itself a function of the column alone."""
    import torch
    d = pkg.derived
    astrom = pkg.PlanetRelAstromObs(period_tables()[0], name="sim")
    b = pkg.Planet(name="b", basis="Visual{KepOrbit}", observations=[astrom],
                   variables=pkg.variables(a=pkg.LogUniform(5, 20), h=pkg.Uniform(-1.0, 1.0), k=pkg.Uniform(-1.0, 1.0), i=pkg.Sine(), Ω=pkg.UniformCircular(),
                                           tp=pkg.Normal(T_REF, 100.0), e=pkg.Derived(lambda v: v.h * v.h + v.k * v.k), ω=pkg.Derived(lambda v: d.atan(v.h, v.k))))
    model = pkg.LogDensityModel(pkg.System(name="hk", companions=[b], observations=[],
                                           variables=pkg.variables(M=pkg.truncated(pkg.Normal(1.2, 0.05), lower=0.1), plx=pkg.truncated(pkg.Normal(50.0, 0.1), lower=0.1))))
    try:
        model.ln_like._check(model.ln_like.lib.octo_ctx_set_option(model.ln_like._ctx, pkg.capi.OPT_BATCH_INVARIANT, 1), "octo_ctx_set_option")
        assert model.names == ["M", "plx", "b_a", "b_h", "b_k", "b_i", "b_Ωx", "b_Ωy", "b_tp"] and model.derived_names == ["b_e", "b_ω"]
        rng = np.random.default_rng(9)
        W = 130
        x = model.sample_priors(rng, W)
        x[3], x[4] = rng.uniform(-0.6, 0.6, W), rng.uniform(-0.6, 0.6, W)      # e <= 0.72
        good = model.link(x)
        bad_cols = np.array([0, 5, 63, 64, 100, 129])
        x[3, bad_cols], x[4, bad_cols] = 0.8, -0.75                            # e = 1.2025
        mixed = model.link(x)
        lp_g, g_g = (t.cpu().numpy() for t in model.logpost_device(torch.as_tensor(good, device="cuda")))
        lp_m, g_m = (t.cpu().numpy() for t in model.logpost_device(torch.as_tensor(mixed, device="cuda")))
        assert np.all(np.isfinite(lp_g))
        assert np.all(np.isneginf(lp_m[bad_cols])) and np.all(g_m[:, bad_cols] == 0.0)
        keep = np.setdiff1d(np.arange(W), bad_cols)
        assert np.array_equal(lp_m[keep], lp_g[keep]) and np.array_equal(g_m[:, keep], g_g[:, keep])      # bitwise
        # and the restatement, by hand: e, ω, the Ω pair
        t = pref.Tape(9)
        e = t.add(t.mul(3, 3), t.mul(4, 4)); w = t.atan2(3, 4)
        O = t.mulc(t.atan2(7, 6), 1.0); term = t.unit_length(6, 7)
        c0, c1 = t.const(0.0), t.const(1.0)
        binds = [(0, n, 0.0) for n in (2, e, 5, w, O, 8, 0, 1, c0, c0, c1, c0)]
        lp_r, g_r, _ = pref.logpost(oracle, model.ln_like.obs_tables, model.ln_like.planet_desc, model.priors, t.ops, binds, [term], mixed)
        within_bars(lp_m, g_m, lp_r, g_r)
    finally:
        model.close()


# ---------------------------------------------------------------------------------------------------- 4. opcodes, shared nodes, the smallest and the largest program
ELEMS = dict(a=10.0, e=0.1, i=0.5, w=0.3, O=0.2, tp=50000.0, M=1.2, plx=50.0, mass=0.0)


def constant_binds(t, **over):
    """bindings of the golden dataset (one planet, one astrometry table) to constants, but for the inputs named in `over` (name -> node)"""
    names = list(ELEMS) + ["jitter", "platescale", "northangle"]
    vals = dict(ELEMS, jitter=0.0, platescale=1.0, northangle=0.0)
    return [(pref.BIND_NODE, over[n] if n in over else t.const(vals[n]), 0.0) for n in names]


def test_every_opcode_and_shared_nodes(pkg, golden):
    import torch
    from octofitter_jl_amd.host.draws import PriorDraws
    from test_program_reference import every_opcode_tape
    tape, outs, _ = every_opcode_tape()
    n_core = tape.D + len(tape.ops)
    priors = [pkg.Uniform(1.0, 2.0), pkg.Uniform(0.5, 1.0), pkg.Uniform(2.0, 2.5)]
    binds = constant_binds(tape)
    rng = np.random.default_rng(2)
    th = rng.normal(0.0, 1.5, (3, 130))
    with PriorDraws(golden["model"], priors=priors, program=(as_program(pkg, tape), binds)) as pd:
        nodes = np.arange(n_core)
        got = pd.program_values(torch.as_tensor(th, device="cuda"), nodes).cpu().numpy()
        want = pref.values(priors, tape.ops, th, nodes)
        assert np.all(np.isfinite(want)) and got.shape == want.shape
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), np.max(np.abs(got - want) / np.abs(want))
        one = pd.program_values(torch.as_tensor(th[:, :1], device="cuda"), [outs[2], 0]).cpu().numpy()
        assert np.array_equal(one, got[[outs[2], 0], :1])


def test_log_of_a_negative_node_costs_that_walker_alone(pkg, oracle, golden):
    from octofitter_jl_amd.host.draws import PriorDraws
    import torch
    priors = [pkg.Normal(0.0, 1.0)]
    th = np.linspace(-2.0, 2.0, 70)[None, :] + 0.013      # x = θ_t: negative in the first half
    neg = th[0] < 0
    for as_term in (True, False):
        t = pref.Tape(1)
        lg = t.log(0)
        if as_term:
            binds, terms = constant_binds(t), [lg]
        else:
            binds, terms = constant_binds(t, e=t.addc(t.mulc(lg, 0.05), 0.3)), []      # the NaN reaches the likelihood as its eccentricity
        with PriorDraws(golden["model"], priors=priors, program=(as_program(pkg, t, terms), binds)) as pd:
            lp, g = (x.cpu().numpy() for x in pd.program_logpost(torch.as_tensor(th, device="cuda")))
            v = pd.program_values(torch.as_tensor(th, device="cuda"), [lg]).cpu().numpy()[0]
        assert np.all(np.isnan(v[neg])) and np.all(np.isfinite(v[~neg]))
        assert np.all(np.isneginf(lp[neg])) and np.all(g[:, neg] == 0.0) and np.all(np.isfinite(lp[~neg])) and np.all(g[:, ~neg] != 0.0)
        lp_r, g_r, _ = pref.logpost(oracle, golden["obs"], golden["planets"], priors, t.ops, binds, terms, th)
        within_bars(lp, g, lp_r, g_r)


def test_no_ops_and_one_parameter(pkg, oracle, golden):
    """n_ops = 0, D = 1: every input is node 0"""
    from octofitter_jl_amd.host.draws import PriorDraws
    import torch
    priors = [pkg.Uniform(0.3, 0.6)]
    t = pref.Tape(1)
    binds = [(pref.BIND_NODE, 0, 0.0)] * 12
    th = np.random.default_rng(4).normal(0, 1.0, (1, 65))
    with PriorDraws(golden["model"], priors=priors, program=(as_program(pkg, t), binds)) as pd:
        lp, g = (x.cpu().numpy() for x in pd.program_logpost(torch.as_tensor(th, device="cuda")))
    lp_r, g_r, _ = pref.logpost(oracle, golden["obs"], golden["planets"], priors, [], binds, [], th)
    assert np.all(np.isfinite(lp_r))
    within_bars(lp, g, lp_r, g_r)


def test_a_program_of_exactly_256_nodes(pkg, oracle, golden):
    """D = 64 and OCTO_DRAWS_PROGRAM_MAX_OPS ops: 128 KB of LDS a block, above the default limit"""
    from octofitter_jl_amd.host.draws import PriorDraws
    import torch
    D = 64
    priors = [pkg.Normal(0.0, 1.0)] * D
    t = pref.Tape(D)
    prev = 0
    for j in range(180):
        prev = t.add(prev, 1 + j % 63) if j % 3 == 0 else t.mulc(prev, 0.5) if j % 3 == 1 else t.sin(prev)
    s = prev      # in [−1, 1]
    over = dict(a=t.addc(t.mulc(s, 2.0), 10.0), e=t.addc(t.mulc(s, 0.1), 0.3), M=t.addc(t.mulc(s, 0.1), 1.2), plx=t.addc(s, 50.0), i=t.addc(t.mulc(s, 0.2), 0.6), w=s, O=s)
    c0, c1, ctp = t.const(0.0), t.const(1.0), t.const(50000.0)
    names = list(ELEMS) + ["jitter", "platescale", "northangle"]
    over.update(tp=ctp, mass=c0, jitter=c0, platescale=c1, northangle=c0)
    binds = [(pref.BIND_NODE, over[n], 0.0) for n in names]
    assert len(t.ops) == pref.MAX_OPS and D + len(t.ops) == 256
    th = np.random.default_rng(6).normal(0, 1.0, (D, 70))
    with PriorDraws(golden["model"], priors=priors, program=(as_program(pkg, t), binds)) as pd:
        tt = torch.as_tensor(th, device="cuda")
        lp, g = (x.cpu().numpy() for x in pd.program_logpost(tt))
        got = pd.program_values(tt, [255, 128, 64, 0]).cpu().numpy()
    want = pref.values(priors, t.ops, th, [255, 128, 64, 0])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    lp_r, g_r, _ = pref.logpost(oracle, golden["obs"], golden["planets"], priors, t.ops, binds, [], th)
    assert np.all(np.isfinite(lp_r))
    within_bars(lp, g, lp_r, g_r)


# ---------------------------------------------------------------------------------------------------- 5. healing and finiteness
def test_healed_prior_and_non_finite_theta(oracle, golden):
    """tests/test_model.py::test_gpu_model_healed_prior_keeps_the_likelihood_gradient's case, as a program"""
    import torch
    g = golden
    th = g["th"][:, :70].copy()
    th[3, 1] = 800.0                 # e == its upper bound: log-Jacobian −Inf -> healed
    th[3, 0] = np.nan                # non-finite θ_t -> −Inf, zero gradient
    th[6, 66] = np.inf
    lp, gr = (x.cpu().numpy() for x in g["pd"].program_logpost(torch.as_tensor(th, device="cuda")))
    lp_o, g_o = oracle.oracle_model_logpost(g["obs"], g["planets"], g["model"]._c_priors, g["model"]._c_esrc, None, th)
    lp_m, g_m = (x.cpu().numpy() for x in g["model"].logpost_device(torch.as_tensor(th, device="cuda")))
    for bad in (0, 66):
        assert np.isneginf(lp[bad]) and np.all(gr[:, bad] == 0.0)
    assert lp[1] < -1e300 and lp_o[1] < -1e300 and np.all(np.isfinite(gr[:, 1])) and np.any(gr[:, 1] != 0.0)
    sc = np.maximum(np.abs(g_o[:, 1]).max(), 1e-300)
    assert np.all(np.abs(gr[:, 1] - g_o[:, 1]) <= 1e-9 * sc) and np.all(np.abs(gr[:, 1] - g_m[:, 1]) <= 1e-9 * sc)
    ok = np.setdiff1d(np.arange(70), [0, 1, 66])
    within_bars(lp[ok], gr[:, ok], lp_o[ok], g_o[:, ok])


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(pkg, golden):
    import torch
    from octofitter_jl_amd.host.draws import PriorDraws
    d = pkg.derived
    model, fn = golden["model"], golden["model"].ln_like
    tape, binds, terms = golden["tape"], golden["binds"], golden["terms"]

    def attempt(pd, ops, bs, ts, n_planets=1, n_obs=1):
        prog = d.Program(11)
        prog.ops, prog.terms = list(ops), list(ts)
        o, n_o, b, n_b, t, n_t = prog.c_arrays(bs)
        st = pd.lib.octo_draws_program_set(pd._h, fn._ds, n_planets, n_obs, C.cast(o, C.c_void_p), n_o, C.cast(b, C.c_void_p), n_b, C.cast(t, C.c_void_p), n_t)
        return st, pd.lib.octo_draws_last_error(pd._h).decode()

    with PriorDraws(model, program=(as_program(pkg, tape, terms), binds)) as pd:
        tt = torch.as_tensor(golden["th"][:, :8], device="cuda").contiguous()
        before = pd.program_logpost(tt)[0].cpu().numpy()
        bad_op = list(tape.ops); bad_op[1] = ("ADD", 0, 1, 0.0); raw = d.Program(11); raw.ops = bad_op
        o, n_o, b, n_b, t, n_t = raw.c_arrays(binds)
        o[1].op = 99
        st = pd.lib.octo_draws_program_set(pd._h, fn._ds, 1, 1, C.cast(o, C.c_void_p), n_o, C.cast(b, C.c_void_p), n_b, C.cast(t, C.c_void_p), 0)
        assert st == EINVAL and "op 1" in pd.lib.octo_draws_last_error(pd._h).decode()
        fwd = list(tape.ops); fwd[2] = ("ADD", 0, 11 + 2, 0.0)      # op 2 reads itself
        st, msg = attempt(pd, fwd, binds, terms)
        assert st == EINVAL and "op 2" in msg and "forward reference" in msg
        st, msg = attempt(pd, tape.ops, binds[:-1], terms)
        assert st == EINVAL and "11 bindings" in msg
        st, msg = attempt(pd, tape.ops, binds, terms, n_obs=2)
        assert st == EINVAL and "bindings" in msg
        moved = list(binds); moved[3], moved[5] = binds[5], binds[3]      # the TPERI binding on the ω slot
        st, msg = attempt(pd, tape.ops, moved, terms)
        assert st == EINVAL and "binding 3" in msg
        far = list(binds); far[7] = (pref.BIND_NODE, 11 + len(tape.ops), 0.0)
        st, msg = attempt(pd, tape.ops, far, terms)
        assert st == EINVAL and "binding 7" in msg
        odd = list(binds); odd[2] = (7, 0, 0.0)
        st, msg = attempt(pd, tape.ops, odd, terms)
        assert st == EINVAL and "binding 2" in msg
        st, msg = attempt(pd, tape.ops, binds, [11 + len(tape.ops)])
        assert st == EINVAL and "term 0" in msg
        ti = list(binds); ti[5] = (pref.BIND_TPERI | pref.BIND_FLAG_TI, binds[5][1], binds[5][2])
        st, msg = attempt(pd, tape.ops, ti, terms)
        assert st == ENOTSUP and "binding 5" in msg
        long = list(tape.ops) + [("ADDC", 0, 0, 1.0)] * (pref.MAX_OPS + 1 - len(tape.ops))
        st, msg = attempt(pd, long, binds, terms)
        assert st == ENOTSUP and "OCTO_DRAWS_PROGRAM_MAX_OPS" in msg
        assert np.array_equal(pd.program_logpost(tt)[0].cpu().numpy(), before)      # a refused program leaves the one in place
        # after program_clear the handle samples, and is a sampling-only handle again
        pd.program_clear()
        with pytest.raises(pkg.capi.OctoError) as e:
            pd.program_logpost(tt)
        assert "no program" in str(e.value)
        with pytest.raises(pkg.capi.OctoError) as e:
            pd.best(1, 64, keep=1)
        assert "no model" in str(e.value)
        lp, ll, dH, acc = pd.hmc_step(tt.clone(), eps=0.05, n_leapfrog=2, seed=1)
        assert lp is None and ll is None and bool(torch.isfinite(dH).all())
        assert pd.sample(1, 0, 4)[0].shape == (11, 4)
    with PriorDraws(model) as with_model:      # a handle with a model refuses a program
        st, msg = attempt(with_model, tape.ops, binds, terms)
        assert st == EINVAL and "has a model" in msg


# ---------------------------------------------------------------------------------------------------- 7. the reference table does not leak in
def test_an_active_reference_table_changes_nothing(golden):
    import torch
    pd = golden["pd"]
    tt = torch.as_tensor(golden["th"][:, :130], device="cuda").contiguous()
    lp0, g0 = (x.cpu().numpy() for x in pd.program_logpost(tt))
    ref = pd.reference_table()
    bad = pd.reference_set(ref, np.linspace(-0.5, 0.5, 11), np.full(11, 0.7))
    with pd.reference(ref):
        lp1, g1 = (x.cpu().numpy() for x in pd.program_logpost(tt))
        lpt = pd.sample(1, 0, 8)[2].cpu().numpy()
    assert int(bad.item()) == 0 and np.all(np.isfinite(lpt))
    assert np.array_equal(lp0, lp1, equal_nan=True) and np.array_equal(g0, g1, equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 8. every consumer is routed
@pytest.fixture(scope="module")
def pair(golden):
    """the program handle, a handle on the device model, and W = 256 starting points"""
    import torch
    from octofitter_jl_amd.host.draws import PriorDraws
    pm = PriorDraws(golden["model"])
    yield golden["pd"], pm, torch.as_tensor(golden["th"], device="cuda").contiguous()
    pm.close()


def lp_matches_its_point(pd, theta_t, lp):
    want = pd.program_logpost(theta_t, grad=False)[0].cpu().numpy()
    lp = lp.cpu().numpy()
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(lp)) and fin.sum() >= 0.9 * fin.size
    assert np.all(np.abs(lp[fin] - want[fin]) <= 1e-12 * np.maximum(1, np.abs(want[fin]))), np.max(np.abs(lp[fin] - want[fin]))


def test_hmc_step_is_routed(pair):
    import torch
    pp, pm, start = pair
    out = {}
    # ε per chain, over two decades of steps chains accept; none so long that |dH| outgrows the 1e-9 bar's meaning in FP64 (at ε = 1e-2
    # this target gives |dH| ~ 3e6, whose ulp is 5e-10)
    eps = torch.logspace(-6, -4, start.shape[1], dtype=torch.float64, device="cuda")
    for name, pd in (("program", pp), ("model", pm)):
        tt = start.clone()
        lp, ll, dH, acc, prop = pd.hmc_step(tt, eps=eps, n_leapfrog=4, seed=11, step=3, want_proposal=True)
        out[name] = [x.cpu().numpy() for x in (tt, lp, dH, acc, prop)]
        tt_h, _, _, acc_h, prop_h = out[name]
        took = acc_h != 0
        assert took.any() and np.array_equal(tt_h[:, took], prop_h[:, took]) and np.array_equal(tt_h[:, ~took], start.cpu().numpy()[:, ~took])
    (_, lp_p, dH_p, _, prop_p), (_, lp_m, dH_m, _, prop_m) = out["program"], out["model"]
    tol = 1e-9 * np.abs(prop_m) + 1e-12 * np.abs(prop_m).max(axis=1, keepdims=True)
    assert np.all(np.abs(prop_p - prop_m) <= tol), np.max(np.abs(prop_p - prop_m) / tol)
    fin = np.isfinite(dH_m)
    assert np.array_equal(fin, np.isfinite(dH_p)) and np.all(np.abs(dH_p[fin] - dH_m[fin]) <= 1e-9)


def test_nuts_slice_lbfgs_and_pathfinder_are_routed(pair):
    pp, _pm, start = pair
    tt = start.clone()
    lp = pp.nuts_step(tt, eps=0.02, max_depth=3, seed=12, step=1)[0]
    lp_matches_its_point(pp, tt, lp)
    tt = start.clone()
    r = pp.slice_step(tt, w=1.0, p=2, n_passes=1, seed=13, step=1)
    lp_matches_its_point(pp, tt, r["logpost"])
    tt = start.clone()
    r = pp.lbfgs(tt, n_rounds=3)
    lp_matches_its_point(pp, tt, r["logpost"])
    tt = start.clone()
    r = pp.pathfinder(tt, n_rounds=1, seed=14)
    lp_matches_its_point(pp, tt, r["logpost"])


def test_best_and_rejection_are_routed(pair, golden, oracle):
    pp, pm, _ = pair
    g = golden
    N = 4096
    for seed in range(1, 20):
        _, tt, lpt = pp.sample(seed, 0, N)
        lp_o, _ = oracle.oracle_model_logpost(g["obs"], g["planets"], g["model"]._c_priors, g["model"]._c_esrc, None, tt.cpu().numpy(), grad=False, n_threads=0)
        top = np.sort(lp_o[np.isfinite(lp_o)])[::-1][:5]
        if np.all(-np.diff(top) > 1e-6):
            break
    assert np.all(-np.diff(top) > 1e-6), top      # the oracle's five best are pairwise more than 1e-6 apart: the order is decided
    th_p, lp_p, ix_p = pp.best(seed, N, keep=4)
    th_m, lp_m, ix_m = pm.best(seed, N, keep=4)
    assert np.array_equal(ix_p, ix_m) and np.array_equal(ix_p, np.argsort(-np.where(np.isfinite(lp_o), lp_o, -np.inf), kind="stable")[:4].astype(np.uint64))
    assert np.array_equal(th_p, th_m) and np.all(np.abs(lp_p - lp_m) <= 1e-12 * np.maximum(1, np.abs(lp_m)))
    # rejection: every draw's acceptance is decided by a margin far above the two routes' difference
    ll_o = lp_o - lpt.cpu().numpy()
    ll_o = np.where(np.isfinite(ll_o), ll_o, -np.inf)
    u = hr.rejection_uniforms(seed, np.arange(N, dtype=np.uint64))
    margin = np.abs(u - np.exp(ll_o - ll_o.max()))
    assert margin.min() > 1e-9, margin.min()
    r_p, r_m = pp.rejection(seed, N), pm.rejection(seed, N)
    assert r_p["n_accepted"] == r_m["n_accepted"] == int(np.sum(u < np.exp(ll_o - ll_o.max()))) and np.array_equal(r_p["index"], r_m["index"])
    assert np.array_equal(r_p["samples"], r_m["samples"])


# ---------------------------------------------------------------------------------------------------- 9. end to end
def test_nuts_driver_end_to_end(pkg):
    model = period_model(pkg, False)
    try:
        r = pkg.octofit_nuts_device(model, n_chains=64, n_warmup=30, n_samples=20, max_depth=6, seed=5)
        assert r["logpost"].shape == (20, 64) and np.all(np.isfinite(r["logpost"]))
        assert set(r["derived"]) == {"b_a", "b_tp"} and r["derived"]["b_a"].shape == (20, 64)
        tape, _binds, _terms, a, tp = period_program(False)
        th = np.moveaxis(r["samples_t"], 1, 0).reshape(14, -1)
        want = pref.values(model.priors, tape.ops, th, [a, tp]).reshape(2, 20, 64)
        for got, ref in ((r["derived"]["b_a"], want[0]), (r["derived"]["b_tp"], want[1])):
            assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref)), np.max(np.abs(got - ref) / np.abs(ref))
    finally:
        model.close()
