"""
The expression programs of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, "Derived variables") restated in plain NumPy: the
forward tape, the reverse sweep, the TPERI binding, the prior part and the rules that join them to the likelihood. Nothing here calls the
library under test: priors are host/priors.py objects (bounds and parameters; their link, density and derivative are the restatement of
tests/hmc_reference.py), ℓ and ∂ℓ/∂inputs come from the oracle (tests/oracle_binding.py: oracle_eval), and θ_at_epoch_to_tperi is written
as a tape of the same primitive ops in the order of the reference's expression (host/model.py: _tperi, against which tests/test_program_reference.py
holds its values), so that its gradient is the reverse sweep's. A plain module, not a conftest and not a test module.
"""
import math

import numpy as np

import hmc_reference as hr

OPS = ("CONST", "ADD", "SUB", "MUL", "DIV", "NEG", "SQRT", "CBRT", "EXP", "LOG", "SIN", "COS", "ATAN2", "POWC", "MULC", "ADDC")
OP = {name: k for k, name in enumerate(OPS)}
BINARY = {"ADD", "SUB", "MUL", "DIV", "ATAN2"}
BIND_NODE, BIND_TPERI, BIND_FLAG_TI = 0, 1, 65536
MAX_OPS = 192
N_EL, N_NUIS = 9, 3
EL_A, EL_E, EL_I, EL_W, EL_O, EL_TP, EL_M, EL_PLX, EL_MASS = range(9)
K_YR, YD = 365.2568983840419, 365.25      # octo_consts_default: kepler_year_to_julian_day, year2day_julian
LOG2PI = math.log(2 * math.pi)


class Tape:
    """An op list under construction: every method appends one op (name, a, b, value) and returns its node index."""

    def __init__(self, D, ops=()):
        self.D, self.ops = int(D), list(ops)

    def emit(self, op, a=0, b=0, value=0.0):
        self.ops.append((op, int(a), int(b), float(value)))
        return self.D + len(self.ops) - 1

    def const(self, v): return self.emit("CONST", value=v)
    def add(self, a, b): return self.emit("ADD", a, b)
    def sub(self, a, b): return self.emit("SUB", a, b)
    def mul(self, a, b): return self.emit("MUL", a, b)
    def div(self, a, b): return self.emit("DIV", a, b)
    def neg(self, a): return self.emit("NEG", a)
    def sqrt(self, a): return self.emit("SQRT", a)
    def cbrt(self, a): return self.emit("CBRT", a)
    def exp(self, a): return self.emit("EXP", a)
    def log(self, a): return self.emit("LOG", a)
    def sin(self, a): return self.emit("SIN", a)
    def cos(self, a): return self.emit("COS", a)
    def atan2(self, y, x): return self.emit("ATAN2", y, x)
    def powc(self, a, c): return self.emit("POWC", a, value=c)
    def mulc(self, a, c): return self.emit("MULC", a, value=c)
    def addc(self, a, c): return self.emit("ADDC", a, value=c)

    def unit_length(self, x, y):
        """logpdf(LogNormal(0, 0.1), sqrt(x² + y²)): the UnitLengthPrior of a UniformCircular pair, src/variables.jl:309-323"""
        r = self.sqrt(self.add(self.mul(x, x), self.mul(y, y)))
        z = self.mulc(self.log(r), 10.0)
        return self.sub(self.mulc(self.neg(self.addc(self.mul(z, z), LOG2PI)), 0.5), self.log(self.mulc(r, 0.1)))

    def tperi(self, th, epoch, M, e, a, i, w, O):
        """θ_at_epoch_to_tperi (src/parameterizations.jl:34-67) in the order of host/model.py: _tperi"""
        cO, sO, cw, sw, ci = self.cos(O), self.sin(O), self.cos(w), self.sin(w), self.cos(i)
        A = self.sub(self.mul(cO, cw), self.mul(self.mul(sO, sw), ci))
        B = self.add(self.mul(sO, cw), self.mul(self.mul(cO, sw), ci))
        F = self.sub(self.neg(self.mul(cO, sw)), self.mul(self.mul(sO, cw), ci))
        G = self.add(self.neg(self.mul(sO, sw)), self.mul(self.mul(cO, cw), ci))
        det = self.sub(self.mul(A, G), self.mul(F, B))
        ct, st = self.cos(th), self.sin(th)
        xr = self.div(self.sub(self.mul(G, ct), self.mul(F, st)), det)
        yr = self.div(self.sub(self.mul(A, st), self.mul(B, ct)), det)
        nu = self.atan2(yr, xr)
        sn, cn = self.sin(nu), self.cos(nu)
        s1 = self.sqrt(self.addc(self.neg(self.mul(e, e)), 1.0))
        s1sn = self.mul(s1, sn)
        MA = self.sub(self.addc(self.atan2(self.neg(s1sn), self.sub(self.neg(e), cn)), math.pi),
                      self.div(self.mul(e, s1sn), self.addc(self.mul(e, cn), 1.0)))
        period_yrs = self.mulc(self.sqrt(self.div(self.powc(a, 3.0), M)), K_YR / YD)
        n = self.div(self.const(2 * math.pi), period_yrs)
        return self.addc(self.neg(self.mulc(self.div(MA, n), YD)), epoch)


def forward(D, ops, x):
    """The node values [N, W] of the tape at natural parameters x [D, W]."""
    x = np.asarray(x, dtype=np.float64).reshape(D, -1)
    f = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide, "ATAN2": np.arctan2, "NEG": np.negative, "SQRT": np.sqrt,
         "CBRT": np.cbrt, "EXP": np.exp, "LOG": np.log, "SIN": np.sin, "COS": np.cos}
    v = list(x)
    with np.errstate(all="ignore"):
        for j, (op, a, b, c) in enumerate(ops):
            assert a < D + j and b < D + j, (j, op, a, b)
            if op == "CONST":
                r = np.full(x.shape[1], c)
            elif op == "POWC":
                r = np.power(v[a], c)
            elif op == "MULC":
                r = v[a] * c
            elif op == "ADDC":
                r = v[a] + c
            else:
                r = f[op](v[a], v[b]) if op in BINARY else f[op](v[a])
            v.append(r)
    return np.stack(v)


def reverse(D, ops, vals, adj):
    """The reverse sweep: adj [N, W] holds the seeds on entry; returns it with every node's adjoint accumulated, ops taken last to first."""
    adj = np.array(adj, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(len(ops) - 1, -1, -1):
            op, a, b, c = ops[j]
            g, va, vb, r = adj[D + j], vals[a], vals[b], vals[D + j]
            if op == "ADD":
                adj[a] += g; adj[b] += g
            elif op == "SUB":
                adj[a] += g; adj[b] -= g
            elif op == "MUL":
                adj[a] += g * vb; adj[b] += g * va
            elif op == "DIV":
                adj[a] += g / vb; adj[b] -= g * r / vb
            elif op == "NEG":
                adj[a] -= g
            elif op == "SQRT":
                adj[a] += g * 0.5 / r
            elif op == "CBRT":
                adj[a] += g / (3.0 * r * r)
            elif op == "EXP":
                adj[a] += g * r
            elif op == "LOG":
                adj[a] += g / va
            elif op == "SIN":
                adj[a] += g * np.cos(va)
            elif op == "COS":
                adj[a] -= g * np.sin(va)
            elif op == "ATAN2":
                h = va * va + vb * vb
                adj[a] += g * vb / h; adj[b] -= g * va / h
            elif op == "POWC":
                adj[a] += g * c * np.power(va, c - 1.0)
            elif op == "MULC":
                adj[a] += g * c
            elif op == "ADDC":
                adj[a] += g
    return adj


def prior_dicts(priors):
    """host/priors.py priors as the dicts of tests/hmc_reference.py"""
    return [hr.prior(p.kind, *p.c_params()) for p in priors]


def expand(D, ops, binds):
    """(ops, nodes): the tape with every TPERI binding written out in primitives behind it, and the node each input reads."""
    t = Tape(D, ops)
    nodes = []
    for k, (kind, node, value) in enumerate(binds):
        if kind & 0xFFFF == BIND_TPERI:
            el = [binds[k - EL_TP + s][1] for s in range(N_EL)]
            node = t.tperi(node, value, el[EL_M], el[EL_E], el[EL_A], el[EL_I], el[EL_W], el[EL_O])
        nodes.append(node)
    return t.ops, nodes


def values(priors, ops, theta_t, nodes):
    """The values [n, W] of the nodes `nodes` at θ_t [D, W]."""
    pr = prior_dicts(priors)
    theta_t = np.asarray(theta_t, dtype=np.float64)
    x = np.stack([hr.invlink(p, theta_t[d])[0] for d, p in enumerate(pr)])
    return forward(len(pr), ops, x)[list(nodes)]


def logpost(oracle, obs_tables, planets, priors, ops, binds, terms, theta_t, grad=True):
    """(ℓπ [W], ∇ℓπ [D, W] or None, inputs [n_in, W]) of the program at θ_t [D, W] by the rules of octo_draws_program_logpost_device."""
    pr = prior_dicts(priors)
    D = len(pr)
    theta_t = np.asarray(theta_t, dtype=np.float64).reshape(D, -1)
    W = theta_t.shape[1]
    with np.errstate(all="ignore"):
        xs = [hr.invlink(p, theta_t[d]) for d, p in enumerate(pr)]
        x, dx = np.stack([v for v, _ in xs]), np.stack([d for _, d in xs])
        prior, gprior = hr.logprior_t(pr, theta_t)
        ops_x, nodes = expand(D, ops, binds)
        vals = forward(D, ops_x, x)
        inputs = vals[nodes]
        n_el = len(planets) * N_EL
        ll, g_el, g_nu = oracle.oracle_eval(obs_tables, planets, inputs[:n_el], inputs[n_el:] if len(nodes) > n_el else None, grad=grad)
        t = np.zeros(W)
        for n in terms:
            t = t + vals[n]
        pp = np.where(np.all(np.isfinite(theta_t), axis=0), prior + t, -np.inf)
        lp = np.where(np.isfinite(pp), pp + ll, pp)
        lp = np.where(np.isnan(lp), -np.inf, lp)
        if not grad:
            return lp, None, inputs
        adj = np.zeros_like(vals)
        g_in = g_el if g_nu is None else np.concatenate([g_el, g_nu])
        for k, n in enumerate(nodes):
            adj[n] += g_in[k]
        for n in terms:
            adj[n] += 1.0
        adj = reverse(D, ops_x, vals, adj)
        g = adj[:D] * dx + gprior
        return lp, np.where(np.isfinite(lp)[None, :], g, 0.0), inputs
