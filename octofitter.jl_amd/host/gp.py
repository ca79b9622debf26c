"""
Celerite kernels for a Gaussian-process RV observation (include/octofitter_hip_draws.h, "The nineteenth").

    StarAbsoluteRVObs(table, name="hires", variables=variables(offset=Normal(0, 10), jitter=LogUniform(0.1, 10), log_S0=Uniform(0, 4),
                                                                Q=Uniform(0.6, 5), w0=LogUniform(0.05, 1)),
                      gaussian_process=lambda θ: Celerite(SHOTerm(S0=derived.exp(θ.log_S0), Q=θ.Q, w0=θ.w0)))

mirrors the reference's `gaussian_process = θ_obs -> Celerite.CeleriteGP(Celerite.SHOTerm(log(S0), log(Q), log(ω0)))`, with the terms in the
library's own parameters (S0, Q, ω0; a, c; a, b, c, d): a log-parameterised variable is `derived.exp` of it. The closure is TRACED, not
compiled, as a Derived variable is (host/derived.py): it is called with symbolic values for θ_obs and what it returns names, per term, the
expression-program nodes the device reads the hyperparameters from. Sums of terms and of kernels are kernels.
"""
from __future__ import annotations

from . import derived

REAL, COMPLEX, SHO = 0, 1, 2      # OCTO_DRAWS_GP_REAL, _COMPLEX, _SHO


class Term:
    kind = None
    names = ()

    def __init__(self, *params):
        if len(params) != len(self.names):
            raise TypeError(f"{type(self).__name__} takes {', '.join(self.names)}")
        self.params = tuple(derived.Sym.of(p) for p in params)      # numbers become constants of the program

    def __add__(self, other):
        return Celerite(self) + other

    __radd__ = lambda self, other: Celerite(other) + self


class RealTerm(Term):
    """k(τ) = a·exp(−c·τ)"""
    kind, names = REAL, ("a", "c")

    def __init__(self, a, c):
        super().__init__(a, c)


class ComplexTerm(Term):
    """k(τ) = exp(−c·τ)·(a·cos dτ + b·sin dτ)"""
    kind, names = COMPLEX, ("a", "b", "c", "d")

    def __init__(self, a, b, c, d):
        super().__init__(a, b, c, d)


class SHOTerm(Term):
    """the stochastically driven damped oscillator with power S0 at ω0 and quality factor Q; either side of Q = ½ walker by walker"""
    kind, names = SHO, ("S0", "Q", "w0")

    def __init__(self, S0, Q, w0):
        super().__init__(S0, Q, w0)


class Celerite:
    """A sum of terms: the kernel a `gaussian_process` closure returns."""

    def __init__(self, *terms):
        flat = []
        for t in terms:
            if isinstance(t, Celerite):
                flat += t.terms
            elif isinstance(t, Term):
                flat.append(t)
            else:
                raise TypeError(f"a Celerite kernel is a sum of RealTerm, ComplexTerm and SHOTerm, not {type(t).__name__}")
        if not flat:
            raise TypeError("a Celerite kernel needs at least one term")
        self.terms = flat

    def __add__(self, other):
        return Celerite(self, other)

    __radd__ = lambda self, other: Celerite(other, self)

    @property
    def kinds(self):
        return [t.kind for t in self.terms]

    @property
    def params(self):
        """the hyperparameters in term order: what the device's hyper rows hold"""
        return [p for t in self.terms for p in t.params]


# ---- dense kernels (include/octofitter_hip_draws.h, "The twentieth"): the reference's AbstractGPs / KernelFunctions kernels, no semiseparable form
#
#     gaussian_process=lambda θ: GP(QuasiPeriodicTerm(a=derived.exp(θ.log_η1), l=θ.η2, P=θ.η3, r=θ.η4))
#
# mirrors `θ_obs -> GP(θ_obs.η₁^2 * (SqExponentialKernel() ∘ ScaleTransform(1/θ_obs.η₂)) * (PeriodicKernel(r=[θ_obs.η₄]) ∘ ScaleTransform(1/θ_obs.η₃)))`.
SE, MATERN32, MATERN52, PERIODIC, QUASIPERIODIC = 16, 17, 18, 19, 20      # OCTO_DRAWS_GP_SE … _QUASIPERIODIC


class DenseTerm:
    kind = None
    names = ()

    def __init__(self, *params):
        if len(params) != len(self.names):
            raise TypeError(f"{type(self).__name__} takes {', '.join(self.names)}")
        self.params = tuple(derived.Sym.of(p) for p in params)

    def __add__(self, other):
        return DenseKernel(self) + other

    __radd__ = lambda self, other: DenseKernel(other) + self


class SqExpTerm(DenseTerm):
    """k(τ) = a²·exp(−τ²/(2l²))"""
    kind, names = SE, ("a", "l")

    def __init__(self, a, l):
        super().__init__(a, l)


class Matern32Term(DenseTerm):
    """k(τ) = a²·(1 + u)·exp(−u), u = √3·τ/l"""
    kind, names = MATERN32, ("a", "l")

    def __init__(self, a, l):
        super().__init__(a, l)


class Matern52Term(DenseTerm):
    """k(τ) = a²·(1 + u + u²/3)·exp(−u), u = √5·τ/l"""
    kind, names = MATERN52, ("a", "l")

    def __init__(self, a, l):
        super().__init__(a, l)


class PeriodicTerm(DenseTerm):
    """k(τ) = a²·exp(−sin²(πτ/P)/(2r²))"""
    kind, names = PERIODIC, ("a", "P", "r")

    def __init__(self, a, P, r):
        super().__init__(a, P, r)


class QuasiPeriodicTerm(DenseTerm):
    """k(τ) = a²·exp(−τ²/(2l²) − sin²(πτ/P)/(2r²)): the reference's RV tutorial kernel for an active star"""
    kind, names = QUASIPERIODIC, ("a", "l", "P", "r")

    def __init__(self, a, l, P, r):
        super().__init__(a, l, P, r)


class DenseKernel:
    """A sum of dense terms. A celerite term does not add to it: the device factors one kind of kernel a table."""

    def __init__(self, *terms):
        flat = []
        for t in terms:
            if isinstance(t, DenseKernel):
                flat += t.terms
            elif isinstance(t, DenseTerm):
                flat.append(t)
            else:
                raise TypeError(f"a dense kernel is a sum of SqExpTerm, Matern32Term, Matern52Term, PeriodicTerm and QuasiPeriodicTerm, not {type(t).__name__}")
        if not flat:
            raise TypeError("a dense kernel needs at least one term")
        self.terms = flat

    def __add__(self, other):
        return DenseKernel(self, other)

    __radd__ = lambda self, other: DenseKernel(other, self)

    kinds = Celerite.kinds
    params = Celerite.params


def as_kernel(x):
    """x as a Celerite or a DenseKernel (a single term becomes a sum of one), or None"""
    if isinstance(x, Term):
        return Celerite(x)
    if isinstance(x, DenseTerm):
        return DenseKernel(x)
    return x if isinstance(x, (Celerite, DenseKernel)) else None


def GP(kernel):
    """Pass-through, so that a closure reads as the reference's `GP(kernel)` does."""
    k = as_kernel(kernel)
    if k is None:
        raise TypeError(f"GP takes a kernel of this module, not {type(kernel).__name__}")
    return k


def probe(closure, names):
    """The kernel `closure` returns for symbolic θ_obs with the variables `names` — a Celerite or a DenseKernel — or None when it is neither (or cannot
    be traced)."""
    ns = derived.Namespace("θ_obs")
    for k, name in enumerate(names):
        ns._set(name, derived.theta(k))
    try:
        kernel = closure(ns)
    except (TypeError, AttributeError):
        return None
    return as_kernel(kernel)
