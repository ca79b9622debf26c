"""
Derived variables of a variable block as expression programs (include/octofitter_hip_draws.h, "Derived variables").

    variables(M=…, P=Uniform(1, 100), τ=UniformCircular(1.0),
              a=Derived(lambda b, system: cbrt(system.M * b.P ** 2)),
              tp=Derived(lambda b, system: b.τ * b.P * 365.25 + 58000.0))

mirrors the deterministic `=` lines of `@variables begin … end` (src/macros.jl): a straight-line list of arithmetic on θ, evaluated in
declaration order. `fn` is TRACED, not compiled: it is called once with symbolic values (Sym) for the variables declared before it in its
own block and — second argument, optional — the system's block, and what it returns is lowered to the op list the device interprets
(Program). Constant sub-expressions fold, a value referenced twice is one node. Control flow and comparisons on a Sym are refused: a
program has none.
"""
from __future__ import annotations

import ctypes as C
import inspect
import math

import numpy as np

OPS = ("CONST", "ADD", "SUB", "MUL", "DIV", "NEG", "SQRT", "CBRT", "EXP", "LOG", "SIN", "COS", "ATAN2", "POWC", "MULC", "ADDC")      # OCTO_DRAWS_OP_*
OP = {name: k for k, name in enumerate(OPS)}
BINARY = ("ADD", "SUB", "MUL", "DIV", "ATAN2")
PROGRAM_MAX_OPS = 192          # OCTO_DRAWS_PROGRAM_MAX_OPS
BIND_NODE, BIND_TPERI, BIND_FLAG_TI = 0, 1, 65536      # OCTO_DRAWS_BIND_*
LOG2PI = 1.8378770664093454835606594728112


class OctoDrawsOp(C.Structure):
    _fields_ = [("op", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("pad", C.c_int32), ("value", C.c_double)]


class OctoDrawsBind(C.Structure):
    _fields_ = [("kind", C.c_int32), ("node", C.c_int32), ("value", C.c_double)]


_FOLD = {"ADD": lambda a, b: a + b, "SUB": lambda a, b: a - b, "MUL": lambda a, b: a * b, "DIV": lambda a, b: a / b, "NEG": lambda a: -a,
         "SQRT": math.sqrt, "CBRT": lambda a: float(np.cbrt(a)),"EXP": math.exp, "LOG": math.log, "SIN": math.sin, "COS": math.cos, "ATAN2": math.atan2}


class Sym:
    """A symbolic value: ("theta", d) a natural parameter, ("const", value), or (op, operands…[, value])."""
    __slots__ = ("op", "args", "value")

    def __init__(self, op, args=(), value=0.0):
        self.op, self.args, self.value = op, tuple(args), float(value)

    @staticmethod
    def of(x):
        if isinstance(x, Sym):
            return x
        if isinstance(x, (int, float, np.floating, np.integer)):
            return Sym("CONST", (), float(x))
        raise TypeError(f"a derived variable is arithmetic on variables and numbers, not {type(x).__name__}")

    @property
    def is_const(self):
        return self.op == "CONST"

    def __add__(self, o): return _binary("ADD", self, o)
    def __radd__(self, o): return _binary("ADD", o, self)
    def __sub__(self, o): return _binary("SUB", self, o)
    def __rsub__(self, o): return _binary("SUB", o, self)
    def __mul__(self, o): return _binary("MUL", self, o)
    def __rmul__(self, o): return _binary("MUL", o, self)
    def __truediv__(self, o): return _binary("DIV", self, o)
    def __rtruediv__(self, o): return _binary("DIV", o, self)
    def __neg__(self): return _unary("NEG", self)
    def __pos__(self): return self

    def __pow__(self, o):
        o = Sym.of(o)
        if not o.is_const:
            raise TypeError("a derived variable takes a power with a constant exponent only")
        if self.is_const:
            return Sym("CONST", (), self.value ** o.value)
        return Sym("POWC", (self,), o.value)

    def __bool__(self):
        raise TypeError("a derived variable has no control flow: comparisons and `if` on a traced value are not part of a program")

    __lt__ = __le__ = __gt__ = __ge__ = lambda self, o: self.__bool__()
    __hash__ = object.__hash__


def _unary(op, a):
    a = Sym.of(a)
    return Sym("CONST", (), _FOLD[op](a.value)) if a.is_const else Sym(op, (a,))


def _binary(op, a, b):
    a, b = Sym.of(a), Sym.of(b)
    if a.is_const and b.is_const:
        return Sym("CONST", (), _FOLD[op](a.value, b.value))
    # a constant operand of + − · / becomes the one-operand form: no CONST node, no second LDS read
    if op == "ADD" and (a.is_const or b.is_const):
        return Sym("ADDC", (b if a.is_const else a,), a.value if a.is_const else b.value)
    if op == "MUL" and (a.is_const or b.is_const):
        return Sym("MULC", (b if a.is_const else a,), a.value if a.is_const else b.value)
    if op == "SUB" and b.is_const:
        return Sym("ADDC", (a,), -b.value)
    if op == "DIV" and b.is_const:
        return Sym("MULC", (a,), 1.0 / b.value)
    return Sym(op, (a, b))


def sqrt(x): return _unary("SQRT", x)
def cbrt(x): return _unary("CBRT", x)
def exp(x): return _unary("EXP", x)
def log(x): return _unary("LOG", x)
def sin(x): return _unary("SIN", x)
def cos(x): return _unary("COS", x)
def atan(y, x): return _binary("ATAN2", y, x)      # the reference spells atan2 `atan(y, x)`


def theta(d):
    """The natural parameter x_d = invlink_d(θ_t[d]): node d of every program."""
    return Sym("theta", (), d)


def unit_length(x, y):
    """logpdf(LogNormal(log(1.0), 0.1), sqrt(x² + y²)) in primitives: the UnitLengthPrior of a UniformCircular pair (src/variables.jl:309-323)."""
    r = sqrt(x * x + y * y)
    z = log(r) * 10.0
    return (-(z * z + LOG2PI)) * 0.5 - log(r * 0.1)


class Derived:
    """`name = f(earlier variables)` of a variable block. fn(block) or fn(block, system): the arguments give the variables declared so far by
    attribute (b.P) or by item (b["P"]); fn returns arithmetic on them."""

    def __init__(self, fn):
        if not callable(fn):
            raise TypeError("Derived takes a function of the block's variables")
        self.fn = fn
        self.n_args = len([p for p in inspect.signature(fn).parameters.values() if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)])
        if self.n_args not in (1, 2):
            raise TypeError("Derived: fn takes the block, or the block and the system's block")

    def trace(self, block, system):
        return Sym.of(self.fn(block) if self.n_args == 1 else self.fn(block, system))


class Namespace:
    """The variables a Derived sees: by attribute or by item."""

    def __init__(self, what):
        object.__setattr__(self, "_what", what)
        object.__setattr__(self, "_vars", {})

    def __getattr__(self, name):
        try:
            return self._vars[name]
        except KeyError:
            raise AttributeError(f"{self._what}: no variable `{name}` is declared before this one") from None

    __getitem__ = __getattr__

    def __contains__(self, name):
        return name in self._vars

    def _set(self, name, sym):
        self._vars[name] = sym


class Program:
    """The op list under construction: node(sym) lowers a Sym (once: the same Sym, or the same natural parameter, is one node) and returns
    its node index."""

    def __init__(self, D):
        self.D = int(D)
        self.ops: list[tuple] = []          # (op name, a, b, value)
        self.terms: list[int] = []
        self._node: dict[int, int] = {}     # id(Sym) -> node
        self._keep: list[Sym] = []          # the Syms behind the ids stay alive
        self._const: dict[float, int] = {}

    @property
    def n_nodes(self):
        return self.D + len(self.ops)

    def _emit(self, op, a=0, b=0, value=0.0):
        self.ops.append((op, int(a), int(b), float(value)))
        return self.n_nodes - 1

    def node(self, sym):
        sym = Sym.of(sym)
        if sym.op == "theta":
            return int(sym.value)
        if id(sym) in self._node:
            return self._node[id(sym)]
        if sym.is_const:
            key = np.float64(sym.value).tobytes()
            if key not in self._const:
                self._const[key] = self._emit("CONST", value=sym.value)
            n = self._const[key]
        else:
            operands = [self.node(a) for a in sym.args]
            n = self._emit(sym.op, *(operands + [0] * (2 - len(operands))), value=sym.value)
        self._node[id(sym)] = n
        self._keep.append(sym)
        return n

    def term(self, sym):
        self.terms.append(self.node(sym))

    def evaluate(self, x):
        """The node values [N, W] at natural parameters x [D, W], in NumPy: the host twin of the forward sweep."""
        x = np.asarray(x, dtype=np.float64).reshape(self.D, -1)
        f = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide, "ATAN2": np.arctan2, "NEG": np.negative, "SQRT": np.sqrt,
             "CBRT": np.cbrt, "EXP": np.exp, "LOG": np.log, "SIN": np.sin, "COS": np.cos}
        v = list(x)
        with np.errstate(all="ignore"):
            for op, a, b, c in self.ops:
                v.append(np.full(x.shape[1], c) if op == "CONST" else v[a] ** c if op == "POWC" else v[a] * c if op == "MULC" else v[a] + c if op == "ADDC"
                         else f[op](v[a], v[b]) if op in BINARY else f[op](v[a]))
        return np.stack(v)

    def op_names(self):
        return [(op, a, b, v) for op, a, b, v in self.ops]

    def c_arrays(self, binds):
        """(ops, n_ops, binds, n_binds, terms, n_terms) as ctypes arrays; binds: [(kind, node, value)]."""
        ops = (OctoDrawsOp * max(len(self.ops), 1))(*[OctoDrawsOp(OP[op], a, b, 0, v) for op, a, b, v in self.ops])
        bs = (OctoDrawsBind * max(len(binds), 1))(*[OctoDrawsBind(int(k), int(n), float(v)) for k, n, v in binds])
        ts = (C.c_int32 * max(len(self.terms), 1))(*self.terms)
        return ops, len(self.ops), bs, len(binds), ts, len(self.terms)


def lower(expr, D):
    """The op list [(op name, a, b, value)] of one expression over natural parameters theta(0) … theta(D − 1), and its node."""
    p = Program(D)
    n = p.node(expr)
    return p.op_names(), n
