"""
Expression programs (include/octofitter_hip_draws.h, "Derived variables") without a device: the NumPy restatement the GPU suite holds the
kernels to (tests/program_reference.py) against mpmath at 40 digits, the tracer of host/derived.py against the op lists it must produce,
the two C structs against their ctypes twins, and the new work layout on host memory (tests/program_layout_check.cpp, in the manner of
tests/test_pt_layout.py). CPU suite: no GPU, nothing but ctypes structs loaded into Python.
"""
import json
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import program_reference as pref

ROOT = Path(__file__).resolve().parent.parent


def every_opcode_tape():
    """D = 3. Every opcode; node s (x0·x1) has three consumers; node `out0` is bound to two inputs. The operands are chosen away from
    cancellation — every sum adds terms of one sign or of very different size, no argument sits near a zero of its function — so that the
    FP64 sweep keeps rel 1e-12 against 40 digits."""
    t = pref.Tape(3)
    s = t.mul(0, 1)                      # three consumers: the next three ops
    u = t.sqrt(s)
    v = t.log(s)
    w = t.exp(t.mulc(s, 0.25))
    c = t.const(1.75)
    q = t.div(t.add(u, c), 2)            # (√s + 1.75)/x2
    r = t.cbrt(t.addc(q, 3.0))
    sn, cs = t.sin(0), t.cos(1)
    at = t.atan2(sn, cs)
    pw = t.powc(2, 1.5)
    ng = t.neg(t.sub(pw, t.mulc(w, 40.0)))      # 40·w − x2^1.5: w ≈ 1.3, x2^1.5 ≈ 3
    out0 = t.add(t.mul(r, at), v)
    out1 = t.mul(ng, out0)
    assert {op for op, *_ in t.ops} == set(pref.OPS)
    return t, [out0, out0, out1], s


def mp_forward(mp, D, ops, x):
    f = {"ADD": lambda a, b: a + b, "SUB": lambda a, b: a - b, "MUL": lambda a, b: a * b, "DIV": lambda a, b: a / b, "ATAN2": mp.atan2,
         "NEG": lambda a: -a, "SQRT": mp.sqrt, "CBRT": mp.cbrt, "EXP": mp.exp, "LOG": mp.log, "SIN": mp.sin, "COS": mp.cos}
    v = list(x)
    for op, a, b, c in ops:
        v.append(mp.mpf(c) if op == "CONST" else v[a] ** mp.mpf(c) if op == "POWC" else v[a] * mp.mpf(c) if op == "MULC" else v[a] + mp.mpf(c) if op == "ADDC"
                 else f[op](v[a], v[b]) if op in pref.BINARY else f[op](v[a]))
    return v


def check_sweep(ops, D, outs, weights, x, rtol):
    """∂(Σ weight_k · node outs[k])/∂x by the reverse sweep against mpmath.diff at 40 digits"""
    import mpmath as mp
    mp.mp.dps = 40
    x = np.asarray(x, dtype=np.float64)
    vals = pref.forward(D, ops, x[:, None])
    adj = np.zeros_like(vals)
    for n, wgt in zip(outs, weights):
        adj[n] += wgt
    got = pref.reverse(D, ops, vals, adj)[:D, 0]
    F = lambda *xs: sum(mp.mpf(wgt) * mp_forward(mp, D, ops, xs)[n] for n, wgt in zip(outs, weights))      # noqa: E731
    for d in range(D):
        want = mp.diff(F, tuple(mp.mpf(float(v)) for v in x), tuple(1 if k == d else 0 for k in range(D)))
        assert abs(mp.mpf(float(got[d])) - want) <= rtol * abs(want), (d, got[d], want)
    return vals


def test_reverse_sweep_against_mpmath_on_every_opcode():
    t, outs, shared = every_opcode_tape()
    assert sum(1 for op, a, b, _ in t.ops if a == shared or (op in pref.BINARY and b == shared)) == 3
    assert outs[0] == outs[1]
    check_sweep(t.ops, 3, outs, [0.7, 1.9, 0.3], [1.3, 0.8, 2.1], 1e-12)


def test_tperi_tape_is_the_reference_expression(pkg):
    """The TPERI binding of the restatement: its value against host/model.py: _tperi, its gradient against mpmath. tp − θ_epoch is a
    difference of the size of a period, so the gradient bar here is the GPU suite's 1e-9, not the sweep's 1e-12."""
    from octofitter_jl_amd.host.model import _tperi
    x = [0.9, 1.1, 0.3, 12.0, 0.7, 2.2, 1.4]      # θ, M, e, a, i, ω, Ω
    t = pref.Tape(7)
    tp = t.tperi(0, 50000.0, 1, 2, 3, 4, 5, 6)
    vals = check_sweep(t.ops, 7, [tp], [1.0], x, 1e-9)
    want = _tperi(x[0], 50000.0, *x[1:])
    assert abs(vals[tp, 0] - want) <= 1e-12 * abs(want), (vals[tp, 0], want)


def test_tracer_lowers_to_the_expected_op_lists(pkg):
    d = pkg.derived
    M, P, x, y = d.theta(0), d.theta(1), d.theta(2), d.theta(3)
    assert d.lower(d.cbrt(M * P ** 2), 4) == ([("POWC", 1, 0, 2.0), ("MUL", 0, 4, 0.0), ("CBRT", 5, 0, 0.0)], 6)
    tau = d.atan(y, x) * (1.0 / (2 * math.pi))
    ops, node = d.lower(tau * P * 365.25 + 58000.0, 4)
    assert ops == [("ATAN2", 3, 2, 0.0), ("MULC", 4, 0, 1.0 / (2 * math.pi)), ("MUL", 5, 1, 0.0), ("MULC", 6, 0, 365.25), ("ADDC", 7, 0, 58000.0)] and node == 8
    # a variable referenced twice is one node; constant sub-expressions fold
    a = d.cbrt(M * P ** 2)
    prog = d.Program(4)
    n1 = prog.node(a * a + a)
    assert [op for op, *_ in prog.ops] == ["POWC", "MUL", "CBRT", "MUL", "ADD"] and prog.ops[3][1:3] == (6, 6) and prog.ops[4][1:3] == (7, 6) and n1 == 8
    assert d.lower(M * (2.0 * 3.0 + 1.0), 4) == ([("MULC", 0, 0, 7.0)], 4)
    assert d.lower(d.sqrt(d.Sym.of(4.0)) + M, 4) == ([("ADDC", 0, 0, 2.0)], 4)
    with pytest.raises(TypeError):
        bool(M > 1.0)
    with pytest.raises(TypeError):
        M ** P


def test_derived_variables_are_a_block_entry(pkg):
    d = pkg.derived
    block = pkg.variables(P=pkg.Uniform(1, 100), a=pkg.Derived(lambda b, system: d.cbrt(system.M * b.P ** 2)))
    assert isinstance(block["a"], pkg.Derived) and block["a"].n_args == 2
    with pytest.raises(TypeError):
        pkg.variables(a="cbrt(M)")


def test_structs_are_the_ctypes_ones(pkg, tmp_path):
    import ctypes as C
    d = pkg.derived
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "octofitter_hip_draws.h"\n'
                   'int main(void) { printf("[%zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %d, %d]\\n", sizeof(octo_draws_op), offsetof(octo_draws_op, a), '
                   'offsetof(octo_draws_op, b), offsetof(octo_draws_op, value), sizeof(octo_draws_bind), offsetof(octo_draws_bind, node), '
                   'offsetof(octo_draws_bind, value), offsetof(octo_draws_op, pad), OCTO_DRAWS_PROGRAM_MAX_OPS, OCTO_DRAWS_N_OPS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", "-o", str(exe), str(src)], check=True)
    got = json.loads(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    O, B = d.OctoDrawsOp, d.OctoDrawsBind
    assert got == [24, 4, 8, 16, 16, 4, 8, 12, d.PROGRAM_MAX_OPS, len(d.OPS)]
    assert got[:8] == [C.sizeof(O), O.a.offset, O.b.offset, O.value.offset, C.sizeof(B), B.node.offset, B.value.offset, O.pad.offset]
    header = (ROOT / "include" / "octofitter_hip_draws.h").read_text()
    defines = dict(line.split()[1:3] for line in header.splitlines() if line.startswith("#define OCTO_DRAWS_") and len(line.split()) >= 3)
    for k, name in enumerate(d.OPS):      # the opcodes of the header, the binding and the restatement
        assert defines[f"OCTO_DRAWS_OP_{name}"] == str(k), name
    assert d.OPS == pref.OPS and d.PROGRAM_MAX_OPS == pref.MAX_OPS and 64 + d.PROGRAM_MAX_OPS == 256
    assert (d.BIND_NODE, d.BIND_TPERI, d.BIND_FLAG_TI) == (pref.BIND_NODE, pref.BIND_TPERI, pref.BIND_FLAG_TI)


LAYOUT_SHAPES = [(1, 1, 9, 1, 64), (11, 40, 12, 1, 256), (64, 256, 96, 8, 64)]      # (D, N, n_in, P, ldw): the smallest, a usual one, the largest program
LAYOUT_NAMES = ["vals", "dx", "gpd", "inputs", "g_in", "gtp", "pp", "ll", "healed"]
LAYOUT_FORMULA = "(N + 2·D + 2·n_in + 7·P + 3)·ldw"


def test_work_layout_on_host_memory(tmp_path):
    exe = tmp_path / "program_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "program_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in LAYOUT_SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    reports = [json.loads(line) for line in r.stdout.splitlines()]
    assert [tuple(rep["shape"]) for rep in reports] == LAYOUT_SHAPES
    for rep, (D, N, n_in, P, ldw) in zip(reports, LAYOUT_SHAPES):
        assert rep["layout"] == "prog_work" and rep["size"] == (N + 2 * D + 2 * n_in + 7 * P + 3) * ldw, rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(LAYOUT_NAMES) and [p["name"] for p in parts] == LAYOUT_NAMES
        assert [p["len"] for p in parts] == [N * ldw, D * ldw, D * ldw, n_in * ldw, n_in * ldw, 7 * P * ldw, ldw, ldw, ldw]
        assert [p["elem"] for p in parts] == [8] * 8 + [4]
        assert all(p["tag_ok"] and p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]      # a double's room per element, whatever its width
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"]      # gapless, in order, inside the allocation
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == len(members)
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md", "octofitter.jl_amd/csrc/draws/octo_draws_layout.h"):
        assert LAYOUT_FORMULA in (ROOT / doc).read_text(), doc
