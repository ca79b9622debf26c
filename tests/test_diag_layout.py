"""
The work layout of the convergence diagnostics (csrc/draws/octo_draws_layout.h: DiagWork, diag_work) on host memory, in the manner of
tests/test_draws_layout.py and alone: tests/diag_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. It sizes the layout with a null base, lays it
out on exactly that many doubles, writes a tag to every element of every part and reads all of them back. Checked here: every tag survived,
the sanitizers were silent, the parts are the pinned ones, each starts on an 8-byte boundary with a double's room per element, they come
gapless in the order the struct declares them, and the size is the documented one. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

import diag_reference as ref

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(8, 1, 1), (9, 3, 2), (35, 257, 3), (400, 64, 2), (130, 1100, 1), (16, 2, 64)]      # (n, W, K)
NAMES = ["keys", "fkeys", "z", "zf", "mu", "var", "part", "rho", "q", "bad", "ok"]
FORMULA = "2K(P + S) + 10KM + 4K·T·(nblk + 1) + 5K"


def dims(n, W, K):
    N, M = n // 2, 2 * W
    S, P = N * M, 2048
    while P < S:
        P *= 2
    return K, P, S, M, -(-N // 16) * 16, -(-M // 256)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("diag_layout") / "diag_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "diag_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in dims(*shape)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_the_layout_ran_on_every_shape_with_the_documented_size(reports):
    assert [tuple(rep["shape"]) for rep in reports] == [dims(*shape) for shape in SHAPES]
    for rep, shape in zip(reports, SHAPES):
        K, P, S, M, T, nblk = rep["shape"]
        assert rep["layout"] == "diag_work" and rep["size"] == 2 * K * (P + S) + 10 * K * M + 4 * K * T * (nblk + 1) + 5 * K == ref.work_doubles(*shape), shape
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md", "octofitter.jl_amd/csrc/draws/octo_draws_layout.h"):
        assert FORMULA in (ROOT / doc).read_text(), doc


def test_the_parts_are_the_pinned_ones_gapless_aligned_and_in_declaration_order(reports):
    for rep in reports:
        K, P, S, M, T, nblk = rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(NAMES) == 11, rep["shape"]
        assert [p["name"] for p in parts] == NAMES
        assert [p["len"] for p in parts] == [K * P, K * P, K * S, K * S, 5 * K * M, 5 * K * M, 4 * K * T * nblk, 4 * K * T, 3 * K, K, K], rep["shape"]
        assert [p["elem"] for p in parts] == [8] * 9 + [4] * 2
        assert all(p["tag_ok"] for p in parts), [p["name"] for p in parts if not p["tag_ok"]]
        assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]      # a double's room per element, whatever its width
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == len(members)
