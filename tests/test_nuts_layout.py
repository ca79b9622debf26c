"""
The work-allocation layout the no-U-turn sampler adds to liboctofitter_hip_draws.so (nuts_work of csrc/draws/octo_draws_layout.h) on host
memory, by the method of tests/test_adapt_layout.py: tests/nuts_layout_check.cpp includes that header alone, is compiled here as plain C++17
with -fsanitize=address,undefined and run as a program of its own. Checked: every tag survived (no two parts overlap), the sanitizers were
silent (nothing out of bounds), every part starts on an 8-byte boundary, the parts come gapless in the order the struct declares them (an
int32 element in a double's room), and the size is the one include/octofitter_hip_draws.h documents — ((14 + 2·max_depth)·D + 18)·ld doubles —
computed here independently. CPU suite.
"""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 1, 1), (14, 72, 4), (5, 65536, 5), (64, 3, 10), (3, 257, 2)]      # (D, ld, max_depth)
PLANES = ["trial", "pt", "qL", "pL", "gL", "qR", "pR", "gR", "prop", "sprop", "rho", "rho_s", "gpr", "glp"]
STACKS = ["ck_p", "ck_r"]
SCALARS = ["lp", "H0", "logw", "logw_s", "sum_acc", "prop_lp", "prop_lpt", "sprop_lp", "sprop_lpt", "out_lp", "out_lpt"]
COUNTERS = ["status", "depth", "n", "nleaf", "v", "sel", "ssel"]


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("nuts_layout") / "nuts_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "nuts_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_nuts_work_ran_on_every_shape_with_the_documented_size(reports):
    assert [tuple(rep["shape"]) for rep in reports] == SHAPES and all(rep["layout"] == "nuts_work" for rep in reports)
    for rep in reports:
        D, ld, md = rep["shape"]
        assert rep["size"] == ((14 + 2 * md) * D + 18) * ld, rep["shape"]
    for doc in (ROOT / "include" / "octofitter_hip_draws.h", ROOT / "DESIGN.md"):
        assert "((14 + 2·max_depth)·D + 18)·ld" in doc.read_text(), doc.name


def test_parts_are_disjoint_aligned_and_in_declaration_order(reports):
    names = PLANES + STACKS + SCALARS + COUNTERS
    for rep in reports:
        D, ld, md = rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(names) == 34
        assert [p["name"] for p in parts] == names
        assert [p["len"] for p in parts] == [D * ld] * 14 + [md * D * ld] * 2 + [ld] * 18
        assert [p["elem"] for p in parts] == [8] * 27 + [4] * 7
        assert all(p["tag_ok"] for p in parts), rep["shape"]
        assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]      # a double's room per element, whatever its size
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"]      # gapless, so in order and inside the allocation
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == len(names)
