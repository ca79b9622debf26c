"""
The work layouts of nested sampling (csrc/draws/octo_draws_layout.h: NestedWork / nested_work, NestedCull / nested_cull) on host memory, in
the manner of tests/test_slice_layout.py and alone: tests/nested_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. It sizes each layout with a null base, lays it
out on exactly that many doubles, writes a tag to every element of every part and reads all of them back. Checked here: every tag survived,
the sanitizers were silent, the parts are the pinned ones, each starts on an 8-byte boundary with a double's room per element, they come
gapless in the order the struct declares them, and the sizes are the documented ones. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 2), (14, 72), (64, 3), (3, 257), (14, 4096)]      # (D, ld); the cull's order at K = ld
PLANES = ["trial", "gpr", "u"]
SCALARS = ["lp", "L", "R", "xp", "keep"]
COUNTERS = ["status", "j", "phase", "s", "J", "Kr", "n_eval", "n_step", "n_shrink", "n_stuck"]
FORMULA = "(3·D + 15)·ld"


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("nested_layout") / "nested_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "nested_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    reps = [json.loads(line) for line in r.stdout.splitlines()]
    return [rep for rep in reps if rep["layout"] == "nested_work"], [rep for rep in reps if rep["layout"] == "nested_cull"]


def test_the_layouts_ran_on_every_shape_with_the_documented_sizes(reports):
    work, cull = reports
    assert [tuple(rep["shape"]) for rep in work] == SHAPES == [tuple(rep["shape"]) for rep in cull]
    for rep, (D, ld) in zip(work, SHAPES):
        assert rep["size"] == (3 * D + 15) * ld, (D, ld)
    for rep, (_D, K) in zip(cull, SHAPES):
        assert rep["size"] == K, K
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md", "octofitter.jl_amd/csrc/draws/octo_draws_layout.h"):
        assert FORMULA in (ROOT / doc).read_text(), doc


def check_parts(rep, names, lens, elems):
    parts = rep["parts"]
    assert len(parts) == rep["members"] == len(names), rep["shape"]
    assert [p["name"] for p in parts] == names
    assert [p["len"] for p in parts] == lens, rep["shape"]
    assert [p["elem"] for p in parts] == elems
    assert all(p["tag_ok"] for p in parts), [p["name"] for p in parts if not p["tag_ok"]]
    assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
    ends = [p["offset"] + 8 * p["len"] for p in parts]      # a double's room per element, whatever its width
    assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
    members = [p["member"] for p in parts]
    assert members == sorted(members) and len(set(members)) == len(members)


def test_the_parts_are_the_pinned_ones_gapless_aligned_and_in_declaration_order(reports):
    work, cull = reports
    for rep in work:
        D, ld = rep["shape"]
        check_parts(rep, PLANES + SCALARS + COUNTERS, [D * ld] * 3 + [ld] * 15, [8] * 8 + [4] * 10)
    for rep in cull:
        check_parts(rep, ["order"], [rep["shape"][1]], [4])
