"""
The layout of the parallel-tempering statistics' block partials (csrc/draws/octo_draws_layout.h: PtPartials, pt_partials) on host memory, in
the manner of tests/test_slice_layout.py and alone: tests/pt_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. It sizes the layout with a null base, lays it
out on exactly that many doubles, writes a tag to every element of every part and reads all of them back. Checked here: every tag survived,
the sanitizers were silent, the parts are the pinned ones, each starts on an 8-byte boundary, they come gapless in the order the struct
declares them, and the size is the documented one. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 1), (7, 2), (63, 4), (4, 65536)]      # (P = T − 1, nblk): the smallest, several blocks, the top of T, the top of Cn
NAMES = ["A", "nf", "mf", "sf", "nb", "mb", "sb"]
FORMULA = "7·(T − 1)·⌈Cn/256⌉"


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pt_layout") / "pt_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "pt_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_the_layout_ran_on_every_shape_with_the_documented_size(reports):
    assert [tuple(rep["shape"]) for rep in reports] == SHAPES
    for rep, (P, nblk) in zip(reports, SHAPES):
        assert rep["layout"] == "pt_partials" and rep["size"] == 7 * P * nblk, (P, nblk)
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md"):
        assert FORMULA in (ROOT / doc).read_text(), doc
    assert "7·P·nblk" in (ROOT / "octofitter.jl_amd/csrc/draws/octo_draws_layout.h").read_text()


def test_the_parts_are_the_pinned_ones_gapless_aligned_and_in_declaration_order(reports):
    for rep in reports:
        P, nblk = rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(NAMES) == 7, rep["shape"]
        assert [p["name"] for p in parts] == NAMES
        assert [p["len"] for p in parts] == [P * nblk] * 7 and [p["elem"] for p in parts] == [8] * 7, rep["shape"]
        assert all(p["tag_ok"] for p in parts), [p["name"] for p in parts if not p["tag_ok"]]
        assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == len(members)
