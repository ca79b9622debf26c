"""
The work layout of differential evolution (csrc/draws/octo_draws_layout.h: DeWork, de_work) on host memory, in the manner of
tests/test_slice_layout.py and alone: tests/de_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. It sizes the layout with a null base, lays it
out on exactly that many doubles, writes a tag to every element of every part and reads all of them back. Checked here: every tag survived,
the sanitizers were silent, the parts are the pinned ones, each starts on an 8-byte boundary with a double's room per element, they come
gapless in the order the struct declares them, and the size is the documented one. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

import de_reference      # noqa: F401  (the restatement this layout serves)

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 4), (14, 72), (64, 5), (3, 257)]      # (D, ld)
PLANES = ["pop0", "pop1", "trial0", "trial1", "gpr"]
SCALARS = ["lp", "f0", "f1", "tlpt0", "tlpt1", "lpt", "F", "CR", "Ft", "CRt"]
COUNTERS = ["n_accept", "improved"]
FORMULA = "(5·D + 12)·ld"


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("de_layout") / "de_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "de_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_the_layout_ran_on_every_shape_with_the_documented_size(reports):
    assert [tuple(rep["shape"]) for rep in reports] == SHAPES
    for rep, (D, ld) in zip(reports, SHAPES):
        assert rep["layout"] == "de_work" and rep["size"] == (5 * D + 12) * ld, (D, ld)
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md", "octofitter.jl_amd/csrc/draws/octo_draws_layout.h"):
        assert FORMULA in (ROOT / doc).read_text(), doc


def test_the_parts_are_the_pinned_ones_gapless_aligned_and_in_declaration_order(reports):
    names = PLANES + SCALARS + COUNTERS
    for rep in reports:
        D, ld = rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(names) == 17, rep["shape"]
        assert [p["name"] for p in parts] == names
        assert [p["len"] for p in parts] == [D * ld] * 5 + [ld] * 12, rep["shape"]
        assert [p["elem"] for p in parts] == [8] * 15 + [4] * 2
        assert all(p["tag_ok"] for p in parts), [p["name"] for p in parts if not p["tag_ok"]]
        assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]      # a double's room per element, whatever its width
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == len(members)
