"""
The layout of the variational leg's reference table (csrc/draws/octo_draws_layout.h: RefTable, ref_table) on host memory, in the manner of
tests/test_pt_layout.py and alone: tests/vref_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. Checked here: every tag survived, the sanitizers
were silent, the parts are the pinned ones, gapless, aligned and in declaration order, the size is the documented 15·D, and
octo_draws_reference_doubles answers the layout program's size. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

import draws_build
import vref_reference as vr

ROOT = Path(__file__).resolve().parent.parent
DIMS = [1, 11, 64]
SHAPES = [(D, vr.PRIOR_NC, vr.IC_N) for D in DIMS] + [(3, 2, 7)]      # (D, nc, icn): the library's constants, and a shape that tells the parts apart
NAMES = ["priors", "pc", "ic", "mean", "sd"]
FORMULA = "15·D"


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vref_layout") / "vref_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "vref_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_the_layout_ran_on_every_shape_with_the_documented_size(reports):
    assert [tuple(rep["shape"]) for rep in reports] == SHAPES
    for rep, (D, nc, icn) in zip(reports, SHAPES):
        assert rep["layout"] == "ref_table" and rep["size"] == (5 + nc + icn + 2) * D, (D, nc, icn)
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md", "octofitter.jl_amd/csrc/draws/octo_draws_layout.h"):
        assert FORMULA in (ROOT / doc).read_text(), doc


def test_the_parts_are_the_pinned_ones_gapless_aligned_and_in_declaration_order(reports):
    for rep in reports:
        D, nc, icn = rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(NAMES) == 5, rep["shape"]
        assert [p["name"] for p in parts] == NAMES
        assert [p["len"] for p in parts] == [5 * D, nc * D, icn * D, D, D] and [p["elem"] for p in parts] == [8] * 5, rep["shape"]
        assert all(p["tag_ok"] for p in parts), [p["name"] for p in parts if not p["tag_ok"]]
        assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == len(members)
        if (nc, icn) == (vr.PRIOR_NC, vr.IC_N):
            assert {p["name"]: (p["offset"] // 8, p["len"]) for p in parts} == vr.parts(D)      # the restatement's offsets


def test_reference_doubles_is_the_layout_programs_size(pkg, reports):
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    for rep in reports:
        D, nc, icn = rep["shape"]
        if (nc, icn) == (vr.PRIOR_NC, vr.IC_N):
            assert lib.octo_draws_reference_doubles(D) == rep["size"] == vr.table_doubles(D), D
    assert lib.octo_draws_reference_doubles(0) == 0 and lib.octo_draws_reference_doubles(-3) == 0
