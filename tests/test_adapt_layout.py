"""
The work-allocation layout the warm-up calls add to liboctofitter_hip_draws.so (moments_partials of csrc/draws/octo_draws_layout.h) on host
memory, by the method of tests/test_draws_layout.py: tests/adapt_layout_check.cpp includes that header alone, is compiled here as plain
C++17 with -fsanitize=address,undefined and run as a program of its own. Checked: every tag survived (no two parts overlap), the sanitizers
were silent (nothing out of bounds), every part starts on an 8-byte boundary, the parts come gapless in the order the struct declares them,
and the size is the one include/octofitter_hip_draws.h documents — ⌈W/256⌉·G·(2K + 1) doubles — computed here independently. CPU suite.
"""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 1, 1), (3, 5, 2), (7, 64, 64), (4, 3, 11)]      # (nblk, G, K)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("adapt_layout") / "adapt_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "adapt_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_moments_partials_ran_on_every_shape_with_the_documented_size(reports):
    assert [tuple(rep["shape"]) for rep in reports] == SHAPES and all(rep["layout"] == "moments_partials" for rep in reports)
    for rep in reports:
        nblk, G, K = rep["shape"]
        assert rep["size"] == nblk * G * (2 * K + 1), rep["shape"]
    text = (ROOT / "include" / "octofitter_hip_draws.h").read_text()
    assert "⌈W/256⌉·G·(2K + 1) doubles" in text


def test_parts_are_disjoint_aligned_and_in_declaration_order(reports):
    for rep in reports:
        nblk, G, K = rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == 3
        assert [p["name"] for p in parts] == ["cnt", "sum", "m2"] and [p["len"] for p in parts] == [nblk * G, nblk * G * K, nblk * G * K]
        assert all(p["tag_ok"] for p in parts), rep["shape"]
        assert all(p["offset"] % 8 == 0 and p["elem"] == 8 for p in parts)
        assert parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"]      # gapless, so in order and inside the allocation
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == 3
