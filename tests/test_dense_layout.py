"""
The block partials of the pooled covariance (csrc/draws/octo_draws_layout.h: CovPartials / cov_partials) on host memory, in the manner of
tests/test_nested_layout.py and alone: tests/dense_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. Checked here: every tag survived, the sanitizers
were silent, the parts are the pinned ones, each starts on an 8-byte boundary, they come gapless in the order the struct declares them, and the
size is the documented one. The samplers' dense kernels need no layout of their own: HmcWork and NutsWork are what they were
(tests/test_draws_layout.py). CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 1), (1, 64), (4, 11), (3, 2), (65536, 14)]      # (nblk, K)
FORMULA = "nblk·(1 + K + K(K+1)/2)"


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dense_layout") / "dense_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "dense_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_the_layout_ran_on_every_shape_with_the_documented_size(reports):
    assert [tuple(rep["shape"]) for rep in reports] == SHAPES and all(rep["layout"] == "cov_partials" for rep in reports)
    for rep, (nblk, K) in zip(reports, SHAPES):
        assert rep["size"] == nblk * (1 + K + K * (K + 1) // 2), (nblk, K)
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md", "octofitter.jl_amd/csrc/draws/octo_draws_layout.h"):
        assert FORMULA in (ROOT / doc).read_text(), doc


def test_the_parts_are_the_pinned_ones_gapless_aligned_and_in_declaration_order(reports):
    for rep in reports:
        nblk, K = rep["shape"]
        parts = rep["parts"]
        assert len(parts) == rep["members"] == 3
        assert [p["name"] for p in parts] == ["cnt", "sum", "m2"]
        assert [p["len"] for p in parts] == [nblk, nblk * K, nblk * (K * (K + 1) // 2)]
        assert [p["elem"] for p in parts] == [8, 8, 8]
        assert all(p["tag_ok"] for p in parts), [p["name"] for p in parts if not p["tag_ok"]]
        assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"]
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == 3
