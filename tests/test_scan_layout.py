"""
The work layouts of along-scan absolute astrometry (csrc/draws/octo_draws_layout.h: ScanWork / scan_work, ScanStaging / scan_staging) on host memory,
in the manner of tests/test_ofti_draws_layout.py and alone: tests/scan_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. It sizes each layout with a null base, lays it out on
exactly that many doubles, writes a tag to every element of every part and reads all of them back. Checked here: every tag survived, the sanitizers
were silent, the parts are the pinned ones, each starts on an 8-byte boundary, they come gapless in the order the struct declares them, and the size
is the documented one. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

import scan_reference      # noqa: F401  (the restatement this layout serves)

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 19, 64, 1, 0), (4, 27, 64, 1, 5), (4, 89, 192, 8, 6), (38, 29, 10048, 2, 5)]      # (n_tasks, n_sums, ldw, P, K)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("scan_layout") / "scan_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "scan_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def check_parts(rep, names, lens):
    parts = rep["parts"]
    assert len(parts) == rep["members"] == len(names), rep["shape"]
    assert [p["name"] for p in parts] == names and [p["len"] for p in parts] == lens, rep["shape"]
    assert all(p["elem"] == 8 and p["tag_ok"] and p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
    ends = [p["offset"] + 8 * p["len"] for p in parts]
    assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
    members = [p["member"] for p in parts]
    assert members == sorted(members) and len(set(members)) == len(members)


def test_the_work_array_is_the_partials_and_the_solve_with_the_documented_size(reports):
    for rep, (n_tasks, n_sums, ldw, _, _) in zip(reports[0::2], SHAPES):
        assert rep["layout"] == "scan_work" and rep["shape"] == [n_tasks, n_sums, ldw]
        assert rep["size"] == (n_tasks * n_sums + 28) * ldw
        check_parts(rep, ["part", "marg"], [n_tasks * n_sums * ldw, 28 * ldw])
    assert "(n_tasks·n_sums + 28)·ldw" in (ROOT / "octofitter.jl_amd/csrc/draws/octo_draws_layout.h").read_text()
    assert "n_sums + 28)·ldw" in (ROOT / "include" / "octofitter_hip_draws.h").read_text()


def test_the_staging_of_the_host_twin(reports):
    for rep, (_, _, ld, P, K) in zip(reports[1::2], SHAPES):
        assert rep["layout"] == "scan_staging" and rep["shape"] == [P, K, ld]
        assert rep["size"] == (2 * P * 9 + 3 * K + 3) * ld
        check_parts(rep, ["elems", "g_elems", "beta", "g_beta", "beta_hat", "jitter", "g_jitter", "ll"], [9 * P * ld] * 2 + [K * ld] * 3 + [ld] * 3)
