"""
The work layouts of the Gaussian-process RV term (csrc/draws/octo_draws_layout.h: GpWork / gp_work, GpStaging / gp_staging) on host memory, in the manner
of tests/test_scan_layout.py and alone: tests/gp_layout_check.cpp includes that header, is compiled here as plain C++17 with -fsanitize=address,undefined
and run as a program of its own; nothing is loaded into Python. It sizes each layout with a null base, lays it out on exactly that many doubles, writes a
tag to every element of every part and reads all of them back. Checked here: every tag survived, the sanitizers were silent, the parts are the pinned
ones, each starts on an 8-byte boundary, they come gapless in the order the struct declares them, and the size is the documented one. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

import gp_reference as gref

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 5, 1, 64, 2, 0, 0), (1, 5, 1, 64, 2, 0, 1), (17, 14, 4, 128, 9, 2, 1), (53, 44, 8, 64, 16, 4, 1), (200, 44, 2, 10048, 12, 1, 0)]      # (n, n_state, P, ldw, H, K, grad)


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gp_layout") / "gp_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "gp_layout_check.cpp")], check=True)
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


def test_the_work_array_has_the_documented_size(reports):
    G, R = gref.SEGMENT, gref.ROWS
    for rep, (n, ns, P, ldw, _, _, grad) in zip(reports[0::2], SHAPES):
        assert rep["layout"] == "gp_work" and rep["shape"] == [n, ns, P, ldw, grad]
        n_seg, n_tasks, n_sums = -(-n // G), -(-n // R), 4 + 6 * P
        assert rep["size"] == (n + 1 + grad * ((n_seg + G) * ns + n_tasks * n_sums)) * ldw
        check_parts(rep, ["res", "ok", "check", "seg", "part"], [n * ldw, ldw, grad * n_seg * ns * ldw, grad * G * ns * ldw, grad * n_tasks * n_sums * ldw])
    assert "(n + 1 + [grad]·((n_seg + SEGMENT)·n_state + n_tasks·n_sums))·ldw" in (ROOT / "octofitter.jl_amd/csrc/draws/octo_draws_layout.h").read_text()
    assert "ldw·(n + 1 + [grad]·(" in (ROOT / "include" / "octofitter_hip_draws.h").read_text()


def test_the_staging_of_the_host_twin(reports):
    for rep, (_, _, P, ld, H, K, _) in zip(reports[1::2], SHAPES):
        assert rep["layout"] == "gp_staging" and rep["shape"] == [P, H, K, ld]
        assert rep["size"] == (2 * P * 9 + 2 * H + 2 * K + 3) * ld
        check_parts(rep, ["elems", "g_elems", "hyper", "g_hyper", "beta", "g_beta", "jitter", "g_jitter", "ll"], [9 * P * ld] * 2 + [H * ld] * 2 + [K * ld] * 2 + [ld] * 3)
