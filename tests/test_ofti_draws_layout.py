"""
The work layouts of the OFTI rejection sampler (csrc/draws/octo_draws_layout.h: OftiWork / ofti_work, OftiRows / ofti_rows) on host memory, in the
manner of tests/test_de_layout.py and alone: tests/ofti_draws_layout_check.cpp includes that header, is compiled here as plain C++17 with
-fsanitize=address,undefined and run as a program of its own; nothing is loaded into Python. It sizes each layout with a null base, lays it out on
exactly that many doubles, writes a tag to every element of every part and reads all of them back. Checked here: every tag survived, the
sanitizers were silent, the parts are the pinned ones, each starts on an 8-byte boundary with a double's room per element, they come gapless in
the order the struct declares them, and the size is the documented one. CPU suite: no GPU.
"""
import json
import subprocess
from pathlib import Path

import pytest

import ofti_draws_reference      # noqa: F401  (the restatement this layout serves)

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(256, 1, 1), (256, 257, 3), (512, 1000, 1000), (1024, 5000, 77)]      # (chunk, N, room)
NAMES = ["theta", "nl", "ll", "pmax", "cnt", "max", "ix", "oll", "olp", "otheta", "onl", "post"]
FORMULA = "10·2^18 + N + 2⌈N/256⌉ + 2 + 29·min(cap, N)"


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ofti_draws_layout") / "ofti_draws_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "ofti_draws_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


def test_the_layouts_ran_on_every_shape_with_the_documented_size(reports):
    work, rows = reports[0::2], reports[1::2]
    assert [tuple(rep["shape"]) for rep in work] == SHAPES and [rep["shape"] for rep in rows] == [[N] for _, N, _ in SHAPES]
    for rep, (chunk, N, room) in zip(work, SHAPES):
        nblk = (N + 255) // 256
        assert rep["layout"] == "ofti_work" and rep["size"] == 10 * chunk + N + 2 * nblk + 2 + 29 * room, (chunk, N, room)
    for rep, (_, N, _) in zip(rows, SHAPES):
        assert rep["layout"] == "ofti_rows" and rep["size"] == 8 * N and rep["members"] == 1 and rep["parts"][0]["tag_ok"]
    assert FORMULA in (ROOT / "include" / "octofitter_hip_draws.h").read_text()
    for doc in ("DESIGN.md", "octofitter.jl_amd/csrc/draws/octo_draws_layout.h"):
        assert "10·chunk + N + 2·nblk + 2 + 29·room" in (ROOT / doc).read_text(), doc


def test_the_parts_are_the_pinned_ones_gapless_aligned_and_in_declaration_order(reports):
    for rep in reports[0::2]:
        chunk, N, room = rep["shape"]
        nblk = (N + 255) // 256
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(NAMES) == 12, rep["shape"]
        assert [p["name"] for p in parts] == NAMES
        assert [p["len"] for p in parts] == [5 * chunk, 5 * chunk, N, nblk, nblk + 1, 1, room, room, room, 5 * room, 5 * room, 16 * room], rep["shape"]
        assert [p["elem"] for p in parts] == [8] * 12
        assert all(p["tag_ok"] for p in parts), [p["name"] for p in parts if not p["tag_ok"]]
        assert all(p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
        ends = [p["offset"] + 8 * p["len"] for p in parts]
        assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
        members = [p["member"] for p in parts]
        assert members == sorted(members) and len(set(members)) == len(members)
