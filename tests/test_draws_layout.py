"""
The work-allocation layouts of liboctofitter_hip_draws.so (csrc/draws/octo_draws_layout.h) on host memory. tests/draws_layout_check.cpp
includes that header alone, is compiled here as plain C++17 with -fsanitize=address,undefined and run as a program of its own: it sizes
every layout with a null base, lays it out on exactly that many doubles, writes a tag of its own to every element of every part and reads
all of them back. Checked here: every tag survived (no two parts overlap), the sanitizers were silent (nothing out of bounds), every part
starts on an 8-byte boundary and has a double's room per element (an int32 element too), parts come gapless in the order their struct
declares them, and the sizes are the ones include/octofitter_hip_draws.h and DESIGN.md document, computed here independently. The parts
of the two layouts the warm-up and the no-U-turn sampler added are pinned by name. CPU suite: no GPU, nothing loaded into Python.
"""
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((1, 1, 1), (3, 5, 2), (64, 7, 8))      # (D, ld, m); the ELBO batch has KW = 5·ld
MOMENT_SHAPES = [(1, 1, 1), (3, 5, 2), (7, 64, 64), (4, 3, 11)]      # (nblk, G, K)
NUTS_SHAPES = [(1, 1, 1), (14, 72, 4), (5, 65536, 5), (64, 3, 10), (3, 257, 2)]      # (D, ld, max_depth)

# doubles of each layout, by the shape the program reports for it
SIZES = {
    "lbfgs_state": lambda D, ld, m: ((5 + 2 * m) * D + 2 * m + 11) * ld,
    "pf_state": lambda D, ld: (D * D + 5 * D + 8) * ld,
    "hmc_work": lambda D, ld: 4 * D * ld + 4 * ld,
    "lbfgs_staging": lambda D, ld: 2 * D * ld + 5 * ld + D,
    "hmc_staging": lambda D, ld: 2 * D * ld + 6 * ld + D,
    "pf_batch": lambda D, KW: (D + 2) * KW,
    "lbfgs_coef": lambda D, ld, m: 2 * m * ld,
    "chunk_bufs": lambda D, chunk, lists: D * chunk + chunk + 2 * lists + 1,
    "draw_arrays": lambda n, nblk: 2 * n + 2 * nblk + 1,
    "outputs": lambda D, n: (D + 3) * n,
}
NUTS_PLANES = ["trial", "pt", "qL", "pL", "gL", "qR", "pR", "gR", "prop", "sprop", "rho", "rho_s", "gpr", "glp"]
NUTS_STACKS = ["ck_p", "ck_r"]
NUTS_SCALARS = ["lp", "H0", "logw", "logw_s", "sum_acc", "prop_lp", "prop_lpt", "sprop_lp", "sprop_lpt", "out_lp", "out_lpt"]
NUTS_COUNTERS = ["status", "depth", "n", "nleaf", "v", "sel", "ssel"]
# The two layouts with shape lists of their own, the warm-up's and the no-U-turn sampler's:
# layout -> (shapes, doubles, the formula as the documents word it, the documents, part names in order, their lengths, their element sizes)
ADDED = {
    "moments_partials": (MOMENT_SHAPES, lambda nblk, G, K: nblk * G * (2 * K + 1), "⌈W/256⌉·G·(2K + 1) doubles", ("include/octofitter_hip_draws.h",),
                         ["cnt", "sum", "m2"], lambda nblk, G, K: [nblk * G, nblk * G * K, nblk * G * K], [8] * 3),
    "nuts_work": (NUTS_SHAPES, lambda D, ld, md: ((14 + 2 * md) * D + 18) * ld, "((14 + 2·max_depth)·D + 18)·ld", ("include/octofitter_hip_draws.h", "DESIGN.md"),
                  NUTS_PLANES + NUTS_STACKS + NUTS_SCALARS + NUTS_COUNTERS, lambda D, ld, md: [D * ld] * 14 + [md * D * ld] * 2 + [ld] * 18, [8] * 27 + [4] * 7),
}


@pytest.fixture(scope="module")
def all_reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("draws_layout") / "draws_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "draws_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    return [json.loads(line) for line in r.stdout.splitlines()]


@pytest.fixture(scope="module")
def reports(all_reports):
    """the ten layouts that run on SHAPES"""
    assert {rep["layout"] for rep in all_reports} == set(SIZES) | set(ADDED)
    return [rep for rep in all_reports if rep["layout"] not in ADDED]


def check_parts(rep):
    """disjoint, aligned, gapless, inside the allocation, in the order the struct declares"""
    what = (rep["layout"], rep["shape"])
    parts = rep["parts"]
    assert len(parts) == rep["members"], what      # the program names every pointer of the struct
    assert all(p["tag_ok"] for p in parts), (what, [p["name"] for p in parts if not p["tag_ok"]])
    assert all(p["offset"] % 8 == 0 and p["elem"] in (4, 8) for p in parts), what
    assert parts[0]["offset"] == 0
    ends = [p["offset"] + 8 * p["len"] for p in parts]      # a double's room per element, whatever its width
    assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], what      # gapless, so in order and inside the allocation
    members = [p["member"] for p in parts]
    assert members == sorted(members) and len(set(members)) == len(members), what      # the order the struct declares


def test_every_layout_ran_on_every_shape(reports):
    seen = {}
    for rep in reports:
        seen.setdefault(rep["layout"], []).append(tuple(rep["shape"]))
    assert set(seen) == set(SIZES)
    assert seen["lbfgs_state"] == list(SHAPES)
    assert seen["pf_state"] == seen["hmc_work"] == seen["lbfgs_staging"] == seen["hmc_staging"] == [(D, ld) for D, ld, _ in SHAPES]
    assert seen["pf_batch"] == [(D, 5 * ld) for D, ld, _ in SHAPES]
    assert all(len(v) == len(SHAPES) for v in seen.values())


def test_sizes_are_the_documented_ones(reports):
    for rep in reports:
        assert rep["size"] == SIZES[rep["layout"]](*rep["shape"]), (rep["layout"], rep["shape"], rep["size"])


def test_parts_are_disjoint_aligned_and_in_declaration_order(reports):
    for rep in reports:
        check_parts(rep)


@pytest.mark.parametrize("layout", ADDED)
def test_added_layout_ran_on_every_shape_with_the_documented_size(all_reports, layout):
    shapes, size, formula, documents = ADDED[layout][:4]
    mine = [rep for rep in all_reports if rep["layout"] == layout]
    assert [tuple(rep["shape"]) for rep in mine] == shapes
    for rep in mine:
        assert rep["size"] == size(*rep["shape"]), rep["shape"]
    for doc in documents:
        assert formula in (ROOT / doc).read_text(), doc


@pytest.mark.parametrize("layout,n_members", [("moments_partials", 3), ("nuts_work", 34)])
def test_added_layout_parts_are_the_pinned_ones(all_reports, layout, n_members):
    """names, lengths and element sizes as pinned; then disjoint, aligned, gapless and in declaration order as every layout"""
    names, lengths, elems = ADDED[layout][4:]
    mine = [rep for rep in all_reports if rep["layout"] == layout]
    assert mine
    for rep in mine:
        parts = rep["parts"]
        assert len(parts) == rep["members"] == len(names) == n_members, rep["shape"]
        assert [p["name"] for p in parts] == names, rep["shape"]
        assert [p["len"] for p in parts] == lengths(*rep["shape"]), rep["shape"]
        assert [p["elem"] for p in parts] == elems, rep["shape"]
        check_parts(rep)
