"""
The work layouts of the catalogue proper-motion anomaly (csrc/draws/octo_draws_layout.h: PmaWork / pma_work, PmaStaging / pma_staging) and the host-made
table algebra (csrc/draws/octo_draws_pma_host.h: pma_table_build) on host memory, in the manner of tests/test_scan_layout.py and alone:
tests/pma_layout_check.cpp includes those headers, is compiled here as plain C++17 with -fsanitize=address,undefined and run as a program of its own;
nothing is loaded into Python. Layouts: every tag survived, the sanitizers were silent, the parts are the pinned ones, each starts on an 8-byte boundary,
they come gapless in the order the struct declares them, and the size is the documented one. Algebra at Q = 1, 6, 8 and K = 0, 2, 4: Σ⁻¹, P_m, N⁻¹HᵀΣ⁻¹
and both constants against numpy at 1e-12 relative to the largest entry; a Σ that is not symmetric positive definite is refused. CPU suite: no GPU.
"""
import json
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pma_reference      # noqa: F401  (the restatement this layout serves)

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 10, 64, 1, 0), (4, 20, 64, 2, 2), (4, 80, 192, 8, 4), (38, 10, 10048, 1, 2)]      # (n_tasks, n_sums, ldw, P, K)
ALGEBRA = [(Q, K) for Q in (1, 6, 8) for K in (0, 2, 4) if K <= Q]      # K > Q: H cannot have full column rank
BAR = 1e-12


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pma_layout") / "pma_layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    f"-I{ROOT / 'octofitter.jl_amd' / 'csrc' / 'draws'}", "-o", str(exe), str(ROOT / "tests" / "pma_layout_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(v) for shape in SHAPES for v in shape] + ["algebra"] + [str(v) for qk in ALGEBRA + [(1, 2), (1, 4)] for v in qk],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr)      # the sanitizers were silent
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    return dict(layouts=[x for x in lines if "layout" in x], algebra=[x for x in lines if "algebra" in x], refusals=[x for x in lines if "refusals" in x])


def check_parts(rep, names, lens):
    parts = rep["parts"]
    assert len(parts) == rep["members"] == len(names), rep["shape"]
    assert [p["name"] for p in parts] == names and [p["len"] for p in parts] == lens, rep["shape"]
    assert all(p["elem"] == 8 and p["tag_ok"] and p["offset"] % 8 == 0 for p in parts) and parts[0]["offset"] == 0
    ends = [p["offset"] + 8 * p["len"] for p in parts]
    assert [p["offset"] for p in parts[1:]] == ends[:-1] and ends[-1] == 8 * rep["size"], rep["shape"]
    members = [p["member"] for p in parts]
    assert members == sorted(members) and len(set(members)) == len(members)


def test_the_work_array_is_the_partials_lambda_and_the_validity_with_the_documented_size(reports):
    for rep, (n_tasks, n_sums, ldw, P, _) in zip(reports["layouts"][0::2], SHAPES):
        assert rep["layout"] == "pma_work" and rep["shape"] == [n_tasks, n_sums, ldw] and n_sums == max(8, 10 * P)
        assert rep["size"] == (n_tasks * n_sums + 9) * ldw
        check_parts(rep, ["part", "lam", "ok"], [n_tasks * n_sums * ldw, 8 * ldw, ldw])
    assert "(n_tasks·n_sums + 9)·ldw" in (ROOT / "octofitter.jl_amd/csrc/draws/octo_draws_layout.h").read_text()
    assert "n_sums + 9)·ldw" in (ROOT / "include" / "octofitter_hip_draws.h").read_text()


def test_the_staging_of_the_host_twin(reports):
    for rep, (_, _, ld, P, K) in zip(reports["layouts"][1::2], SHAPES):
        assert rep["layout"] == "pma_staging" and rep["shape"] == [P, K, ld]
        assert rep["size"] == (2 * P * 9 + 3 * K + 1) * ld
        check_parts(rep, ["elems", "g_elems", "gamma", "g_gamma", "gamma_hat", "ll"], [9 * P * ld] * 2 + [K * ld] * 3 + [ld])
    assert "(2·P·9 + 3·K + 1)·ld" in (ROOT / "include" / "octofitter_hip_draws.h").read_text()


def near(x, ref, what):
    x, ref = np.asarray(x, dtype=np.float64).reshape(np.shape(ref)), np.asarray(ref, dtype=np.float64)
    scale = max(1.0, float(np.max(np.abs(ref)))) if ref.size else 1.0
    err = float(np.max(np.abs(x - ref))) / scale if ref.size else 0.0
    assert err <= BAR, (what, err)


def test_the_host_algebra_against_numpy(reports):
    assert [tuple(r["algebra"]) for r in reports["algebra"]] == ALGEBRA + [(1, 2), (1, 4)]
    for r in reports["algebra"]:
        Q, K = r["algebra"]
        assert r["rc"] == 0 and r["padded"]
        cov = np.array(r["cov"]).reshape(Q, Q)
        H = np.array(r["H"]).reshape(Q, K)
        assert np.array_equal(cov, cov.T) and np.array_equal(np.array(r["H_out"]).reshape(Q, K), H) and np.array_equal(r["d"], r["d_in"])
        Si = np.linalg.inv(cov)
        c0 = -0.5 * (Q * math.log(2 * math.pi) + np.linalg.slogdet(cov)[1])
        near(r["Sinv"], Si, ("Sinv", Q, K))
        near(r["cst"][0], c0, ("c0", Q, K))
        if K > Q:      # more parameters than catalogue values: N is singular, no error, no marginal mode
            assert r["marg_ok"] == 0
            continue
        assert r["marg_ok"] == (1 if K else 0)
        if K:
            N = H.T @ Si @ H
            G = np.linalg.solve(N, H.T @ Si)
            near(r["G"], G, ("G", Q, K))
            near(r["Pm"], Si - Si @ H @ G, ("Pm", Q, K))
            near(r["cst"][1], c0 + 0.5 * K * math.log(2 * math.pi) - 0.5 * np.linalg.slogdet(N)[1], ("c1", Q, K))


def test_a_covariance_that_is_not_symmetric_positive_definite_is_refused(reports):
    assert len(reports["refusals"]) == len(ALGEBRA) + 2
    for r in reports["refusals"]:
        Q, K = r["refusals"]
        assert r["indefinite"] == 2 and r["asymmetric"] == 1, r
        if K > 1:
            assert r["rank_deficient"] == [0, 0], r      # a rank-deficient H is no error of the table: the marginal mode is switched off
