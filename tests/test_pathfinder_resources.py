"""
Build checks of Pathfinder inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_pathfinder.hip): its kernels are among the compiled
kernels of csrc/draws/build/, none of them spills, uses scratch or carries a private segment (nothing of a chain lives in a private array),
the fit kernel is one wave a block with its matrix in dynamic LDS; the three functions are declared, exported and bound; the constants
agree; the L-BFGS kernels keep their instantiation counts. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import pytest

import companion_checks as cc
import pathfinder_reference as ref

KERNELS = {"k_pf_open", "k_pf_fit", "k_pf_normals", "k_pf_map", "k_pf_elbo", "k_pf_mask"}
FUNCTIONS = {"octo_draws_pathfinder_fit_device", "octo_draws_pathfinder_device", "octo_draws_pathfinder_draw_device"}


@pytest.fixture(scope="module")
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    return build_draws()


def test_pathfinder_kernels_are_built_without_scratch(draws_lib):
    rows, names = cc.check_kernels_have_no_scratch("draws", sgpr_too=False)
    assert KERNELS <= names, names
    mine = [r for r in rows if "k_pf_" in r["name"]]
    assert len(mine) == len(KERNELS), [r["name"] for r in mine]      # no template: one instantiation each
    assert all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in mine), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in mine]
    # the L-BFGS is called, not copied: its kernels as tests/test_lbfgs_resources.py counts them
    assert len([r for r in rows if "k_lbfgs_advance" in r["name"]]) == 3 and len([r for r in rows if "k_lbfgs_direction" in r["name"]]) == 1


def test_pathfinder_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_pathfinder.hip")


def test_pathfinder_functions_are_declared_exported_and_bound(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    text = cc.check_header_library_and_binding_agree("draws", draws, draws_lib, FUNCTIONS, exact=False)
    for name, value, mine in (("PF_MAX_D", 64, ref.MAX_D), ("PF_MAX_ELBO_DRAWS", 32, ref.MAX_ELBO_DRAWS), ("PURPOSE_ELBO", 4, ref.PURPOSE_ELBO),
                              ("PURPOSE_PATHFINDER", 5, ref.PURPOSE_PATHFINDER)):
        assert any(line.split() == ["#define", f"OCTO_DRAWS_{name}", str(value)] for line in text.splitlines()), name
        assert getattr(draws, name) == value == mine
    assert callable(pkg.pathfinder_device)
    assert all(callable(getattr(draws.PriorDraws, f)) for f in ("pathfinder_fit", "pathfinder", "pathfinder_draw"))
