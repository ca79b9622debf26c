"""
Build checks of the batched L-BFGS inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_lbfgs.hip): its kernels are among the compiled
kernels of csrc/draws/build/, none of them spills, uses scratch or carries a private segment (a per-lane ring position never indexes a
private array), the advance kernel stays at four waves per SIMD; the three functions are declared, exported and bound; the constants
agree. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import pytest

import companion_checks as cc
import lbfgs_reference as ref


@pytest.fixture(scope="module")
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    return build_draws()


def test_lbfgs_kernels_are_built_without_scratch(draws_lib):
    rows, names = cc.check_kernels_have_no_scratch("draws", sgpr_too=False)
    assert {"k_lbfgs_advance", "k_lbfgs_direction"} <= names, names
    adv = [r for r in rows if "k_lbfgs_advance" in r["name"]]
    assert len(adv) == 3, [r["name"] for r in adv]      # the opening launch, a round, the outputs alone
    mine = adv + [r for r in rows if "k_lbfgs_direction" in r["name"]]
    assert len(mine) == 4 and all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in mine), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in mine]


def test_lbfgs_functions_are_declared_exported_and_bound(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    new = {"octo_draws_lbfgs_direction_device", "octo_draws_lbfgs_device", "octo_draws_lbfgs"}
    text = cc.check_header_library_and_binding_agree("draws", draws, draws_lib, new, exact=False)
    for name, value in (("MAX_M", 8), ("ACTIVE", 0), ("GTOL", 1), ("FTOL", 2), ("LINESEARCH", 3), ("DEAD", 4)):
        assert any(line.split() == ["#define", f"OCTO_DRAWS_LBFGS_{name}", str(value)] for line in text.splitlines()), name
        assert getattr(draws, f"LBFGS_{name}") == value == getattr(ref, name)
    assert callable(pkg.optimize_starting_points_device) and callable(draws.PriorDraws.lbfgs) and callable(draws.PriorDraws.lbfgs_direction)
