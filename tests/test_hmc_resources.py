"""
Build checks of the tempered HMC explorer inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_hmc.hip): its kernels are among the
compiled kernels of csrc/draws/build/ and none of them spills a VGPR, uses scratch or carries a private segment; the three functions are
declared, exported and bound. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import pytest

import companion_checks as cc


@pytest.fixture(scope="module")
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    return build_draws()


def test_hmc_kernels_are_built_without_scratch(draws_lib):
    rows, names = cc.check_kernels_have_no_scratch("draws", sgpr_too=False)
    assert {"k_hmc_momentum", "k_hmc_leap"} <= names, names
    leap = [r for r in rows if "k_hmc_leap" in r["name"]]
    assert len(leap) == 3, [r["name"] for r in leap]      # the start point, a point inside the trajectory, the end point
    # no coefficient table hoisted out of the coordinate loops: four waves per SIMD at the least
    assert all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in leap), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in leap]
    mom = [r for r in rows if "k_hmc_momentum" in r["name"]]
    assert mom and all(r["vgpr_count"] + r["agpr_count"] <= 64 for r in mom)


def test_hmc_functions_are_declared_exported_and_bound(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    new = {"octo_draws_momentum_device", "octo_draws_hmc_step_device", "octo_draws_hmc_step"}
    text = cc.check_header_library_and_binding_agree("draws", draws, draws_lib, new, exact=False)
    assert "#define OCTO_DRAWS_PURPOSE_MOMENTUM 2" in text and "#define OCTO_DRAWS_PURPOSE_ACCEPT   3" in text
    assert (draws.PURPOSE_MOMENTUM, draws.PURPOSE_ACCEPT) == (2, 3)
