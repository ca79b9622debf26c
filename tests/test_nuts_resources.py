"""
Build checks of the no-U-turn sampler inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_nuts.hip): its kernels are among the compiled
kernels of csrc/draws/build/ and none of them spills a VGPR, uses scratch or carries a private segment; k_nuts_leaf keeps k_hmc_leap's
register bar; the function is declared, exported and bound; the tempered target's device routines exist once, in the shared header. CPU
suite: hipcc cross-compiles, no GPU needed.
"""
import re

import pytest

import companion_checks as cc


@pytest.fixture(scope="module")
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    return build_draws()


def test_nuts_kernels_are_built_without_scratch(draws_lib):
    rows, names = cc.check_kernels_have_no_scratch("draws", sgpr_too=False)
    assert {"k_nuts_open", "k_nuts_leaf", "k_nuts_report", "k_hmc_leap"} <= names, names
    for kernel in ("k_nuts_open", "k_nuts_leaf"):
        mine = [r for r in rows if kernel in r["name"]]
        assert len(mine) == 1, [r["name"] for r in mine]
        # no table hoisted out of the coordinate loops: four waves per SIMD at the least, as k_hmc_leap
        assert all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in mine), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in mine]
    leap = [r for r in rows if "k_hmc_leap" in r["name"]]
    assert len(leap) == 3 and all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in leap)


def test_nuts_function_is_declared_exported_and_bound(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    text = cc.check_header_library_and_binding_agree("draws", draws, draws_lib, {"octo_draws_nuts_device"}, exact=False)
    for name, value in (("NUTS_DIRECTION", 6), ("NUTS_LEAF", 7), ("NUTS_MERGE", 8)):
        assert re.search(rf"#define OCTO_DRAWS_PURPOSE_{name}\s+{value}\b", text), name
    assert "#define OCTO_DRAWS_NUTS_MAX_DEPTH 10" in text
    assert (draws.PURPOSE_NUTS_DIRECTION, draws.PURPOSE_NUTS_LEAF, draws.PURPOSE_NUTS_MERGE, draws.NUTS_MAX_DEPTH) == (6, 7, 8, 10)
    assert all(callable(getattr(pkg, f)) for f in ("octofit_nuts_device", "octofit_hmc_device", "hmc_warmup"))
    assert all(callable(getattr(draws.PriorDraws, f)) for f in ("nuts", "nuts_step"))


def test_the_tempered_target_is_stated_once():
    """tempered_energy, dead_state and the prior loop are shared by the HMC step and NUTS through octo_draws_common.h, not copied"""
    src = cc.CSRC / "draws"
    for routine in ("tempered_energy", "dead_state", "tempered_gradient", "prior_loop"):
        defs = {f.name for f in list(src.glob("*.hip")) + list(src.glob("*.h")) if re.search(rf"__device__ __forceinline__ \w+ {routine}\(", f.read_text())}
        assert defs == {"octo_draws_common.h"}, (routine, defs)
    for unit in ("octo_draws_hmc.hip", "octo_draws_nuts.hip"):
        text = (src / unit).read_text()
        assert "prior_loop(" in text and "tempered_energy(" in text and "prior_density_lanes(" not in text, unit
