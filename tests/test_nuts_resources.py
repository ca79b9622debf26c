"""
Build checks of the no-U-turn sampler inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_nuts.hip): its kernels are among the compiled
kernels of csrc/draws/build/ and none of them spills a VGPR, uses scratch or carries a private segment; k_nuts_leaf keeps k_hmc_leap's
register bar; the function is declared, exported and bound; the tempered target's device routines exist once, in the shared header. CPU
suite: hipcc cross-compiles, no GPU needed. The expectations of the build are the nuts row of tests/draws_build.py (k_hmc_leap's own count and
bar are the hmc row's).
"""
import re

import companion_checks as cc
import draws_build


def test_nuts_kernels_are_built_without_scratch():
    draws_build.check_kernels("nuts")


def test_nuts_function_is_declared_exported_and_bound(pkg):
    draws_build.check_functions_constants_and_callables(pkg, "nuts")


def test_the_tempered_target_is_stated_once():
    """tempered_energy, dead_state and the prior loop are shared by the HMC step and NUTS through octo_draws_common.h, not copied"""
    src = cc.CSRC / "draws"
    for routine in ("tempered_energy", "dead_state", "tempered_gradient", "prior_loop"):
        defs = {f.name for f in list(src.glob("*.hip")) + list(src.glob("*.h")) if re.search(rf"__device__ __forceinline__ \w+ {routine}\(", f.read_text())}
        assert defs == {"octo_draws_common.h"}, (routine, defs)
    for unit in ("octo_draws_hmc.hip", "octo_draws_nuts.hip"):
        text = (src / unit).read_text()
        assert "prior_loop(" in text and "tempered_energy(" in text and "prior_density_lanes(" not in text, unit
