"""
Build checks of the tempered HMC explorer inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_hmc.hip): its kernels are among the
compiled kernels of csrc/draws/build/ and none of them spills a VGPR, uses scratch or carries a private segment; the three functions are
declared, exported and bound. The expectations are the hmc row of tests/draws_build.py. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import draws_build


def test_hmc_kernels_are_built_without_scratch():
    draws_build.check_kernels("hmc")


def test_hmc_functions_are_declared_exported_and_bound(pkg):
    draws_build.check_functions_constants_and_callables(pkg, "hmc")
