"""
Build checks of the warm-up statistics inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_adapt.hip): its kernels are among the compiled
kernels of csrc/draws/build/, none of them spills, uses scratch or carries a private segment, each has at most 128 VGPRs and one
instantiation — k_adapt_partials, a template on whether its one row is the acceptance probability made on the fly, has its two —; the five
functions are declared, exported and bound; OCTO_DRAWS_MAX_GROUPS agrees between header, binding and restatement; the explorer's kernels keep
their instantiation counts (the hmc row). The expectations of the build are the adapt row of tests/draws_build.py. CPU suite: hipcc
cross-compiles, no GPU needed.
"""
import companion_checks as cc
import draws_build


def test_adapt_kernels_are_built_without_scratch():
    draws_build.check_kernels("adapt")


def test_adapt_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_adapt.hip")


def test_adapt_functions_are_declared_exported_and_bound(pkg):
    draws_build.check_functions_constants_and_callables(pkg, "adapt")


def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_adapt.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_moments_device(None, 4, 4, 1, None, None, 1, 0, None, None, None, None) == EINVAL
    assert lib.octo_draws_metric_device(None, 1, None, None, None, 1, None, None) == EINVAL
    assert lib.octo_draws_hmc_adapt_init_device(None, 1, None, 0.1, None, None) == EINVAL
    assert lib.octo_draws_hmc_adapt_device(None, 4, None, 1, None, None, 1, 0.8, 0.05, 10.0, 0.75, None, None, 0, None, None) == EINVAL
    assert lib.octo_draws_chain_moments_device(None, 4, 4, 1, 1, None, None, None, None) == EINVAL
