"""
Build checks of the companion library liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, csrc/draws/) for the prior draws and the
two optimisers built on them: what it exports against what its header declares and host/draws.py binds, the argument check that needs no
device, and the compiled kernels' resources. The expectations are the rows of tests/draws_build.py's FEATURES and the checks are its
functions, shared with the samplers' files (tests/test_hmc_resources.py, test_adapt_resources.py, test_nuts_resources.py): the build is
disassembled once for all four, and the header, the exports and the binding are compared as a whole here, once. Linkage and the main library's symbol set are checked for all four companion
libraries in tests/test_companion_libraries.py. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import ctypes as C

import pytest

import companion_checks as cc
import draws_build

MINE = ("prior_draws", "lbfgs", "pathfinder")


@pytest.mark.parametrize("feature", MINE)
def test_kernels_are_built_without_scratch(feature):
    draws_build.check_kernels(feature)


def test_header_library_and_binding_agree(pkg):
    draws_build.check_header_library_and_binding_agree()
    assert len(cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")) >= 6


@pytest.mark.parametrize("feature", MINE)
def test_functions_constants_and_callables(pkg, feature):
    draws_build.check_functions_constants_and_callables(pkg, feature)


def test_pathfinder_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_pathfinder.hip")


def test_create_with_null_context_is_einval(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    h = C.c_void_p()
    pr = (pkg.capi.OctoPrior * 1)()
    pr[0].kind, pr[0].p0, pr[0].p1 = pkg.capi.PRIOR_UNIFORM, 0.0, 1.0
    assert lib.octo_draws_create(None, None, pr, 1, 0, C.byref(h)) == pkg.capi.OCTO_EINVAL
    assert not h.value and b"null" in lib.octo_draws_last_error(None)
    assert lib.octo_draws_best(None, 0, 0, 1, 1, None, None, None) == pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_destroy(None) == pkg.capi.OCTO_OK
