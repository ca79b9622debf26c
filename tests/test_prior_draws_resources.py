"""
Build checks of the companion library liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, csrc/draws/): what it exports against what
its header declares and host/draws.py binds, the argument check that needs no device, and the compiled kernels' resources read from the
code objects (tools/kernel_resources.py). The bodies every companion library shares are in tests/companion_checks.py; linkage and the main
library's symbol set are checked for all four in tests/test_companion_libraries.py. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import ctypes as C

import pytest

import companion_checks as cc


@pytest.fixture(scope="module")
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()           # no-ops when csrc/build/ and csrc/draws/build/ are up to date
    return build_draws()


def test_header_library_and_binding_agree(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    cc.check_header_library_and_binding_agree("draws", draws, draws_lib, {"octo_draws_create", "octo_draws_destroy", "octo_draws_sample_device",
                                                                          "octo_draws_best", "octo_draws_rejection", "octo_draws_last_error"}, exact=False)
    assert len(cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")) >= 6


def test_create_with_null_context_is_einval(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    lib = draws.load_library()
    h = C.c_void_p()
    pr = (pkg.capi.OctoPrior * 1)()
    pr[0].kind, pr[0].p0, pr[0].p1 = pkg.capi.PRIOR_UNIFORM, 0.0, 1.0
    assert lib.octo_draws_create(None, None, pr, 1, 0, C.byref(h)) == pkg.capi.OCTO_EINVAL
    assert not h.value and b"null" in lib.octo_draws_last_error(None)
    assert lib.octo_draws_best(None, 0, 0, 1, 1, None, None, None) == pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_destroy(None) == pkg.capi.OCTO_OK


def test_companion_kernels_have_no_scratch(draws_lib):
    rows, names = cc.check_kernels_have_no_scratch("draws", sgpr_too=False)
    assert {"k_draw", "k_topk", "k_loglike", "k_max", "k_count", "k_scan", "k_scatter"} <= names, names
    # the draw kernel is one thread per draw with no loop over the coordinates: held to the registers of eight waves per SIMD
    draw = [r for r in rows if r["name"].startswith("k_draw")]
    assert draw and all(r["vgpr_count"] + r["agpr_count"] <= 64 for r in draw), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in draw]
