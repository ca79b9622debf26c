"""
Build checks of the dense metric inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_dense.hip and the dense kernels of octo_draws_hmc.hip
and octo_draws_nuts.hip): the k_dense_* families are exactly the listed ones with their instantiation counts, each within k_hmc_leap's register
bar and without a spilled VGPR, a scratch instruction or a private segment; the samplers' own families are what they were; the four functions
are declared, exported and bound with their parameter counts; the constant agrees between header, binding and restatement; the two triangular
products exist once, in the shared header; the main library's sources are untouched. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import ctypes as C
import re

import companion_checks as cc
import dense_reference as dref
import draws_build

DENSE_KERNELS = {"k_dense_cov_partials": 1, "k_dense_cov_merge": 1, "k_dense_factor": 1, "k_dense_apply": 1, "k_dense_hmc_leap": 3, "k_dense_nuts_open": 1,
                 "k_dense_nuts_leaf": 1}
DENSE_FUNCTIONS = {"octo_draws_cov_device": 10, "octo_draws_metric_dense_device": 8, "octo_draws_metric_apply_device": 8, "octo_draws_use_metric": 2}
REGISTER_BAR = 128


def test_dense_kernels_are_the_listed_families_without_scratch():
    built = draws_build.kernels()      # none of the build's kernels spills, uses scratch or has a private segment
    assert {k for k in built if k.startswith("k_dense_")} == set(DENSE_KERNELS), sorted(built)
    for family, count in DENSE_KERNELS.items():
        mine = built[family]
        assert len(mine) == count, (family, [r["name"] for r in mine])
        assert all(r["vgpr_count"] + r["agpr_count"] <= REGISTER_BAR for r in mine), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in mine]
    assert not any("cube" in k for k in built if k.startswith("k_dense_"))


def test_the_samplers_families_are_what_they_were():
    for feature in ("hmc", "nuts", "adapt", "pathfinder"):
        draws_build.check_kernels(feature)


def test_dense_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    header = cc.ROOT / "include" / "octofitter_hip_draws.h"
    declared = cc.declared_functions(header, "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for fn, n_params in DENSE_FUNCTIONS.items():
        assert declared.get(fn) == n_params, (fn, declared.get(fn))
        assert fn in exported and fn in draws.EXPORTED_SYMBOLS and len(draws._SIGS[fn][1]) == n_params, fn
    draws_build.check_header_library_and_binding_agree()
    assert ("#define", "OCTO_DRAWS_DENSE_MAX_D", "64") in [tuple(line.split()) for line in header.read_text().splitlines()]
    assert draws.DENSE_MAX_D == dref.MAX_D == 64
    for name in ("cov", "metric_dense", "metric_apply", "use_metric"):
        assert callable(getattr(draws.PriorDraws, name)), name
    assert callable(draws.pack_lower) and callable(draws.unpack_lower)


def test_the_two_products_are_stated_once_and_every_dense_kernel_reaches_them():
    src = cc.CSRC / "draws"
    for routine in ("metric_lower", "metric_lower_t", "metric_gradient"):
        defs = {f.name for f in list(src.glob("*.hip")) + list(src.glob("*.h")) if re.search(rf"__device__ __forceinline__ void {routine}\(", f.read_text())}
        assert defs == {"octo_draws_common.h"}, (routine, defs)
    for unit, calls in (("octo_draws_hmc.hip", ("metric_gradient<DENSE>(", "metric_lower(")), ("octo_draws_nuts.hip", ("metric_gradient<DENSE>(", "metric_lower(")),
                        ("octo_draws_dense.hip", ("metric_lower(", "metric_lower_t("))):
        text = (src / unit).read_text()
        assert all(c in text for c in calls), unit
    for unit in ("octo_draws_hmc.hip", "octo_draws_nuts.hip"):      # what tests/test_nuts_resources.py holds them to
        text = (src / unit).read_text()
        assert "prior_loop(" in text and "tempered_energy(" in text and "prior_density_lanes(" not in text, unit


def test_main_library_sources_are_untouched():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_dense.hip")


def test_a_null_handle_is_refused(pkg):
    """Without a device no handle can be made: the NULL handle, refused before anything else; the same arguments on a real handle are in
    tests/test_dense.py."""
    draws_build.draws_lib()
    from octofitter_jl_amd.host import draws
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    for fn in DENSE_FUNCTIONS:
        args = [None if t is C.c_void_p else 0 for t in draws._SIGS[fn][1]]
        assert getattr(lib, fn)(*args) == EINVAL, fn
