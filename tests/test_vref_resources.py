"""
Build checks of the variational reference inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_vref.hip), modelled on
tests/test_pt_resources.py: exactly its two kernel families are among the compiled kernels of csrc/draws/build/, one instantiation each, none
of them spills a VGPR, uses scratch or carries a private segment, and each stays within k_hmc_leap's register bar; the five functions are
declared, exported and bound with their parameter counts; the prior routine and the layout are taken from the shared headers, not restated; a
NULL handle is refused before anything else; and the main library's sources did not change. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import companion_checks as cc
import draws_build

KERNELS = ("k_vref_table", "k_vref_exchange")
REGISTER_BAR = 128      # VGPRs + AGPRs: k_hmc_leap's bar, four waves per SIMD at the least
N_PARAMETERS = {"octo_draws_reference_doubles": 1, "octo_draws_reference_set_device": 6, "octo_draws_reference_fit_device": 8,
                "octo_draws_use_reference": 2, "octo_draws_reference_exchange_device": 17}


def test_vref_kernels_are_built_without_scratch_within_the_register_bar():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_vref_")} == set(KERNELS), sorted(built)
    for family in KERNELS:
        rows = built[family]
        assert len(rows) == 1, (family, [r["name"] for r in rows])
        r = rows[0]
        assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
        assert r["vgpr_count"] + r["agpr_count"] <= REGISTER_BAR, (family, r["vgpr_count"], r["agpr_count"])
        print(family, r["vgpr_count"], "VGPRs,", r["agpr_count"], "AGPRs")
    assert draws_build.FEATURES["hmc"]["kernels"]["k_hmc_leap"][1] == REGISTER_BAR


def test_vref_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_vref.hip")


def test_vref_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for name, n in N_PARAMETERS.items():
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported, name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    handle = ("reference_table", "reference_set", "reference_fit", "reference", "use_reference", "reference_exchange", "reference_moments")
    assert all(callable(getattr(draws.PriorDraws, f)) for f in handle) and callable(pkg.octofit_pigeons_device)
    import inspect
    sig = inspect.signature(pkg.octofit_pigeons_device).parameters
    assert (sig["n_temps_variational"].default, sig["first_tuning_round"].default, sig["inflate"].default) == (0, 5, 1.0)


def test_the_prior_routine_and_the_layout_are_taken_from_the_shared_headers():
    text = (cc.CSRC / "draws" / "octo_draws_vref.hip").read_text()
    for routine in ("prior_loop(", "ref_table", "carve_size(", "carve_at("):
        assert routine in text, routine
    for restated in ("prior_density_lanes", "prior_link_lanes", "atomicAdd", "hipMalloc", "hipStreamSynchronize", "hipMemcpy"):
        assert restated not in text, restated
    common = (cc.CSRC / "draws" / "octo_draws_common.h").read_text()
    assert common.count("double prior_loop(") == 1 and "own_priors" in common


def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_vref.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    E = pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_reference_set_device(None, None, None, None, None, None) == E
    assert lib.octo_draws_reference_fit_device(None, None, None, None, 1.0, None, None, None) == E
    assert lib.octo_draws_use_reference(None, None) == E
    assert lib.octo_draws_reference_exchange_device(None, 1, 2, None, 2, None, None, None, None, 2, None, 2, None, None, None, None, None) == E
