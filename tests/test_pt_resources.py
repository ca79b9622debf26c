"""
Build checks of the parallel-tempering statistics inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_pt.hip): exactly its three kernel
families are among the compiled kernels of csrc/draws/build/, one instantiation each, none of them spills a VGPR, uses scratch or carries a
private segment, and each stays within k_hmc_leap's register bar; the two functions are declared, exported and bound with their parameter
counts; the wave sum and the block order are taken from the shared header, not restated; a NULL handle is refused before anything else; and
the main library's sources did not change. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import companion_checks as cc
import draws_build
import pt_reference as pt

KERNELS = ("k_ptadapt_partials", "k_ptadapt_merge", "k_ptadapt_schedule")
REGISTER_BAR = 128      # VGPRs + AGPRs: k_hmc_leap's bar, four waves per SIMD at the least
N_PARAMETERS = {"octo_draws_pt_stats_device": 10, "octo_draws_pt_schedule_device": 10}


def test_pt_kernels_are_built_without_scratch_within_the_register_bar():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_ptadapt_")} == set(KERNELS), sorted(built)
    for family in KERNELS:
        rows = built[family]
        assert len(rows) == 1, (family, [r["name"] for r in rows])
        r = rows[0]
        assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
        assert r["vgpr_count"] + r["agpr_count"] <= REGISTER_BAR, (family, r["vgpr_count"], r["agpr_count"])
        print(family, r["vgpr_count"], "VGPRs,", r["agpr_count"], "AGPRs")
    assert draws_build.FEATURES["hmc"]["kernels"]["k_hmc_leap"][1] == REGISTER_BAR


def test_pt_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_pt.hip")


def test_pt_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for name, n in N_PARAMETERS.items():
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported, name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    assert all(callable(getattr(draws.PriorDraws, f)) for f in ("pt_state", "pt_stats", "pt_schedule")) and callable(pkg.octofit_pigeons_device)
    assert len(draws.PT_ACC_COLUMNS) == 8 and len(draws.PT_SUMMARY) == 4 and draws.MAX_GROUPS == pt.MAX_GROUPS


def test_the_sums_are_taken_from_the_shared_header():
    text = (cc.CSRC / "draws" / "octo_draws_pt.hip").read_text()
    for routine in ("wave_sum(", "waves_total(", "pt_partials"):
        assert routine in text, routine
    for restated in ("double wave_sum", "double waves_total", "atomicAdd", "__shfl_down"):
        assert restated not in text, restated
    common = (cc.CSRC / "draws" / "octo_draws_common.h").read_text()
    assert common.count("double wave_sum(") == 1
    for unit in ("octo_draws_adapt.hip", "octo_draws_diag.hip"):      # one statement of the butterfly for the three units that sum across chains
        assert "double wave_sum(" not in (cc.CSRC / "draws" / unit).read_text(), unit


def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_pt.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    assert lib.octo_draws_pt_stats_device(None, 2, 1, None, None, None, None, None, None, None) == pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_pt_schedule_device(None, 2, None, None, 1, 1, None, None, None, None) == pkg.capi.OCTO_EINVAL
