"""
Build checks of differential evolution inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_de.hip), modelled on
tests/test_slice_resources.py: exactly its three kernel families are among the compiled kernels of csrc/draws/build/, one instantiation each,
none of them spills a VGPR, uses scratch or carries a private segment (the coordinate loop addresses global memory only), and each stays
within k_hmc_leap's register bar; the functions are declared, exported and bound with their parameter counts; the macros agree with the
binding's constants and the restatement's; the target, the round driver and the generator are taken from the shared header, not copied; a
NULL handle is refused before anything else; and the main library's sources did not change. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import companion_checks as cc
import de_reference as de
import draws_build

KERNELS = ("k_de_open", "k_de_round", "k_de_report")
REGISTER_BAR = 128      # VGPRs + AGPRs: k_hmc_leap's bar, four waves per SIMD at the least
MACROS = dict(PURPOSE_DE=(12, de.PURPOSE_DE), DE_TAU_F=(0.1, de.TAU_F), DE_F_LOW=(0.1, de.F_LOW), DE_F_SPAN=(0.9, de.F_SPAN), DE_TAU_CR=(0.1, de.TAU_CR),
              DE_F0=(0.5, de.F0), DE_CR0=(0.9, de.CR0))
N_PARAMETERS = 19
SOURCE = cc.CSRC / "draws" / "octo_draws_de.hip"


def test_de_kernels_are_built_without_scratch_within_the_register_bar():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_de_")} == set(KERNELS), sorted(built)
    for family in KERNELS:
        rows = built[family]
        assert len(rows) == 1, (family, [r["name"] for r in rows])
        r = rows[0]
        assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
        assert r["vgpr_count"] + r["agpr_count"] <= REGISTER_BAR, (family, r["vgpr_count"], r["agpr_count"])
    assert draws_build.FEATURES["hmc"]["kernels"]["k_hmc_leap"][1] == REGISTER_BAR


def test_de_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_de.hip")


def test_de_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    for name, n in (("octo_draws_de_device", N_PARAMETERS), ("octo_draws_de_work_doubles", 2)):
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in cc.dynamic_symbols(draws_build.draws_lib()), name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    assert callable(draws.PriorDraws.de) and callable(draws.PriorDraws.de_step)
    assert callable(pkg.global_search_device) and callable(pkg.initialize_device)
    assert len(draws.DE_OUTPUTS) == 7


def test_de_macros_are_the_bindings_constants():
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for name, (value, restated) in MACROS.items():
        assert ("#define", f"OCTO_DRAWS_{name}", str(value)) in lines, name      # the whole line
        assert getattr(draws, name) == value == restated, name
    for macro in ("OCTO_DRAWS_DE_TAU_F", "OCTO_DRAWS_DE_F_LOW", "OCTO_DRAWS_DE_F_SPAN", "OCTO_DRAWS_DE_TAU_CR", "OCTO_DRAWS_DE_F0", "OCTO_DRAWS_DE_CR0", "OCTO_DRAWS_PURPOSE_DE"):
        assert macro in SOURCE.read_text(), macro      # the kernels read the header's constants, not literals of their own


def test_the_shared_routines_are_used_and_not_copied():
    text = SOURCE.read_text()
    for routine in ("chain_of(", "target_at(", "dead_state(", "run_rounds(", "check_sampler_call(", "philox4x64(", "u01(", "carve_at(", "de_work"):
        assert routine in text, routine
    for copied in ("prior_density_lanes(", "prior_link_lanes(", "double prior_loop", "void philox4x64", "double u01", "bool dead_state", "int run_rounds", "PHILOX_M0",
                   "atomicAdd(", "hipGraph", "hipMalloc", "hipStreamSynchronize", "hipDeviceSynchronize", "tempered_gradient("):
        assert copied not in text, copied


def test_the_work_array_is_sized_by_the_layout_and_the_null_handle_is_refused_first(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_de.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    assert lib.octo_draws_de_device(None, 0, 0, 8, 8, None, None, None, 8, 0, 0, None, None, None, None, None, None, None, None) == pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_de_device(None, 0, 0, 1, 0, None, None, None, -1, -1, 1, None, None, None, None, None, None, None, None) == pkg.capi.OCTO_EINVAL
    for D, ld in ((1, 4), (14, 72), (64, 5), (3, 257)):
        assert lib.octo_draws_de_work_doubles(D, ld) == (5 * D + 12) * ld
    assert lib.octo_draws_de_work_doubles(0, 8) == 0 and lib.octo_draws_de_work_doubles(3, -1) == 0
