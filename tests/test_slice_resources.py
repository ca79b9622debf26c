"""
Build checks of the slice sampler inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_slice.hip): exactly its three kernel families are
among the compiled kernels of csrc/draws/build/, one instantiation each, none of them spills a VGPR, uses scratch or carries a private
segment (a chain's coordinate index addresses global memory only), and each stays within k_hmc_leap's register bar; the function is declared,
exported and bound with its parameter count; the macros agree with the binding's constants and the restatement's; the tempered target is
taken from the shared header, not copied; a NULL handle is refused before anything else; and the main library's sources did not change.
CPU suite: hipcc cross-compiles, no GPU needed.
"""
import companion_checks as cc
import draws_build
import slice_reference as sl

KERNELS = ("k_slice_open", "k_slice_round", "k_slice_report")
REGISTER_BAR = 128      # VGPRs + AGPRs: k_hmc_leap's bar, four waves per SIMD at the least
MACROS = dict(PURPOSE_SLICE=(9, sl.PURPOSE_SLICE), SLICE_MAX_DOUBLINGS=(8, sl.MAX_DOUBLINGS), SLICE_MAX_SHRINK=(64, sl.MAX_SHRINK), SLICE_MAX_PASSES=(1024, sl.MAX_PASSES),
              SLICE_ACTIVE=(0, sl.ACTIVE), SLICE_DONE=(1, sl.DONE), SLICE_DEAD=(2, sl.DEAD))
N_PARAMETERS = 24


def test_slice_kernels_are_built_without_scratch_within_the_register_bar():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_slice")} == set(KERNELS), sorted(built)
    for family in KERNELS:
        rows = built[family]
        assert len(rows) == 1, (family, [r["name"] for r in rows])
        r = rows[0]
        assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
        assert r["vgpr_count"] + r["agpr_count"] <= REGISTER_BAR, (family, r["vgpr_count"], r["agpr_count"])
    assert draws_build.FEATURES["hmc"]["kernels"]["k_hmc_leap"][1] == REGISTER_BAR


def test_slice_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_slice.hip")


def test_slice_function_is_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    name = "octo_draws_slice_device"
    assert name in decl and name in draws.EXPORTED_SYMBOLS and name in cc.dynamic_symbols(draws_build.draws_lib())
    assert decl[name] == N_PARAMETERS == len(draws._SIGS[name][1])
    assert callable(draws.PriorDraws.slice) and callable(draws.PriorDraws.slice_step) and callable(pkg.octofit_pt_device)
    assert len(draws.SLICE_OUTPUTS) == 8


def test_slice_macros_are_the_bindings_constants():
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for name, (value, restated) in MACROS.items():
        assert ("#define", f"OCTO_DRAWS_{name}", str(value)) in lines, name      # the whole line
        assert getattr(draws, name) == value == restated, name


def test_the_tempered_target_is_taken_from_the_shared_header():
    text = (cc.CSRC / "draws" / "octo_draws_slice.hip").read_text()
    for routine in ("chain_of(", "target_at(", "tempered_energy(", "dead_state(", "run_rounds(", "check_sampler_call("):
        assert routine in text, routine
    for copied in ("prior_density_lanes(", "prior_link_lanes(", "__device__ __forceinline__ double tempered_energy", "atomicAdd(double", "tempered_gradient("):
        assert copied not in text, copied


def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_slice.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    assert lib.octo_draws_slice_device(None, 0, 0, 0, 1, 1, None, None, None, 1.0, 3, 1, 64, 0, 0, None, None, None, None, None, None, None, None, None) == pkg.capi.OCTO_EINVAL
