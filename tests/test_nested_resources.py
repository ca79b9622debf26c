"""
Build checks of nested sampling inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_nested.hip): exactly the kernel families listed here are
among the compiled kernels of csrc/draws/build/, one instantiation each, none of them spills a VGPR, uses scratch or carries a private segment
(a chain's coordinate index addresses global memory only), and each stays within k_hmc_leap's register bar; k_draw keeps its own; the four
functions are declared, exported and bound with their parameter counts; the macros agree with the binding's constants and the restatement's;
the shared routines are taken from the shared header, not copied; a NULL handle is refused before anything else; and the main library's
sources did not change. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import companion_checks as cc
import draws_build
import nested_reference as nr

KERNELS = ("k_nested_sort", "k_nested_width", "k_nested_scatter", "k_nested_gather", "k_nested_open", "k_nested_round", "k_nested_report")
CUBE_KERNELS = ("k_cube", "k_from_cube")
REGISTER_BAR = 128      # VGPRs + AGPRs: k_hmc_leap's bar, four waves per SIMD at the least
MACROS = dict(PURPOSE_NESTED_SEED=(10, nr.PURPOSE_NESTED_SEED), PURPOSE_NESTED_MOVE=(11, nr.PURPOSE_NESTED_MOVE), NESTED_MAX_LIVE=(4096, nr.MAX_LIVE),
              NESTED_MAX_STEPS=(64, nr.MAX_STEPS), NESTED_MAX_SHRINK=(64, nr.MAX_SHRINK), NESTED_MAX_PASSES=(1024, nr.MAX_PASSES),
              NESTED_ACTIVE=(0, nr.ACTIVE), NESTED_DONE=(1, nr.DONE))
N_PARAMETERS = {"octo_draws_cube_device": 7, "octo_draws_from_cube_device": 8, "octo_draws_nested_cull_device": 19, "octo_draws_nested_move_device": 26}
SOURCE = cc.CSRC / "draws" / "octo_draws_nested.hip"


def test_nested_kernels_are_built_without_scratch_within_the_register_bar():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_nested")} == set(KERNELS), sorted(built)
    assert {k for k in built if "cube" in k} == set(CUBE_KERNELS), sorted(built)
    for family in KERNELS + CUBE_KERNELS:
        rows = built[family]
        assert len(rows) == 1, (family, [r["name"] for r in rows])
        r = rows[0]
        assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
        assert r["vgpr_count"] + r["agpr_count"] <= REGISTER_BAR, (family, r["vgpr_count"], r["agpr_count"])
    assert draws_build.FEATURES["hmc"]["kernels"]["k_hmc_leap"][1] == REGISTER_BAR
    draws_build.check_kernels("prior_draws")      # k_draw, which now shares draw_block with k_from_cube, keeps its bar of 64


def test_nested_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_nested.hip")


def test_nested_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for name, n in N_PARAMETERS.items():
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported, name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    for method in ("cube", "from_cube", "nested_state", "nested_cull", "nested_move", "nested_step"):
        assert callable(getattr(draws.PriorDraws, method)), method
    assert callable(pkg.octofit_nested_device)
    assert len(draws.NESTED_MOVE_OUTPUTS) == 7 and len(draws.NESTED_STATE) == 6


def test_nested_macros_are_the_bindings_constants():
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for name, (value, restated) in MACROS.items():
        assert ("#define", f"OCTO_DRAWS_{name}", str(value)) in lines, name      # the whole line
        assert getattr(draws, name) == value == restated, name


def test_the_shared_routines_are_used_not_copied():
    text = SOURCE.read_text()
    for routine in ("chain_of(", "target_at(", "run_rounds(", "draw_block(", "cube_link(", "sampler_head(", "philox4x64("):
        assert routine in text, routine
    for copied in ("prior_density_lanes(", "prior_link_lanes(", "prior_quantile(", "prior_link_forward(", "normcdfinv(", "atomicAdd(double", "tempered_gradient(",
                   ".grad(", "__device__ __forceinline__ void philox4x64"):
        assert copied not in text, copied
    # k_draw and k_from_cube make a draw by the same routine of the shared header, and the move's round has the quantile at one call site
    common = (cc.CSRC / "draws" / "octo_draws_common.h").read_text()
    assert "void draw_block(" in common and "double cube_link(" in common
    assert "draw_block(" in (cc.CSRC / "draws" / "octo_draws.hip").read_text()
    assert sum(line.split("//")[0].count("cube_link(") for line in text.splitlines()) == 1


def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_nested.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    einval = pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_cube_device(None, 0, 0, 1, 1, None, None) == einval
    assert lib.octo_draws_from_cube_device(None, 1, 1, None, None, None, None, None) == einval
    assert lib.octo_draws_nested_cull_device(None, 0, 0, 2, 2, None, None, None, 1, 1, 0, 1, None, None, None, None, None, None, None) == einval
    assert lib.octo_draws_nested_move_device(None, 0, 0, 2, 2, None, None, None, 1, 1, None, None, 1.0, 1, 1, 1, 0, 0, None, None, None, None, None, None, None,
                                             None) == einval
