"""
Build checks of the expression programs of liboctofitter_hip_draws.so (csrc/draws/octo_draws_program.hip): the header, the exports and the
binding name the same functions with the same arity; the part came with no edit directly under csrc/ (the main library's kernels and its
counter evidence are untouched); and its kernels are built without scratch and without a spilled VGPR, read from the code object's metadata
as the other tests/test_*_resources.py do. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import companion_checks as cc
import draws_build

FUNCTIONS = {"octo_draws_program_set", "octo_draws_program_clear", "octo_draws_program_logpost_device", "octo_draws_program_values_device"}
KERNELS = {"k_prog_fwd": 2, "k_prog_values": 1, "k_prog_bwd": 1}      # family -> instantiations


def test_header_library_and_binding_agree(pkg):
    from octofitter_jl_amd.host import draws
    header = cc.check_header_library_and_binding_agree("draws", draws, draws_build.draws_lib(), FUNCTIONS, exact=False)
    assert "OCTO_DRAWS_PROGRAM_MAX_OPS 192" in header
    assert all(callable(getattr(draws.PriorDraws, f)) for f in ("program_set", "program_clear", "program_logpost", "program_values"))
    assert callable(pkg.Derived) and callable(pkg.derived.lower)


def test_program_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_program.hip")


def test_kernels_are_built_without_scratch():
    built = draws_build.kernels()      # every kernel of the build: no spilled VGPR, no scratch instruction, no private segment
    assert {k for k in built if k.startswith("k_prog_")} == set(KERNELS), sorted(built)
    for family, count in KERNELS.items():
        rows = built[family]
        assert len(rows) == count, (family, [r["name"] for r in rows])
        for r in rows:
            assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, r["name"]
            assert r["vgpr_count"] + r["agpr_count"] <= 256, (r["name"], r["vgpr_count"], r["agpr_count"])      # two waves a SIMD at the least
