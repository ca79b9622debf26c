"""
The build checks of the nineteenth part of liboctofitter_hip_draws.so (csrc/draws/octo_draws_gp.hip), with tests/draws_build.py and
tests/companion_checks.py as they are. CPU suite: no GPU (hipcc cross-compiles).

The register bars: 256 VGPRs + AGPRs for the two sequential kernels (two waves a SIMD), 128 for the row-parallel ones (k_hmc_leap's bar). As built:
k_gp_factor 79-83 / 112-114 / 206-208 at R' = 2 / 4 / 8, k_gp_back 100 / 118 / 228, k_gp_rows 64, k_gp_adj 88, k_gp_finish 104.
"""
import re

import companion_checks as cc
import draws_build
import gp_cases as gc
import gp_reference as gref

KERNELS = {"k_gp_rows": (1, 128), "k_gp_factor": (6, 256), "k_gp_back": (3, 256), "k_gp_adj": (1, 128), "k_gp_finish": (1, 128)}      # family: (instantiations, bar)
FUNCTIONS = dict(octo_draws_gp_set=12, octo_draws_gp_clear=1, octo_draws_gp_work_doubles=5, octo_draws_gp_eval_device=14, octo_draws_gp_eval=12,
                 octo_draws_gp_values_device=11, octo_draws_gp_bind=3, octo_draws_gp_unbind=1)
SOURCE = cc.CSRC / "draws" / "octo_draws_gp.hip"


def test_exactly_the_gp_kernels_are_built_without_scratch():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_gp_")} == set(KERNELS), sorted(built)
    for family, (count, _) in KERNELS.items():
        assert len(built[family]) == count, (family, [r["name"] for r in built[family]])
        for r in built[family]:
            assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
    for prefix in {p["only"] for p in draws_build.FEATURES.values() if "only" in p}:
        assert not any(k.startswith(prefix) for k in KERNELS), prefix      # no other feature's prefix matches


def test_every_kernel_is_under_its_bar():
    built = draws_build.kernels()
    over = [(r["name"], r["vgpr_count"], r["agpr_count"]) for family, (_, bar) in KERNELS.items() for r in built[family] if r["vgpr_count"] + r["agpr_count"] > bar]
    for family in KERNELS:
        print([(r["name"], r["vgpr_count"], r["agpr_count"], r["group_segment_fixed_size"]) for r in built[family]])
    assert not over, over


def test_gp_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_gp.hip")


def test_gp_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for name, n in FUNCTIONS.items():
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported, name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    assert "draws_gp_accumulate" not in exported      # what the expression program takes from the unit stays inside the library
    for f in ("gp_set", "gp_clear", "gp_eval", "gp_eval_host", "gp_values", "gp_bind", "gp_unbind", "gp_work_doubles"):
        assert callable(getattr(draws.PriorDraws, f)), f


def test_the_constants_agree_in_the_header_the_binding_and_the_reference(pkg):
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for macro, value in (("GP_MAX_K", 4), ("GP_MAX_TERMS", 4), ("GP_MAX_SLOTS", 8), ("GP_SEGMENT", 16), ("GP_REAL", 0), ("GP_COMPLEX", 1), ("GP_SHO", 2)):
        assert ("#define", f"OCTO_DRAWS_{macro}", str(value)) in lines and getattr(draws, macro) == value, macro
    assert (gref.MAX_K, gref.MAX_TERMS, gref.MAX_SLOTS, gref.SEGMENT, gref.ROWS) == (4, 4, 8, 16, draws.SCAN_ROWS) and gc.G == 16
    assert (gref.REAL, gref.COMPLEX, gref.SHO) == (0, 1, 2) and gref.N_HYPER == draws.GP_N_HYPER and gref.N_SLOTS == draws.GP_N_SLOTS
    text = SOURCE.read_text()
    for routine in ("walker_setup(", "kepler_solve<2, false>(", "planet_finish<", "setup_valid<true>(", "grow_to(", "gp_work", "gp_staging", "OCTO_DRAWS_GP_SEGMENT",
                    "OCTO_DRAWS_SCAN_ROWS"):
        assert routine in text, routine
    for absent in ("atomicAdd(", "hipDeviceSynchronize", "hipGraph"):
        assert absent not in text, absent
    assert set(re.findall(r"\bvoid (k_\w+)\(", text)) == set(KERNELS)


def test_the_null_handle_is_refused_first_and_the_work_formula(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    einval = pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_gp_set(None, None, 0, None, None, None, None, None, -1, 0, None, 0) == einval
    assert lib.octo_draws_gp_clear(None) == einval and lib.octo_draws_gp_unbind(None) == einval
    assert lib.octo_draws_gp_eval_device(None, None, 0, -1, None, None, None, None, None, None, None, None, 0, None) == einval
    assert lib.octo_draws_gp_eval(None, None, 0, -1, None, None, None, None, None, None, None, None) == einval
    assert lib.octo_draws_gp_values_device(None, None, 0, -1, None, None, None, None, None, 0, None) == einval
    assert lib.octo_draws_gp_bind(None, None, 0) == einval
    G, R = gref.SEGMENT, gref.ROWS
    for n, slots, P, W in ((1, 1, 1, 1), (53, 5, 8, 130), (5000, 8, 2, 10048), (200, 3, 1, 64)):
        rp = 2 if slots <= 2 else 4 if slots <= 4 else 8
        ns, ldw = rp * (rp + 1) // 2 + rp, -(-W // 64) * 64
        assert lib.octo_draws_gp_work_doubles(n, slots, P, W, 0) == ldw * (n + 1)
        assert lib.octo_draws_gp_work_doubles(n, slots, P, W, 1) == ldw * (n + 1 + (-(-n // G) + G) * ns + -(-n // R) * (4 + 6 * P))
    assert lib.octo_draws_gp_work_doubles(0, 1, 1, 1, 0) == -1 and lib.octo_draws_gp_work_doubles(5, 9, 1, 1, 0) == -1
