"""
The build checks of the twentieth part of liboctofitter_hip_draws.so (csrc/draws/octo_draws_gpd.hip: the Gaussian-process RV table under dense kernels), with
tests/draws_build.py and tests/companion_checks.py as they are. CPU suite: no GPU (hipcc cross-compiles).

The register bar is 128 VGPRs + AGPRs for every k_gpd_ kernel (four waves a SIMD; one workgroup of four waves a walker). As built: k_gpd_factor 82 (LDS) /
84 (work array), k_gpd_grad 112 / 112; no static LDS (the triangle and the vectors are dynamic: 8·(n(n + 1)/2 + 4n + 128) bytes, 155 392 at 192 rows).
"""
import re

import companion_checks as cc
import draws_build
import gpd_reference as dref

KERNELS = {"k_gpd_factor": (2, 128), "k_gpd_grad": (2, 128)}      # family: (instantiations: the triangle in LDS and in the work array; bar)
SOURCE = cc.CSRC / "draws" / "octo_draws_gpd.hip"
CONSTANTS = (("GP_SE", 16), ("GP_MATERN32", 17), ("GP_MATERN52", 18), ("GP_PERIODIC", 19), ("GP_QUASIPERIODIC", 20), ("GP_DENSE_LDS_ROWS", 192),
             ("GP_DENSE_MAX_N", 2048))


def test_exactly_the_gpd_kernels_are_built_without_scratch():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_gpd_")} == set(KERNELS), sorted(built)
    for family, (count, bar) in KERNELS.items():
        assert len(built[family]) == count, (family, [r["name"] for r in built[family]])
        for r in built[family]:
            print(r["name"], r["vgpr_count"], r["agpr_count"], r["group_segment_fixed_size"])
            assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
            assert r["vgpr_count"] + r["agpr_count"] <= bar, (r["name"], r["vgpr_count"], r["agpr_count"])
    text = SOURCE.read_text()
    assert set(re.findall(r"\bvoid (k_\w+)\(", text)) == set(KERNELS)
    for absent in ("atomicAdd(", "hipDeviceSynchronize", "hipGraph"):
        assert absent not in text, absent
    for present in ("static_assert(gpd_lds_bytes(GPD_LDS_ROWS, true) <= GPD_LDS_LIMIT", "hipDeviceAttributeMaxSharedMemoryPerBlock", "setup_valid<true>("):
        assert present in text, present


def test_gpd_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_gpd.hip")


def test_the_new_export_is_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    name = "octo_draws_gp_dense_work_doubles"
    assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported
    assert decl[name] == 4 == len(draws._SIGS[name][1])
    assert not {s for s in exported if s.startswith("draws_gpd_")}      # what octo_draws_gp.hip takes from the unit stays inside the library


def test_the_constants_agree_in_the_header_the_binding_and_the_reference(pkg):
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for macro, value in CONSTANTS:
        assert ("#define", f"OCTO_DRAWS_{macro}", str(value)) in lines and getattr(draws, macro) == value, macro
    assert (dref.SE, dref.MATERN32, dref.MATERN52, dref.PERIODIC, dref.QUASIPERIODIC) == (16, 17, 18, 19, 20)
    assert (dref.LDS_ROWS, dref.MAX_N, dref.MAX_TERMS) == (draws.GP_DENSE_LDS_ROWS, draws.GP_DENSE_MAX_N, draws.GP_MAX_TERMS)
    assert dref.N_HYPER == draws.GP_DENSE_N_HYPER and draws.GP_N_HYPER == {0: 2, 1: 4, 2: 3} and draws.GP_N_SLOTS == {0: 1, 1: 2, 2: 2}
    assert pkg.gp.QUASIPERIODIC == draws.GP_QUASIPERIODIC and pkg.gp.SE == draws.GP_SE


def test_the_null_handle_is_refused_first_and_the_work_formula(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    kinds = (draws.C.c_int32 * 1)(draws.GP_QUASIPERIODIC)
    assert lib.octo_draws_gp_set(None, None, 0, None, None, None, None, None, -1, 0, kinds, 1) == pkg.capi.OCTO_EINVAL
    L, R = dref.LDS_ROWS, 8      # OCTO_DRAWS_SCAN_ROWS
    assert draws.SCAN_ROWS == R
    for n, P, W in ((1, 1, 1), (L, 2, 130), (L + 1, 8, 3), (2048, 1, 64)):
        ldw, tri = -(-W // 64) * 64, (W * n * (n + 1) // 2 if n > L else 0)
        assert lib.octo_draws_gp_dense_work_doubles(n, P, W, 0) == ldw * (n + 1) + tri, (n, P, W)
        assert lib.octo_draws_gp_dense_work_doubles(n, P, W, 1) == ldw * (n + 1 + -(-n // R) * (4 + 6 * P)) + tri, (n, P, W)
    for bad in ((0, 1, 1), (2049, 1, 1), (5, 0, 1), (5, 9, 1), (5, 1, -1)):
        assert lib.octo_draws_gp_dense_work_doubles(*bad, 0) == -1, bad
