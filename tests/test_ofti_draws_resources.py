"""
Build checks of the OFTI rejection sampler inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_ofti.hip), modelled on
tests/test_de_resources.py: exactly its three kernel families are among the compiled kernels of csrc/draws/build/ under their prefix, one
instantiation each, none of them spills a VGPR, uses scratch or carries a private segment, and each stays within k_hmc_leap's register bar; the
functions are declared, exported and bound with their parameter counts; the purpose is 13 in the header, the binding and the restatement; the
generator and the layout routines are taken from the shared headers, not copied, and the unit allocates nothing by itself; a NULL handle is
refused before anything else; and the main library's sources did not change. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import re

import companion_checks as cc
import draws_build
import ofti_draws_reference as oref

KERNELS = ("k_oftis_nl", "k_oftis_ll", "k_oftis_post")
REGISTER_BAR = 128      # VGPRs + AGPRs: k_hmc_leap's bar, four waves per SIMD at the least
FUNCTIONS = dict(octo_draws_ofti_set=12, octo_draws_ofti_clear=1, octo_draws_ofti_nl_device=6, octo_draws_ofti_posterior_device=8, octo_draws_ofti_rejection=11)
SOURCE = cc.CSRC / "draws" / "octo_draws_ofti.hip"


def test_ofti_kernels_are_built_without_scratch_within_the_register_bar():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_oftis_")} == set(KERNELS), sorted(built)
    for family in KERNELS:
        rows = built[family]
        assert len(rows) == 1, (family, [r["name"] for r in rows])
        r = rows[0]
        assert r["vgpr_spill_count"] == 0 and r["scratch_instructions"] == 0 and r["private_segment_fixed_size"] == 0, (family, r)
        assert r["vgpr_count"] + r["agpr_count"] <= REGISTER_BAR, (family, r["vgpr_count"], r["agpr_count"])
    assert draws_build.FEATURES["hmc"]["kernels"]["k_hmc_leap"][1] == REGISTER_BAR
    draws_build.check_kernels("prior_draws")      # the rejection's kernels, which the driver launches unchanged, are where they were


def test_ofti_draws_add_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_ofti.hip")


def test_ofti_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    decl = cc.declared_functions(cc.ROOT / "include" / "octofitter_hip_draws.h", "octo_draws")
    exported = cc.dynamic_symbols(draws_build.draws_lib())
    for name, n in FUNCTIONS.items():
        assert name in decl and name in draws.EXPORTED_SYMBOLS and name in exported, name
        assert decl[name] == n == len(draws._SIGS[name][1]), name
    assert not {"draws_launch_draw", "draws_max_pass", "draws_accept_pass"} & exported      # what the unit takes from octo_draws.hip stays inside the library
    for f in ("ofti_set", "ofti_clear", "ofti_nl", "ofti_posterior", "ofti_rejection"):
        assert callable(getattr(draws.PriorDraws, f)), f
    assert callable(pkg.octofit_ofti_device)
    assert len(draws.OFTI_OUTPUTS) == draws.OFTI_N_OUT == oref.N_OUT == 16 and draws.OFTI_OUTPUTS == oref.OUTPUTS


def test_the_purpose_is_13_in_the_header_the_binding_and_the_restatement():
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    assert ("#define", "OCTO_DRAWS_PURPOSE_OFTI", "13") in lines and ("#define", "OCTO_DRAWS_OFTI_N_OUT", "16") in lines      # the whole lines
    assert draws.PURPOSE_OFTI == 13 == oref.PURPOSE_OFTI
    text = SOURCE.read_text()
    assert "OCTO_DRAWS_PURPOSE_OFTI" in text and "OCTO_DRAWS_OFTI_N_OUT" in text      # the kernel reads the header's constants, not literals of its own
    purposes = [int(l[2]) for l in lines if len(l) == 3 and l[0] == "#define" and l[1].startswith("OCTO_DRAWS_PURPOSE_")]
    assert len(purposes) == len(set(purposes)), purposes


def test_the_shared_routines_are_used_and_not_copied():
    text = SOURCE.read_text()
    for routine in ("philox4x64(", "u01(", "grow_to(", "ofti_work", "ofti_rows", "kepler_solve<-1, false>(", "constant_rows(", "draws_launch_draw(", "draws_max_pass(",
                    "draws_accept_pass(", "octo_ofti_create(", "octo_ofti_eval_device(", "main_call("):
        assert routine in text, routine
    for copied in ("void philox4x64", "double u01", "PHILOX_M0", "hipMalloc", "hipFree", "atomicAdd(", "hipGraph", "hipDeviceSynchronize"):
        assert copied not in text, copied
    # the unit defines and launches its own three kernels and no other: the rejection's are launched where they live (comments may name them)
    assert set(re.findall(r"\bvoid (k_\w+)\(", text)) == set(KERNELS)
    assert set(re.findall(r"hipLaunchKernelGGL\((\w+)", text)) == set(KERNELS)
    main = (cc.CSRC / "draws" / "octo_draws.hip").read_text()
    for kernel in ("k_max", "k_count", "k_scan", "k_scatter"):      # launched once each, from the routines both drivers call
        assert len(re.findall(rf"hipLaunchKernelGGL\({kernel}\b", main)) == 1, kernel
    assert main.count("draws_max_pass(") == 2 and main.count("draws_accept_pass(") == 2      # the definition and octo_draws_rejection's call
    layout = (cc.CSRC / "draws" / "octo_draws_layout.h").read_text()
    assert "struct OftiWork" in layout and "struct OftiRows" in layout and "carve_at(" in (cc.CSRC / "draws" / "octo_draws_common.h").read_text()


def test_the_null_handle_is_refused_first(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_ofti_draws.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    einval = pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_ofti_set(None, None, None, None, None, None, None, -1, -1.0, 7, 0.0, None) == einval
    assert lib.octo_draws_ofti_clear(None) == einval
    assert lib.octo_draws_ofti_nl_device(None, -1, 0, None, None, None) == einval
    assert lib.octo_draws_ofti_posterior_device(None, 0, -1, 0, None, None, None, None) == einval
    assert lib.octo_draws_ofti_rejection(None, 0, 0, 0, -1, None, None, None, None, None, None) == einval
