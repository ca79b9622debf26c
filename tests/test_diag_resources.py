"""
Build checks of the convergence diagnostics inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_diag.hip): its kernel families are among
the compiled kernels of csrc/draws/build/, one instantiation each, and none of them spills, uses scratch or carries a private segment (the
sliding window of k_diag_acov lives in registers); the three functions are declared, exported and bound; the macros agree with the binding's
constants and the restatement's; the work size is the documented formula, with no device; a NULL handle is refused before anything else; and
the main library's sources did not change. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import companion_checks as cc
import diag_reference as ref
import draws_build

KERNELS = ("k_diag_keys", "k_diag_sort_local", "k_diag_sort_global", "k_diag_quant", "k_diag_rank", "k_diag_moments", "k_diag_acov", "k_diag_finish")
FUNCTIONS = {"octo_draws_diagnose_device", "octo_draws_rank_device", "octo_draws_diagnose_work_doubles"}
MACROS = dict(RHAT=0, ESS_BULK=1, ESS_TAIL=2, RHAT_BASIC=3, ESS_BASIC=4, Q05=5, Q50=6, Q95=7, N_STATS=8)


def test_diag_kernels_are_built_without_scratch():
    built = draws_build.kernels()      # fails on any kernel of the build with a spilled VGPR, a scratch instruction or a private segment
    assert {k for k in built if k.startswith("k_diag_")} == set(KERNELS), sorted(built)
    for family in KERNELS:
        rows = built[family]
        assert len(rows) == 1, (family, [r["name"] for r in rows])
        assert rows[0]["vgpr_count"] + rows[0]["agpr_count"] <= 160, (family, rows[0]["vgpr_count"], rows[0]["agpr_count"])      # three waves per SIMD at the least
    assert built["k_diag_acov"][0]["vgpr_count"] >= 64      # sixteen sums and a window of sixteen doubles are held in registers


def test_diag_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_diag.hip")


def test_diag_functions_are_declared_exported_and_bound(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.check_header_library_and_binding_agree()
    header = cc.ROOT / "include" / "octofitter_hip_draws.h"
    decl = cc.declared_functions(header, "octo_draws")
    assert FUNCTIONS <= set(decl) and FUNCTIONS <= set(draws.EXPORTED_SYMBOLS) and FUNCTIONS <= cc.dynamic_symbols(draws_build.draws_lib())
    assert (decl["octo_draws_diagnose_device"], decl["octo_draws_rank_device"], decl["octo_draws_diagnose_work_doubles"]) == (9, 11, 3)
    assert callable(pkg.diagnose_draws_device) and callable(draws.PriorDraws.diagnose) and callable(draws.PriorDraws.ranks)


def test_diag_macros_are_the_bindings_constants():
    from octofitter_jl_amd.host import draws
    lines = [tuple(line.split()) for line in (cc.ROOT / "include" / "octofitter_hip_draws.h").read_text().splitlines()]
    for name, value in MACROS.items():
        assert ("#define", f"OCTO_DRAWS_DIAG_{name}", str(value)) in lines, name      # the whole line
        assert getattr(draws, f"DIAG_{name}") == value == getattr(ref, name), name
    assert draws.DIAG_NAMES == ref.NAMES and len(draws.DIAG_NAMES) == draws.DIAG_N_STATS


def test_work_size_is_the_documented_formula(pkg):
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib = draws.load_library()
    for n, W, K in ((8, 1, 1), (9, 3, 2), (35, 257, 3), (400, 64, 2), (130, 1100, 1), (16, 2, 64), (1000, 1024, 11), (2048, 1, 1), (8, 1 << 21, 64)):
        N, M = n // 2, 2 * W
        S, P = N * M, 2048
        while P < S:
            P *= 2
        T, nblk = -(-N // 16) * 16, -(-M // 256)
        want = 2 * K * (P + S) + 10 * K * M + 4 * K * T * (nblk + 1) + 5 * K
        assert lib.octo_draws_diagnose_work_doubles(n, W, K) == want == ref.work_doubles(n, W, K), (n, W, K)
    for n, W, K in ((7, 1, 1), (8, 0, 1), (8, 1, 0), (8, 1, 65), (8, (1 << 21) + 1, 1), (1 << 40, 1 << 40, 1)):
        assert lib.octo_draws_diagnose_work_doubles(n, W, K) == 0, (n, W, K)
    for doc in ("include/octofitter_hip_draws.h", "DESIGN.md"):
        assert "2K(P + S) + 10KM + 4K·T·(nblk + 1) + 5K" in (cc.ROOT / doc).read_text(), doc


def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_diag.py."""
    from octofitter_jl_amd.host import draws
    draws_build.draws_lib()
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_diagnose_device(None, 8, 1, 1, 1, 1, None, None, None) == EINVAL
    assert lib.octo_draws_rank_device(None, 8, 1, 1, 1, 1, None, 0, None, None, None) == EINVAL
