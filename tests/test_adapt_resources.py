"""
Build checks of the warm-up statistics inside liboctofitter_hip_draws.so (csrc/draws/octo_draws_adapt.hip): its kernels are among the compiled
kernels of csrc/draws/build/, none of them spills, uses scratch or carries a private segment, each has at most 128 VGPRs and one
instantiation — k_adapt_partials, a template on whether its one row is the acceptance probability made on the fly, has its two —; the five
functions are declared, exported and bound; OCTO_DRAWS_MAX_GROUPS agrees between header, binding and restatement; the explorer's kernels keep
their instantiation counts. CPU suite: hipcc cross-compiles, no GPU needed.
"""
import pytest

import adapt_reference as ref
import companion_checks as cc

KERNELS = {"k_adapt_partials": 2, "k_adapt_merge": 1, "k_adapt_metric": 1, "k_adapt_init": 1, "k_adapt_da": 1, "k_adapt_eps": 1, "k_adapt_chain": 1}
FUNCTIONS = {"octo_draws_moments_device", "octo_draws_metric_device", "octo_draws_hmc_adapt_init_device", "octo_draws_hmc_adapt_device",
             "octo_draws_chain_moments_device"}


@pytest.fixture(scope="module")
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    return build_draws()


def test_adapt_kernels_are_built_without_scratch(draws_lib):
    rows, names = cc.check_kernels_have_no_scratch("draws", sgpr_too=False)
    assert set(KERNELS) <= names, names
    mine = [r for r in rows if "k_adapt_" in r["name"]]
    for name, count in KERNELS.items():
        assert len([r for r in mine if name in r["name"]]) == count, (name, [r["name"] for r in mine])
    assert len(mine) == sum(KERNELS.values())
    assert all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in mine), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in mine]
    # the explorer is called, not edited: its kernels as tests/test_hmc_resources.py counts them
    assert len([r for r in rows if "k_hmc_leap" in r["name"]]) == 3 and len([r for r in rows if "k_hmc_momentum" in r["name"]]) == 1


def test_adapt_adds_nothing_to_the_main_library():
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/draws/octo_draws_adapt.hip")


def test_adapt_functions_are_declared_exported_and_bound(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    text = cc.check_header_library_and_binding_agree("draws", draws, draws_lib, FUNCTIONS, exact=False)
    assert any(line.split() == ["#define", "OCTO_DRAWS_MAX_GROUPS", "64"] for line in text.splitlines())
    assert draws.MAX_GROUPS == 64 == ref.MAX_GROUPS
    assert all(callable(getattr(pkg, f)) for f in ("warmup_windows", "hmc_warmup", "octofit_hmc_device", "octofit_pt_device"))
    assert all(callable(getattr(draws.PriorDraws, f)) for f in ("moments", "metric", "adapt_init", "adapt_step", "chain_moments"))


def test_argument_checks_that_need_no_device(pkg, draws_lib):
    """Without a device no handle can be made: the NULL handle is refused before anything else; the rest is in tests/test_adapt.py."""
    from octofitter_jl_amd.host import draws
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_moments_device(None, 4, 4, 1, None, None, 1, 0, None, None, None, None) == EINVAL
    assert lib.octo_draws_metric_device(None, 1, None, None, None, 1, None, None) == EINVAL
    assert lib.octo_draws_hmc_adapt_init_device(None, 1, None, 0.1, None, None) == EINVAL
    assert lib.octo_draws_hmc_adapt_device(None, 4, None, 1, None, None, 1, 0.8, 0.05, 10.0, 0.75, None, None, 0, None, None) == EINVAL
    assert lib.octo_draws_chain_moments_device(None, 4, 4, 1, 1, None, None, None, None) == EINVAL
