"""
What the build of liboctofitter_hip_draws.so has to show, feature by feature, and the checks that hold it to that; the callers are
tests/test_draws_resources.py and the samplers' tests/test_hmc_resources.py, test_adapt_resources.py, test_nuts_resources.py. A plain
module, not a conftest and not a test module. The library is built and its code objects are disassembled (tools/kernel_resources.py)
once a session, whichever file asks first; a check that fails is made again by the next caller, so each reports it. The header, the
exports and the binding are compared as a whole by one test of tests/test_draws_resources.py. Every assertion carries its own message
(pytest does not rewrite the assertions of a plain module). The bodies every companion library shares are in tests/companion_checks.py.
"""
import functools

import adapt_reference
import companion_checks as cc
import lbfgs_reference
import pathfinder_reference

# One row a feature:
#   kernels      family -> (instantiations, or None for "at least one"; the most VGPRs + AGPRs of any, or None for no bar of its own)
#   only         a prefix under which the library has the families of `kernels` and no other
#   functions    what the header declares, the library exports and the binding binds
#   constants    header macro (after OCTO_DRAWS_), which is the binding's name too -> (value, the restatement's value or None)
#   package      callables of the package; handle: callables of host/draws.py's PriorDraws
FEATURES = {
    "prior_draws": dict(
        # the draw kernel is one thread per draw with no loop over the coordinates: held to the registers of eight waves per SIMD
        kernels={"k_draw": (None, 64), "k_topk": (None, None), "k_loglike": (None, None), "k_max": (None, None), "k_count": (None, None), "k_scan": (None, None),
                 "k_scatter": (None, None)},
        functions={"octo_draws_create", "octo_draws_destroy", "octo_draws_sample_device", "octo_draws_best", "octo_draws_rejection", "octo_draws_last_error"}),
    "hmc": dict(
        # k_hmc_leap: the start point, a point inside the trajectory, the end point; no coefficient table hoisted out of the coordinate
        # loops: four waves per SIMD at the least
        kernels={"k_hmc_leap": (3, 128), "k_hmc_momentum": (1, 64)},
        functions={"octo_draws_momentum_device", "octo_draws_hmc_step_device", "octo_draws_hmc_step"},
        constants={"PURPOSE_MOMENTUM": (2, None), "PURPOSE_ACCEPT": (3, None)}),
    "lbfgs": dict(
        # k_lbfgs_advance: the opening launch, a round, the outputs alone; a per-lane ring position never indexes a private array
        kernels={"k_lbfgs_advance": (3, 128), "k_lbfgs_direction": (1, 128)},
        functions={"octo_draws_lbfgs_direction_device", "octo_draws_lbfgs_device", "octo_draws_lbfgs"},
        constants={f"LBFGS_{name}": (value, getattr(lbfgs_reference, name))
                   for name, value in (("MAX_M", 8), ("ACTIVE", 0), ("GTOL", 1), ("FTOL", 2), ("LINESEARCH", 3), ("DEAD", 4))},
        package=("optimize_starting_points_device",), handle=("lbfgs", "lbfgs_direction")),
    "pathfinder": dict(
        # no template: one instantiation each; nothing of a chain lives in a private array
        kernels={k: (1, 128) for k in ("k_pf_open", "k_pf_fit", "k_pf_normals", "k_pf_map", "k_pf_elbo", "k_pf_mask")}, only="k_pf_",
        functions={"octo_draws_pathfinder_fit_device", "octo_draws_pathfinder_device", "octo_draws_pathfinder_draw_device"},
        constants={"PF_MAX_D": (64, pathfinder_reference.MAX_D), "PF_MAX_ELBO_DRAWS": (32, pathfinder_reference.MAX_ELBO_DRAWS),
                   "PURPOSE_ELBO": (4, pathfinder_reference.PURPOSE_ELBO), "PURPOSE_PATHFINDER": (5, pathfinder_reference.PURPOSE_PATHFINDER)},
        package=("pathfinder_device",), handle=("pathfinder_fit", "pathfinder", "pathfinder_draw")),
    "adapt": dict(
        # k_adapt_partials, a template on whether its one row is the acceptance probability made on the fly, has its two
        kernels={"k_adapt_partials": (2, 128), "k_adapt_merge": (1, 128), "k_adapt_metric": (1, 128), "k_adapt_init": (1, 128), "k_adapt_da": (1, 128),
                 "k_adapt_eps": (1, 128), "k_adapt_chain": (1, 128)}, only="k_adapt_",
        functions={"octo_draws_moments_device", "octo_draws_metric_device", "octo_draws_hmc_adapt_init_device", "octo_draws_hmc_adapt_device",
                   "octo_draws_chain_moments_device"},
        constants={"MAX_GROUPS": (64, adapt_reference.MAX_GROUPS)},
        package=("warmup_windows", "hmc_warmup", "octofit_hmc_device", "octofit_pt_device"), handle=("moments", "metric", "adapt_init", "adapt_step", "chain_moments")),
    "nuts": dict(
        # k_nuts_leaf keeps k_hmc_leap's register bar: no table hoisted out of the coordinate loops
        kernels={"k_nuts_open": (1, 128), "k_nuts_leaf": (1, 128), "k_nuts_report": (None, None)},
        functions={"octo_draws_nuts_device"},
        constants={"PURPOSE_NUTS_DIRECTION": (6, None), "PURPOSE_NUTS_LEAF": (7, None), "PURPOSE_NUTS_MERGE": (8, None), "NUTS_MAX_DEPTH": (10, None)},
        package=("octofit_nuts_device", "octofit_hmc_device", "hmc_warmup"), handle=("nuts", "nuts_step")),
}


@functools.lru_cache(maxsize=None)
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()           # no-ops when csrc/build/ and csrc/draws/build/ are up to date
    return build_draws()


@functools.lru_cache(maxsize=None)
def kernels():
    """family -> its rows of tools/kernel_resources.py; every kernel of the build disassembled once, none of them with a spilled VGPR, a
    scratch instruction or a private segment"""
    draws_lib()
    rows, names = cc.check_kernels_have_no_scratch("draws", sgpr_too=False)
    by_family = {name: [] for name in names}
    for r in rows:
        by_family[r["name"].split("(")[0].split("<")[0].replace("void ", "")].append(r)
    return by_family


def check_kernels(feature):
    """the feature's kernel families are in the build with their instantiation counts and under their register bars"""
    row, built = FEATURES[feature], kernels()
    assert set(row["kernels"]) <= set(built), (feature, sorted(built))
    if "only" in row:
        assert {k for k in built if k.startswith(row["only"])} == set(row["kernels"]), (feature, sorted(built))
    for family, (count, bar) in row["kernels"].items():
        mine = built[family]
        assert mine and (count is None or len(mine) == count), (feature, family, [r["name"] for r in mine])
        assert bar is None or all(r["vgpr_count"] + r["agpr_count"] <= bar for r in mine), (feature, [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in mine])


def check_header_library_and_binding_agree():
    """the header declares, the library exports and host/draws.py binds the same functions with the same parameter counts, those of every
    row among them"""
    from octofitter_jl_amd.host import draws
    cc.check_header_library_and_binding_agree("draws", draws, draws_lib(), set().union(*(row["functions"] for row in FEATURES.values())), exact=False)


def check_functions_constants_and_callables(pkg, feature):
    """the feature's functions are declared, exported and bound; its constants agree between header, binding and restatement; its callables exist"""
    from octofitter_jl_amd.host import draws
    row = FEATURES[feature]
    header = cc.ROOT / "include" / "octofitter_hip_draws.h"
    missing = row["functions"] - set(cc.declared_functions(header, "octo_draws")), row["functions"] - set(draws.EXPORTED_SYMBOLS), \
        row["functions"] - cc.dynamic_symbols(draws_lib())
    assert not any(missing), (feature, "not declared, not bound, not exported", missing)
    lines = [tuple(line.split()) for line in header.read_text().splitlines()]
    for macro, (value, restated) in row.get("constants", {}).items():
        assert ("#define", f"OCTO_DRAWS_{macro}", str(value)) in lines, (feature, macro)      # the whole line
        assert getattr(draws, macro) == value and (restated is None or restated == value), (feature, macro, getattr(draws, macro), restated)
    assert all(callable(getattr(pkg, f)) for f in row.get("package", ())), (feature, row.get("package"))
    assert all(callable(getattr(draws.PriorDraws, f)) for f in row.get("handle", ())), (feature, row.get("handle"))
