"""
Build checks of the companion library liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, csrc/draws/): what it exports against what
its header declares and host/draws.py binds, that the main library's symbol set did not move, the argument check that needs no device,
and the compiled kernels' resources read from the code objects (tools/kernel_resources.py). CPU suite: hipcc cross-compiles, no GPU needed.
"""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
HEADER = ROOT / "include" / "octofitter_hip_draws.h"
MAIN_LIB = ROOT / "octofitter.jl_amd" / "lib" / "liboctofitter_hip.so"
DRAWS_BUILD = ROOT / "octofitter.jl_amd" / "csrc" / "draws" / "build"


@pytest.fixture(scope="module")
def draws_lib():
    from __graft_entry__ import build_draws, build_hip
    build_hip()           # no-ops when csrc/build/ and csrc/draws/build/ are up to date
    return build_draws()


def declared_functions():
    """{name: number of parameters} of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(octo_draws_\w+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def dynamic_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_library_and_binding_agree(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    decl = declared_functions()
    assert len(decl) >= 6 and {"octo_draws_create", "octo_draws_destroy", "octo_draws_sample_device", "octo_draws_best", "octo_draws_rejection",
                               "octo_draws_last_error"} <= set(decl)
    exported = {s for s in dynamic_symbols(draws_lib) if s.startswith("octo_")}
    assert exported == set(decl), (sorted(exported), sorted(decl))
    assert set(draws.EXPORTED_SYMBOLS) == set(decl)
    lib = draws.load_library()
    for name, n_params in decl.items():
        assert len(draws._SIGS[name][1]) == n_params, name
        assert getattr(lib, name).argtypes is not None


def test_main_library_exports_no_draws_symbol(draws_lib):
    syms = dynamic_symbols(MAIN_LIB)
    assert any(s.startswith("octo_") for s in syms)
    assert not [s for s in syms if s.startswith("octo_draws")]


def test_companion_links_the_main_library_by_origin(draws_lib):
    dyn = subprocess.run(["readelf", "-d", str(draws_lib)], capture_output=True, text=True, check=True).stdout
    assert "liboctofitter_hip.so" in dyn and "$ORIGIN" in dyn


def test_create_with_null_context_is_einval(pkg, draws_lib):
    from octofitter_jl_amd.host import draws
    lib = draws.load_library()
    h = C.c_void_p()
    pr = (pkg.capi.OctoPrior * 1)()
    pr[0].kind, pr[0].p0, pr[0].p1 = pkg.capi.PRIOR_UNIFORM, 0.0, 1.0
    assert lib.octo_draws_create(None, None, pr, 1, 0, C.byref(h)) == pkg.capi.OCTO_EINVAL
    assert not h.value and b"null" in lib.octo_draws_last_error(None)
    assert lib.octo_draws_best(None, 0, 0, 1, 1, None, None, None) == pkg.capi.OCTO_EINVAL
    assert lib.octo_draws_destroy(None) == pkg.capi.OCTO_OK


def test_companion_kernels_have_no_scratch(draws_lib):
    import kernel_resources as kr
    rows = kr.resources(build_dir=DRAWS_BUILD)
    names = {r["name"].split("(")[0] for r in rows}
    assert {"k_draw", "k_topk", "k_loglike", "k_max", "k_count", "k_scan", "k_scatter"} <= names, names
    bad = [(r["name"], r["vgpr_spill_count"], r["scratch_instructions"], r["private_segment_fixed_size"]) for r in rows
           if r["vgpr_spill_count"] or r["scratch_instructions"] or r["private_segment_fixed_size"]]
    assert not bad, bad
    # the draw kernel is one thread per draw with no loop over the coordinates: held to the registers of eight waves per SIMD
    draw = [r for r in rows if r["name"].startswith("k_draw")]
    assert draw and all(r["vgpr_count"] + r["agpr_count"] <= 64 for r in draw), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in draw]
