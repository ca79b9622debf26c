"""
Build checks of the companion library liboctofitter_hip_psis.so (include/octofitter_hip_psis.h, csrc/psis/): what it exports against what its
header declares and host/psis.py binds, that the main library's symbol set and sources did not move and that it links nothing of it, the
argument checks that need no device, and the compiled kernels' resources read from the code objects (tools/kernel_resources.py). CPU suite:
hipcc cross-compiles.
"""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
HEADER = ROOT / "include" / "octofitter_hip_psis.h"
MAIN_LIB = ROOT / "octofitter.jl_amd" / "lib" / "liboctofitter_hip.so"
PSIS_BUILD = ROOT / "octofitter.jl_amd" / "csrc" / "psis" / "build"


@pytest.fixture(scope="module")
def psis_lib():
    from __graft_entry__ import build_hip, build_psis
    build_hip()           # no-ops when csrc/build/ and csrc/psis/build/ are up to date
    return build_psis()


def declared_functions():
    """{name: number of parameters} of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(octo_psis_\w+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def dynamic_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_library_and_binding_agree(pkg, psis_lib):
    ps = pkg.psis
    decl = declared_functions()
    assert {"octo_psis_create", "octo_psis_destroy", "octo_psis_last_error", "octo_psis_sync", "octo_psis_tail_len", "octo_psis_loo_device",
            "octo_psis_loo", "octo_psis_max_samples"} == set(decl)
    exported = {s for s in dynamic_symbols(psis_lib) if s.startswith("octo_")}
    assert exported == set(decl), (sorted(exported), sorted(decl))
    assert set(ps.EXPORTED_SYMBOLS) == set(decl)
    lib = ps.load_library()
    for name, n_params in decl.items():
        assert len(ps._SIGS[name][1]) == n_params, name
        assert getattr(lib, name).argtypes is not None
    # the constants of the binding are those of the header
    text = HEADER.read_text()
    for k, name in enumerate(ps.STAT_FIELDS):
        assert re.search(rf"#define OCTO_PSIS_{name.upper()}\s+{k}\b", text), name
    assert re.search(rf"#define OCTO_PSIS_N_STATS\s+{ps.N_STATS}\b", text) and ps.N_STATS == len(ps.STAT_FIELDS)
    # … and the package exports the class and the caller
    assert pkg.Psis is ps.Psis and callable(pkg.loo)


def test_main_library_exports_no_psis_symbol(psis_lib):
    syms = dynamic_symbols(MAIN_LIB)
    assert any(s.startswith("octo_") for s in syms)
    assert not [s for s in syms if s.startswith("octo_psis")]


def test_companion_links_nothing_of_the_main_library(psis_lib):
    dyn = subprocess.run(["readelf", "-d", str(psis_lib)], capture_output=True, text=True, check=True).stdout
    assert "liboctofitter_hip" not in dyn


def _git(*args):
    return subprocess.run(["git", "-C", str(ROOT), *args], capture_output=True, text=True)


def test_main_library_sources_untouched():
    """The PSIS library came with no change to a file directly under csrc/ (kernel_source_hash() covers exactly those, and the committed
    counter evidence is keyed to it): neither the commit that added include/octofitter_hip_psis.h nor, while that header is still
    uncommitted, the working tree differs from its parent there."""
    if _git("rev-parse", "--is-inside-work-tree").stdout.strip() != "true":
        pytest.skip("not a git checkout")
    files = [":(glob)octofitter.jl_amd/csrc/*.h", ":(glob)octofitter.jl_amd/csrc/*.hip"]      # directly under csrc/: `*` stops at a slash
    added = _git("log", "--diff-filter=A", "--format=%H", "--", "include/octofitter_hip_psis.h").stdout.split()
    if not added:      # the header is not committed yet: the working tree against HEAD
        r = _git("diff", "--quiet", "HEAD", "--", *files)
        assert r.returncode == 0, _git("diff", "--stat", "HEAD", "--", *files).stdout
        untracked = _git("ls-files", "--others", "--exclude-standard", "--", *files).stdout.split()
        assert not untracked, untracked
        return
    commit = added[-1]
    if _git("rev-parse", "--verify", "--quiet", commit + "~").returncode != 0:
        pytest.skip("the parent of the commit that added the header is not in this (shallow) checkout")
    r = _git("diff", "--quiet", commit + "~", commit, "--", *files)
    assert r.returncode == 0, _git("diff", "--stat", commit + "~", commit, "--", *files).stdout


def test_argument_checks_that_need_no_device(pkg, psis_lib):
    import psis_reference as pr
    capi, ps = pkg.capi, pkg.psis
    lib = ps.load_library()
    # M(n), host only: the reference's double-arithmetic formula
    for n in list(range(0, 10001)) + [10 ** 6]:
        assert lib.octo_psis_tail_len(n) == pr.tail_len(n), n
    assert lib.octo_psis_tail_len(-3) == 0
    # the largest S whose tail the sort buffer holds
    s_max = lib.octo_psis_max_samples()
    assert pr.tail_len(s_max) <= ps.MAX_TAIL < pr.tail_len(s_max + 1) and s_max == 1864135
    assert lib.octo_psis_create(0, None) == capi.OCTO_EINVAL                                                # NULL out pointer
    assert b"null out" in lib.octo_psis_last_error(None)
    # calls on a NULL handle
    ll, out = np.zeros((2, 8)), np.zeros((ps.N_STATS, 2))
    assert lib.octo_psis_loo(None, capi._dptr(ll), 8, 2, 8, capi._dptr(out), None, 0) == capi.OCTO_EINVAL
    assert lib.octo_psis_loo_device(None, None, 8, 2, 8, None, None, 0, None) == capi.OCTO_EINVAL
    assert lib.octo_psis_sync(None) == capi.OCTO_EINVAL
    assert lib.octo_psis_destroy(None) == capi.OCTO_OK
    # with a handle (a machine with a device) the shape checks answer before anything is launched; without one, create says so
    h = C.c_void_p()
    st = lib.octo_psis_create(0, C.byref(h))
    assert st in (capi.OCTO_OK, capi.OCTO_ENODEV), (st, lib.octo_psis_last_error(None))
    if st == capi.OCTO_ENODEV:
        assert not h.value and b"no HIP device" in lib.octo_psis_last_error(None)
        with pytest.raises(capi.OctoError) as ex:
            pkg.Psis()
        assert ex.value.status == capi.OCTO_ENODEV
        return
    try:
        lw = np.zeros((2, 8))
        call = lambda ld, R, S, o=out, w=None, ld_w=0, m=ll: lib.octo_psis_loo(h, capi._dptr(m), ld, R, S, capi._dptr(o), capi._dptr(w), ld_w)      # noqa: E731
        assert call(8, -1, 8) == capi.OCTO_EINVAL
        assert call(8, 2, 0) == capi.OCTO_EINVAL
        assert call(7, 2, 8) == capi.OCTO_EINVAL and b"ld" in lib.octo_psis_last_error(h)
        assert call(8, 2, 8, w=lw, ld_w=7) == capi.OCTO_EINVAL
        assert call(8, 2, 8, o=None) == capi.OCTO_EINVAL and call(8, 2, 8, m=None) == capi.OCTO_EINVAL
        assert call(s_max + 1, 1, s_max + 1) == capi.OCTO_ENOTSUP and b"octo_psis_max_samples" in lib.octo_psis_last_error(h)      # answered before the matrix is read
        assert call(8, 0, 8, o=None, m=None) == capi.OCTO_OK                                               # no rows: nothing to do
    finally:
        lib.octo_psis_destroy(h)


def test_psis_kernels_have_no_scratch(psis_lib):
    import kernel_resources as kr
    rows = kr.resources(build_dir=PSIS_BUILD)
    names = {r["name"].split("(")[0].split("<")[0].replace("void ", "") for r in rows}
    assert any(n.endswith("k_psis") for n in names), names
    bad = [(r["name"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["scratch_instructions"], r["private_segment_fixed_size"]) for r in rows
           if r["vgpr_spill_count"] or r["sgpr_spill_count"] or r["scratch_instructions"] or r["private_segment_fixed_size"]]
    assert not bad, bad
    assert len(rows) <= 6
