"""
Build checks of the companion library liboctofitter_hip_predict.so (include/octofitter_hip_predict.h, csrc/predict/): what it exports against
what its header declares and host/predict.py binds, that the main library's symbol set and sources did not move, the argument checks that
need no device, and the compiled kernels' resources read from the code objects (tools/kernel_resources.py). CPU suite: hipcc cross-compiles.
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
HEADER = ROOT / "include" / "octofitter_hip_predict.h"
MAIN_LIB = ROOT / "octofitter.jl_amd" / "lib" / "liboctofitter_hip.so"
PREDICT_BUILD = ROOT / "octofitter.jl_amd" / "csrc" / "predict" / "build"


@pytest.fixture(scope="module")
def predict_lib():
    from __graft_entry__ import build_hip, build_predict
    build_hip()           # no-ops when csrc/build/ and csrc/predict/build/ are up to date
    return build_predict()


def declared_functions():
    """{name: number of parameters} of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(octo_predict_\w+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def dynamic_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_library_and_binding_agree(pkg, predict_lib):
    predict = pkg.predict
    decl = declared_functions()
    assert {"octo_predict_create", "octo_predict_destroy", "octo_predict_last_error", "octo_predict_sync", "octo_predict_eval_device",
            "octo_predict_eval", "octo_predict_summary_device", "octo_predict_summary"} <= set(decl)
    exported = {s for s in dynamic_symbols(predict_lib) if s.startswith("octo_")}
    assert exported == set(decl), (sorted(exported), sorted(decl))
    assert set(predict.EXPORTED_SYMBOLS) == set(decl)
    lib = predict.load_library()
    for name, n_params in decl.items():
        assert len(predict._SIGS[name][1]) == n_params, name
        assert getattr(lib, name).argtypes is not None
    # the constants of the binding are those of the header
    text = HEADER.read_text()
    for q, name in enumerate(predict.QUANTITY_NAMES):
        assert re.search(rf"#define OCTO_PREDICT_{name}\s+{q}\b", text), name
    assert re.search(rf"#define OCTO_PREDICT_MAX_CHANNELS\s+{predict.MAX_CHANNELS}\b", text)
    assert re.search(rf"#define OCTO_PREDICT_N_QUANTITIES\s+{predict.N_QUANTITIES}\b", text)


def test_main_library_exports_no_predict_symbol(predict_lib):
    syms = dynamic_symbols(MAIN_LIB)
    assert any(s.startswith("octo_") for s in syms)
    assert not [s for s in syms if s.startswith("octo_predict")]


def test_companion_links_the_main_library_by_origin(predict_lib):
    dyn = subprocess.run(["readelf", "-d", str(predict_lib)], capture_output=True, text=True, check=True).stdout
    assert "liboctofitter_hip.so" in dyn and "$ORIGIN" in dyn


def _git(*args):
    return subprocess.run(["git", "-C", str(ROOT), *args], capture_output=True, text=True)


def test_main_library_sources_untouched():
    """The model-value library came with no change to a file directly under csrc/ (kernel_source_hash() covers exactly those, and the committed
    counter evidence is keyed to it): neither the commit that added include/octofitter_hip_predict.h nor, while that header is still
    uncommitted, the working tree differs from its parent there."""
    if _git("rev-parse", "--is-inside-work-tree").stdout.strip() != "true":
        pytest.skip("not a git checkout")
    files = [":(glob)octofitter.jl_amd/csrc/*.h", ":(glob)octofitter.jl_amd/csrc/*.hip"]      # directly under csrc/: `*` stops at a slash
    added = _git("log", "--diff-filter=A", "--format=%H", "--", "include/octofitter_hip_predict.h").stdout.split()
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


def test_argument_checks_that_need_no_device(pkg, predict_lib):
    capi, predict = pkg.capi, pkg.predict
    lib = predict.load_library()
    epochs = np.array([58000.0, 58010.0])
    visual = capi.pack_planets([dict(orbit_kind=capi.ORBIT_VISUAL_KEP, has_mass=0)])
    radvel = capi.pack_planets([dict(orbit_kind=capi.ORBIT_RADVEL, has_mass=0)])
    ti = capi.pack_planets([dict(orbit_kind=capi.ORBIT_THIELE_INNES, has_mass=0)])

    def create(planets, n_planets, channels, out=True, ep=epochs):
        h = C.c_void_p()
        st = lib.octo_predict_create(0, None, planets, n_planets, capi._dptr(ep), len(ep), None, predict.pack_channels(channels), len(channels),
                                     C.byref(h) if out else None)
        assert not h.value
        return st, (lib.octo_predict_last_error(None) or b"").decode()

    assert create(visual, 1, [(predict.RAOFF, 0)], out=False)[0] == capi.OCTO_EINVAL                      # NULL out pointer
    st, msg = create(visual, 0, [(predict.RAOFF, 0)])
    assert st == capi.OCTO_EINVAL and "n_planets" in msg                                                  # 0 planets
    st, msg = create(visual, 1, [(predict.N_QUANTITIES, 0)])
    assert st == capi.OCTO_EINVAL and "unknown quantity" in msg
    assert create(visual, 1, [(-1, 0)])[0] == capi.OCTO_EINVAL
    st, msg = create(radvel, 1, [(predict.RAOFF, 0)])
    assert st == capi.OCTO_EINVAL and "parallax" in msg                                                   # astrometric channel on a RadVel planet
    assert create(radvel, 1, [(predict.ASTROM_SEP, 0)])[0] == capi.OCTO_EINVAL
    st, msg = create(ti, 1, [(predict.RADVEL, 0)])
    assert st == capi.OCTO_EINVAL and "ThieleInnes" in msg                                                # RV quantity on a Thiele-Innes planet
    assert create(ti, 1, [(predict.RV_STAR, -1)])[0] == capi.OCTO_EINVAL
    assert create(visual, 1, [(predict.RAOFF, 1)])[0] == capi.OCTO_EINVAL                                 # planet outside the system
    assert create(visual, 1, [(predict.RV_STAR, 0)])[0] == capi.OCTO_EINVAL                               # RV_STAR takes planet = -1
    assert create(visual, 1, [(predict.RAOFF, 0)] * (predict.MAX_CHANNELS + 1))[0] == capi.OCTO_EINVAL
    assert create(visual, 1, [(predict.RAOFF, 0)], ep=np.array([58000.0, np.nan]))[0] == capi.OCTO_EINVAL
    # calls on a NULL handle
    assert lib.octo_predict_eval(None, None, 0, 0, None, None, None, 0) == capi.OCTO_EINVAL
    assert lib.octo_predict_summary(None, None, 0, 0, None, None, None) == capi.OCTO_EINVAL
    assert lib.octo_predict_destroy(None) == capi.OCTO_OK


def test_predict_kernels_have_no_scratch(predict_lib):
    import kernel_resources as kr
    rows = kr.resources(build_dir=PREDICT_BUILD)
    names = {r["name"].split("(")[0].split("<")[0].replace("void ", "") for r in rows}
    assert {"k_predict_cube", "k_predict_cube_n", "k_predict_part", "k_predict_part_n", "k_predict_merge"} <= names, names
    bad = [(r["name"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["scratch_instructions"], r["private_segment_fixed_size"]) for r in rows
           if r["vgpr_spill_count"] or r["scratch_instructions"] or r["private_segment_fixed_size"]]
    assert not bad, bad
    # the single-planet cube kernels are held to the registers of four waves per SIMD (128 of the 512 per lane)
    one = [r for r in rows if "k_predict_cube<1," in r["name"]]
    assert len(one) >= 1 and all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in one), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in one]
    assert len([r for r in rows if "k_predict" in r["name"]]) <= 16      # the instantiation count stays small
