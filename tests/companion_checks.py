"""
Helpers shared by the build checks of the companion libraries (tests/test_companion_libraries.py, tests/test_*_resources.py). A plain
module, not a conftest.
"""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
MAIN_LIB = ROOT / "octofitter.jl_amd" / "lib" / "liboctofitter_hip.so"
CSRC = ROOT / "octofitter.jl_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tools"))


def declared_functions(header, prefix):
    """{name: number of parameters} of every function `prefix`_* the header declares."""
    text = re.sub(r"/\*.*?\*/", " ", Path(header).read_text(), flags=re.S)
    out = {}
    for m in re.finditer(rf"\b({prefix}_\w+)\s*\(([^()]*)\)\s*;", text):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def dynamic_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def _git(*args):
    return subprocess.run(["git", "-C", str(ROOT), *args], capture_output=True, text=True)


def check_main_library_sources_untouched(added_file):
    """The change that added `added_file` (a path from the repository root) came with no change to a file directly under csrc/
    (kernel_source_hash() covers exactly those, and the committed counter evidence is keyed to it): neither the commit that added the file
    nor, while it is still uncommitted, the working tree differs from its parent there."""
    if _git("rev-parse", "--is-inside-work-tree").stdout.strip() != "true":
        pytest.skip("not a git checkout")
    files = [":(glob)octofitter.jl_amd/csrc/*.h", ":(glob)octofitter.jl_amd/csrc/*.hip"]      # directly under csrc/: `*` stops at a slash
    added = _git("log", "--diff-filter=A", "--format=%H", "--", added_file).stdout.split()
    if not added:      # the file is not committed yet: the working tree against HEAD
        r = _git("diff", "--quiet", "HEAD", "--", *files)
        assert r.returncode == 0, _git("diff", "--stat", "HEAD", "--", *files).stdout
        untracked = _git("ls-files", "--others", "--exclude-standard", "--", *files).stdout.split()
        assert not untracked, untracked
        return
    commit = added[-1]
    if _git("rev-parse", "--verify", "--quiet", commit + "~").returncode != 0:
        pytest.skip("the parent of the commit that added the file is not in this (shallow) checkout")
    r = _git("diff", "--quiet", commit + "~", commit, "--", *files)
    assert r.returncode == 0, _git("diff", "--stat", commit + "~", commit, "--", *files).stdout


def check_header_library_and_binding_agree(name, mod, lib_path, required, exact):
    """include/octofitter_hip_<name>.h, the built library and the host module `mod` name the same functions with the same parameter counts.
    required: functions the header must declare (exact: and no others). Returns the header's text for the library's own constant checks."""
    header = ROOT / "include" / f"octofitter_hip_{name}.h"
    decl = declared_functions(header, f"octo_{name}")
    assert (required == set(decl)) if exact else (required <= set(decl)), sorted(decl)
    exported = {s for s in dynamic_symbols(lib_path) if s.startswith("octo_")}
    assert exported == set(decl), (sorted(exported), sorted(decl))
    assert set(mod.EXPORTED_SYMBOLS) == set(decl)
    lib = mod.load_library()
    for fn, n_params in decl.items():
        assert len(mod._SIGS[fn][1]) == n_params, fn
        assert getattr(lib, fn).argtypes is not None
    return header.read_text()


def check_kernels_have_no_scratch(name, sgpr_too):
    """No kernel under csrc/<name>/build/ spills VGPRs (sgpr_too: or SGPRs), has a scratch instruction or a private segment. Returns
    (rows of tools/kernel_resources.py, the kernels' family names) for the library's own name and count assertions."""
    import kernel_resources as kr
    rows = kr.resources(build_dir=CSRC / name / "build")
    names = {r["name"].split("(")[0].split("<")[0].replace("void ", "") for r in rows}
    bad = [(r["name"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["scratch_instructions"], r["private_segment_fixed_size"]) for r in rows
           if r["vgpr_spill_count"] or (sgpr_too and r["sgpr_spill_count"]) or r["scratch_instructions"] or r["private_segment_fixed_size"]]
    assert not bad, bad
    return rows, names
