"""
Build checks over all four companion libraries (liboctofitter_hip_{draws,predict,pointwise,psis}.so): that the main library exports none of
their symbols and how each is linked; then the shared scaffold itself (the build table, the symbol check of build(), the loader,
csrc/companion/). Each library's header / binding agreement, argument checks and kernel resources are in its tests/test_*_resources.py,
over the bodies of tests/companion_checks.py. CPU suite: hipcc cross-compiles.
"""
import importlib
import subprocess

import pytest

import companion_checks as cc

NAMES = ("draws", "predict", "pointwise", "psis")

LAST_SENTENCE = {
    "draws": "Prior draws on the device have no CPU fallback.",
    "predict": "Model values on the device have no CPU fallback.",
    "pointwise": "The pointwise log-likelihood on the device has no CPU fallback.",
    "psis": "PSIS-LOO on the device has no CPU fallback.",
}


def header(name):
    return cc.ROOT / "include" / f"octofitter_hip_{name}.h"


def host_module(pkg, name):
    return importlib.import_module(f"{pkg.__name__}.host.{name}")


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as g
    g.build_hip()           # no-ops when csrc/build/ and csrc/<name>/build/ are up to date
    return {name: g.build_companion(name) for name in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_main_library_exports_no_companion_symbol(libs, name):
    syms = cc.dynamic_symbols(cc.MAIN_LIB)
    assert any(s.startswith("octo_") for s in syms)
    assert not [s for s in syms if s.startswith(f"octo_{name}")]


@pytest.mark.parametrize("name", ("draws", "predict", "pointwise"))
def test_companion_links_the_main_library_by_origin(libs, name):
    dyn = subprocess.run(["readelf", "-d", str(libs[name])], capture_output=True, text=True, check=True).stdout
    assert "liboctofitter_hip.so" in dyn and "$ORIGIN" in dyn


def test_companion_links_nothing_of_the_main_library(libs):
    dyn = subprocess.run(["readelf", "-d", str(libs["psis"])], capture_output=True, text=True, check=True).stdout
    assert "liboctofitter_hip" not in dyn


def test_main_library_sources_untouched_by_draws():
    """The other three libraries carry this check in their own files; the draws library came with no edit directly under csrc/ either."""
    cc.check_main_library_sources_untouched("include/octofitter_hip_draws.h")


# ---- the scaffold itself -------------------------------------------------------------------------------------------------------------------
def test_build_table_covers_every_companion(pkg, libs):
    import __graft_entry__ as g
    assert tuple(g.COMPANIONS) == NAMES
    wrappers = {"draws": (g.build_draws, g.DRAWS_LIB), "predict": (g.build_predict, g.PREDICT_LIB), "pointwise": (g.build_pointwise, g.POINTWISE_LIB),
                "psis": (g.build_psis, g.PSIS_LIB)}
    for name in NAMES:
        build, lib = wrappers[name]
        mod = host_module(pkg, name)
        assert lib == libs[name] == g.companion_lib(name) == getattr(mod, f"{name.upper()}_LIB_PATH")
        assert build() == lib                                           # up to date: a no-op
        assert header(name).name == g.COMPANIONS[name]["header"] and header(name).exists()
        assert g.COMPANIONS[name]["links_main"] == g.COMPANIONS[name]["main_headers"] == (name != "psis")
    with pytest.raises(KeyError):
        g.build_companion("nonesuch")


def test_build_checks_the_symbols_of_every_library(pkg, libs, monkeypatch):
    import __graft_entry__ as g
    g.check_exported_symbols()
    for name in NAMES:      # draws among them: a name its library does not export stops build()
        mod = host_module(pkg, name)
        with monkeypatch.context() as m:
            m.setattr(mod, "EXPORTED_SYMBOLS", mod.EXPORTED_SYMBOLS + (f"octo_{name}_no_such_function",))
            with pytest.raises(AttributeError, match=f"octo_{name}_no_such_function"):
                g.check_exported_symbols()


@pytest.mark.parametrize("name", NAMES)
def test_load_library_of_a_missing_file_says_what_to_do(pkg, libs, name, tmp_path):
    mod = host_module(pkg, name)
    missing = tmp_path / f"liboctofitter_hip_{name}.so"
    with pytest.raises(FileNotFoundError) as ex:
        mod.load_library(path=missing)
    msg = str(ex.value)
    assert str(missing) in msg and "g.build()" in msg and msg.endswith(LAST_SENTENCE[name]), msg
    assert all(LAST_SENTENCE[other] not in msg for other in NAMES if other != name)
    # a path given by hand is never cached: the default library still loads, and is the cached one
    assert mod.load_library() is mod.load_library()


def test_shared_headers_live_under_csrc_companion():
    shared = sorted(p.name for p in (cc.CSRC / "companion").glob("*.h"))
    assert shared == ["octo_companion_device.h", "octo_companion_host.h"]
    host = (cc.CSRC / "companion" / "octo_companion_host.h").read_text()
    assert "octo_kernels.h" not in [line.split('"')[1] for line in host.splitlines() if line.startswith('#include "')]      # PSIS includes it
    # … and they came with no change to a file directly under csrc/
    cc.check_main_library_sources_untouched("octofitter.jl_amd/csrc/companion/octo_companion_host.h")
