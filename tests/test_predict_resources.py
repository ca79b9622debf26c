"""
Build checks of the companion library liboctofitter_hip_predict.so (include/octofitter_hip_predict.h, csrc/predict/): what it exports against
what its header declares and host/predict.py binds, that the main library's sources did not move, the argument checks that need no device,
and the compiled kernels' resources read from the code objects (tools/kernel_resources.py). The bodies every companion library shares are
in tests/companion_checks.py; linkage and the main library's symbol set are checked for all four in tests/test_companion_libraries.py.
CPU suite: hipcc cross-compiles.
"""
import ctypes as C
import re

import numpy as np
import pytest

import companion_checks as cc

FUNCTIONS = {"octo_predict_create", "octo_predict_destroy", "octo_predict_eval", "octo_predict_eval_device", "octo_predict_last_error",
             "octo_predict_summary", "octo_predict_summary_device", "octo_predict_sync"}


@pytest.fixture(scope="module")
def predict_lib():
    from __graft_entry__ import build_hip, build_predict
    build_hip()           # no-ops when csrc/build/ and csrc/predict/build/ are up to date
    return build_predict()


def test_header_library_and_binding_agree(pkg, predict_lib):
    predict = pkg.predict
    text = cc.check_header_library_and_binding_agree("predict", predict, predict_lib, FUNCTIONS, exact=False)
    # the constants of the binding are those of the header
    for q, name in enumerate(predict.QUANTITY_NAMES):
        assert re.search(rf"#define OCTO_PREDICT_{name}\s+{q}\b", text), name
    assert re.search(rf"#define OCTO_PREDICT_MAX_CHANNELS\s+{predict.MAX_CHANNELS}\b", text)
    assert re.search(rf"#define OCTO_PREDICT_N_QUANTITIES\s+{predict.N_QUANTITIES}\b", text)


def test_main_library_sources_untouched():
    """The model-value library came with no change to a file directly under csrc/."""
    cc.check_main_library_sources_untouched("include/octofitter_hip_predict.h")


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
    rows, names = cc.check_kernels_have_no_scratch("predict", sgpr_too=False)
    assert {"k_predict_cube", "k_predict_cube_n", "k_predict_part", "k_predict_part_n", "k_predict_merge"} <= names, names
    # the single-planet cube kernels are held to the registers of four waves per SIMD (128 of the 512 per lane)
    one = [r for r in rows if "k_predict_cube<1," in r["name"]]
    assert len(one) >= 1 and all(r["vgpr_count"] + r["agpr_count"] <= 128 for r in one), [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in one]
    assert len([r for r in rows if "k_predict" in r["name"]]) <= 16      # the instantiation count stays small
