"""
Build checks of the companion library liboctofitter_hip_pointwise.so (include/octofitter_hip_pointwise.h, csrc/pointwise/): what it exports against
what its header declares and host/pointwise.py binds, that the main library's sources did not move, the argument checks that need no device,
and the compiled kernels' resources read from the code objects (tools/kernel_resources.py). The bodies every companion library shares are
in tests/companion_checks.py; linkage and the main library's symbol set are checked for all four in tests/test_companion_libraries.py.
CPU suite: hipcc cross-compiles.
"""
import ctypes as C
import re

import numpy as np
import pytest

import companion_checks as cc

FUNCTIONS = {"octo_pointwise_create", "octo_pointwise_destroy", "octo_pointwise_eval", "octo_pointwise_eval_device", "octo_pointwise_last_error",
             "octo_pointwise_n_rows", "octo_pointwise_row_table", "octo_pointwise_summary", "octo_pointwise_summary_device", "octo_pointwise_sync"}


@pytest.fixture(scope="module")
def pointwise_lib():
    from __graft_entry__ import build_hip, build_pointwise
    build_hip()           # no-ops when csrc/build/ and csrc/pointwise/build/ are up to date
    return build_pointwise()


def test_header_library_and_binding_agree(pkg, pointwise_lib):
    pw = pkg.pointwise
    text = cc.check_header_library_and_binding_agree("pointwise", pw, pointwise_lib, FUNCTIONS, exact=True)
    # the constants of the binding are those of the header
    for k, name in enumerate(pw.SUMMARY_FIELDS):
        assert re.search(rf"#define OCTO_POINTWISE_{name.upper()}\s+{k}\b", text), name
    assert re.search(rf"#define OCTO_POINTWISE_N_STATS\s+{pw.N_STATS}\b", text) and pw.N_STATS == len(pw.SUMMARY_FIELDS)
    assert re.search(rf"#define OCTO_POINTWISE_MAX_TABLES\s+{pw.MAX_TABLES}\b", text)
    # … and the package exports the class and the two callers
    assert pkg.Pointwise is pw.Pointwise and callable(pkg.pointwise_like_rows) and callable(pkg.waic)


def _table(capi, kind, planet=0, n=3, **over):
    t = np.array([58000.0, 58010.0, 58030.0])[:n]
    astrom = kind in (capi.ASTROM_RADEC, capi.ASTROM_SEPPA, capi.ONEIL_RADEC, capi.ONEIL_SEPPA)
    tab = dict(kind=kind, planet=planet, epoch=t, y1=np.full(n, 10.0), y2=np.full(n, 20.0) if astrom else None,
               s1=np.full(n, 1.0), s2=np.full(n, 2.0) if astrom else None, cor=None, extra=None)
    if kind == capi.HGCA:
        tab.update(planet=-1, y1=np.zeros(n), y2=np.zeros(n), s1=None, s2=None, extra=np.tile([1.0, 1.0, 0.1, 0.1, 0.0], 3))
    tab.update(over)
    return tab


def test_main_library_sources_untouched():
    """The pointwise library came with no change to a file directly under csrc/."""
    cc.check_main_library_sources_untouched("include/octofitter_hip_pointwise.h")


def test_argument_checks_that_need_no_device(pkg, pointwise_lib):
    capi, pw = pkg.capi, pkg.pointwise
    lib = pw.load_library()
    visual = [dict(orbit_kind=capi.ORBIT_VISUAL_KEP, has_mass=1)]
    radvel = [dict(orbit_kind=capi.ORBIT_RADVEL, has_mass=1)]
    ti = [dict(orbit_kind=capi.ORBIT_THIELE_INNES, has_mass=1)]

    def create(tabs, planets, n_planets=None, out=True, n_obs=None):
        h = C.c_void_p()
        obs_arr, keep = capi.pack_obs(tabs)
        st = lib.octo_pointwise_create(0, None, obs_arr, len(tabs) if n_obs is None else n_obs, capi.pack_planets(planets),
                                       len(planets) if n_planets is None else n_planets, C.byref(h) if out else None)
        del keep
        assert not h.value or st == capi.OCTO_OK
        if h.value:
            lib.octo_pointwise_destroy(h)
        return st, (lib.octo_pointwise_last_error(None) or b"").decode()

    # the kinds whose value is no sum over rows: OCTO_ENOTSUP, the message names the table and the kind
    good = _table(capi, capi.ASTROM_RADEC)
    for kind, name in ((capi.RV_ABS_MARG, "OCTO_RV_ABS_MARG"), (capi.HGCA, "OCTO_HGCA"), (capi.ONEIL_RADEC, "OCTO_ONEIL_RADEC"),
                       (capi.ONEIL_SEPPA, "OCTO_ONEIL_SEPPA")):
        st, msg = create([good, _table(capi, kind)], visual)
        assert st == capi.OCTO_ENOTSUP and "table 1" in msg and name in msg, (kind, st, msg)
    # an RV table next to a Thiele-Innes planet
    st, msg = create([_table(capi, capi.RV_ABS, planet=-1)], ti)
    assert st == capi.OCTO_ENOTSUP and "table 0" in msg and "ThieleInnes" in msg, (st, msg)
    st, msg = create([_table(capi, capi.RV_REL)], ti)
    assert st == capi.OCTO_ENOTSUP and "ThieleInnes" in msg
    # the input rules of octo_dataset_create
    assert create([good], visual, out=False)[0] == capi.OCTO_EINVAL                                        # NULL out pointer
    st, msg = create([good], visual, n_planets=0)
    assert st == capi.OCTO_EINVAL and "n_planets" in msg
    assert create([good], visual * (capi.MAX_PLANETS + 1))[0] == capi.OCTO_EINVAL
    assert create([good], visual, n_obs=-1)[0] == capi.OCTO_EINVAL
    assert create([good], visual, n_obs=pw.MAX_TABLES + 1)[0] == capi.OCTO_EINVAL
    assert create([good], [dict(orbit_kind=7, has_mass=0)])[0] == capi.OCTO_EINVAL                         # unknown orbit kind
    assert create([_table(capi, 8)], visual)[0] == capi.OCTO_EINVAL                                        # unknown observation kind
    st, msg = create([_table(capi, capi.ASTROM_RADEC, s1=np.array([1.0, 0.0, 1.0]))], visual)
    assert st == capi.OCTO_EINVAL and "table 0 row 1" in msg                                               # σ <= 0
    assert create([_table(capi, capi.ASTROM_SEPPA, s2=np.array([1.0, 1.0, np.inf]))], visual)[0] == capi.OCTO_EINVAL
    assert create([_table(capi, capi.RV_ABS, planet=-1, y1=np.array([1.0, np.nan, 1.0]))], visual)[0] == capi.OCTO_EINVAL
    assert create([_table(capi, capi.RV_REL, epoch=np.array([1.0, 2.0, np.inf]))], visual)[0] == capi.OCTO_EINVAL
    st, msg = create([_table(capi, capi.ASTROM_RADEC, cor=np.array([0.0, 1.0, 0.0]))], visual)
    assert st == capi.OCTO_EINVAL and "correlation" in msg                                                 # |cor| >= 1
    st, msg = create([_table(capi, capi.ASTROM_RADEC, planet=1)], visual)
    assert st == capi.OCTO_EINVAL and "planet index" in msg                                                # planet outside the system
    assert create([_table(capi, capi.RV_REL, planet=-1)], visual)[0] == capi.OCTO_EINVAL
    st, msg = create([_table(capi, capi.ASTROM_SEPPA)], radvel)
    assert st == capi.OCTO_EINVAL and "parallax" in msg                                                    # astrometry on a planet without parallax
    st, msg = create([_table(capi, capi.RV_ABS, planet=-1)], [dict(orbit_kind=capi.ORBIT_VISUAL_KEP, has_mass=0)])
    assert st == capi.OCTO_EINVAL and "mass" in msg
    assert create([_table(capi, capi.RV_ABS, planet=-1, extra=np.array([1.0, 2.0]))], visual)[0] == capi.OCTO_EINVAL      # basis of the wrong length
    assert create([_table(capi, capi.RV_ABS, planet=-1, extra=np.array([1.0, np.nan, 2.0]))], visual)[0] == capi.OCTO_EINVAL
    assert create([_table(capi, capi.ASTROM_RADEC, extra=np.array([1.0, 2.0, 3.0]))], visual)[0] == capi.OCTO_EINVAL
    assert create([_table(capi, capi.ASTROM_RADEC, y2=None)], visual)[0] == capi.OCTO_EINVAL               # missing column
    # valid input gets past every check: what is left is the device (none in the CPU suite)
    st, msg = create([good, _table(capi, capi.RV_ABS, planet=-1, extra=np.array([1.0, 2.0, 3.0]))], visual)
    assert st in (capi.OCTO_OK, capi.OCTO_ENODEV), (st, msg)
    # the Python face raises what the library answers
    with pytest.raises(capi.OctoError) as ex:
        pkg.Pointwise([_table(capi, capi.RV_ABS_MARG, planet=-1)], visual)
    assert ex.value.status == capi.OCTO_ENOTSUP and "OCTO_RV_ABS_MARG" in str(ex.value)
    # calls on a NULL handle
    assert lib.octo_pointwise_eval(None, None, 0, 0, None, None, 0) == capi.OCTO_EINVAL
    assert lib.octo_pointwise_eval_device(None, None, 0, 0, None, None, 0, None) == capi.OCTO_EINVAL
    assert lib.octo_pointwise_summary(None, None, 0, 0, None, None) == capi.OCTO_EINVAL
    assert lib.octo_pointwise_summary_device(None, None, 0, 0, None, None, None) == capi.OCTO_EINVAL
    assert lib.octo_pointwise_sync(None) == capi.OCTO_EINVAL
    assert lib.octo_pointwise_row_table(None, None) == capi.OCTO_EINVAL
    assert lib.octo_pointwise_n_rows(None) == -1
    assert lib.octo_pointwise_destroy(None) == capi.OCTO_OK


def test_pointwise_kernels_have_no_scratch(pointwise_lib):
    rows, names = cc.check_kernels_have_no_scratch("pointwise", sgpr_too=True)
    assert {"k_pointwise", "k_pointwise_n", "k_pointwise_merge"} <= names, names
    # the single-planet matrix kernel is held to the registers of four waves per SIMD (128 of the 512 per lane)
    one = [r for r in rows if "k_pointwise<1, false>" in r["name"]]
    assert len(one) == 1 and one[0]["vgpr_count"] + one[0]["agpr_count"] <= 128, [(r["name"], r["vgpr_count"], r["agpr_count"]) for r in one]
    assert len(rows) <= 16      # the instantiation count stays small (every kernel of the library, the included k_setup among them)
