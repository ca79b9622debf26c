"""
Build checks of the companion library liboctofitter_hip_psis.so (include/octofitter_hip_psis.h, csrc/psis/): what it exports against
what its header declares and host/psis.py binds, that the main library's sources did not move, the argument checks that need no device,
and the compiled kernels' resources read from the code objects (tools/kernel_resources.py). The bodies every companion library shares are
in tests/companion_checks.py; linkage and the main library's symbol set are checked for all four in tests/test_companion_libraries.py.
CPU suite: hipcc cross-compiles.
"""
import ctypes as C
import re

import numpy as np
import pytest

import companion_checks as cc

FUNCTIONS = {"octo_psis_create", "octo_psis_destroy", "octo_psis_last_error", "octo_psis_loo", "octo_psis_loo_device", "octo_psis_max_samples",
             "octo_psis_sync", "octo_psis_tail_len"}


@pytest.fixture(scope="module")
def psis_lib():
    from __graft_entry__ import build_hip, build_psis
    build_hip()           # no-ops when csrc/build/ and csrc/psis/build/ are up to date
    return build_psis()


def test_header_library_and_binding_agree(pkg, psis_lib):
    ps = pkg.psis
    text = cc.check_header_library_and_binding_agree("psis", ps, psis_lib, FUNCTIONS, exact=True)
    # the constants of the binding are those of the header
    for k, name in enumerate(ps.STAT_FIELDS):
        assert re.search(rf"#define OCTO_PSIS_{name.upper()}\s+{k}\b", text), name
    assert re.search(rf"#define OCTO_PSIS_N_STATS\s+{ps.N_STATS}\b", text) and ps.N_STATS == len(ps.STAT_FIELDS)
    # … and the package exports the class and the caller
    assert pkg.Psis is ps.Psis and callable(pkg.loo)


def test_main_library_sources_untouched():
    """The PSIS library came with no change to a file directly under csrc/."""
    cc.check_main_library_sources_untouched("include/octofitter_hip_psis.h")


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
    rows, names = cc.check_kernels_have_no_scratch("psis", sgpr_too=True)
    assert any(n.endswith("k_psis") for n in names), names
    assert len(rows) <= 6
