"""
ctypes binding of the companion C ABI in include/octofitter_hip_pointwise.h (lib/liboctofitter_hip_pointwise.so) and its host face.

    pw = Pointwise(obs_tables, planets)                            # as given to capi.pack_obs / capi.pack_planets
    pw.n_rows, pw.row_table                                        # R = Σ n_epochs; the table index of each row
    LL = pw.values(elems, nuis=None)                               # [R, W]: NumPy in, NumPy out; torch tensors on the device stay there
    s = pw.summary(elems, nuis=None)                               # dict(n, lppd, mean, var, elpd_is_loo, min, max), each [R]
    pw.close()

The pointwise log-likelihood of `pointwise_like` (src/cross-validation.jl:17-46) at the grain model comparison needs: one row per DATUM,
ll[row][posterior sample], the log-density of that row alone (what a one-row table scores), and its reduction over the samples to the
WAIC / importance-sampling LOO sums. A value is a function of (θ, the table's nuisances, the row) alone — bit-identical whatever batch,
walker index or entry point evaluates it. Like capi.py this is plumbing that FAILS LOUDLY when the library has not been built: there is
no NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import capi, companion

POINTWISE_LIB_PATH = capi.PKG_DIR / "lib" / "liboctofitter_hip_pointwise.so"
MAX_TABLES = 1024      # OCTO_POINTWISE_MAX_TABLES
SUMMARY_FIELDS = ("n", "lppd", "mean", "var", "elpd_is_loo", "min", "max")      # OCTO_POINTWISE_N … OCTO_POINTWISE_MAX
N_STATS = 7            # OCTO_POINTWISE_N_STATS
SERVED_KINDS = (capi.ASTROM_RADEC, capi.ASTROM_SEPPA, capi.RV_ABS, capi.RV_REL)

_SIGS = {
    "octo_pointwise_create": (C.c_int32, [C.c_int32, C.POINTER(capi.OctoConsts), C.POINTER(capi.OctoObsDesc), C.c_int32,
                                          C.POINTER(capi.OctoPlanetDesc), C.c_int32, C.POINTER(C.c_void_p)]),
    "octo_pointwise_destroy": (C.c_int32, [C.c_void_p]),
    "octo_pointwise_last_error": (C.c_char_p, [C.c_void_p]),
    "octo_pointwise_sync": (C.c_int32, [C.c_void_p]),
    "octo_pointwise_n_rows": (C.c_int64, [C.c_void_p]),
    "octo_pointwise_row_table": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32)]),
    "octo_pointwise_eval_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "octo_pointwise_eval": (C.c_int32, [C.c_void_p, capi.c_double_p, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, C.c_int64]),
    "octo_pointwise_summary_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_pointwise_summary": (C.c_int32, [C.c_void_p, capi.c_double_p, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

def load_library(path=None):
    """Load liboctofitter_hip_pointwise.so (after the main library it links against). Raises if it has not been built."""
    return companion.load_library(path, POINTWISE_LIB_PATH, "OCTOFITTER_HIP_POINTWISE_LIB", _SIGS, needs_main=True,
                                  no_fallback="The pointwise log-likelihood on the device has no CPU fallback.")


class Pointwise(companion.Handle):
    """The handle of octo_pointwise_create: the observation tables (dicts of kind, planet and NumPy columns, as capi.pack_obs takes them)
    and the planet list of a system. Kinds served: ASTROM_RADEC, ASTROM_SEPPA, RV_ABS, RV_REL; any other raises OctoError(OCTO_ENOTSUP)."""

    PREFIX = "octo_pointwise"

    def __init__(self, obs_tables, planets, device=0, consts=None):
        self._open(load_library(), device)
        self.n_obs, self.n_planets = len(obs_tables), len(planets)
        obs_arr, keep = capi.pack_obs(obs_tables)
        st = self.lib.octo_pointwise_create(self.device_index, None if consts is None else C.byref(consts), obs_arr, self.n_obs,
                                            capi.pack_planets(planets), self.n_planets, C.byref(self._h))
        del keep
        self._created(st)
        self.n_rows = int(self.lib.octo_pointwise_n_rows(self._h))
        self.row_table = np.zeros(self.n_rows, dtype=np.int32)
        self._check(self.lib.octo_pointwise_row_table(self._h, self.row_table.ctypes.data_as(C.POINTER(C.c_int32))))

    def _host_inputs(self, elems, nuis):
        elems = np.ascontiguousarray(elems, dtype=np.float64)
        if elems.ndim != 2 or elems.shape[0] != self.n_planets * capi.N_EL:
            raise ValueError(f"elems must be [{self.n_planets * capi.N_EL}, W]")
        W = elems.shape[1]
        if nuis is not None:
            nuis = np.ascontiguousarray(nuis, dtype=np.float64)
            if nuis.shape != (self.n_obs * capi.N_NUIS, W):
                raise ValueError(f"nuis must be [{self.n_obs * capi.N_NUIS}, W]")
        return elems, nuis, W

    def _device_inputs(self, elems, nuis):
        import torch
        if elems.dtype != torch.float64 or elems.dim() != 2 or elems.shape[0] != self.n_planets * capi.N_EL or elems.stride(1) != 1:
            raise ValueError(f"elems must be a float64 tensor [{self.n_planets * capi.N_EL}, W] with the walker index fastest")
        if elems.device.index != self.device_index:
            raise ValueError(f"elems is on {elems.device}, the handle on device {self.device_index}")
        W, ld = int(elems.shape[1]), max(int(elems.stride(0)), 1)
        if nuis is not None:
            if nuis.dtype != torch.float64 or tuple(nuis.shape) != (self.n_obs * capi.N_NUIS, W) or nuis.device != elems.device:
                raise ValueError(f"nuis must be a float64 tensor [{self.n_obs * capi.N_NUIS}, W] on the elements' device")
            if nuis.stride(1) != 1 or (W > 1 and nuis.stride(0) != ld):
                nuis = torch.empty_strided(tuple(nuis.shape), (ld, 1), dtype=torch.float64, device=elems.device).copy_(nuis)      # the rows share the elements' leading dimension
        return W, ld, nuis

    def values(self, elems, nuis=None, stream=None):
        """The matrix [R, W]. NumPy inputs: the blocking host-buffer call, NumPy out. A torch tensor on the handle's device: the device
        call, asynchronous on `stream` (default: torch's current stream), a torch tensor out."""
        if companion.is_torch(elems) and elems.is_cuda:
            import torch
            W, ld, nu = self._device_inputs(elems, nuis)
            out = torch.empty((self.n_rows, W), dtype=torch.float64, device=elems.device)
            self._keep = (elems, nu)
            self._check(self.lib.octo_pointwise_eval_device(self._h, elems.data_ptr(), ld, W, None if nu is None else nu.data_ptr(),
                                                            out.data_ptr(), max(W, 1), self._stream(stream, elems.device)))
            return out
        elems, nuis, W = self._host_inputs(elems, nuis)
        out = np.empty((self.n_rows, W))
        self._check(self.lib.octo_pointwise_eval(self._h, capi._dptr(elems), W, W, capi._dptr(nuis), capi._dptr(out), W))
        return out

    def summary(self, elems, nuis=None, stream=None):
        """The reduction over the walkers with a finite value, the matrix never stored: dict(n, lppd, mean, var, elpd_is_loo, min, max),
        each [R] (NumPy for NumPy inputs, torch tensors for device inputs). var is the sample variance (n − 1): NaN for n = 1."""
        if companion.is_torch(elems) and elems.is_cuda:
            import torch
            W, ld, nu = self._device_inputs(elems, nuis)
            out = torch.empty((N_STATS, self.n_rows), dtype=torch.float64, device=elems.device)
            self._keep = (elems, nu)
            self._check(self.lib.octo_pointwise_summary_device(self._h, elems.data_ptr(), ld, W, None if nu is None else nu.data_ptr(),
                                                               out.data_ptr(), self._stream(stream, elems.device)))
            return dict(zip(SUMMARY_FIELDS, out))
        elems, nuis, W = self._host_inputs(elems, nuis)
        out = np.empty((N_STATS, self.n_rows))
        self._check(self.lib.octo_pointwise_summary(self._h, capi._dptr(elems), W, W, capi._dptr(nuis), capi._dptr(out)))
        return dict(zip(SUMMARY_FIELDS, out))
