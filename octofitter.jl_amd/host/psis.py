"""
ctypes binding of the companion C ABI in include/octofitter_hip_psis.h (lib/liboctofitter_hip_psis.so) and its host face.

    ps = Psis()
    out = ps.loo(LL, weights=False)      # LL [R, S]: row = datum, sample index fastest — the matrix of Pointwise.values()
    out["pareto_k"], out["elpd_loo"], out["lppd"], out["ess"], out["n"], out["tail_len"]      # each [R]; out["log_weights"] [R, S] when asked
    ps.close()

PSIS-LOO (Vehtari, Gelman & Gabry 2017) of a pointwise log-likelihood matrix on the device: per datum the Pareto shape k̂ of the fit to the
largest importance ratios (the diagnostic), the smoothed elpd_loo, the lppd and the effective sample size. The header states the algorithm.
NumPy in gives NumPy out through the blocking host-buffer call; a torch tensor on the device gives the device call on torch's current stream
and torch tensors out. Like capi.py this is plumbing that FAILS LOUDLY when the library has not been built: there is no NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import capi, companion

PSIS_LIB_PATH = capi.PKG_DIR / "lib" / "liboctofitter_hip_psis.so"
STAT_FIELDS = ("n", "tail_len", "pareto_k", "elpd_loo", "lppd", "ess")      # OCTO_PSIS_N … OCTO_PSIS_ESS
N_STATS = 6            # OCTO_PSIS_N_STATS
MAX_TAIL = 4096        # the tail the kernel's sort buffer holds: octo_psis_max_samples() is the largest S with M(S) <= MAX_TAIL

_SIGS = {
    "octo_psis_create": (C.c_int32, [C.c_int32, C.POINTER(C.c_void_p)]),
    "octo_psis_destroy": (C.c_int32, [C.c_void_p]),
    "octo_psis_last_error": (C.c_char_p, [C.c_void_p]),
    "octo_psis_sync": (C.c_int32, [C.c_void_p]),
    "octo_psis_tail_len": (C.c_int64, [C.c_int64]),
    "octo_psis_max_samples": (C.c_int64, []),
    "octo_psis_loo_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "octo_psis_loo": (C.c_int32, [C.c_void_p, capi.c_double_p, C.c_int64, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, C.c_int64]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

def load_library(path=None):
    """Load liboctofitter_hip_psis.so (it links nothing of the main library). Raises if it has not been built."""
    return companion.load_library(path, PSIS_LIB_PATH, "OCTOFITTER_HIP_PSIS_LIB", _SIGS, needs_main=False,
                                  no_fallback="PSIS-LOO on the device has no CPU fallback.")


class Psis(companion.Handle):
    """The handle of octo_psis_create: a stream and the buffers of the host-buffer call."""

    PREFIX = "octo_psis"

    def __init__(self, device=0):
        self._open(load_library(), device)
        self._created(self.lib.octo_psis_create(self.device_index, C.byref(self._h)))

    def loo(self, ll, weights=False, stream=None):
        """dict(n, tail_len, pareto_k, elpd_loo, lppd, ess), each [R], of the matrix ll [R, S]; with weights=True also log_weights [R, S], the
        smoothed normalised log-weights (−Inf where ll is not finite). NumPy input: the blocking host-buffer call, NumPy out. A torch
        tensor on the handle's device (sample index fastest; the row stride is the leading dimension): the device call, asynchronous on
        `stream` (default: torch's current stream), torch tensors out."""
        if companion.is_torch(ll) and ll.is_cuda:
            import torch
            if ll.dtype != torch.float64 or ll.dim() != 2 or (ll.shape[1] > 1 and ll.stride(1) != 1):
                raise ValueError("ll must be a float64 tensor [R, S] with the sample index fastest")
            if ll.device.index != self.device_index:
                raise ValueError(f"ll is on {ll.device}, the handle on device {self.device_index}")
            R, S = int(ll.shape[0]), int(ll.shape[1])
            ld = max(int(ll.stride(0)), S) if R > 1 else S
            out = torch.empty((N_STATS, R), dtype=torch.float64, device=ll.device)
            lw = torch.empty((R, S), dtype=torch.float64, device=ll.device) if weights else None
            self._keep = ll
            self._check(self.lib.octo_psis_loo_device(self._h, ll.data_ptr(), ld, R, S, out.data_ptr(), None if lw is None else lw.data_ptr(),
                                                      max(S, 1), self._stream(stream, ll.device)))
            res = dict(zip(STAT_FIELDS, out))
        else:
            ll = np.ascontiguousarray(ll, dtype=np.float64)
            if ll.ndim != 2:
                raise ValueError("ll must be [R, S]")
            R, S = ll.shape
            out = np.empty((N_STATS, R))
            lw = np.empty((R, S)) if weights else None
            self._check(self.lib.octo_psis_loo(self._h, capi._dptr(ll), S, R, S, capi._dptr(out), capi._dptr(lw), S))
            res = dict(zip(STAT_FIELDS, out))
        if weights:
            res["log_weights"] = lw
        return res
