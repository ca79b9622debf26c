"""
ctypes binding of the companion C ABI in include/octofitter_hip_predict.h (lib/liboctofitter_hip_predict.so) and its host face.

    pr = Predictor(planets, epochs, channels, basis=None)          # planets: [dict(orbit_kind, has_mass)], channels: [(quantity, planet)]
    cube = pr.values(elems, add0=None, add1=None)                  # [C, T, W]: NumPy in, NumPy out; torch tensors on the device stay there
    band = pr.summary(elems)                                       # dict(n_valid, mean, sd, min, max), each [C, T]
    pr.close()

The model values of `simulate!` for a batch of parameter sets: sky offsets, separations, position angles and radial velocities of each
companion at each epoch, with the reflex terms of the tables' models. A value is a function of (θ, epoch, channel) alone — bit-identical
whatever batch, walker index or grid order evaluates it. Like capi.py this is plumbing that FAILS LOUDLY when the library has not been
built: there is no NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import capi, companion

PREDICT_LIB_PATH = capi.PKG_DIR / "lib" / "liboctofitter_hip_predict.so"
MAX_CHANNELS = 32      # OCTO_PREDICT_MAX_CHANNELS
RAOFF, DECOFF, SEP, PA, RADVEL, ASTROM_RA, ASTROM_DEC, ASTROM_SEP, ASTROM_PA, RV_STAR, RV_REL = range(11)
N_QUANTITIES = 11
QUANTITY_NAMES = ("RAOFF", "DECOFF", "SEP", "PA", "RADVEL", "ASTROM_RA", "ASTROM_DEC", "ASTROM_SEP", "ASTROM_PA", "RV_STAR", "RV_REL")
RV_QUANTITIES = (RADVEL, RV_STAR, RV_REL)
SUMMARY_FIELDS = ("n_valid", "mean", "sd", "min", "max")


class OctoPredictChannel(C.Structure):
    _fields_ = [("quantity", C.c_int32), ("planet", C.c_int32)]


_SIGS = {
    "octo_predict_create": (C.c_int32, [C.c_int32, C.POINTER(capi.OctoConsts), C.POINTER(capi.OctoPlanetDesc), C.c_int32, capi.c_double_p, C.c_int64,
                                        capi.c_double_p, C.POINTER(OctoPredictChannel), C.c_int32, C.POINTER(C.c_void_p)]),
    "octo_predict_destroy": (C.c_int32, [C.c_void_p]),
    "octo_predict_last_error": (C.c_char_p, [C.c_void_p]),
    "octo_predict_sync": (C.c_int32, [C.c_void_p]),
    "octo_predict_eval_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "octo_predict_eval": (C.c_int32, [C.c_void_p, capi.c_double_p, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, capi.c_double_p, C.c_int64]),
    "octo_predict_summary_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_predict_summary": (C.c_int32, [C.c_void_p, capi.c_double_p, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, capi.c_double_p]),
    "octo_predict_set_variant": (C.c_int32, [C.c_void_p, C.c_int32]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

def load_library(path=None):
    """Load liboctofitter_hip_predict.so (after the main library it links against). Raises if it has not been built."""
    return companion.load_library(path, PREDICT_LIB_PATH, "OCTOFITTER_HIP_PREDICT_LIB", _SIGS, needs_main=True,
                                  no_fallback="Model values on the device have no CPU fallback.")


def pack_channels(channels):
    """[(quantity, planet)] (quantity: an int or a name of QUANTITY_NAMES) -> ctypes array."""
    arr = (OctoPredictChannel * max(len(channels), 1))()
    for k, (q, p) in enumerate(channels):
        arr[k].quantity = QUANTITY_NAMES.index(q) if isinstance(q, str) else int(q)
        arr[k].planet = int(p)
    return arr


class Predictor(companion.Handle):
    """The handle of octo_predict_create: a planet list, an epoch grid [T] (MJD, any order), up to 32 channels (quantity, planet) and an
    optional basis column [T] that an RV channel's add1 multiplies."""

    PREFIX = "octo_predict"

    def __init__(self, planets, epochs, channels, basis=None, device=0, consts=None):
        self.epochs = np.ascontiguousarray(epochs, dtype=np.float64).reshape(-1)
        self.basis = None if basis is None else np.ascontiguousarray(basis, dtype=np.float64).reshape(-1)
        if self.basis is not None and self.basis.shape != self.epochs.shape:
            raise ValueError("Predictor: the basis column has one value per epoch")
        self.channels = [(QUANTITY_NAMES.index(q) if isinstance(q, str) else int(q), int(p)) for q, p in channels]
        self.n_planets, self.T, self.C = len(planets), int(self.epochs.size), len(self.channels)
        self._open(load_library(), device)
        st = self.lib.octo_predict_create(self.device_index, None if consts is None else C.byref(consts), capi.pack_planets(planets), self.n_planets,
                                          capi._dptr(self.epochs), self.T, capi._dptr(self.basis), pack_channels(self.channels), self.C, C.byref(self._h))
        self._created(st)

    def _host_inputs(self, elems, add0, add1):
        elems = np.ascontiguousarray(elems, dtype=np.float64)
        if elems.ndim != 2 or elems.shape[0] != self.n_planets * capi.N_EL:
            raise ValueError(f"elems must be [{self.n_planets * capi.N_EL}, W]")
        W = elems.shape[1]
        adds = []
        for a in (add0, add1):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (self.C, W):
                    raise ValueError(f"add rows must be [{self.C}, W]")
            adds.append(a)
        return elems, adds[0], adds[1], W

    def _device_inputs(self, elems, add0, add1):
        import torch
        if elems.dtype != torch.float64 or elems.dim() != 2 or elems.shape[0] != self.n_planets * capi.N_EL or elems.stride(1) != 1:
            raise ValueError(f"elems must be a float64 tensor [{self.n_planets * capi.N_EL}, W] with the walker index fastest")
        W, ld = int(elems.shape[1]), int(elems.stride(0)) if elems.shape[1] > 1 else max(int(elems.stride(0)), 1)
        ptrs = []
        for a in (add0, add1):
            if a is None:
                ptrs.append(None)
                continue
            if a.dtype != torch.float64 or tuple(a.shape) != (self.C, W) or a.device != elems.device:
                raise ValueError(f"add rows must be float64 tensors [{self.C}, W] on the elements' device")
            if a.stride(1) != 1 or (W > 1 and a.stride(0) != ld):
                a = torch.empty_strided((self.C, W), (ld, 1), dtype=torch.float64, device=elems.device).copy_(a)      # the rows share the elements' leading dimension
            ptrs.append(a)
        return W, ld, ptrs[0], ptrs[1]

    def values(self, elems, add0=None, add1=None, stream=None):
        """The cube [C, T, W]. NumPy inputs: the blocking host-buffer call, NumPy out. A torch tensor on the handle's device: the device
        call, asynchronous on `stream` (default: torch's current stream), a torch tensor out."""
        if companion.is_torch(elems) and elems.is_cuda:
            import torch
            W, ld, a0, a1 = self._device_inputs(elems, add0, add1)
            ldo = W + (W & 1)      # an even leading dimension: 16-byte stores
            buf = torch.empty((self.C * self.T, ldo), dtype=torch.float64, device=elems.device)
            self._keep = (elems, a0, a1)
            self._check(self.lib.octo_predict_eval_device(self._h, elems.data_ptr(), ld, W, None if a0 is None else a0.data_ptr(),
                                                          None if a1 is None else a1.data_ptr(), buf.data_ptr(), ldo, self._stream(stream, elems.device)))
            return buf[:, :W].reshape(self.C, self.T, W)
        elems, add0, add1, W = self._host_inputs(elems, add0, add1)
        out = np.empty((self.C, self.T, W))
        self._check(self.lib.octo_predict_eval(self._h, capi._dptr(elems), W, W, capi._dptr(add0), capi._dptr(add1), capi._dptr(out), W))
        return out

    def summary(self, elems, add0=None, add1=None, stream=None):
        """Statistics over the valid walkers for every (channel, epoch), the cube never stored: dict(n_valid, mean, sd, min, max), each [C, T]
        (NumPy for NumPy inputs, torch tensors for device inputs). sd is the sample standard deviation (n − 1): NaN for one valid walker."""
        if companion.is_torch(elems) and elems.is_cuda:
            import torch
            W, ld, a0, a1 = self._device_inputs(elems, add0, add1)
            out = torch.empty((len(SUMMARY_FIELDS), self.C, self.T), dtype=torch.float64, device=elems.device)
            self._keep = (elems, a0, a1)
            self._check(self.lib.octo_predict_summary_device(self._h, elems.data_ptr(), ld, W, None if a0 is None else a0.data_ptr(),
                                                             None if a1 is None else a1.data_ptr(), out.data_ptr(), self._stream(stream, elems.device)))
            return dict(zip(SUMMARY_FIELDS, out))
        elems, add0, add1, W = self._host_inputs(elems, add0, add1)
        out = np.empty((len(SUMMARY_FIELDS), self.C, self.T))
        self._check(self.lib.octo_predict_summary(self._h, capi._dptr(elems), W, W, capi._dptr(add0), capi._dptr(add1), capi._dptr(out)))
        return dict(zip(SUMMARY_FIELDS, out))

    def set_variant(self, variant):
        """Measurement hook: the cube kernel's store width (0 / 2: two walkers per lane and 16-byte stores where the output allows, 1: 8-byte)."""
        self._check(self.lib.octo_predict_set_variant(self._h, int(variant)))
