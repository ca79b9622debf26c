"""
ctypes binding of the companion C ABI in include/octofitter_hip_draws.h (lib/liboctofitter_hip_draws.so) and its host face.

    draws = PriorDraws(model)                       # model: LogDensityModel
    θ, θ_t, logprior_t = draws.sample(seed, first, n)       # torch tensors on the model's device: [D, n], [D, n], [n]
    θ, logpost, index = draws.best(seed, N, keep=8)         # NumPy: [D, keep], [keep], [keep]
    chain = draws.rejection(seed, N)                        # dict: samples [D, n_accepted], loglike, logpost, index, …

Draw i of a seed is a pure function of (seed, i): Philox4x64-10 with key (seed, "octodraw") and counter (i, d // 4, purpose, 0)
— the same number whatever call, batch or chunk produces it. Like capi.py this is plumbing that FAILS LOUDLY when the library
has not been built: the draws have no NumPy fallback here (host/callers.py keeps the host-side twins of both drivers).
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import capi, companion

DRAWS_LIB_PATH = capi.PKG_DIR / "lib" / "liboctofitter_hip_draws.so"
MAX_KEEP = 64                      # OCTO_DRAWS_MAX_KEEP
PHILOX_KEY1 = 0x6F63746F64726177   # second key word; the first is the seed
PURPOSE_PRIOR, PURPOSE_UNIFORM = 0, 1

c_uint64_p = C.POINTER(C.c_uint64)

_SIGS = {
    "octo_draws_create": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(capi.OctoPrior), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "octo_draws_destroy": (C.c_int32, [C.c_void_p]),
    "octo_draws_detach": (C.c_int32, [C.c_void_p]),
    "octo_draws_last_error": (C.c_char_p, [C.c_void_p]),
    "octo_draws_sample_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_sync": (C.c_int32, [C.c_void_p]),
    "octo_draws_best": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, capi.c_double_p, capi.c_double_p, c_uint64_p]),
    "octo_draws_rejection": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, capi.c_double_p,
                                         c_uint64_p, C.POINTER(C.c_int64), capi.c_double_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

def load_library(path=None):
    """Load liboctofitter_hip_draws.so (after the main library it links against). Raises if it has not been built."""
    return companion.load_library(path, DRAWS_LIB_PATH, "OCTOFITTER_HIP_DRAWS_LIB", _SIGS, needs_main=True,
                                  no_fallback="Prior draws on the device have no CPU fallback.")


def _u64ptr(a):
    return a.ctypes.data_as(c_uint64_p)


class PriorDraws(companion.Handle):
    """The handle of octo_draws_create. PriorDraws(model): for one LogDensityModel — its priors, its device model, its context.
    PriorDraws(priors=[…], device=0): a list of host/priors.py priors and a context of its own — sampling only (no best / rejection)."""

    PREFIX = "octo_draws"

    def __init__(self, model=None, priors=None, device=0):
        if (model is None) == (priors is None):
            raise ValueError("PriorDraws takes a LogDensityModel or a list of priors")
        self.model = model
        self._own_ctx = None
        self._open(load_library(), model.ln_like.device_index if model is not None else device)
        if model is not None:
            self.D = int(model.D)
            ctx, m, self._c_priors = model.ln_like._ctx, model._m, model._c_priors
        else:
            self.D = len(priors)
            self._c_priors = (capi.OctoPrior * max(self.D, 1))()
            for k, p in enumerate(priors):
                self._c_priors[k].kind = p.kind
                self._c_priors[k].p0, self._c_priors[k].p1, self._c_priors[k].lo, self._c_priors[k].hi = p.c_params()
            main = capi.load_library()
            ctx, m = C.c_void_p(), None
            st = main.octo_ctx_create(C.byref(ctx), self.device_index)
            if st != capi.OCTO_OK:
                raise capi.OctoError(st, "octo_ctx_create")
            self._own_ctx = ctx
        self._created(self.lib.octo_draws_create(ctx, m, self._c_priors, self.D, self.device_index, C.byref(self._h)))

    def sample(self, seed, first, n, theta=True, theta_t=True, logprior_t=True, stream=None):
        """Draws first … first + n − 1 of stream `seed` as torch float64 tensors on the model's device: (θ [D, n] natural domain,
        θ_t [D, n] linked, logprior_t [n]); None for an output switched off. Asynchronous on `stream` (default: torch's current stream)."""
        import torch
        dev = torch.device("cuda", self.device_index)
        n = int(n)
        th = torch.empty((self.D, n), dtype=torch.float64, device=dev) if theta else None
        tt = torch.empty((self.D, n), dtype=torch.float64, device=dev) if theta_t else None
        lp = torch.empty(n, dtype=torch.float64, device=dev) if logprior_t else None
        ptr = lambda x: None if x is None else x.data_ptr()      # noqa: E731
        self._check(self.lib.octo_draws_sample_device(self._h, int(seed), int(first), n, n, ptr(th), ptr(tt), ptr(lp), self._stream(stream, dev)))
        return th, tt, lp

    def best(self, seed, N, keep=1, first=0):
        """The `keep` highest log-posteriors among draws first … first + N − 1, best first (ties: lower draw index):
        (θ [D, keep] natural domain, logpost [keep], index [keep] uint64)."""
        keep = int(keep)
        th = np.empty((self.D, max(keep, 1)))
        lp = np.empty(max(keep, 1))
        ix = np.empty(max(keep, 1), dtype=np.uint64)
        self._check(self.lib.octo_draws_best(self._h, int(seed), int(first), int(N), keep, capi._dptr(th), capi._dptr(lp), _u64ptr(ix)))
        return th, lp, ix

    def rejection(self, seed, N, cap=None, first=0):
        """Rejection sampling with the prior as proposal over draws first … first + N − 1: the accepted draws in draw-index order,
        at most `cap` of them stored (default: all). dict(samples [D, n_stored], loglike, logpost, index, n_accepted, max_loglike)."""
        N = int(N)
        n_acc, mx = C.c_int64(0), C.c_double(0.0)
        room = min(N, max(65536, N // 16)) if cap is None else int(cap)
        while True:
            th = np.empty((self.D, max(room, 1)))      # the [D][cap] layout of the C call; only the accepted columns are ever touched
            ll, lp, ix = np.empty(max(room, 1)), np.empty(max(room, 1)), np.empty(max(room, 1), dtype=np.uint64)
            self._check(self.lib.octo_draws_rejection(self._h, int(seed), int(first), N, room, capi._dptr(th), capi._dptr(ll), capi._dptr(lp), _u64ptr(ix),
                                                      C.byref(n_acc), C.byref(mx)))
            if cap is not None or n_acc.value <= room:
                break
            room = int(n_acc.value)                    # more accepted than the first guess held: once more with room for all
        cap = room
        ns = min(int(n_acc.value), cap)
        return dict(samples=np.ascontiguousarray(th[:, :ns]), loglike=ll[:ns].copy(), logpost=lp[:ns].copy(), index=ix[:ns].copy(),
                    n_accepted=int(n_acc.value), max_loglike=float(mx.value))

    def close(self):
        if getattr(self, "_h", None) and self.model is not None and not getattr(self.model.ln_like, "_ctx", None):
            self.lib.octo_draws_detach(self._h)      # the model was closed first: its context is gone
        super().close()
        if getattr(self, "_own_ctx", None):
            capi.load_library().octo_ctx_destroy(self._own_ctx)
            self._own_ctx = None
