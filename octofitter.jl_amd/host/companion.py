"""
What the bindings of the companion libraries (draws.py, predict.py, pointwise.py, psis.py) share: the loader and the base class of their
handles. A companion module keeps its `_SIGS`, its `*_LIB_PATH`, a one-call `load_library(path=None)` and a handle class that derives
from Handle and holds only what is its own.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

from . import capi

_libs = {}      # env var -> the library loaded from its default place


def load_library(path, default, env, sigs, needs_main, no_fallback):
    """The companion library at `path`, else at $env, else at `default`, with the signatures of `sigs` bound. Cached only for path=None.
    needs_main: the main library it links against is loaded first. no_fallback: the sentence that ends the FileNotFoundError."""
    if path is None and env in _libs:
        return _libs[env]
    if needs_main:
        capi.load_library()
    p = Path(path or os.environ.get(env, default))
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: build the companion library first (python -c 'import __graft_entry__ as g; g.build()'). " + no_fallback)
    lib = C.CDLL(str(p), mode=C.RTLD_GLOBAL)
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _libs[env] = lib
    return lib


def is_torch(x):
    return type(x).__module__.startswith("torch")


class Handle:
    """A handle of octo_<PREFIX>_create. A subclass calls _open(), then its library's create with C.byref(self._h), then _created(status)."""

    PREFIX = None      # "octo_psis": the library's functions are octo_psis_last_error, _sync, _destroy

    def _open(self, lib, device):
        self.lib = lib
        self.device_index = int(device)
        self._h = C.c_void_p()
        self._keep = None      # the tensors of the last device call: alive until the next one

    def _fn(self, name):
        return getattr(self.lib, f"{self.PREFIX}_{name}")

    def _created(self, status):
        if status != capi.OCTO_OK:
            self._h = None
            self.close()
            raise capi.OctoError(status, (self._fn("last_error")(None) or b"").decode())

    def _check(self, status):
        if status != capi.OCTO_OK:
            raise capi.OctoError(status, (self._fn("last_error")(self._h) or b"").decode())

    @staticmethod
    def _stream(stream, device):
        """`stream`, or torch's current stream on `device`."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(device).cuda_stream
        return C.c_void_p(stream)

    def sync(self):
        self._check(self._fn("sync")(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None
        self._keep = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
