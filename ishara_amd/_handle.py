"""One library handle (`ishara_create`) with its parameter entries and the device buffers bound to it: what `model.Model` (the Keras
hybrid family) and `conformer._TorchFamilyEncoder` (the torch encoder families) share."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import IsharaError


class Handle:
    def _create_handle(self, cfg: _lib.Config):
        """Creates the handle and reads its parameter layout: `entries` = [(name, shape, offset, trainable)], `n_total`, `n_train`."""
        self._lib = _lib.load()
        self._cfg = cfg
        self._h = C.c_void_p()
        _lib.check(self._lib.ishara_create(C.byref(cfg), C.byref(self._h)), "ishara_create")
        self.max_batch = cfg.max_batch
        self.n_total = int(self._lib.ishara_param_total(self._h))
        self.n_train = int(self._lib.ishara_param_trainable(self._h))
        self.entries = []
        for i in range(self._lib.ishara_param_entries(self._h)):
            name, nd, sh, off, tr = C.c_char_p(), C.c_int32(), (C.c_int64 * 2)(), C.c_int64(), C.c_int32()
            _lib.check(self._lib.ishara_param_info(self._h, i, C.byref(name), C.byref(nd), C.byref(sh), C.byref(off), C.byref(tr)))
            shape = (int(sh[0]),) if nd.value == 1 else (int(sh[0]), int(sh[1]))
            self.entries.append((name.value.decode(), shape, int(off.value), bool(tr.value)))
        self.device = None

    def _bind_device(self, device):
        """Allocates the flat parameter / gradient / optimizer buffers and the workspace on `device` and binds them to the handle."""
        if not torch.cuda.is_available():
            raise IsharaError("ishara_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.device = dev = torch.device(device)
        torch.cuda.set_device(dev)
        self.params = torch.zeros(self.n_total, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(self.n_total, dtype=torch.float32, device=dev)
        self.opt_m = torch.zeros(self.n_train, dtype=torch.float32, device=dev)
        self.opt_v = torch.zeros(self.n_train, dtype=torch.float32, device=dev)
        self.opt_slow = torch.zeros(self.n_train, dtype=torch.float32, device=dev)
        wsb = int(self._lib.ishara_workspace_bytes(self._h))
        self.workspace, ws = _lib.aligned(wsb, dev)
        self._ws_ptr = ws.value
        _lib.check(self._lib.ishara_bind(self._h, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.opt_m), _lib.ptr(self.opt_v),
                                         _lib.ptr(self.opt_slow), ws, wsb), "ishara_bind")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.ishara_destroy(self._h)
                self._h = None
        except Exception:
            pass
