"""What the Table API handles' wrappers (over.py, timejoin.py) share: a native handle behind a C prefix ("fw_over",
"fw_tjoin") with the same create / last_error / rows_device / clear_pending / get_stats / destroy calls."""
import ctypes

from . import _native as N


class _TableHandle:
    _prefix = None  # the C functions' prefix
    _Rows = None    # ctypes struct of the pending rows' columns
    _Stats = None   # ctypes struct get_stats fills

    def _fn(self, name):
        return getattr(N.lib(), f"{self._prefix}_{name}")

    def _create(self, cfg):
        self._h = ctypes.c_void_p()
        rc = self._fn("create")(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != N.FW_OK:
            msg = self._fn("last_error")(self._h).decode() if self._h else "error"
            self._fn("destroy")(self._h)
            self._h = None
            raise N.NativeError(rc, msg)

    def _check(self, rc):
        if rc != N.FW_OK:
            raise N.NativeError(rc, self._fn("last_error")(self._h).decode())

    def _rows_device(self):
        rows, n = self._Rows(), ctypes.c_int64()
        self._check(self._fn("rows_device")(self._h, ctypes.byref(rows), ctypes.byref(n)))
        return rows, n.value

    def clear_pending(self):
        self._check(self._fn("clear_pending")(self._h))

    def stats(self):
        s = self._Stats()
        self._check(self._fn("get_stats")(self._h, ctypes.byref(s)))
        return {f: getattr(s, f) for f, _ in self._Stats._fields_}

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
